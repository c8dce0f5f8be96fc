"""Host-side mirror of the reference's public API for the predict path (vaporetto/src/lib.rs:82-91):
`Model`, `Predictor`, `Sentence`, `CharacterBoundary`, `CharacterType`, `VaporettoError`.

Same names, argument meaning and error behaviour as the Rust crate, over the C ABI of libvaporetto_hip.so.
All scoring happens in the HIP kernels; this module only parses text and moves buffers.
"""
from __future__ import annotations

import ctypes as C
import enum
import re
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, modelfmt


class VaporettoError(Exception):
    """errors.rs:15-38.  `kind` is "InvalidModel", "InvalidArgument" or "Runtime"."""

    def __init__(self, kind: str, message: str):
        super().__init__(message)
        self.kind = kind


def _raise(status: int):
    msg = _lib.last_error()
    kind = {_lib.VPT_INVALID_MODEL: "InvalidModel", _lib.VPT_INVALID_ARGUMENT: "InvalidArgument"}.get(status, "Runtime")
    raise VaporettoError(kind, msg)


class CharacterType(enum.IntEnum):  # sentence.rs:11-29
    Digit = 1
    Roman = 2
    Hiragana = 3
    Katakana = 4
    Kanji = 5
    Other = 6

    @staticmethod
    def get_type(c: str) -> "CharacterType":  # sentence.rs:50-67
        return CharacterType(int(_types_of(np.array([ord(c)], dtype=np.uint32))[0]))


class CharacterBoundary(enum.IntEnum):  # sentence.rs:70-82
    NotWordBoundary = 0
    WordBoundary = 1
    Unknown = 2


_RANGES = [  # (lo, hi, type) -- sentence.rs:52-65
    (0x30, 0x39, 1), (0xFF10, 0xFF19, 1),
    (0x41, 0x5A, 2), (0x61, 0x7A, 2), (0xFF21, 0xFF3A, 2), (0xFF41, 0xFF5A, 2),
    (0x3040, 0x3096, 3),
    (0x30A0, 0x30FA, 4), (0x30FC, 0x30FF, 4), (0xFF66, 0xFF9F, 4),
    (0x3400, 0x4DBF, 5), (0x4E00, 0x9FFF, 5), (0xF900, 0xFAFF, 5), (0x20000, 0x2A6DF, 5), (0x2A700, 0x2B73F, 5),
    (0x2B740, 0x2B81F, 5), (0x2B820, 0x2CEAF, 5), (0x2F800, 0x2FA1F, 5),
]


def _types_of(cps: np.ndarray) -> np.ndarray:
    out = np.full(cps.shape, 6, dtype=np.uint8)
    for lo, hi, t in _RANGES:
        out[(cps >= lo) & (cps <= hi)] = t
    return out


class KyteaFullwidthFilter:
    """vaporetto_rules/src/string_filters/kytea_fullwidth.rs:13-117 (host-side statement of the map the kernels apply
    when `fullwidth=True` is passed; useful to build the normalised text that tokens are NOT taken from)."""

    _PAIRS = None

    @classmethod
    def table(cls) -> dict:
        if cls._PAIRS is None:
            t = {}
            for i in range(26):
                t[ord("a") + i] = 0xFF41 + i
                t[ord("A") + i] = 0xFF21 + i
            for i in range(10):
                t[ord("0") + i] = 0xFF10 + i
            t.update({ord("("): 0xFF08, ord(")"): 0xFF09, ord("{"): 0xFF5B, ord("}"): 0xFF5D, ord("<"): 0xFF1C, ord(">"): 0xFF1E,
                      0xFF62: 0x300C, 0xFF63: 0x300D, ord("["): 0xFF3B, ord("]"): 0xFF3D, ord("-"): 0x2212, 0xFF5E: 0x301C,
                      ord("."): 0x3002, 0xFF0D: 0x30FC, ord("/"): 0xFF0F, ord("_"): 0xFF3F, ord(","): 0xFF0C, ord("%"): 0xFF05,
                      ord("?"): 0xFF1F, 0xFF64: 0x3001, 0x2015: 0x30FC, ord('"'): 0x201D, ord("'"): 0x2019, 0xFF65: 0x30FB,
                      0x2500: 0x30FC, ord("+"): 0xFF0B, ord(":"): 0xFF1A, 0x2013: 0x30FC, ord("!"): 0xFF01, 0xFF61: 0x3002,
                      ord("&"): 0xFF06, ord("*"): 0xFF0A, ord("@"): 0xFF20, ord("="): 0xFF1D})
            cls._PAIRS = t
        return cls._PAIRS

    def filter(self, string: str) -> str:
        return string.translate(self.table())


class ConcatGraphemeClustersFilter:
    """vaporetto_rules/src/sentence_filters/concat_grapheme_clusters.rs:10-36 (the CLI's `--wsconst G`, predict/src/main.rs:101-104): a
    sentence filter between predict and fill_tags -- every boundary inside an extended grapheme cluster (UAX #29) becomes
    NotWordBoundary, so a ZWJ sequence or a base + modifier is never cut.  THIS class is the host form (the oracle of the device filter's
    tests, and for callers that want another order); `wsconst=("G", ..)` everywhere in this module is VPT_FLAG_CONCAT_GRAPHEMES, the
    same filter as a launch on the device behind the scoring launch (Predictor.concat_graphemes_packed: on the caller's labels).  The reference segments with the `unicode-segmentation`
    crate (1.12.0); here the clusters come from the `regex` module's \\X, whichever Unicode version that module carries (the crate's and
    the module's rules agree on everything the reference's tests hold: concat_grapheme_clusters.rs:43-88).  It only CLEARS boundaries, so it
    commutes with KyteaWsConstFilter (which clears too) -- but not with SplitLinebreaksFilter, which SETS the boundary between "\r" and "\n"
    while CR LF is one cluster: the reference applies its filters in the caller's order (predict/src/main.rs:130-134);
    on the device "G" always runs LAST -- wsconst types, split_linebreaks, "G" (`Predictor.tokenize(wsconst=("G", ..),
    split_linebreaks=True)`), or with linebreaks_first split_linebreaks, wsconst types, "G" (the tantivy adapter's result for any place of
    "G" in its string) -- so "\r\n" stays joined.  A caller that wants the other order runs this filter (or concat_graphemes_packed) itself
    between `predict_packed(.., wsconst=.., split_linebreaks=False)` and its own SplitLinebreaksFilter pass."""

    _X = None

    @classmethod
    def cluster_lengths(cls, text: str) -> List[int]:
        """Chars of every extended grapheme cluster of `text`, in order."""
        if cls._X is None:
            try:
                import regex
            except ImportError as e:   # no silent "one char per cluster"
                raise ImportError("ConcatGraphemeClustersFilter needs the `regex` module (UAX #29 segmentation)") from e
            cls._X = regex.compile(r"\X")
        return [len(m.group()) for m in cls._X.finditer(text)]

    def filter(self, sentence: "Sentence") -> None:
        b = sentence.boundaries_mut()
        start = 0
        for n in self.cluster_lengths(sentence.as_raw_text()):
            b[start:start + n - 1] = CharacterBoundary.NotWordBoundary
            start += n

    def filter_packed(self, texts: Sequence[str], out_offsets: np.ndarray, labels: np.ndarray) -> None:
        """The same on a packed batch's labels (sentence i's boundaries are labels[out_offsets[i]:out_offsets[i + 1]]), in place."""
        for i, t in enumerate(texts):
            if t.isascii():      # a cluster of several ASCII chars is CR LF only
                if "\r\n" not in t:
                    continue
            start = int(out_offsets[i])
            for n in self.cluster_lengths(t):
                if n > 1:
                    labels[start:start + n - 1] = CharacterBoundary.NotWordBoundary
                start += n


class PatternMatchTagger:
    """vaporetto_rules/src/sentence_filters/pattern_match_tagger.rs:10-41: a table surface -> tags that fills the tag slots fill_tags left
    None.  `rules`: {surface: [tag or None, ...]} (or a sequence of such pairs: a repeated surface keeps the last, like HashMap::insert).
    `filter` is the host form, a plain restatement of the Rust (the oracle of the device form, and for callers who order their filters
    differently); the `tagger=` keyword of Predictor.fill_tags_batch / write_tokenized_batch / tokenize and DeviceBatch.set_pattern_tagger
    run it on the device behind fill_tags (vpt_pattern_tagger_*, kernels_pattern.hip)."""

    def __init__(self, rules):
        pairs = list(rules.items()) if hasattr(rules, "items") else list(rules)
        self._pairs = [(str(k), [None if t is None else str(t) for t in v]) for k, v in pairs]
        self.rules = dict(self._pairs)
        self._handles = {}   # id(predictor) -> (handle, predictor): the table lives on the predictor's device, with its n_tags

    def filter(self, sentence: "Sentence") -> None:  # pattern_match_tagger.rs:22-40
        n_tags = sentence.n_tags()
        queue = []
        for token in sentence.tokens():
            for j, tag in enumerate(token.tags()):
                if tag is None:
                    tags = self.rules.get(token.surface())
                    if tags is not None:
                        queue.append((token.end() - 1, j, tags[j] if j < len(tags) else None))
        for i, j, tag in queue:
            sentence._tags[i * n_tags + j] = tag

    def _packed(self):
        surf = [k.encode("utf-8", "surrogatepass") if isinstance(k, str) else bytes(k) for k, _ in self._pairs]
        utf8, off = pack_texts(surf) if surf else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        counts = np.array([len(v) for _, v in self._pairs], dtype=np.uint32)
        present, tags = [], []
        for _, v in self._pairs:
            for t in v:
                present.append(0 if t is None else 1)
                tags.append(b"" if t is None else t.encode("utf-8"))
        tb, toff = pack_texts(tags) if tags else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        return utf8, off, counts, np.array(present, dtype=np.uint8), tb, toff

    def handle(self, predictor: "Predictor"):
        """The device table for `predictor` (vpt_pattern_tagger_create), built on first use and kept."""
        got = self._handles.get(id(predictor))
        if got is not None:
            return got[0]
        utf8, off, counts, present, tb, toff = self._packed()
        h = C.c_void_p()
        keep = [a if len(a) else np.zeros(1, a.dtype) for a in (utf8, counts, present, tb)]
        st = _lib.load().vpt_pattern_tagger_create(predictor.handle, keep[0].ctypes.data, off.ctypes.data, len(self._pairs), keep[1].ctypes.data,
                                                   keep[2].ctypes.data, keep[3].ctypes.data, toff.ctypes.data, C.byref(h))
        if st != _lib.VPT_OK:
            _raise(st)
        self._handles[id(predictor)] = (h, predictor)
        return h

    def __del__(self):
        for h, _ in getattr(self, "_handles", {}).values():
            try:
                _lib.load().vpt_pattern_tagger_destroy(h)
            except Exception:
                pass
        self._handles = {}

    def n_tags(self, predictor: "Predictor") -> int:
        """vpt_pattern_tagger_n_tags: the distinct tag strings of the rules (the ids of the -(2 + id) encoding)."""
        v = C.c_uint32()
        st = _lib.load().vpt_pattern_tagger_n_tags(self.handle(predictor), C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value)

    def tag(self, predictor: "Predictor", tag_id: int) -> str:
        ptr, n = C.c_void_p(), C.c_size_t()
        st = _lib.load().vpt_pattern_tagger_tag(self.handle(predictor), int(tag_id), C.byref(ptr), C.byref(n))
        if st != _lib.VPT_OK:
            _raise(st)
        return C.string_at(ptr.value, n.value).decode("utf-8") if n.value else ""

    def max_tag_suffix(self, predictor: "Predictor") -> int:
        v = C.c_uint32()
        st = _lib.load().vpt_pattern_tagger_max_tag_suffix(self.handle(predictor), C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value)

    def info(self, predictor: "Predictor") -> dict:
        k, n, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = _lib.load().vpt_pattern_tagger_info(self.handle(predictor), C.byref(k), C.byref(n), C.byref(m))
        if st != _lib.VPT_OK:
            _raise(st)
        return {"n_keys": int(k.value), "n_slots": int(n.value), "max_surface_chars": int(m.value)}

    @staticmethod
    def tile() -> int:
        v = C.c_uint32()
        st = _lib.load().vpt_pattern_tagger_tile(C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value)


class Model:
    """model.rs:55-169."""

    def __init__(self, data: Optional[modelfmt.ModelData], raw: Optional[bytes] = None):
        self._data_ = data      # decoded records; None until somebody asks for them (a 34 MB model takes Python 20 s)
        self._raw = raw
        assert data is not None or raw is not None

    @property
    def _data(self) -> modelfmt.ModelData:
        if self._data_ is None:
            try:
                self._data_ = modelfmt.decode_model(self._raw)[0]
            except modelfmt.ModelFormatError as e:   # cannot happen after read_slice's validation; still the crate's error type
                raise VaporettoError("InvalidModel", "InvalidModelError: %s" % e)
        return self._data_

    @staticmethod
    def read(rdr) -> "Model":  # model.rs:138-153
        return Model.read_slice(rdr.read())[0]

    @staticmethod
    def read_slice(buf: bytes) -> Tuple["Model", bytes]:  # model.rs:127-135
        """The bytes are validated by the library's decoder (the same one vpt_predictor_create uses); the Python records
        behind dictionary() / tag_models() are decoded on first use."""
        buf = bytes(buf)
        try:
            L = _lib.load()
        except OSError:
            # Reading, inspecting or converting a model needs no GPU and no built library (model tooling on a host without
            # ROCm): the Python codec decodes -- and so validates -- the records right away instead.  COMPUTE never takes this
            # route: Predictor() loads the library and fails loudly without it.
            try:
                data, n_used = modelfmt.decode_model(buf)
            except modelfmt.ModelFormatError as e:
                raise VaporettoError("InvalidModel", "InvalidModelError: %s" % e)
            return Model(data, buf[:n_used]), buf[n_used:]
        used = C.c_size_t(0)
        st = L.vpt_model_read_len(buf, len(buf), C.byref(used))
        if st != _lib.VPT_OK:
            raise VaporettoError("InvalidModel" if st == _lib.VPT_INVALID_MODEL else "Runtime", L.vpt_last_error().decode("utf-8"))
        return Model(None, buf[:used.value]), buf[used.value:]

    def to_vec(self) -> bytes:  # model.rs:99-104
        if self._raw is None:
            self._raw = modelfmt.encode_model(self._data)
        return self._raw

    def write(self, wtr) -> None:  # model.rs:112-121
        wtr.write(self.to_vec())

    def dictionary(self):  # model.rs:155-158
        return self._data.dict_model

    def replace_dictionary(self, dict_records) -> None:  # model.rs:160-163
        self._data.dict_model = list(dict_records)
        self._raw = None

    def tag_models(self):  # model.rs:165-168
        return self._data.tag_models


class Token:
    """sentence.rs:1195-1263: a token of a Sentence, chars [start, end)."""

    def __init__(self, sentence: "Sentence", start: int, end: int):
        self._s, self._start, self._end = sentence, start, end

    def surface(self) -> str:
        return self._s._text[self._start:self._end]

    def tags(self) -> List[Optional[str]]:  # sentence.rs:1210-1214
        nt = self._s._n_tags
        return list(self._s._tags[(self._end - 1) * nt:self._end * nt])

    def tag_candidates(self) -> List[List[Tuple[str, int]]]:  # sentence.rs:1216-1250
        """Per tag slot the candidates with their scores (score 0 for the only candidate of a slot).  Like the reference this
        requires Predictor.store_tag_scores(True) before fill_tags."""
        if not self._s._tag_scores:
            raise AssertionError("Predictor::store_tag_scores() must be set to true to use this function.")
        entry = self._s._tag_scores[self._end - 1]
        results = []
        if entry is not None:
            tags, scores = entry
            i = 0
            for cands in tags:
                if len(cands) == 1:
                    results.append([(cands[0], 0)])
                else:
                    results.append([(c, scores[i + k]) for k, c in enumerate(cands)])
                    i += len(cands)
        return results

    def start(self) -> int:
        return self._start

    def end(self) -> int:
        return self._end


class Sentence:
    """sentence.rs:85-101 (raw-text path).  Holds the text, its character types, and after `predict`
    the boundary scores and labels."""

    def __init__(self):
        self._set_default()

    def _set_default(self):  # sentence.rs:140-158: a single space
        self._text = " "
        self._utf8 = b" "
        self._char_types = np.array([6], dtype=np.uint8)
        self._boundaries = np.zeros(0, dtype=np.uint8)
        self._scores = np.zeros(0, dtype=np.int32)
        self._has_scores = False
        self._predictor = None
        self._tags = []
        self._n_tags = 0
        self._tag_scores = []

    @staticmethod
    def default() -> "Sentence":
        return Sentence()

    def _parse_raw(self, text: str):  # sentence.rs:160-196
        if "\0" in text:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: text: must not contain NULL")
        if len(text) == 0:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: text: must contain at least one character")
        cps = np.frombuffer(text.encode("utf-32-le"), dtype=np.uint32)
        self._text = text
        self._utf8 = text.encode("utf-8")
        self._char_types = _types_of(cps)
        self._boundaries = np.full(len(cps) - 1, CharacterBoundary.Unknown, dtype=np.uint8)
        self._scores = np.zeros(0, dtype=np.int32)
        self._has_scores = False
        self._predictor = None
        self._tags = []
        self._n_tags = 0
        self._tag_scores = []

    @staticmethod
    def from_raw(text: str) -> "Sentence":  # sentence.rs:217-245
        s = Sentence()
        s._parse_raw(text)
        return s

    def update_raw(self, text: str) -> None:  # sentence.rs:264-283: on error the sentence becomes " "
        try:
            self._parse_raw(text)
        except VaporettoError:
            self._set_default()
            raise

    def _parse_tokenized(self, text: str):  # sentence.rs:285-400, through the library's host parser (vpt_parse_tokenized_batch)
        try:
            p = parse_tokenized_host([text.encode("utf-8")])
        except VaporettoError as e:   # one sentence: the reference's message, without the batch's line number
            raise VaporettoError(e.kind, str(e).replace(" (line 0)", "")) from None
        raw = bytes(p["raw"]).decode("utf-8")
        nt = int(p["n_tags"][0])
        ti, so, tb = p["tag_index"], p["span_offsets"], bytes(p["tag_bytes"])
        tags: List[Optional[str]] = []
        for c in range(len(ti) - 1):
            own = [tb[int(so[k]):int(so[k + 1])].decode("utf-8") for k in range(int(ti[c]), int(ti[c + 1]))]
            own += [""] * (nt - len(own))
            tags += [t if t else None for t in own]
        self._parse_raw(raw)
        self._boundaries = p["labels"].copy()
        self._tags = tags
        self._n_tags = nt

    @staticmethod
    def from_tokenized(text: str) -> "Sentence":  # sentence.rs:402-459
        s = Sentence()
        s._parse_tokenized(text)
        return s

    def update_tokenized(self, text: str) -> None:  # sentence.rs:482-514: on error the sentence becomes " "
        try:
            self._parse_tokenized(text)
        except VaporettoError:
            self._set_default()
            raise

    @staticmethod
    def from_partial_annotation(text: str) -> "Sentence":
        """sentence.rs:516-769, restated on the host (training input only): chars alternate with boundary marks '|' WordBoundary,
        '-' NotWordBoundary, ' ' Unknown; '/' starts a tag of the char in front of it, '\\' escapes the next char of a tag."""
        def err(msg):
            return VaporettoError("InvalidArgument", "InvalidArgumentError: partial_annotation_text: " + msg)
        if not text:
            raise err("must contain at least one character")
        chars, bounds, tags_tmp = [], [], []
        tag, escape, is_char = None, False, True
        for c in text:
            if is_char:
                if c == "\0":
                    raise err("must not contain NULL")
                chars.append(c)
                tags_tmp.append([])
                is_char = False
                continue
            if not escape and c == "\\":
                escape = True
            elif not escape and c in " -|":
                if tag is not None:
                    tags_tmp[-1].append(tag)
                    tag = None
                bounds.append({" ": CharacterBoundary.Unknown, "-": CharacterBoundary.NotWordBoundary, "|": CharacterBoundary.WordBoundary}[c])
                is_char = True
            elif not escape and c == "/":
                if tag is not None:
                    tags_tmp[-1].append(tag)
                tag = ""
            else:
                escape = False
                if tag is None:
                    raise err("contains an invalid boundary character: '%s'" % c)
                tag += c
        if is_char:
            raise err("invalid annotation")
        if tag is not None:
            tags_tmp[-1].append(tag)
        n_tags = max(len(t) for t in tags_tmp)
        s = Sentence()
        s._parse_raw("".join(chars))
        s._boundaries = np.array(bounds, dtype=np.uint8)
        s._tags = [(t if t else None) for ts in tags_tmp for t in ts + [""] * (n_tags - len(ts))]
        s._n_tags = n_tags
        return s

    def as_raw_text(self) -> str:  # sentence.rs:782
        return self._text

    def __len__(self) -> int:
        return len(self._char_types)

    def char_types(self) -> np.ndarray:  # sentence.rs:1034
        return self._char_types

    def boundaries(self) -> np.ndarray:  # sentence.rs:993
        return self._boundaries

    def boundaries_mut(self) -> np.ndarray:  # sentence.rs:1016
        return self._boundaries

    def boundary_scores(self) -> np.ndarray:  # sentence.rs:1040-1046
        return self._scores if self._has_scores else np.zeros(0, dtype=np.int32)

    def char_to_str_pos(self) -> List[int]:
        pos, out = 0, [0]
        for ch in self._text:
            pos += len(ch.encode("utf-8"))
            out.append(pos)
        return out

    def n_tags(self) -> int:  # sentence.rs:1161
        return self._n_tags

    def tags(self) -> List[Optional[str]]:  # sentence.rs:1068: len() * n_tags entries, set on a token's LAST char
        return self._tags

    def fill_tags(self) -> None:
        """sentence.rs:1144-1148: tags for the current boundaries, with the predictor that last predicted this
        sentence (which must have been created with predict_tags = True, predictor.rs:548-551)."""
        if self._predictor is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: sentence: predict() has not been called")
        self._predictor.fill_tags_batch([self])

    def _token_ranges(self):
        """(start, end) char ranges of the tokens; tokens adjacent to an Unknown boundary are skipped
        (TokenIterator, sentence.rs:1265-1309)."""
        n = len(self)
        start, valid = 0, True
        for e in range(n):
            b = CharacterBoundary.WordBoundary if e == n - 1 else int(self._boundaries[e])
            if b == CharacterBoundary.Unknown:
                valid = False
            elif b == CharacterBoundary.WordBoundary:
                if valid:
                    yield start, e
                start, valid = e + 1, True

    def iter_tokens(self) -> Iterable[str]:  # sentence.rs:819 (surfaces only)
        for a, e in self._token_ranges():
            yield self._text[a:e + 1]

    def tokens(self) -> List["Token"]:  # sentence.rs:819: the Token objects of iter_tokens (surface, tags, tag_candidates, start, end)
        return [Token(self, a, e + 1) for a, e in self._token_ranges()]

    def write_tokenized_text(self) -> str:  # sentence.rs:850-886
        def esc(tok):
            return "".join("\\" + c if c in " \\/" else c for c in tok)
        out = []
        for a, e in self._token_ranges():
            parts = [esc(self._text[a:e + 1])]
            if self._n_tags:
                row = list(self._tags[e * self._n_tags:(e + 1) * self._n_tags])
                while row and row[-1] is None:   # up to the last Some (sentence.rs:868)
                    row.pop()
                parts += [esc(t) if t is not None else "" for t in row]
            out.append("/".join(parts))
        return " ".join(out)

    def write_partial_annotation_text(self) -> str:  # sentence.rs:907-944: tags are written as they are, not escaped
        marks = {int(CharacterBoundary.NotWordBoundary): "-", int(CharacterBoundary.WordBoundary): "|", int(CharacterBoundary.Unknown): " "}
        out = []
        for c, ch in enumerate(self._text):
            if c:
                out.append(marks[int(self._boundaries[c - 1])])
            out.append(ch)
            if self._n_tags:
                row = list(self._tags[c * self._n_tags:(c + 1) * self._n_tags])
                while row and row[-1] is None:   # up to the last Some (sentence.rs:914, 927)
                    row.pop()
                out += ["/" + (t if t is not None else "") for t in row]
        return "".join(out)


class Predictor:
    """predictor.rs:433-665 (boundary prediction)."""

    def __init__(self, model: Model, predict_tags: bool = False, device: int = 0):  # Predictor::new, predictor.rs:450
        raw = model.to_vec()
        self._model = model
        self._predict_tags = bool(predict_tags)
        self._tag_models = None
        self._store_tag_scores = False
        self._h = C.c_void_p()
        st = _lib.load().vpt_predictor_create(raw, len(raw), int(predict_tags), device, C.byref(self._h))
        if st != _lib.VPT_OK:
            self._h = None
            _raise(st)
        self.device = device

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().vpt_predictor_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @classmethod
    def _adopt(cls, handle, model: Optional[Model], device: int) -> "Predictor":
        self = cls.__new__(cls)
        self._h = handle
        self._model = model
        self._tag_models = None
        self._store_tag_scores = False
        self.device = device
        self._predict_tags = bool(self.info()["predict_tags"])
        return self

    def store_tag_scores(self, flag: bool) -> None:  # predictor.rs:510-514
        """Stores tag scores if `flag` is true: fill_tags then keeps every token's score vector for Token.tag_candidates."""
        self._store_tag_scores = bool(flag)

    def tag_score_stride(self) -> int:
        """vpt_predictor_tag_score_stride: the longest score vector (TagPredictor bias) over the tag models."""
        v = C.c_uint32()
        st = _lib.load().vpt_predictor_tag_score_stride(self._h, C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return v.value

    def fill_tags_scores_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, out_offsets: np.ndarray, labels: np.ndarray,
                                fullwidth: bool = False):
        """fill_tags_packed plus what Predictor::store_tag_scores(true) keeps (predictor.rs:599-601): returns (tags, scores, models)
        -- tags int32 [chars, n_tags]; scores int32 [chars, stride]: at a token's last char its score vector in entries
        [0, bias.len()), zeros elsewhere; models int32 [chars]: index into Model.tag_models() of the token's tag model or -1."""
        L = _lib.load()
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        S = len(byte_offsets) - 1
        nt = self.n_tags() if self._predict_tags else 0
        stride = self.tag_score_stride() if self._predict_tags else 0
        total_c = int(out_offsets[S]) + S
        tags = np.full((total_c, max(nt, 1)), -1, dtype=np.int32)
        scores = np.zeros((total_c, max(stride, 1)), dtype=np.int32)
        models = np.full(total_c, -1, dtype=np.int32)
        lab = labels if len(labels) else np.zeros(1, dtype=np.uint8)
        st = L.vpt_fill_tags_scores_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, out_offsets.ctypes.data, lab.ctypes.data,
                                          _lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0, tags.ctypes.data, scores.ctypes.data, models.ctypes.data)
        if st != _lib.VPT_OK:
            _raise(st)
        return tags[:, :nt], scores[:, :stride], models

    def save_compiled(self) -> bytes:
        """Predictor::serialize_to_vec (predictor.rs:640-651), in this library's own format: the device tables + a header."""
        L = _lib.load()
        need = C.c_size_t(0)
        st = L.vpt_predictor_save(self._h, None, 0, C.byref(need))
        if st != _lib.VPT_OK:
            _raise(st)
        buf = np.empty(need.value, dtype=np.uint8)
        st = L.vpt_predictor_save(self._h, buf.ctypes.data, buf.nbytes, C.byref(need))
        if st != _lib.VPT_OK:
            _raise(st)
        return buf.tobytes()

    @classmethod
    def load_compiled(cls, blob, device: int = 0, model: Optional[Model] = None) -> "Predictor":
        """Predictor::deserialize_from_slice_unchecked (predictor.rs:653-664).  `model` is only needed to turn tag indices
        into tag strings (Sentence.tags); scoring does not use it."""
        arr = np.frombuffer(blob, dtype=np.uint8)
        h = C.c_void_p()
        st = _lib.load().vpt_predictor_load(arr.ctypes.data, arr.nbytes, device, C.byref(h))
        if st != _lib.VPT_OK:
            _raise(st)
        return cls._adopt(h, model, device)

    def clone_to_device(self, device: int) -> "Predictor":
        """The same predictor on another GPU of the node: the compiled tables go device to device (xGMI), nothing is
        compiled again."""
        h = C.c_void_p()
        st = _lib.load().vpt_predictor_clone_to_device(self._h, device, C.byref(h))
        if st != _lib.VPT_OK:
            _raise(st)
        return Predictor._adopt(h, self._model, device)

    def info(self) -> dict:
        mi = _lib.ModelInfo()
        st = _lib.load().vpt_predictor_info(self._h, C.byref(mi))
        if st != _lib.VPT_OK:
            _raise(st)
        return mi.as_dict()

    def max_tag_suffix(self) -> int:
        """vpt_predictor_max_tag_suffix: the most bytes "/tag/tag.." can add per char (sizes write_tagged's output)."""
        sfx = C.c_uint32(0)
        st = _lib.load().vpt_predictor_max_tag_suffix(self._h, C.byref(sfx))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(sfx.value)

    def predict(self, sentence: Sentence) -> None:  # predictor.rs:518-543
        """One sentence through vpt_predict_one: two kernel launches and a synchronisation, tens of microseconds for work the
        reference does in one -- it exists for API parity and tests.  Anything with more than a handful of sentences belongs in
        predict_batch / predict_packed (one launch for all of them); a loop over this method is the slowest way to use the library."""
        n = len(sentence)
        scores = np.zeros(max(n - 1, 1), dtype=np.int32)
        labels = np.zeros(max(n - 1, 1), dtype=np.uint8)
        nb = C.c_size_t()
        raw = sentence._utf8
        st = _lib.load().vpt_predict_one(self._h, raw, len(raw), scores.ctypes.data, labels.ctypes.data, C.byref(nb))
        if st != _lib.VPT_OK:
            _raise(st)
        sentence._scores = scores[:nb.value]
        sentence._boundaries = labels[:nb.value]
        sentence._has_scores = True
        sentence._predictor = self   # predictor.rs:542: enables a later fill_tags

    def predict_batch(self, sentences: Sequence[Sentence], fullwidth: bool = False) -> None:
        """Predictor::predict for many sentences in one launch."""
        if not sentences:
            return
        utf8, boff = pack_texts([s._utf8 for s in sentences])
        scores, labels, ooff = self.predict_packed(utf8, boff, fullwidth=fullwidth)
        for i, s in enumerate(sentences):
            a, b = int(ooff[i]), int(ooff[i + 1])
            s._scores = scores[a:b]
            s._boundaries = labels[a:b]
            s._has_scores = True
            s._predictor = self

    def n_tags(self) -> int:
        v = C.c_uint32()
        st = _lib.load().vpt_predictor_n_tags(self._h, C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return v.value

    def tag_strings(self) -> List[str]:
        """The predictor's tag vocabulary (vpt_predictor_n_tag_strings / vpt_predictor_tag_string): the distinct raw tag strings of its tag
        models in order of first appearance over tag models, slots, candidates -- what the ids >= 0 of DeviceBatch.token_tags name.  Empty
        without predict_tags or without tag models."""
        L = _lib.load()
        n = C.c_uint32()
        st = L.vpt_predictor_n_tag_strings(self._h, C.byref(n))
        if st != _lib.VPT_OK:
            _raise(st)
        out = []
        for k in range(n.value):
            ptr, ln = C.c_void_p(), C.c_size_t()
            st = L.vpt_predictor_tag_string(self._h, k, C.byref(ptr), C.byref(ln))
            if st != _lib.VPT_OK:
                _raise(st)
            out.append(C.string_at(ptr.value, ln.value).decode("utf-8") if ln.value else "")
        return out

    def token_stream_tagged_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, wsconst: str = "", tagger: Optional["PatternMatchTagger"] = None,
                                   stop: Optional["TagStopFilter"] = None):
        """vpt_token_stream_tagged_batch: token_stream_packed with every token's tags and, with `stop`, without the stopped tokens ->
        (token_offsets uint64 [n + 1], token_starts, token_ends, token_positions uint32, token_tags int32 [tokens, n_tags]): a token's
        offset_from / offset_to, its index in its document BEFORE filtering, and per slot an id of tag_strings(), -1 (None) or
        -(2 + id) (a rule tag of `tagger`)."""
        flags = wsconst_flags(wsconst, allow_graphemes=True)
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        S, nt = len(byte_offsets) - 1, self.n_tags() if self._predict_tags else 0
        cap = max(int(byte_offsets[-1] - byte_offsets[0]), 1) if S else 1
        toff = np.zeros(S + 1, np.uint64)
        starts, ends, pos = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        tags = np.zeros(cap * max(nt, 1), np.int32)
        src = utf8 if len(utf8) else np.zeros(1, np.uint8)
        st = _lib.load().vpt_token_stream_tagged_batch(self._h, src.ctypes.data, byte_offsets.ctypes.data, S, flags,
                                                       tagger.handle(self) if tagger is not None else None,
                                                       stop.handle if stop is not None else None, toff.ctypes.data, starts.ctypes.data,
                                                       ends.ctypes.data, pos.ctypes.data, tags.ctypes.data, cap)
        if st != _lib.VPT_OK:
            _raise(st)
        n = int(toff[S])
        return toff, starts[:n].copy(), ends[:n].copy(), pos[:n].copy(), tags[:n * nt].reshape(n, nt).copy()

    def token_ids_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, vocab: "Vocabulary", wsconst: str = "", normalize: bool = True,
                         tagger: Optional["PatternMatchTagger"] = None, stop: Optional["TagStopFilter"] = None, tags: bool = False):
        """vpt_token_stream_ids_batch: the token stream with every token's id in `vocab` -> (token_offsets uint64 [n + 1], token_starts,
        token_ends, token_positions uint32, token_tags int32 [tokens, n_tags] or None, token_ids int32).  normalize: the surface looked up is
        the KyteaFullwidthFilter image of the token (the text as it was scored), else the caller's bytes.  Without tagger, stop and tags the
        untagged stream's steps run (no predict_tags needed) and token_tags is None."""
        flags = wsconst_flags(wsconst, allow_graphemes=True)
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        tagged = bool(tags) or tagger is not None or stop is not None
        S, nt = len(byte_offsets) - 1, self.n_tags() if (tagged and self._predict_tags) else 0
        cap = max(int(byte_offsets[-1] - byte_offsets[0]), 1) if S else 1
        toff = np.zeros(S + 1, np.uint64)
        starts, ends, pos = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        tag_arr = np.zeros(cap * max(nt, 1), np.int32) if tagged else None
        ids = np.zeros(cap, np.int32)
        src = utf8 if len(utf8) else np.zeros(1, np.uint8)
        st = _lib.load().vpt_token_stream_ids_batch(self._h, src.ctypes.data, byte_offsets.ctypes.data, S, flags,
                                                    tagger.handle(self) if tagger is not None else None, stop.handle if stop is not None else None,
                                                    vocab.handle if vocab is not None else None, _lib.VPT_FLAG_KYTEA_FULLWIDTH if normalize else 0,
                                                    toff.ctypes.data, starts.ctypes.data, ends.ctypes.data, pos.ctypes.data,
                                                    tag_arr.ctypes.data if tagged else None, ids.ctypes.data, cap)
        if st != _lib.VPT_OK:
            _raise(st)
        n = int(toff[S])
        return (toff, starts[:n].copy(), ends[:n].copy(), pos[:n].copy(), tag_arr[:n * nt].reshape(n, nt).copy() if tagged else None,
                ids[:n].copy())

    def count_tokens_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, counter: "VocabularyCounter", wsconst: str = "", normalize: bool = True,
                            tagger: Optional["PatternMatchTagger"] = None, stop: Optional["TagStopFilter"] = None) -> None:
        """vpt_token_stream_count_batch: every token of the stream into `counter`, on the device; nothing comes back.  normalize: the surface
        counted is the KyteaFullwidthFilter image of the token (the text as it was scored), else the caller's bytes.  Without tagger and stop
        the untagged stream's steps run (no predict_tags needed)."""
        flags = wsconst_flags(wsconst, allow_graphemes=True)
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        src = utf8 if len(utf8) else np.zeros(1, np.uint8)
        st = _lib.load().vpt_token_stream_count_batch(self._h, src.ctypes.data, byte_offsets.ctypes.data, len(byte_offsets) - 1, flags,
                                                      tagger.handle(self) if tagger is not None else None, stop.handle if stop is not None else None,
                                                      counter.handle if counter is not None else None, _lib.VPT_FLAG_KYTEA_FULLWIDTH if normalize else 0)
        if st != _lib.VPT_OK:
            _raise(st)

    def postings_packed(self, token_offsets: np.ndarray, token_ids: np.ndarray, n_terms: int, doc_base: int = 0, positions: bool = False,
                        token_positions: Optional[np.ndarray] = None) -> "Postings":
        """vpt_postings_batch_device over host arrays: token_offsets uint64 [n + 1] and token_ids int32 (what token_ids_packed / encode_batch
        return) go to the device, the pass runs once, the segment's Postings come back.  positions: with `first` and `order` (the tokens of
        every posting) and `positions` (vpt_postings_positions_device: every posting's position list; token_positions uint32 per token, what
        the stream calls return, default the token's index inside its document)."""
        import torch
        toff = np.ascontiguousarray(token_offsets, dtype=np.uint64)
        ids = np.ascontiguousarray(token_ids, dtype=np.int32)
        n_docs, n_tok, n_terms = len(toff) - 1, len(ids), int(n_terms)
        if not 0 <= n_terms <= 1 << 24:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: n_terms: must be between 1 and 2^24")
        dev = torch.device("cuda", self.device)

        def d(n, dt):
            return torch.zeros(max(n, 1), dtype=dt, device=dev)
        d_toff = torch.from_numpy(toff.view(np.int64)).to(dev)
        d_ids = torch.from_numpy(ids if n_tok else np.zeros(1, np.int32)).to(dev)
        d_term, d_docs, d_tfs, d_cnt = d(n_terms + 1, torch.int64), d(n_tok, torch.int32), d(n_tok, torch.int32), d(2, torch.int64)
        d_first, d_order = (d(n_tok + 1, torch.int64), d(n_tok, torch.int32)) if positions else (None, None)
        batch = DeviceBatch(self)
        batch.postings(d_toff.data_ptr(), n_docs, d_ids.data_ptr(), n_tok, n_terms, doc_base, d_term.data_ptr(), d_docs.data_ptr(), d_tfs.data_ptr(), n_tok,
                       d_first.data_ptr() if positions else 0, d_order.data_ptr() if positions else 0, d_cnt.data_ptr(),
                       torch.cuda.current_stream(dev).cuda_stream)
        d_ppos = None
        if positions:
            d_ppos = d(n_tok, torch.int32)
            d_tpos = None
            if token_positions is not None:
                tpos = np.ascontiguousarray(token_positions, dtype=np.uint32)
                if len(tpos) != n_tok:
                    raise VaporettoError("InvalidArgument", "InvalidArgumentError: token_positions: one per token")
                d_tpos = torch.from_numpy((tpos if n_tok else np.zeros(1, np.uint32)).view(np.int32)).to(dev)
            batch.postings_positions(d_toff.data_ptr(), n_docs, n_tok, d_tpos.data_ptr() if d_tpos is not None else 0, d_term.data_ptr(), n_terms,
                                     d_first.data_ptr(), n_tok, d_order.data_ptr(), d_ppos.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        batch.sync()
        cnt = d_cnt.cpu().numpy().view(np.uint64)
        n_post = int(cnt[0])
        first = d_first.cpu().numpy().view(np.uint64)[:n_post + 1].copy() if positions else None
        out = Postings(d_term.cpu().numpy().view(np.uint64)[:n_terms + 1].copy(), d_docs.cpu().numpy().view(np.uint32)[:n_post].copy(),
                       d_tfs.cpu().numpy().view(np.uint32)[:n_post].copy(), first,
                       d_order.cpu().numpy().view(np.uint32)[:int(first[n_post])].copy() if positions else None, int(cnt[1]))
        if positions:
            out.positions = d_ppos.cpu().numpy().view(np.uint32)[:int(first[n_post])].copy()
        return out

    def token_postings_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, vocab: "Vocabulary", wsconst: str = "", normalize: bool = True,
                              tagger: Optional["PatternMatchTagger"] = None, stop: Optional["TagStopFilter"] = None, doc_base: int = 0,
                              capacity: Optional[int] = None, positions: bool = False) -> "Postings":
        """vpt_token_stream_postings_batch: documents in, the segment's Postings out (no `first` / `order`); n_terms is the vocabulary's key
        count.  capacity: what the posting arrays hold (default: the text's bytes, which always suffices).  positions:
        vpt_token_stream_positional_postings_batch -- with `first` and `positions`, every posting's position list from the stream's
        token positions (no `order`: the token indices stay in the call)."""
        flags = wsconst_flags(wsconst, allow_graphemes=True)
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        S = len(byte_offsets) - 1
        cap = (max(int(byte_offsets[-1] - byte_offsets[0]), 1) if S else 1) if capacity is None else int(capacity)
        n_terms = vocab.info()["n_keys"] if vocab is not None else 0
        term = np.zeros(n_terms + 1, np.uint64)
        docs, tfs = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        n_post, n_drop = C.c_uint64(), C.c_uint64()
        src = utf8 if len(utf8) else np.zeros(1, np.uint8)
        if positions:
            cap_pos = max(int(byte_offsets[-1] - byte_offsets[0]), 1) if S else 1
            first, ppos, n_pos = np.zeros(max(cap, 1) + 1, np.uint64), np.zeros(cap_pos, np.uint32), C.c_uint64()
            st = _lib.load().vpt_token_stream_positional_postings_batch(
                self._h, src.ctypes.data, byte_offsets.ctypes.data, S, flags, tagger.handle(self) if tagger is not None else None,
                stop.handle if stop is not None else None, vocab.handle if vocab is not None else None,
                _lib.VPT_FLAG_KYTEA_FULLWIDTH if normalize else 0, int(doc_base), term.ctypes.data, docs.ctypes.data, tfs.ctypes.data,
                first.ctypes.data, cap, ppos.ctypes.data, cap_pos, C.byref(n_post), C.byref(n_drop), C.byref(n_pos))
        else:
            st = _lib.load().vpt_token_stream_postings_batch(self._h, src.ctypes.data, byte_offsets.ctypes.data, S, flags,
                                                             tagger.handle(self) if tagger is not None else None, stop.handle if stop is not None else None,
                                                             vocab.handle if vocab is not None else None, _lib.VPT_FLAG_KYTEA_FULLWIDTH if normalize else 0,
                                                             int(doc_base), term.ctypes.data, docs.ctypes.data, tfs.ctypes.data, cap, C.byref(n_post), C.byref(n_drop))
        if st != _lib.VPT_OK:
            try:
                _raise(st)
            except VaporettoError as e:
                e.n_postings = int(n_post.value)   # (too small a capacity: the number needed)
                raise
        n = int(n_post.value)
        out = Postings(term, docs[:n].copy(), tfs[:n].copy(), first[:n + 1].copy() if positions else None, None, int(n_drop.value))
        if positions:
            out.positions = ppos[:int(n_pos.value)].copy()
        out._predictor = self
        return out

    def fill_tags_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, out_offsets: np.ndarray, labels: np.ndarray,
                         fullwidth: bool = False, tagger: Optional["PatternMatchTagger"] = None) -> np.ndarray:
        """Predictor::predict_tags over a packed batch (predictor.rs:546-637).  labels: uint8 per boundary (0/1/2).
        Returns int32 [total chars, n_tags]: candidate index per slot, -1 = None; with `tagger` its rules run behind fill_tags on the
        device and a rule tag is -(2 + id) (PatternMatchTagger.tag)."""
        L = _lib.load()
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        S = len(byte_offsets) - 1
        nt = self.n_tags() if self._predict_tags else 0
        total_c = int(out_offsets[S]) + S
        tags = np.full((total_c, max(nt, 1)), -1, dtype=np.int32)
        lab = labels if len(labels) else np.zeros(1, dtype=np.uint8)
        if tagger is not None:
            st = L.vpt_fill_tags_batch_rules(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, out_offsets.ctypes.data, lab.ctypes.data,
                                             tags.ctypes.data, _lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0, tagger.handle(self))
        else:
            st = L.vpt_fill_tags_batch_flags(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, out_offsets.ctypes.data,
                                             lab.ctypes.data, tags.ctypes.data, _lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0)
        if st != _lib.VPT_OK:
            _raise(st)
        return tags[:, :nt]

    def max_tag_listing(self) -> int:
        """vpt_predictor_max_tag_listing: the most bytes the candidates of one token take in the tag block of a listing."""
        v = C.c_uint32(0)
        st = _lib.load().vpt_predictor_max_tag_listing(self._h, C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value)

    def listing_capacity(self, text_bytes: int, n_chars: int, n_lines: int, listing: int) -> int:
        """The capacity bound include/vaporetto_hip.h documents for vpt_predict_listing_batch."""
        cap = 3 * text_bytes + n_lines
        if listing & _lib.VPT_LISTING_TAGGED:
            cap += n_chars * self.max_tag_suffix()
        if listing & _lib.VPT_LISTING_SCORES:
            cap += 32 * (n_chars - n_lines) + n_lines
        if listing & _lib.VPT_LISTING_TAG_SCORES:
            cap += 3 * text_bytes + n_chars + n_lines + n_chars * self.max_tag_listing()
        return cap

    def predict_listing_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, listing: int, flags: int = 0,
                               scores: Optional[np.ndarray] = None, labels: Optional[np.ndarray] = None, capacity: Optional[int] = None):
        """vpt_predict_listing_batch over a packed batch: (uint8 bytes, uint64 [S+1] offsets) -- what the `predict` CLI writes for these lines
        with --scores / --tag-scores (predict/src/main.rs:66-93, 122-176), formatted on the device.  `listing`: VPT_LISTING_* bits; `labels`
        (and `scores`): list these instead of predicting (a host filter ran between predict and the listing)."""
        L = _lib.load()
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        S = len(byte_offsets) - 1
        if capacity is None:
            n_chars = int(np.count_nonzero((utf8 & 0xC0) != 0x80))
            capacity = self.listing_capacity(len(utf8), n_chars, S, listing)
        out = np.zeros(max(capacity, 1), dtype=np.uint8)
        offs = np.zeros(S + 1, dtype=np.uint64)
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.uint8)
            if len(labels) == 0:
                labels = np.zeros(1, dtype=np.uint8)
            if scores is not None:
                scores = np.ascontiguousarray(scores, dtype=np.int32)
        st = L.vpt_predict_listing_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, int(flags), int(listing),
                                         scores.ctypes.data if (labels is not None and scores is not None and len(scores)) else None,
                                         labels.ctypes.data if labels is not None else None, out.ctypes.data, capacity, offs.ctypes.data)
        if st != _lib.VPT_OK:
            _raise(st)
        return out[:int(offs[S])], offs

    def predict_listing(self, texts: Sequence[str], scores: bool = False, tag_scores: bool = False, tagged: bool = False, fullwidth: bool = True,
                        wsconst: Sequence = (), no_norm_order: bool = False, split_linebreaks: bool = False) -> List[bytes]:
        """predict_listing_arena cut into one bytes object per line (a convenience for callers that want the lines apart; the CLI writes
        the arena as it is)."""
        if not texts:
            return []
        out, offs = self.predict_listing_arena(texts, scores=scores, tag_scores=tag_scores, tagged=tagged, fullwidth=fullwidth, wsconst=wsconst,
                                               no_norm_order=no_norm_order, split_linebreaks=split_linebreaks)
        raw = out.tobytes()
        return [raw[int(offs[i]):int(offs[i + 1])] for i in range(len(texts))]

    def predict_listing_arena(self, texts: Sequence[str], scores: bool = False, tag_scores: bool = False, tagged: bool = False,
                              fullwidth: bool = True, wsconst: Sequence = (), no_norm_order: bool = False, split_linebreaks: bool = False):
        """The `predict` CLI's output for these lines (predict/src/main.rs:122-176) as the device made it: (uint8 arena, uint64 [S+1] offsets
        of the lines in it).  Per line T, the --scores block and the --tag-scores block, in the normalising loop's order or (no_norm_order)
        the --no-norm loop's.  `wsconst` as for tokenize ("G": VPT_FLAG_CONCAT_GRAPHEMES, in the same one call)."""
        if not texts:
            return np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
        utf8, boff = pack_texts([t.encode("utf-8") for t in texts])
        listing = ((_lib.VPT_LISTING_SCORES if scores else 0) | (_lib.VPT_LISTING_TAG_SCORES if tag_scores else 0) |
                   (_lib.VPT_LISTING_TAGGED if tagged else 0) | (_lib.VPT_LISTING_NO_NORM_ORDER if no_norm_order else 0))
        flags = (_lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0) | _label_flags(wsconst, split_linebreaks)
        return self.predict_listing_packed(utf8, boff, listing, flags=flags)

    def tokenize_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, tagged: bool = False, flags: int = 0,
                        text_out: Optional[np.ndarray] = None, offsets_out: Optional[np.ndarray] = None,
                        tagger: Optional["PatternMatchTagger"] = None):
        """vpt_tokenize_batch (with `tagger`: vpt_tokenize_batch_rules, its suffix bound added to the capacity) over a packed batch: (uint8 tokenized text, uint64 [S+1] offsets).  `text_out` / `offsets_out` may be
        preallocated (pinned) arrays; text_out needs 3 x the text bytes (+ text bytes x max_tag_suffix() when tagged)."""
        L = _lib.load()
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        S = len(byte_offsets) - 1
        cap = 3 * len(utf8) + (len(utf8) * (self.max_tag_suffix() + (tagger.max_tag_suffix(self) if tagger is not None else 0)) if tagged else 0)
        if text_out is None:
            text_out = np.zeros(max(cap, 1), dtype=np.uint8)
        if offsets_out is None:
            offsets_out = np.zeros(S + 1, dtype=np.uint64)
        if tagger is not None:
            st = L.vpt_tokenize_batch_rules(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, flags, int(tagged), text_out.ctypes.data,
                                            min(cap, text_out.nbytes), offsets_out.ctypes.data, tagger.handle(self))
        else:
            st = L.vpt_tokenize_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, flags, int(tagged), text_out.ctypes.data,
                                      min(cap, text_out.nbytes), offsets_out.ctypes.data)
        if st != _lib.VPT_OK:
            _raise(st)
        return text_out[:int(offsets_out[S])], offsets_out

    def tokenize(self, texts: Sequence[str], tagged: bool = False, fullwidth: bool = False, wsconst: Sequence = (),
                 split_linebreaks: bool = False, tagger: Optional["PatternMatchTagger"] = None) -> List[str]:
        """Lines in, tokenized lines out (vpt_tokenize_batch): the CLI's loop (predict/src/main.rs:122-176) for a batch,
        with char counting, scoring, post-filters, tagging and the writer on the device.  `wsconst`: CharacterType values (the
        KyteaWsConstFilter of that type) and / or "G" (ConcatGraphemeClustersFilter, predict/src/main.rs:101-104: VPT_FLAG_CONCAT_GRAPHEMES, a
        launch behind the scoring launch that runs after the other label filters) -- one call either way."""
        if not texts:
            return []
        utf8, boff = pack_texts([t.encode("utf-8") for t in texts])
        S = len(texts)
        flags = (_lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0) | _label_flags(wsconst, split_linebreaks)
        text, toff = self.tokenize_packed(utf8, boff, tagged=tagged, flags=flags, tagger=tagger)
        raw = bytes(text)
        return [raw[int(toff[i]):int(toff[i + 1])].decode("utf-8") for i in range(S)]

    def write_tokenized_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, out_offsets: np.ndarray,
                               labels: np.ndarray, tagged: bool = False, fullwidth: bool = False,
                               tagger: Optional["PatternMatchTagger"] = None):
        """Sentence::write_tokenized_text (sentence.rs:850-886) over a packed batch on the device; with `tagged`
        (predictors created with predict_tags) fill_tags runs first and every token gets its "/tag" suffixes.
        Returns (uint8 text, uint64 [S+1] offsets): sentence i is text[offsets[i]:offsets[i+1]]."""
        L = _lib.load()
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        S = len(byte_offsets) - 1
        nbytes = int(byte_offsets[S] - byte_offsets[0]) if S else 0
        nchars = int(out_offsets[S] - out_offsets[0]) + S if S else 0
        cap = 2 * nbytes + nchars
        if tagged:
            sfx = C.c_uint32(0)
            if L.vpt_predictor_max_tag_suffix(self._h, C.byref(sfx)) != _lib.VPT_OK:
                _raise(_lib.VPT_INVALID_ARGUMENT)
            cap += nchars * (int(sfx.value) + (tagger.max_tag_suffix(self) if tagger is not None else 0))
        text = np.zeros(max(cap, 1), dtype=np.uint8)
        toff = np.zeros(S + 1, dtype=np.uint64)
        lab = labels if len(labels) else np.zeros(1, dtype=np.uint8)
        if tagged and tagger is not None:
            st = L.vpt_write_tagged_batch_rules(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, out_offsets.ctypes.data, lab.ctypes.data,
                                                _lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0, text.ctypes.data, cap, toff.ctypes.data,
                                                tagger.handle(self))
        elif tagged:
            st = L.vpt_write_tagged_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, out_offsets.ctypes.data, lab.ctypes.data,
                                          _lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0, text.ctypes.data, cap, toff.ctypes.data)
        else:
            st = L.vpt_write_tokenized_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, out_offsets.ctypes.data,
                                             lab.ctypes.data, text.ctypes.data, cap, toff.ctypes.data)
        if st != _lib.VPT_OK:
            _raise(st)
        return text[:int(toff[S])], toff

    def write_tokenized_batch(self, sentences: Sequence["Sentence"], tagged: bool = False,
                              tagger: Optional["PatternMatchTagger"] = None) -> List[str]:
        """write_tokenized_text for many sentences in one launch.  tagged: fill_tags + "/tag" suffixes on the device
        (the sentences' own tags are not touched); otherwise sentences that carry tags take the host writer."""
        if not sentences:
            return []
        if tagged:
            utf8, boff = pack_texts([s._utf8 for s in sentences])
            ooff = np.zeros(len(sentences) + 1, dtype=np.uint64)
            ooff[1:] = np.cumsum([len(s) - 1 for s in sentences])
            labels = np.concatenate([np.asarray(s._boundaries, dtype=np.uint8) for s in sentences]) if int(ooff[-1]) else np.zeros(0, np.uint8)
            text, toff = self.write_tokenized_packed(utf8, boff, ooff, labels, tagged=True, tagger=tagger)
            raw = bytes(text)
            return [raw[int(toff[i]):int(toff[i + 1])].decode("utf-8") for i in range(len(sentences))]
        utf8, boff = pack_texts([s._utf8 for s in sentences])
        ooff = np.zeros(len(sentences) + 1, dtype=np.uint64)
        ooff[1:] = np.cumsum([len(s) - 1 for s in sentences])
        labels = np.concatenate([np.asarray(s._boundaries, dtype=np.uint8) for s in sentences]) if int(ooff[-1]) else np.zeros(0, np.uint8)
        text, toff = self.write_tokenized_packed(utf8, boff, ooff, labels)
        raw = bytes(text)
        out = []
        for i, s in enumerate(sentences):
            t = raw[int(toff[i]):int(toff[i + 1])].decode("utf-8")
            if s._n_tags:   # "/tag" suffixes: splice them in token by token (rare path, host strings)
                t = s.write_tokenized_text()
            out.append(t)
        return out

    def fill_tags_batch(self, sentences: Sequence["Sentence"], tagger: Optional["PatternMatchTagger"] = None) -> None:
        """Sentence::fill_tags for many sentences in one launch; candidate indices are mapped to the tag strings of
        the tag model whose token equals the token's surface (the LAST one of a repeated token, predictor.rs:466-478).
        `tagger`: a PatternMatchTagger applied behind fill_tags on the device; its tags come back through PatternMatchTagger.tag.  Not
        together with store_tag_scores(True) in this mirror (VaporettoError): rule tags have no scores, and the host pipeline that returns
        scores takes no tagger -- a caller that wants both binds the tagger to a DeviceBatch and calls fill_tags_scores there."""
        if not sentences:
            return
        utf8, boff = pack_texts([s._utf8 for s in sentences])
        ooff = np.zeros(len(sentences) + 1, dtype=np.uint64)
        ooff[1:] = np.cumsum([len(s) - 1 for s in sentences])
        labels = np.concatenate([np.asarray(s._boundaries, dtype=np.uint8) for s in sentences]) if int(ooff[-1]) else np.zeros(0, np.uint8)
        scores = models = None
        if self._store_tag_scores and tagger is not None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: tagger: not with store_tag_scores (rule tags have no scores)")
        if self._store_tag_scores:
            tags, scores, models = self.fill_tags_scores_packed(utf8, boff, ooff, labels)
        else:
            tags = self.fill_tags_packed(utf8, boff, ooff, labels, tagger=tagger)
        nt = tags.shape[1]
        rule_tags = {}   # -(2 + id) -> the tagger's string
        tag_model_list = self._model.tag_models() if scores is not None else None
        if self._tag_models is None:
            self._tag_models = {tm.token: tm for tm in self._model.tag_models()}
        for i, s in enumerate(sentences):
            g0 = int(ooff[i]) + i
            n = len(s)
            s._n_tags = nt
            s._tags = [None] * (n * nt)
            s._tag_scores = []   # sentence.rs:96: Vec<Option<(&[Vec<String>], Vec<i32>)>>, empty unless store_tag_scores
            if scores is not None and nt:
                s._tag_scores = [None] * n
                for e in range(n):
                    mi = int(models[g0 + e])
                    if mi >= 0:
                        tm_ = tag_model_list[mi]
                        s._tag_scores[e] = (tm_.tags, scores[g0 + e, :len(tm_.bias)].tolist())
            if nt == 0:
                continue
            start, valid = 0, True
            for e in range(n):
                b = CharacterBoundary.WordBoundary if e == n - 1 else int(s._boundaries[e])
                if b == CharacterBoundary.Unknown:
                    valid = False
                    continue
                if b != CharacterBoundary.WordBoundary:
                    continue
                if valid:
                    for j in range(nt if tagger is not None else 0):   # rule tags: -(2 + id), resolved through the tagger
                        idx = int(tags[g0 + e, j])
                        if idx <= -2:
                            if idx not in rule_tags:
                                rule_tags[idx] = tagger.tag(self, -2 - idx)
                            s._tags[e * nt + j] = rule_tags[idx]
                    tm = self._tag_models.get(s._text[start:e + 1])
                    if tm is not None:
                        for j in range(min(nt, len(tm.tags))):
                            idx = int(tags[g0 + e, j])
                            if idx >= 0:
                                s._tags[e * nt + j] = tm.tags[j][idx]
                start, valid = e + 1, True

    def predict_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, fullwidth: bool = False,
                       wsconst: Sequence = (), split_linebreaks: bool = False, linebreaks_first: bool = False):
        """utf8: uint8[total bytes]; byte_offsets: uint64[S+1].  Returns (scores, labels, out_offsets).
        fullwidth: score the text as KyteaFullwidthFilter would rewrite it (the CLI's default normalisation).
        wsconst: CharacterTypes for KyteaWsConstFilter and / or "G" (ConcatGraphemeClustersFilter: VPT_FLAG_CONCAT_GRAPHEMES, always the last
        filter); split_linebreaks: SplitLinebreaksFilter (labels only), after the wsconst filters unless linebreaks_first
        (VPT_FLAG_LINEBREAKS_FIRST: the order of vaporetto_tantivy's post-filters)."""
        flags = (_lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0) | _label_flags(wsconst, split_linebreaks, linebreaks_first)
        L = _lib.load()
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        S = len(byte_offsets) - 1
        ooff = np.zeros(S + 1, dtype=np.uint64)
        st = L.vpt_count_boundaries(utf8.ctypes.data, byte_offsets.ctypes.data, S, ooff.ctypes.data)
        if st != _lib.VPT_OK:
            _raise(st)
        nb = int(ooff[S])
        scores = np.zeros(max(nb, 1), dtype=np.int32)
        labels = np.zeros(max(nb, 1), dtype=np.uint8)
        st = L.vpt_predict_batch_flags(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, scores.ctypes.data,
                                       labels.ctypes.data, ooff.ctypes.data, flags)
        if st != _lib.VPT_OK:
            _raise(st)
        return scores[:nb], labels[:nb], ooff

    def concat_graphemes_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, out_offsets: np.ndarray, labels: np.ndarray,
                                fullwidth: bool = False) -> np.ndarray:
        """vpt_concat_graphemes_batch: ConcatGraphemeClustersFilter on the CALLER'S labels (uint8 per boundary, 0 / 1 / 2), on the device -- a
        copy with every label inside an extended grapheme cluster cleared; fullwidth: the clusters of the KyteaFullwidthFilter image."""
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        out = np.array(labels, dtype=np.uint8, copy=True)
        lab = out if len(out) else np.zeros(1, dtype=np.uint8)
        st = _lib.load().vpt_concat_graphemes_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, len(byte_offsets) - 1, out_offsets.ctypes.data,
                                                    _lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0, lab.ctypes.data)
        if st != _lib.VPT_OK:
            _raise(st)
        return out

    def token_spans_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, out_offsets: np.ndarray, labels: np.ndarray):
        """vpt_token_spans_batch: the token spans (vaporetto_tantivy/src/lib.rs:183-192) of a packed batch for the CALLER'S labels, on the
        device.  Returns (token_offsets uint64 [S+1], token_ends uint32): document i owns token_ends[token_offsets[i]:token_offsets[i+1]], the
        byte offset behind every one of its tokens from its first byte."""
        L = _lib.load()
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        S = len(byte_offsets) - 1
        cap = (int(out_offsets[S] - out_offsets[0]) + S) if S else 0
        toff = np.zeros(S + 1, dtype=np.uint64)
        ends = np.zeros(max(cap, 1), dtype=np.uint32)
        lab = labels if len(labels) else np.zeros(1, dtype=np.uint8)
        st = L.vpt_token_spans_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, out_offsets.ctypes.data, lab.ctypes.data,
                                     toff.ctypes.data, ends.ctypes.data, cap)
        if st != _lib.VPT_OK:
            _raise(st)
        return toff, ends[:int(toff[S])]

    def token_stream_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, wsconst: str = "", ends_out: Optional[np.ndarray] = None,
                            offsets_out: Optional[np.ndarray] = None):
        """vpt_token_stream_batch: VaporettoTokenizer::token_stream (vaporetto_tantivy/src/lib.rs:160-192) for a packed batch of documents
        (empty ones allowed) -- KyteaFullwidthFilter, predict, SplitLinebreaksFilter, the wsconst filters, the spans, all on the device.
        `wsconst`: chars of "DRHTKOG" ("G": ConcatGraphemeClustersFilter, the last filter wherever it stands).  Returns (token_offsets, token_ends) as
        token_spans_packed; `ends_out` / `offsets_out` may be preallocated (pinned) arrays, ends_out of one uint32 per text byte."""
        L = _lib.load()
        flags = wsconst_flags(wsconst, allow_graphemes=True)
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        S = len(byte_offsets) - 1
        cap = int(byte_offsets[S] - byte_offsets[0]) if S else 0
        if offsets_out is None:
            offsets_out = np.zeros(S + 1, dtype=np.uint64)
        if ends_out is None:
            ends_out = np.zeros(max(cap, 1), dtype=np.uint32)
        st = L.vpt_token_stream_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, flags, offsets_out.ctypes.data,
                                      ends_out.ctypes.data, min(cap, len(ends_out)))
        if st != _lib.VPT_OK:
            _raise(st)
        return offsets_out, ends_out[:int(offsets_out[S])]

    def _parse_packed(self, entry, utf8: np.ndarray, byte_offsets: np.ndarray, capacity: Optional[int]) -> dict:
        """One of the device parsers (`entry`: its C entry point) over a packed batch; capacity: what the output buffers hold."""
        import torch
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        S = len(byte_offsets) - 1
        B = len(utf8) if capacity is None else int(capacity)
        dev = torch.device("cuda", self.device)

        def d(n, dt):
            return torch.zeros(max(n, 1), dtype=dt, device=dev)
        d_text = torch.from_numpy(np.concatenate([utf8, np.zeros(1, np.uint8)])).to(dev)
        d_boff = torch.from_numpy(byte_offsets.view(np.int64)).to(dev)
        o = {"raw": d(B, torch.uint8), "raw_offsets": d(S + 1, torch.int64), "out_offsets": d(S + 1, torch.int64), "labels": d(B, torch.uint8),
             "n_tags": d(S, torch.int32), "tag_index": d(B + 1, torch.int64), "span_offsets": d(B + 1, torch.int64), "tag_bytes": d(B, torch.uint8)}
        batch = DeviceBatch(self)
        stream = torch.cuda.current_stream(dev).cuda_stream
        st = entry(self._h, batch._h, d_text.data_ptr(), d_boff.data_ptr(), S, B, *[o[k].data_ptr() for k in _PARSED_KEYS], stream)
        if st != _lib.VPT_OK:
            _raise(st)
        batch.sync()
        h = {k: v.cpu().numpy() for k, v in o.items()}
        for k in ("raw_offsets", "out_offsets", "tag_index", "span_offsets"):
            h[k] = h[k].view(np.uint64)
        h["n_tags"] = h["n_tags"].view(np.uint32)[:S]
        return _trim_parsed(h, S)

    def parse_tokenized_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray) -> dict:
        """Sentence::from_tokenized for a packed batch of tokenized lines, on the device (vpt_parse_tokenized_batch_device).  Returns
        the arrays of parse_tokenized_host."""
        return self._parse_packed(_lib.load().vpt_parse_tokenized_batch_device, utf8, byte_offsets, None)

    def parse_partial_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, capacity: Optional[int] = None) -> dict:
        """Sentence::from_partial_annotation for a packed batch of partially annotated lines, on the device (vpt_parse_partial_batch_device).
        Returns the arrays of parse_partial_host.  capacity: what the output buffers hold (default: the input's bytes)."""
        return self._parse_packed(_lib.load().vpt_parse_partial_batch_device, utf8, byte_offsets, capacity)

    def write_partial_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, out_offsets: np.ndarray, labels: np.ndarray,
                             n_tags: Optional[np.ndarray] = None, tag_index: Optional[np.ndarray] = None,
                             span_offsets: Optional[np.ndarray] = None, tag_bytes: Optional[np.ndarray] = None, capacity: Optional[int] = None):
        """Sentence::write_partial_annotation_text (sentence.rs:907-944) over a packed batch on the device (vpt_write_partial_batch_device), from
        the arrays the parsers return; n_tags None: no tags.  Returns (uint8 text, uint64 [S+1] offsets)."""
        import torch
        a = _partial_writer_args(utf8, byte_offsets, out_offsets, labels, n_tags, tag_index, span_offsets, tag_bytes)
        S, cap = a["S"], a["cap"] if capacity is None else int(capacity)
        dev = torch.device("cuda", self.device)

        def up(x):
            x = x if len(x) else np.zeros(1, x.dtype)
            signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(x.dtype)
            return torch.from_numpy(x.view(signed) if signed else x).to(dev)
        dv = {k: up(a[k]) for k in ("utf8", "boff", "ooff", "labels")}
        if a["n_tags"] is not None:
            dv.update({k: up(a[k]) for k in ("n_tags", "tag_index", "span_offsets", "tag_bytes")})
        ptr = lambda k: dv[k].data_ptr() if k in dv else None
        d_text = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
        d_toff = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        batch = DeviceBatch(self)
        stream = torch.cuda.current_stream(dev).cuda_stream
        st = _lib.load().vpt_write_partial_batch_device(self._h, batch._h, ptr("utf8"), ptr("boff"), S, ptr("ooff"), ptr("labels"), ptr("n_tags"),
                                                        ptr("tag_index"), ptr("span_offsets"), ptr("tag_bytes"), d_text.data_ptr(), cap,
                                                        d_toff.data_ptr(), stream)
        if st != _lib.VPT_OK:
            _raise(st)
        batch.sync()
        toff = d_toff.cpu().numpy().view(np.uint64)
        return d_text.cpu().numpy()[:int(toff[S])], toff

    def evaluate(self, lines: Sequence[str], predict_tags: bool = False, wsconst: Sequence = (), no_norm: bool = False) -> dict:
        """The `evaluate` CLI (evaluate/src/main.rs:91-193) over tokenized lines: empty lines are skipped, every other line must parse.
        wsconst: CharacterType values and / or "G".  The "(line N)" of a parse error counts the given lines, empty ones included.  Returns the counters (tp, tn, fp, fn, n_sys, n_ref, n_cor, n_sentences) and the
        P / R / F1 of both metrics (char_*, word_*; NaN for 0 / 0).  The whole pipeline is one call (vpt_evaluate_batch), "G"
        (VPT_FLAG_CONCAT_GRAPHEMES) included: the filter's launch sits between a chunk's scoring and its fill_tags + compare."""
        if predict_tags and not self._predict_tags:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: this predictor is created with predict_tags = false")
        index = [k for k, ln in enumerate(lines) if ln]   # the input line of every line evaluated (errors name the input's line)
        lines = [lines[k] for k in index]
        try:
            return self._evaluate(lines, predict_tags, wsconst, no_norm)
        except VaporettoError as e:
            m = re.search(r" \(line (\d+)\)$", str(e))
            if not m or int(m.group(1)) >= len(index):
                raise
            raise VaporettoError(e.kind, str(e)[:m.start()] + " (line %d)" % index[int(m.group(1))]) from None

    def _evaluate(self, lines, predict_tags, wsconst, no_norm) -> dict:
        flags = (0 if no_norm else _lib.VPT_FLAG_KYTEA_FULLWIDTH) | _label_flags(wsconst)
        utf8, boff = pack_texts([ln.encode("utf-8") for ln in lines])
        counts = np.zeros(8, dtype=np.uint64)
        st = _lib.load().vpt_evaluate_batch(self._h, utf8.ctypes.data, boff.ctypes.data, len(lines), flags, int(bool(predict_tags)),
                                            counts.ctypes.data)
        if st != _lib.VPT_OK:
            _raise(st)
        return evaluation_result(counts)

    def char_types_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, out_offsets: np.ndarray, fullwidth: bool = False) -> np.ndarray:
        """Sentence::char_types for a packed batch, from the device: uint8 per char (char c of sentence i at out_offsets[i] + i + c)."""
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        S = len(byte_offsets) - 1
        types = np.zeros(int(out_offsets[S]) + S + 1, dtype=np.uint8)
        st = _lib.load().vpt_char_types_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, out_offsets.ctypes.data,
                                              _lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0, types.ctypes.data)
        if st != _lib.VPT_OK:
            _raise(st)
        return types[:int(out_offsets[S]) + S]


def predict_packed_sharded(predictors: Sequence[Predictor], utf8: np.ndarray, byte_offsets: np.ndarray, out_offsets: Optional[np.ndarray] = None,
                           scores: Optional[np.ndarray] = None, labels: Optional[np.ndarray] = None, flags: int = 0, want_scores: bool = True):
    """vpt_predict_batch_sharded: one batch over several predictors (one per GPU), contiguous shards balanced by chars.
    `scores` / `labels` may be preallocated (pinned) arrays.  Returns (scores, labels, out_offsets); with want_scores=False the
    scores stay on the device (NULL scores_out: a tokenizer only needs the labels, and 4 of the 5 bytes per boundary that
    would cross the link back are scores) and None is returned for them."""
    L = _lib.load()
    utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
    byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
    S = len(byte_offsets) - 1
    if out_offsets is None:
        out_offsets = count_boundaries(utf8, byte_offsets)
    out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
    nb = int(out_offsets[S])
    if scores is None and want_scores:
        scores = np.zeros(max(nb, 1), dtype=np.int32)
    if labels is None:
        labels = np.zeros(max(nb, 1), dtype=np.uint8)
    handles = (C.c_void_p * len(predictors))(*[p.handle for p in predictors])
    st = L.vpt_predict_batch_sharded(handles, len(predictors), utf8.ctypes.data, byte_offsets.ctypes.data, S,
                                     scores.ctypes.data if want_scores else None, labels.ctypes.data, out_offsets.ctypes.data, flags)
    if st != _lib.VPT_OK:
        _raise(st)
    return (scores[:nb] if want_scores else None), labels[:nb], out_offsets


def shard_bounds(out_offsets: np.ndarray, n_shards: int) -> np.ndarray:
    """vpt_shard_bounds: contiguous sentence ranges balanced by characters."""
    out_offsets = np.ascontiguousarray(out_offsets, dtype=np.uint64)
    bounds = np.zeros(n_shards + 1, dtype=np.uint64)
    st = _lib.load().vpt_shard_bounds(out_offsets.ctypes.data, len(out_offsets) - 1, n_shards, bounds.ctypes.data)
    if st != _lib.VPT_OK:
        _raise(st)
    return bounds


class PinnedArray:
    """A numpy array over page-locked host memory from vpt_host_alloc (hipHostMalloc): copies to and from the device are
    DMA transfers at the PCIe rate.  Keep the object alive as long as `.array` is in use."""

    def __init__(self, shape, dtype):
        self.array = None
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._ptr = C.c_void_p()
        st = _lib.load().vpt_host_alloc(max(n, 1), C.byref(self._ptr))
        if st != _lib.VPT_OK:
            self._ptr = None
            _raise(st)
        buf = (C.c_uint8 * max(n, 1)).from_address(self._ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def __del__(self):
        if getattr(self, "_ptr", None):
            self.array = None
            _lib.load().vpt_host_free(self._ptr)
            self._ptr = None


class DeviceBatch:
    """Per-caller workspace for the device-resident entry point (vpt_batch)."""

    def __init__(self, predictor: Predictor, timing: bool = False):
        self._p = predictor
        self._h = C.c_void_p()
        L = _lib.load()
        st = L.vpt_batch_create(predictor.handle, C.byref(self._h))
        if st != _lib.VPT_OK:
            self._h = None
            _raise(st)
        if timing:
            st = L.vpt_batch_set_timing(self._h, 1)
            if st != _lib.VPT_OK:
                _raise(st)

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().vpt_batch_destroy(self._h)
            self._h = None

    def predict(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int,
                max_sentence_bytes: int, d_scores: int, d_labels: int, stream: int = 0) -> None:
        """All pointers are raw device addresses (e.g. torch.Tensor.data_ptr()); enqueues and returns."""
        st = _lib.load().vpt_predict_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_sentences,
                                                  total_boundaries, max_sentence_bytes, d_scores, d_labels, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def fill_tags(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int, d_labels: int,
                  d_tags: int, stream: int = 0) -> None:
        """Device-resident Sentence::fill_tags for the batch (vpt_fill_tags_batch_device); enqueues and returns.  d_tags = 0 (NULL): the
        tags stay in the workspace as one record per token that has a tag model (what write_tagged reads; expand_tags makes the dense array)."""
        st = _lib.load().vpt_fill_tags_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_sentences,
                                                    total_boundaries, d_labels, d_tags or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def expand_tags(self, n_sentences: int, total_boundaries: int, d_tags: int, stream: int = 0) -> None:
        """Sentence::tags() of the batch of the last fill_tags call on this workspace as the dense int32 [chars, n_tags] array
        (vpt_expand_tags_batch_device): None (-1) everywhere but at the last char of a token that has a tag model."""
        st = _lib.load().vpt_expand_tags_batch_device(self._p.handle, self._h, n_sentences, total_boundaries, d_tags, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def fill_tags_scores(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int, d_labels: int,
                         d_tags: int, d_tag_scores: int, d_tag_models: int, stream: int = 0) -> None:
        """fill_tags plus Predictor::store_tag_scores' score vectors and every token's tag model (vpt_fill_tags_scores_batch_device);
        d_tag_scores / d_tag_models may be 0 (NULL)."""
        st = _lib.load().vpt_fill_tags_scores_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_sentences, total_boundaries,
                                                           d_labels, d_tags, d_tag_scores or None, d_tag_models or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def write_tokenized(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int, d_labels: int,
                        d_text_out: int, text_capacity: int, d_text_offsets: int, stream: int = 0) -> None:
        """Device-resident write_tokenized_text for the batch (vpt_write_tokenized_batch_device); enqueues and returns."""
        st = _lib.load().vpt_write_tokenized_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_sentences,
                                                          total_boundaries, d_labels, d_text_out, text_capacity, d_text_offsets, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def token_spans(self, d_utf8: int, d_boff: int, d_ooff: int, n_documents: int, total_boundaries: int, d_labels: int,
                    d_token_offsets: int, d_token_ends: int, capacity: int, stream: int = 0) -> None:
        """Device-resident token spans of the batch for the labels at d_labels (vpt_token_spans_batch_device); enqueues and returns."""
        st = _lib.load().vpt_token_spans_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_documents, total_boundaries,
                                                      d_labels or None, d_token_offsets, d_token_ends or None, capacity, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def token_tags(self, d_utf8: int, d_boff: int, d_ooff: int, n_documents: int, total_boundaries: int, d_labels: int,
                   d_token_offsets: int, d_token_ends: int, d_token_tags: int, capacity: int, stream: int = 0) -> None:
        """Device-resident token spans with n_tags int32 per token at d_token_tags (vpt_token_tags_batch_device): >= 0 an id of
        Predictor.tag_strings(), -1 None, -(2 + id) a rule tag of the pattern tagger set on this workspace.  After fill_tags on this
        workspace for the same batch and labels; enqueues and returns."""
        st = _lib.load().vpt_token_tags_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_documents, total_boundaries,
                                                     d_labels or None, d_token_offsets, d_token_ends or None, d_token_tags or None, capacity, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def token_filter(self, stop, d_token_offsets: int, d_token_ends: int, d_token_tags: int, n_documents: int, capacity_in: int, d_offsets_out: int,
                     d_starts_out: int, d_ends_out: int, d_positions_out: int, d_tags_out: int, capacity: int, stream: int = 0) -> None:
        """Device-resident stop filter over a finished CSR (vpt_token_filter_batch_device; stop: a TagStopFilter or None); enqueues and returns."""
        st = _lib.load().vpt_token_filter_batch_device(self._p.handle, self._h, stop.handle if stop is not None else None, d_token_offsets,
                                                       d_token_ends or None, d_token_tags or None, n_documents, capacity_in, d_offsets_out,
                                                       d_starts_out or None, d_ends_out or None, d_positions_out or None, d_tags_out or None,
                                                       capacity, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def token_ids(self, vocab: "Vocabulary", d_utf8: int, d_boff: int, n_documents: int, d_token_offsets: int, d_token_starts: int, d_token_ends: int,
                  capacity_in: int, d_token_ids: int, flags: int = 0, stream: int = 0) -> None:
        """Device-resident vocabulary ids of a finished CSR (vpt_token_ids_batch_device): int32 per token at d_token_ids, vocab.unk_id for a token
        that is no entry.  d_token_starts 0: the spans of token_spans / token_tags; else the filter's starts.  flags: 0 or VPT_FLAG_KYTEA_FULLWIDTH.
        Enqueues and returns."""
        st = _lib.load().vpt_token_ids_batch_device(self._p.handle, self._h, vocab.handle if vocab is not None else None, d_utf8, d_boff, n_documents,
                                                    d_token_offsets, d_token_starts or None, d_token_ends or None, capacity_in, flags,
                                                    d_token_ids or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def count_tokens(self, counter: "VocabularyCounter", d_utf8: int, d_boff: int, n_documents: int, d_token_offsets: int, d_token_starts: int,
                     d_token_ends: int, capacity_in: int, flags: int = 0, stream: int = 0) -> None:
        """Device-resident count of a finished CSR's token surfaces into `counter` (vpt_vocab_count_batch_device): the arrays and flags of
        token_ids.  One call at a time on a counter, in stream order.  Enqueues and returns; errors (a hostile CSR, a full counter) at sync()."""
        st = _lib.load().vpt_vocab_count_batch_device(self._p.handle, self._h, counter.handle if counter is not None else None, d_utf8, d_boff,
                                                      n_documents, d_token_offsets, d_token_starts or None, d_token_ends or None, capacity_in, flags,
                                                      stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def postings(self, d_token_offsets: int, n_documents: int, d_token_ids: int, capacity_in: int, n_terms: int, doc_base: int, d_term_offsets: int,
                 d_post_docs: int, d_post_tfs: int, capacity_out: int, d_post_first: int = 0, d_token_order: int = 0, d_counts: int = 0,
                 stream: int = 0) -> None:
        """Device-resident postings of a finished CSR's ids (vpt_postings_batch_device): term -> (document, tf), term-major; d_post_first and
        d_token_order both 0 (NULL) or neither.  Enqueues and returns; errors (a hostile CSR, more postings than capacity_out) at sync()."""
        for name, v, top in (("n_terms", n_terms, 1 << 32), ("doc_base", doc_base, 1 << 64), ("capacity_in", capacity_in, 1 << 64),
                             ("capacity_out", capacity_out, 1 << 64)):
            if not 0 <= int(v) < top:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
        st = _lib.load().vpt_postings_batch_device(self._p.handle, self._h, d_token_offsets or None, n_documents, d_token_ids or None, int(capacity_in),
                                                   int(n_terms), int(doc_base), d_term_offsets or None, d_post_docs or None, d_post_tfs or None,
                                                   int(capacity_out), d_post_first or None, d_token_order or None, d_counts or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def merge_postings(self, segments: Sequence[Tuple[int, int, int, int, int]], n_terms_out: int, d_term_offsets: int, d_post_docs: int,
                       d_post_tfs: int, capacity_out: int, d_counts: int, ordered: bool = False, stream: int = 0, flags: Optional[int] = None) -> None:
        """Device-resident merge of postings segments (vpt_postings_merge_device).  segments: (d_term_offsets, d_post_docs, d_post_tfs, n_terms,
        capacity) each, raw device pointers; the outputs must not alias them.  ordered: the promise VPT_POSTINGS_MERGE_ORDERED (flags, when
        given, is passed as it is).  Enqueues and returns; errors (a hostile segment, a broken promise, a tf above 32 bits, more postings
        than capacity_out) at sync()."""
        segs = (_lib.PostingsSegment * max(len(segments), 1))()
        for k, (toff, docs, tfs, n_terms, cap) in enumerate(segments):
            for name, v, top in (("segment n_terms", n_terms, 1 << 32), ("segment capacity", cap, 1 << 64)):
                if not 0 <= int(v) < top:
                    raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
            segs[k] = _lib.PostingsSegment(toff or None, docs or None, tfs or None, int(n_terms), int(cap))
        for name, v, top in (("n_terms_out", n_terms_out, 1 << 32), ("capacity_out", capacity_out, 1 << 64)):
            if not 0 <= int(v) < top:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
        f = (_lib.VPT_POSTINGS_MERGE_ORDERED if ordered else 0) if flags is None else int(flags)
        st = _lib.load().vpt_postings_merge_device(self._p.handle, self._h, C.addressof(segs), len(segments), int(n_terms_out), f, d_term_offsets or None,
                                                   d_post_docs or None, d_post_tfs or None, int(capacity_out), d_counts or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def merge_positional_postings(self, segments: Sequence[Tuple[int, int, int, int, int, int, int, int]], n_terms_out: int, d_term_offsets: int,
                                  d_post_docs: int, d_post_tfs: int, d_post_first: int, capacity_out: int, d_post_positions: int,
                                  capacity_positions_out: int, d_counts: int, ordered: bool = False, stream: int = 0,
                                  flags: Optional[int] = None) -> None:
        """Device-resident merge of POSITIONAL segments (vpt_postings_merge_positional_device).  segments: (d_term_offsets, d_post_docs,
        d_post_tfs, d_post_first, d_post_positions, n_terms, capacity, capacity_positions) each, raw device pointers; the outputs must not alias
        them.  d_counts: uint64 [3] = merged postings, combined postings, merged positions.  Enqueues and returns; errors (merge_postings' list,
        post_first that is no segment's, positions that do not ascend or repeat, more positions than capacity_positions_out) at sync()."""
        segs = (_lib.PostingsPositionalSegment * max(len(segments), 1))()
        for k, (toff, docs, tfs, first, ppos, n_terms, cap, cap_pos) in enumerate(segments):
            for name, v, top in (("segment n_terms", n_terms, 1 << 32), ("segment capacity", cap, 1 << 64), ("segment capacity_positions", cap_pos, 1 << 64)):
                if not 0 <= int(v) < top:
                    raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
            segs[k] = _lib.PostingsPositionalSegment(toff or None, docs or None, tfs or None, first or None, ppos or None, int(n_terms), int(cap), int(cap_pos))
        for name, v, top in (("n_terms_out", n_terms_out, 1 << 32), ("capacity_out", capacity_out, 1 << 64),
                             ("capacity_positions_out", capacity_positions_out, 1 << 64)):
            if not 0 <= int(v) < top:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
        f = (_lib.VPT_POSTINGS_MERGE_ORDERED if ordered else 0) if flags is None else int(flags)
        st = _lib.load().vpt_postings_merge_positional_device(self._p.handle, self._h, C.addressof(segs), len(segments), int(n_terms_out), f,
                                                              d_term_offsets or None, d_post_docs or None, d_post_tfs or None, d_post_first or None,
                                                              int(capacity_out), d_post_positions or None, int(capacity_positions_out),
                                                              d_counts or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    @staticmethod
    def postings_merge_limit() -> int:
        """the most segments one merge takes (vpt_postings_merge_limits)"""
        v = C.c_uint32()
        st = _lib.load().vpt_postings_merge_limits(C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value)

    def search_postings(self, d_term_offsets: int, d_post_docs: int, d_post_tfs: int, n_terms: int, capacity_postings: int, doc_base: int,
                        n_documents: int, d_doc_lens: int, d_query_offsets: int, d_query_terms: int, d_query_weights: int, n_queries: int,
                        capacity_slots: int, k1: float, b: float, avgdl: float, k: int, capacity_candidates: int, d_hit_docs: int, d_hit_scores: int,
                        d_hit_counts: int, d_match_counts: int, d_counts: int, stream: int = 0) -> None:
        """Device-resident BM25 top-k search of a batch of queries over one segment (vpt_postings_search_device), raw device pointers.
        Enqueues and returns; errors (a hostile segment or query CSR, a bad weight, a query above the slot limit, more candidates than
        capacity_candidates) at sync()."""
        for name, v, top in (("n_terms", n_terms, 1 << 32), ("n_queries", n_queries, 1 << 32), ("k", k, 1 << 32), ("doc_base", doc_base, 1 << 64),
                             ("n_documents", n_documents, 1 << 64), ("capacity_postings", capacity_postings, 1 << 64),
                             ("capacity_slots", capacity_slots, 1 << 64), ("capacity_candidates", capacity_candidates, 1 << 64)):
            if not 0 <= int(v) < top:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
        st = _lib.load().vpt_postings_search_device(self._p.handle, self._h, d_term_offsets or None, d_post_docs or None, d_post_tfs or None, int(n_terms),
                                                    int(capacity_postings), int(doc_base), int(n_documents), d_doc_lens or None, d_query_offsets or None,
                                                    d_query_terms or None, d_query_weights or None, int(n_queries), int(capacity_slots), float(k1), float(b),
                                                    float(avgdl), int(k), int(capacity_candidates), d_hit_docs or None, d_hit_scores or None,
                                                    d_hit_counts or None, d_match_counts or None, d_counts or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def boolean_search_postings(self, d_term_offsets: int, d_post_docs: int, d_post_tfs: int, n_terms: int, capacity_postings: int, doc_base: int,
                                n_documents: int, d_doc_lens: int, d_query_offsets: int, d_query_terms: int, d_query_weights: int, d_query_occurs: int,
                                n_queries: int, capacity_slots: int, k1: float, b: float, avgdl: float, k: int, capacity_candidates: int,
                                d_hit_docs: int, d_hit_scores: int, d_hit_counts: int, d_match_counts: int, d_counts: int, stream: int = 0) -> None:
        """Device-resident BM25 top-k search with MUST / SHOULD / MUST_NOT slots (vpt_postings_boolean_search_device), raw device pointers:
        search_postings' arguments and d_query_occurs (uint8 per slot, Occur) behind the weights; capacity_candidates bounds the PLACES.
        Enqueues and returns; errors (search_postings' and an occur above 2) at sync()."""
        for name, v, top in (("n_terms", n_terms, 1 << 32), ("n_queries", n_queries, 1 << 32), ("k", k, 1 << 32), ("doc_base", doc_base, 1 << 64),
                             ("n_documents", n_documents, 1 << 64), ("capacity_postings", capacity_postings, 1 << 64),
                             ("capacity_slots", capacity_slots, 1 << 64), ("capacity_candidates", capacity_candidates, 1 << 64)):
            if not 0 <= int(v) < top:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
        st = _lib.load().vpt_postings_boolean_search_device(self._p.handle, self._h, d_term_offsets or None, d_post_docs or None, d_post_tfs or None,
                                                            int(n_terms), int(capacity_postings), int(doc_base), int(n_documents), d_doc_lens or None,
                                                            d_query_offsets or None, d_query_terms or None, d_query_weights or None,
                                                            d_query_occurs or None, int(n_queries), int(capacity_slots), float(k1), float(b),
                                                            float(avgdl), int(k), int(capacity_candidates), d_hit_docs or None, d_hit_scores or None,
                                                            d_hit_counts or None, d_match_counts or None, d_counts or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    @staticmethod
    def postings_search_limit() -> int:
        """the most slots a query of a search may have (vpt_postings_search_limits)"""
        v = C.c_uint32()
        st = _lib.load().vpt_postings_search_limits(C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value)

    def postings_positions(self, d_token_offsets: int, n_documents: int, capacity_in: int, d_token_positions: int, d_term_offsets: int, n_terms: int,
                           d_post_first: int, capacity_postings: int, d_token_order: int, d_post_positions: int, stream: int = 0) -> None:
        """Device-resident position lists of a segment (vpt_postings_positions_device), behind postings() with the optional pair;
        d_token_positions 0 (NULL): a token's index inside its document.  Enqueues and returns; errors (a hostile CSR, positions that do not
        strictly ascend inside a posting) at sync()."""
        for name, v, top in (("n_terms", n_terms, 1 << 32), ("capacity_in", capacity_in, 1 << 64), ("capacity_postings", capacity_postings, 1 << 64)):
            if not 0 <= int(v) < top:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
        st = _lib.load().vpt_postings_positions_device(self._p.handle, self._h, d_token_offsets or None, n_documents, int(capacity_in),
                                                       d_token_positions or None, d_term_offsets or None, int(n_terms), d_post_first or None,
                                                       int(capacity_postings), d_token_order or None, d_post_positions or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def phrase_search_postings(self, d_term_offsets: int, d_post_docs: int, d_post_tfs: int, d_post_first: int, d_post_positions: int, n_terms: int,
                               capacity_postings: int, capacity_positions: int, doc_base: int, n_documents: int, d_doc_lens: int,
                               d_query_offsets: int, d_query_terms: int, d_query_weights: int, n_queries: int, capacity_slots: int, k1: float,
                               b: float, avgdl: float, k: int, capacity_probes: int, d_hit_docs: int, d_hit_scores: int, d_hit_freqs: int,
                               d_hit_counts: int, d_match_counts: int, d_counts: int, stream: int = 0, slops: Optional[int] = None) -> None:
        """Device-resident exact-phrase BM25 top-k search over one positional segment (vpt_postings_phrase_search_device), raw device
        pointers; a query is one phrase with one weight; d_hit_freqs may be 0 (NULL).  slops: a device pointer to one uint32 slop per query
        (0: NULL, every slop 0) makes it the sloppy search (vpt_postings_sloppy_phrase_search_device); None: the exact call.  Enqueues and
        returns; errors at sync()."""
        for name, v, top in (("n_terms", n_terms, 1 << 32), ("n_queries", n_queries, 1 << 32), ("k", k, 1 << 32), ("doc_base", doc_base, 1 << 64),
                             ("n_documents", n_documents, 1 << 64), ("capacity_postings", capacity_postings, 1 << 64),
                             ("capacity_positions", capacity_positions, 1 << 64), ("capacity_slots", capacity_slots, 1 << 64),
                             ("capacity_probes", capacity_probes, 1 << 64)):
            if not 0 <= int(v) < top:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
        head = (self._p.handle, self._h, d_term_offsets or None, d_post_docs or None, d_post_tfs or None, d_post_first or None, d_post_positions or None,
                int(n_terms), int(capacity_postings), int(capacity_positions), int(doc_base), int(n_documents), d_doc_lens or None,
                d_query_offsets or None, d_query_terms or None, d_query_weights or None)
        tail = (int(n_queries), int(capacity_slots), float(k1), float(b), float(avgdl), int(k), int(capacity_probes), d_hit_docs or None,
                d_hit_scores or None, d_hit_freqs or None, d_hit_counts or None, d_match_counts or None, d_counts or None, stream)
        if slops is None:
            st = _lib.load().vpt_postings_phrase_search_device(*(head + tail))
        else:
            st = _lib.load().vpt_postings_sloppy_phrase_search_device(*(head + (slops or None,) + tail))
        if st != _lib.VPT_OK:
            _raise(st)

    def phrase_lists_postings(self, d_term_offsets: int, d_post_docs: int, d_post_tfs: int, d_post_first: int, d_post_positions: int, n_terms: int,
                              capacity_postings: int, capacity_positions: int, doc_base: int, n_documents: int, d_phrase_offsets: int,
                              d_phrase_terms: int, n_phrases: int, capacity_slots: int, capacity_probes: int, d_list_offsets: int, d_list_docs: int,
                              d_list_tfs: int, capacity_lists: int, d_counts: int, stream: int = 0, slops: Optional[int] = None) -> None:
        """Device-resident phrases to posting lists over one positional segment (vpt_postings_phrase_lists_device), raw device pointers: per
        phrase the matching documents (global numbers, ascending) and their phrase frequencies, what clause_search_postings takes as derived
        lists.  slops: as in phrase_search_postings (vpt_postings_sloppy_phrase_lists_device).  Enqueues and returns; errors (the phrase
        search's, and capacity_lists too small with the need in counts[1]) at sync()."""
        for name, v, top in (("n_terms", n_terms, 1 << 32), ("n_phrases", n_phrases, 1 << 32), ("doc_base", doc_base, 1 << 64),
                             ("n_documents", n_documents, 1 << 64), ("capacity_postings", capacity_postings, 1 << 64),
                             ("capacity_positions", capacity_positions, 1 << 64), ("capacity_slots", capacity_slots, 1 << 64),
                             ("capacity_probes", capacity_probes, 1 << 64), ("capacity_lists", capacity_lists, 1 << 64)):
            if not 0 <= int(v) < top:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
        head = (self._p.handle, self._h, d_term_offsets or None, d_post_docs or None, d_post_tfs or None, d_post_first or None, d_post_positions or None,
                int(n_terms), int(capacity_postings), int(capacity_positions), int(doc_base), int(n_documents), d_phrase_offsets or None,
                d_phrase_terms or None)
        tail = (int(n_phrases), int(capacity_slots), int(capacity_probes), d_list_offsets or None, d_list_docs or None, d_list_tfs or None,
                int(capacity_lists), d_counts or None, stream)
        if slops is None:
            st = _lib.load().vpt_postings_phrase_lists_device(*(head + tail))
        else:
            st = _lib.load().vpt_postings_sloppy_phrase_lists_device(*(head + (slops or None,) + tail))
        if st != _lib.VPT_OK:
            _raise(st)

    def clause_search_postings(self, d_term_offsets: int, d_post_docs: int, d_post_tfs: int, n_terms: int, capacity_postings: int, d_list_offsets: int,
                               d_list_docs: int, d_list_tfs: int, n_lists: int, capacity_lists: int, doc_base: int, n_documents: int, d_doc_lens: int,
                               d_query_offsets: int, d_query_terms: int, d_query_weights: int, d_query_occurs: int, n_queries: int, capacity_slots: int,
                               k1: float, b: float, avgdl: float, k: int, capacity_candidates: int, d_hit_docs: int, d_hit_scores: int,
                               d_hit_counts: int, d_match_counts: int, d_counts: int, stream: int = 0) -> None:
        """Device-resident boolean search over a segment plus derived lists (vpt_postings_clause_search_device), raw device pointers:
        boolean_search_postings' arguments and the lists phrase_lists_postings wrote; a slot's term t in [n_terms, n_terms + n_lists) names
        list t - n_terms.  May follow phrase_lists_postings on the same stream without a sync: an error of that call leaves the outputs
        alone.  Enqueues and returns; errors at sync()."""
        for name, v, top in (("n_terms", n_terms, 1 << 32), ("n_lists", n_lists, 1 << 32), ("n_queries", n_queries, 1 << 32), ("k", k, 1 << 32),
                             ("doc_base", doc_base, 1 << 64), ("n_documents", n_documents, 1 << 64), ("capacity_postings", capacity_postings, 1 << 64),
                             ("capacity_lists", capacity_lists, 1 << 64), ("capacity_slots", capacity_slots, 1 << 64),
                             ("capacity_candidates", capacity_candidates, 1 << 64)):
            if not 0 <= int(v) < top:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: out of range" % name)
        st = _lib.load().vpt_postings_clause_search_device(self._p.handle, self._h, d_term_offsets or None, d_post_docs or None, d_post_tfs or None,
                                                           int(n_terms), int(capacity_postings), d_list_offsets or None, d_list_docs or None,
                                                           d_list_tfs or None, int(n_lists), int(capacity_lists), int(doc_base), int(n_documents),
                                                           d_doc_lens or None, d_query_offsets or None, d_query_terms or None, d_query_weights or None,
                                                           d_query_occurs or None, int(n_queries), int(capacity_slots), float(k1), float(b),
                                                           float(avgdl), int(k), int(capacity_candidates), d_hit_docs or None, d_hit_scores or None,
                                                           d_hit_counts or None, d_match_counts or None, d_counts or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    @staticmethod
    def postings_phrase_limit() -> int:
        """the most slots a phrase may have (vpt_postings_phrase_limits)"""
        v = C.c_uint32()
        st = _lib.load().vpt_postings_phrase_limits(C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value)

    @staticmethod
    def postings_sloppy_phrase_limits():
        """(the most slots a phrase may have, the largest slop) (vpt_postings_sloppy_phrase_limits)"""
        v, s = C.c_uint32(), C.c_uint32()
        st = _lib.load().vpt_postings_sloppy_phrase_limits(C.byref(v), C.byref(s))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value), int(s.value)

    @staticmethod
    def postings_tile() -> int:
        v = C.c_uint32()
        st = _lib.load().vpt_postings_tile(C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value)

    def concat_graphemes(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int, d_labels: int, stream: int = 0) -> None:
        """Device-resident ConcatGraphemeClustersFilter on the labels at d_labels, in place (vpt_concat_graphemes_batch_device; the clusters of
        the KyteaFullwidthFilter image when set_flags / set_fullwidth say so); enqueues and returns."""
        st = _lib.load().vpt_concat_graphemes_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_sentences, total_boundaries,
                                                           d_labels or None, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def predict_listing(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int, text_bytes: int, d_scores: int,
                        d_labels: int, listing: int, d_out: int, capacity: int, d_listing_offsets: int, stream: int = 0) -> None:
        """The predict CLI's listing of the batch from the scores and labels on the device (vpt_predict_listing_batch_device); enqueues and
        returns."""
        st = _lib.load().vpt_predict_listing_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_sentences, total_boundaries, text_bytes,
                                                          d_scores or None, d_labels or None, int(listing), d_out or None, capacity,
                                                          d_listing_offsets, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def predict_write(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int, max_sentence_bytes: int,
                      d_scores: int, d_labels: int, d_text_out: int, text_capacity: int, d_text_offsets: int, stream: int = 0) -> None:
        """Predictor::predict and write_tokenized_text (no tags) in ONE scoring launch (vpt_predict_write_batch_device): the tiles of the
        specialised kernel write their tokenized text themselves.  d_scores / d_labels may be 0; enqueues and returns."""
        st = _lib.load().vpt_predict_write_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_sentences, total_boundaries,
                                                        max_sentence_bytes, d_scores or None, d_labels or None, d_text_out, text_capacity,
                                                        d_text_offsets, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def write_tagged(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int, d_labels: int,
                     d_tags: int, d_text_out: int, text_capacity: int, d_text_offsets: int, stream: int = 0) -> None:
        """write_tokenized_text with "/tag" suffixes from the records the fill_tags call on this workspace left for this batch
        (vpt_write_tagged_batch_device; d_tags is not read any more and may be 0); enqueues and returns."""
        st = _lib.load().vpt_write_tagged_batch_device(self._p.handle, self._h, d_utf8, d_boff, d_ooff, n_sentences, total_boundaries,
                                                       d_labels, d_tags or None, d_text_out, text_capacity, d_text_offsets, stream)
        if st != _lib.VPT_OK:
            _raise(st)

    def set_pattern_tagger(self, tagger: Optional["PatternMatchTagger"]) -> None:
        """vpt_batch_set_pattern_tagger: the rules applied behind every fill_tags on this workspace (None: none)."""
        self._tagger = tagger   # (keeps the table alive while it is bound)
        st = _lib.load().vpt_batch_set_pattern_tagger(self._h, tagger.handle(self._p) if tagger is not None else None)
        if st != _lib.VPT_OK:
            _raise(st)

    def set_fullwidth(self, enabled: bool) -> None:
        """Score the text as KyteaFullwidthFilter would rewrite it (vpt_batch_set_flags)."""
        st = _lib.load().vpt_batch_set_flags(self._h, _lib.VPT_FLAG_KYTEA_FULLWIDTH if enabled else 0)
        if st != _lib.VPT_OK:
            _raise(st)

    def set_flags(self, flags: int) -> None:
        """VPT_FLAG_* for the calls that follow on this workspace (vpt_batch_set_flags): KyteaFullwidthFilter on the text, KyteaWsConstFilter /
        SplitLinebreaksFilter / ConcatGraphemeClustersFilter (VPT_FLAG_CONCAT_GRAPHEMES, always the last) on the labels."""
        st = _lib.load().vpt_batch_set_flags(self._h, int(flags))
        if st != _lib.VPT_OK:
            _raise(st)

    def set_max_sentence_chars(self, max_chars: int) -> None:
        """Optional tighter bound than max_sentence_bytes (fuller tiles); 0 = unknown."""
        st = _lib.load().vpt_batch_set_max_sentence_chars(self._h, int(max_chars))
        if st != _lib.VPT_OK:
            _raise(st)

    def sync(self) -> None:
        st = _lib.load().vpt_batch_sync(self._h)
        if st != _lib.VPT_OK:
            _raise(st)

    def kernel_ms(self) -> Tuple[float, int]:
        ms, nt = C.c_float(), C.c_uint32()
        st = _lib.load().vpt_batch_kernel_ms(self._h, C.byref(ms), C.byref(nt))
        if st != _lib.VPT_OK:
            _raise(st)
        return ms.value, nt.value


    def last_plan(self) -> dict:
        """How the last predict call cut its batch (vpt_batch_last_plan)."""
        n, tf, kind = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = _lib.load().vpt_batch_last_plan(self._h, C.byref(n), C.byref(tf), C.byref(kind))
        if st != _lib.VPT_OK:
            _raise(st)
        runs, run_sent = C.c_uint64(), C.c_uint32()
        st = _lib.load().vpt_batch_tag_plan(self._h, C.byref(runs), C.byref(run_sent))
        if st != _lib.VPT_OK:
            _raise(st)
        pol = C.c_uint32()
        st = _lib.load().vpt_batch_last_text_policy(self._h, C.byref(pol))
        if st != _lib.VPT_OK:
            _raise(st)
        # tag_runs / tag_run_sent: the front-end runs of the last fill_tags call and the sentences of a run (vpt_batch_tag_plan);
        # text_policy: how the scoring launch loaded its text (vpt_batch_last_text_policy)
        return {"tiles": n.value, "tile_flat": tf.value, "kind": ("general kernels", "whole-sentence tiles", "cut tiles")[min(kind.value, 2)],
                "tag_runs": runs.value, "tag_run_sent": run_sent.value, "text_policy": ("plain", "nt")[min(pol.value, 1)]}

    def kernel_times(self) -> np.ndarray:
        """Durations (ms) of the timed scoring-kernel launches since the last kernel_ms(), oldest first (at most 256)."""
        out = np.zeros(256, dtype=np.float32)
        n = C.c_size_t(0)
        st = _lib.load().vpt_batch_kernel_times(self._h, out.ctypes.data, len(out), C.byref(n))
        if st != _lib.VPT_OK:
            _raise(st)
        return out[:n.value].copy()

    def phase_cycles(self):
        """Per-phase shader cycles of the specialised kernel (needs VPT_PROFILE_PHASES set before creation)."""
        arr = (C.c_uint64 * 8)()
        st = _lib.load().vpt_batch_phase_cycles(self._h, C.byref(arr))
        if st != _lib.VPT_OK:
            _raise(st)
        return list(arr)

    def node_reads(self):
        """Node reads the specialised kernel issued since the last call (vpt_batch_node_reads; needs VPT_PROFILE_PHASES)."""
        arr = (C.c_uint64 * 8)()
        st = _lib.load().vpt_batch_node_reads(self._h, C.byref(arr))
        if st != _lib.VPT_OK:
            _raise(st)
        return dict(zip(["unigram_nodes", "bigram_nodes", "trigram_nodes", "deep_entries", "deep_rows", "global_type_rows"], [int(x) for x in arr][:6]))


def _trim_parsed(h: dict, S: int) -> dict:
    ro, oo = h["raw_offsets"][:S + 1], h["out_offsets"][:S + 1]
    n_chars = int(oo[S]) + S if S else 0
    ti = h["tag_index"][:n_chars + 1]
    n_t = int(ti[n_chars]) if S else 0
    so = h["span_offsets"][:n_t + 1]
    return {"raw": h["raw"][:int(ro[S]) if S else 0], "raw_offsets": ro, "out_offsets": oo, "labels": h["labels"][:int(oo[S]) if S else 0],
            "n_tags": h["n_tags"][:S], "tag_index": ti, "span_offsets": so, "tag_bytes": h["tag_bytes"][:int(so[n_t]) if S else 0]}


_PARSED_KEYS = ("raw", "raw_offsets", "out_offsets", "labels", "n_tags", "tag_index", "span_offsets", "tag_bytes")


def _parse_host(entry, lines: Sequence[bytes]) -> dict:
    """One of the host parsers (`entry`: its C entry point) over lines."""
    utf8, boff = pack_texts(list(lines))
    S, B = len(lines), len(utf8)
    h = {"raw": np.zeros(max(B, 1), np.uint8), "raw_offsets": np.zeros(S + 1, np.uint64), "out_offsets": np.zeros(S + 1, np.uint64),
         "labels": np.zeros(max(B, 1), np.uint8), "n_tags": np.zeros(max(S, 1), np.uint32), "tag_index": np.zeros(B + 1, np.uint64),
         "span_offsets": np.zeros(B + 1, np.uint64), "tag_bytes": np.zeros(max(B, 1), np.uint8)}
    u = utf8 if B else np.zeros(1, np.uint8)
    st = entry(u.ctypes.data, boff.ctypes.data, S, *[h[k].ctypes.data for k in _PARSED_KEYS])
    if st != _lib.VPT_OK:
        _raise(st)
    return _trim_parsed(h, S)


def parse_tokenized_host(lines: Sequence[bytes]) -> dict:
    """vpt_parse_tokenized_batch (host): tokenized lines -> {raw, raw_offsets, out_offsets, labels, n_tags, tag_index, span_offsets,
    tag_bytes} as include/vaporetto_hip.h describes them."""
    return _parse_host(_lib.load().vpt_parse_tokenized_batch, lines)


def parse_partial_host(lines: Sequence[bytes]) -> dict:
    """vpt_parse_partial_batch (host): partially annotated lines -> the arrays of parse_tokenized_host, labels 0 / 1 / 2 and tags on any char."""
    return _parse_host(_lib.load().vpt_parse_partial_batch, lines)


def _partial_writer_args(utf8, byte_offsets, out_offsets, labels, n_tags, tag_index, span_offsets, tag_bytes) -> dict:
    a = {"utf8": np.ascontiguousarray(utf8, dtype=np.uint8), "boff": np.ascontiguousarray(byte_offsets, dtype=np.uint64),
         "ooff": np.ascontiguousarray(out_offsets, dtype=np.uint64), "labels": np.ascontiguousarray(labels, dtype=np.uint8), "n_tags": None}
    a["S"] = len(a["boff"]) - 1
    a["cap"] = len(a["utf8"]) + len(a["labels"])
    if n_tags is not None:
        a["n_tags"] = np.ascontiguousarray(n_tags, dtype=np.uint32)
        a["tag_index"] = np.ascontiguousarray(tag_index, dtype=np.uint64)
        a["span_offsets"] = np.ascontiguousarray(span_offsets, dtype=np.uint64)
        a["tag_bytes"] = np.ascontiguousarray(tag_bytes, dtype=np.uint8)
        a["cap"] += len(a["span_offsets"]) + len(a["tag_bytes"])
    return a


def write_partial_host(utf8: np.ndarray, byte_offsets: np.ndarray, out_offsets: np.ndarray, labels: np.ndarray, n_tags: Optional[np.ndarray] = None,
                       tag_index: Optional[np.ndarray] = None, span_offsets: Optional[np.ndarray] = None, tag_bytes: Optional[np.ndarray] = None,
                       capacity: Optional[int] = None):
    """vpt_write_partial_batch (host): Sentence::write_partial_annotation_text over a packed batch, from the arrays the parsers return;
    n_tags None: no tags.  Returns (uint8 text, uint64 [S+1] offsets)."""
    a = _partial_writer_args(utf8, byte_offsets, out_offsets, labels, n_tags, tag_index, span_offsets, tag_bytes)
    S, cap = a["S"], a["cap"] if capacity is None else int(capacity)
    text = np.zeros(max(cap, 1), np.uint8)
    toff = np.zeros(S + 1, np.uint64)
    keep = [x if len(x) else np.zeros(1, x.dtype) for x in (a["utf8"], a["labels"])]
    tags = [None] * 4
    if a["n_tags"] is not None:
        keep += [x if len(x) else np.zeros(1, x.dtype) for x in (a["n_tags"], a["tag_index"], a["span_offsets"], a["tag_bytes"])]
        tags = [x.ctypes.data for x in keep[2:]]
    st = _lib.load().vpt_write_partial_batch(keep[0].ctypes.data, a["boff"].ctypes.data, S, a["ooff"].ctypes.data, keep[1].ctypes.data, *tags,
                                             text.ctypes.data, cap, toff.ctypes.data)
    if st != _lib.VPT_OK:
        _raise(st)
    return text[:int(toff[S])], toff


def evaluation_result(counts) -> dict:
    """The counters of vpt_evaluate_batch with the P / R / F1 the `evaluate` CLI prints (evaluate/src/main.rs:139-191), in f64."""
    c = [int(x) for x in counts]
    r = dict(zip(("tp", "tn", "fp", "fn", "n_sys", "n_ref", "n_cor", "n_sentences"), c))

    def div(a, b):
        return float(a) / float(b) if b else (float("nan") if a == 0 else float("inf"))

    def f1(p, q):
        return div(2.0 * p * q, p + q) if not (p + q == 0 or p != p or q != q) else float("nan")
    for name, num, den_p, den_r in (("char", r["tp"], r["tp"] + r["fp"], r["tp"] + r["fn"]), ("word", r["n_cor"], r["n_sys"], r["n_ref"])):
        p, q = div(num, den_p), div(num, den_r)
        r[name + "_precision"], r[name + "_recall"], r[name + "_f1"] = p, q, f1(p, q)
    return r


_WSCONST_TYPES = {"D": 1, "R": 2, "H": 3, "T": 4, "K": 5, "O": 6}


def _label_flags(wsconst: Sequence, split_linebreaks: bool = False, linebreaks_first: bool = False) -> int:
    """The VPT_FLAG_* label post-filter bits of a `wsconst` sequence of CharacterType values and / or "G" (VPT_FLAG_CONCAT_GRAPHEMES)."""
    flags = 0
    for t in wsconst:
        flags |= _lib.VPT_FLAG_CONCAT_GRAPHEMES if (isinstance(t, str) and t == "G") else _lib.VPT_FLAG_WSCONST(int(t))
    if split_linebreaks:
        flags |= _lib.VPT_FLAG_SPLIT_LINEBREAKS
    if linebreaks_first:
        flags |= _lib.VPT_FLAG_LINEBREAKS_FIRST
    return flags


def wsconst_flags(wsconst: str, allow_graphemes: bool = False) -> int:
    """The VPT_FLAG_WSCONST bits of a wsconst string of vaporetto_tantivy (D R H T K O; vaporetto_tantivy/src/lib.rs:69-86); with
    allow_graphemes "G" is VPT_FLAG_CONCAT_GRAPHEMES (the device applies it last, which is the adapter's result for any place of "G")."""
    flags = 0
    for c in wsconst:
        if c == "G" and allow_graphemes:
            flags |= _lib.VPT_FLAG_CONCAT_GRAPHEMES
            continue
        if c not in _WSCONST_TYPES:
            raise VaporettoError("InvalidArgument", "Could not parse a wsconst value")   # lib.rs:82
        flags |= _lib.VPT_FLAG_WSCONST(_WSCONST_TYPES[c])
    return flags


class TantivyToken:
    """tantivy's Token as VaporettoTokenStream fills it (vaporetto_tantivy/src/lib.rs:204-219): byte offsets into the caller's text."""
    __slots__ = ("text", "offset_from", "offset_to", "position", "position_length", "id")   # id: only under VaporettoTokenizer(vocab=...)

    def __init__(self, text: str, offset_from: int, offset_to: int, position: int, position_length: int):
        self.text, self.offset_from, self.offset_to, self.position, self.position_length = text, offset_from, offset_to, position, position_length

    def _key(self):
        return (self.text, self.offset_from, self.offset_to, self.position, self.position_length)

    def __eq__(self, other):
        return isinstance(other, TantivyToken) and self._key() == other._key()

    def __repr__(self):
        return "Token(text=%r, offset_from=%d, offset_to=%d, position=%d, position_length=%d)" % self._key()


class TagStopFilter:
    """vpt_tag_stop_create: a stop set for the tagged token stream from (slot, tag string) pairs -- a token is dropped when, for some pair, its
    slot's tag equals the pair's string (a tag model's or, with `tagger`, a rule's; None never matches; an unknown string matches nothing).
    Tied to `predictor` (and `tagger`); immutable."""

    def __init__(self, predictor: "Predictor", pairs, tagger: Optional["PatternMatchTagger"] = None):
        pairs = list(pairs)
        slots = np.array([int(s) for s, _ in pairs] or [0], np.uint32)
        raws = [t.encode("utf-8") for _, t in pairs]
        tb, toff = pack_texts(raws)
        tb = tb if len(tb) else np.zeros(1, np.uint8)
        h = C.c_void_p()
        self._keep = (predictor, tagger)
        st = _lib.load().vpt_tag_stop_create(predictor.handle, tagger.handle(predictor) if tagger is not None else None, slots.ctypes.data,
                                             tb.ctypes.data, toff.ctypes.data, len(pairs), C.byref(h))
        if st != _lib.VPT_OK:
            _raise(st)
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None:
            try:
                _lib.load().vpt_tag_stop_destroy(h)
            except Exception:
                pass
            self.handle = None


class Vocabulary:
    """vpt_vocab_create: token surface -> int32 id on the predictor's device.  `surfaces`: a sequence of str (or bytes); entry k gets id k, a
    token that is no entry `unk_id`.  An empty surface, a NUL, invalid UTF-8 and a repeated surface are errors that name the entry.  Tied to
    `predictor`; immutable."""

    def __init__(self, predictor: "Predictor", surfaces, unk_id: int = -1):
        raws = [s.encode("utf-8", "surrogatepass") if isinstance(s, str) else bytes(s) for s in surfaces]
        sb, off = pack_texts(raws)
        sb = sb if len(sb) else np.zeros(1, np.uint8)
        h = C.c_void_p()
        self._keep = predictor
        self.unk_id = int(unk_id)
        st = _lib.load().vpt_vocab_create(predictor.handle, sb.ctypes.data, off.ctypes.data, len(raws), self.unk_id, C.byref(h))
        if st != _lib.VPT_OK:
            _raise(st)
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None:
            try:
                _lib.load().vpt_vocab_destroy(h)
            except Exception:
                pass
            self.handle = None

    def info(self) -> dict:
        k, n, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = _lib.load().vpt_vocab_info(self.handle, C.byref(k), C.byref(n), C.byref(m))
        if st != _lib.VPT_OK:
            _raise(st)
        return {"n_keys": int(k.value), "n_slots": int(n.value), "max_surface_chars": int(m.value)}

    def surface(self, entry_id: int) -> str:
        ptr, n = C.c_void_p(), C.c_size_t()
        st = _lib.load().vpt_vocab_surface(self.handle, int(entry_id), C.byref(ptr), C.byref(n))
        if st != _lib.VPT_OK:
            _raise(st)
        return C.string_at(ptr.value, n.value).decode("utf-8") if n.value else ""

    @staticmethod
    def tile() -> int:
        v = C.c_uint32()
        st = _lib.load().vpt_vocab_tile(C.byref(v))
        if st != _lib.VPT_OK:
            _raise(st)
        return int(v.value)


class VocabularyCounter:
    """vpt_vocab_counter_create: an accumulating table token surface -> count on the predictor's device; what it counted goes to Vocabulary.
    max_keys: the distinct surfaces it can hold (1 .. 2^24); a token of more than max_surface_chars chars is skipped; arena_chars: the code
    points it can keep, 0 = 8 * max_keys.  Tied to `predictor`.  MUTABLE: one call at a time, in stream order.  A counter that has become full
    raises "vocab counter: full" at the sync, at later count calls and at finish(), until reset()."""

    def __init__(self, predictor: "Predictor", max_keys: int, max_surface_chars: int = 64, arena_chars: int = 0):
        for name, v in (("max_keys", max_keys), ("max_surface_chars", max_surface_chars), ("arena_chars", arena_chars)):
            if not 0 <= int(v) < 1 << 64:
                raise VaporettoError("InvalidArgumentError: %s: out of range" % name)
        h = C.c_void_p()
        self._keep = predictor
        st = _lib.load().vpt_vocab_counter_create(predictor.handle, int(max_keys), int(max_surface_chars), int(arena_chars), C.byref(h))
        if st != _lib.VPT_OK:
            _raise(st)
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None:
            try:
                _lib.load().vpt_vocab_counter_destroy(h)
            except Exception:
                pass
            self.handle = None

    def info(self) -> dict:
        k, c, s, n, f = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        st = _lib.load().vpt_vocab_counter_info(self.handle, C.byref(k), C.byref(c), C.byref(s), C.byref(n), C.byref(f))
        if st != _lib.VPT_OK:
            _raise(st)
        return {"n_keys": int(k.value), "n_counted": int(c.value), "n_skipped": int(s.value), "n_slots": int(n.value), "full": bool(f.value)}

    def reset(self) -> None:
        st = _lib.load().vpt_vocab_counter_reset(self.handle)
        if st != _lib.VPT_OK:
            _raise(st)

    def finish_raw(self, min_count: int = 1, max_entries: Optional[int] = None):
        """vpt_vocab_counter_finish as it is: (surfaces uint8, offsets uint64 [n + 1], counts uint64 [n]), copies of the handle's arrays --
        what vpt_vocab_create takes."""
        sp, op, cp, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        st = _lib.load().vpt_vocab_counter_finish(self.handle, int(min_count), int(max_entries or 0), C.byref(sp), C.byref(op), C.byref(cp), C.byref(n))
        if st != _lib.VPT_OK:
            _raise(st)
        k = n.value
        offsets = np.frombuffer(C.string_at(op.value, 8 * (k + 1)), np.uint64).copy()
        counts = np.frombuffer(C.string_at(cp.value, 8 * k), np.uint64).copy() if k else np.zeros(0, np.uint64)
        nb = int(offsets[k])
        surfaces = np.frombuffer(C.string_at(sp.value, nb), np.uint8).copy() if nb else np.zeros(0, np.uint8)
        return surfaces, offsets, counts

    def finish(self, min_count: int = 1, max_entries: Optional[int] = None):
        """A snapshot (counting may go on): (surfaces list[str], counts uint64) of the keys of count >= min_count, by count descending, then by
        code points ascending; the first max_entries of them (None or 0: all)."""
        surfaces, offsets, counts = self.finish_raw(min_count, max_entries)
        raw = surfaces.tobytes()
        return [raw[int(offsets[k]):int(offsets[k + 1])].decode("utf-8") for k in range(len(counts))], counts


def bm25_idf(n_documents: int, df: int) -> np.float32:
    """tantivy's BM25 idf, float32(log(1 + (N - df + 0.5) / (df + 0.5))) evaluated in double (vpt_okapi_idf: the one implementation of every binding)"""
    v = C.c_float()
    if not (0 <= int(n_documents) < 1 << 64 and 0 <= int(df) < 1 << 64):
        raise VaporettoError("InvalidArgument", "InvalidArgumentError: df: above n_documents")
    st = _lib.load().vpt_okapi_idf(int(n_documents), int(df), C.byref(v))
    if st != _lib.VPT_OK:
        _raise(st)
    return np.float32(v.value)


def _slops_of(slop, n: int, what: str) -> Optional[np.ndarray]:
    """slop= of the phrase searches -> None (the int 0: the exact call) or one uint32 per phrase / clause; a value outside [0, 2^32) is refused
    here, one above the limit by the device (vpt_postings_sloppy_phrase_limits)"""
    if isinstance(slop, (int, np.integer)):
        if int(slop) == 0:
            return None
        values = [int(slop)] * n
    else:
        values = [int(s) for s in slop]
        if len(values) != n:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: slop: an int or one per %s" % what)
    if any(not 0 <= s < 1 << 32 for s in values):
        raise VaporettoError("InvalidArgument", "InvalidArgumentError: query: a slop above 31")
    return np.array(values + [0], np.uint32)


class Occur(enum.IntEnum):  # VPT_OCCUR_*: tantivy's Occur of a BooleanQuery's clause
    SHOULD = 0
    MUST = 1
    MUST_NOT = 2


class Postings:
    """The postings of one batch (a segment), term-major (vpt_postings_batch_device): term k's postings are [term_offsets[k], term_offsets[k + 1])
    of `docs` (doc_base + the document's index, ascending within a term) and `tfs`.  With positions: posting q's tokens are
    order[first[q] : first[q + 1]], ascending token indices of the batch; else `first` and `order` are None.  `positions`: an array, or None --
    posting q's position list is positions[first[q] : first[q + 1]], strictly ascending (vpt_postings_positions_device); with it the postings
    are a positional segment and phrase_search runs.  n_dropped: the tokens whose id was no term (negative or >= n_terms)."""

    def __init__(self, term_offsets: np.ndarray, docs: np.ndarray, tfs: np.ndarray, first: Optional[np.ndarray], order: Optional[np.ndarray],
                 n_dropped: int):
        self.term_offsets, self.docs, self.tfs, self.first, self.order, self.n_dropped = term_offsets, docs, tfs, first, order, int(n_dropped)
        self.positions = None    # uint32 [indexed tokens]: every posting's position list (postings_packed / index_batch with positions=True)
        self.n_combined = 0      # merge: the input postings that were combined into another
        self._predictor = None   # who made it (merge's default device)
        self.doc_lens = None     # search: uint32, the token count of document doc_base + i (index_batch / index_batches attach both)
        self.doc_base = None

    def __len__(self) -> int:
        return len(self.docs)

    def df(self) -> np.ndarray:
        """the document frequency of every term: uint64 [n_terms]"""
        return np.diff(self.term_offsets)

    def postings(self, term: int):
        """(docs, tfs) of one term"""
        a, b = int(self.term_offsets[term]), int(self.term_offsets[term + 1])
        return self.docs[a:b], self.tfs[a:b]

    @staticmethod
    def merge(segments: Sequence["Postings"], ordered: bool = False, predictor: Optional["Predictor"] = None, n_terms: Optional[int] = None,
              capacity: Optional[int] = None, positions: bool = False, capacity_positions: Optional[int] = None) -> "Postings":
        """The merge of segments that share a term id space (vpt_postings_merge): per term the union of their lists by document, a document
        that stands in several of them one posting whose tf is the sum; n_dropped the segments' sum, n_combined the postings that went into
        another.  ordered: the promise that every segment's documents are above those of the one before (checked on the device; no sort).
        n_terms: the merged term count (default: the largest of the segments').  predictor: whose device (default: the one that made the
        first segment).  No `order`: token indices are local to a segment.  positions: the position lists are merged too
        (vpt_postings_merge_positional; every segment must carry `first` and `positions`): the result has `first` and `positions`, a merged
        posting's list the ascending union of its inputs', and phrase_search runs on it; without it `first` and `positions` are None."""
        segments = list(segments)
        pred = predictor or next((s._predictor for s in segments if getattr(s, "_predictor", None) is not None), None)
        if pred is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: merge: no predictor (pass predictor=)")
        if positions and any(s.first is None or s.positions is None for s in segments):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: merge: a segment was made without positions")
        keep = [(np.ascontiguousarray(s.term_offsets, dtype=np.uint64), np.ascontiguousarray(s.docs, dtype=np.uint32),
                 np.ascontiguousarray(s.tfs, dtype=np.uint32)) for s in segments]
        for t, d, f in keep:
            if len(t) == 0 or len(d) != len(f):
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: merge: a segment's arrays do not belong together")
        n_out = max([len(t) - 1 for t, _, _ in keep] + [0]) if n_terms is None else int(n_terms)
        cap = sum(len(d) for _, d, _ in keep) if capacity is None else int(capacity)
        term = np.zeros(max(n_out, 0) + 1, np.uint64)
        docs, tfs = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        n_post, n_comb, n_pos = C.c_uint64(), C.c_uint64(), C.c_uint64()
        if not 0 <= n_out < 1 << 32:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: n_terms: must be between 1 and 2^24")
        flags = _lib.VPT_POSTINGS_MERGE_ORDERED if ordered else 0
        if positions:
            pkeep = [(np.ascontiguousarray(s.first, dtype=np.uint64), np.ascontiguousarray(s.positions, dtype=np.uint32)) for s in segments]
            for (_, d, _), (fi, _) in zip(keep, pkeep):
                if len(fi) != len(d) + 1:
                    raise VaporettoError("InvalidArgument", "InvalidArgumentError: merge: a segment's arrays do not belong together")
            segs = (_lib.PostingsPositionalSegment * max(len(keep), 1))()
            for k, ((t, d, f), (fi, pp)) in enumerate(zip(keep, pkeep)):
                segs[k] = _lib.PostingsPositionalSegment(t.ctypes.data, d.ctypes.data if len(d) else None, f.ctypes.data if len(f) else None, fi.ctypes.data,
                                                         pp.ctypes.data if len(pp) else None, len(t) - 1, len(d), len(pp))
            cap_pos = sum(len(pp) for _, pp in pkeep) if capacity_positions is None else int(capacity_positions)
            first, ppos = np.zeros(max(cap, 0) + 1, np.uint64), np.zeros(max(cap_pos, 1), np.uint32)
            st = _lib.load().vpt_postings_merge_positional(pred.handle, C.addressof(segs), len(keep), n_out, flags, term.ctypes.data, docs.ctypes.data,
                                                           tfs.ctypes.data, first.ctypes.data, cap, ppos.ctypes.data, cap_pos, C.byref(n_post),
                                                           C.byref(n_comb), C.byref(n_pos))
        else:
            segs = (_lib.PostingsSegment * max(len(keep), 1))()
            for k, (t, d, f) in enumerate(keep):
                segs[k] = _lib.PostingsSegment(t.ctypes.data, d.ctypes.data if len(d) else None, f.ctypes.data if len(f) else None, len(t) - 1, len(d))
            st = _lib.load().vpt_postings_merge(pred.handle, C.addressof(segs), len(keep), n_out, flags, term.ctypes.data, docs.ctypes.data,
                                                tfs.ctypes.data, cap, C.byref(n_post), C.byref(n_comb))
        if st != _lib.VPT_OK:
            try:
                _raise(st)
            except VaporettoError as e:
                e.n_postings = int(n_post.value)   # (too small a capacity: the numbers needed)
                e.n_positions = int(n_pos.value)
                raise
        n = int(n_post.value)
        out = Postings(term, docs[:n].copy(), tfs[:n].copy(), first[:n + 1].copy() if positions else None, None, sum(s.n_dropped for s in segments))
        if positions:
            out.positions = ppos[:int(n_pos.value)].copy()
        out.n_combined = int(n_comb.value)
        out._predictor = pred
        return out

    def search(self, queries: Sequence[Sequence[int]], k: int = 10, doc_lens=None, doc_base: Optional[int] = None, k1: float = 1.2, b: float = 0.75,
               weights=None, predictor: Optional["Predictor"] = None):
        """BM25 top-k of every query over this segment (vpt_postings_search; the definition is in include/vaporetto_hip.h).  queries: a sequence
        of term-id sequences, a slot per id, ids outside the vocabulary score nothing.  doc_lens / doc_base: the documents' lengths (default:
        what index_batch / index_batches attached).  weights: a sequence of float sequences shaped as queries (default: bm25_idf(n_documents,
        df[term]) per slot).  avgdl = float32(sum(doc_lens) / n_documents), in double.  Returns (hits, match_counts): hits[q] the list of
        (document, score float32) pairs, at most k, by score descending, then document ascending; match_counts uint64 [n_queries]."""
        return self._search("search", queries, None, k, doc_lens, doc_base, k1, b, weights, predictor)

    def boolean_search(self, queries, k: int = 10, doc_lens=None, doc_base: Optional[int] = None, k1: float = 1.2, b: float = 0.75,
                       predictor: Optional["Predictor"] = None):
        """BM25 top-k of every boolean query over this segment (vpt_postings_boolean_search; the definition is in include/vaporetto_hip.h).
        queries: a sequence of sequences of (term, occur) or (term, occur, weight), a slot each, occur an Occur.  A document matches when every
        MUST slot has it, no MUST_NOT slot has it and, without a MUST slot, some SHOULD slot has it; MUST and SHOULD slots that have it add to
        its score.  A slot without a weight gets bm25_idf(n_documents, df[term]), a MUST_NOT slot 0.0.  doc_lens / doc_base / avgdl / the
        return value: as in search.  last_search_counts: places, matches, skipped slots."""
        queries = [[tuple(x) for x in q] for q in queries]
        if any(len(x) not in (2, 3) for q in queries for x in q):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: boolean_search: a slot is (term, occur) or (term, occur, weight)")
        occurs = [[int(x[1]) for x in q] for q in queries]
        if any(not 0 <= o <= 255 for q in occurs for o in q):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: occurs: a value above 2")
        weights = [[(np.float32(0.0) if int(x[1]) == Occur.MUST_NOT else None) if len(x) == 2 else x[2] for x in q] for q in queries]
        return self._search("boolean_search", [[x[0] for x in q] for q in queries], occurs, k, doc_lens, doc_base, k1, b, weights, predictor)

    def _search(self, name, queries, occurs, k, doc_lens, doc_base, k1, b, weights, predictor):
        """search (occurs None) and boolean_search: the host call over this segment's arrays.  A weight of None: the slot's bm25_idf."""
        pred = predictor or self._predictor
        if pred is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: no predictor (pass predictor=)" % name)
        doc_lens = self.doc_lens if doc_lens is None else doc_lens
        doc_base = self.doc_base if doc_base is None else doc_base
        if doc_lens is None or doc_base is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: %s: the postings carry no doc_lens / doc_base (pass them)" % name)
        dl = np.ascontiguousarray(doc_lens, dtype=np.uint32)
        n_docs, n_terms, n_q = len(dl), len(self.term_offsets) - 1, len(queries)
        if n_q == 0:
            return [], np.zeros(0, np.uint64)
        if n_docs == 0:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: avgdl: must be between 2^-32 and 2^32")
        avgdl = np.float32(float(int(dl.sum(dtype=np.uint64))) / float(n_docs))
        qoff = np.zeros(n_q + 1, np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
        n_slots = int(qoff[-1])
        terms = np.array([t for q in queries for t in q] + [0], np.int64).astype(np.int32)
        if weights is None:
            df, idf = self.df(), {}
            w = np.zeros(n_slots + 1, np.float32)
            for s in range(n_slots):
                t = int(terms[s])
                if 0 <= t < n_terms:
                    if t not in idf:
                        idf[t] = bm25_idf(n_docs, int(df[t]))
                    w[s] = idf[t]
        else:
            flat = [x for q in weights for x in q] + [0]
            if len(flat) != n_slots + 1 or any(len(a) != len(c) for a, c in zip(weights, queries)):
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: weights: not shaped as the queries")
            if any(x is None for x in flat):
                df, idf = self.df(), {}
                for s, x in enumerate(flat):
                    if x is None:
                        t = int(terms[s])
                        if 0 <= t < n_terms and t not in idf:
                            idf[t] = bm25_idf(n_docs, int(df[t]))
                        flat[s] = idf.get(t, 0.0)
            w = np.array(flat, np.float32)
        if not (0 <= int(k) < 1 << 32 and 0 <= n_terms < 1 << 32 and 0 <= n_q < 1 << 32 and 0 <= int(doc_base) < 1 << 64):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: k: must be at least 1, and n_queries * k below 2^32")
        term = np.ascontiguousarray(self.term_offsets, dtype=np.uint64)
        docs, tfs = np.ascontiguousarray(self.docs, dtype=np.uint32), np.ascontiguousarray(self.tfs, dtype=np.uint32)
        n_out = max(n_q * int(k), 1)
        hd, hs, hc, mc, cnt = np.zeros(n_out, np.uint32), np.zeros(n_out, np.float32), np.zeros(n_q, np.uint32), np.zeros(n_q, np.uint64), np.zeros(3, np.uint64)
        head = (pred.handle, term.ctypes.data, docs.ctypes.data if len(docs) else None, tfs.ctypes.data if len(tfs) else None, n_terms, int(doc_base),
                n_docs, dl.ctypes.data, qoff.ctypes.data, terms.ctypes.data, w.ctypes.data)
        tail = (n_q, float(k1), float(b), float(avgdl), int(k), hd.ctypes.data, hs.ctypes.data, hc.ctypes.data, mc.ctypes.data, cnt.ctypes.data)
        if occurs is None:
            st = _lib.load().vpt_postings_search(*(head + tail))
        else:
            occ = np.array([o for q in occurs for o in q] + [0], np.uint8)
            st = _lib.load().vpt_postings_boolean_search(*(head + (occ.ctypes.data,) + tail))
        if st != _lib.VPT_OK:
            _raise(st)
        self.last_search_counts = cnt   # candidates (boolean_search: places), matches, skipped slots
        k = int(k)
        return [[(int(hd[q * k + j]), hs[q * k + j]) for j in range(int(hc[q]))] for q in range(n_q)], mc

    def phrase_search(self, phrases: Sequence[Sequence[int]], k: int = 10, doc_lens=None, doc_base: Optional[int] = None, k1: float = 1.2,
                      b: float = 0.75, weights=None, predictor: Optional["Predictor"] = None, slop=0):
        """Exact-phrase BM25 top-k of every phrase over this positional segment (vpt_postings_phrase_search; the definition is in
        include/vaporetto_hip.h).  phrases: a sequence of term-id sequences, each ONE phrase: its ids at consecutive positions, in order; an id
        outside the vocabulary makes the phrase match nothing.  weights: one float per phrase (default: tantivy's phrase weight, the float32
        sum in slot order of bm25_idf(n_documents, df[term]) over the slots).  doc_lens / doc_base / avgdl as in search.  Returns (hits,
        match_counts): hits[q] the list of (document, score float32, freq) triples, at most k, by score descending, then document
        ascending; freq the phrase's occurrences in the document.  slop: an int for every phrase or one int per phrase, each in [0, 31]:
        anything but the int 0 makes it the SLOPPY search (vpt_postings_sloppy_phrase_search; tantivy's set_slop, defined in the header)."""
        if self.first is None or self.positions is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: phrase_search: the postings were made without positions")
        slops = _slops_of(slop, len(phrases), "phrase")
        pred = predictor or self._predictor
        if pred is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: phrase_search: no predictor (pass predictor=)")
        doc_lens = self.doc_lens if doc_lens is None else doc_lens
        doc_base = self.doc_base if doc_base is None else doc_base
        if doc_lens is None or doc_base is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: phrase_search: the postings carry no doc_lens / doc_base (pass them)")
        dl = np.ascontiguousarray(doc_lens, dtype=np.uint32)
        n_docs, n_terms, n_q = len(dl), len(self.term_offsets) - 1, len(phrases)
        if n_q == 0:
            return [], np.zeros(0, np.uint64)
        if n_docs == 0:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: avgdl: must be between 2^-32 and 2^32")
        avgdl = np.float32(float(int(dl.sum(dtype=np.uint64))) / float(n_docs))
        qoff = np.zeros(n_q + 1, np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in phrases], dtype=np.uint64)
        terms = np.array([t for q in phrases for t in q] + [0], np.int64).astype(np.int32)
        if weights is None:
            df, idf = self.df(), {}
            w = np.zeros(n_q, np.float32)
            for i, q in enumerate(phrases):
                total = None
                for t in q:
                    t = int(t)
                    if not 0 <= t < n_terms:
                        continue
                    if t not in idf:
                        idf[t] = bm25_idf(n_docs, int(df[t]))
                    total = idf[t] if total is None else np.float32(total + idf[t])
                w[i] = np.float32(0) if total is None else total
        else:
            w = np.array(list(weights), np.float32)
            if len(w) != n_q:
                raise VaporettoError("InvalidArgument", "InvalidArgumentError: weights: one per phrase")
        if not (0 <= int(k) < 1 << 32 and 0 <= n_terms < 1 << 32 and 0 <= n_q < 1 << 32 and 0 <= int(doc_base) < 1 << 64):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: k: must be at least 1, and n_queries * k below 2^32")
        term = np.ascontiguousarray(self.term_offsets, dtype=np.uint64)
        docs, tfs = np.ascontiguousarray(self.docs, dtype=np.uint32), np.ascontiguousarray(self.tfs, dtype=np.uint32)
        first, ppos = np.ascontiguousarray(self.first, dtype=np.uint64), np.ascontiguousarray(self.positions, dtype=np.uint32)
        if len(docs) != len(tfs) or len(first) != len(docs) + 1 or int(term[-1]) != len(docs) or int(first[-1]) != len(ppos):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: phrase_search: the postings' arrays do not belong together")
        n_out = max(n_q * int(k), 1)
        hd, hs, hf = np.zeros(n_out, np.uint32), np.zeros(n_out, np.float32), np.zeros(n_out, np.uint32)
        hc, mc, cnt = np.zeros(n_q, np.uint32), np.zeros(n_q, np.uint64), np.zeros(3, np.uint64)
        head = (pred.handle, term.ctypes.data, docs.ctypes.data if len(docs) else None, tfs.ctypes.data if len(tfs) else None, first.ctypes.data,
                ppos.ctypes.data if len(ppos) else None, n_terms, int(doc_base), n_docs, dl.ctypes.data, qoff.ctypes.data, terms.ctypes.data, w.ctypes.data)
        tail = (n_q, float(k1), float(b), float(avgdl), int(k), hd.ctypes.data, hs.ctypes.data, hf.ctypes.data, hc.ctypes.data, mc.ctypes.data,
                cnt.ctypes.data)
        if slops is None:
            st = _lib.load().vpt_postings_phrase_search(*(head + tail))
        else:
            st = _lib.load().vpt_postings_sloppy_phrase_search(*(head + (slops.ctypes.data,) + tail))
        if st != _lib.VPT_OK:
            _raise(st)
        self.last_search_counts = cnt   # probes, matches, skipped queries
        k = int(k)
        return [[(int(hd[q * k + j]), hs[q * k + j], int(hf[q * k + j])) for j in range(int(hc[q]))] for q in range(n_q)], mc

    def clause_search(self, queries, k: int = 10, doc_lens=None, doc_base: Optional[int] = None, k1: float = 1.2, b: float = 0.75,
                      predictor: Optional["Predictor"] = None, slop: int = 0):
        """BM25 top-k of every boolean query of CLAUSES over this positional segment (vpt_postings_clause_search; the definition is in
        include/vaporetto_hip.h).  A query is a sequence of clauses (terms, occur) or (terms, occur, weight): terms a sequence of term ids.  A
        clause of one term is a slot of that term, as in boolean_search; every other clause is ONE exact phrase, scored by its phrase
        frequency (an id outside the vocabulary makes it match nothing, and so does an empty clause).  The default weight is the phrase weight
        of phrase_search (the float32 sum in slot order of bm25_idf over the clause's terms), 0.0 for MUST_NOT.  Returns (hits, match_counts)
        as boolean_search does; last_search_counts: places, matches, skipped clauses.  slop: an int in [0, 31] for every phrase clause
        (phrase_search's; anything but 0: vpt_postings_sloppy_clause_search).  Clauses have no syntax for it."""
        if self.first is None or self.positions is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: clause_search: the postings were made without positions")
        pred = predictor or self._predictor
        if pred is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: clause_search: no predictor (pass predictor=)")
        doc_lens = self.doc_lens if doc_lens is None else doc_lens
        doc_base = self.doc_base if doc_base is None else doc_base
        if doc_lens is None or doc_base is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: clause_search: the postings carry no doc_lens / doc_base (pass them)")
        queries = [list(q) for q in queries]
        flat = [x for q in queries for x in q]
        if any(len(x) not in (2, 3) for x in flat):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: clause_search: a clause is (terms, occur) or (terms, occur, weight)")
        if any(not 0 <= int(x[1]) <= 2 for x in flat):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: occurs: a value above 2")
        dl = np.ascontiguousarray(doc_lens, dtype=np.uint32)
        n_docs, n_terms, n_q = len(dl), len(self.term_offsets) - 1, len(queries)
        if n_q == 0:
            return [], np.zeros(0, np.uint64)
        if n_docs == 0:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: avgdl: must be between 2^-32 and 2^32")
        avgdl = np.float32(float(int(dl.sum(dtype=np.uint64))) / float(n_docs))
        qoff = np.zeros(n_q + 1, np.uint64)
        qoff[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
        coff = np.zeros(len(flat) + 1, np.uint64)
        coff[1:] = np.cumsum([len(x[0]) for x in flat], dtype=np.uint64)
        terms = np.array([t for x in flat for t in x[0]] + [0], np.int64).astype(np.int32)
        occ = np.array([int(x[1]) for x in flat] + [0], np.uint8)
        w = np.zeros(len(flat) + 1, np.float32)
        df, idf = None, {}
        for c, x in enumerate(flat):
            if len(x) == 3:
                w[c] = x[2]
            elif int(x[1]) != Occur.MUST_NOT:
                total = None
                for t in x[0]:
                    t = int(t)
                    if not 0 <= t < n_terms:
                        continue
                    if t not in idf:
                        df = self.df() if df is None else df
                        idf[t] = bm25_idf(n_docs, int(df[t]))
                    total = idf[t] if total is None else np.float32(total + idf[t])
                w[c] = np.float32(0) if total is None else total
        if not (0 <= int(k) < 1 << 32 and 0 <= n_terms < 1 << 32 and 0 <= n_q < 1 << 32 and 0 <= int(doc_base) < 1 << 64):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: k: must be at least 1, and n_queries * k below 2^32")
        term = np.ascontiguousarray(self.term_offsets, dtype=np.uint64)
        docs, tfs = np.ascontiguousarray(self.docs, dtype=np.uint32), np.ascontiguousarray(self.tfs, dtype=np.uint32)
        first, ppos = np.ascontiguousarray(self.first, dtype=np.uint64), np.ascontiguousarray(self.positions, dtype=np.uint32)
        if len(docs) != len(tfs) or len(first) != len(docs) + 1 or int(term[-1]) != len(docs) or int(first[-1]) != len(ppos):
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: clause_search: the postings' arrays do not belong together")
        n_out = max(n_q * int(k), 1)
        hd, hs, hc, mc, cnt = np.zeros(n_out, np.uint32), np.zeros(n_out, np.float32), np.zeros(n_q, np.uint32), np.zeros(n_q, np.uint64), np.zeros(3, np.uint64)
        head = (pred.handle, term.ctypes.data, docs.ctypes.data if len(docs) else None, tfs.ctypes.data if len(tfs) else None, first.ctypes.data,
                ppos.ctypes.data if len(ppos) else None, n_terms, int(doc_base), n_docs, dl.ctypes.data, qoff.ctypes.data, coff.ctypes.data,
                terms.ctypes.data, w.ctypes.data, occ.ctypes.data)
        tail = (n_q, float(k1), float(b), float(avgdl), int(k), hd.ctypes.data, hs.ctypes.data, hc.ctypes.data, mc.ctypes.data, cnt.ctypes.data)
        slops = _slops_of(int(slop), len(flat) + 1, "clause")
        if slops is None:
            st = _lib.load().vpt_postings_clause_search(*(head + tail))
        else:
            st = _lib.load().vpt_postings_sloppy_clause_search(*(head + (slops.ctypes.data,) + tail))
        if st != _lib.VPT_OK:
            _raise(st)
        self.last_search_counts = cnt   # places, matches, skipped clauses
        k = int(k)
        return [[(int(hd[q * k + j]), hs[q * k + j]) for j in range(int(hc[q]))] for q in range(n_q)], mc

    def tokens(self, q: int) -> np.ndarray:
        """the token indices of posting q, ascending (needs positions)"""
        if self.first is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: tokens: the postings were made without positions")
        return self.order[int(self.first[q]):int(self.first[q + 1])]


class TaggedToken(TantivyToken):
    """A token of the tagged stream: TantivyToken plus `tags`, a tuple of Optional[str] per slot.  Under a stop filter `position` is the index
    before filtering and `position_length` the count before filtering."""

    def __init__(self, text, offset_from, offset_to, position, position_length, tags):
        super().__init__(text, offset_from, offset_to, position, position_length)
        self.tags = tuple(tags)

    def __eq__(self, other):
        return isinstance(other, TaggedToken) and self._key() == other._key() and self.tags == other.tags

    def __repr__(self):
        return super().__repr__()[:-1] + ", tags=%r)" % (self.tags,)


class VaporettoTokenizer:
    """vaporetto_tantivy's VaporettoTokenizer (vaporetto_tantivy/src/lib.rs:62-229) over the C ABI: KyteaFullwidthFilter always, Predictor::new(model,
    false), SplitLinebreaksFilter first, then one filter per char of `wsconst` (D R H T K O: KyteaWsConstFilter; G: ConcatGraphemeClustersFilter).
    A batch is ONE call (vpt_token_stream_batch: only the text goes to the device, the spans come back), "G" included: the device applies it
    last, which is the adapter's result for any place of "G" in the string."""

    def __init__(self, model: Model, wsconst: str = "", device: int = 0, _predictor: Optional[Predictor] = None, predict_tags: bool = False,
                 tagger: Optional["PatternMatchTagger"] = None, stop_tags=None, vocab=None, vocab_normalize: bool = True):
        """predict_tags (beyond the adapter, which predicts none): the tokens are TaggedToken, with `tagger`'s rule tags behind the tag models'
        and without the tokens of `stop_tags` ((slot, tag string) pairs).  Without it the class is the adapter's.
        vocab (a Vocabulary of this tokenizer's predictor, or a sequence of surfaces; also beyond the adapter): every token carries `.id`, its
        entry in the vocabulary or the vocabulary's unk_id, looked up on the device -- with vocab_normalize on the KyteaFullwidthFilter image of
        the token (the text as it was scored), else on the caller's bytes; encode_batch returns the ids alone."""
        self._flags = wsconst_flags(wsconst, allow_graphemes=True)
        self._wsconst = wsconst
        self._predictor = _predictor if _predictor is not None else Predictor(model, bool(predict_tags), device=device)
        if (tagger is not None or stop_tags is not None) and not predict_tags:
            raise VaporettoError("InvalidArgumentError: tagger / stop_tags: need predict_tags = True")
        self._tagged, self._tagger = bool(predict_tags), tagger
        self._stop = TagStopFilter(self._predictor, stop_tags, tagger) if stop_tags is not None else None
        self._vocab = vocab if vocab is None or isinstance(vocab, Vocabulary) else Vocabulary(self._predictor, vocab)
        self._vocab_normalize = bool(vocab_normalize)

    @classmethod
    def deserialize(cls, blob, wsconst: str = "", device: int = 0, predict_tags: bool = False, tagger: Optional["PatternMatchTagger"] = None,
                    stop_tags=None, vocab=None, vocab_normalize: bool = True) -> "VaporettoTokenizer":
        """lib.rs:121-146, from Predictor.save_compiled's bytes (vpt_predictor_load); predict_tags needs bytes of a predictor made with it."""
        wsconst_flags(wsconst, allow_graphemes=True)
        return cls(None, wsconst, device, _predictor=Predictor.load_compiled(blob, device=device), predict_tags=predict_tags, tagger=tagger,
                   stop_tags=stop_tags, vocab=vocab, vocab_normalize=vocab_normalize)

    @property
    def predictor(self) -> Predictor:
        return self._predictor

    def token_spans(self, texts: Sequence[str]):
        """(utf8, byte_offsets, token_offsets, token_ends) of a batch of documents."""
        raws = [t.encode("utf-8") for t in texts]
        utf8, boff = pack_texts(raws)
        toff, ends = self._predictor.token_stream_packed(utf8, boff, self._wsconst)
        return utf8, boff, toff, ends

    def token_stream_batch(self, texts: Sequence[str]) -> List[List[TantivyToken]]:
        if not texts:
            return []
        if self._tagged:
            return self._tagged_batch(texts)
        if self._vocab is not None:
            return self._ids_batch(texts)
        utf8, boff, toff, ends = self.token_spans(texts)
        out = []
        for i, _ in enumerate(texts):
            raw = bytes(utf8[int(boff[i]):int(boff[i + 1])])
            e = [int(x) for x in ends[int(toff[i]):int(toff[i + 1])]]
            toks, start = [], 0
            for k, end in enumerate(e):
                toks.append(TantivyToken(raw[start:end].decode("utf-8"), start, end, k, len(e)))
                start = end
            out.append(toks)
        return out

    def _stream_ids(self, utf8, boff):
        return self._predictor.token_ids_packed(utf8, boff, self._vocab, self._wsconst, self._vocab_normalize, self._tagger, self._stop,
                                                tags=self._tagged)

    def encode_batch(self, texts: Sequence[str]):
        """(token_offsets uint64 [n + 1], ids int32) of a batch of documents: the stream's vocabulary ids and nothing else -- no token string is
        built on the way (vpt_token_stream_ids_batch).  Needs vocab=."""
        if self._vocab is None:
            raise VaporettoError("InvalidArgumentError: encode_batch: the tokenizer has no vocab")
        utf8, boff = pack_texts([t.encode("utf-8") for t in texts])
        out = self._stream_ids(utf8, boff)
        return out[0], out[5]

    def set_vocab(self, vocab: Optional["Vocabulary"]) -> None:
        """The vocabulary of `.id` and encode_batch from here on (one of this tokenizer's predictor, as build_vocab returns), or None."""
        self._vocab = vocab

    def count_batch(self, texts: Sequence[str], counter: "VocabularyCounter") -> None:
        """Every token this tokenizer streams for `texts` (tagger and stop set included) into `counter`, on the device
        (vpt_token_stream_count_batch); the surface is the one encode_batch looks up (vocab_normalize).  No token string is built."""
        utf8, boff = pack_texts([t.encode("utf-8") for t in texts])
        self._predictor.count_tokens_packed(utf8, boff, counter, self._wsconst, self._vocab_normalize, self._tagger, self._stop)

    def build_vocab(self, batches, min_count: int = 1, max_size: Optional[int] = None, specials=(), unk_id: int = -1,
                    max_keys: int = 1 << 20) -> "Vocabulary":
        """corpus -> Vocabulary without a token string leaving the device before the vocabulary itself is read out.  batches: an iterable of
        lists of str, each counted with count_batch into one VocabularyCounter(max_keys).  The specials get ids 0.. in the order given (and
        leave the counted list if they occur in it); the ids behind them follow the counter's finish order -- count descending, then code
        points ascending -- over the surfaces of count >= min_count, at most max_size of them (None: all)."""
        counter = VocabularyCounter(self._predictor, max_keys)
        for texts in batches:
            self.count_batch(list(texts), counter)
        surfaces, _counts = counter.finish(min_count, max_size)
        specials = list(specials)
        taken = set(specials)
        return Vocabulary(self._predictor, specials + [s for s in surfaces if s not in taken], unk_id)

    def index_batch(self, texts: Sequence[str], doc_base: int = 0, positions: bool = False) -> "Postings":
        """The postings of a batch of documents (a segment) over this tokenizer's vocabulary: term = vocabulary id, document = doc_base + the
        text's index, tf = the term's tokens in it (vpt_token_stream_postings_batch; tagger and stop set included).  A token whose id is no
        entry (unk_id outside the vocabulary) is counted in n_dropped.  positions: a positional segment (`first`, `positions`: the stream's
        token positions, with the gaps a stop set leaves), what phrase_search reads.  Needs vocab=."""
        if self._vocab is None:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: index_batch: the tokenizer has no vocab")
        utf8, boff = pack_texts([t.encode("utf-8") for t in texts])
        out = self._predictor.token_postings_packed(utf8, boff, self._vocab, self._wsconst, self._vocab_normalize, self._tagger, self._stop, doc_base,
                                                    positions=positions)
        # what Postings.search needs of the documents: their token counts (the stream's tokens, those without a vocabulary entry included)
        out.doc_lens = np.diff(self._stream_ids(utf8, boff)[0]).astype(np.uint32) if len(texts) else np.zeros(0, np.uint32)
        out.doc_base = int(doc_base)
        return out

    def index_batches(self, batches: Iterable[Sequence[str]], doc_base: int = 0, ordered: bool = True, positions: bool = False) -> "Postings":
        """The postings of a corpus given as batches of documents: every batch is indexed as a segment (index_batch) with a running doc_base,
        and the segments are merged on the device (Postings.merge; ordered: the running doc_bases keep the promise of the ordered route).
        Equal to index_batch of the concatenation.  positions: positional segments, merged with their position lists -- equal to
        index_batch(concatenation, positions=True), and phrase_search runs on it.  No batch: the empty postings over the vocabulary."""
        segments, base = [], int(doc_base)
        for texts in batches:
            texts = list(texts)
            segments.append(self.index_batch(texts, base, positions=positions))
            base += len(texts)
        if not segments:
            return self.index_batch([], base, positions=positions)
        out = Postings.merge(segments, ordered=ordered, predictor=self._predictor, positions=positions)
        out.doc_lens, out.doc_base = np.concatenate([s.doc_lens for s in segments]), int(doc_base)   # (the running doc_bases are contiguous)
        return out

    def search(self, postings: "Postings", texts: Sequence[str], k: int = 10, doc_lens=None, doc_base: Optional[int] = None, k1: float = 1.2,
               b: float = 0.75, weights=None):
        """BM25 top-k of query TEXTS over `postings`: the texts are tokenised and encoded as documents are (encode_batch), every token a slot --
        nothing is dropped, a token without a vocabulary entry is a slot that scores nothing -- then Postings.search.  Needs vocab=."""
        toff, ids = self.encode_batch(list(texts))
        queries = [ids[int(toff[i]):int(toff[i + 1])].tolist() for i in range(len(toff) - 1)]
        return postings.search(queries, k, doc_lens, doc_base, k1, b, weights, predictor=self._predictor)

    def boolean_search(self, postings: "Postings", texts: Sequence[str], k: int = 10, doc_lens=None, doc_base: Optional[int] = None, k1: float = 1.2,
                       b: float = 0.75, phrases: bool = False, slop: int = 0):
        """BM25 top-k of boolean query TEXTS over `postings`.  A text is split on ASCII spaces into CLAUSES: one that starts with `+` is MUST,
        one that starts with `-` is MUST_NOT, any other is SHOULD; the rest of the clause is tokenised and encoded as documents are; an empty
        clause adds nothing.  By default every token of a clause is a slot of the clause's occur: `+東京都` requires each of its tokens
        somewhere in the document; then Postings.boolean_search.  phrases=True (what tantivy's query parser does; `postings` from
        index_batch(positions=True)): a clause of several tokens is ONE exact phrase -- a token without a vocabulary entry makes it match
        nothing -- a clause of one token a term slot, and a clause that yields no token (a stop set took them all) adds nothing, as in the
        default; then Postings.clause_search.  slop (with phrases=True): the slop of every phrase clause; a `~` in a text stays a character
        of its clause.  Needs vocab=."""
        clauses, owner = [], []
        for i, text in enumerate(texts):
            for clause in text.split(" "):
                occur = Occur.MUST if clause[:1] == "+" else Occur.MUST_NOT if clause[:1] == "-" else Occur.SHOULD
                body = clause[1:] if occur != Occur.SHOULD else clause
                if body:
                    clauses.append(body)
                    owner.append((i, occur))
        queries = [[] for _ in texts]
        if clauses:
            toff, ids = self.encode_batch(clauses)
            for c, (i, occur) in enumerate(owner):
                if phrases and toff[c] == toff[c + 1]:
                    continue
                if phrases:
                    queries[i].append((ids[int(toff[c]):int(toff[c + 1])].tolist(), occur))
                else:
                    queries[i] += [(int(t), occur) for t in ids[int(toff[c]):int(toff[c + 1])]]
        if phrases:
            return postings.clause_search(queries, k, doc_lens, doc_base, k1, b, predictor=self._predictor, slop=slop)
        if slop:
            raise VaporettoError("InvalidArgument", "InvalidArgumentError: boolean_search: slop needs phrases=True")
        return postings.boolean_search(queries, k, doc_lens, doc_base, k1, b, predictor=self._predictor)

    def phrase_search(self, postings: "Postings", texts: Sequence[str], k: int = 10, doc_lens=None, doc_base: Optional[int] = None, k1: float = 1.2,
                      b: float = 0.75, weights=None, slop=0):
        """Exact-phrase BM25 top-k of query TEXTS over `postings` (index_batch(positions=True)): each text is tokenised and encoded as documents
        are and is ONE phrase, every token a slot -- a token without a vocabulary entry makes it match nothing -- then Postings.phrase_search
        (slop: its keyword).  Needs vocab=."""
        toff, ids = self.encode_batch(list(texts))
        phrases = [ids[int(toff[i]):int(toff[i + 1])].tolist() for i in range(len(toff) - 1)]
        return postings.phrase_search(phrases, k, doc_lens, doc_base, k1, b, weights, predictor=self._predictor, slop=slop)

    def _ids_batch(self, texts: Sequence[str]) -> List[List[TantivyToken]]:
        utf8, boff = pack_texts([t.encode("utf-8") for t in texts])
        toff, starts, ends, pos, _, ids = self._stream_ids(utf8, boff)
        out = []
        for i, _t in enumerate(texts):
            raw = bytes(utf8[int(boff[i]):int(boff[i + 1])])
            a, b = int(toff[i]), int(toff[i + 1])
            toks = []
            for k in range(a, b):
                tok = TantivyToken(raw[int(starts[k]):int(ends[k])].decode("utf-8"), int(starts[k]), int(ends[k]), int(pos[k]), b - a)
                tok.id = int(ids[k])
                toks.append(tok)
            out.append(toks)
        return out

    def _tagged_batch(self, texts: Sequence[str]) -> List[List["TaggedToken"]]:
        p = self._predictor
        utf8, boff = pack_texts([t.encode("utf-8") for t in texts])
        ids = None
        if self._vocab is not None:
            toff, starts, ends, pos, tags, ids = self._stream_ids(utf8, boff)
        else:
            toff, starts, ends, pos, tags = p.token_stream_tagged_packed(utf8, boff, self._wsconst, self._tagger, self._stop)
        # position_length is the count before filtering, which the filtered arrays no longer hold: under a stop filter the UNTAGGED stream
        # (vpt_token_stream_batch: scoring and spans a second time, no fill_tags, no tags) gives it.  Callers that do not need
        # position_length take token_stream_tagged_packed, which is one pass.
        full = toff if self._stop is None else p.token_stream_packed(utf8, boff, self._wsconst)[0]
        vocab = p.tag_strings()
        rule = [self._tagger.tag(p, k) for k in range(self._tagger.n_tags(p))] if self._tagger is not None and tags.shape[1] else []
        out = []
        for i, _ in enumerate(texts):
            raw = bytes(utf8[int(boff[i]):int(boff[i + 1])])
            n = int(full[i + 1]) - int(full[i])
            out.append([TaggedToken(raw[int(starts[k]):int(ends[k])].decode("utf-8"), int(starts[k]), int(ends[k]), int(pos[k]), n,
                                    [None if v == -1 else vocab[v] if v >= 0 else rule[-2 - v] for v in (int(x) for x in tags[k])])
                        for k in range(int(toff[i]), int(toff[i + 1]))])
            if ids is not None:
                for tok, k in zip(out[-1], range(int(toff[i]), int(toff[i + 1]))):
                    tok.id = int(ids[k])
        return out

    def token_stream(self, text: str) -> List[TantivyToken]:
        return self.token_stream_batch([text])[0]


def pack_texts(raws: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    boff = np.zeros(len(raws) + 1, dtype=np.uint64)
    boff[1:] = np.cumsum([len(r) for r in raws], dtype=np.uint64)
    return np.frombuffer(b"".join(raws), dtype=np.uint8), boff


def count_boundaries(utf8: np.ndarray, byte_offsets: np.ndarray) -> np.ndarray:
    utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
    byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
    S = len(byte_offsets) - 1
    ooff = np.zeros(S + 1, dtype=np.uint64)
    st = _lib.load().vpt_count_boundaries(utf8.ctypes.data, byte_offsets.ctypes.data, S, ooff.ctypes.data)
    if st != _lib.VPT_OK:
        _raise(st)
    return ooff


def model_inspect(model_bytes: bytes, predict_tags: bool = False) -> dict:
    mi = _lib.ModelInfo()
    st = _lib.load().vpt_model_inspect(model_bytes, len(model_bytes), int(predict_tags), C.byref(mi))
    if st != _lib.VPT_OK:
        _raise(st)
    return mi.as_dict()


class SolverType(enum.IntEnum):  # trainer.rs:20-45; the primal TRON solvers 0 and 2 and, on a Trainer(l1r=True), solver 5, on a Trainer(l1r_lr=True), solver 6 are implemented
    L2RegularizedLogistic = 0
    L2RegularizedL2LossSVCDual = 1
    L2RegularizedL2LossSVC = 2
    L2RegularizedL1LossSVCDual = 3
    CrammerSingerSVC = 4
    L1RegularizedL2LossSVC = 5
    L1RegularizedLogistic = 6
    L2RegularizedLogisticDual = 7


class Trainer:
    """Trainer (trainer.rs:201-490), on the device (vpt_trainer_*).  By default only the boundary model is trained: a sentence that
    carries a tag is an error unless `ignore_tags` is set, which drops the tags (the train CLI's --ignore-tags) and writes a model
    without tag models.  With `train_tags=True` the tags are kept and the tag models are trained too (tag_trainer.rs);
    `tag_dictionary` is then the reference's tag dictionary: tagged Sentences, or (surface, tags) pairs, whose first occurrence of a
    surface gives the tags of a surface the corpus does not contain.  With `l1r=True` (VPT_TRAIN_L1R) train also accepts
    SolverType.L1RegularizedL2LossSVC, the solver the reference's README trains with: most weights end at exactly 0 and are not written.
    Solvers 0 and 2 train as without it; tag models are not trained with solver 5 unless `l1r_tags=True` (VPT_TRAIN_TAGS_L1R, which
    needs both `l1r` and `train_tags`): then solver 5 trains every tag problem by the same coordinate descent, one-vs-rest, and the tag
    models are sparse too; tag_stats() then carries sweeps and halvings as last_stats() does.  With `l1r_lr=True` (VPT_TRAIN_L1R_LR,
    alone or beside any of the above) train also accepts SolverType.L1RegularizedLogistic: liblinear's newGLMNET on the device, a sparse
    boundary model with the logistic loss; last_stats() then carries Newton iterations and inner sweeps.  Tag models are not trained
    with solver 6 -- with `train_tags` it is refused -- unless `l1r_lr_tags=True` (VPT_TRAIN_TAGS_L1R_LR, which needs both `l1r_lr` and
    `train_tags`): then solver 6 trains every tag problem by the same newGLMNET, one-vs-rest, the tag models are sparse and their
    scores are log-odds; tag_stats() then carries Newton iterations and inner sweeps."""

    def __init__(self, charw: int, charn: int, typew: int, typen: int, dict_words: Sequence[str] = (), dictn: int = 0, device: int = 0,
                 ignore_tags: bool = False, train_tags: bool = False, tag_dictionary: Sequence = (), l1r: bool = False,
                 l1r_tags: bool = False, l1r_lr: bool = False, l1r_lr_tags: bool = False):
        if l1r_tags and not (l1r and train_tags):
            raise ValueError("l1r_tags needs l1r=True and train_tags=True")
        if l1r_lr_tags and not (l1r_lr and train_tags):
            raise ValueError("l1r_lr_tags needs l1r_lr=True and train_tags=True")
        if ignore_tags and train_tags:
            raise ValueError("ignore_tags and train_tags exclude each other")
        if tag_dictionary and not train_tags:
            raise ValueError("tag_dictionary needs train_tags=True")
        self.ignore_tags = bool(ignore_tags)
        self.train_tags = bool(train_tags)
        self._L = _lib.load()
        self._h = C.c_void_p()
        self._charw, self._typew = charw, typew
        self.dict_words = list(dict_words)
        self.l1r = bool(l1r)
        self.l1r_tags = bool(l1r_tags)
        self.l1r_lr = bool(l1r_lr)
        self.l1r_lr_tags = bool(l1r_lr_tags)
        prm = _lib.TrainParams(charw, charn, typew, typen, dictn, (_lib.VPT_TRAIN_TAGS if train_tags else 0) | (_lib.VPT_TRAIN_L1R if l1r else 0) |
                               (_lib.VPT_TRAIN_TAGS_L1R if l1r_tags else 0) | (_lib.VPT_TRAIN_L1R_LR if l1r_lr else 0) |
                               (_lib.VPT_TRAIN_TAGS_L1R_LR if l1r_lr_tags else 0))
        utf8, off = pack_texts([w.encode("utf-8") for w in self.dict_words])
        st = self._L.vpt_trainer_create(C.addressof(prm), utf8.ctypes.data, off.ctypes.data, len(self.dict_words), device, C.byref(self._h))
        if st != _lib.VPT_OK:
            self._h = None
            _raise(st)
        if tag_dictionary:
            self.set_tag_dictionary(tag_dictionary)

    def set_tag_dictionary(self, entries: Sequence) -> None:
        """trainer.rs:231-238: per token of the entries (Sentences, or (surface, [tag or None, ...]) pairs) its tags; the first occurrence wins."""
        pairs = []
        for e in entries:
            if isinstance(e, Sentence):
                pairs += [(tk.surface(), tk.tags()) for tk in e.tokens()]
            else:
                pairs.append((e[0], list(e[1])))
        surf, soff = pack_texts([p[0].encode("utf-8") for p in pairs])
        nt = np.array([len(p[1]) for p in pairs] + [0], np.uint32)
        tb, so = pack_texts([(t or "").encode("utf-8") for p in pairs for t in p[1]])
        tb = np.concatenate([tb, np.zeros(1, np.uint8)])
        surf = np.concatenate([surf, np.zeros(1, np.uint8)])
        st = self._L.vpt_trainer_set_tag_dictionary(self._h, surf.ctypes.data, soff.ctypes.data, len(pairs), nt.ctypes.data, so.ctypes.data, tb.ctypes.data)
        if st != _lib.VPT_OK:
            _raise(st)

    def add_packed_tagged(self, utf8: np.ndarray, byte_offsets: np.ndarray, labels: np.ndarray, n_tags: np.ndarray, tag_index: np.ndarray,
                          span_offsets: np.ndarray, tag_bytes: np.ndarray, fullwidth: bool = False) -> None:
        """The raw text, labels and tags as parse_tokenized_host returns them (vpt_trainer_add_tagged_batch); needs train_tags=True."""
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        n_tags = np.ascontiguousarray(n_tags, dtype=np.uint32)
        tag_index = np.ascontiguousarray(tag_index, dtype=np.uint64)
        span_offsets = np.ascontiguousarray(span_offsets, dtype=np.uint64)
        tag_bytes = np.ascontiguousarray(tag_bytes, dtype=np.uint8)
        S = len(byte_offsets) - 1
        if len(n_tags) != S or len(span_offsets) < 1:
            raise ValueError("n_tags needs an entry per sentence and span_offsets at least one entry")
        n_chars = S + len(labels)
        if len(tag_index) != n_chars + 1:
            raise ValueError("tag_index needs an entry per char and one more")
        tb = tag_bytes if len(tag_bytes) else np.zeros(1, np.uint8)
        st = self._L.vpt_trainer_add_tagged_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, S, labels.ctypes.data, n_tags.ctypes.data,
                                                  tag_index.ctypes.data, span_offsets.ctypes.data, tb.ctypes.data, len(span_offsets) - 1,
                                                  len(tag_bytes), _lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0)
        if st != _lib.VPT_OK:
            _raise(st)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.vpt_trainer_destroy(self._h)
            self._h = None

    def add_packed(self, utf8: np.ndarray, byte_offsets: np.ndarray, labels: np.ndarray, fullwidth: bool = False) -> None:
        utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
        byte_offsets = np.ascontiguousarray(byte_offsets, dtype=np.uint64)
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        st = self._L.vpt_trainer_add_batch(self._h, utf8.ctypes.data, byte_offsets.ctypes.data, len(byte_offsets) - 1, labels.ctypes.data,
                                           _lib.VPT_FLAG_KYTEA_FULLWIDTH if fullwidth else 0)
        if st != _lib.VPT_OK:
            _raise(st)

    def add_device(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int, d_labels: int, flags: int = 0,
                   stream: int = 0) -> None:
        """Device-resident add_packed (vpt_trainer_add_batch_device): all pointers are raw device addresses, e.g. the raw text, raw offsets,
        out_offsets and labels vpt_parse_tokenized_batch_device wrote; the examples are appended after `stream`'s work so far.
        total_boundaries is exact, out_offsets[n_sentences]; d_labels may be 0 (NULL) when it is 0."""
        st = self._L.vpt_trainer_add_batch_device(self._h, d_utf8 or None, d_boff or None, d_ooff or None, n_sentences, total_boundaries,
                                                  d_labels or None, flags, stream or None)
        if st != _lib.VPT_OK:
            _raise(st)

    def add_tagged_device(self, d_utf8: int, d_boff: int, d_ooff: int, n_sentences: int, total_boundaries: int, d_labels: int, d_n_tags: int,
                          d_tag_index: int, d_span_offsets: int, d_tag_bytes: int, n_spans: int, n_tag_bytes: int, flags: int = 0,
                          stream: int = 0) -> None:
        """Device-resident add_packed_tagged (vpt_trainer_add_tagged_batch_device) on the arrays either device parser wrote; needs
        train_tags=True."""
        st = self._L.vpt_trainer_add_tagged_batch_device(self._h, d_utf8 or None, d_boff or None, d_ooff or None, n_sentences, total_boundaries,
                                                         d_labels or None, d_n_tags or None, d_tag_index or None, d_span_offsets or None,
                                                         d_tag_bytes or None, n_spans, n_tag_bytes, flags, stream or None)
        if st != _lib.VPT_OK:
            _raise(st)

    def add_examples(self, sentences: Sequence["Sentence"], fullwidth: bool = False) -> None:
        if not sentences:
            return
        if not self.ignore_tags and not self.train_tags:
            for i, s in enumerate(sentences):
                if any(t is not None for t in s.tags()):
                    raise VaporettoError("InvalidArgument", "InvalidArgumentError: sentence %d: carries tags; tag models are not trained "
                                         "(ignore_tags=True drops them, train_tags=True trains them)" % i)
        utf8, boff = pack_texts([s.as_raw_text().encode("utf-8") for s in sentences])
        labels = np.concatenate([np.asarray(s.boundaries(), dtype=np.uint8) for s in sentences])
        if not self.train_tags:
            self.add_packed(utf8, boff, labels, fullwidth=fullwidth)
            return
        # the parser's CSR from Sentence.tags(): per char its slots up to the last Some, a None among them an empty span
        n_tags, tindex, spans = [], [0], []
        for s in sentences:
            nt, tags = s.n_tags(), s.tags()
            n_tags.append(nt)
            for c in range(len(s)):
                row = list(tags[c * nt:(c + 1) * nt])
                while row and row[-1] is None:
                    row.pop()
                spans += [(t or "").encode("utf-8") for t in row]
                tindex.append(len(spans))
        tb, so = pack_texts(spans)
        self.add_packed_tagged(utf8, boff, labels, np.array(n_tags, np.uint32), np.array(tindex, np.uint64), so, tb, fullwidth=fullwidth)

    def add_example(self, sentence: "Sentence") -> None:  # trainer.rs:321-350
        self.add_examples([sentence])

    def n_features(self) -> int:  # trainer.rs:489
        n = C.c_size_t()
        st = self._L.vpt_trainer_n_features(self._h, C.byref(n))
        if st != _lib.VPT_OK:
            _raise(st)
        return n.value

    def csr(self):
        """(row_ptr, cols, counts) of the design matrix: rows = boundaries in corpus order, columns = features in key order."""
        nr, nz = C.c_size_t(), C.c_size_t()
        st = self._L.vpt_trainer_csr(self._h, None, None, None, 0, C.byref(nr), C.byref(nz))
        if st != _lib.VPT_OK:
            _raise(st)
        ptr = np.zeros(nr.value + 1, np.uint64)
        cols = np.zeros(max(nz.value, 1), np.uint32)
        cnt = np.zeros(max(nz.value, 1), np.uint16)
        st = self._L.vpt_trainer_csr(self._h, ptr.ctypes.data, cols.ctypes.data, cnt.ctypes.data, len(cols), C.byref(nr), C.byref(nz))
        if st != _lib.VPT_OK:
            _raise(st)
        return ptr, cols[:nz.value], cnt[:nz.value]

    def train_bytes(self, epsilon: float, cost: float, solver: int) -> bytes:
        need = C.c_size_t()
        st = self._L.vpt_trainer_train(self._h, (C.c_double * 2)(float(epsilon), float(cost)), int(solver), None, 0, C.byref(need))
        if st != _lib.VPT_OK:
            _raise(st)
        buf = (C.c_uint8 * need.value)()
        st = self._L.vpt_trainer_model(self._h, buf, need.value, C.byref(need))
        if st != _lib.VPT_OK:
            _raise(st)
        return bytes(buf)

    def train(self, epsilon: float, cost: float, solver: int) -> Model:  # trainer.rs:352-487
        return Model.read_slice(self.train_bytes(epsilon, cost, solver))[0]

    def weights(self):
        """After train: (fp64 weights in key order, bias, keys as Python ints)."""
        n = C.c_size_t()
        st = self._L.vpt_trainer_weights(self._h, None, None, None, 0, C.byref(n))
        if st != _lib.VPT_OK:
            _raise(st)
        w = np.zeros(max(n.value, 1), np.float64)
        k = np.zeros(2 * max(n.value, 1), np.uint64)
        b = C.c_double()
        st = self._L.vpt_trainer_weights(self._h, w.ctypes.data, C.addressof(b), k.ctypes.data, n.value, C.byref(n))
        if st != _lib.VPT_OK:
            _raise(st)
        keys = [int(k[2 * j]) | (int(k[2 * j + 1]) << 64) for j in range(n.value)]
        return w[:n.value], b.value, keys

    def last_stats(self) -> dict:
        s = _lib.TrainStats()
        st = self._L.vpt_trainer_last_stats(self._h, C.addressof(s))
        if st != _lib.VPT_OK:
            _raise(st)
        return {k: getattr(s, k) for k, _ in s._fields_}

    # ---- tag models (train_tags=True)
    def set_tag_path(self, mode: int) -> None:
        """0: the solver is picked by a problem's size; 1: every tag problem goes through the global-memory solver."""
        st = self._L.vpt_trainer_set_tag_path(self._h, int(mode))
        if st != _lib.VPT_OK:
            _raise(st)

    def n_tag_models(self) -> int:
        n, m = C.c_size_t(), C.c_size_t()
        st = self._L.vpt_trainer_n_tag_problems(self._h, C.byref(n), C.byref(m))
        if st != _lib.VPT_OK:
            _raise(st)
        return m.value

    def tag_problems(self) -> List[dict]:
        """The trained (surface, slot) problems in model order: surface, slot, candidates in id order, rows, sorted keys (Python ints),
        row_ptr, cols, y, and `path` (0 before training, 1 in-kernel, 2 global-memory)."""
        n = C.c_size_t()
        st = self._L.vpt_trainer_n_tag_problems(self._h, C.byref(n), None)
        if st != _lib.VPT_OK:
            _raise(st)
        out = []
        for i in range(n.value):
            info = _lib.TagProblemInfo()
            st = self._L.vpt_trainer_tag_problem(self._h, i, C.addressof(info), None, None, None, None, None, None, None)
            if st != _lib.VPT_OK:
                _raise(st)
            surf = np.zeros(info.surface_bytes + 1, np.uint8)
            cb = np.zeros(info.cand_bytes + 1, np.uint8)
            co = np.zeros(info.n_classes + 1, np.uint64)
            keys = np.zeros(2 * info.n_features + 2, np.uint64)
            rp = np.zeros(info.n_rows + 1, np.uint64)
            cols = np.zeros(info.nnz + 1, np.uint32)
            y = np.zeros(info.n_rows + 1, np.uint32)
            st = self._L.vpt_trainer_tag_problem(self._h, i, C.addressof(info), surf.ctypes.data, cb.ctypes.data, co.ctypes.data, keys.ctypes.data,
                                                 rp.ctypes.data, cols.ctypes.data, y.ctypes.data)
            if st != _lib.VPT_OK:
                _raise(st)
            out.append({"surface": bytes(surf[:info.surface_bytes]).decode("utf-8"), "slot": info.slot, "path": info.path, "model": info.model,
                        "candidates": [bytes(cb[int(co[c]):int(co[c + 1])]).decode("utf-8") for c in range(info.n_classes)],
                        "n_rows": info.n_rows, "keys": [int(keys[2 * j]) | (int(keys[2 * j + 1]) << 64) for j in range(info.n_features)],
                        "row_ptr": rp, "cols": cols[:info.nnz], "y": y[:info.n_rows]})
        return out

    def _tag_weights_stats(self, i: int, n_classes: int, n_features: int):
        w = np.zeros((n_classes, n_features + 1), np.float64)
        stats = (_lib.TrainStats * n_classes)()
        st = self._L.vpt_trainer_tag_weights(self._h, i, w.ctypes.data, w.size, C.addressof(stats))
        if st != _lib.VPT_OK:
            _raise(st)
        return w, [{k: getattr(s, k) for k, _ in s._fields_} for s in stats]

    def tag_weights(self, i: int) -> np.ndarray:
        """After train: problem i's fp64 weights [classes][features + 1], the bias last."""
        info = _lib.TagProblemInfo()
        st = self._L.vpt_trainer_tag_problem(self._h, i, C.addressof(info), None, None, None, None, None, None, None)
        if st != _lib.VPT_OK:
            _raise(st)
        return self._tag_weights_stats(i, info.n_classes, info.n_features)[0]

    def tag_stats(self) -> dict:
        """After train: {"problems": per problem {"path", "classes": [TRON stats per class]}, "summary": problems and seconds per path}."""
        probs = []
        n = C.c_size_t()
        st = self._L.vpt_trainer_n_tag_problems(self._h, C.byref(n), None)
        if st != _lib.VPT_OK:
            _raise(st)
        for i in range(n.value):
            info = _lib.TagProblemInfo()
            st = self._L.vpt_trainer_tag_problem(self._h, i, C.addressof(info), None, None, None, None, None, None, None)
            if st != _lib.VPT_OK:
                _raise(st)
            probs.append({"path": info.path, "seconds_setup": info.seconds_setup, "seconds_solve": info.seconds_solve,
                          "classes": self._tag_weights_stats(i, info.n_classes, info.n_features)[1]})
        sm = _lib.TagTrainSummary()
        st = self._L.vpt_trainer_tag_summary(self._h, C.addressof(sm))
        if st != _lib.VPT_OK:
            _raise(st)
        return {"problems": probs, "summary": {k: getattr(sm, k) for k, _ in sm._fields_}}
