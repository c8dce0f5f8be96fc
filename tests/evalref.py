"""TEST INFRASTRUCTURE: a plain-Python restatement of the reference's tokenized-text parser and of its `evaluate` CLI, the yardstick the
new kernels are checked against.  It is never on the product path.

parse_tokenized: vaporetto/src/sentence.rs:285-400 (+ the n_tags division of from_tokenized, :450, where an input without chars
panics in the reference -- here the "must contain at least one character" error of the library).
evaluate: evaluate/src/main.rs:91-193."""
from typing import List, Optional, Sequence, Tuple

MSG = {1: "must contain at least one character", 2: "must not start with a whitespace", 3: "must not contain consecutive whitespaces",
       4: "must not end with a whitespace", 5: "a slash must follow a character", 6: "must not contain NULL"}


class ParseError(Exception):
    def __init__(self, reason: int):
        super().__init__("InvalidArgumentError: tokenized_text: " + MSG[reason])
        self.reason = reason


def parse_tokenized(text: str) -> Tuple[str, List[int], List[Optional[str]], int]:
    """-> (raw text, boundaries (0/1), tags (len(raw) * n_tags, None or str), n_tags); raises ParseError."""
    if not text:
        raise ParseError(1)
    raw: List[str] = []
    boundaries: List[int] = []
    tags_tmp: List[List[str]] = []
    tag_str: Optional[List[str]] = None
    prev_boundary = escape = False
    for c in text:                                         # sentence.rs:308-361
        if not escape and c == "\\":
            escape = True
        elif not escape and c == " ":
            if not raw:
                raise ParseError(2)
            if prev_boundary:
                raise ParseError(3)
            if tag_str is not None:
                tags_tmp[-1].append("".join(tag_str))
                tag_str = None
            prev_boundary = True
        elif not escape and c == "/":
            if not raw or prev_boundary:
                raise ParseError(5)
            if tag_str is not None:
                tags_tmp[-1].append("".join(tag_str))
            tag_str = []
        else:
            escape = False
            if c == "\0":
                raise ParseError(6)
            if tag_str is not None:
                tag_str.append(c)
                continue
            if raw:
                boundaries.append(1 if prev_boundary else 0)
            prev_boundary = False
            raw.append(c)
            tags_tmp.append([])
    if prev_boundary:                                       # sentence.rs:363-368
        raise ParseError(4)
    if tag_str is not None:
        tags_tmp[-1].append("".join(tag_str))
    if not raw:
        raise ParseError(1)
    n_tags = max(len(t) for t in tags_tmp)                  # sentence.rs:381-398
    tags: List[Optional[str]] = []
    for ts in tags_tmp:
        tags += [t if t else None for t in ts] + [None] * (n_tags - len(ts))
    return "".join(raw), boundaries, tags, n_tags


def tag_rows(tags: Sequence[Optional[str]], n_tags: int, n_chars: int) -> List[List[Optional[str]]]:
    return [list(tags[i * n_tags:(i + 1) * n_tags]) for i in range(n_chars)]


def counts(results) -> dict:
    """results: per sentence (ref_boundaries, ref_tag_rows, sys_boundaries, sys_tag_rows) -> the CLI's counters
    (evaluate/src/main.rs:124-191)."""
    c = dict(tp=0, tn=0, fp=0, fn=0, n_sys=0, n_ref=0, n_cor=0, n_sentences=0)
    for rb, rt, sb, st in results:
        for r, h in zip(rb, sb):
            if r == h:
                c["tp" if h == 1 else "tn"] += 1
            else:
                c["fp" if h == 1 else "fn"] += 1
        matched = True
        for r_b, r_t, s_b, s_t in zip(rb, rt, sb, st):
            if r_b == s_b:
                if s_b == 1:
                    if matched and r_t == s_t:
                        c["n_cor"] += 1
                    matched = True
                    c["n_ref"] += 1
                    c["n_sys"] += 1
            else:
                if s_b == 1:
                    c["n_sys"] += 1
                else:
                    c["n_ref"] += 1
                matched = False
        if matched and rt[-1] == st[-1]:
            c["n_cor"] += 1
        c["n_sys"] += 1
        c["n_ref"] += 1
        c["n_sentences"] += 1
    return c


def evaluate(lines: Sequence[str], system, predict_tags: bool = False, no_norm: bool = False) -> dict:
    """The CLI's loop (evaluate/src/main.rs:91-122).  system(raw_texts, normalised) -> (labels per sentence, tag rows per sentence
    or None when no tags are predicted); the caller supplies predict + filters (+ fill_tags) from the oracle."""
    parsed = [parse_tokenized(ln) for ln in lines if ln]
    sys_b, sys_t = system([p[0] for p in parsed], not no_norm)
    results = []
    for k, (raw, rb, tags, nt) in enumerate(parsed):
        rt = tag_rows(tags, nt, len(raw))
        if sys_t is not None:
            st = sys_t[k]
        elif no_norm:
            st = rt                                     # the parsed sentence keeps its gold tags
        else:
            st = [[] for _ in range(len(raw))]          # from_raw: n_tags = 0
        results.append((rb, rt, list(sys_b[k]), st))
    return counts(results)
