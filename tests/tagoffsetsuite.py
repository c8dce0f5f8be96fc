"""Hostile out_offsets for the device-resident tag entry points (vpt_fill_tags_batch_device, vpt_fill_tags_scores_batch_device,
vpt_expand_tags_batch_device, vpt_write_tagged_batch_device) on batches that span SEVERAL front-end runs (kernels_tags.hip): offsets that do not
describe the text are an error at sync, never a write outside the batch's arrays -- the caller's or the workspace's.  Run on the CPU emulator by
tests/test_tag_offsets_emu.py (in child processes: tearing the workspace down is where hipemu checks the red zones around every hipMalloc, and it
aborts when one is touched) and on the MI355X by tests/test_tag_offsets_gpu.py.

The expected outcome of every case is a status word.  The detectors are the guard words around every array the caller passes (GUARD_WORDS of a
known pattern on both sides, compared after the calls) and, on the emulator, the red zones.  After the bad call the same workspace takes the true
offsets and its dense tags, the records expanded by vpt_expand_tags_batch_device and the tagged text must equal, int for int and byte for byte,
what oracle.cbind.OraclePredictor.predict_tags gives sentence by sentence.

    python -m tests.tagoffsetsuite --emu BATCH VARIANT      runs the cases of one (batch, variant) on the emulator, prints "ran N cases", exits 0

CASES (counted and asserted, nothing is skipped): per batch the corruptions of CORRUPTIONS that apply to it -- A: 13, B: 14, C: 14 -- times the
three VARIANTS: 123."""
import random
import sys

import numpy as np

from tests import devmem, randmodel
from vaporetto_amd import api
from vaporetto_amd.modelfmt import TagModel, TagNgramData, TagWeight

ALPHA = "あいう"
GUARD_WORDS = 64
PATTERN = 0xA5
MESSAGE = "do not match the text"

BATCHES = ("A", "B", "C")
VARIANTS = ("plain", "pattern", "scores")   # dense tags only | a PatternMatchTagger attached (the merge kernels run) | scores and tag models too
# name -> the batches it applies to.  Each makes S + 1 values from the true offsets (and the total_boundaries the calls are given).
CORRUPTIONS = {
    "down_at_run_boundary": "ABC",     # (1) every run keeps its own offsets in order; the runs alternate between the batch's ends
    "down_inside_run": "BC",           # (2)
    "sawtooth": "ABC",                 # (3) every other offset near total_boundaries, every other near 0
    "last_larger": "ABC",              # (4) the last offset against total_boundaries, both ways, from either side
    "last_smaller": "ABC",
    "total_larger": "ABC",             #     (an upper bound of the last offset is what the header allows: see UPPER_BOUND_IS_VALID)
    "total_smaller": "ABC",
    "all_zero": "ABC",                 # (5)
    "all_total": "ABC",
    "one_2_63": "ABC",                 # (6) ooff[i] + i wraps or leaves the 32-bit index range
    "one_2_64_minus_1": "ABC",
    "one_2_32_plus_k": "ABC",
    "run_of_2_31": "ABC",              #     a run of 0x7FFFFF00 chars and more by its offsets (in a batch this small such a run also ends past
                                       #     total_chars: a run that long INSIDE the batch takes a batch of 2^31 chars, which no test can hold)
    "rewritten_behind_fill_tags": "ABC",   # (7) valid for fill_tags, overwritten in place by (1) in front of the consumers on the stream
}
# include/vaporetto_hip.h, vpt_predict_batch_device: "total_boundaries = out_offsets[S] ..., or any upper bound of it ... the same bound must then be
# passed to the fill_tags / write calls that follow".  So a total_boundaries LARGER than the last offset describes the text: that case asserts that
# sync reports nothing and that the call itself, on the larger arrays, gives the oracle's tags and text -- with every other check as it is.
UPPER_BOUND_IS_VALID = ("total_larger",)
CASES_PER_BATCH = {b: sum(1 for v in CORRUPTIONS.values() if b in v) for b in BATCHES}
assert CASES_PER_BATCH == {"A": 13, "B": 14, "C": 14}
N_CASES = sum(CASES_PER_BATCH.values()) * len(VARIANTS)
assert N_CASES == 123


def tag_model_data():
    """A tag model on every single char of ALPHA, 2 slots of 2 .. 3 candidates, with context n-grams so that the choice depends on the text: with
    labels all 1 every char is a token, a candidate and a record."""
    m = randmodel.rand_model(4242, alphabet=list(ALPHA), wc=2, wt=2, n_tag_models=0, n_char=12, n_type=4, n_dict=4, max_word=3)
    rng = random.Random(99)
    for k, ch in enumerate(ALPHA):
        slots = [["%sa%d" % ("xyz"[k], q) for q in range(2 + (k & 1))], ["%sb%d" % ("xyz"[k], q) for q in range(3 - (k & 1))]]
        zlen = sum(len(s) for s in slots)
        tm = TagModel(ch, slots, bias=[rng.randint(-20, 20) for _ in range(zlen)])
        for left in ALPHA:
            tm.char_ngram_model.append(TagNgramData(left + ch, [TagWeight(0, [rng.randint(-40, 40) for _ in range(zlen)])]))
        for right in ALPHA[:2]:
            tm.char_ngram_model.append(TagNgramData(ch + right, [TagWeight(1, [rng.randint(-40, 40) for _ in range(zlen)])]))
        m.tag_models.append(tm)
    return m


def batch_texts(name):
    rng = random.Random({"A": 1, "B": 2, "C": 3}[name])
    lens = {"A": [1500] * 4, "B": [100] * 64, "C": [rng.randint(1, 40) for _ in range(300)]}[name]
    return ["".join(rng.choice(ALPHA) for _ in range(n)) for n in lens]


RULES = {"あ": ["Ra", "Rb"], "い": [None, "Rc"], "うう": ["Rd", "Re"]}


class Env:
    """One (batch, variant): the predictor, the texts, the true offsets, what the oracle says the tags and the tagged text are."""

    def __init__(self, batch, variant):
        from oracle import cbind
        self.batch, self.variant = batch, variant
        m = tag_model_data()
        raw = api.Model(m).to_vec()
        self.pred = api.Predictor(api.Model.read_slice(raw)[0], True, device=0)
        self.tagger = api.PatternMatchTagger(RULES) if variant == "pattern" else None
        self.texts = batch_texts(batch)
        self.utf8, self.boff = api.pack_texts([t.encode("utf-8") for t in self.texts])
        self.ooff = api.count_boundaries(self.utf8, self.boff).astype(np.uint64)
        self.S, self.nb, self.nt = len(self.texts), int(self.ooff[-1]), self.pred.n_tags()
        assert self.nt == 2
        self.stride = self.pred.tag_score_stride()
        oracle = cbind.OraclePredictor(raw, True)
        rows, lines = [], []
        by_token = {tm.token: tm.tags for tm in m.tag_models}
        for t in self.texts:
            tags, nt = oracle.predict_tags(t, np.ones(max(len(t) - 1, 1), np.uint8))
            assert nt == self.nt and (tags >= 0).all()   # every slot of every char is Some: the rules change nothing
            rows.append(tags)
            lines.append(" ".join(c + "".join("/" + by_token[c][j][int(v)] for j, v in enumerate(row)) for c, row in zip(t, tags)).encode("utf-8"))
        self.want_tags = np.concatenate(rows).astype(np.int32)
        self.want_lines = lines
        self.cap = 3 * len(self.utf8) + (self.nb + self.S) * (self.pred.max_tag_suffix() + (self.tagger.max_tag_suffix(self.pred) if self.tagger else 0)) + 16
        self.run_sent = None

    def check_geometry(self, plan):
        """What the workspace says of the last fill_tags call: at least 3 runs, and the sentences of a run."""
        runs, per = plan["tag_runs"], plan["tag_run_sent"]
        assert runs >= 3 and per >= 1 and (runs - 1) * per < self.S <= runs * per, plan
        want = {"A": (4, 1), "B": (4, 20)}.get(self.batch)   # A: four runs of one sentence; B: 20, 20, 20 and a short last run of 4
        if want:
            assert (runs, per) == want, plan
        else:
            assert 60 <= per <= 140, plan                        # C: about 2 K chars of sentences that hold 20 on average
        self.run_sent = per


def corrupt(env, name):
    """-> (offsets uint64 [S + 1], the total_boundaries the calls are given)"""
    o, S, nb, R = [int(x) for x in env.ooff], env.S, env.nb, env.run_sent
    bad = list(o)
    tb = nb
    if name in ("down_at_run_boundary", "rewritten_behind_fill_tags"):
        if env.batch == "A":
            bad = [0, 4400, 100, 4500, 5996]   # the reproduction of the out-of-bounds write
            assert nb == 5996
        else:   # run k keeps its sentences' lengths; odd runs are pushed to the batch's end, even ones pulled to its start
            for k in range(1, (S + R - 1) // R):
                a, b = k * R, min((k + 1) * R, S)
                shift = nb - o[b] if k & 1 else k - o[a]
                for i in range(a, b):
                    bad[i] = o[i] + shift
        assert bad != o and bad[-1] == nb
    elif name == "down_inside_run":
        i = R + R // 2
        assert i % R != 0 and i < S
        bad[i] = bad[i - 1] // 2
    elif name == "sawtooth":
        for i in range(1, S):
            bad[i] = nb - (S - i) if i & 1 else i
    elif name == "last_larger":
        bad[-1] = nb + 7
    elif name == "last_smaller":
        bad[-1] = nb - 7
    elif name == "total_larger":
        tb = nb + 5
    elif name == "total_smaller":
        tb = nb - 5
    elif name == "all_zero":
        bad = [0] * (S + 1)
    elif name == "all_total":
        bad = [nb] * (S + 1)
    elif name == "one_2_63":
        bad[R] = 1 << 63
    elif name == "one_2_64_minus_1":
        bad[R] = (1 << 64) - 1
    elif name == "one_2_32_plus_k":
        bad[2 * R] = (1 << 32) + o[2 * R]
    elif name == "run_of_2_31":
        for i in range(2 * R, S + 1):
            bad[i] = o[i] + 0x7FFFFF00   # run 1 is 0x7FFFFF00 chars longer than its text
    else:
        raise KeyError(name)
    return np.array(bad, dtype=np.uint64), tb


class Guarded:
    """A caller's array with GUARD_WORDS words of PATTERN bytes on both sides (4-byte words at least, so that every dtype's guard is 256 bytes
    and the array keeps the allocation's alignment)."""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        self.dtype, self.n = arr.dtype, len(arr)
        self.g = GUARD_WORDS * max(4 // arr.dtype.itemsize, 1)
        full = np.empty(self.n + 2 * self.g, arr.dtype)
        full.view(np.uint8)[:] = PATTERN
        full[self.g:self.g + self.n] = arr
        self.buf = devmem.put(full)
        self.ptr = self.buf.ptr + self.g * arr.dtype.itemsize
        self.sent = arr.copy()

    def get(self, n=None):
        return self.buf.get()[self.g:self.g + (self.n if n is None else n)]

    def set(self, arr):
        full = self.buf.get()
        full[self.g:self.g + len(arr)] = arr
        self.buf.set(full)

    def guards_intact(self):
        b = self.buf.get().view(np.uint8)
        w = self.g * self.dtype.itemsize
        return bool((b[:w] == PATTERN).all() and (b[len(b) - w:] == PATTERN).all())


def run_case(env, name):
    """One corruption on a workspace of its own; every check of the module's docstring.  The workspace is destroyed before this returns."""
    S, nb, nt = env.S, env.nb, env.nt
    have_plan = env.run_sent is not None
    st = devmem.stream()
    batch = api.DeviceBatch(env.pred)
    batch.set_pattern_tagger(env.tagger)
    pad = np.zeros(32, np.uint8)
    d_text = devmem.put(np.concatenate([env.utf8, pad]))
    d_boff = devmem.put(env.boff.astype(np.uint64))
    if not have_plan:   # the run geometry, from the workspace itself: a valid call first
        d_o = devmem.put(env.ooff)
        d_l = devmem.put(np.ones(nb + 16, np.uint8))
        batch.fill_tags(d_text.ptr, d_boff.ptr, d_o.ptr, S, nb, d_l.ptr, 0, st)
        batch.sync()
        env.check_geometry(batch.last_plan())
    bad, tb = corrupt(env, name)
    rewritten = name == "rewritten_behind_fill_tags"
    tc = max(tb, nb) + S   # chars of the arrays: what the caller promises (total_boundaries + S), and never less than the true batch takes below
    arrays = {
        "offsets": Guarded(env.ooff if rewritten else bad),
        "labels": Guarded(np.ones(max(tb, nb, 1), np.uint8)),
        "tags": Guarded(np.full(tc * nt, 0x5A5A5A5A, np.int32)),
        "tags2": Guarded(np.full(tc * nt, 0x5A5A5A5A, np.int32)),
        "out": Guarded(np.zeros(env.cap, np.uint8)),
        "out_offsets": Guarded(np.zeros(S + 1, np.uint64)),
    }
    if env.variant == "scores":
        arrays["scores"] = Guarded(np.zeros(tc * env.stride, np.int32))
        arrays["models"] = Guarded(np.full(tc, -1, np.int32))
    A = arrays

    def fill(total_boundaries):
        if env.variant == "scores":
            batch.fill_tags_scores(d_text.ptr, d_boff.ptr, A["offsets"].ptr, S, total_boundaries, A["labels"].ptr, A["tags"].ptr, A["scores"].ptr,
                                   A["models"].ptr, st)
        else:
            batch.fill_tags(d_text.ptr, d_boff.ptr, A["offsets"].ptr, S, total_boundaries, A["labels"].ptr, A["tags"].ptr, st)

    def consumers(total_boundaries):
        """enqueued behind fill_tags without a sync: each returns an error or leaves the guards intact (checked by the caller)"""
        refused = 0
        for call in (lambda: batch.expand_tags(S, total_boundaries, A["tags2"].ptr, st),
                     lambda: batch.write_tagged(d_text.ptr, d_boff.ptr, A["offsets"].ptr, S, total_boundaries, A["labels"].ptr, 0, A["out"].ptr, env.cap,
                                                A["out_offsets"].ptr, st)):
            try:
                call()
            except api.VaporettoError:
                refused += 1
        return refused

    # ---- the bad call and the consumers behind it
    fill(tb)
    if rewritten:
        A["offsets"].set(bad)   # in stream order behind fill_tags, in front of the consumers
    consumers(tb)
    try:
        batch.sync()
        raised = None
    except api.VaporettoError as e:
        raised = str(e)
    if name in UPPER_BOUND_IS_VALID:
        assert raised is None, (name, raised)
        n = (nb + S) * nt
        assert np.array_equal(A["tags"].get(n), env.want_tags.reshape(-1)) and np.array_equal(A["tags2"].get(n), env.want_tags.reshape(-1)), name
        assert (A["tags"].get()[n:] == -1).all() and (A["tags2"].get()[n:] == -1).all(), name   # chars the bound promises and the text does not have: None
        toff = A["out_offsets"].get()
        text = bytes(A["out"].get(int(toff[S])))
        assert [text[int(toff[i]):int(toff[i + 1])] for i in range(S)] == env.want_lines, (name, "tagged text")
    else:
        assert raised is not None and MESSAGE in raised, (name, raised)
    batch.sync()   # reported once
    broken = [k for k, a in A.items() if not a.guards_intact()]
    assert not broken, (name, "guard words overwritten around", broken)
    if rewritten:   # fill_tags itself saw the true offsets: its dense array is the batch's
        assert np.array_equal(A["tags"].get(), env.want_tags.reshape(-1)), name

    # ---- the workspace stays usable: the true offsets on the same arrays
    A["offsets"].set(env.ooff)
    A["tags"].set(np.full(tc * nt, 0x5A5A5A5A, np.int32))
    A["tags2"].set(np.full(tc * nt, 0x5A5A5A5A, np.int32))
    fill(nb)
    assert consumers(nb) == 0
    batch.sync()
    n = (nb + S) * nt
    want = env.want_tags.reshape(-1)
    assert np.array_equal(A["tags"].get(n), want), (name, "dense tags")
    assert np.array_equal(A["tags2"].get(n), want), (name, "expanded records")
    assert (A["tags"].get()[n:] == 0x5A5A5A5A).all() and (A["tags2"].get()[n:] == 0x5A5A5A5A).all(), name
    toff = A["out_offsets"].get()
    text = bytes(A["out"].get(int(toff[S])))
    assert [text[int(toff[i]):int(toff[i + 1])] for i in range(S)] == env.want_lines, (name, "tagged text")
    broken = [k for k, a in A.items() if not a.guards_intact()]
    assert not broken, (name, "guard words overwritten around", broken)
    plan = batch.last_plan()
    assert (plan["tag_runs"], plan["tag_run_sent"]) == ((S + env.run_sent - 1) // env.run_sent, env.run_sent)
    del batch


def names_for(batch):
    return [n for n, where in CORRUPTIONS.items() if batch in where]


def run_group(batch, variant, log=None):
    """Every case of one (batch, variant); -> the number of cases run."""
    env = Env(batch, variant)
    ran = 0
    for name in names_for(batch):
        if log:
            log("case %s %s %s" % (batch, variant, name))
        run_case(env, name)
        ran += 1
    assert ran == CASES_PER_BATCH[batch]
    return ran


def main(argv):
    assert len(argv) == 3 and argv[0] == "--emu", "usage: python -m tests.tagoffsetsuite --emu BATCH VARIANT"
    import gc
    from tests import emu
    from vaporetto_amd import _lib
    _lib._lib = emu.load()
    devmem.EMULATED = True

    def log(line):
        print(line, flush=True)

    ran = run_group(argv[1], argv[2], log)
    gc.collect()   # batch and predictor destroyed: hipemu has checked the red zones of every allocation it freed
    print("ran %d cases" % ran, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
