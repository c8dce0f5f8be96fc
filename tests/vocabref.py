"""TEST INFRASTRUCTURE: a numpy / Python restatement of the vocabulary of the token stream's id pass (vaporetto_amd/csrc/vocab_table.hpp,
kernels_vocab.hip): the hash of a surface, where the builder places every key, and the ids of a span CSR by a plain dict lookup on the
(optionally normalised) substring.  Nothing here is on the product path."""
import numpy as np

from vaporetto_amd import api

M64 = (1 << 64) - 1
SEED, PRIME = 0xCBF29CE484222325, 0x100000001B3


def surface_hash(surface: str) -> int:
    """FNV-1a over the code points, finished with the length (pattern_tagger.hpp: rule_hash_step / rule_hash_finish)."""
    h = SEED
    for c in surface:
        h = ((h ^ ord(c)) * PRIME) & M64
    x = h ^ len(surface)
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    return x ^ (x >> 33)


def hash_many(cps: np.ndarray) -> np.ndarray:
    """surface_hash of every row of a [n, length] array of code points (uint64 arithmetic wraps as the C++ does)."""
    cps = np.asarray(cps, np.uint64)
    with np.errstate(over="ignore"):
        h = np.full(len(cps), SEED, np.uint64)
        for j in range(cps.shape[1]):
            h = (h ^ cps[:, j]) * np.uint64(PRIME)
        x = h ^ np.uint64(cps.shape[1])
        x ^= x >> np.uint64(33)
        x = x * np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x = x * np.uint64(0xC4CEB9FE1A85EC53)
        return x ^ (x >> np.uint64(33))


def table_bits(n_keys: int) -> int:
    bits = 1
    while (1 << bits) < 2 * n_keys:
        bits += 1
    return bits


def home(surface: str, bits: int) -> int:
    return surface_hash(surface) & ((1 << bits) - 1)


def fingerprint(surface: str) -> int:
    return surface_hash(surface) >> 32


def place(surfaces):
    """-> (bits, slots, where): slots[s] = None or (id, chars, fingerprint, first code point); where[id] = (home slot, slot, probes).  Linear
    probing in the order of the ids, as build_vocab_table does."""
    bits = table_bits(len(surfaces))
    mask = (1 << bits) - 1
    slots, where, at = [None] * (1 << bits), [], 0
    for k, s in enumerate(surfaces):
        h = surface_hash(s)
        slot, probes = h & mask, 1
        while slots[slot] is not None:
            slot, probes = (slot + 1) & mask, probes + 1
        slots[slot] = (k, len(s), h >> 32, at)
        where.append((h & mask, slot, probes))
        at += len(s)
    return bits, slots, where


_NORM = api.KyteaFullwidthFilter()


def ids_from_csr(docs, token_offsets, starts, ends, vocab: dict, unk_id: int, normalize: bool):
    """docs: the documents' bytes.  starts None: a token starts where the one before it in its document ends, or at 0."""
    out = []
    for i, raw in enumerate(docs):
        a, b = int(token_offsets[i]), int(token_offsets[i + 1])
        for k in range(a, b):
            s = int(starts[k]) if starts is not None else (int(ends[k - 1]) if k > a else 0)
            sub = raw[s:int(ends[k])].decode("utf-8")
            if normalize:
                sub = _NORM.filter(sub)
            out.append(vocab.get(sub, unk_id))
    return np.array(out, np.int32)


def find_same_home(n_keys: int, want_home: int, count: int, seed: int = 5, alphabet="あいう漢字AB09𠮷é"):
    """`count` distinct surfaces whose home slot in a table of n_keys keys is want_home (a plain search over random short strings)."""
    import random
    rng = random.Random(seed)
    bits, got, seen = table_bits(n_keys), [], set()
    while len(got) < count:
        s = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 4)))
        if s not in seen and home(s, bits) == want_home:
            got.append(s)
        seen.add(s)
    return got


def find_fingerprint_twins(bits: int, n: int = 1 << 20, seed: int = 12345, length: int = 4):
    """Two different surfaces of `length` chars with the same fingerprint (high 32 bits) and the same home slot in a table of 2^bits slots: a
    birthday search over n random candidates -- 32 + bits bits to collide in, n^2 / 2 pairs.  -> (a, b) or None"""
    rng = np.random.default_rng(seed)
    cps = rng.integers(0x3041, 0x3097, size=(n, length), dtype=np.uint64)   # hiragana
    h = hash_many(cps)
    key = ((h >> np.uint64(32)) << np.uint64(bits)) | (h & np.uint64((1 << bits) - 1))
    order = np.argsort(key, kind="stable")
    ks = key[order]
    for j in np.nonzero(ks[1:] == ks[:-1])[0]:
        a, b = cps[order[j]], cps[order[j + 1]]
        if not np.array_equal(a, b):
            return "".join(chr(int(c)) for c in a), "".join(chr(int(c)) for c in b)
    return None
