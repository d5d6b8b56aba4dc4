"""The case table of the string dictionary, shared by tests/test_strdict_model.py (the model against the oracle, on the CPU) and
tests/test_gpu_strdict.py (aqg_str_encode against the model).  A case is a POOL of distinct contents (bytes, or None for a NULL row
pointer) and an index per row into it, so that the cost of building a column grows with the pool and not with the row count.
Every case is a function of the row count n alone (seeded), holds every string of its pool from n = MIN_ROWS on, and says whether it
holds two different strings under one 64-bit hash and length (`collides`: the device dictionary must then be rejected)."""
import functools

import numpy as np

import strdict_model as sm

WORD_EDGE_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 63, 64, 65, 4099)
# the empty marks of the library's tables as 64-bit hashes: 0, EMPTY64, the sign bit and its neighbours (MERGE_EMPTY / XS_EMPTY = 2^63 + 1);
# then EMPTY32 = 0x80000000 in either dword and in both, for the wide build, whose keys travel as dword planes
CHOSEN_HASHES = (0, 2 ** 64 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 63 - 1, 0x80000000, 0xFFFFFFFF80000000, 0x8000000080000000, 0x80000000FFFFFFFF)
MIN_ROWS = 2049                                 # the largest pool of the table (distinct_2049): every case holds all its strings from here on
SIZES = (65_535, 65_536, 65_537, 70_003)        # the host map's last size, the device dictionary's first two, and one no multiple of 16


class Case:
    def __init__(self, name, pool, idx, collides=False):
        self.name, self.pool, self.idx, self.collides = name, list(pool), np.ascontiguousarray(idx, dtype=np.int64), collides

    def strs(self):
        """the column as a list of n bytes objects / None"""
        return [self.pool[i] for i in self.idx.tolist()]


def _rng(*key):
    return np.random.default_rng([0x57D1C7] + [int(k) for k in key])


def _cover(rng, n, npool):
    """n random pool indices among which every pool entry occurs (n >= npool)"""
    assert n >= npool
    idx = rng.integers(0, npool, n)
    idx[rng.permutation(n)[:npool]] = np.arange(npool)
    return idx


def word_edge_pool():
    """one string of every length at and around the 8-byte words of the hash, a second that differs from it in its LAST byte only and,
    from 9 bytes on, a third that differs in byte 0 only"""
    pool = []
    for L in WORD_EDGE_LENGTHS:
        s = bytes((i * 37 + L) % 251 + 1 for i in range(L))
        pool.append(s)
        if L >= 1:
            pool.append(s[:-1] + bytes([s[-1] % 255 + 1]))
        if L >= 9:
            pool.append(bytes([s[0] % 255 + 1]) + s[1:])
    assert len(set(pool)) == len(pool) and all(0 not in s for s in pool)
    return pool


def high_low_pool():
    """strings over {0x01, 0x7F, 0x80, 0xFE, 0xFF} at lengths 1 .. 17, and for each pairs that differ by 0x7F against 0xFF in ONE
    position (first, middle, last), and pairs that both start with 0xFF and differ in byte 1 only: a byte sign-extended into its word
    would smear the 0xFF over the bytes above it, and the two of such a pair would hash alike"""
    rng = _rng(3)
    alphabet = np.array([0x01, 0x7F, 0x80, 0xFE, 0xFF], np.uint8)
    pool = []
    for L in range(1, 18):
        s = bytearray(alphabet[rng.integers(0, 5, L)].tobytes())
        pool.append(bytes(s))
        for pos in sorted({0, L // 2, L - 1}):
            for v in (0x7F, 0xFF):
                t = bytearray(s); t[pos] = v
                pool.append(bytes(t))
        if L >= 2:
            for v in (0x01, 0x80):
                pool.append(b"\xff" + bytes([v]) + bytes(s[2:]))
    return list(dict.fromkeys(pool))


def _ordinary(k, stem=b"ord"):
    return [stem + b"%04d" % i + b"x" * (i % 13) for i in range(k)]


def span_edge_rows(n):
    """the rows either side of every multiple of n // 16 and of every start of the host walk's sixteen thread spans (n * t // 16)"""
    rows = set()
    for t in range(1, 16):
        for m in (t * (n // 16), n * t // 16):
            rows |= {m - 1, m, m + 1}
    return sorted(r for r in rows if 0 < r < n - 1)


def _far_apart(n, last_only):
    """five fillers of unequal lengths; a string of its own in every row around a span edge; X in row 0 and row n - 1 only, or
    (last_only) Y in row n - 1 only"""
    rng = _rng(6, n)
    fill = [b"f", b"fill-22", b"filler-333333", b"", b"f" * 40]
    edges = span_edge_rows(n)
    pool = fill + [b"E%d_" % r + b"e" * (r % 11) for r in edges] + [b"only-at-the-ends" if not last_only else b"only-in-the-last-row"]
    idx = rng.integers(0, len(fill), n)
    idx[: len(fill)] = np.arange(len(fill))                       # (rows 0 .. 4 lie before the first edge: n // 16 >= 8)
    idx[edges] = len(fill) + np.arange(len(edges))
    idx[n - 1] = len(pool) - 1
    if not last_only:
        idx[0] = len(pool) - 1
        idx[5] = 0                                                # the filler that row 0 held
    return pool, idx


def pairs(k):
    """k colliding pairs (seeded: the same in every process)"""
    rng = _rng(9)
    return [sm.collision(rng) for _ in range(k)]


def _collision_shapes(n, partner):
    """the collision columns; partner(a, b) -> the string that stands where B would: B itself, or a control that does not collide"""
    (a, b0), (a2, b20), (a3, b30) = pairs(3)
    b, b2, b3 = partner(a, b0), partner(a2, b20), partner(a3, b30)
    half = np.arange(n) % 2
    yield "interleaved_a_first", [a, b], half
    yield "interleaved_b_first", [b, a], half
    last = np.zeros(n, np.int64); last[n - 1] = 1
    yield "b_in_the_last_row", [a, b], last
    first = np.zeros(n, np.int64); first[0] = 1
    yield "b_in_row_0_only", [a, b], first
    yield "pair_among_1000", _ordinary(1000) + [a, b], _cover(_rng(10, n), n, 1002)
    yield "three_pairs", _ordinary(20) + [a, b, a2, b2, a3, b3], _cover(_rng(11, n), n, 26)
    # pairs that share their first 8 and their first 4,096 bytes: only the last 16 bytes tell the two apart
    rng, pool = _rng(13), _ordinary(20)
    for words in (1, 512):
        prefix = bytes(rng.integers(1, 256, 8 * words, dtype=np.uint8))
        pa, pb = sm.collision(rng, prefix)
        pool += [pa, partner(pa, pb)]
    yield "shared_prefix", pool, _cover(_rng(14, n), n, len(pool))


@functools.lru_cache(maxsize=None)
def cases(n):
    """the whole table at n rows (made once per n and shared: nobody writes to a case)"""
    assert n >= MIN_ROWS
    out = []
    pool = word_edge_pool()
    out.append(Case("word_edges", pool, _cover(_rng(1, n), n, len(pool))))
    pool = [b"a" * k for k in range(41)] + [b"a" * (k - 1) + b"b" for k in range(1, 41)]      # ... and, of every length, one that leaves the chain in its last byte
    out.append(Case("prefixes", pool, _cover(_rng(2, n), n, len(pool))))
    pool = high_low_pool()
    out.append(Case("high_low_bytes", pool, _cover(_rng(3, n), n, len(pool))))
    out.append(Case("empty_only", [b""], np.zeros(n, np.int64)))
    out.append(Case("null_only", [None], np.zeros(n, np.int64)))
    for first, name in ((1, "null"), (0, "empty"), (2, "real")):
        pool = [b"", None, b"x1", b"yy-and-longer"]
        idx = _cover(_rng(4, n), n, 4)
        if idx[0] != first:
            idx[int(np.flatnonzero(idx == first)[0])] = idx[0]    # swap, so that every entry stays in the column
            idx[0] = first
        out.append(Case("mixed_first_row_" + name, pool, idx))
    out.append(Case("one_distinct", [b"the-only-one"], np.zeros(n, np.int64)))
    out.append(Case("all_distinct", [b"%d" % i for i in range(n)], np.arange(n)))
    for k in (2048, 2049):
        out.append(Case("distinct_%d" % k, _ordinary(k, b"d"), _cover(_rng(5, n, k), n, k)))
    out.append(Case("far_apart_first_and_last", *_far_apart(n, False)))
    out.append(Case("far_apart_last_only", *_far_apart(n, True)))
    rng = _rng(7)
    pool = _ordinary(50) + [sm.with_hash(t, rng) for t in CHOSEN_HASHES]
    out.append(Case("chosen_hashes", pool, _cover(_rng(8, n), n, len(pool))))
    for name, pool, idx in _collision_shapes(n, lambda a, b: b):
        out.append(Case("collision_" + name, pool, idx, collides=True))
    crng = _rng(12)
    for name, pool, idx in _collision_shapes(n, lambda a, b: sm.ordinary16(crng, [a, b], a[:-16])):
        out.append(Case("control_" + name, pool, idx))
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.idx.setflags(write=False)
    return tuple(out)


NAMES = [c.name for c in cases(MIN_ROWS)]


def case(name, n):
    return next(c for c in cases(n) if c.name == name)
