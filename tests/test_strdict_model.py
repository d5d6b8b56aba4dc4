"""The model of the string dictionary (tests/strdict_model.py) held to itself and to the oracle, on the CPU: the inverted hash really
hits its targets, the colliding pairs really collide, and codes() over the whole case table of tests/test_gpu_strdict.py
(tests/strdict_cases.py) is the oracle's typed group-by of the same strings."""
import ctypes as C
import os

import numpy as np
import pytest

import checker as ck
import strdict_cases as sc
import strdict_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
TARGETS = (0, 2 ** 64 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 63 - 1, 1)


def test_hash64_by_hand():
    """the empty string takes no word step; one byte is one zero-padded word; 8 and 9 bytes are one and two words"""
    M, S = sm.MUL, sm.SEED
    def fin(h):
        h = h * M % 2 ** 64
        return h ^ h >> 29
    def step(h, w):
        h = (h ^ w) * M % 2 ** 64
        return h ^ h >> 32
    assert sm.hash64(b"") == fin(S)
    assert sm.hash64(b"\x80") == fin(step(S ^ 1, 0x80))
    assert sm.hash64(b"abcdefgh") == fin(step(S ^ 8, int.from_bytes(b"abcdefgh", "little")))
    assert sm.hash64(b"abcdefghi") == fin(step(step(S ^ 9, int.from_bytes(b"abcdefgh", "little")), ord("i")))
    assert len({sm.hash64(b"a" * k) for k in range(41)}) == 41               # the length in the seed tells zero-padded prefixes apart


def test_with_hash_hits_its_target():
    rng = np.random.default_rng(1)
    targets = list(TARGETS) + [int(t) for t in rng.integers(0, 2 ** 64, 100, dtype=np.uint64)]
    for t in targets:
        s = sm.with_hash(t, rng)
        assert len(s) == 16 and 0 not in s
        assert sm.hash64(s) == t


def test_collision_pairs_collide():
    rng = np.random.default_rng(2)
    seen = set()
    for _ in range(50):
        a, b = sm.collision(rng)
        assert a != b and len(a) == len(b) == 16 and 0 not in a and 0 not in b
        assert sm.hash64(a) == sm.hash64(b)
        seen.add(a)
    assert len(seen) == 50
    c = sm.ordinary16(rng, [a, b])
    assert len(c) == 16 and 0 not in c and sm.hash64(c) != sm.hash64(a)
    for words in (1, 2, 512):                                                # a shared prefix of whole words: the last 16 bytes differ
        prefix = bytes(rng.integers(1, 256, 8 * words, dtype=np.uint8))
        a, b = sm.collision(rng, prefix)
        assert a != b and a[:-16] == b[:-16] == prefix and len(a) == len(b) and 0 not in a and 0 not in b and sm.hash64(a) == sm.hash64(b)
        assert a[-16:-8] != b[-16:-8] and a[-8:] != b[-8:]


def test_codes_by_hand():
    c, nd, first = sm.codes([b"b", None, b"a", b"", b"b", b"ab", b"a"])
    assert c.tolist() == [0, 1, 2, 1, 0, 3, 2] and c.dtype == np.uint32
    assert nd == 4 and first.tolist() == [0, 1, 2, 5]
    c, nd, first = sm.codes([])
    assert c.size == 0 and nd == 0 and first.size == 0
    assert sm.expected_route(65_535, True) == (sm.ROUTE_HOST, 0)
    assert sm.expected_route(65_536, False) == (sm.ROUTE_DEVICE, 0)
    assert sm.expected_route(65_536, True) == (sm.ROUTE_FALLBACK, 1)


@pytest.mark.parametrize("name", sc.NAMES)
def test_codes_equal_the_oracle_over_the_case_table(oracle, name):
    """at MIN_ROWS rows, the fewest at which every case holds every string of its pool; a NULL row reaches the oracle as b"" """
    case = sc.case(name, sc.MIN_ROWS)
    assert set(case.idx.tolist()) == set(range(len(case.pool)))             # every string of the pool is in the column
    strs = case.strs()
    c, nd, first = sm.codes(strs)
    o = oracle.groupby_typed([(ck.STR, [b"" if s is None else s for s in strs])])
    assert nd == o["ngroups"]
    assert np.array_equal(c, o["reversemap"])
    assert np.array_equal(first, o["first_rows"])
    assert case.collides == (len({(sm.hash64(sm.content(s)), len(sm.content(s))) for s in case.pool}) < len({sm.content(s) for s in case.pool}))


def test_case_table_is_what_it_says():
    """the properties the GPU cases lean on, checked where they are made"""
    pool = sc.word_edge_pool()
    assert sorted({len(s) for s in pool}) == list(sc.WORD_EDGE_LENGTHS)
    by_len = {}
    for s in pool:
        by_len.setdefault(len(s), []).append(s)
    for L, ss in by_len.items():
        assert len(ss) == (1 if L == 0 else 2 if L < 9 else 3)
        if L >= 1:
            assert ss[0][:-1] == ss[1][:-1] and ss[0][-1] != ss[1][-1]       # the last byte only
        if L >= 9:
            assert ss[0][1:] == ss[2][1:] and ss[0][0] != ss[2][0]           # byte 0 only
    hl = sc.high_low_pool()
    assert {len(s) for s in hl} == set(range(1, 18)) and all(set(s) <= {0x01, 0x7F, 0x80, 0xFE, 0xFF} for s in hl)
    assert any(a != b and len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 1 and {x for x, y in zip(a, b) if x != y} | {y for x, y in zip(a, b) if x != y} == {0x7F, 0xFF}
               for a in hl for b in hl)
    for n in (sc.MIN_ROWS, 70_003):
        for last_only in (False, True):
            c = sc.case("far_apart_last_only" if last_only else "far_apart_first_and_last", n)
            x = len(c.pool) - 1
            assert np.flatnonzero(c.idx == x).tolist() == ([n - 1] if last_only else [0, n - 1])
            for r in sc.span_edge_rows(n):
                assert np.count_nonzero(c.idx == c.idx[r]) == 1              # a string of its own
        for t in range(1, 16):
            assert {n * t // 16 - 1, n * t // 16, t * (n // 16) - 1, t * (n // 16), t * (n // 16) + 1} <= set(sc.span_edge_rows(n))
    ch = sc.case("chosen_hashes", sc.MIN_ROWS)
    assert set(sc.CHOSEN_HASHES) <= {sm.hash64(s) for s in ch.pool}
    for name in ("null", "empty", "real"):
        c = sc.case("mixed_first_row_" + name, 70_003)
        assert {"null": c.pool[c.idx[0]] is None, "empty": c.pool[c.idx[0]] == b"", "real": bool(c.pool[c.idx[0]])}[name]
    assert sc.case("all_distinct", 70_003).idx.size == len(set(sc.case("all_distinct", 70_003).pool)) == 70_003


def test_codes_sharded_is_codes_of_the_concatenation():
    rng = np.random.default_rng(3)
    case = sc.case("word_edges", sc.MIN_ROWS)
    strs = case.strs() + [None, b"", b"seen-last"]
    want, nd, _ = sm.codes(strs)
    n = len(strs)
    for world in (1, 2, 3, 5):
        for _ in range(5):
            cuts = [0] + sorted(rng.integers(0, n + 1, world - 1).tolist()) + [n]
            shards = [strs[cuts[r]:cuts[r + 1]] for r in range(world)]
            got, gnd = sm.codes_sharded(shards)
            assert gnd == nd and [len(g) for g in got] == [len(s) for s in shards]
            assert np.array_equal(np.concatenate(got), want)
    got, gnd = sm.codes_sharded([[], strs, [], []])                          # empty shards at either end
    assert gnd == nd and [len(g) for g in got] == [0, n, 0, 0] and np.array_equal(got[1], want)
    got, gnd = sm.codes_sharded([[], []])
    assert gnd == 0 and all(g.size == 0 for g in got)
    got, gnd = sm.codes_sharded([[b"b"], [b"a", b"b"], [None, b"a"]])        # a later rank's codes follow the earlier ranks' dictionary
    assert gnd == 3 and [g.tolist() for g in got] == [[0], [1, 0], [2, 1]]


def test_library_exports_the_route_diagnostic():
    from aquery2_amd import capi
    assert set(capi.STR_PROTOTYPES) == {"aqg_str_encode_last"}
    assert (capi.STR_ROUTE_HOST, capi.STR_ROUTE_DEVICE, capi.STR_ROUTE_FALLBACK) == (sm.ROUTE_HOST, sm.ROUTE_DEVICE, sm.ROUTE_FALLBACK)
    assert callable(capi.Device.str_encode_last)
    lib = capi.load_library()
    for name, argtypes in capi.STR_PROTOTYPES.items():
        fn = getattr(lib, name)                                              # AttributeError: the library does not export it
        assert list(fn.argtypes) == argtypes and fn.restype is C.c_int
    with open(os.path.join(os.path.dirname(HERE), "include", "aqg.h")) as f:
        header = f.read()
    assert "int aqg_str_encode_last(" in header
    assert "AQG_STR_ROUTE_HOST = 1, AQG_STR_ROUTE_DEVICE = 2, AQG_STR_ROUTE_FALLBACK = 4" in header
