"""The model of the joins on composite and typed keys (tests/join_keys_model.py) against the one-integer-key model
(tests/join_model.py), against nested loops, and against the REAL reference's equality (the group ids of
tests/golden/ref_golden_keys.json); and aqg_join_tuple_slots, which is host code.  No GPU."""
import json
import os

import numpy as np
import pytest

import checker as ck
import join_keys_model as jkm
import join_model as jm
import keycases

GOLD = {c["name"]: c for c in json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_golden_keys.json")))["cases"]}
KEY_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.bool_]
KINDS = (jkm.INNER, jkm.LEFT, jkm.SEMI, jkm.ANTI)


def one(a):
    return [(ck.tag_of(a), a)]


@pytest.mark.parametrize("dt", KEY_DTYPES, ids=lambda d: np.dtype(d).name)
def test_one_integer_key_equals_the_integer_model(dt):
    rng = np.random.default_rng(61)
    for nb, npr in ((0, 7), (7, 0), (1, 1), (50, 120), (400, 90)):
        if dt == np.bool_:
            build, probe = rng.integers(0, 2, nb).astype(dt), rng.integers(0, 2, npr).astype(dt)
        else:
            info = np.iinfo(dt)
            pool = np.array([info.min, info.max, 0, 1, info.max - 1] + rng.integers(info.min, info.max, 20, dtype=dt, endpoint=True).tolist(), dtype=dt)
            build, probe = rng.choice(pool[:-5], nb).astype(dt), rng.choice(pool, npr).astype(dt)
        pr, br = jkm.pairs(jkm.INNER, one(build), one(probe))
        wp, wb = jm.pairs(build, probe)
        assert pr.dtype == br.dtype == np.uint32 and np.array_equal(pr, wp) and np.array_equal(br, wb), (nb, npr)
        assert jkm.count(jkm.INNER, one(build), one(probe)) == jm.count(build, probe)
        assert np.array_equal(jkm.lookup(one(build), one(probe)), jm.lookup(build, probe))


def brute(build_cols, probe_cols):
    """for every probe row its build rows, by a nested loop over C-like `==` on the raw values"""
    def eq(tag, a, b):
        if tag == ck.DATE: return bytes(a[:4]) == bytes(b[:4])
        if tag == ck.TIME: return bytes(a[:7]) == bytes(b[:7])
        return a == b                                # numpy scalars: NaN != NaN, -0.0 == 0.0
    nb, npr = len(build_cols[0][1]), len(probe_cols[0][1])
    return [[r for r in range(nb) if all(eq(t, bc[r], pc[i]) for (t, bc), (_, pc) in zip(build_cols, probe_cols))] for i in range(npr)]


def small_sides(rng, which):
    nb, npr = 60, 80
    f = np.array([0.0, -0.0, 1.5, np.nan, -np.nan, 2.0], dtype=np.float64)
    t = np.zeros((4, 8), np.uint8); t[:, 0] = [1, 1, 2, 3]; t[:, 6] = [0, 0, 0, 5]
    def side(n, x):                                   # x: the probe side draws from one more value (rows without a partner)
        if which == "two":
            return [(ck.INT32, rng.integers(-1, 1 + x, n).astype(np.int32)), (ck.UINT8, rng.integers(254, 256, n).astype(np.uint8))]
        if which == "three":
            return [(ck.INT8, rng.integers(-1, 1 + x, n).astype(np.int8)), (ck.INT64, rng.choice(np.array([-1, 2**40, 2**40 + 1], np.int64), n)), (ck.BOOL, rng.integers(0, 2, n).astype(np.bool_))]
        if which == "float":
            return [(ck.DOUBLE, rng.choice(f, n)), (ck.INT16, rng.integers(0, 2 + x, n).astype(np.int16))]
        if which == "float32":
            return [(ck.FLOAT, rng.choice(f.astype(np.float32), n))]
        tt = t[rng.integers(0, 4, n)].copy(); tt[:, 7] = rng.integers(0, 256, n)
        return [(ck.TIME, tt), (ck.INT32, rng.integers(0, 2 + x, n).astype(np.int32))]
    return side(nb, 0), side(npr, 1)


@pytest.mark.parametrize("which", ["two", "three", "float", "float32", "time"])
def test_model_equals_a_nested_loop(which):
    build, probe = small_sides(np.random.default_rng(62), which)
    m = brute(build, probe)
    assert sum(len(b) > 0 for b in m) > 10 and sum(len(b) == 0 for b in m) > 5
    assert np.array_equal(jkm.lookup(build, probe), np.array([b[0] if b else jkm.NONE for b in m], np.uint32))
    for kind in KINDS:
        pr, br = jkm.pairs(kind, build, probe)
        if kind == jkm.SEMI:
            want_p, want_b = [i for i, b in enumerate(m) if b], None
        elif kind == jkm.ANTI:
            want_p, want_b = [i for i, b in enumerate(m) if not b], None
        else:
            mm = [b if b or kind == jkm.INNER else [jkm.NONE] for b in m]
            want_p, want_b = [i for i, b in enumerate(mm) for _ in b], [r for b in mm for r in b]
        assert pr.tolist() == want_p and (br is None if want_b is None else br.tolist() == want_b), kind
        assert jkm.count(kind, build, probe) == len(want_p)


def nan_rows(cols):
    bad = np.zeros(len(cols[0][1]), bool)
    for tag, data in cols:
        if tag in (ck.FLOAT, ck.DOUBLE):
            bad |= np.isnan(data)
    return bad


def golden_self_join(name, cols):
    """what the reference's grouping of `cols` says about their self-join: (look-up answers, INNER count)"""
    g = GOLD[name]
    first, rev = np.array(g["first_rows"], np.uint32), np.array(g["reversemap"], np.int64)
    bad = nan_rows(cols)
    want = first[rev]
    want[bad] = jkm.NONE
    sizes = np.bincount(rev[~bad], minlength=g["ngroups"])
    return want, sum((sizes * sizes).tolist())


@pytest.mark.parametrize("name", sorted(GOLD))
def test_model_agrees_with_the_references_equality(name):
    cols = dict(keycases.cases())[name]
    want, cnt = golden_self_join(name, cols)
    assert np.array_equal(jkm.lookup(cols, cols), want)
    assert jkm.count(jkm.INNER, cols, cols) == cnt


def test_tuple_slots_on_the_host():
    """aqg_join_tuple_slots is pure host code: slots within the table, a function of the tuple's VALUE alone"""
    from aquery2_amd import capi
    rng = np.random.default_rng(63)
    n = 4000
    a, b = rng.integers(-5, 5, n).astype(np.int32), rng.integers(0, 3, n).astype(np.uint16)
    for slots in (16, 2048, 1 << 20):
        s = capi.join_tuple_slots([a, b], slots)
        assert s.dtype == np.uint32 and len(s) == n and s.max() < slots
        seen = {}
        for t, v in zip(zip(a.tolist(), b.tolist()), s.tolist()):
            assert seen.setdefault(t, v) == v                # equal tuples, equal slots
    assert len(set(capi.join_tuple_slots([a, b], 1 << 20).tolist())) > 20             # and not one slot for all
    wide = capi.join_tuple_slots([a.astype(np.int64), b], 2048)                       # (int64, uint16): 10 bytes, the WIDE form
    assert wide.max() < 2048 and len(set(wide.tolist())) > 20
    z = np.array([0.0, -0.0, 1.0], np.float64)
    for dt in (np.float64, np.float32):
        s = capi.join_tuple_slots([z.astype(dt), np.array([7, 7, 7], np.int64)], 1 << 16)
        assert s[0] == s[1]
    t = np.zeros((3, 8), np.uint8); t[:, 0] = 9; t[:, 5] = 30; t[1, 7] = 0xAB; t[2, 6] = 1
    s = capi.join_tuple_slots([(ck.TIME, t)], 1 << 30)
    assert s[0] == s[1] and s[0] != s[2]
    ts = np.zeros((2, 12), np.uint8); ts[:, 0] = 3; ts[:, 4] = 9; ts[1, 11] = 0x5A
    s = capi.join_tuple_slots([(ck.TIMESTAMP, ts), a[:2] * 0], 1 << 30)
    assert s[0] == s[1]
    lib = capi.load_library()
    import ctypes as C
    out = np.zeros(3, np.uint32)
    ptr = (C.c_void_p * 1)(z.ctypes.data)
    assert lib.aqg_join_tuple_slots(1, (C.c_int * 1)(ck.STR), ptr, 3, 16, out.ctypes.data) == 2          # AQG_ERR_DTYPE
    assert lib.aqg_join_tuple_slots(1, (C.c_int * 1)(ck.DOUBLE), ptr, 3, 24, out.ctypes.data) == 3       # not a power of two: AQG_ERR_ARG
