"""aqg_count_distinct / aqg_grouped_count_distinct / aqg_grouped_count_distinct_flat (distinct.hip): count(distinct x) of a column and
of every group of a build.  Everything goes through the C-ABI and must EQUAL the numpy model of tests/distinct_model.py (the size of
the reference's std::unordered_set: -0.0 == +0.0, every NaN row a value of its own) -- integers, no tolerance.

The shapes are built from T = the tile size aqg_distinct_last reports: a group inside one tile is counted by that tile alone, a group
that crosses a tile edge leaves (group, value) pairs for a count-only group-by.  aqg_distinct_last pins which of the two happened.
Group ids follow first occurrence, so keys = repeat(arange(G), sizes) puts group g at flat positions [sum(sizes[:g]), +sizes[g])."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import distinct_model as dm
import extremes as ex
from aquery2_amd.capi import BOOL, I128, INT128, U128, UINT128, AqgError, DevBuf

pytestmark = pytest.mark.gpu
DTYPES = ex.NUM_DTYPES + [np.dtype(np.bool_)]


@pytest.fixture(scope="module")
def dev():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def T(dev):
    t, crossing, pairs = dev.distinct_last()
    assert t >= 64 and t % 64 == 0
    return t


def as_model(a):
    return a.astype(np.uint8) if a.dtype == np.bool_ else a


def upload(dev, a, shift=0):
    """the column on the device, `shift` elements off an aligned base; bool columns tagged BOOL"""
    a = np.ascontiguousarray(a)
    host = as_model(a)
    base = dev.to_device(np.concatenate([np.zeros(shift, host.dtype), host]))
    buf = DevBuf(dev, base.ptr + shift * host.itemsize, host.dtype, host.size, owned=False)
    buf._base = base
    if a.dtype == np.bool_:
        buf._tag = BOOL
    return buf


def through(dt, a):
    """integers carried into the dtype: wrapped for the narrow ones, 0 / 1 for bool"""
    a = np.asarray(a)
    return (a % 2).astype(np.bool_) if dt == np.bool_ else a.astype(dt)


def flat_inputs(rng, dt, n):
    r = ex.full_range(rng, dt, n)
    yield "random", r
    yield "equal", np.repeat(ex.full_range(rng, dt, 1), n)
    yield "two", ex.full_range(rng, dt, 2)[rng.integers(0, 2, n)]
    yield "arange", through(dt, np.arange(n))
    yield "ascending", np.sort(r)
    yield "descending", np.sort(r)[::-1].copy()


@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
def test_flat_every_size_and_input(dev, T, dt):
    rng = np.random.default_rng(2000 + DTYPES.index(dt))
    for n in (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 3 * T + 5, (1 << 20) + 3):
        for name, col in flat_inputs(rng, dt, n):
            want = dm.flat(col)
            for shift in ((0, 1, 3) if n <= 3 * T + 5 else (0,)):
                x = upload(dev, col, shift)
                got = dev.count_distinct(x)
                assert got == want, (ex.nm(dt), n, name, shift, got, want)
                t, crossing, pairs = dev.distinct_last()
                assert t == T and crossing == (1 if n > T else 0) and (pairs > 0) == (n > T), (n, crossing, pairs)
                assert np.array_equal(x.to_host().view(np.uint8), as_model(col).view(np.uint8)), "the input column was modified"


def check_grouped(dev, sizes, x, keys=None):
    """both layouts against the model; returns (crossing groups, pairs) of the row-layout call (the flat one must report the same)"""
    keys = [np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)] if keys is None else keys
    gid, G = dm.first_occurrence_ids(*keys)
    want = dm.grouped(as_model(x), gid, G)
    gb = dev.groupby_build(keys)
    assert gb.ngroups == G
    xd = upload(dev, x)
    got = dev.grouped_count_distinct(gb, xd)
    assert got.dtype == np.uint32 and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    diag = dev.distinct_last()
    xf = dev.grouped_flatten(gb, xd, keep=True)
    if x.dtype == np.bool_:
        xf._tag = BOOL
    before = xf.to_host()
    got = dev.grouped_count_distinct(gb, xf, layout="flat")
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert dev.distinct_last() == diag
    assert np.array_equal(xd.to_host().view(np.uint8), as_model(x).view(np.uint8)), "x was modified"
    assert np.array_equal(xf.to_host().view(np.uint8), before.view(np.uint8)), "xflat was modified"
    gb.destroy()
    return diag[1], diag[2]


def shapes(T):
    """name -> (group sizes in flat order, groups that cross a tile edge)"""
    return {
        "end and start on an edge": ([T, T, 5, T - 5, 1, T - 1, 7], 0),
        "cross one edge": ([100, T, 50], 1),
        "cross three edges": ([7, 3 * T + 1, 9], 1),
        "whole column": ([5 * T + 17], 1),
        "whole column, one tile": ([T], 0),
        "one-row groups fill a tile": ([1] * T + [3] + [1] * (T - 3) + [2, 2], 0),
        "every edge crossed": ([T - 1] + [T] * 4 + [1], 4),
        "crossing groups back to back": ([T // 2, T, T, 3 * T, T // 2], 3),
    }


@pytest.mark.parametrize("dt", [np.dtype(t) for t in (np.int8, np.uint16, np.int32, np.float32, np.uint64, np.float64, np.bool_)], ids=ex.nm)
def test_grouped_tile_shapes(dev, T, dt):
    rng = np.random.default_rng(31)
    for name, (sizes, crossing_want) in shapes(T).items():
        n = int(np.sum(sizes))
        for kind, x in (("narrow", through(dt, rng.integers(0, 7, n))), ("full range", ex.full_range(rng, dt, n))):
            crossing, pairs = check_grouped(dev, sizes, x)
            print(ex.nm(dt), name, kind, crossing, pairs)
            assert crossing == crossing_want, (name, crossing)
            assert (pairs == 0) == (crossing_want == 0), (name, pairs)


def test_no_groups(dev):
    gb0 = dev.groupby_build([np.zeros(0, np.int32)])
    assert gb0.ngroups == 0
    for layout in ("row", "flat"):
        assert len(dev.grouped_count_distinct(gb0, np.zeros(0, np.int32), layout=layout)) == 0
    assert dev.distinct_last()[1:] == (0, 0)


def test_same_value_in_neighbouring_groups_does_not_merge(dev, T):
    # one value everywhere: every group counts it once, the small ones of one tile and the crossing ones alike
    sizes = [3, 1, 5, T, 2, 2, 2 * T, 1]
    n = int(np.sum(sizes))
    for dt in (np.int32, np.float64, np.uint8):
        crossing, pairs = check_grouped(dev, sizes, np.full(n, 7, dt))
        assert crossing == 2
        # a crossing group leaves one pair per tile it touches: T rows from position 9 touch 2 tiles, 2T rows from T + 13 touch 3
        assert pairs == 2 + 3
    # the same few values in every group
    check_grouped(dev, sizes, (np.arange(n) % 3).astype(np.int16))


def test_same_value_in_every_tile_of_a_crossing_group_counts_once(dev, T):
    k = 6
    x = np.tile(np.array([4, 9, 4, 1, 9], np.int64), k * T // 5 + 1)[:k * T]
    crossing, pairs = check_grouped(dev, [k * T], x)
    assert crossing == 1 and pairs == 3 * k                    # three values, every tile of the group sends each once
    x5 = (np.arange(k * T) % 5).astype(np.float32)
    crossing, pairs = check_grouped(dev, [k * T], x5)
    assert crossing == 1 and pairs <= 5 * k
    assert dev.count_distinct(x5) == 5 and dev.distinct_last()[2] <= 5 * k


def test_all_distinct_crossing_group_sends_every_row(dev, T):
    rng = np.random.default_rng(5)
    for dt in (np.int32, np.uint64, np.float32, np.float64):
        big = rng.permutation(4 * T).astype(dt)
        x = np.concatenate([np.zeros(10, dt), big, np.ones(6, dt)])
        crossing, pairs = check_grouped(dev, [10, 4 * T, 6], x)
        assert crossing == 1 and pairs == 4 * T


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_zeros_nans_and_infinities(dev, T, dt):
    rng = np.random.default_rng(17)
    u = np.uint32 if dt.itemsize == 4 else np.uint64
    payload = np.array([0x7FC00001, 0xFFC12345], np.uint32).view(np.float32) if dt.itemsize == 4 else \
        np.array([0x7FF8000000000001, 0xFFF0000000000123], np.uint64).view(np.float64)
    pool = np.concatenate([np.array([0.0, -0.0, np.nan, ex._neg_nan(dt), np.inf, -np.inf, 1.5, -1.5], dtype=dt), payload.astype(dt)])
    assert len(np.unique(pool.view(u))) == len(pool)
    sizes = [1, 2, 3, 9, 2 * T + 11, 40, T, 5, 3 * T, 1]        # small groups, crossing groups, a whole tile
    n = int(np.sum(sizes))
    x = pool[rng.integers(0, len(pool), n)]
    gid = np.repeat(np.arange(len(sizes)), sizes)
    assert np.isnan(x[gid == 4]).sum() > 100, "the crossing group holds many NaN rows: each of them counts"
    check_grouped(dev, sizes, x)
    for name, col in (("only NaNs", np.where(rng.integers(0, 2, n) == 1, ex._neg_nan(dt), dt.type(np.nan)).astype(dt)),
                      ("only -0.0", np.full(n, -0.0, dt)), ("both zeros", np.where(rng.integers(0, 2, n) == 1, dt.type(-0.0), dt.type(0.0)))):
        crossing, pairs = check_grouped(dev, sizes, col)
        want = n if name == "only NaNs" else 1
        assert dev.count_distinct(col) == want == dm.flat(col), name
        if name == "only NaNs":
            assert pairs == 0, "NaN rows never become pairs"


def test_diagnostics_pin_the_algorithm(dev, T):
    rng = np.random.default_rng(3)
    sizes = []
    for tile in range(5):                                        # many small groups, every tile filled exactly: no group crosses an edge
        left = T
        while left:
            c = min(left, int(rng.integers(1, 9)))
            sizes.append(c)
            left -= c
    n = int(np.sum(sizes))
    assert n == 5 * T and len(sizes) > T
    crossing, pairs = check_grouped(dev, sizes, ex.full_range(rng, np.dtype(np.int32), n))
    assert (crossing, pairs) == (0, 0)


def test_errors(dev):
    lib = dev.lib
    keys = np.arange(10, dtype=np.int32) % 3
    gb = dev.groupby_build([keys])
    sentinel = np.full(4, 0x5A5A5A5A, np.uint32)
    out = dev.to_device(sentinel)
    for tag, npdt in ((INT128, I128), (UINT128, U128)):
        x = dev.to_device(np.zeros(10, npdt))
        host = C.c_uint32(0x77777777)
        assert lib.aqg_count_distinct(dev.ctx, tag, x.ptr, 10, C.byref(host)) == 2          # AQG_ERR_DTYPE
        assert host.value == 0x77777777
        for fn in (lib.aqg_grouped_count_distinct, lib.aqg_grouped_count_distinct_flat):
            assert fn(dev.ctx, gb.h, tag, x.ptr, out.ptr) == 2
        assert np.array_equal(out.to_host(), sentinel), "the output was written"
    x = dev.to_device(np.arange(10, dtype=np.int32))
    host = C.c_uint32()
    assert lib.aqg_count_distinct(dev.ctx, 0, None, 10, C.byref(host)) == 3                   # AQG_ERR_ARG: null column
    assert lib.aqg_count_distinct(dev.ctx, 0, x.ptr, 10, None) == 3
    assert lib.aqg_count_distinct(None, 0, x.ptr, 10, C.byref(host)) == 3
    for fn in (lib.aqg_grouped_count_distinct, lib.aqg_grouped_count_distinct_flat):
        assert fn(dev.ctx, None, 0, x.ptr, out.ptr) == 3
        assert fn(dev.ctx, gb.h, 0, None, out.ptr) == 3
        assert fn(dev.ctx, gb.h, 0, x.ptr, None) == 3
        assert fn(None, gb.h, 0, x.ptr, out.ptr) == 3
    assert lib.aqg_distinct_last(dev.ctx, None, None, None) == 3
    # a fused group-by handle has no reversemap: rejected like aqg_grouped_scan rejects it
    import checker as ck
    agg = dev.groupby_agg([keys], [ck.RED_SUM], [np.arange(10, dtype=np.int32)])
    for layout in ("row", "flat"):
        with pytest.raises(AqgError) as e:
            dev.grouped_count_distinct(agg, x, layout=layout, out=out)
        assert e.value.code == 3
    assert np.array_equal(out.to_host(), sentinel)
    assert dev.count_distinct(np.zeros(0, np.float64)) == 0 and dev.distinct_last()[1:] == (0, 0)


@pytest.mark.parametrize("seed", range(int(os.environ.get("AQG_FUZZ_SEEDS", "50"))))
def test_random_cases(dev, T, seed):
    rng = np.random.default_rng(int(os.environ.get("AQG_FUZZ_BASE", "12000")) + seed)
    dt = DTYPES[int(rng.integers(len(DTYPES)))]
    n = int(rng.choice([1, 5, 300, T, T + 1, 5000, 65_537, 200_000, 1 << 18]))
    nkeys = int(rng.integers(1, 4))
    # one dominant group next to many tiny ones, or plain uniform keys
    card = int(rng.choice([1, 3, 40, max(1, n // 50), max(1, n // 3)]))
    keys = []
    for k in range(nkeys):
        col = rng.integers(0, max(1, round(card ** (1 / nkeys)) + 1), n)
        if rng.integers(2):
            col[rng.random(n) < 0.6] = 0                        # the dominant tuple
        keys.append(col.astype([np.int32, np.int16, np.int64, np.uint8][int(rng.integers(4))]))
    width = int(rng.choice([1, 2, 5, 100, 70_000]))             # the value domain
    if rng.integers(3) == 0:
        x = ex.full_range(rng, dt, n)
    else:
        x = through(dt, rng.integers(0, width, n)) if dt.kind != "f" else (rng.integers(-width, width + 1, n) / 2).astype(dt)
    if dt.kind == "f" and rng.integers(2):
        special = np.array([np.nan, ex._neg_nan(dt), -0.0, 0.0, np.inf, -np.inf], dtype=dt)
        hit = rng.random(n) < 0.1
        x[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    if rng.integers(2):
        p = rng.permutation(n)
        keys, x = [k[p] for k in keys], x[p]
    check_grouped(dev, None, x, keys=keys)
    assert dev.count_distinct(x) == dm.flat(as_model(x))


def test_emitted_group_loop_count_distinct(tmp_path):
    """the generated group loop `out[g] = (col[vecs[g]]).distinct_size()` and the flat `(col).distinct_size()`
    (tests/emitted/count_distinct.cpp) over host_main's h2o9 dataset, 1e7 rows in 1e4 groups: a table column goes through
    aqg_grouped_count_distinct, an expression over gathers through aqg_grouped_count_distinct_flat -- one grouped call for ALL
    groups -- and the whole column through aqg_count_distinct"""
    from test_gpu_emitted import EM, _mix, run
    subprocess.check_call(["make", "-C", EM, "build/count_distinct.so", "build/host_main"], stdout=subprocess.DEVNULL)
    n = 10_000_000
    i = np.arange(n, dtype=np.uint64)
    id2 = (1 + _mix(i) % np.uint64(100)).astype(np.int32)
    id4 = (1 + _mix(np.uint64(5000000000) + i) % np.uint64(100)).astype(np.int32)
    v1 = (1 + _mix(np.uint64(9000000000) + i) % np.uint64(5)).astype(np.int32)
    v2 = (1 + _mix(np.uint64(13000000000) + i) % np.uint64(15)).astype(np.int32)
    gid, G = dm.first_occurrence_ids(id2, id4)
    first = np.full(G, n, np.int64)
    np.minimum.at(first, gid, np.arange(n))
    run("count_distinct.so", "h2o9", "dll_cd", "dll_cd_expr", "dll_cd_flat", cwd=str(tmp_path))
    for out in ("cd", "cde"):
        assert np.array_equal(np.fromfile(tmp_path / f"{out}.out.0", np.int32), id2[first])
        assert np.array_equal(np.fromfile(tmp_path / f"{out}.out.1", np.int32), id4[first])
    assert np.array_equal(np.fromfile(tmp_path / "cd.out.2", np.uint32), dm.grouped(v1, gid, G))
    e = v1.astype(np.float64) * 0.5 + v2.astype(np.float64)                    # halves of small integers: exact in float and in double alike
    assert np.array_equal(np.fromfile(tmp_path / "cde.out.2", np.uint32), dm.grouped(e, gid, G))
    assert np.fromfile(tmp_path / "cdf.out.0", np.uint32).tolist() == [dm.flat(v2)] == [15]
    for out in ("cd", "cde"):
        calls, groups = (int(t) for t in (tmp_path / f"{out}.calls").read_text().split())
        assert groups == G == 10_000 and calls == 1, "one grouped call for all groups"
