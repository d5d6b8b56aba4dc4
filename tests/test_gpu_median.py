"""aqg_median / aqg_grouped_median / aqg_grouped_median_flat (select.hip): the lower / upper median by device radix selection.
Everything goes through the C-ABI and is compared BIT FOR BIT with the numpy model of tests/median_model.py; the groups the model's
predicate flags (the rank lands on a zero of a group that holds both zeros, or on a NaN) are compared by value.  In every seeded case
the flagged groups are at most 1 % of the groups -- asserted on the model before the device is asked -- except in the two cases
written to exercise them (test_mixed_zeros_and_nans_flat / _grouped).

Pass counts: a histogram pass fixes one 8-bit digit, so no group needs more than ceil(bits / 8) passes, and a column that is all one
value, or only zeros and ones, must finish in fewer passes than a random column of the same dtype.  One pass is the least any
selection takes, and it is all a one-digit (1-byte) dtype ever needs, so there `fewer` can only be `no more`; the strict
inequality is asserted for the 2-, 4- and 8-byte dtypes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import extremes as ex
import median_model as mm
from aquery2_amd.capi import (BOOL, I128, INT128, ROUTE_GROUP, ROUTE_SMALL, ROUTE_SPLIT, SEL_LOWER, SEL_UPPER, U128, UINT128,
                              AqgError, DevBuf)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL_MAX = 256          # select.hip: AQG_SELECT_SMALL_MAX default (groups ranked in LDS)
SMALL_CAP = 512          # ... and its largest value
SPLIT_MIN = 1 << 20      # select.hip: AQG_SELECT_SPLIT_MIN default (groups cut into chunks)
DTYPES = ex.NUM_DTYPES + [np.dtype(np.bool_)]
SIZES = [0, 1, 2, 3, 63, 64, 65, SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, SPLIT_MIN - 1, SPLIT_MIN, SPLIT_MIN + 1, 1_000_003]
WHICH = (SEL_LOWER, SEL_UPPER)


@pytest.fixture(scope="module")
def dev():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def upload(dev, a, shift=0):
    """the column on the device, `shift` elements off an aligned base; bool columns tagged BOOL"""
    a = np.ascontiguousarray(a)
    host = a.astype(np.uint8) if a.dtype == np.bool_ else a
    base = dev.to_device(np.concatenate([np.zeros(shift, host.dtype), host]))
    buf = DevBuf(dev, base.ptr + shift * host.itemsize, host.dtype, host.size, owned=False)
    buf._base = base
    if a.dtype == np.bool_:
        buf._tag = BOOL
    return buf


def as_model(a):
    return a.astype(np.uint8) if a.dtype == np.bool_ else a


def flat_inputs(rng, dt, n):
    """random full-range values, an all-equal column, two distinct values, sorted both ways, the special values planted"""
    r = ex.full_range(rng, dt, n)
    two = ex.full_range(rng, dt, 2)
    yield "random", r
    yield "equal", np.repeat(ex.full_range(rng, dt, 1), n)
    yield "two", two[rng.integers(0, 2, n)]
    yield "ascending", np.sort(r)
    yield "descending", np.sort(r)[::-1].copy()
    yield "pools", ex.unary_column(dt, n, int(rng.integers(1 << 30)), nan=False)


def flagged_share_ok(flags):
    return flags.sum() * 100 <= max(len(flags), 1) or len(flags) < 100 and not flags.any()


@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
def test_flat_every_size_and_input(dev, dt):
    rng = np.random.default_rng(1000 + DTYPES.index(dt))
    case = 0
    for n in SIZES:
        for name, col in flat_inputs(rng, dt, n):
            col = as_model(col)
            model = mm.flat_both(col) if n else {w: mm.flat(col, w) for w in WHICH}
            assert not any(flag for _, flag in model.values()), "seeded flat inputs keep the rank off mixed zeros and NaNs"
            for shift in ((0, 1, 3) if n <= SMALL_MAX + 1 else ((0, 1, 3)[case % 3],)):
                x = upload(dev, col, shift)
                for which in WHICH:
                    want, flag = model[which]
                    got = dev.median(x, which)
                    assert mm.same(got, want, flag), (ex.nm(dt), n, name, shift, which, got, want)
                    routes, passes = dev.select_last_routes()
                    assert routes == (0 if n == 0 else ROUTE_SMALL if n <= SMALL_MAX else ROUTE_GROUP if n < SPLIT_MIN else ROUTE_SPLIT), (n, routes)
                    assert passes <= max(1, col.dtype.itemsize) and (passes >= 1) == (n > 0), (n, passes)
                assert np.array_equal(x.to_host().view(np.uint8), col.view(np.uint8)), "the input column was modified"
            case += 1


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_mixed_zeros_and_nans_flat(dev, dt):
    """written to exercise the flagged answers: compared by value"""
    rng = np.random.default_rng(5)
    for n in (5, 64, 300, 70_000, SPLIT_MIN + 7):
        zeros = np.where(rng.integers(0, 2, n) == 1, dt.type(-0.0), dt.type(0.0))
        nans = np.where(rng.integers(0, 2, n) == 1, ex._neg_nan(dt), dt.type(np.nan)).astype(dt)
        lows = -np.abs(ex.full_range(rng, dt, n)) - dt.type(1)
        for name, col in (("zeros", zeros), ("nans", nans), ("mostly nans", np.where(np.arange(n) % 3 == 0, lows, nans)),
                          ("zeros in the middle", np.where(np.arange(n) % 5 == 0, lows, np.where(np.arange(n) % 5 == 1, -lows, zeros))),
                          ("only -0.0", np.full(n, -0.0, dt))):
            col = rng.permutation(col.astype(dt))
            for which in WHICH:
                want, flag = mm.flat(col, which)
                assert flag or name == "only -0.0"
                got = dev.median(col, which)
                assert mm.same(got, want, flag), (n, name, which, got, want)
                if name == "only -0.0":
                    assert np.signbit(got)


def check_grouped(dev, keys, x, tagged_bool=False, expect_routes=None, layouts=("row", "flat")):
    gid, G = mm.first_occurrence_ids(*keys)
    xm = as_model(x)
    gb = dev.groupby_build(keys)
    assert gb.ngroups == G
    xd = upload(dev, x)
    xf = None
    out = {}
    model = mm.grouped_both(xm, gid, G)
    for which in WHICH:
        want, flags = model[which]
        assert flagged_share_ok(flags), "seeded inputs keep the flagged groups at or below 1 %"
        for layout in layouts:
            if layout == "flat" and xf is None:
                xf = dev.grouped_flatten(gb, xd, keep=True)
                if x.dtype == np.bool_:
                    xf._tag = BOOL
                xf_before = xf.to_host()
            got = dev.grouped_median(gb, xf if layout == "flat" else xd, which, flat=layout == "flat")
            assert mm.same(got, want, flags), (layout, which, np.flatnonzero(got.view(np.uint8).reshape(G, -1).any(axis=1) != want.view(np.uint8).reshape(G, -1).any(axis=1))[:5])
            routes, passes = dev.select_last_routes()
            assert 1 <= passes <= xm.dtype.itemsize
            if expect_routes is not None:
                assert routes == expect_routes, (routes, expect_routes)
            out[which] = got
    assert np.array_equal(xd.to_host().view(np.uint8), xm.view(np.uint8)), "x was modified"
    if xf is not None:
        assert np.array_equal(xf.to_host().view(np.uint8), xf_before.view(np.uint8)), "xflat was modified"
    gb.destroy()
    return out


def seeded_shape(seed):
    rng = np.random.default_rng(4200 + seed)
    dt = DTYPES[seed % len(DTYPES)]
    n = [1, 2, 777, 5000, 70_001, 300_001, 1_000_003, 2_000_000, 3_000_017, 20_000_000][seed % 10]
    kind = seed % 6
    if kind == 0:
        keys = np.zeros(n, np.int32)                                      # one group
    elif kind == 1:
        keys = rng.permutation(n).astype(np.int32)                        # every row its own group
    elif kind == 2:
        keys = rng.integers(0, max(1, n // 3), n).astype(np.int32)        # a few rows per group
    elif kind == 3:
        keys = rng.integers(0, max(1, n // 200), n).astype(np.int32)      # around the SMALL threshold
    elif kind == 4:
        keys = rng.integers(0, 100, n).astype(np.int32)
    else:
        keys = (rng.integers(0, 1000, n) ** 2 // 1000).astype(np.int32)   # skewed sizes
    return dt, n, keys, rng


@pytest.mark.parametrize("seed", range(30))
def test_grouped_seeded_shapes(dev, seed):
    dt, n, keys, rng = seeded_shape(seed)
    x = ex.full_range(rng, dt, n) if seed % 2 else rng.choice(ex.full_range(rng, dt, 40), n)
    check_grouped(dev, [keys], x, layouts=("row", "flat") if n <= 3_000_017 else ("row",))


def test_grouped_skewed_sizes_take_all_three_routes(dev):
    """one group with half the rows next to 1e5 groups of one to three rows, and a band of mid-sized groups"""
    rng = np.random.default_rng(77)
    small = np.repeat(np.arange(1, 100_001), rng.integers(1, 4, 100_000))
    mid = np.repeat(np.arange(200_000, 200_050), 5000)
    rest = np.concatenate([small, mid])
    keys = rng.permutation(np.concatenate([np.zeros(max(len(rest), SPLIT_MIN + 5), np.int64), rest])).astype(np.int32)
    for dt in (np.dtype(np.float32), np.dtype(np.int64), np.dtype(np.uint8)):
        check_grouped(dev, [keys], ex.full_range(rng, dt, len(keys)), expect_routes=ROUTE_SMALL | ROUTE_GROUP | ROUTE_SPLIT)


def test_grouped_sizes_at_both_thresholds(dev):
    rng = np.random.default_rng(78)
    sizes = [SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, 1, 2, 3, 2047, 2048, 2049, SPLIT_MIN - 1, SPLIT_MIN, SPLIT_MIN + 1, 64, 65, SMALL_MAX] * 2
    keys = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    for dt in (np.dtype(np.float64), np.dtype(np.int16), np.dtype(np.uint32)):
        check_grouped(dev, [keys], ex.full_range(rng, dt, len(keys)), expect_routes=ROUTE_SMALL | ROUTE_GROUP | ROUTE_SPLIT)
    # a run of groups of exactly SMALL_MAX rows: every tile border is straddled
    keys = np.repeat(np.arange(300), SMALL_MAX).astype(np.int32)
    check_grouped(dev, [rng.permutation(keys)], ex.full_range(rng, np.dtype(np.int32), len(keys)), expect_routes=ROUTE_SMALL)


def test_grouped_two_key_columns_and_bool(dev):
    rng = np.random.default_rng(79)
    n = 400_003
    k1, k2 = rng.integers(0, 30, n).astype(np.int16), rng.integers(-5, 5, n).astype(np.int64)
    check_grouped(dev, [k1, k2], ex.full_range(rng, np.dtype(np.float32), n))
    check_grouped(dev, [k1, k2], rng.integers(0, 2, n).astype(np.bool_))


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_mixed_zeros_and_nans_grouped(dev, dt):
    """written to exercise the flagged answers: most groups here are compared by value"""
    rng = np.random.default_rng(80)
    n = 2 * SPLIT_MIN + 300_000
    keys = np.concatenate([np.zeros(SPLIT_MIN + 9, np.int32), np.ones(SPLIT_MIN + 10, np.int32), rng.integers(2, 3000, n - 2 * SPLIT_MIN - 19).astype(np.int32)])
    pool = np.array([0.0, -0.0, np.nan, ex._neg_nan(dt), -1.5, 2.5, -np.inf], dtype=dt)
    x = pool[rng.integers(0, len(pool), n)]
    x[keys == 1] = np.where(rng.integers(0, 4, int((keys == 1).sum())) == 0, dt.type(1.0), ex._neg_nan(dt))
    p = rng.permutation(n)
    keys, x = keys[p], x[p]
    gid, G = mm.first_occurrence_ids(keys)
    gb = dev.groupby_build([keys])
    for which in WHICH:
        want, flags = mm.grouped(x, gid, G, which)
        assert flags.mean() > 0.2
        assert mm.same(dev.grouped_median(gb, x, which), want, flags)
    gb.destroy()


PRELUDE = r'''
import hashlib
import sys
import numpy as np
sys.path.insert(0, "tests")
import aquery2_amd, extremes as ex, median_model as mm
gpu = aquery2_amd.Device(0)
rng = np.random.default_rng(91)
res = []
for dt in (np.int8, np.uint16, np.int32, np.float32, np.uint64, np.float64):
    keys = rng.integers(0, 37, N).astype(np.int32)
    keys[:LONG] = 5
    x = ex.full_range(rng, np.dtype(dt), N)
    gid, G = mm.first_occurrence_ids(keys)
    gb = gpu.groupby_build([keys])
    for which in (0, 1):
        want, flags = mm.grouped(x, gid, G, which)
        assert not flags.any()
        got = gpu.grouped_median(gb, x, which)
        assert gpu.select_last_routes()[0] == WANT, gpu.select_last_routes()
        assert mm.same(got, want, flags), (dt, which)
        w1, f1 = mm.flat(x[:FLAT], which)
        g1 = gpu.median(x[:FLAT], which)
        assert gpu.select_last_routes()[0] == WANT, gpu.select_last_routes()
        assert mm.same(g1, w1, f1)
        res += [got.tobytes().hex(), g1.tobytes().hex()]
print("OK", hashlib.sha256("".join(res).encode()).hexdigest(), flush=True)
'''


def run_pinned(want, env, n, long_group, flat_n):
    head = f"WANT, N, LONG, FLAT = {want}, {n}, {long_group}, {flat_n}\n"
    out = subprocess.run([sys.executable, "-c", head + PRELUDE], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env), cwd=ROOT)
    assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
    return out.stdout.split()[-1]


def test_every_route_alone_gives_the_same_answers():
    """the same small input through one route alone (mask exactly 1, 2, 4) with equal answers, in fresh processes: the thresholds are read
    once.  SMALL cannot take a group above its 512-row cap, so it is compared with GROUP on an input whose groups fit; GROUP and SPLIT
    take any size and are compared on one with a 9000-row group"""
    group = {"AQG_SELECT_SMALL_MAX": "0", "AQG_SELECT_SPLIT_MIN": "4000000000"}
    split = {"AQG_SELECT_SMALL_MAX": "0", "AQG_SELECT_SPLIT_MIN": "1"}
    small = {"AQG_SELECT_SMALL_MAX": str(SMALL_CAP)}
    assert run_pinned(ROUTE_GROUP, group, 30_011, 9000, 30_011) == run_pinned(ROUTE_SPLIT, split, 30_011, 9000, 30_011), "GROUP and SPLIT disagree"
    fits = (ROUTE_SMALL, small, 9_011, 150, 300), (ROUTE_GROUP, group, 9_011, 150, 300), (ROUTE_SPLIT, split, 9_011, 150, 300)
    a, b, c = (run_pinned(*args) for args in fits)
    assert a == b == c, "SMALL, GROUP and SPLIT disagree"


@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
@pytest.mark.parametrize("n", [200_003, SPLIT_MIN + 11], ids=["group", "split"])
def test_pass_counts(dev, dt, n):
    rng = np.random.default_rng(300)
    limit = dt.itemsize                                                   # ceil(bits / 8)
    passes = {}
    for name, col in (("random", ex.full_range(rng, dt, n)), ("equal", np.repeat(ex.full_range(rng, dt, 1), n)), ("zero-one", rng.integers(0, 2, n).astype(dt))):
        for which in WHICH:
            want, flag = mm.flat(as_model(col), which)
            assert mm.same(dev.median(upload(dev, col), which), want, flag)
            routes, p = dev.select_last_routes()
            assert routes == (ROUTE_GROUP if n < SPLIT_MIN else ROUTE_SPLIT)
            assert 1 <= p <= limit, (name, p)
            passes[name] = max(passes.get(name, 0), p)
    print("passes", ex.nm(dt), n, passes)
    if limit > 1 and dt.kind != "b":
        assert passes["equal"] < passes["random"], passes
        assert passes["zero-one"] < passes["random"], passes
    else:
        assert passes["equal"] <= passes["random"] and passes["zero-one"] <= passes["random"], passes


def test_h2o_q6_shape(dev):
    """median(v3), stddev(v3) by id4, id5 (benchmark/h2o/groupby.sql:11-12) at 2e7 rows: the median through aqg_grouped_median and
    the standard deviation through aqg_grouped_reduce on the same handle; group order = first occurrence"""
    import checker as ck
    rng = np.random.default_rng(66)
    n = 20_000_000
    id4, id5 = rng.integers(1, 101, n).astype(np.int32), rng.integers(1, 101, n).astype(np.int32)
    v3 = np.round(rng.uniform(0, 100, n), 2).astype(np.float32)          # h2o: round(runif(N, max=100), 6) read as two decimals here
    gid, G = mm.first_occurrence_ids(id4, id5)
    assert G == 10_000
    gb = dev.groupby_build([id4, id5])
    assert gb.ngroups == G
    first = gb.first_rows()
    assert np.array_equal(gid[first], np.arange(G)) and np.all(np.diff(first.astype(np.int64)) > 0), "group order is first occurrence"
    assert np.array_equal(gb.keys(0, np.int32), id4[first]) and np.array_equal(gb.keys(1, np.int32), id5[first])
    xd = dev.to_device(v3)
    for which in WHICH:
        want, flags = mm.grouped(v3, gid, G, which)
        assert flagged_share_ok(flags)
        assert mm.same(dev.grouped_median(gb, xd, which), want, flags)
        assert dev.select_last_routes()[0] == ROUTE_GROUP
    sd = dev.grouped_reduce(gb, ck.RED_STDDEV, xd)
    order = np.argsort(gid, kind="stable")
    counts = np.bincount(gid, minlength=G)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    # the reference's var (aggregations.h:332-348): s = sum x, q = sum x * x with the product in the column's own type (float), both
    # summed in double; (q - s * s / (n + 1)) / (n + 1).  The device adds the rows of a group in another order, so each moment is within
    # c * 2^-53 of itself relative to the second moment (include/aqg.h, floating sums); q - s * s / (n + 1) cancels, hence a bound
    # relative to q: |var - want| <= q / (c + 1) * c * 2^-50, the form tests/test_gpu_sharded.py uses for moments summed in another order
    s1 = np.add.reduceat(v3[order].astype(np.float64), starts)
    q = np.add.reduceat((v3[order] * v3[order]).astype(np.float64), starts)
    want_var = (q - s1 * s1 / (counts + 1)) / (counts + 1)
    tol = q / (counts + 1) * counts * 2.0 ** -50
    print("q6 stddev: largest |var - want| / tol =", float((np.abs(sd * sd - want_var) / tol).max()))
    assert np.all(np.abs(sd * sd - want_var) <= tol + 4 * np.spacing(want_var)), float((np.abs(sd * sd - want_var) / tol).max())   # (+ the rounding of sqrt, squared again)
    assert np.array_equal(xd.to_host().view(np.uint32), v3.view(np.uint32))
    gb.destroy()


def test_errors(dev):
    import ctypes as C
    lib = dev.lib
    keys = np.arange(10, dtype=np.int32) % 3
    gb = dev.groupby_build([keys])
    sentinel = np.full(4, 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = dev.to_device(sentinel)
    for tag, npdt in ((INT128, I128), (UINT128, U128)):
        x = dev.to_device(np.zeros(10, npdt))
        host = (C.c_ubyte * 16)(*([0x77] * 16))
        assert lib.aqg_median(dev.ctx, SEL_LOWER, tag, x.ptr, 10, host) == 2          # AQG_ERR_DTYPE
        assert bytes(host) == b"\x77" * 16
        for fn in (lib.aqg_grouped_median, lib.aqg_grouped_median_flat):
            assert fn(dev.ctx, gb.h, SEL_LOWER, tag, x.ptr, out.ptr) == 2
        assert np.array_equal(out.to_host(), sentinel), "the output was written"
    x = dev.to_device(np.arange(10, dtype=np.int32))
    host = (C.c_ubyte * 16)()
    assert lib.aqg_median(dev.ctx, SEL_LOWER, 0, None, 10, host) == 3                  # AQG_ERR_ARG: null column
    assert lib.aqg_median(dev.ctx, SEL_LOWER, 0, x.ptr, 10, None) == 3
    assert lib.aqg_median(None, SEL_LOWER, 0, x.ptr, 10, host) == 3
    assert lib.aqg_median(dev.ctx, 2, 0, x.ptr, 10, host) == 3
    for fn in (lib.aqg_grouped_median, lib.aqg_grouped_median_flat):
        assert fn(dev.ctx, None, SEL_LOWER, 0, x.ptr, out.ptr) == 3
        assert fn(dev.ctx, gb.h, SEL_LOWER, 0, None, out.ptr) == 3
        assert fn(dev.ctx, gb.h, SEL_LOWER, 0, x.ptr, None) == 3
        assert fn(dev.ctx, gb.h, 7, 0, x.ptr, out.ptr) == 3
        assert fn(None, gb.h, SEL_LOWER, 0, x.ptr, out.ptr) == 3
    assert lib.aqg_select_last_routes(dev.ctx, None, None) == 3
    assert np.array_equal(out.to_host(), sentinel)
    # a fused group-by handle has no reversemap: rejected like aqg_grouped_scan rejects it
    import checker as ck
    agg = dev.groupby_agg([keys], [ck.RED_SUM], [np.arange(10, dtype=np.int32)])
    with pytest.raises(AqgError) as e:
        dev.grouped_median(agg, x)
    assert e.value.code == 3
    with pytest.raises(AqgError) as e2:
        dev.grouped_scan(agg, ck.SCAN_SUMS, x)
    assert e2.value.code == e.value.code
    # empty inputs
    assert dev.median(np.zeros(0, np.float64)) == 0 and dev.select_last_routes() == (0, 0)
    gb0 = dev.groupby_build([np.zeros(0, np.int32)])
    assert gb0.ngroups == 0 and len(dev.grouped_median(gb0, np.zeros(0, np.int32))) == 0


def test_emitted_group_loop_q6(tmp_path):
    """the generated group loop `out[g] = median(col[vecs[g]])` (tests/emitted/median_q6.cpp) over host_main's h2o9 dataset, 1e7 rows in
    1e4 groups: a table column goes through aqg_grouped_median, an expression over gathers through aqg_grouped_median_flat -- one
    grouped call per aggregate for ALL groups, however many there are"""
    from test_gpu_emitted import EM, _mix, run
    subprocess.check_call(["make", "-C", EM, "build/median_q6.so", "build/host_main"], stdout=subprocess.DEVNULL)
    n = 10_000_000
    i = np.arange(n, dtype=np.uint64)
    id2 = (1 + _mix(i) % np.uint64(100)).astype(np.int32)
    id4 = (1 + _mix(np.uint64(5000000000) + i) % np.uint64(100)).astype(np.int32)
    v1 = (1 + _mix(np.uint64(9000000000) + i) % np.uint64(5)).astype(np.int32)
    v2 = (1 + _mix(np.uint64(13000000000) + i) % np.uint64(15)).astype(np.int32)
    gid, G = mm.first_occurrence_ids(id2, id4)
    first = np.full(G, n, np.int64)
    np.minimum.at(first, gid, np.arange(n))
    run("median_q6.so", "h2o9", "dll_q6", "dll_q6_expr", cwd=str(tmp_path))
    for out in ("q6", "q6e"):
        assert np.array_equal(np.fromfile(tmp_path / f"{out}.out.0", np.int32), id2[first])
        assert np.array_equal(np.fromfile(tmp_path / f"{out}.out.1", np.int32), id4[first])
    want, flags = mm.grouped(v1, gid, G, SEL_LOWER)
    assert np.fromfile(tmp_path / "q6.out.2", np.int32).tobytes() == want.tobytes()
    counts = np.bincount(gid, minlength=G)
    order = np.argsort(gid, kind="stable")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    v = v1[order].astype(np.int64)
    s1, s2 = np.add.reduceat(v, starts), np.add.reduceat(v * v, starts)
    sd = np.fromfile(tmp_path / "q6.out.3", np.float64)
    want_sd = np.sqrt((s2 - s1 * s1 / (counts + 1)) / (counts + 1))            # the reference's formula and divisor (aggregations.h:332-348)
    assert np.allclose(sd, want_sd, rtol=1e-9), np.abs(sd / want_sd - 1).max()
    raw = (tmp_path / "q6e.out.2").read_bytes()
    edt = {4 * G: np.float32, 8 * G: np.float64}[len(raw)]                      # the element-wise operators' own result type
    e = (v1.astype(edt) * edt(0.5) + v2.astype(edt)).astype(edt)               # halves of small integers: exact in either type
    want_e, flags_e = mm.grouped(e, gid, G, SEL_LOWER)
    assert not flags_e.any() and np.frombuffer(raw, edt).tobytes() == want_e.tobytes()
    calls, groups = (int(t) for t in (tmp_path / "q6.calls").read_text().split())
    assert groups == G == 10_000 and calls == 2, "one grouped call for the median, one for the stddev"
    calls, groups = (int(t) for t in (tmp_path / "q6e.calls").read_text().split())
    assert groups == G and calls == 1
