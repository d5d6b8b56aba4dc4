"""aqg_quantiles / aqg_grouped_quantiles / aqg_grouped_quantiles_flat (quantile.hip): several ranks of a column, of every group, in one
device radix selection.  Everything goes through the C-ABI and is compared BIT FOR BIT with the numpy model of tests/quantile_model.py;
the slots the model flags (the rank lands on a zero of a group that holds both zeros, or on a NaN) are compared by value.  In every
seeded case the flagged slots are at most 1 % of G * nq -- asserted on the model before the device is asked -- except in the test
written to exercise them (test_mixed_zeros_and_nans).  The cases live in tests/quantile_cases.py; tests/test_quantile_model.py shows
on the CPU that they refuse every listed corruption.

Pass counts: a histogram pass fixes one 8-bit digit of EVERY rank of a group, so no group needs more than ceil(bits / 8) passes over
its rows whatever nq is -- `passes <= itemsize` is the assertion that ranks share passes -- and an all-equal or 0/1 column finishes in
strictly fewer passes than a random one (asserted for the 2-, 4- and 8-byte dtypes: a 1-byte column never needs more than one)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import extremes as ex
import quantile_cases as qc
import quantile_model as qm
from aquery2_amd.capi import (BOOL, I128, INT128, ROUTE_GROUP, ROUTE_SMALL, ROUTE_SPLIT, SEL_LOWER, SEL_UPPER, U128, UINT128,
                              AqgError, DevBuf)
from quantile_cases import DTYPES, PERCENTILES, QLISTS, SMALL_CAP, SMALL_MAX, SPLIT_MIN, WHICH, as_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ROUTES = ROUTE_SMALL | ROUTE_GROUP | ROUTE_SPLIT


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


def flagged_share_ok(flags):
    return flags.sum() * 100 <= max(flags.size, 1) or flags.size < 100 and not flags.any()


def flat_route(n):
    return 0 if n == 0 else ROUTE_SMALL if n <= SMALL_MAX else ROUTE_GROUP if n < SPLIT_MIN else ROUTE_SPLIT


@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
def test_flat_every_size_and_input(dev, dt):
    rng = np.random.default_rng(2000 + DTYPES.index(dt))
    case = 0
    for n in qc.FLAT_SIZES:
        for name, col in qc.flat_inputs(rng, dt, n):
            col = as_model(col)
            s = qm.Sorted(col, np.zeros(n, np.int64), 1) if n else None
            for shift in ((0, 1, 3) if n <= SMALL_MAX + 1 else ((0, 1, 3)[case % 3],)):
                x = upload(dev, col, shift)
                for (nums, den), which in ((q, w) for q in QLISTS for w in WHICH):
                    if n:
                        want, flags = s.quantiles(nums, den, which)
                        want, flags = want[0], flags[0]
                    else:
                        want, flags = qm.flat(col, nums, den, which)
                    assert not flags.any(), "seeded flat inputs keep the ranks off mixed zeros and NaNs"
                    got = dev.quantiles(x, nums, den, which)
                    assert qm.same(got, want, flags), (ex.nm(dt), n, name, shift, nums, den, which, got, want)
                    routes, passes = dev.select_last_routes()
                    assert routes == flat_route(n), (n, routes)
                    assert passes <= max(1, col.dtype.itemsize) and (passes >= 1) == (n > 0), (n, nums, passes)
                assert np.array_equal(x.to_host().view(np.uint8), col.view(np.uint8)), "the input column was modified"
            case += 1


def check_grouped(dev, keys, x, expect_routes=None, layouts=("row", "flat"), qlists=QLISTS):
    gid, G = qm.first_occurrence_ids(*keys)
    xm = as_model(x)
    s = qm.Sorted(xm, gid, G)
    gb = dev.groupby_build(keys)
    assert gb.ngroups == G
    xd = upload(dev, x)
    xf = xf_before = None
    for nums, den in qlists:
        for which in WHICH:
            want, flags = s.quantiles(nums, den, which)
            assert flagged_share_ok(flags), "seeded inputs keep the flagged slots at or below 1 %"
            for layout in layouts:
                if layout == "flat" and xf is None:
                    xf = dev.grouped_flatten(gb, xd, keep=True)
                    if x.dtype == np.bool_:
                        xf._tag = BOOL
                    xf_before = xf.to_host()
                got = dev.grouped_quantiles(gb, xf if layout == "flat" else xd, nums, den, which, flat=layout == "flat")
                assert got.shape == (G, len(nums))
                assert qm.same(got, want, flags), (layout, nums, den, which, np.argwhere(got.view(np.uint8).reshape(G, len(nums), -1).any(axis=2) != want.view(np.uint8).reshape(G, len(nums), -1).any(axis=2))[:5])
                routes, passes = dev.select_last_routes()
                assert 1 <= passes <= xm.dtype.itemsize, (nums, passes)
                if expect_routes is not None:
                    assert routes == expect_routes, (routes, expect_routes)
    assert np.array_equal(xd.to_host().view(np.uint8), xm.view(np.uint8)), "x was modified"
    if xf is not None:
        assert np.array_equal(xf.to_host().view(np.uint8), xf_before.view(np.uint8)), "xflat was modified"
    return gb, xd, s


@pytest.mark.parametrize("dt", [np.dtype(np.float64), np.dtype(np.int16), np.dtype(np.uint32)], ids=ex.nm)
def test_grouped_sizes_at_both_thresholds(dev, dt):
    """all three routes in one call; and grouped_quantiles([1], 2, which) is grouped_median(which) byte for byte"""
    keys, x = qc.threshold_case(dt)
    gb, xd, s = check_grouped(dev, keys, x, expect_routes=ALL_ROUTES)
    for which in WHICH:
        want, flags = s.quantiles([1], 2, which)
        q = dev.grouped_quantiles(gb, xd, [1], 2, which)
        m = dev.grouped_median(gb, xd, which)
        assert not flags.any() and q[:, 0].tobytes() == m.tobytes() == want[:, 0].tobytes(), "quantile 1/2 is not the median"
    gb.destroy()


def test_grouped_run_of_full_small_groups(dev):
    keys, x = qc.tile_border_case()
    check_grouped(dev, keys, x, expect_routes=ROUTE_SMALL)[0].destroy()


@pytest.mark.parametrize("bool_values", [False, True], ids=["f32", "bool"])
def test_grouped_two_key_columns(dev, bool_values):
    keys, x = qc.two_keys_case(bool_values)
    check_grouped(dev, keys, x)[0].destroy()


@pytest.mark.parametrize("seed", qc.SEEDS)
def test_grouped_seeded_shapes(dev, seed):
    keys, x = qc.seeded_case(seed)
    check_grouped(dev, keys, x)[0].destroy()


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_mixed_zeros_and_nans(dev, dt):
    """written to exercise the flagged answers: compared by value"""
    rng = np.random.default_rng(5)
    pool = np.array([0.0, -0.0, np.nan, ex._neg_nan(dt), -1.5, 2.5, -np.inf], dtype=dt)
    nums, den = PERCENTILES
    for n in (5, 300, 70_000):
        mixed = pool[rng.integers(0, len(pool), n)]
        mixed[:4] = pool[:4]                                # both zeros and both NaNs, whatever n is
        for name, col in (("pool", mixed), ("only -0.0", np.full(n, -0.0, dt))):
            for which in WHICH:
                want, flags = qm.flat(col, nums, den, which)
                assert flags.mean() > 0.2 or name == "only -0.0"
                got = dev.quantiles(col, nums, den, which)
                assert qm.same(got, want, flags), (n, name, which, got, want)
                if name == "only -0.0":
                    assert np.all(np.signbit(got)) and not np.any(got)
    n = SPLIT_MIN + 300_000
    keys = np.concatenate([np.zeros(SPLIT_MIN + 9, np.int32), np.ones(5000, np.int32), rng.integers(2, 3000, n - SPLIT_MIN - 5009).astype(np.int32)])
    x = pool[rng.integers(0, len(pool), n)]
    p = rng.permutation(n)
    keys, x = keys[p], x[p]
    gid, G = qm.first_occurrence_ids(keys)
    gb = dev.groupby_build([keys])
    s = qm.Sorted(x, gid, G)
    for which in WHICH:
        want, flags = s.quantiles(nums, den, which)
        assert flags.mean() > 0.2
        assert qm.same(dev.grouped_quantiles(gb, x, nums, den, which), want, flags)
        assert dev.select_last_routes()[0] == ALL_ROUTES
    gb.destroy()


PRELUDE = r'''
import hashlib
import sys
import numpy as np
sys.path.insert(0, "tests")
import aquery2_amd, extremes as ex, quantile_model as qm
gpu = aquery2_amd.Device(0)
rng = np.random.default_rng(91)
nums, den = [0, 1, 5, 25, 50, 75, 95, 100], 100
res = []
for dt in (np.int8, np.uint16, np.int32, np.float32, np.uint64, np.float64):
    keys = rng.integers(0, 37, N).astype(np.int32)
    keys[:LONG] = 5
    x = ex.full_range(rng, np.dtype(dt), N)
    gid, G = qm.first_occurrence_ids(keys)
    gb = gpu.groupby_build([keys])
    for which in (0, 1):
        want, flags = qm.grouped(x, gid, G, nums, den, which)
        assert not flags.any()
        got = gpu.grouped_quantiles(gb, x, nums, den, which)
        assert gpu.select_last_routes()[0] == WANT, gpu.select_last_routes()
        assert qm.same(got, want, flags), (dt, which)
        w1, f1 = qm.flat(x[:FLAT], nums, den, which)
        g1 = gpu.quantiles(x[:FLAT], nums, den, which)
        assert gpu.select_last_routes()[0] == WANT, gpu.select_last_routes()
        assert qm.same(g1, w1, f1)
        res += [got.tobytes().hex(), g1.tobytes().hex()]
print("OK", hashlib.sha256("".join(res).encode()).hexdigest(), flush=True)
'''


def run_pinned(want, env, n, long_group, flat_n):
    head = f"WANT, N, LONG, FLAT = {want}, {n}, {long_group}, {flat_n}\n"
    out = subprocess.run([sys.executable, "-c", head + PRELUDE], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env), cwd=ROOT)
    assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
    return out.stdout.split()[-1]


def test_every_route_alone_gives_the_same_answers():
    """the same small input and eight ranks through one route alone (mask exactly 1, 2, 4) with equal answers, in fresh processes: the
    thresholds are read once.  SMALL cannot take a group above its 512-row cap, so it is compared on an input whose groups fit"""
    group = {"AQG_SELECT_SMALL_MAX": "0", "AQG_SELECT_SPLIT_MIN": "4000000000"}
    split = {"AQG_SELECT_SMALL_MAX": "0", "AQG_SELECT_SPLIT_MIN": "1"}
    small = {"AQG_SELECT_SMALL_MAX": str(SMALL_CAP)}
    assert run_pinned(ROUTE_GROUP, group, 30_011, 9000, 30_011) == run_pinned(ROUTE_SPLIT, split, 30_011, 9000, 30_011), "GROUP and SPLIT disagree"
    fits = (ROUTE_SMALL, small, 9_011, 150, 300), (ROUTE_GROUP, group, 9_011, 150, 300), (ROUTE_SPLIT, split, 9_011, 150, 300)
    a, b, c = (run_pinned(*args) for args in fits)
    assert a == b == c, "SMALL, GROUP and SPLIT disagree"


@pytest.mark.parametrize("dt", [d for d in ex.NUM_DTYPES if d.itemsize >= 2], ids=ex.nm)
@pytest.mark.parametrize("n", [200_003, SPLIT_MIN + 11], ids=["group", "split"])
def test_pass_counts(dev, dt, n):
    rng = np.random.default_rng(300)
    nums, den = PERCENTILES
    passes = {}
    for name, col in (("random", ex.full_range(rng, dt, n)), ("equal", np.repeat(ex.full_range(rng, dt, 1), n)), ("zero-one", rng.integers(0, 2, n).astype(dt))):
        x = upload(dev, col)
        for which in WHICH:
            want, flags = qm.flat(col, nums, den, which)
            assert qm.same(dev.quantiles(x, nums, den, which), want, flags)
            routes, p = dev.select_last_routes()
            assert routes == (ROUTE_GROUP if n < SPLIT_MIN else ROUTE_SPLIT)
            assert 1 <= p <= dt.itemsize, (name, p)
            passes[name] = max(passes.get(name, 0), p)
    print("passes", ex.nm(dt), n, passes)
    assert passes["equal"] < passes["random"], passes
    assert passes["zero-one"] < passes["random"], passes


def test_errors(dev):
    import ctypes as C
    lib = dev.lib
    keys = np.arange(10, dtype=np.int32) % 3
    gb = dev.groupby_build([keys])
    sentinel = np.full(32, 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = dev.to_device(sentinel)
    x = dev.to_device(np.arange(10, dtype=np.int32))
    I32 = 0

    def nums(*v):
        return (C.c_uint32 * max(1, len(v)))(*v)

    def flat(ctx, which, nq, num, den, t, xp, n, with_out=True):
        host = (C.c_ubyte * 128)(*([0x77] * 128))
        rc = lib.aqg_quantiles(ctx, which, nq, num, den, t, xp, n, host if with_out else None)
        assert bytes(host) == b"\x77" * 128, "the host output was written"
        return rc

    for tag, npdt in ((INT128, I128), (UINT128, U128)):
        x16 = dev.to_device(np.zeros(10, npdt))
        assert flat(dev.ctx, SEL_LOWER, 1, nums(1), 2, tag, x16.ptr, 10) == 2             # AQG_ERR_DTYPE
        for fn in (lib.aqg_grouped_quantiles, lib.aqg_grouped_quantiles_flat):
            assert fn(dev.ctx, gb.h, SEL_LOWER, 1, nums(1), 2, tag, x16.ptr, out.ptr) == 2
    bad = [(SEL_LOWER, 0, nums(), 2), (SEL_LOWER, 9, nums(*range(9)), 100), (SEL_LOWER, 1, nums(0), 0), (SEL_LOWER, 2, nums(1, 3), 2),
           (2, 1, nums(1), 2), (-1, 1, nums(1), 2), (SEL_LOWER, 1, None, 2)]
    for which, nq, num, den in bad:                                                    # AQG_ERR_ARG
        assert flat(dev.ctx, which, nq, num, den, I32, x.ptr, 10) == 3, (which, nq, den)
        for fn in (lib.aqg_grouped_quantiles, lib.aqg_grouped_quantiles_flat):
            assert fn(dev.ctx, gb.h, which, nq, num, den, I32, x.ptr, out.ptr) == 3, (which, nq, den)
    assert flat(dev.ctx, SEL_LOWER, 1, nums(1), 2, I32, None, 10) == 3                     # null column
    assert flat(dev.ctx, SEL_LOWER, 1, nums(1), 2, I32, x.ptr, 10, with_out=False) == 3
    assert flat(None, SEL_LOWER, 1, nums(1), 2, I32, x.ptr, 10) == 3
    for fn in (lib.aqg_grouped_quantiles, lib.aqg_grouped_quantiles_flat):
        assert fn(dev.ctx, None, SEL_LOWER, 1, nums(1), 2, I32, x.ptr, out.ptr) == 3
        assert fn(dev.ctx, gb.h, SEL_LOWER, 1, nums(1), 2, I32, None, out.ptr) == 3
        assert fn(dev.ctx, gb.h, SEL_LOWER, 1, nums(1), 2, I32, x.ptr, None) == 3
        assert fn(None, gb.h, SEL_LOWER, 1, nums(1), 2, I32, x.ptr, out.ptr) == 3
    # a fused group-by handle has no reversemap: rejected as the median rejects it
    import checker as ck
    agg = dev.groupby_agg([keys], [ck.RED_SUM], [np.arange(10, dtype=np.int32)])
    for fn in (lib.aqg_grouped_quantiles, lib.aqg_grouped_quantiles_flat):
        assert fn(dev.ctx, agg.h, SEL_LOWER, 1, nums(1), 2, I32, x.ptr, out.ptr) == 3
    with pytest.raises(AqgError) as e:
        dev.grouped_quantiles(agg, x, [1], 2)
    assert e.value.code == 3
    assert np.array_equal(out.to_host(), sentinel), "the output was written"
    # empty inputs
    got = dev.quantiles(np.zeros(0, np.float64), [0, 1, 2], 2)
    assert got.shape == (3,) and not got.view(np.uint8).any() and dev.select_last_routes() == (0, 0)
    gb0 = dev.groupby_build([np.zeros(0, np.int32)])
    assert gb0.ngroups == 0 and dev.grouped_quantiles(gb0, np.zeros(0, np.int32), [1, 2], 2).shape == (0, 2)
    # valid calls on the same handle still work after the refused ones
    want, flags = qm.grouped(np.arange(10, dtype=np.int32), *qm.first_occurrence_ids(keys), [0, 1, 2], 2)
    assert qm.same(dev.grouped_quantiles(gb, x, [0, 1, 2], 2), want, flags)
    gb.destroy()


def _synthetic():
    """host_main's `synthetic` dataset: columns a and c of its LCG"""
    x, a, c = 12345, [], []
    for _ in range(200000):
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        a.append((x >> 33) % 1000)
        c.append((x >> 20) % 97)
    return np.array(a, np.int32), np.array(c, np.int32)


def test_emitted_group_loop_quantiles(tmp_path):
    """the generated group loop `col[g] = quantile(95, 100, c[vecs[g]])` and `quantiles(100, {5, 50, 95}, c[vecs[g]] + a[vecs[g]])`
    (tests/emitted/quantiles.cpp) over host_main's synthetic dataset, 2e5 rows in 1e3 groups: a table column goes through
    aqg_grouped_quantiles once per distinct quantile list, an expression over gathers through ONE aqg_grouped_quantiles_flat for its
    three ranks -- grouped calls for ALL groups, however many there are"""
    from test_gpu_emitted import EM, run
    subprocess.check_call(["make", "-C", EM, "build/quantiles.so", "build/host_main"], stdout=subprocess.DEVNULL)
    a, c = _synthetic()
    gid, G = qm.first_occurrence_ids(a)
    assert G == 1000
    first = np.full(G, len(a), np.int64)
    np.minimum.at(first, gid, np.arange(len(a)))
    run("quantiles.so", "synthetic", "dll_qt", "dll_qt_multi", cwd=str(tmp_path))
    for out in ("qt", "qtm"):
        assert np.array_equal(np.fromfile(tmp_path / f"{out}.out.0", np.int32), a[first])
    s = qm.Sorted(c, gid, G)
    assert np.fromfile(tmp_path / "qt.out.1", np.int32).tobytes() == s.quantiles([95], 100)[0].tobytes()
    assert np.fromfile(tmp_path / "qt.out.2", np.int32).tobytes() == s.quantiles([1], 4)[0].tobytes()
    raw = (tmp_path / "qtm.out.1").read_bytes()
    edt = {4 * 3 * G: np.int32, 8 * 3 * G: np.int64}[len(raw)]                      # the element-wise operators' own result type
    want, flags = qm.grouped(c.astype(edt) + a.astype(edt), gid, G, [5, 50, 95], 100)
    assert not flags.any() and raw == want.tobytes()
    calls, groups = (int(t) for t in (tmp_path / "qt.calls").read_text().split())
    assert groups == G and calls == 2, "one grouped call per quantile list"
    calls, groups = (int(t) for t in (tmp_path / "qtm.calls").read_text().split())
    assert groups == G and calls == 1, "three ranks, one grouped call"
