"""What one shared body for the prefix scans (csrc/scan_prefix.hpp: prefix_reduce_kernel, prefix_scan_kernel, emit) means, stated
between its layouts and writers rather than against the oracle: a grouping of one group scans to the bits of the whole column, a
per-group reduction is the last row of the per-group scan, and the whole-column pass scans its tile aggregates in two levels above
4 * 2048 tiles like the grouped one (test_gpu_grouped_scan_extremes.py test_two_level_carry_scan).
Integer results and min / max are exact arithmetic; floating sums, moments and moving averages take the same bracketing in both
layouts -- the lane's serial loop, block_scan_excl, the tile prefix -- so they are held to bit equality as well."""
import numpy as np
import pytest

import checker as ck
import golden_util as gu
from test_gpu_basic import rand
from test_gpu_edges import view

pytestmark = pytest.mark.gpu
TS = 2048
SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 40_001]        # below, on and above a lane block and a tile; 20 tiles
DTYPES = [np.int8, np.int32, np.int64, np.uint64, np.float32, np.float64]
SCANS = ("sums", "avgs", "mins", "maxs", "vars", "stddevs")
# starts at 0, 1, 2047, 2048, 4096, 4105: on and just before a tile border, a one-row group, one group across ten tiles
GROUP_SIZES = [1, 2046, 1, 2048, 9, 20_000]
N = 40_001
TWO_LEVEL_N = 8194 * TS - 5                            # 8194 tiles > 4 * CH: chunk sums, their scan, chunk scans


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def column(dt, n, seed=0):
    rng = np.random.default_rng(5000 + seed + np.dtype(dt).num)
    return np.round(rng.uniform(-1000, 1000, n), 3).astype(dt) if np.dtype(dt).kind == "f" else rand(rng, dt, n, small=True)


def one_group(gpu, n):
    gb = gpu.groupby_build([np.zeros(n, np.int32)])
    assert gb.ngroups == 1
    return gb


@pytest.mark.parametrize("dt", DTYPES)
def test_one_group_is_the_whole_column(gpu, dt):
    for n in SIZES:
        x = column(dt, n)
        gb = one_group(gpu, n)
        xflat = gpu.grouped_flatten(gb, x, keep=True)
        for name in SCANS:
            op = ck.SCAN_NAMES[name]
            assert gu.same_bits(gpu.grouped_scan(gb, op, xflat, flat=True), gpu.scan(op, xflat)), (name, n, dt)
        if n == N:                                       # a column offset by one element: the scalar path of load_tile_items
            for name in SCANS:
                op = ck.SCAN_NAMES[name]
                assert gu.same_bits(gpu.grouped_scan(gb, op, view(gpu, x, 1), flat=True), gpu.scan(op, view(gpu, x, 1))), (name, dt, "offset by one element")
        gb.destroy()


@pytest.mark.parametrize("dt", [np.int32, np.float64])
def test_one_group_is_the_whole_column_ema(gpu, dt):
    from aquery2_amd.capi import EMA_ADJUSTED, EMA_RECURSIVE
    for n in SIZES:
        x = column(dt, n)
        decay = np.random.default_rng(5100 + n).uniform(0.0, 1.0, n)
        gb = one_group(gpu, n)
        for mode in (EMA_RECURSIVE, EMA_ADJUSTED):
            for kw in ({"alpha": 0.1}, {"decay": decay}):
                got = gpu.grouped_ema(gb, x, mode=mode, flat=True, **kw)
                assert gu.same_bits(got, gpu.ema(x, mode=mode, **kw)), (mode, sorted(kw), n, dt)
        gb.destroy()


@pytest.mark.parametrize("dt", [np.int32, np.int64, np.float64])
def test_grouped_reductions_are_the_scans_last_rows(gpu, dt):
    """grouped_reduce_flat and grouped_scan(flat=True) leave through one writer: sum / avg / min / max of a group are the bits of
    sums / avgs / mins / maxs at the group's last position.  One caveat, the reference's own: `avgs` of an 8-byte integer column starts
    from the group's first row ROUNDED to double (first_row_rounding, the avg8 path of W_AVGS) and `avg` (W_RED_AVG) does not, so the
    two agree only while every group's first row is exact in a double -- as here (small values).  Neither path is to be "fixed" to the
    other (test_gpu_grouped_scan_extremes.py pins the rounding, test_gpu_groupagg_extremes.py the reduction)."""
    sizes = GROUP_SIZES + [N - sum(GROUP_SIZES)]
    gb = gpu.groupby_build([np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)])
    off = gpu.group_offsets(gb)
    assert sorted(np.diff(off.astype(np.int64)).tolist()) == sorted(sizes) and set([0, 1, 2047, 2048, 4096, 4105]) <= set(off.tolist())
    last = off[1:].astype(np.int64) - 1
    xflat = gpu.to_device(column(dt, N, seed=7))
    for red, scan in (("sum", "sums"), ("avg", "avgs"), ("min", "mins"), ("max", "maxs")):
        got = gpu.grouped_reduce_flat(gb, ck.RED_NAMES[red], xflat)
        rows = gpu.grouped_scan(gb, ck.SCAN_NAMES[scan], xflat, flat=True)
        assert gu.same_bits(got, rows[last]), (red, dt)
    gb.destroy()


def test_whole_column_two_level_aggregate_scan(gpu, oracle):
    """aqg_scan over 8194 tiles: launch_agg_scan takes the chunked form for the sums (avgs against the oracle, to the bits) and for the
    moments (vars against the grouping of one group, whose carries go the same way)"""
    n = TWO_LEVEL_N
    x = np.random.default_rng(5200).integers(-128, 128, n).astype(np.int8)
    d = gpu.to_device(x)
    assert gu.same_bits(gpu.scan(ck.SCAN_AVGS, d), oracle.scan(ck.SCAN_AVGS, x, 0))
    gb = one_group(gpu, n)
    assert gu.same_bits(gpu.grouped_scan(gb, ck.SCAN_VARS, d, flat=True), gpu.scan(ck.SCAN_VARS, d))
    gb.destroy()
