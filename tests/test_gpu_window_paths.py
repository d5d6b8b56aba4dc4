"""Every branch of the one window dispatch (csrc/scan_window.hpp window_scan) in both layouts -- a whole column (aqg_scan) and the flat
layout of a grouping (aqg_grouped_scan) -- at fixed inputs: the fuzz tests reach the wide-window and LDS paths of the grouped layout
only by the luck of the draw.  The path named next to each window follows from the thresholds of the dispatch:
TS = 2048 rows per tile, ext = 2048 + (w - 1 rounded up to 8), and a tile kernel runs while its LDS fits HALO_MAX_BYTES = 98304:
    minw / maxw   column: ext * 2 * sizeof(T)                  grouped: ext * (2 * sizeof(T) + 2) + 16
    sumw / avgw   column: ext * sizeof(A)                      grouped: ext * sizeof(A) + ext / 8 * 4 + 16
                  (A = 8 bytes for <= 4-byte integers and floating columns, 16 bytes for 8-byte integers)
Comparisons and bounds are those of test_scans_sums, test_gpu_grouped_scan.py and exact_moments.py (tests/window_checks.py)."""
import numpy as np
import pytest

import checker as ck
import exact_moments as em
import golden_util as gu
import window_checks as wc
from test_gpu_basic import rand
from test_gpu_edges import view
from test_gpu_grouped_scan import compose, pos_in_group

pytestmark = pytest.mark.gpu
N = 40_001
DTYPES = [np.int8, np.int32, np.int64, np.float32, np.float64]
# starts at 0, 1, 2047, 2048, 4096, 4105: on and just before a tile border, a one-row group, and one group that crosses ten tiles and
# is longer than every window below
GROUP_SIZES = [1, 2046, 1, 2048, 9, 20_000]

MINMAX_W = [
    2,       # K = 1: one register level, no second span
    3,       # K = 1, off = 1: the second span
    10,      # K = 3: the three register levels, off = 2
    100,     # K = 6: LDS levels 3 .. 5, off = 36
    2047,    # halo 2048 = the tile; ext = 4096: 65536 (column, 8-byte) / 73744 (grouped) bytes, the tile kernel.  An aligned
    2048,    #     column takes van Herk from w = 128 on, so the doubling kernel also gets a column offset by one element
    2049,
    0,       # running form
    N,       # running form
]
# ext = 7048: 112768 bytes for 8-byte elements (grouped 126880): doubling through HBM; van Herk has no C for 8-byte elements and
# a halo of 5000; for 4-byte elements (56384 / 70496) still the tile kernel
MINMAX_WIDE = [(5000, np.int64), (5000, np.float64)]
MINMAX_WIDE_GROUPED = [(30_000, np.int8)]          # ext = 32048: 128208 bytes
SUM_W = [
    2, 10, 64,     # floating columns: direct (w <= 64); integers: the tile kernel
    65, 100,       # the tile kernel (prefix difference) for every type
    2048,          # ext = 4096: 32768 bytes, 65536 for int64 (grouped 34832 / 67600): the tile kernel
]
SUM_WIDE = [(5000, np.int64),        # 16-byte accumulators: 7048 * 16 = 112768 bytes: prefix through HBM
            (12_000, np.float64)]    # ext = 14048: 112384 bytes: prefix through HBM
VAR_W = [2, 8,         # differences in registers (w <= 8)
         9, 64,        # two passes over LDS (w <= 64)
         65, 5000]     # prefix moments through HBM


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def column(dt):
    rng = np.random.default_rng(4000 + np.dtype(dt).num)
    return np.round(rng.uniform(-1000, 1000, N), 3).astype(dt) if np.dtype(dt).kind == "f" else rand(rng, dt, N, small=True)


@pytest.fixture(scope="module")
def grouping(gpu, oracle):
    sizes = GROUP_SIZES + [N - sum(GROUP_SIZES)]
    keys = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    ogb = oracle.groupby([keys])
    assert [int(c) for c in ogb["counts"]] == sizes
    return gpu.groupby_build([keys]), ogb, pos_in_group(ogb, N)


def out_dtype(oracle, op, x):
    return ck.TAG2NP[oracle.scan_out_dtype(op, ck.tag_of(x))]


@pytest.mark.parametrize("dt", DTYPES)
def test_minmax_column(gpu, oracle, dt):
    x = column(dt)
    for w in MINMAX_W + [w for w, d in MINMAX_WIDE if d == dt]:
        for name in ("minw", "maxw"):
            op = ck.SCAN_NAMES[name]
            want = oracle.scan(op, x, w)
            assert gu.same_bits(gpu.scan(op, x, w), want), (name, w, dt)
            if w in (2047, 2048, 2049):
                assert gu.same_bits(gpu.scan(op, view(gpu, x, 1), w), want), (name, w, dt, "offset by one element")


@pytest.mark.parametrize("dt", DTYPES)
def test_minmax_grouped(gpu, oracle, grouping, dt):
    gb, ogb, pos = grouping
    x = column(dt)
    for w in MINMAX_W + [w for w, d in MINMAX_WIDE + MINMAX_WIDE_GROUPED if d == dt]:
        for name in ("minw", "maxw"):
            op = ck.SCAN_NAMES[name]
            want = compose(ogb, x, lambda v: oracle.scan(op, v, w), x.dtype)
            wc.grouped_window(name, dt, gpu.grouped_scan(gb, op, x, w), want, None, pos, (name, w, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_sums_column(gpu, oracle, dt):
    x = column(dt)
    for w in SUM_W + [w for w, d in SUM_WIDE if d == dt]:
        for name in ("sumw", "avgw"):
            op = ck.SCAN_NAMES[name]
            wc.column_sum_scan(name, w, x, gpu.scan(op, x, w), oracle.scan(op, x, w))


@pytest.mark.parametrize("dt", DTYPES)
def test_sums_grouped(gpu, oracle, grouping, dt):
    gb, ogb, pos = grouping
    x = column(dt)
    absx = np.abs(x[ogb["row_ids"]].astype(np.float64))
    for w in SUM_W + [w for w, d in SUM_WIDE if d == dt]:
        for name in ("sumw", "avgw"):
            op = ck.SCAN_NAMES[name]
            want = compose(ogb, x, lambda v: oracle.scan(op, v, w), out_dtype(oracle, op, x))
            wc.grouped_window(name, dt, gpu.grouped_scan(gb, op, x, w), want, absx, pos, (name, w, dt))


@pytest.mark.parametrize("dt", DTYPES)
def test_variances(gpu, oracle, grouping, dt):
    gb, ogb, _ = grouping
    x = column(dt)
    xf = x[ogb["row_ids"]]
    whole, grouped = em.Exact(x), em.Exact(xf, ogb["offsets"])
    for w in VAR_W:
        for name in ("varw", "stddevw"):
            op = ck.SCAN_NAMES[name]
            cheap = N * w <= 3_000_000                         # the oracle walks every window
            wc.variance(whole, name, w, gpu.scan(op, x, w), ("column", name, w, dt), oracle.scan(op, x, w) if cheap else None)
            want = compose(ogb, x, lambda v: oracle.scan(op, v, w), np.float64) if cheap else None
            wc.variance(grouped, name, w, gpu.grouped_scan(gb, op, x, w), ("grouped", name, w, dt), want)


@pytest.mark.parametrize("dt", DTYPES)
def test_one_group_is_the_whole_column(gpu, dt):
    """what the shared kernels state: the flat layout of a single group scans to the bits of the whole-column scan"""
    x = column(dt)
    gb = gpu.groupby_build([np.zeros(N, np.int32)])
    assert gb.ngroups == 1
    xflat = gpu.grouped_flatten(gb, x, keep=True)
    for name in ("minw", "maxw") + (("sumw",) if np.dtype(dt).kind != "f" else ()):
        op = ck.SCAN_NAMES[name]
        for w in (3, 100, 2048, 5000):
            assert gu.same_bits(gpu.grouped_scan(gb, op, xflat, w, flat=True), gpu.scan(op, xflat, w)), (name, w, dt)
