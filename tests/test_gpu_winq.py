"""aqg_window_quantiles / aqg_grouped_window_quantiles / aqg_grouped_window_quantiles_flat (window_quantile.hip): moving quantiles of
every row's window, per group and flat.  Everything goes through the C-ABI and is compared BIT FOR BIT with the numpy model of
tests/winq_model.py; the slots the model flags (the rank lands on a zero of a window that holds both zeros, or on a NaN) are compared by
value.  The general cases hold no NaN and no -0.0, so nothing is flagged there -- asserted on the model before the device is asked --
and test_mixed_zeros_and_nans is the one written to exercise the flags.  The cases live in tests/winq_cases.py, placed on the tile
edges the device reports (aqg_window_quantiles_last); tests/test_winq_model.py shows on the CPU that they refuse every planted mistake."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import checker as ck
import extremes as ex
import quantile_model as qm
import winq_cases as wc
import winq_model as wm
from aquery2_amd.capi import I128, INT128, SEL_LOWER, SEL_UPPER, U128, UINT128, WINQ_MAX_W, AqgError, DevBuf
from test_gpu_quantiles import _synthetic, upload
from test_winq_model import golden_cases

pytestmark = pytest.mark.gpu
ERR_DTYPE, ERR_ARG = 2, 3


@pytest.fixture(scope="module")
def dev():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def ts(dev):
    """the rows a workgroup owns, as the device reports them"""
    dev.window_quantiles(np.arange(4, dtype=np.int32), [1], 2, 2)
    tile, halo = dev.window_quantiles_last()
    assert tile >= 2048 and halo == 1
    return tile


def ask_all(dev, s, xd, gb=None, flat=False, what=()):
    """every quantile list and both ranks of one column on the device against the model's windows `s`"""
    for nums, den in wc.QLISTS:
        for which in wc.WHICH:
            want, flags = s.quantiles(nums, den, which)
            assert not flags.any(), "general cases keep the ranks off mixed zeros and NaNs"
            got = dev.window_quantiles(xd, nums, den, s.w, which) if gb is None else dev.grouped_window_quantiles(gb, xd, nums, den, s.w, which, flat=flat)
            assert got.shape == want.shape
            if not wm.same(got, want, flags):
                j, i = np.argwhere(got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,)))[0][:2]
                raise AssertionError((what, s.w, nums, den, which, "plane", j, "row", i, got[j, i], want[j, i]))


FLAT_PARAMS = [(dt, w) for dt in wc.FULL_DTYPES for w in wc.W_ALL] + [(dt, None) for dt in wc.DTYPES if dt not in wc.FULL_DTYPES]


@pytest.mark.parametrize("dt,w", FLAT_PARAMS, ids=lambda v: "all" if v is None else str(v))
def test_flat_grid(dev, ts, dt, w):
    """the full grid of windows x sizes x inputs for INT32 and DOUBLE (a window per case), the reduced grid for the other nine dtypes"""
    for w, n, name, col, shift in wc.flat_grid(dt, ts, ws=None if w is None else (w,)):
        cm = wc.as_model(col)
        x = upload(dev, col, shift)
        ask_all(dev, wm.Windows(cm, w), x, what=(ex.nm(dt), n, name, shift))
        assert dev.window_quantiles_last() == (ts, min(w, n) - 1)
        assert np.array_equal(x.to_host().view(np.uint8), cm.view(np.uint8)), "the input column was modified"


GROUPED_PARAMS = [(dt, w) for dt in wc.GROUPED_DTYPES for w in (wc.GROUPED_W if dt in wc.FULL_DTYPES else (8, 1024))]


@pytest.mark.parametrize("dt,w", GROUPED_PARAMS, ids=str)
def test_grouped_edges_both_layouts(dev, ts, dt, w):
    """group starts on the tile's and the halo's edges, groups of 1, w - 1, w and w + 1 rows, a group over three tiles, extremes beside a
    tame group, G == n and G == 1: x in row layout and in the flat layout"""
    for lay, xflat in wc.grouped_cases(w, ts, dt):
        xm = wc.as_model(xflat)
        s = wm.Windows(xm, w, lay.gid)
        gb = dev.groupby_build([lay.keys])
        assert gb.ngroups == lay.G
        xrow = lay.scatter(xflat)
        xd, xf = upload(dev, xrow, 1), upload(dev, xflat, 3)
        assert np.array_equal(dev.grouped_flatten(gb, xd).view(np.uint8), xm.view(np.uint8))
        ask_all(dev, s, xd, gb, flat=False, what=(lay.name, "row"))
        ask_all(dev, s, xf, gb, flat=True, what=(lay.name, "flat"))
        assert np.array_equal(xd.to_host().view(np.uint8), wc.as_model(xrow).view(np.uint8)), "x was modified"
        assert np.array_equal(xf.to_host().view(np.uint8), xm.view(np.uint8)), "xflat was modified"
        gb.destroy()


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_mixed_zeros_and_nans(dev, ts, dt):
    """written to exercise the flagged answers: compared by value there, bit for bit elsewhere; a window of NaNs returns a NaN, a rank
    on a zero of a window with both zeros returns a zero"""
    n = ts + 700
    x = wc.mixed_column(dt, n)
    lay = wc.Layout("mixed", [1, 2, 5, 300, ts - 308, 700])
    gb = dev.groupby_build([lay.keys])
    for w in (1, 3, 64, 1024):
        for gid in (None, lay.gid):
            s = wm.Windows(x, w, gid)
            for (nums, den), which in ((q, wh) for q in wc.QLISTS for wh in wc.WHICH):
                want, flags = s.quantiles(nums, den, which)
                assert w == 1 or flags.any()
                got = dev.window_quantiles(x, nums, den, w, which) if gid is None else dev.grouped_window_quantiles(gb, x, nums, den, w, which, flat=True)
                assert wm.same(got, want, flags), (w, gid is None, nums, which)
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0, want == 0)
    only = np.full(n, -0.0, dt)
    got = dev.window_quantiles(only, [0, 1, 2], 2, 9)
    assert np.all(np.signbit(got)) and not np.any(got), "a column of -0.0 alone returns -0.0"
    gb.destroy()


@pytest.mark.parametrize("dt", [np.dtype(t) for t in (np.int32, np.float64, np.uint16, np.int64)], ids=ex.nm)
def test_the_ends_are_minw_and_maxw(dev, ts, dt):
    rng = np.random.default_rng(77)
    x = upload(dev, wc.tame(ex.full_range(rng, dt, 2 * ts + 31)))
    for w in (2, 9, 100, 1000):
        got = dev.window_quantiles(x, [0, 5], 5, w, SEL_UPPER)
        assert got[0].tobytes() == dev.scan(ck.SCAN_MINW, x, w).tobytes()
        assert got[1].tobytes() == dev.scan(ck.SCAN_MAXW, x, w).tobytes()


@pytest.mark.parametrize("dt", [np.dtype(t) for t in (np.int8, np.float32, np.uint64)], ids=ex.nm)
def test_a_window_over_the_column_ends_in_its_quantiles(dev, dt):
    rng = np.random.default_rng(78)
    for n in (1, 2, 333, 1024):
        x = upload(dev, wc.tame(ex.full_range(rng, dt, n)))
        for (nums, den), which in ((q, wh) for q in wc.QLISTS for wh in wc.WHICH):
            for w in (n, n + 1, 5000):
                assert dev.window_quantiles(x, nums, den, w, which)[:, -1].tobytes() == dev.quantiles(x, nums, den, which).tobytes()


def test_planes_past_2_to_32_elements(dev):
    """8 planes of 2^29 + 5 one-byte rows: the last plane starts past element 2^31 and ends past 2^32, where a 32-bit j * n + i would wrap.
    w = 2, so plane 0 (num 0) is the least and plane 7 (num den) the greatest of every row and its predecessor"""
    n = (1 << 29) + 5
    block = np.random.default_rng(80).integers(0, 256, (1 << 20) + 7, dtype=np.uint8)
    x = np.tile(block, n // len(block) + 1)[:n]
    out = dev.window_quantiles(x, [0, 1, 1, 1, 1, 1, 1, 2], 2, 2, keep=True)
    prev = np.concatenate([x[:1], x[:-1]])
    for j, want in ((0, np.minimum(x, prev)), (7, np.maximum(x, prev))):
        plane = DevBuf(dev, out.ptr + j * n, np.uint8, n, owned=False)
        assert np.array_equal(plane.to_host(), want), j
    out.free()


def test_window_limit(dev, ts):
    rng = np.random.default_rng(79)
    x100 = rng.integers(-50, 50, 100).astype(np.int32)
    assert dev.window_quantiles(x100, [1, 3], 4, 5000).tobytes() == dev.window_quantiles(x100, [1, 3], 4, 100).tobytes() == wm.windows(x100, 100, [1, 3], 4)[0].tobytes()
    assert dev.window_quantiles_last() == (ts, 99)
    assert WINQ_MAX_W == 1024
    x = rng.integers(-50, 50, 1025).astype(np.int32)
    sentinel = np.full(1025, 0x5A5A5A5A, np.uint32).view(np.int32)
    out = dev.to_device(sentinel)
    with pytest.raises(AqgError) as e:
        dev.window_quantiles(x, [1], 2, 1025, out=out)
    assert e.value.code == ERR_ARG
    with pytest.raises(AqgError):
        dev.window_quantiles(x, [1], 2, 2 ** 32 - 1, out=out)
    keys = np.zeros(1025, np.int32)
    keys[:3] = 1                                             # the limit is min(w, n) of the call, whatever the groups are
    gb = dev.groupby_build([keys])
    for flat in (False, True):
        with pytest.raises(AqgError) as e:
            dev.grouped_window_quantiles(gb, x, [1], 2, 1025, flat=flat, out=out)
        assert e.value.code == ERR_ARG
    assert np.array_equal(out.to_host(), sentinel), "the output was written"
    assert dev.window_quantiles(x, [1], 2, 1024, keep=True, out=out) is out
    assert out.to_host().tobytes() == wm.windows(x, 1024, [1], 2)[0].tobytes()
    assert dev.window_quantiles(x[:1024], [1], 2, 1025).tobytes() == wm.windows(x[:1024], 1024, [1], 2)[0].tobytes()
    gb.destroy()


def test_errors(dev):
    lib = dev.lib
    keys = np.arange(10, dtype=np.int32) % 3
    gb = dev.groupby_build([keys])
    sentinel = np.full(64, 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = dev.to_device(sentinel)
    xbuf = dev.to_device(np.arange(40, dtype=np.int32))
    x = xbuf.ptr
    I32 = 0

    def nums(*v):
        return (C.c_uint32 * max(1, len(v)))(*v)

    def grouped(ctx, h, which, nq, num, den, t, xp, n, w, op):
        return [lib.aqg_grouped_window_quantiles(ctx, h, which, nq, num, den, t, xp, w, op),
                lib.aqg_grouped_window_quantiles_flat(ctx, h, which, nq, num, den, t, xp, w, op)]

    def entries(ctx, h, which, nq, num, den, t, xp, n, w, op):
        """the status of the three entries for one argument list (the grouped ones take their n from the handle)"""
        return [lib.aqg_window_quantiles(ctx, which, nq, num, den, t, xp, n, w, op)] + grouped(ctx, h, which, nq, num, den, t, xp, n, w, op)

    for tag, npdt in ((INT128, I128), (UINT128, U128)):
        x16 = dev.to_device(np.zeros(10, npdt))
        assert entries(dev.ctx, gb.h, SEL_LOWER, 1, nums(1), 2, tag, x16.ptr, 10, 3, out.ptr) == [ERR_DTYPE] * 3
    bad = [(SEL_LOWER, 0, nums(), 2, 3), (SEL_LOWER, 9, nums(*range(9)), 100, 3), (SEL_LOWER, 1, nums(0), 0, 3), (SEL_LOWER, 2, nums(1, 3), 2, 3),
           (2, 1, nums(1), 2, 3), (-1, 1, nums(1), 2, 3), (SEL_LOWER, 1, None, 2, 3), (SEL_LOWER, 1, nums(1), 2, 0)]
    for which, nq, num, den, w in bad:
        assert entries(dev.ctx, gb.h, which, nq, num, den, I32, x, 10, w, out.ptr) == [ERR_ARG] * 3, (which, nq, den, w)
    assert entries(dev.ctx, gb.h, SEL_LOWER, 1, nums(1), 2, I32, None, 10, 3, out.ptr) == [ERR_ARG] * 3          # null column
    assert entries(dev.ctx, gb.h, SEL_LOWER, 1, nums(1), 2, I32, x, 10, 3, None) == [ERR_ARG] * 3                # null output
    assert entries(None, gb.h, SEL_LOWER, 1, nums(1), 2, I32, x, 10, 3, out.ptr) == [ERR_ARG] * 3
    assert grouped(dev.ctx, None, SEL_LOWER, 1, nums(1), 2, I32, x, 10, 3, out.ptr) == [ERR_ARG] * 2
    # out overlapping x: the first plane, the last plane's last element, x inside out
    for op in (x, x + 4 * 9, x - 4 * 19, x - 4):
        assert entries(dev.ctx, gb.h, SEL_LOWER, 2, nums(0, 1), 2, I32, x + 4 * 20, 10, 3, op + 4 * 20) == [ERR_ARG] * 3, op - x
    assert np.array_equal(xbuf.to_host(), np.arange(40, dtype=np.int32)), "a refused call wrote"
    # a fused group-by handle has no reversemap: rejected as the median rejects it
    agg = dev.groupby_agg([keys], [ck.RED_SUM], [np.arange(10, dtype=np.int32)])
    assert grouped(dev.ctx, agg.h, SEL_LOWER, 1, nums(1), 2, I32, x, 10, 3, out.ptr) == [ERR_ARG] * 2
    with pytest.raises(AqgError) as e:
        dev.grouped_window_quantiles(agg, np.arange(10, dtype=np.int32), [1], 2, 3)
    assert e.value.code == ERR_ARG
    assert np.array_equal(out.to_host(), sentinel), "the output was written"
    # empty inputs
    assert dev.window_quantiles(np.zeros(0, np.float64), [0, 1, 2], 2, 5).shape == (3, 0)
    gb0 = dev.groupby_build([np.zeros(0, np.int32)])
    assert gb0.ngroups == 0 and dev.grouped_window_quantiles(gb0, np.zeros(0, np.int32), [1, 2], 2, 4).shape == (2, 0)
    # out right behind x is no overlap, and valid calls on the same handle still work after the refused ones
    assert entries(dev.ctx, gb.h, SEL_LOWER, 2, nums(0, 1), 2, I32, x, 10, 3, x + 4 * 10) == [0] * 3
    xr = np.arange(10, dtype=np.int32)
    want = wm.windows(dev.grouped_flatten(gb, xr), 3, [0, 1, 2], 2, gid=np.sort(keys))[0]
    assert dev.grouped_window_quantiles(gb, xr, [0, 1, 2], 2, 3).tobytes() == want.tobytes()
    gb.destroy()


def test_last_reports_tile_and_halo(dev, ts):
    x = np.arange(50, dtype=np.int16)
    for w, halo in ((1, 0), (7, 6), (50, 49), (51, 49), (4000, 49)):
        dev.window_quantiles(x, [1], 2, w)
        assert dev.window_quantiles_last() == (ts, halo)
    gb = dev.groupby_build([(np.arange(50) % 4).astype(np.int32)])
    dev.grouped_window_quantiles(gb, x, [1], 2, 9)
    assert dev.window_quantiles_last() == (ts, 8)
    t, h = C.c_uint32(), C.c_uint32()
    assert dev.lib.aqg_window_quantiles_last(dev.ctx, None, C.byref(h)) == ERR_ARG and dev.lib.aqg_window_quantiles_last(None, C.byref(t), C.byref(h)) == ERR_ARG
    gb.destroy()


def test_pandas_rolling_quantile_through_the_cabi(dev):
    """tests/golden/winq_pandas_rolling.json: rolling(w, min_periods=1).quantile(q, 'lower' | 'higher'), plain and under groupby.  The
    flat layout lists a group's rows in descending row id, so the grouped questions are put with the rows reversed"""
    for x, by, answers in golden_cases():
        n = len(x)
        if by is not None:
            gb = dev.groupby_build([by[::-1].copy()])
            rows = n - 1 - dev.grouped_flatten(gb, np.arange(n, dtype=np.int32))        # the row of every flat position
            xr = upload(dev, x[::-1].copy())
        else:
            xd = upload(dev, x)
        for w in sorted({k[0] for k in answers}):
            for which in wc.WHICH:
                qs = sorted({k[1:3] for k in answers if k[0] == w and k[3] == which})
                nums, den = [q[0] for q in qs], qs[0][1]
                assert all(q[1] == den for q in qs) and len(nums) <= 8
                got = dev.window_quantiles(xd, nums, den, w, which) if by is None else dev.grouped_window_quantiles(gb, xr, nums, den, w, which)
                for j, num in enumerate(nums):
                    want = answers[(w, num, den, which)]
                    per_row = got[j]
                    if by is not None:
                        per_row = np.empty_like(want)
                        per_row[rows] = got[j]
                    assert per_row.tobytes() == want.tobytes(), (by is None, w, num, den, which)
        if by is not None:
            gb.destroy()


def test_emitted_medianw_and_quantilew(tmp_path):
    """tests/emitted/window_quantiles.cpp over host_main's synthetic dataset, 2e5 rows: `medianw(5, c)` flat through aqg_window_quantiles,
    and the generated group loop `medianw(5, c[vecs[g]])`, `quantilew(20, 9, 10, c[vecs[g]] + a[vecs[g]])` over 1e3 groups through ONE
    aqg_grouped_window_quantiles_flat each, however many groups there are; and `medianw(1100, c)`, a window beyond AQG_WINQ_MAX_W, through
    the header layer's host loop"""
    from test_gpu_emitted import EM, run
    subprocess.check_call(["make", "-C", EM, "build/window_quantiles.so", "build/host_main"], stdout=subprocess.DEVNULL)
    a, c = _synthetic()
    run("window_quantiles.so", "synthetic", "dll_wq_flat", "dll_wq_group", "dll_wq_wide", cwd=str(tmp_path))
    wide = np.fromfile(tmp_path / "wqw.out.0", np.int32)
    assert len(wide) == len(c) and wide[:3000].tobytes() == wm.windows(c[:3000], 1100, [1], 2)[0].tobytes()
    for i in np.random.default_rng(8).integers(3000, len(c), 60):
        assert wide[i] == np.sort(c[i - 1099:i + 1])[(1100 - 1) // 2]
    assert np.fromfile(tmp_path / "wqf.out.0", np.int32).tobytes() == wm.windows(c, 5, [1], 2)[0].tobytes()
    gid, G = qm.first_occurrence_ids(a)
    assert G == 1000
    # the group loop's row lists: groups in first-occurrence order, a group's rows in descending row id (the flat layout)
    order = np.lexsort((-np.arange(len(a)), gid))
    fg = gid[order]
    first = np.full(G, len(a), np.int64)
    np.minimum.at(first, gid, np.arange(len(a)))
    assert np.array_equal(np.fromfile(tmp_path / "wqg.out.0", np.int32), a[first])
    assert np.fromfile(tmp_path / "wqg.out.1", np.int32).tobytes() == wm.windows(c[order], 5, [1], 2, gid=fg)[0].tobytes()
    raw = (tmp_path / "wqg.out.2").read_bytes()
    edt = {4 * len(a): np.int32, 8 * len(a): np.int64}[len(raw)]                    # the element-wise operators' own result type
    want, flags = wm.windows(c[order].astype(edt) + a[order].astype(edt), 20, [9], 10, gid=fg)
    assert not flags.any() and raw == want.tobytes()
    calls, groups = (int(t) for t in (tmp_path / "wqg.calls").read_text().split())
    assert groups == G and calls == 2, "one grouped call per grouped form"
