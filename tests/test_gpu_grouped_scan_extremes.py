"""The per-group scans (aqg_grouped_scan, aqg_grouped_scan_flat, aqg_grouped_flatten: csrc/segscan.hip and the by_group forms of
csrc/scan_window.hpp) at the numeric extremes, on every route, against the oracle's scan of every group's rows.

Layouts, columns, routes and the comparisons are those of tests/grouped_scan_cases.py (its docstring states every bound; the CPU tests
of tests/test_grouped_scan_cases.py show that the comparisons refuse what these kernels could get wrong).  Every op runs through three
entry points whose results have to agree bit for bit before one of them is compared: aqg_grouped_scan on the row-order column, and
aqg_grouped_scan_flat with the flat column and the output each on an aligned address or one element past one, all four pairs (the
vector and the scalar shift kernel; vector and scalar tile loads with vector and scalar stores).

Left out, as in test_gpu_extremes.py: avgw of uint32 / uint64 columns, int32 / int64 columns halved for avgw;
variance data stays inside |x - K| < 2^63 (scan_dev.hpp), i.e. the "offset" and "full" families of test_gpu_variance.py."""
import numpy as np
import pytest

import checker as ck
import exact_moments as em
import extremes as ex
import grouped_scan_cases as gc
from test_gpu_edges import view

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def builds(gpu, oracle):
    """name -> (layout, build); the device's offsets are the layout's"""
    made = {}

    def get(name):
        if name not in made:
            lay = gc.layout(name)
            gb = gpu.groupby_build([lay.keys])
            assert gb.ngroups == lay.G and np.array_equal(gpu.group_offsets(gb), lay.offsets)
            made[name] = (lay, gb)
        return made[name]
    return get


class Column:
    """one flat column on the device in the three forms the entry points take"""

    def __init__(self, gpu, lay, gb, flat):
        self.gpu, self.lay, self.gb, self.flat = gpu, lay, gb, flat
        self.row, self.aligned, self.offset = gpu.to_device(lay.scatter(flat)), gpu.to_device(flat), view(gpu, flat, 1)

    def scan(self, oracle, name, w, what):
        gpu, gb, n = self.gpu, self.gb, self.lay.n
        op = ck.SCAN_NAMES[name]
        a = gpu.grouped_scan(gb, op, self.row, w)
        b = gpu.grouped_scan(gb, op, self.aligned, w, flat=True)
        ot = gc.out_dtype(oracle, name, self.flat.dtype)
        past = lambda: view(gpu, np.zeros(n, ot), 1)
        c = gpu.grouped_scan(gb, op, self.offset, w, flat=True, out=past())
        d = gpu.grouped_scan(gb, op, self.aligned, w, flat=True, out=past())          # vector tile loads, element-at-a-time stores
        e = gpu.grouped_scan(gb, op, self.offset, w, flat=True)                       # and the reverse
        for other, entry in ((b, "aligned column and output"), (c, "column and output one element past an aligned address"),
                             (d, "aligned column, output one element past an aligned address"), (e, "column one element past an aligned address, aligned output")):
            if not ex.same(other, a):
                r = ex.first_diff(other, a)
                raise AssertionError(f"{what} {name} w={w}: flat row {r}: aqg_grouped_scan_flat, {entry}: {other[r]!r}, aqg_grouped_scan {a[r]!r}")
        return a


def cases(fam, dt, lay):
    """[(op, w, route label)] of a family"""
    if fam == "prefix":
        return [(name, 0, "carry") for name in gc.FAMILIES[fam]]
    if fam == "shifts":
        return [(name, 0, "shift") for name in ("deltas", "prev", "aggnext")] + [("ratiow", w, "shift") for w in (gc.RATIO_W if lay.name == "borders" else (1, 7))]
    out = [(name, w, route) for route, w in gc.windows(fam, dt, lay.n) for name in gc.FAMILIES[fam][-2:]]
    return ([(name, 0, "carry") for name in ("vars", "stddevs")] if fam == "variance" else []) + out


def skipped(name, dt):
    return name == "avgw" and dt.kind == "u" and dt.itemsize >= 4              # module docstring


@pytest.mark.parametrize("fam", list(gc.FAMILIES))
@pytest.mark.parametrize("dt", ex.NUM_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("lname", gc.LAYOUTS)
def test_every_op_on_every_route(gpu, oracle, builds, lname, dt, fam):
    lay, gb = builds(lname)
    cols = {}
    for name, w, route in cases(fam, dt, lay):
        if skipped(name, dt):
            continue
        for cname, flat in gc.columns(lay, dt, fam, name):
            key = (cname, name == "avgw")
            if key not in cols:
                cols[key] = (Column(gpu, lay, gb, flat), em.Exact(flat, lay.offsets) if fam == "variance" else None, {})
            col, exact, own = cols[key]
            what = f"{lay.name} {ex.nm(dt)} {cname} [{route}]"
            got = col.scan(oracle, name, w, what)
            want = None if fam == "variance" else gc.expected(oracle, lay, name, flat, w)
            gc.check(name, lay, flat, w, got, want, what, exact, own)


@pytest.mark.parametrize("dt", [np.dtype(np.int64), np.dtype(np.uint64)], ids=ex.nm)
def test_avgs_sums_from_the_groups_first_row_rounded_to_double(gpu, oracle, builds, dt):
    """`s = ret[0] = arr[0]` per group: every first row a double cannot hold as the first flat row of groups of many rows that start on a
    tile border, on a lane-block border, in a tile's last position (its other rows sit in the next tile) and inside a lane block;
    prefix_scan_kernel reads that row back (x[s - 1]) for every later row.  The rows behind it are chosen so that each mean shows
    whether the rounding was carried (grouped_scan_cases.planted_first_rows; the CPU test of the same name shows it start by start)."""
    lay, gb = builds("first-rows")
    for first, flat in gc.planted_first_rows(lay, dt):
        got = Column(gpu, lay, gb, flat).scan(oracle, "avgs", 0, f"first row {first}")
        want = gc.expected(oracle, lay, "avgs", flat)
        for start in gc.FIRST_ROW_STARTS:
            r = gc.same_rows(got, want, gc.planted_rows(lay, start))
            assert r < 0, (int(first), start, r, got[r], want[r])
        gc.check("avgs", lay, flat, 0, got, want, f"first row {first}")


@pytest.mark.parametrize("dt", ex.NUM_DTYPES, ids=ex.nm)
def test_ratiow_short_rule_is_keyed_by_the_window(gpu, oracle, builds, dt):
    """the bitmap of short groups is cached in the handle and keyed by w: two windows in turn on one handle, then the first again"""
    lay, gb = builds("borders")
    flat = gc.columns(lay, dt, "shifts", "ratiow")[0][1]
    col = Column(gpu, lay, gb, flat)
    for w in (7, 100, 7, 2, 100):
        gc.check("ratiow", lay, flat, w, col.scan(oracle, "ratiow", w, "in turn"), gc.expected(oracle, lay, "ratiow", flat, w), "in turn")


@pytest.mark.parametrize("fam", list(gc.FAMILIES))
@pytest.mark.parametrize("dt", ex.NUM_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("lname", gc.LAYOUTS)
def test_a_poisoned_group_changes_no_bit_of_its_neighbours(gpu, oracle, builds, lname, dt, fam):
    """odd-numbered groups of NaN, +-Inf and +-max (integers: the type's ends), even-numbered groups of ordinary values: the even groups'
    rows equal, bit for bit, those of the twin column whose odd groups are zeros -- and the twin's result meets the oracle's composition,
    which sees every group's own rows only"""
    lay, gb = builds(lname)
    bad, twin = gc.poisoned(lay, dt)
    cb, ct = Column(gpu, lay, gb, bad), Column(gpu, lay, gb, twin)
    exact, own = em.Exact(twin, lay.offsets) if fam == "variance" else None, {}
    for name, w, route in cases(fam, dt, lay):
        if skipped(name, dt):
            continue
        what = f"{lay.name} {ex.nm(dt)} [{route}]"
        got_bad, got_twin = cb.scan(oracle, name, w, what + " poisoned"), ct.scan(oracle, name, w, what + " twin")
        gc.check_poisoned(name, lay, twin, w, got_bad, got_twin, None if fam == "variance" else gc.expected(oracle, lay, name, twin, w), what, exact, own)


def test_window_zero_is_rejected_per_group(gpu, builds):
    import aquery2_amd
    lay, gb = builds("borders")
    x = np.arange(lay.n, dtype=np.int32)
    for name in gc.NEEDS_W:
        for flat in (False, True):
            with pytest.raises(aquery2_amd.AqgError):
                gpu.grouped_scan(gb, ck.SCAN_NAMES[name], x, 0, flat=flat)


@pytest.mark.parametrize("dt", [np.int8, np.uint16, np.int32, np.float32, np.uint64, np.float64], ids=ex.nm)
@pytest.mark.parametrize("lname", gc.LAYOUTS)
def test_flatten_moves_bits(gpu, builds, lname, dt):
    """NaN payloads of both signs, -0.0, subnormals, integer patterns with the top bit set: the flat column is x[row_ids], byte for byte"""
    lay, gb = builds(lname)
    x = ex.unary_column(np.dtype(dt), lay.n, 7900)
    assert gpu.grouped_flatten(gb, x).tobytes() == x[lay.row_ids].tobytes()


def test_two_level_carry_scan(gpu):
    """8194 tiles: launch_agg_scan scans the segmented tile carries {value, last start, groups so far} in two levels (chunk sums, their scan,
    chunk scans).  Five groups; one starts on the border between the fourth and the fifth chunk, one on the position before it, one on the
    first position of the last tile.  The flat order is every key run reversed, so the expected values are numpy's."""
    lay = gc.two_level_layout()
    n = lay.n
    assert (n + gc.TS - 1) // gc.TS > gc.TWO_LEVEL_TILES and set(gc.TWO_LEVEL_STARTS) == set(lay.starts().tolist())
    rng = np.random.default_rng(7950)
    flat = rng.integers(-128, 128, n).astype(np.int8)
    flat[lay.starts()] = [100, -100, 127, -128, 3]
    runs = [slice(int(s), int(e)) for s, e in zip(lay.offsets[:-1], lay.offsets[1:])]
    gb = gpu.groupby_build([lay.keys])
    assert gb.ngroups == lay.G and np.array_equal(gpu.group_offsets(gb), lay.offsets)
    d = gpu.grouped_flatten(gb, lay.scatter(flat), keep=True)
    for name, acc in (("mins", np.minimum), ("maxs", np.maximum)):
        got = gpu.grouped_scan(gb, ck.SCAN_NAMES[name], d, flat=True)
        want = np.concatenate([acc.accumulate(flat[r]) for r in runs])
        assert ex.same(got, want), (name, ex.first_diff(got, want))
    sums = [int(flat[r].sum(dtype=np.int64)) for r in runs]
    assert ck.i128_to_int(gpu.grouped_reduce_flat(gb, ck.RED_SUM, d)) == sums
    assert ex.same(gpu.grouped_reduce_flat(gb, ck.RED_AVG, d), np.array([float(s) / float(c) for s, c in zip(sums, lay.sizes)]))
    assert ex.same(gpu.grouped_reduce_flat(gb, ck.RED_MIN, d), np.array([flat[r].min() for r in runs], np.int8))
    assert ex.same(gpu.grouped_reduce_flat(gb, ck.RED_MAX, d), np.array([flat[r].max() for r in runs], np.int8))
    # var: (ssq - s * s / (len + 1)) / (len + 1) with exact integer sums, the reference's formula (prefix_scan_kernel, W_RED_VAR)
    ssq = [int((flat[r].astype(np.int64) ** 2).sum()) for r in runs]
    var = np.array([(float(q) - float(s * s) / float(c + 1)) / float(c + 1) for s, q, c in zip(sums, ssq, lay.sizes.tolist())])
    tol = np.array([4 * 2.0 ** -53 * (q + s * s / (c + 1)) / (c + 1) for s, q, c in zip(sums, ssq, lay.sizes.tolist())])   # four roundings of terms of at most q, s^2 / (len + 1)
    got = gpu.grouped_reduce_flat(gb, ck.RED_VAR, d)
    assert np.all(np.abs(got - var) <= tol), (got, var, tol)
    # a window through HBM: its distance column (position_rows, W_DIST) takes the same carry scan
    w = gc.first_hbm_w(gc.minmax_route, np.int8)
    got = gpu.grouped_scan(gb, ck.SCAN_MINW, d, w, flat=True)
    for r in runs:                                        # behind every start, where the window closes, anywhere, and the group's last rows
        c = r.stop - r.start
        pos = np.unique(np.clip(np.concatenate([np.arange(40), np.arange(w - 3, w + 3), rng.integers(0, c, 50), np.arange(c - 40, c)]), 0, c - 1))
        want = np.array([flat[r.start + max(0, p - w + 1):r.start + p + 1].min() for p in pos.tolist()], np.int8)
        assert ex.same(got[r.start + pos], want), (r, pos[ex.first_diff(got[r.start + pos], want)])
    gb.destroy()
