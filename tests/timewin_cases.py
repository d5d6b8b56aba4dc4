"""The named cases of the time-range windows, at the smallest shapes that can break the kernels of aquery2_amd/csrc/range_window.hip.
The geometry -- the radix of the block tree and the tile -- is read from the code here, and tests/test_gpu_timewin.py holds it against
what aqg_rangew_last reports.  Every case is a column in ONE layout: `starts` None (one slice) or the first positions of the groups
of a flat layout; rows() gives the row layout whose build has exactly that flat layout (a group's rows in descending row-id order)."""
import functools
import os
import re
from dataclasses import dataclass

import numpy as np

import timewin_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def geometry():
    """(radix of the block tree, tile rows) from the kernels' constants"""
    def const(src, name):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src)
        return m.group(1).strip()
    rw = open(os.path.join(ROOT, "aquery2_amd", "csrc", "range_window.hip")).read()
    sd = open(os.path.join(ROOT, "aquery2_amd", "csrc", "scan_dev.hpp")).read()
    return int(const(rw, "RX")), int(const(sd, "SB")) * int(const(sd, "IT"))


def levels(n):
    """what aqg_rangew_last reports for a fold of n rows: (nlevels, rows per block at each level)"""
    rx, _ = geometry()
    L, m = 1, n
    while m > rx:
        m = -(-m // rx)
        L += 1
    return L, [min(rx ** (k + 1), 2 ** 32 - 1) for k in range(L)]


@dataclass(eq=False)
class Case:
    name: str
    t: np.ndarray
    x: np.ndarray
    span: float
    frame: int
    starts: object = None            # first positions of the groups in the flat layout
    kind: object = None              # "date" / "time": t is an (n, bytes) uint8 array
    ordered: bool = True

    @property
    def n(self):
        return len(self.t)

    def rows(self):
        """(keys_row, t_row, x_row): group g owns the row ids [starts[g], starts[g+1]), reversed in the flat layout"""
        edges = list(self.starts) + [self.n]
        perm = np.concatenate([np.arange(a, b)[::-1] for a, b in zip(edges[:-1], edges[1:])])
        keys = np.repeat(np.arange(len(self.starts), dtype=np.int32), np.diff(edges))
        return keys, self.t[perm], self.x[perm]


def asc(n, seed, step=9, dtype=np.int64, base=0):
    """irregular non-decreasing stamps with runs of ties"""
    r = np.random.default_rng(seed)
    return (base + np.cumsum(r.integers(0, step + 1, size=n) * (r.random(n) < 0.7))).astype(dtype)


def vals(n, seed, dtype):
    r = np.random.default_rng(seed + 1000)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (r.integers(-2 ** 20, 2 ** 20, size=n) * 2.0 ** r.integers(-30, 30, size=n)).astype(dt)
    info = np.iinfo(dt)
    return r.integers(max(info.min, -2 ** 40), min(info.max, 2 ** 40), size=n, endpoint=True).astype(dt)


def sizes():
    rx, tile = geometry()
    ns = {1, 2, rx - 1, rx, rx + 1, rx * rx - 1, rx * rx, rx * rx + 1, tile - 1, tile, tile + 1, 2 * tile + 1}
    return sorted(ns)


@functools.lru_cache(maxsize=None)
def flat_cases():
    rx, tile = geometry()
    C = []
    dts = [np.int32, np.float64, np.int64, np.float32, np.uint8, np.uint64, np.int16]
    # every n of the grid: a short span (windows inside a block), a span of a few blocks, and one beyond the tile and its predecessor
    for k, n in enumerate(sizes()):
        dt = dts[k % len(dts)]
        t = asc(n, n)
        for span, fr in ((7, tm.OPEN), (40.5, tm.CLOSED), (5.0 * rx * 3, tm.CLOSED), (5.0 * (2 * tile + rx), tm.OPEN)):
            C.append(Case("grid-n%d-s%g-f%d" % (n, span, fr), t, vals(n, n, dt), span, fr))
    n = rx * rx + rx + 5
    t = asc(n, 7)
    # windows of length 1; all-equal stamps (every window is the slice prefix); ties across block edges
    C.append(Case("len1", np.arange(n, dtype=np.int64) * 10, vals(n, 1, np.float64), 3, tm.OPEN))
    C.append(Case("len1-closed0", np.arange(n, dtype=np.int64), vals(n, 1, np.int64), 0, tm.CLOSED))
    C.append(Case("all-equal", np.full(n, 42, np.int32), vals(n, 2, np.int32), 1, tm.OPEN))
    C.append(Case("all-equal-closed0", np.full(n, -5, np.int64), vals(n, 2, np.float64), 0, tm.CLOSED))
    tt = np.repeat(np.arange(-(-n // 48), dtype=np.int64), 48)[:n]          # runs of 48 ties: they straddle every block edge in turn
    C.append(Case("tie-runs", tt, vals(n, 3, np.int16), 1, tm.CLOSED))
    C.append(Case("tie-runs-open", tt, vals(n, 3, np.float32), 1, tm.OPEN))
    # lo and i on, before and after the edges of levels 0 and 1: regular stamps, so that lo = i - w + 1 exactly
    reg = np.arange(2 * rx * rx + 3 * rx, dtype=np.int64)
    for w in (rx - 1, rx, rx + 1, 2 * rx, rx * rx - 1, rx * rx, rx * rx + 1, rx * rx + rx):
        C.append(Case("edges-w%d" % w, reg, vals(len(reg), w, np.int64 if w % 2 else np.float64), w - 1, tm.CLOSED))
    # OPEN against CLOSED with d == span exactly; fractional spans on integer stamps
    t5 = np.arange(300, dtype=np.int64) * 5
    for span in (5, 10, 2.5, 4.999, 5.001, 0.5):
        for fr in (tm.OPEN, tm.CLOSED):
            C.append(Case("exact-s%g-f%d" % (span, fr), t5, vals(300, 4, np.int32), span, fr))
    C.append(Case("exact-unit-open3", np.arange(200, dtype=np.int32), vals(200, 4, np.int8), 3, tm.OPEN))
    tf = np.arange(300, dtype=np.float64) * 0.25
    for fr in (tm.OPEN, tm.CLOSED):
        C.append(Case("exact-fp-f%d" % fr, tf, vals(300, 5, np.float64), 0.75, fr))
        C.append(Case("f32-stamps-f%d" % fr, (np.arange(300) * 0.1).astype(np.float32), vals(300, 6, np.float32), 0.35, fr))
        C.append(Case("f64-irregular-f%d" % fr, np.cumsum(np.random.default_rng(8).random(n)), vals(n, 8, np.float64), 17.25, fr))
    # +Inf: the running aggregates of the slice
    C.append(Case("inf-open", t, vals(n, 9, np.int64), float("inf"), tm.OPEN))
    C.append(Case("inf-closed-fp", t.astype(np.float64), vals(n, 9, np.float64), float("inf"), tm.CLOSED))
    # both ends of int64 / uint64, dmax saturated: t - span would wrap
    i64 = np.iinfo(np.int64)
    te = np.array([i64.min, i64.min + 1, i64.min + 7, -3, 0, 2, i64.max - 9, i64.max - 1, i64.max, i64.max], np.int64)
    xe = np.array([i64.max, i64.max, i64.min, 5, i64.max, i64.min, i64.min, -1, i64.max, i64.max], np.int64)
    for span in (3, 9.5, 2.0 ** 63, 2.0 ** 64, 1e30):
        C.append(Case("int64-ends-s%g" % span, te, xe, span, tm.CLOSED))
        C.append(Case("int64-ends-open-s%g" % span, te, xe, span, tm.OPEN))
    tu = np.array([0, 1, 2, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 3, 2 ** 64 - 1], np.uint64)
    xu = np.array([2 ** 64 - 1, 2 ** 64 - 1, 0, 2 ** 64 - 1, 7, 2 ** 63, 2 ** 64 - 1], np.uint64)
    for span in (2, 2.0 ** 63, 2.0 ** 64):
        C.append(Case("uint64-ends-s%g" % span, tu, xu, span, tm.CLOSED))
    # descending stamps
    C.append(Case("descending", t[::-1].copy(), vals(n, 10, np.int32), 25, tm.OPEN))
    C.append(Case("descending-fp", -np.cumsum(np.random.default_rng(11).random(n)), vals(n, 11, np.float64), 9.5, tm.CLOSED))
    # DATE across a leap day, TIME
    days = [(2024, 2, d) for d in range(20, 30)] + [(2024, 3, d) for d in range(1, 12)] + [(2025, 2, 27), (2025, 2, 28), (2025, 3, 1), (2025, 3, 2)]
    C.append(Case("date-leap", tm.date_col(days), vals(len(days), 12, np.int32), 3, tm.CLOSED, kind="date"))
    C.append(Case("date-leap-open", tm.date_col(days), vals(len(days), 12, np.float64), 3, tm.OPEN, kind="date"))
    tod = [(9, 59, 58, 0), (9, 59, 59, 500), (9, 59, 59, 999), (10, 0, 0, 0), (10, 0, 0, 1), (10, 0, 4, 999), (10, 0, 5, 0), (23, 59, 59, 999)]
    C.append(Case("time", tm.time_col(tod), vals(len(tod), 13, np.int64), 5000, tm.CLOSED, kind="time"))
    C.append(Case("time-open", tm.time_col(tod), vals(len(tod), 13, np.float32), 5000, tm.OPEN, kind="time"))
    # all-negative MAX; MIN / MAX at the ends of the types
    C.append(Case("all-negative", t, -np.abs(vals(n, 14, np.float64)) - 1.0, 30, tm.OPEN))
    C.append(Case("all-negative-int", t, (-np.abs(vals(n, 14, np.int32).astype(np.int64)) - 1).astype(np.int64), 30, tm.OPEN))
    for dt in (np.int8, np.uint8, np.int32, np.uint32, np.int64, np.uint64):
        info = np.iinfo(dt)
        xs = np.array([info.min, info.max, info.min, info.min, info.max, info.max, 0, 1, info.max, info.min] * 20, dt)
        C.append(Case("type-ends-%s" % np.dtype(dt).name, np.arange(len(xs), dtype=np.int64), xs, 2, tm.CLOSED))
    fe = np.array([np.finfo(np.float64).max, -np.finfo(np.float64).max, 5e-324, -5e-324, 1.0, -1.0] * 20)
    C.append(Case("type-ends-float64", np.arange(len(fe), dtype=np.int64), fe, 1, tm.CLOSED))
    # a NaN row, an Inf row and an Inf pair in one window each; the neighbouring windows stay finite and within bound
    xn = vals(n, 15, np.float64)
    xn[100], xn[rx * 5 - 1], xn[rx * 20], xn[rx * 20 + 2] = np.nan, np.inf, np.inf, -np.inf
    xn[rx * 40] = -np.inf
    xn[rx * 30] = 1e300
    C.append(Case("nonfinite", np.arange(n, dtype=np.int64), xn, 3, tm.CLOSED))
    C.append(Case("nonfinite-wide", np.arange(n, dtype=np.int64), xn, rx * 2 + 1, tm.CLOSED))
    with np.errstate(over="ignore"):                                        # (1e300 becomes one more Inf row)
        C.append(Case("nonfinite-f32", np.arange(n, dtype=np.int64), xn.astype(np.float32), 3, tm.CLOSED))
    return C


@functools.lru_cache(maxsize=None)
def grouped_cases():
    rx, tile = geometry()
    C = []

    def grouped(name, sizes_, span, frame, dtype, seed, desc=True, tdtype=np.int64):
        """groups of the given sizes; the stamps ascend in ROW order, so they descend inside every group of the flat layout"""
        n = sum(sizes_)
        starts = np.concatenate([[0], np.cumsum(sizes_)[:-1]]).astype(np.int64)
        t_row = asc(n, seed, dtype=tdtype)
        c = Case(name, t_row, vals(n, seed, dtype), span, frame, starts=starts)
        if desc:                                                            # t above is the ROW layout: bring it into the flat layout
            edges = list(starts) + [n]
            perm = np.concatenate([np.arange(a, b)[::-1] for a, b in zip(edges[:-1], edges[1:])])
            c.t = t_row[perm]
        return c
    # groups that start on block and tile edges; a one-row group between long ones
    C.append(grouped("g-block-edges", [rx, rx, 2 * rx, rx - 1, 1, rx + 1, rx * rx, rx * rx + rx], 30, tm.OPEN, np.int32, 1))
    C.append(grouped("g-tile-edges", [tile, 1, tile - 1, tile, tile + 1, 3], 60.5, tm.CLOSED, np.float64, 2))
    C.append(grouped("g-one-row-between", [3 * tile + 5, 1, 2 * tile + 9], 1e9, tm.CLOSED, np.int64, 3))
    C.append(grouped("g-one-row-between-fp", [tile + 5, 1, rx * rx + 9], float("inf"), tm.OPEN, np.float64, 3, tdtype=np.float64))
    C.append(grouped("g-every-row", [1] * 300, 5, tm.OPEN, np.int16, 4))
    C.append(grouped("g-ascending-flat", [100, 1, 700, rx * rx + 3], 25, tm.OPEN, np.float32, 5, desc=False))
    C.append(grouped("g-many", [int(v) for v in np.random.default_rng(6).integers(1, 40, size=400)], 12, tm.CLOSED, np.int64, 6))
    # a group of 1e30s next to a group of ones: the floating sums of the ones must meet their own bound
    c = grouped("g-1e30-beside-ones", [rx * 3 + 7, rx * rx + 11, 50], 1e9, tm.CLOSED, np.float64, 7)
    c.x = np.concatenate([np.full(rx * 3 + 7, 1e30), np.ones(rx * rx + 11), np.full(50, -1e30)])
    C.append(c)
    c = grouped("g-nan-group", [200, 300, 200], 1e9, tm.CLOSED, np.float64, 8)
    c.x[250] = np.nan
    C.append(c)
    return C


@functools.lru_cache(maxsize=None)
def big_case():
    """a column long enough that the top level of the tree holds two whole elements inside one window: the size comes from the
    geometry, the fourth level's block being the first that no smaller case reaches"""
    rx, tile = geometry()
    n = 3 * rx ** 3 + 3 * rx * rx + 2 * rx + 3
    assert levels(n)[0] == 4
    t = np.arange(n, dtype=np.int64) * 3
    x = np.random.default_rng(99).integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32)
    w = 2 * rx ** 3 + 3 * rx * rx                                           # rows of a full window: it slides over the last third
    return Case("big", t, x, 3.0 * (w - 1), tm.CLOSED)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(lo, Windows) of a case by the search statement of the model: computed once, shared, never changed"""
    fp, st = tm.stamps(case.t, case.kind)
    lo = tm.search_bounds(fp, st, case.starts, case.span, case.frame)
    w = tm.search_windows(case.x, lo)
    lo.setflags(write=False)
    return lo, w
