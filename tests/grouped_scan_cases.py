"""Layouts, columns, routes and comparisons of tests/test_gpu_grouped_scan_extremes.py (a plain module: pytest collects nothing
from it; tests/test_grouped_scan_cases.py holds it to account without a GPU).

LAYOUTS.  Keys are np.repeat(arange(G), sizes): group g owns rows offsets[g] .. offsets[g + 1], and the flat layout lists them in
descending row id, so flat position p of group g is row offsets[g] + offsets[g + 1] - 1 - p.  Columns are written in FLAT order, where
the kernels' tiles, halos and lane blocks are, and scattered into row order: x[row_ids] = flat.

ROUTES.  sum_route / minmax_route / var_route restate the by_group thresholds of window_scan (csrc/scan_window.hpp) and of scan_flat
(csrc/segscan.hip: minw / maxw with w == 0 or w >= n take the running form); test_routes_are_the_ones_named (CPU) asserts that every
window of windows() lands on the route it is named for, so a change of the constants breaks that test.

COMPARISONS.  `check` is the one comparison the GPU tests apply to a device result; the CPU tests apply it to corrupted compositions
of the oracle and expect it to refuse them.
    integers         bit for bit, except
      avgw           the exact window mean of the group's rows to one ulp (test_gpu_extremes.check_int_avgw, per group), and the oracle's
                     recurrence under the bound of check_fp_sums, per group
      var family     exact_moments.Exact with the group offsets (window_checks.variance)
    floating         mins maxs minw maxw deltas prev aggnext ratiow: bit for bit, NaN where NaN (extremes.same)
      sum family     check_fp_sums per group: the row's position in ITS group and the group's cumulative |x|, up to the oracle's first NaN
                     output inside that group (windows); on the direct and tile routes also against the sum of the rows the route adds --
                     the window itself, or the group's rows inside the tile and its halo -- under the bound over those rows of the group
The per-group forms below are written over whole flat columns (a Python loop over ten thousand groups would take seconds per call);
test_vector_forms_are_the_per_group_calls asserts that they decide exactly as check_fp_sums / check_int_avgw called on every group's slice."""
import ctypes as C
import functools

import numpy as np

import checker as ck
import exact_moments as em
import extremes as ex
import window_checks as wc
from test_gpu_extremes import fp_columns, inf_runs_column, int_column
from test_gpu_variance import family

TS = 2048                        # rows per tile (scan_dev.hpp: SB * IT)
HALO_MAX_BYTES = 98304
DIRECT_MAX_W = 64                # floating sumw / avgw up to this long add their rows one by one
VAR_REG_W = 8
VAR_DIRECT_MAX_W = 64
TWO_LEVEL_TILES = 4 * 2048       # launch_agg_scan: more tiles than this take chunk sums + scan + chunk scan

OPS = ("sums", "avgs", "mins", "maxs", "deltas", "prev", "aggnext", "sumw", "avgw", "minw", "maxw", "ratiow", "vars", "stddevs", "varw", "stddevw")
SUM_OPS, VAR_OPS = ("sums", "avgs", "sumw", "avgw"), ("vars", "stddevs", "varw", "stddevw")
NEEDS_W = ("sumw", "avgw", "varw", "stddevw")          # w == 0 is rejected before any launch
FAMILIES = {"prefix": ("sums", "avgs", "mins", "maxs"), "shifts": ("deltas", "prev", "aggnext", "ratiow"), "sumwin": ("sumw", "avgw"),
            "minmaxwin": ("minw", "maxw"), "variance": VAR_OPS}
RATIO_W = (1, 2, 7, 100)


# ---- routes ------------------------------------------------------------------------------------------------------------------------------
def _ext(w):
    return TS + (w - 1 + 7) // 8 * 8                   # tile + halo rounded up to whole blocks of 8


def sum_route(dt, n, w):
    """sumw / avgw per group (window_scan over by_group; scan_flat clamps w at n)"""
    dt = np.dtype(dt)
    w = min(w, n)
    if dt.kind == "f" and w <= DIRECT_MAX_W:
        return "direct"
    acc = 8 if dt.kind == "f" or dt.itemsize <= 4 else 16
    return "tile" if _ext(w) * acc + _ext(w) // 8 * 4 + 16 <= HALO_MAX_BYTES else "hbm"


def minmax_route(dt, n, w):
    """minw / maxw per group: the running form, else doubling -- all levels in registers while 2^K < 16, further levels in LDS, or
    every level through HBM"""
    if w == 0 or w >= n:
        return "running"
    if _ext(w) * (2 * np.dtype(dt).itemsize + 2) + 16 > HALO_MAX_BYTES:
        return "hbm"
    return "registers" if w < 16 else "lds"


def var_route(dt, n, w):
    w = min(w, n)
    return "registers" if w <= VAR_REG_W else "lds" if w <= VAR_DIRECT_MAX_W else "hbm"


ROUTE_OF = {"sumwin": sum_route, "minmaxwin": minmax_route, "variance": var_route}


def first_hbm_w(route, dt, n=1 << 30):
    """the shortest window that `route` sends through HBM"""
    w = 1
    while route(dt, n, w) != "hbm":
        w += 1
    return w


LDS_W = (3, 5, 40, 100, 2500)                          # the windows of the LDS routes below; with RATIO_W: the group lengths of "borders"


def windows(fam, dt, n):
    """[(route name, w)] of a family for one dtype over n rows: one window on every route"""
    dt = np.dtype(dt)
    if fam == "sumwin":
        return ([("direct", 5)] if dt.kind == "f" else []) + [("tile", 100), ("tile", 2500), ("hbm", first_hbm_w(sum_route, dt))]
    if fam == "minmaxwin":
        return [("registers", 3), ("lds", 100), ("lds", 2500), ("hbm", first_hbm_w(minmax_route, dt)), ("running", 0), ("running", n)]
    if fam == "variance":
        return [("registers", 5), ("lds", 40), ("hbm", 100)]
    raise KeyError(fam)


WIDEST_HBM_W = max(first_hbm_w(r, dt) for r in (sum_route, minmax_route) for dt in ex.NUM_DTYPES)


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, name, sizes):
        self.name, self.sizes = name, np.asarray(sizes, np.int64)
        assert np.all(self.sizes > 0)
        self.G, self.n = len(sizes), int(self.sizes.sum())
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)])                # G + 1 entries; flat and row ranges alike
        self.keys = np.repeat(np.arange(self.G, dtype=np.int32), self.sizes)
        self.gid = self.keys.astype(np.int64)                                      # group of every flat position
        self.pos = np.arange(self.n) - self.offsets[self.gid]                      # predecessors inside the group
        self.row_ids = (self.offsets[self.gid] + self.offsets[self.gid + 1] - 1 - np.arange(self.n)).astype(np.uint32)
        self.ogb = dict(ngroups=self.G, counts=self.sizes.astype(np.uint32), offsets=self.offsets[:-1].astype(np.uint32), row_ids=self.row_ids)

    def starts(self):
        return self.offsets[:-1]

    def scatter(self, flat):
        """the row-order column whose flat layout is `flat`"""
        x = np.empty_like(flat)
        x[self.row_ids] = flat
        return x

    def group_at(self, p):
        g = int(np.searchsorted(self.offsets, p, side="right")) - 1
        assert self.offsets[g] == p, (self.name, p)
        return g


BORDER_STARTS = (0, 1, 7, 8, 9, 2047, 2048, 2049, 4096)
BORDER_W = tuple(sorted(set(LDS_W + RATIO_W)))
LONG_GROUP = 22_000                                                                # ten tiles and more, longer than every window of BORDER_W


def _borders():
    sizes = list(np.diff(BORDER_STARTS))
    sizes += [1] * 20 + [2] * 20                                                   # from 4096 on: a run of singletons, a run of pairs
    for w in BORDER_W:
        sizes += [s for s in (w - 1, w, w + 1) if s > 0]
    return Layout("borders", sizes + [LONG_GROUP, 3, 1])


def _wide():
    long_ = WIDEST_HBM_W + 479
    return Layout("wide", [3, long_, 1, 2, 700, long_ + 999, 5])                   # the groups behind a long one start inside every window's reach


def _dense():
    sizes = np.random.default_rng(31).integers(1, 4, 12_000)                       # 1, 2 and 3 mixed: about four starts in every lane block
    return Layout("dense", sizes)


# Groups of MANY rows that start on a tile border (0, 4096, 8192), on a lane-block border (8), in a tile's last position (2047: every
# row behind the first sits in the next tile and learns the start from the tile's carry) and inside a lane block (6149, 8292): where
# prefix_scan_kernel re-reads the group's first row for avgs of 8-byte integers.  (In "borders" the issue's starts 0, 8, 2047 and 2048 are
# followed by starts at 1, 9, 2048 and 2049: one-row groups, whose avgs is the first row rounded whatever the kernel adds.)
FIRST_ROW_STARTS = (0, 8, 2047, 4096, 6149, 8192, 8292)


def _first_rows():
    return Layout("first-rows", list(np.diff(FIRST_ROW_STARTS)) + [3000, 5])


@functools.lru_cache(maxsize=None)
def layout(name):
    return {"borders": _borders, "wide": _wide, "dense": _dense, "first-rows": _first_rows}[name]()


LAYOUTS = ("borders", "wide", "dense")


def compose_flat(lay, xf, fn, out_dtype, left=0, right=0):
    """test_gpu_grouped_scan.compose over a column already in flat order: out[offsets[g] + i] = fn(xf[offsets[g] : offsets[g + 1]])[i].
    left / right > 0 hand fn that many rows of the NEIGHBOURING groups as well and cut its result back: what a kernel that reads across
    a group's border computes (the CPU tests' corruptions; the GPU tests pass 0)."""
    out = np.zeros(lay.n, dtype=out_dtype)
    off = lay.offsets
    for g in range(lay.G):
        s, e = int(off[g]), int(off[g + 1])
        a, b = max(0, s - left), min(lay.n, e + right)
        out[s:e] = fn(xf[a:b])[s - a:s - a + e - s]
    return out


def out_dtype(oracle, name, dt):
    return ck.TAG2NP[oracle.scan_out_dtype(ck.SCAN_NAMES[name], ex.tag(dt))]


def expected(oracle, lay, name, xf, w=0, **kw):
    """the oracle's scan of every group's rows, laid out by the offsets: compose(ogb, x, lambda v: oracle.scan(op, v, w), ot) of
    test_gpu_grouped_scan.py.  Without corruptions (**kw of compose_flat) the oracle reads every group's rows and writes its results in
    place in the flat buffers -- the same calls without an allocation and a copy for each of ten thousand groups."""
    op, ot = ck.SCAN_NAMES[name], out_dtype(oracle, name, xf.dtype)
    left, right = kw.pop("left", 0), kw.pop("right", 0)
    assert not kw, kw
    xf = np.ascontiguousarray(xf)
    out = np.zeros(lay.n, dtype=ot)
    t, xp, outp, isz, osz = ex.tag(xf.dtype), xf.ctypes.data, out.ctypes.data, xf.itemsize, ot.itemsize
    tmp = np.zeros(int(lay.sizes.max()) + left + right, dtype=ot)              # (corruptions: the oracle scans the group and its neighbours' rows into here)
    tmpp = tmp.ctypes.data
    for s, c in zip(lay.offsets[:-1].tolist(), lay.sizes.tolist()):
        a, b = max(0, s - left), min(lay.n, s + c + right)
        direct = a == s and b == s + c
        oracle.scan_at(op, t, xp + a * isz, b - a, w, outp + s * osz if direct else tmpp)
        if not direct:
            out[s:s + c] = tmp[s - a:s - a + c]
    return out


def group_accumulate(lay, a, ufunc=np.add):
    """ufunc.accumulate over every group's rows, row after row as np.cumsum goes: groups of up to 8 rows all at once, one step per
    position in the group; longer groups one by one"""
    out = np.array(a, copy=True)
    small = lay.sizes <= 8
    srow = small[lay.gid]
    for j in range(1, 8):
        idx = np.nonzero(srow & (lay.pos == j))[0]
        if len(idx):
            out[idx] = ufunc(out[idx - 1], a[idx])
    for g in np.nonzero(~small)[0]:
        s, e = int(lay.offsets[g]), int(lay.offsets[g + 1])
        out[s:e] = ufunc.accumulate(a[s:e])
    return out


def trail_grouped(lay, a, k):
    """sum of the last min(k, rows of the group so far) values of `a` at every flat position, in double, groups apart"""
    out = np.zeros(lay.n)
    small = lay.sizes <= 8
    srow = small[lay.gid]
    for j in range(min(k, 8)):                                                     # short groups: one pass per lag over all of them
        take = np.nonzero(srow & (lay.pos >= j))[0]
        out[take] += a[take - j]
    swv = np.lib.stride_tricks.sliding_window_view
    for g in np.nonzero(~small)[0]:
        s, e = int(lay.offsets[g]), int(lay.offsets[g + 1])
        kk = min(k, e - s)
        out[s:e] = swv(np.concatenate([np.zeros(kk - 1), a[s:e]]), kk).sum(axis=1)
    return out


# ---- columns (flat order) ---------------------------------------------------------------------------------------------------------------------
def seed_of(lay, dt, k=0):
    return 7000 + 100 * (LAYOUTS + ("first-rows",)).index(lay.name) + 10 * k + ex.NUM_DTYPES.index(np.dtype(dt))


def one_sign_columns(lay, dt):
    """8-byte integers: all max (all min), a 1 every seventh row -- the 128-bit running sum carries (borrows) on every row and every group
    start has to clear it"""
    ii = np.iinfo(dt)
    cols = []
    for v in (ii.max,) + ((ii.min,) if dt.kind == "i" else ()):
        x = np.full(lay.n, v, dtype=dt)
        x[::7] = 1
        cols.append((f"all-{v}", x))
    return cols


def tie_breaker(first):
    """the smallest second row after which the exact sum and the sum that starts from `first` rounded to double round to different doubles:
    the running mean of the very next row tells whether the rounding of the first row was carried"""
    f, r = int(first), int(float(first))
    for k in range(1, 1 << 13):
        for x1 in ((k, -k) if f < 0 else (k,)):
            if float(f + x1) != float(r + x1):
                return x1
    raise AssertionError(first)


QUIET_ROWS = 2100                                                                  # more than a tile: zeros behind the first two rows


def planted_first_rows(lay, dt):
    """[(first row, column)] over the "first-rows" layout: every value a double cannot hold as the first flat row of the groups that start
    at FIRST_ROW_STARTS, followed by the row that makes the exact sum and the sum from the rounded first row round apart, and then by
    zeros for up to 2100 rows -- so every one of those rows, in the group's first tile and in the next, in every lane block, has a mean
    that tells whether the first row's rounding was carried"""
    cols = []
    for k, first in enumerate(ex.unrepresentable_first_rows(dt)):
        x = ex.unary_column(dt, lay.n, seed_of(lay, dt, 5) + k)
        for p in FIRST_ROW_STARTS:
            c = int(lay.sizes[lay.group_at(p)])
            x[p:p + min(c, QUIET_ROWS)] = 0
            x[p], x[p + 1] = first, dt.type(tie_breaker(first))
        cols.append((first, x))
    return cols


def planted_rows(lay, start):
    """the flat rows of the group that starts at `start`, behind its first row (the first row's mean is the row itself, rounded)"""
    return (lay.gid == lay.group_at(start)) & (lay.pos >= 1)


def inf_columns(lay, dt):
    """inf_runs_column of both signs, with further runs that begin exactly at a group start and runs that end with a group's last row"""
    cols = []
    st = lay.starts()
    picks = st[:: max(1, lay.G // 12)][1:]
    for sign in (1.0, -1.0):
        x = inf_runs_column(dt, lay.n, seed_of(lay, dt, 1), sign)
        a, b = dt.type(sign * np.inf), dt.type(-sign * np.inf)
        for k, s in enumerate(picks):
            s = int(s)
            if k % 2 == 0:
                x[s:min(lay.n, s + 5)] = a if k % 4 == 0 else b                     # begins where the group does
            else:
                x[max(0, s - 5):s] = a if k % 4 == 1 else b                         # ends with the last row of the group in front
        cols.append(("inf%+d" % sign, x))
    return cols


def ramps(lay, dt):
    """full range, but every group of more than 300 rows climbs from the type's min to its max over its first half and comes down again over
    its second; the groups longer than every window ("wide") climb, or come down, from end to end in turn.  The min of a window inside a
    climb (the max inside a descent) is its OLDEST row, so a window one row too long or too short shows -- over thousands of full-range
    rows of a narrow type every window holds the type's ends and no window length can be told from another"""
    x = ex.unary_column(dt, lay.n, seed_of(lay, dt, 7))
    ii = np.iinfo(dt)
    lo, span = int(ii.min), int(ii.max) - int(ii.min)
    climb = lambda h: np.array([lo + k * span // (h - 1) for k in range(h)], dtype=object).astype(dt)
    whole = 0
    for g in np.nonzero(lay.sizes > 300)[0]:
        s, c = int(lay.offsets[g]), int(lay.sizes[g])
        if c > WIDEST_HBM_W + 2:
            x[s:s + c] = climb(c)[::1 if whole % 2 == 0 else -1]
            whole += 1
        else:
            h = c // 2
            x[s:s + h] = climb(h)
            x[s + c - h:s + c] = climb(h)[::-1]
    return x


def columns(lay, dt, fam, name=None):
    """[(label, flat column)] a family of ops is run on"""
    dt = np.dtype(dt)
    n = lay.n
    if fam == "variance":
        rng = np.random.default_rng(seed_of(lay, dt, 4))
        return [(f, family(rng, f, dt, n)) for f in ("offset", "full")]
    if dt.kind != "f":
        cols = [("full-range", int_column(dt, n, seed_of(lay, dt), name))]
        if name in ("mins", "maxs", "minw", "maxw"):
            cols.append(("ramps", ramps(lay, dt)))
        if dt.itemsize == 8 and name in ("sums", "avgs", "sumw"):
            cols += one_sign_columns(lay, dt)
        if dt.itemsize == 8 and name == "avgw":
            cols += one_sign_columns(lay, dt)[:1]                                  # (all max: arr[i] - arr[i-w] stays inside the type)
        return cols
    if name in ("mins", "maxs", "minw", "maxw"):
        return inf_columns(lay, dt)
    if name in SUM_OPS:
        return list(fp_columns(dt, n, seed_of(lay, dt, 2)))
    return [("specials", ex.unary_column(dt, n, seed_of(lay, dt, 3)))]            # shifts and ratiow: NaNs, both zeros, subnormals, infinities


def poisoned(lay, dt):
    """(poisoned, twin) flat columns: ordinary values in the even-numbered groups; the odd-numbered groups hold NaN, +Inf, -Inf and +-max
    (integers: the type's max, every other one its min, so sums wrap and 16-byte accumulators carry) in the first column, zeros in the twin.
    Unsigned types: min is the twin's zero -- a zero that leaks changes the poisoned result and the twin's alike, and the twin's then misses
    the oracle's composition, which check_poisoned holds it to"""
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed_of(lay, dt, 6))
    base = family(rng, "full", dt, lay.n)
    odd = lay.gid % 2 == 1
    twin = base.copy()
    twin[odd] = 0
    bad = base.copy()
    if dt.kind == "f":
        fm = np.finfo(dt).max
        bad[odd] = np.array([np.nan, np.inf, -np.inf, fm, -fm], dtype=dt)[np.arange(lay.n) % 5][odd]
    else:
        ii = np.iinfo(dt)
        lo = odd & (lay.gid % 4 == 3)
        bad[odd] = ii.max
        bad[lo] = ii.min
    assert ex.same(bad[~odd], twin[~odd]) and lay.G >= 3
    return bad, twin


# ---- comparisons -------------------------------------------------------------------------------------------------------------------------
def _fail(name, w, what, r, lay, msg):
    g = int(lay.gid[r])
    raise AssertionError(f"{what} {name} w={w}: flat row {r} (group {g}, row {int(lay.pos[r])} of {int(lay.sizes[g])}): {msg}")


def fp_sums_bad(name, got, want, xf, lay, w):
    """(rows that miss, rows that count, got, want, bound) of check_fp_sums(name, got[s:e], want[s:e], xf[s:e], w) for every group (s, e) at once: the bound (i + 1) eps sum|x| with i the row's
    position in its group and the sum over the group's rows so far; windows stop at the oracle's first NaN output INSIDE the group"""
    i = lay.pos.astype(np.float64)
    absx = np.abs(xf.astype(np.float64))
    absx[~np.isfinite(absx)] = 0.0
    eps = 2.0 ** -23 if (name == "avgw" and xf.dtype == np.float32) else 2.0 ** -52
    bound = (i + 1) * eps * group_accumulate(lay, absx)
    if name == "avgs":
        bound /= i + 1
    if name == "avgw":
        bound /= np.minimum(i + 1, w)
    g, t = got.astype(np.float64), want.astype(np.float64)
    live = np.ones(lay.n, bool)
    if name in ("sumw", "avgw") and np.isnan(t).any():
        live = ~group_accumulate(lay, np.isnan(t), np.maximum)
    fin, inf, nan = np.isfinite(t), np.isinf(t), np.isnan(t)
    with np.errstate(invalid="ignore"):
        bad = live & ((fin & ~(np.abs(g - t) <= bound)) | (inf & (g != t)) | (nan & ~np.isnan(g)))
    return bad, live, g, t, bound


def fp_sums_grouped(name, got, want, xf, lay, w, what=""):
    bad, live, g, t, bound = fp_sums_bad(name, got, want, xf, lay, w)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        _fail(name, w, what, r, lay, f"device {g[r]!r}, oracle {t[r]!r}, bound {bound[r]!r}")
    return live


def int_avgw_bad(got, xf, lay, w):
    """(rows that miss, exact means) of check_int_avgw(got[s:e], xf[s:e], w) for every group at once: the exact sum of the window's rows -- of the row's own group --
    rounded to double once, divided by the window's length, to one ulp"""
    c = np.concatenate([[0], np.cumsum(xf.astype(np.int64))]) if xf.dtype.itemsize < 8 else np.concatenate([np.array([0], dtype=object), np.cumsum(xf.astype(object))])
    ln = np.minimum(lay.pos + 1, w)
    hi = np.arange(lay.n) + 1
    exact = (c[hi] - c[hi - ln]).astype(np.float64) / ln
    return ~(np.abs(got - exact) <= np.spacing(np.abs(exact))), exact


def int_avgw_grouped(got, xf, lay, w, what=""):
    bad, exact = int_avgw_bad(got, xf, lay, w)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        _fail("avgw", w, what, r, lay, f"device {got[r]!r}, exact mean {exact[r]!r}")


def own_rows(lay, xf, w, route):
    """(sums, bounds) of the rows a floating sumw / avgw adds on the direct and tile routes, in double: the window itself (direct), or --
    the tile kernel restarts its prefix at every group start -- at most the group's last 2048 + halo rows (tile); the bound is
    span * 2^-52 * sum|x| over those rows of the same group.  One pair serves sumw and avgw of a column: the caller keeps it."""
    span = w if route == "direct" else _ext(w)
    x64 = xf.astype(np.float64)
    ax = np.abs(x64)
    ax[~np.isfinite(ax)] = np.inf
    with np.errstate(all="ignore"):
        return trail_grouped(lay, x64, w), span * (2.0 ** -52 * trail_grouped(lay, ax, span) + 5e-324)


def own_rows_window(name, got, lay, w, route, live, own, what=""):
    """floating sumw / avgw against own_rows.  Rows whose span holds an infinity are left to the oracle comparison."""
    ref, rb = own
    with np.errstate(all="ignore"):
        if name == "avgw":
            ln = np.minimum(lay.pos + 1, w)
            ref, rb = ref / ln, rb / ln
        bad = live & np.isfinite(ref) & np.isfinite(rb) & ~(np.abs(got.astype(np.float64) - ref) <= rb)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        _fail(name, w, what + f" ({route} route)", r, lay, f"device {got[r]!r}, sum of the route's rows of the group {ref[r]!r}, bound {rb[r]!r}")


def check(name, lay, xf, w, got, want, what="", exact=None, own=None):
    """the comparison of one device result `got` (flat order) with the oracle's composition `want` (module docstring); exact: the column's
    em.Exact, own: a dict the caller keeps for the column (own_rows by window) -- both are made here when not given"""
    dt = xf.dtype
    if name in VAR_OPS:
        wc.variance(exact if exact is not None else em.Exact(xf, lay.offsets), name, w, got, f"{what} {name} w={w}")
        return
    if name == "avgw" and dt.kind != "f":
        int_avgw_grouped(got, xf, lay, w, what)
        fp_sums_grouped(name, got, want, xf, lay, w, what)
        return
    if dt.kind == "f" and name in SUM_OPS:
        live = fp_sums_grouped(name, got, want, xf, lay, w, what)
        route = sum_route(dt, lay.n, w) if name in ("sumw", "avgw") else None
        if route in ("direct", "tile"):
            own = {} if own is None else own                  # the caller's, one per column: sumw and avgw share the sums and the bounds
            if (w, route) not in own:
                own[(w, route)] = own_rows(lay, xf, w, route)
            own_rows_window(name, got, lay, w, route, live, own[(w, route)], what)
        return
    if not ex.same(got, want):
        r = ex.first_diff(got, want)
        _fail(name, w, what, r, lay, f"device {got[r]!r}, oracle {want[r]!r}")


def same_rows(a, b, rows):
    """bit for bit (NaN where NaN) on the flat rows `rows`: index of the first row that differs, or -1"""
    a, b = a[rows], b[rows]
    if ex.same(a, b):
        return -1
    return int(np.nonzero(rows)[0][ex.first_diff(a, b)])


def check_isolated(name, lay, w, got_bad, got_twin, what=""):
    """the even-numbered groups' rows of the poisoned column's result equal, bit for bit, the twin's"""
    r = same_rows(got_bad, got_twin, lay.gid % 2 == 0)
    if r >= 0:
        _fail(name, w, what, r, lay, f"beside poisoned groups {got_bad[r]!r}, beside zeros {got_twin[r]!r}")


def check_poisoned(name, lay, twin, w, got_bad, got_twin, want_twin, what="", exact=None, own=None):
    """both halves of the isolation test: no bit of an even group differs between the poisoned column and its twin, and the twin's result
    is the oracle's composition, which sees every group's own rows only"""
    check_isolated(name, lay, w, got_bad, got_twin, what)
    check(name, lay, twin, w, got_twin, want_twin, what + " twin", exact, own)


# ---- the two-level carry scan ----------------------------------------------------------------------------------------------------------------
CHUNK_ROWS = 2048 * TS                                                             # rows of one chunk of tile carries (CH tiles)
TWO_LEVEL_N = (TWO_LEVEL_TILES + 1) * TS + 100                                     # 8194 tiles: five chunks, the last of two tiles
TWO_LEVEL_STARTS = (0, 3_000_001, 4 * CHUNK_ROWS - 1, 4 * CHUNK_ROWS, (TWO_LEVEL_TILES + 1) * TS)


def two_level_layout():
    return Layout("two-level", np.diff(TWO_LEVEL_STARTS + (TWO_LEVEL_N,)))
