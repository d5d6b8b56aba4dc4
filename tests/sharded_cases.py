"""Cuts, inputs, models and comparisons of tests/test_gpu_sharded_extremes.py (a plain module: pytest collects nothing from it;
tests/test_sharded_cases.py holds it to account without a GPU).

CUTS.  `shards(name, n)`: a named, fixed cut of a column of n rows into row ranges, one per rank; what the name promises is asserted
when the cut is made.  N = 70 001 rows for the flat operations (beyond a 2048-row tile, a chain link and the largest LDS halo, so the
50 000-row window that goes through HBM still fits); N_TINY = 5 rows (world >= rows).

INPUTS.  All from tests/extremes.py and the column recipes of test_gpu_extremes.py / groupagg_cases.py: `reduce_cases()` is the case
list of aqg_reduce_sharded, `corr_cases()` of aqg_corr_sharded and aqg_corr, `scan_plan(dt)` of aqg_scan_sharded, `groupby_layout` /
`groupby_cuts` of aqg_groupby_agg_sharded.

MODELS.  `fold_reduce`, `model_scan` and `model_groupby` compose the sharded answer from oracle calls on every SHARD with the fold
csrc/sharded.hip and csrc/exchange.hip have to make; `fault=` corrupts that fold in one of the ways FAULTS names.  The CPU tests put
the models through the comparisons below: the right fold passes, every corrupted one is refused by a case of the GPU test's own list.

COMPARISONS.  `check_reduce`, `check_scan`: the standards of test_gpu_extremes.py's module docstring, through its own helpers (fp_sum_ok,
var_bound, check_fp_sums, check_window_route, check_int_avgw) -- no constant is restated here.  They return |got - want| / bound where
a bound applies, so that the GPU tests can print the largest ratio they saw."""
import functools

import numpy as np

import checker as ck
import exact_moments as em
import extremes as ex
import groupagg_cases as gc
import grouped_scan_cases as gsc
import window_checks as wc
from test_gpu_extremes import (check_fp_sums, check_int_avgw, check_var_stddev_any, check_var_stddev_safe, check_window_route, exact_sum_fast, fp_columns,
                               fp_sum_ok, int_column, sum_route, var_bound)
from test_gpu_variance import family

N, N_TINY, N_GROUPBY = 70_001, 5, 60_011
TS = 2048                                            # rows per tile (scan_dev.hpp)
BORDER = 17 * TS                                     # a tile border near the middle of N rows
M64, M128 = (1 << 64) - 1, (1 << 128) - 1
I64, U64 = np.dtype(np.int64), np.dtype(np.uint64)

# ---- cuts --------------------------------------------------------------------------------------------------------------------------------
CUT_NAMES = ("even3", "tiny_middle", "tiny_first", "empty_first", "empty_last", "empty_middle_then_tiny", "one_holds_all", "tile_border", "tile_border_plus1")


def shards(name, n):
    """[(lo, hi)] per rank"""
    a, b = n // 3, 2 * n // 3
    t = min(3, max(1, n - 2))                        # rows of a tiny shard
    m = (n - t) // 2
    edges = {"even3": [0, a, b, n], "tiny_middle": [0, m, m + t, n], "tiny_first": [0, t, max(t, n // 2), n], "empty_first": [0, 0, n // 2, n],
             "empty_last": [0, n // 2, n, n], "empty_middle_then_tiny": [0, a, a, a + 1, max(b, a + 2), n], "one_holds_all": [0, 0, n, n],
             "tile_border": [0, BORDER, n], "tile_border_plus1": [0, BORDER + 1, n]}[name]
    sh = [(edges[r], edges[r + 1]) for r in range(len(edges) - 1)]
    rows = [hi - lo for lo, hi in sh]
    assert sh[0][0] == 0 and sh[-1][1] == n and all(r >= 0 for r in rows) and all(sh[r][1] == sh[r + 1][0] for r in range(len(sh) - 1)) and len(sh) <= 5, (name, n, sh)
    if name == "even3": assert len(sh) == 3 and max(rows) - min(rows) <= 1 or n < 6
    if name == "tiny_middle": assert rows[1] == t and min(rows[0], rows[2]) > (30_000 if n == N else 0)
    if name == "tiny_first": assert rows[0] == t and rows[0] > 0
    if name == "empty_first": assert rows[0] == 0 and rows[1] > 0 and rows[2] > 0
    if name == "empty_last": assert rows[2] == 0 and rows[0] > 0 and rows[1] > 0
    if name == "empty_middle_then_tiny": assert len(sh) == 5 and rows[1] == 0 and rows[2] == 1 and rows[0] > 0 and rows[4] > 0
    if name == "one_holds_all": assert rows == [0, n, 0]
    if name == "tile_border": assert sh[0][1] % TS == 0 and 0 < sh[0][1] < n
    if name == "tile_border_plus1": assert sh[0][1] % TS == 1 and 0 < sh[0][1] < n
    return sh


def cut_names(n):
    return tuple(c for c in CUT_NAMES if not c.startswith("tile_border") or n > BORDER + 1)


def pieces(x, sh):
    return [np.ascontiguousarray(x[lo:hi]) for lo, hi in sh]


# ---- inputs: reductions ------------------------------------------------------------------------------------------------------------------
INT_RED_OPS = tuple(ck.RED_NAMES)                    # every op, bit for bit
PROBE_E = (53, 64, 77)


def carry_columns(dt, n=N):
    """test_reduce_accumulator_carries_and_borrows' columns: a walk over the type's ends; runs of one sign, which carry (borrow) on every row"""
    dt = np.dtype(dt)
    ii = np.iinfo(dt)
    rng = np.random.default_rng(n + dt.num)
    ends = np.array([ii.max, ii.max - 1, ii.min, ii.min + 1, 1, 0] + ([-1] if dt.kind == "i" else []), dtype=dt)
    up = np.full(n, ii.max, dtype=dt)
    cols = [("walk", ends[rng.integers(0, len(ends), n)]), ("all-max", up)]
    if dt.kind == "i":
        lows = np.full(n, ii.min, dtype=dt)
        lows[[0, -1]] = -1                            # (70 001 rows of the minimum alone cut into three even shards: equal high words, low words 2^63, 0, 0 -- no carry in the fold)
        cols += [("all-min", lows), ("max-then-min", np.concatenate([up[: n // 2], np.full(n - n // 2, ii.min, dtype=dt)]))]
    return cols


def seed_columns(dt, n=N):
    """the seeds of min and max (numeric_limits<T>::max() / ::min(), the smallest POSITIVE normal): strictly negative and all-+Inf columns, and columns
    whose leading (trailing) two thirds are such and whose rest is tame"""
    dt = np.dtype(dt)
    tiny = dt.type(np.finfo(dt).tiny)
    tame = ex.sum_safe(ex.one_sign_zeros(ex.unary_column(dt, n, 3100 + dt.num, nan=False, inf=False)))      # (no order of summation overflows)
    neg = (-np.abs(tame) - tiny).astype(dt)
    assert np.all(neg < 0) and np.isfinite(neg).all()
    inf = np.full(n, np.inf, dtype=dt)
    k = 2 * n // 3 + 1                               # past the second cut of even3: the first two shards whole, and a row of the third
    lead = lambda a: np.concatenate([a[:k], tame[k:]])
    tail = lambda a: np.concatenate([tame[:n - k], a[n - k:]])
    return [("strictly-negative", neg), ("all+inf", inf), ("negative-then-tame", lead(neg)), ("+inf-then-tame", lead(inf)), ("tame-then-negative", tail(neg)),
            ("tame-then+inf", tail(inf))]


@functools.lru_cache(maxsize=None)
def reduce_cases(n=N):
    """[dict(name, x, kind)]: kind "int" (every op bit for bit), "fp" (fp_columns: the flat standards), "fp_sq" (square_safe: var / stddev under var_bound),
    "fp_bits" (seeds, -0.0, subnormals: sum / avg under the bound, min / max / first / last bit for bit), "nan" (the call succeeds; count / first / last)"""
    out = []
    for dt in ex.INT_DTYPES:
        out.append(dict(name=f"unary_column({dt.name})", x=ex.unary_column(dt, n, 3000 + dt.num), kind="int"))
    for dt in (I64, U64):
        for cname, x in carry_columns(dt, n):
            out.append(dict(name=f"carry {cname}({dt.name})", x=x, kind="int"))
    for dt in ex.FP_DTYPES:
        for cname, x in fp_columns(dt, n, 3200 + dt.num):
            out.append(dict(name=f"fp_columns {cname}({dt.name})", x=x, kind="fp"))
        fin = ex.one_sign_zeros(ex.unary_column(dt, n, 3300 + dt.num, nan=False, inf=False))
        out.append(dict(name=f"square_safe({dt.name})", x=ex.square_safe(fin), kind="fp_sq"))
        for cname, x in seed_columns(dt, n):
            out.append(dict(name=f"seeds {cname}({dt.name})", x=x, kind="fp_bits"))
        out.append(dict(name=f"only -0.0({dt.name})", x=np.full(n, -0.0, dtype=dt), kind="fp_bits"))
        fi = np.finfo(dt)
        sub = (np.random.default_rng(3400 + dt.num).integers(1, 1 << (fi.nmant - 1), n).astype(np.uint64)).astype({4: np.uint32, 8: np.uint64}[dt.itemsize]).view(dt)
        sub[::3] = -sub[::3]
        assert np.all(np.abs(sub) < fi.tiny) and np.all(sub != 0)
        out.append(dict(name=f"only subnormals({dt.name})", x=sub, kind="fp_bits"))
        places = (("first shard", [5]), ("tiny shard", [(n - 3) // 2 + 1]), ("last row of a shard", [n // 3 - 1]), ("first and last row", [0, n - 1])) if n >= 100 else (("middle", [n // 2]),)
        for where, rows in places:
            x = fp_columns(dt, n, 3500 + dt.num)[0][1].copy()
            x[rows] = np.nan
            out.append(dict(name=f"NaN in the {where}({dt.name})", x=x, kind="nan"))
    return out


def probe_cases():
    """[(name, column head, exact sum)]: ex.avg_probe_column's rows up to the sums S - 1, S and S + 1 (S: an exact tie of the rounding to double)"""
    out = []
    for dt in (I64, U64):
        for e in PROBE_E:
            for neg in ((False, True) if dt == I64 else (False,)):
                x, sums = ex.avg_probe_column(dt, e, negative=neg)
                for j, s in enumerate(sums):
                    out.append((f"avg_probe({dt.name}, e={e}{', negative' if neg else ''}) S{j - 1:+d}", x[: len(x) - 2 + j], s))
    return out


def probe_cuts(cnt):
    """cuts of a probe column's head that put its last rows -- the remainder and the two ones -- into shards of their own"""
    tail = [(max(0, cnt - 3), max(0, cnt - 2)), (max(0, cnt - 2), cnt - 1), (cnt - 1, cnt)]
    return {"even3": shards("even3", cnt), "last-rows-apart": [(0, tail[0][0])] + tail, "one-row-last": [(0, cnt - 1), (cnt - 1, cnt - 1), (cnt - 1, cnt)]}


def corr_cases(n=N):
    """[(name, x, y)]: groupagg_cases.CORR_PAIRS at full range, the full product of two pools, a constant column (zero variance)"""
    out = []
    for k, (tx, ty) in enumerate(gc.CORR_PAIRS):
        rng = np.random.default_rng(3600 + k)
        out.append((f"full_range({np.dtype(tx).name}, {np.dtype(ty).name})", ex.full_range(rng, tx, n), ex.full_range(rng, ty, n)))
        px, py = ex.product_columns(tx, ty)
        out.append((f"product_columns({np.dtype(tx).name}, {np.dtype(ty).name})", px, py))
    out.append(("constant x", np.full(n, 7, np.int32), ex.full_range(np.random.default_rng(3650), np.int32, n)))
    out.append(("constant x and y", np.full(n, -3, np.int16), np.full(n, 11, np.int16)))
    return out


# ---- inputs: scans -------------------------------------------------------------------------------------------------------------------------
WINDOWS = (1, 2, 3, 5, 100, 128, 1000, 2500, 25_000, 50_000, N, N + 3)
RATIO_W = gsc.RATIO_W + (25_000, N - 1, N, N + 5, 0)
PREFIX_OPS = ("sums", "avgs", "mins", "maxs", "deltas", "prev", "aggnext")
BITWISE_INT = ("sums", "avgs", "mins", "maxs", "deltas", "prev", "aggnext", "ratiow", "sumw", "minw", "maxw")
VAR_W = (5, 40, 100, 2500)


TINY_WINDOWS, TINY_RATIO_W = (1, 2, 3, 5, 8), (1, 2, 4, 5, 10, 0)


def windows_of(name, n=N):
    """the window lengths an op is run with over a column of n rows (N, or the five rows of N_TINY)"""
    if name in PREFIX_OPS:
        return (0,)
    if n != N:
        return {"ratiow": TINY_RATIO_W, "minw": TINY_WINDOWS + (0,), "maxw": TINY_WINDOWS + (0,)}.get(name, TINY_WINDOWS)
    return {"ratiow": RATIO_W, "minw": WINDOWS + (0,), "maxw": WINDOWS + (0,), "varw": VAR_W, "stddevw": VAR_W}.get(name, WINDOWS)


SCAN_OPS = tuple(o for o in gsc.OPS if o not in ("vars", "stddevs"))


@functools.lru_cache(maxsize=None)
def scan_columns(dtname, name, n=N):
    """[(label, column)] an op of aqg_scan_sharded is run on (test_gpu_extremes.py's recipes at n rows)"""
    dt = np.dtype(dtname)
    if name in gsc.VAR_OPS:
        rng = np.random.default_rng(3700 + dt.num)
        return [(f, family(rng, f, dt, n)) for f in ("offset", "full")]
    if dt.kind != "f":
        cols = [("full-range", int_column(dt, n, 3800 + dt.num, name))]
        if dt.itemsize == 8 and name == "avgs":
            for k, first in enumerate(ex.unrepresentable_first_rows(dt)[:4]):
                x = ex.unary_column(dt, n, 3810 + k)
                x[0] = first
                cols.append((f"first row {int(first)}", x))
        if dt.itemsize == 8 and name in ("sums", "avgs", "sumw"):
            cols.append(("all-max", np.full(n, np.iinfo(dt).max, dtype=dt)))
        return cols
    if name in ("deltas", "prev", "aggnext", "ratiow"):
        return [("specials", ex.unary_column(dt, n, 3900 + dt.num))]            # NaNs, both zeros, subnormals, infinities move as bits
    cols = [(c, x) for c, x in fp_columns(dt, n, 3920 + dt.num)]                 # (sum_safe and zeros of one sign: every family takes them)
    if name in ("mins", "maxs", "minw", "maxw"):
        cols += [(c, x) for c, x in seed_columns(dt, n) if "then-tame" in c]
    return cols


def skipped_by_contract(dt, name):
    return name == "avgw" and dt.kind == "u" and dt.itemsize >= 4          # the reference wraps arr[i] - arr[i-w] there


def scan_plan(dt, n=N, names=None):
    """[(op name, label, column, w)]: the calls of aqg_scan_sharded made for one dtype under every cut.  The seed columns (strictly negative or all-+Inf
    shards in front of tame ones) meet the prefix forms and the windows that never close or are as long as the column -- where a seed can leak"""
    dt = np.dtype(dt)
    plan = []
    for name in names or SCAN_OPS:
        if skipped_by_contract(dt, name):
            continue
        for label, x in scan_columns(dt.name, name, n):
            for w in windows_of(name, n):
                if "then-tame" in label and not (w == 0 or w >= n):
                    continue
                plan.append((name, label, x, w))
    return plan


def zero_border_column(dt, sh, n=N):
    """-0.0 as the last row of every shard (prev, deltas, mins and maxs of the next shard see it); no other zero"""
    dt = np.dtype(dt)
    x = ex.unary_column(dt, n, 3950 + dt.num, nan=False, inf=False)
    x[x == 0] = dt.type(1)
    for lo, hi in sh:
        if hi > lo:
            x[hi - 1] = -0.0
    return x


NAN_PLACES = {"first shard": 5, "tiny shard": (N - 3) // 2 + 1, "last row of a shard": N // 3 - 1}      # (tiny_middle's middle shard; even3's first)


def nan_column(dt, where, n=N):
    x = fp_columns(np.dtype(dt), n, 3970 + np.dtype(dt).num)[0][1].copy()
    x[NAN_PLACES[where]] = np.nan
    return x


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------------
def _ratio(got, want, bound):
    got, want = float(got), float(want)
    if not np.isfinite(want) or not np.isfinite(got):
        return 0.0
    d = abs(got - want)
    return 0.0 if d == 0 else (d / bound if bound > 0 else np.inf)


def check_reduce(case, name, got, want, wv=None, gv=None):
    """one reduction of one case against the oracle's of the whole column; returns |got - want| / bound (0.0 where the comparison is bit for bit).
    stddev of a square_safe column is judged next to the variances (wv oracle, gv device)"""
    x, kind, what = case["x"], case["kind"], (case["name"], name)
    n = len(x)
    if kind == "nan" and name not in ("count", "first", "last"):
        return 0.0                                   # (the call succeeded: module docstring of the GPU test)
    if kind == "int" or name in ("count", "min", "max", "first", "last"):
        ok = (got == want) if isinstance(want, int) else ex.same(np.asarray(got), np.asarray(want))
        assert ok, what + (got, want)
        return 0.0
    if name in ("sum", "avg"):
        bound = n * 2.0 ** -52 * float(np.abs(x[np.isfinite(x)].astype(np.float64)).sum()) / (n if name == "avg" else 1)
        assert fp_sum_ok(got, want, bound), what + (got, want, bound)
        return _ratio(got, want, bound)
    if kind == "fp_sq":
        bound = var_bound(x)
        if name == "var":
            assert np.isfinite(float(want)) and abs(float(got) - float(want)) <= bound, what + (got, want, bound)
        else:
            check_var_stddev_safe(gv, wv, got, want, bound, what)
        return _ratio(got, want, bound) if name == "var" else 0.0
    check_var_stddev_any(name, got, want, x, what)
    return _ratio(got, want, var_bound(x)) if name == "var" else 0.0


def check_scan(name, x, w, got, want, sh=None, one_device=None, first_nan=None, what=""):
    """one op of aqg_scan_sharded, the ranks' rows laid end to end, against the oracle's scan of the whole column (and `one_device`: aqg_scan of the
    whole column, for the results that are bit for bit).  first_nan: the column's first NaN row -- the rows before it are compared.  Returns the
    largest |got - want| / bound of the floating sum family, else 0.0"""
    dt, n = x.dtype, len(x)
    what = f"{what} {dt.name} {name} w={w}"
    if name in gsc.VAR_OPS:                           # (want: not needed -- the exact variance is the standard)
        assert got.shape == (n,) and got.dtype == np.float64, (what, got.shape, got.dtype)
        wc.variance(exact_of(x), name, w, got, what)
        return 0.0
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.dtype)
    stop = n if first_nan is None else first_nan
    if name == "avgw" and dt.kind != "f":
        check_fp_sums(name, got[:stop], want[:stop], x[:stop], min(w, n))       # the oracle's recurrence, inside its own drift
        check_int_avgw(got[:stop], x[:stop], min(w, n))
        return 0.0
    if dt.kind == "f" and name in gsc.SUM_OPS:
        ww = min(w, n) if w else None
        check_fp_sums(name, got[:stop], want[:stop], x[:stop], ww)
        if name in ("sumw", "avgw") and sh is not None:
            check_window_rows(name, got, want, x, ww, sh, stop, what)
        return fp_sum_ratio(name, got[:stop], want[:stop], x[:stop], ww)
    g, t = got[:stop], want[:stop]
    if not ex.same(g, t):
        r = ex.first_diff(g, t)
        raise AssertionError(f"{what}: row {r}: device {g[r]!r}, oracle {t[r]!r}")
    if one_device is not None and dt.kind != "f":
        assert ex.same(got, one_device), (what, "differs from aqg_scan of the whole column at row", ex.first_diff(got, one_device))
    return 0.0


_EXACT = {}


def exact_of(x):
    key = (x.dtype.name, len(x), x[:64].tobytes(), x[-64:].tobytes())
    if key not in _EXACT:
        _EXACT[key] = e = em.Exact(x)
        e.var = functools.lru_cache(maxsize=None)(e.var)          # (one exact variance per window length, whatever the cut)
    return _EXACT[key]


def fp_sum_ratio(name, got, want, x, w):
    """largest |got - want| / bound over the rows check_fp_sums compares against the oracle (its bound, restated only to report the ratio)"""
    n = len(x)
    i = np.arange(n, dtype=np.float64)
    absx = np.abs(x.astype(np.float64))
    absx[~np.isfinite(absx)] = 0.0
    eps = 2.0 ** -23 if (name == "avgw" and x.dtype == np.float32) else 2.0 ** -52
    bound = (i + 1) * eps * np.cumsum(absx)
    if name == "avgs":
        bound /= i + 1
    if name == "avgw":
        bound /= np.minimum(i + 1, w)
    g, t = got.astype(np.float64), want.astype(np.float64)
    stop = n
    if name in ("sumw", "avgw") and np.isnan(t).any():
        stop = int(np.nonzero(np.isnan(t))[0][0])
    with np.errstate(all="ignore"):
        r = np.abs(g[:stop] - t[:stop]) / bound[:stop]
    r = r[np.isfinite(t[:stop]) & np.isfinite(g[:stop]) & (bound[:stop] > 0)]
    return float(r.max()) if len(r) else 0.0


def check_window_rows(name, got, want, x, w, sh, stop, what):
    """floating sumw / avgw, "a window's rows are the window's": every shard's rows against the sum of the rows the device's route adds.  A shard
    behind the column's first row is computed twice (csrc/sharded.hip): aqg_scan over the shard's own rows, whose tiles start at the shard, and --
    the first w rows, which see the halo -- aqg_scan over [last min(w, rows before) rows of the predecessors | the shard's first w rows].  Each part
    is held to window_reference over the column THAT call saw, on the route that call took (direct or lds; the hbm route sums the whole prefix and
    has only the oracle's prefix-wide bound)."""
    t = want.astype(np.float64)
    if np.isnan(t[:stop]).any():
        stop = int(np.nonzero(np.isnan(t[:stop]))[0][0])
    g = got.astype(np.float64)
    for lo, hi in sh:
        if hi <= lo or lo >= stop:
            continue
        h = min(lo, w)
        m = min(hi - lo, w) if lo else 0             # rows recomputed with the halo
        if m:
            small = x[lo - h: lo + m]
            route = sum_route(x.dtype, len(small), w)
            if route in ("direct", "lds"):
                end = min(lo + m, stop)
                check_window_route(name, g[lo - h:end], small, w, route, first=h)
        if hi - lo > m:                              # rows whose window lies inside the shard (lo == 0: every row)
            own = x[lo:hi]
            route = sum_route(x.dtype, len(own), w)
            if route in ("direct", "lds"):
                end = min(hi, stop)
                if end > lo + m:
                    check_window_route(name, g[lo:end], own, w, route, first=m)


# ---- models: the fold over shards, right and corrupted ----------------------------------------------------------------------------------------
FAULTS = ("carry_high_word_dropped", "low_half_sign_extended", "avg_rounded_per_shard", "var_n_plus_1_of_the_shard", "zero_moment_from_a_shard_without_rows",
          "type_seed_from_an_empty_shard", "seed_from_the_predecessor_only", "halo_of_the_nearest_shard_only", "next_from_an_empty_successor",
          "ratiow_length_of_the_shard", "first_rows_local", "running_min_from_the_seeded_moment")


def _wrap128(v, signed):
    v &= M128
    return v - (1 << 128) if signed and v >> 127 else v


def fold128(parts, signed, fault=None):
    """the 128-bit total of the shards' 128-bit sums (python ints)"""
    if fault == "carry_high_word_dropped":
        lo = sum(p & M64 for p in parts) & M64
        hi = sum((p >> 64) & M64 for p in parts) & M64
        return _wrap128((hi << 64) | lo, signed)
    if fault == "low_half_sign_extended":
        sx = lambda v: v - (1 << 64) if v >> 63 else v
        return _wrap128(sum(((p >> 64) & M64) << 64 for p in parts) + sum(sx(p & M64) for p in parts), signed)
    return _wrap128(sum(parts), signed)


def wrapped_squares_sum(x):
    """sum of `a[i] * a[i]` in the C++ promoted type of the column, wrapping, as the reference adds it into its 128-bit sum (signed products sign-extended)"""
    dt = x.dtype
    if dt.itemsize <= 2 or dt == np.int32:           # int products, of 1- and 2-byte unsigned columns too (uint16: they wrap negative from 46341 on)
        p = x.astype(np.int64) ** 2
        return int((((p + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)).sum())
    if dt == np.uint32:
        return int(((x.astype(np.uint64) ** 2) & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))
    with np.errstate(over="ignore"):
        return exact_sum_fast(x * x)


def shard_moments(oracle, x):
    """what one shard ships: rows, sum, sum of squares, min, max (the reference's, seeds included), first and last row"""
    if len(x) == 0:
        return dict(n=0)
    fp = x.dtype.kind == "f"
    m = dict(n=len(x), first=x[0], last=x[-1], min=oracle.reduce(ck.RED_MIN, x), max=oracle.reduce(ck.RED_MAX, x))
    if fp:
        with np.errstate(all="ignore"):
            m["sum"] = float(oracle.reduce(ck.RED_SUM, x))
            m["ssq"] = float(np.sum((x * x).astype(np.float64)))
    else:
        m["sum"] = exact_sum_fast(x)
        m["ssq"] = wrapped_squares_sum(x)
    return m


def fold_reduce(dt, moms, fault=None):
    """{op name: value} of the whole column from the shards' moments, folded in rank order as csrc/sharded.hip's aqg_reduce_sharded has to"""
    dt = np.dtype(dt)
    fp, signed = dt.kind == "f", dt.kind == "i"
    live = [m for m in moms if m["n"]]
    n = sum(m["n"] for m in moms)
    out = {"count": n, "first": live[0]["first"], "last": live[-1]["last"]}
    mins, maxs = [m["min"] for m in live], [m["max"] for m in live]
    if fault == "zero_moment_from_a_shard_without_rows" and len(live) < len(moms):
        mins, maxs = mins + [dt.type(0)], maxs + [dt.type(0)]
    out["min"], out["max"] = dt.type(min(mins)), dt.type(max(maxs))
    np1 = float(((live[0]["n"] if fault == "var_n_plus_1_of_the_shard" else n) + 1) & 0xFFFFFFFF)
    with np.errstate(all="ignore"):
        if fp:
            s, q = np.float64(0), np.float64(0)
            for m in live:
                s, q = s + np.float64(m["sum"]), q + np.float64(m["ssq"])
            out["sum"], out["avg"] = s, s / np.float64(n)
            var = (q - s * s / np1) / np1
        else:
            s = fold128([m["sum"] for m in live], signed, fault)
            q = fold128([m["ssq"] for m in live], signed, fault)
            out["sum"] = s
            out["avg"] = np.float64(sum(float(m["sum"]) for m in live) / float(n)) if fault == "avg_rounded_per_shard" else np.float64(float(s) / float(n))
            var = np.float64((float(q) - float(_wrap128(s * s, signed)) / np1) / np1)
        out["var"], out["stddev"] = np.float64(var), np.sqrt(np.float64(var))
    return out


def _add128(arr, carry):
    """a 128-bit (lo, hi) structured array plus a python int, mod 2^128"""
    out = arr.copy()
    c = carry & M128
    with np.errstate(over="ignore"):
        lo = arr["lo"] + np.uint64(c & M64)
        out["lo"] = lo
        hi = arr["hi"].view(np.uint64) + np.uint64(c >> 64) + (lo < arr["lo"]).astype(np.uint64)
    out["hi"] = hi.view(arr.dtype["hi"])
    return out


def model_scan(oracle, name, x, sh, w=0, fault=None):
    """the ranks' rows of aqg_scan_sharded laid end to end, every rank's from oracle calls over ITS rows, what the earlier (for aggnext: later)
    shards ship and the fold csrc/sharded.hip has to make.  Offered for the ops the corruptions are about: integer sums, mins / maxs, minw / maxw,
    sumw / avgw, ratiow, deltas, prev, aggnext."""
    op, dt, n = ck.SCAN_NAMES[name], x.dtype, len(x)
    xs = pieces(x, sh)
    out = []
    signed = dt.kind == "i"
    for r, (lo, hi) in enumerate(sh):
        mine = xs[r]
        if hi == lo:
            continue
        before = [p for p in xs[:r] if len(p)]
        if name == "sums":
            assert dt.kind != "f"
            loc = oracle.scan(op, mine)
            carry = fold128([exact_sum_fast(p) for p in before], signed, fault) if before else 0
            out.append(_add128(loc, carry) if loc.dtype.names else (loc.astype(object) + carry).astype(loc.dtype) if carry else loc)
        elif name in ("mins", "maxs"):
            red, pick = (ck.RED_MIN, np.minimum) if name == "mins" else (ck.RED_MAX, np.maximum)
            loc = oracle.scan(op, mine)
            use = before[-1:] if fault == "seed_from_the_predecessor_only" else before
            for p in use:
                loc = pick(loc, oracle.reduce(red, p))
            out.append(loc.astype(dt))
        elif name in ("minw", "maxw") and w == 0:     # the running form has no seed: the predecessors ship their TRUE extreme
            red, pick = (ck.RED_MIN, np.minimum) if name == "minw" else (ck.RED_MAX, np.maximum)
            loc = oracle.scan(op, mine, 0)
            for p in before:
                loc = pick(loc, oracle.reduce(red, p) if fault == "running_min_from_the_seeded_moment" else oracle.scan(op, p, 0)[-1])
            if fault == "type_seed_from_an_empty_shard" and any(len(p) == 0 for p in xs[:r]):
                seed = (np.finfo(dt).max if name == "minw" else np.finfo(dt).tiny) if dt.kind == "f" else (np.iinfo(dt).max if name == "minw" else np.iinfo(dt).min)
                loc = pick(loc, dt.type(seed))
            out.append(loc.astype(dt))
        elif name == "aggnext":
            loc = oracle.scan(op, mine)
            later = xs[r + 1:]
            if fault == "next_from_an_empty_successor":
                later = later[:1]
                if later and len(later[0]) == 0:
                    loc[-1] = 0
            nxt = [p for p in later if len(p)]
            if nxt:
                loc[-1] = nxt[0][0]
            out.append(loc)
        else:
            reach = w if name in ("sumw", "avgw", "minw", "maxw", "ratiow") else 1
            ww = w
            if name == "ratiow" and (n if fault != "ratiow_length_of_the_shard" else len(mine)) <= w:
                ww = 1 if w else 0
                reach = ww
            tails = [p[-reach:] if reach else p[:0] for p in xs[:r]]
            if fault == "halo_of_the_nearest_shard_only":
                tails = [t for t in tails if len(t)][-1:]
            halo = np.concatenate(tails + [mine[:0]])[-reach:] if reach and tails else mine[:0]
            small = np.concatenate([halo, mine])
            if name == "ratiow" and ww and len(small) <= ww < n:        # the reference keeps its window only while the column is longer than it
                small = np.concatenate([small, np.ones(ww + 1 - len(small), dtype=dt)])
            out.append(oracle.scan(op, small, ww)[len(halo):len(halo) + len(mine)])
    return np.concatenate(out)


def _as_int(v):
    return ck.i128_to_int(np.array([v], dtype=v.dtype))[0] if v.dtype.names else int(v)


def model_groupby(oracle, keys, ops, vals, sh, fault=None):
    """aqg_groupby_agg_sharded from the oracle's group-by of every SHARD: the shard tables merged by key in rank order (= global first occurrence),
    first rows made global with the shard's row base, partials folded.  SUM / MIN / MAX / COUNT / AVG of integer columns, SUM / MIN / MAX of floating ones."""
    table, order = {}, []
    for r, (lo, hi) in enumerate(sh):
        if hi == lo:
            continue
        k = [np.ascontiguousarray(c[lo:hi]) for c in keys]
        o = oracle.groupby(k)
        part = []
        for op, v in zip(ops, vals):
            v = np.ascontiguousarray(v[lo:hi])
            need = {gc.AVG: (gc.SUM, gc.COUNT)}.get(op, (op,))
            part.append([oracle.grouped_reduce(p, v, o) for p in need])
        for g in range(o["ngroups"]):
            f = int(o["first_rows"][g])
            key = tuple(int(c[f]) for c in k)
            if key not in table:
                table[key] = dict(first=f + (0 if fault == "first_rows_local" else lo), parts=[[] for _ in ops], ranks=set())
                order.append(key)
            table[key]["ranks"].add(r)
            for j in range(len(ops)):
                table[key]["parts"][j].append([p[g] for p in part[j]])
    live_ranks = {r for r, (lo, hi) in enumerate(sh) if hi > lo}
    G = len(order)
    res = []
    for j, (op, v) in enumerate(zip(ops, vals)):
        dt = v.dtype
        ot = ck.TAG2NP[oracle.reduce_out_dtype(op, ck.tag_of(v))]
        col = np.zeros(G, dtype=ot)
        for g, key in enumerate(order):
            ps = table[key]["parts"][j]
            missing = fault == "zero_moment_from_a_shard_without_rows" and table[key]["ranks"] != live_ranks
            if op in (gc.MIN, gc.MAX):
                vals_g = [p[0] for p in ps] + ([dt.type(0)] if missing else [])
                col[g] = min(vals_g) if op == gc.MIN else max(vals_g)
            elif op == gc.COUNT:
                col[g] = sum(int(p[0]) for p in ps)
            elif dt.kind == "f":
                s = np.float64(0)
                with np.errstate(all="ignore"):
                    for p in ps:
                        s = s + np.float64(p[0])
                col[g] = s
            else:
                ints = [_as_int(p[0]) for p in ps]
                s = fold128(ints, dt.kind == "i", fault)
                if op == gc.SUM:
                    col[g] = (s & M64, (s >> 64) & M64 if dt.kind == "u" else s >> 64) if ot.names else s
                else:
                    cnt = sum(int(p[1]) for p in ps)
                    col[g] = sum(float(i) for i in ints) / float(cnt) if fault == "avg_rounded_per_shard" else float(s) / float(cnt)
        res.append(col)
    return dict(ngroups=G, first=np.array([table[k]["first"] for k in order], dtype=np.int64), keys=order, res=res)


# ---- inputs: the sharded group-by -----------------------------------------------------------------------------------------------------------
GMAX_SMALL = 341                                     # gmax of the one-launch merge at a world of three: 3 * 341 <= XS_ROWS = 1024 (csrc/exchange.hip)


def groupby_cuts(lay):
    """even3, tiny_middle, an empty rank, and `split`: shard 1 is exactly the dominant group's rows, so that group lies in one shard only"""
    n = lay.n
    lo = n // 7
    return {"even3": shards("even3", n), "tiny_middle": shards("tiny_middle", n), "empty_rank": shards("empty_first", n), "split": [(0, lo), (lo, lo + lay.big), (lo + lay.big, n)]}


def shards_holding(rows, sh):
    return {r for r, (lo, hi) in enumerate(sh) if np.any((rows >= lo) & (rows < hi))}


@functools.lru_cache(maxsize=None)
def groupby_layout(G, n=N_GROUPBY):
    """groupagg_cases.Layout (a group of a third of the rows, 60 one-row groups, the reserved all-+Inf / all--Inf / strictly-negative groups) under the
    first seed that puts the all-+Inf and the strictly-negative group into ONE shard of `split` each (asserted: test_sharded_cases.py)"""
    for seed in range(400):
        lay = gc.Layout(n, G, 7000 + seed)
        sh = groupby_cuts(lay)["split"]
        if all(len(shards_holding(lay.sized_rows[k], sh)) == 1 for k in (0, 2)):
            return lay
    raise AssertionError("no seed puts the reserved groups into one shard each")


@functools.lru_cache(maxsize=None)
def groupby_carry_layout(G, dtname, n=N_GROUPBY):
    """groupagg_cases.carry_layout -- the reserved groups hold the avg probes -- under the first seed that lays every probe group across two shards of
    `split` or more.  Six probe groups, e = 53 and 64, at this size: the three groups of e = 77 take 49 161 rows, more than the column has beside a
    group of a third of its rows (aqg_reduce_sharded's probe cases run e = 77)"""
    for seed in range(3000):
        lay = gc.carry_layout(n, G, 7500 + seed, np.dtype(dtname))
        sh = groupby_cuts(lay)["split"]
        if all(len(shards_holding(rows, sh)) >= 2 for rows in lay.sized_rows):
            return lay
    raise AssertionError("no seed splits every probe group")


def payload_columns(ops, dt):
    """8-byte payload columns one call's ops put into the exchange (exchange.hip add_part: identical partials travel once; a 128-bit partial takes two)"""
    dt = np.dtype(dt)
    wide_sum = 2 if dt.kind in "iu" and dt.itemsize == 8 else 1
    wide_sq = 2 if dt.kind in "iu" else 1
    parts = set()
    for op in ops:
        if op in (gc.SUM, gc.AVG, gc.VAR, gc.STDDEV): parts.add("sum")
        if op in (gc.COUNT, gc.AVG, gc.VAR, gc.STDDEV): parts.add("count")
        if op in (gc.VAR, gc.STDDEV): parts.add("sq")
        if op in (gc.MIN, gc.MAX): parts.add(op)
    return sum(wide_sum if p == "sum" else wide_sq if p == "sq" else 1 for p in parts)


def takes_small_merge(ops, dt, nkeys, gmax, world, key_dt=np.int32):
    """whether csrc/exchange.hip merges one call's exchange in one launch (exchange_core, `bool small = ...`): a bound on the shard tables is given,
    one key column of a non-floating type of at most 8 bytes, at most XS_MAXCOL = 6 payload columns, gmax * world <= XS_ROWS = 1024, and every payload
    column an integer SUM / MIN / MAX or a double SUM (floating sums of either width travel as doubles) -- a floating MIN / MAX sends the WHOLE call
    through concatenate + re-aggregate"""
    dt, key_dt = np.dtype(dt), np.dtype(key_dt)
    fp_minmax = dt.kind == "f" and any(op in (gc.MIN, gc.MAX) for op in ops)
    return bool(gmax) and nkeys == 1 and key_dt.kind in "iu" and key_dt.itemsize <= 8 and payload_columns(ops, dt) <= 6 and gmax * world <= 1024 and not fp_minmax


def pack_exchange_calls(ops, dt, max_cols=6, minmax_apart=False):
    """`ops` over one column cut into calls of at most max_cols payload columns (the one-launch merge takes six); minmax_apart: MIN / MAX of a
    floating column in a call of their own, so that its SUM / COUNT / AVG stay on the one-launch merge"""
    dt = np.dtype(dt)
    if minmax_apart and dt.kind == "f":
        mm = [op for op in ops if op in (gc.MIN, gc.MAX)]
        rest = [op for op in ops if op not in (gc.MIN, gc.MAX)]
        return pack_exchange_calls(rest, dt, max_cols) + ([mm] if mm else [])
    calls, cur = [], []
    for op in ops:
        if cur and payload_columns(cur + [op], dt) > max_cols:
            calls.append(cur)
            cur = []
        cur.append(op)
    return calls + ([cur] if cur else [])
