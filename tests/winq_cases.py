"""The cases tests/test_gpu_winq.py runs on the device, shared with tests/test_winq_model.py, which shows on the CPU that this very list
refuses every planted mistake.  Everything is parametrised by TS, the rows a workgroup owns as the device reports them
(aqg_window_quantiles_last); the CPU test takes DEFAULT_TS.  Nothing here needs a GPU.

General inputs hold no NaN and no -0.0, so the model flags nothing; mixed_column is the one input written to exercise the flags."""
import numpy as np

import extremes as ex

DEFAULT_TS = 2048
MAX_W = 1024                         # AQG_WINQ_MAX_W
DTYPES = ex.NUM_DTYPES + [np.dtype(np.bool_)]
FULL_DTYPES = [np.dtype(np.int32), np.dtype(np.float64)]
WHICH = (0, 1)
W_ALL = [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024]
W_REDUCED = [1, 8, 65, 1024]
# (nums, den): the median alone, {0, 1/2, 1}, eight ranks with repeats, out of order
QLISTS = [([1], 2), ([0, 1, 2], 2), ([7, 1, 8, 0, 4, 1, 7, 3], 8)]
SHIFTS = (0, 1, 3)                   # elements the column's base pointer is moved off an aligned address


def as_model(a):
    return a.astype(np.uint8) if a.dtype == np.bool_ else a


def sizes(w, ts, full=True):
    if not full:
        return sorted({w, ts + w - 1, 3 * ts + 5})
    return sorted(n for n in {1, 2, w - 1, w, w + 1, ts - 1, ts, ts + 1, ts + w - 2, ts + w - 1, ts + w, 3 * ts + 5} if n >= 1)


def tame(a):
    """no -0.0 (NaNs: full_range and pool(nan=False) hold none)"""
    if a.dtype.kind == "f":
        a = a.copy()
        a[a == 0] = 0.0
    return a


def extremes_pool(dt):
    return tame(ex.pool(dt, nan=False))


def ascending(dt, n):
    """strictly ascending over the type's whole range where it holds n values, else every value of the type in order, repeated"""
    if dt.kind == "f":
        return (np.arange(n, dtype=np.float64) - n / 2 + 0.25).astype(dt)
    ii = np.iinfo(dt)
    span = int(ii.max) - int(ii.min)
    if span + 1 >= n:
        step = max(1, span // max(n - 1, 1))
        return np.array([int(ii.min) + k * step for k in range(n)], dtype=object).astype(dt)
    return np.sort(np.array([int(ii.min) + k % (span + 1) for k in range(n)], dtype=object).astype(dt))


def saw_period(w):
    """the smallest divisor of w above 1 (w itself when it is prime; 1 for w == 1)"""
    return next((p for p in range(2, w + 1) if w % p == 0), 1)


def flat_inputs(rng, dt, n, w):
    """random, all-equal, strictly ascending / descending, a saw-tooth whose period divides w, a 0/1 column, the type's extremes"""
    if dt.kind == "b":
        yield "random", rng.integers(0, 2, n).astype(np.bool_)
        yield "equal", np.ones(n, np.bool_)
        yield "saw", (np.arange(n) % saw_period(w) % 2).astype(np.bool_)
        return
    yield "random", tame(ex.full_range(rng, dt, n))
    yield "equal", np.repeat(tame(ex.full_range(rng, dt, 1)), n)
    up = ascending(dt, n)
    yield "ascending", up
    yield "descending", up[::-1].copy()
    yield "saw", (np.arange(n) % saw_period(w)).astype(dt)
    yield "zero-one", rng.integers(0, 2, n).astype(dt)
    p = extremes_pool(dt)
    yield "extremes", p[rng.integers(0, len(p), n)]


def flat_grid(dt, ts, ws=None):
    """(w, n, name, column, shift) of the flat test of one dtype: the full grid for FULL_DTYPES, the reduced one for the others"""
    dt = np.dtype(dt)
    full = dt in FULL_DTYPES
    rng = np.random.default_rng(6100 + DTYPES.index(dt))
    case = 0
    for w in (ws if ws is not None else (W_ALL if full else W_REDUCED)):
        for n in sizes(w, ts, full):
            for name, col in flat_inputs(rng, dt, n, w):
                yield w, n, name, col, SHIFTS[case % 3]
                case += 1


def mixed_column(dt, n, seed=5):
    """both zeros, NaNs of both signs, infinities and a few ordinary values: most windows hold both zeros or a NaN"""
    rng = np.random.default_rng(seed)
    pool = np.array([0.0, -0.0, np.nan, ex._neg_nan(dt), -1.5, 2.5, -np.inf, np.inf, 1e-30], dtype=dt)
    x = pool[rng.integers(0, len(pool), n)]
    x[:4] = pool[:4]
    return x


# ---- grouped ---------------------------------------------------------------------------------------------------------------------------------
class Layout:
    """keys = repeat(arange(G), sizes): group g owns rows and flat positions offsets[g] .. offsets[g + 1]; the flat layout lists a group's
    rows in descending row id (tests/grouped_scan_cases.py), so a column written in FLAT order goes to row order by scatter()"""

    def __init__(self, name, group_sizes):
        self.name, self.sizes = name, np.asarray(group_sizes, np.int64)
        assert np.all(self.sizes > 0)
        self.G, self.n = len(self.sizes), int(self.sizes.sum())
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)])
        self.keys = np.repeat(np.arange(self.G, dtype=np.int32), self.sizes)
        self.gid = self.keys.astype(np.int64)
        self.row_ids = self.offsets[self.gid] + self.offsets[self.gid + 1] - 1 - np.arange(self.n)

    def scatter(self, flat):
        x = np.empty_like(flat)
        x[self.row_ids] = flat
        return x


def edges_layout(w, ts):
    """group starts at ts - 1, ts, ts + 1 and around the halo's edge ts - (w - 1) (+-1), then groups of 1, w - 1, w and w + 1 rows, one
    group over three tiles, and a group of extremes beside a tame one (the last two groups)"""
    starts = sorted({0} | {s for s in (ts - (w - 1) - 1, ts - (w - 1), ts - (w - 1) + 1, ts - 1, ts, ts + 1, ts + 2) if s > 0})
    group_sizes = list(np.diff(starts)) + [1, 1] + [s for s in (w - 1, w, w + 1) if s > 0] + [2 * ts + 7, 1, 70, 70]
    return Layout(f"edges w={w}", group_sizes)


def edges_column(lay, dt, rng):
    """flat order: random rows; the last group but one holds the type's extremes, the last one small values"""
    x = tame(ex.full_range(rng, dt, lay.n))
    if dt.kind != "b":
        p = extremes_pool(dt)
        a, b, c = (int(v) for v in lay.offsets[-3:])
        x[a:b] = p[rng.integers(0, len(p), b - a)]
        x[b:c] = (np.arange(c - b) % 10).astype(dt)
    return x


def grouped_cases(w, ts, dt):
    """(layout, flat column): the edges, every row its own group (G == n), one group (G == 1)"""
    dt = np.dtype(dt)
    rng = np.random.default_rng(6900 + 7 * w + DTYPES.index(dt))
    lay = edges_layout(w, ts)
    yield lay, edges_column(lay, dt, rng)
    n = ts + w + 3
    yield Layout("singletons", np.ones(n, np.int64)), tame(ex.full_range(rng, dt, n))
    yield Layout("one group", [n]), tame(ex.full_range(rng, dt, n))


GROUPED_W = [1, 2, 8, 65, 256, 1023, 1024]
GROUPED_DTYPES = [np.dtype(t) for t in (np.int32, np.float64, np.uint8, np.int16, np.float32, np.uint64, np.bool_)]
