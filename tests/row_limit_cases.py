"""Inputs and expected answers of the row-limit tests (tests/test_gpu_row_limit.py), in closed form.  No GPU code here.

A column of AQG_MAX_ROWS - 1 = 4,293,918,719 rows cannot be scanned on the CPU, so nothing here ever holds one.  What a check expects
comes from three sources that do not depend on the kernel under test:

  the generator    aqg_gen_column is bit-identical to the oracle's gen_column (gen.hip), a counter-based generator: `Source` makes
                   any slice [lo, hi) of the device's column on the CPU.  V1 (1..5), ID1 with K = 100 (1..100), PRICE (50..500) and
                   TIMESTAMP (row + 1, read as uint32 so that it keeps ascending past 2^31).
  histograms       `Hist`: how many rows hold each value of v1, id1, price and each pair (id1, v1).  On the device they come from
                   aqg_groupby_agg, which test_maximum_row_count holds at the limit; here from np.bincount.  With le[v] = rows whose
                   value is <= v and lt[v] = le[v] - cnt[v], the sorted column is value v on positions [lt[v], le[v]), rank_min(v) =
                   1 + lt[v], the element of rank r is the least v with le[v] > r, and so on: every global order statistic.
  slices + halo    the local families (windows, moving averages, the joins' probe rows) are compared on `probes(n)`: 4096 rows on
                   both sides of 2^28, 2^29, 2^30 and 2^31 -- where the BYTE offset of a 16-, 8-, 4- and 2-byte element crosses
                   2^32; 2^31 is also where a signed 32-bit index turns negative -- of 2^31 + 2^30, where the 32-bit byte offset of a
                   4-byte element wraps for the third time, and the last 4096 rows.  The family's own numpy model runs on the slice
                   with the rows in front of it that its window reaches (the halo); the halo's own outputs are dropped.

Every check is written against a small backend (`HostBackend` here over numpy arrays, the device one in the GPU test over device
columns): gather from a small table, compare, count, sum, shift by one row, fetch a slice.  The SAME check functions run
  - on the CPU at n = SMALL over the models' whole-column answers (tests/test_row_limit_cases.py: the checker is checked, and fed
    the pattern a 32-bit wrap produces it must refuse it), and
  - on the device at n = SMALL and at LIMIT (or PAST31 for a family whose buffers do not fit at LIMIT).
At n < 2^28 + 4096 the thresholds are replaced by n/16, n/8, n/4, n/2, 3n/4.

Memory: `NEED[family](n)` is the device memory the family's test holds at its peak -- its columns (live at once, as the test frees
them) plus the entry's workspace as its launcher sizes it.  `size_of(family)` is LIMIT when that is below BUDGET, else PAST31."""
import numpy as np

import checker as ck

MAX_ROWS = 2**32 - 2**20                     # include/aqg.h: AQG_MAX_ROWS
LIMIT = MAX_ROWS - 1                         # n % 4 == 3, as in test_maximum_row_count
PAST31 = 2**31 + 2**20 + 3
SMALL = 100_003
SEED, K = 42, 100
HALF = 4096
THRESHOLDS = (2**28, 2**29, 2**30, 2**31, 2**31 + 2**30)
BUDGET = 200e9                               # a family that needs more at LIMIT runs at PAST31
NONE = 0xFFFFFFFF
LE, EQ, LT, GT = ck.OP_LE, ck.OP_EQ, ck.OP_LT, ck.OP_GT


def thresholds(n):
    if n >= THRESHOLDS[0] + HALF:
        return [t for t in THRESHOLDS if t + HALF <= n]
    return [n // 16, n // 8, n // 4, n // 2, (3 * n) // 4]


def probes(n):
    """[lo, hi) row ranges every local family is compared on"""
    return [(max(t - HALF, 0), min(t + HALF, n)) for t in thresholds(n)] + [(max(n - HALF, 0), n)]


def straddles(n):
    """(threshold, element bytes whose 32-bit byte offset i * bytes wraps there: t * bytes is a multiple of 2^32) the probes of an
    n-row column cover; 2^31 is also the sign bit of a 32-bit index"""
    return [(t, b) for t, b in zip(THRESHOLDS, (16, 8, 4, 2, 4)) if t + HALF <= n]


class Source:
    """any slice of the n-row table's columns, from the oracle's generator"""

    def __init__(self, oracle, n):
        self.oracle, self.n = oracle, int(n)

    def rows(self, col, lo, hi):
        lo, hi = max(int(lo), 0), min(int(hi), self.n)
        a = self.oracle.gen_column(col, SEED, lo, max(hi - lo, 0), self.n, K)
        return a.view(np.uint32) if col == ck.GEN_TIMESTAMP else a

    def at(self, col, rows):
        return np.array([self.rows(col, r, r + 1)[0] for r in np.asarray(rows, np.int64).tolist()])

    def first_row_of(self, col, v):
        """the first row that holds v (v1 / id1: found in the first few thousand rows)"""
        a = self.rows(col, 0, 1 << 16)
        return int(np.flatnonzero(a == v)[0])

    def last_row_of(self, col, v):
        lo = max(self.n - (1 << 16), 0)
        a = self.rows(col, lo, self.n)
        return lo + int(np.flatnonzero(a == v)[-1])


class Hist:
    """rows per value: v1[v], id1[g], price[p], pair[g][v], every array indexed by the value itself (index 0 unused)"""

    def __init__(self, v1=None, id1=None, price=None, pair=None):
        self.v1, self.id1, self.price, self.pair = (None if a is None else np.asarray(a, np.int64) for a in (v1, id1, price, pair))
        have = [a for a in (self.v1, self.id1, self.price, self.pair) if a is not None]
        self.n = int(have[0].sum())
        assert all(int(a.sum()) == self.n for a in have), "the histograms count different numbers of rows"
        if self.pair is not None:
            assert self.id1 is None or np.array_equal(self.pair.sum(axis=1), self.id1)
            assert self.v1 is None or np.array_equal(self.pair.sum(axis=0), self.v1)

    @classmethod
    def of_columns(cls, v1, id1, price):
        pair = np.zeros((K + 1, 6), np.int64)
        np.add.at(pair, (id1, v1), 1)
        return cls(np.bincount(v1, minlength=6), np.bincount(id1, minlength=K + 1), np.bincount(price, minlength=501), pair)

    @classmethod
    def of_tables(cls, v1=None, id1=None, price=None, pair=None):
        """from (keys, counts) of a group-by over v1, id1 and price, and (id1 keys, v1 keys, counts) of one over the pair"""
        def one(kc, size):
            if kc is None:
                return None
            a = np.zeros(size, np.int64)
            a[np.asarray(kc[0], np.int64)] = np.asarray(kc[1], np.int64)
            return a
        p = None
        if pair is not None:
            p = np.zeros((K + 1, 6), np.int64)
            p[np.asarray(pair[0], np.int64), np.asarray(pair[1], np.int64)] = np.asarray(pair[2], np.int64)
        return cls(one(v1, 6), one(id1, K + 1), one(price, 501), p)


# ---- closed forms over one count table `cnt` (cnt[v] = rows holding v) ---------------------------------------------------------------
def le_lt(cnt):
    cnt = np.asarray(cnt, np.int64)
    le = np.cumsum(cnt)
    return le, le - cnt


def runs(cnt, desc=False):
    """(first, last) 0-based position of every value's run in the sorted column (meaningless where cnt[v] == 0)"""
    le, lt = le_lt(cnt)
    n = int(le[-1])
    return (n - le, n - lt - 1) if desc else (lt, le - 1)


def value_at(cnt, r, desc=False):
    """the element of 0-based rank r in ascending (descending) order"""
    le, _ = le_lt(cnt)
    n = int(le[-1])
    assert 0 <= r < n
    return int(np.searchsorted(le, (n - 1 - r) if desc else r, side="right"))


def rank_tables(cnt, desc=False):
    """(min, max, dense) rank of value v, 1-based"""
    first, last = runs(cnt, desc)
    present = (np.asarray(cnt) > 0).astype(np.int64)
    dense = np.cumsum(present[::-1])[::-1] if desc else np.cumsum(present)
    return first + 1, last + 1, dense


def quantile_rank(num, den, c, upper):
    p = int(num) * (int(c) - 1)
    return -((-p) // int(den)) if upper else p // int(den)


def median_of(cnt, upper=False):
    n = int(np.sum(cnt))
    return value_at(cnt, n // 2 if upper else (n - 1) // 2)


def quantiles_of(cnt, nums, den, upper=False):
    n = int(np.sum(cnt))
    return [value_at(cnt, quantile_rank(q, den, n, upper)) for q in nums]


def topk_of(cnt, k, desc):
    n = int(np.sum(cnt))
    return [value_at(cnt, r, desc) for r in range(min(k, n))]


def distinct_of(cnt):
    return int((np.asarray(cnt) > 0).sum())


def ntile_of(o, c, k):
    """include/aqg.h, ranking: the bucket of the 0-based FIRST rank o among c rows in k buckets"""
    o = np.asarray(o, np.int64)
    q, r = c // k, c % k
    if q == 0:
        return o + 1
    return np.where(o < r * (q + 1), o // (q + 1) + 1, r + (o - r * (q + 1)) // q + 1)


# ---- the backend over numpy arrays -----------------------------------------------------------------------------------------------------
class HostBackend:
    """columns are numpy arrays"""

    def table(self, a):
        return np.ascontiguousarray(a)

    def gather(self, tab, idx):
        return np.asarray(tab)[np.asarray(idx).astype(np.int64)]

    def cmp(self, op, a, b):
        a, b = np.asarray(a), np.asarray(b)
        return {LE: np.less_equal, EQ: np.equal, LT: np.less, GT: np.greater}[op](a, b).astype(np.uint8)

    def count(self, mask):
        return int(np.asarray(mask).sum(dtype=np.uint64))

    def total(self, x):
        return int(np.asarray(x).astype(np.uint64).sum())

    def prev(self, x):
        x = np.asarray(x)
        return np.concatenate([x[:1], x[:-1]])

    def rows(self, x, lo, hi):
        return np.asarray(x)[int(lo):int(hi)].copy()

    def at(self, x, idx):
        return np.asarray(x)[np.asarray(idx, np.int64)]

    def free(self, *cols):
        pass


def wrapped(x, modulus):
    """what a 32-bit wrap leaves behind: element i >= modulus holds what belongs at i - modulus k (i mod modulus)"""
    x = np.asarray(x)
    return x[np.arange(len(x)) % int(modulus)]


def _all(B, mask, n, what):
    got = B.count(mask)
    B.free(mask)
    assert got == n, "%s: %d of %d rows differ from the closed form" % (what, n - got, n)


# ---- sort ------------------------------------------------------------------------------------------------------------------------------
def check_sort(B, src, h, v1, ts, order, desc):
    """`order` = stable aqg_sort_rows of the column by v1.  (a) v1[order[p]] is the run layout: position p + 1 = ts[p] lies inside the
    run of the value found there; (b) ids ascend strictly inside every run: order[p] <= order[p - 1] happens exactly at row 0 (the
    shift's own first row) and at the run boundaries where the ids read back say so; (c) every run starts at its value's first row and
    ends at its last (the oracle's head and tail); (d) the ids sum to n (n - 1) / 2.  (a) + (b) make every run the ascending list of
    ALL rows of its value: the stable sort, and a permutation."""
    n = h.n
    first, last = runs(h.v1, desc)
    g = B.gather(v1, order)
    lo = B.gather(B.table((first + 1).astype(np.uint32)), g)
    _all(B, B.cmp(LE, lo, ts), n, "sort: run starts")
    B.free(lo)
    hi = B.gather(B.table((last + 1).astype(np.uint32)), g)
    _all(B, B.cmp(LE, ts, hi), n, "sort: run ends")
    B.free(hi, g)
    p = B.prev(order)
    falls = B.count(B.cmp(LE, order, p))
    B.free(p)
    vals = [v for v in (range(5, 0, -1) if desc else range(1, 6)) if h.v1[v]]
    edge = np.array([first[v] for v in vals[1:]], np.int64)                   # the first position of every run but the first
    before, after = B.at(order, edge - 1).astype(np.int64), B.at(order, edge).astype(np.int64)
    assert falls == 1 + int((after <= before).sum()), "sort: %d descents, the run boundaries explain %d" % (falls - 1, int((after <= before).sum()))
    for v in vals:
        got = B.at(order, np.array([first[v], last[v]], np.int64)).astype(np.int64).tolist()
        assert got == [src.first_row_of(ck.GEN_V1, v), src.last_row_of(ck.GEN_V1, v)], ("sort: run of %d" % v, got)
    assert B.total(order) == n * (n - 1) // 2, "sort: the ids do not sum to n (n - 1) / 2"


# ---- rank ------------------------------------------------------------------------------------------------------------------------------
RANK_K = 7


def check_rank_values(B, h, v1, got, method, desc):
    """min / max / dense ranks over v1 against a gather from the six-entry table, over the whole column"""
    tab = dict(zip(("min", "max", "dense"), rank_tables(h.v1, desc)))[method]
    want = B.gather(B.table(tab.astype(np.uint32)), v1)
    _all(B, B.cmp(EQ, got, want), h.n, "rank %s%s" % (method, " desc" if desc else ""))
    B.free(want)


def check_row_number(B, h, ts, order, first):
    """first[order[p]] == p + 1: the row numbers follow the stable order (held by check_sort)"""
    g = B.gather(first, order)
    _all(B, B.cmp(EQ, g, ts), h.n, "row number")
    B.free(g)


def check_ntile(B, h, first, ntile, k=RANK_K):
    for lo, hi in probes(h.n):
        o = B.rows(first, lo, hi).astype(np.int64) - 1
        assert np.array_equal(B.rows(ntile, lo, hi).astype(np.int64), ntile_of(o, h.n, k)), ("ntile", lo)


# ---- median / quantiles / top-k / count distinct ------------------------------------------------------------------------------------------
QUANT = ((0, 1, 25, 50, 95, 99, 100), 100)
TOPK = 16
SELECT_COLS = (("v1", ck.GEN_V1), ("price", ck.GEN_PRICE))


def select_expected(h, name):
    cnt = getattr(h, name)
    nums, den = QUANT
    return {"median": (median_of(cnt), median_of(cnt, True)), "quantiles": (quantiles_of(cnt, nums, den), quantiles_of(cnt, nums, den, True)),
            "top": {False: topk_of(cnt, TOPK, False), True: topk_of(cnt, TOPK, True)}, "distinct": distinct_of(cnt)}


def check_select(src, h, name, col, got):
    """got: {"median": (lower, upper), "quantiles": (lower list, upper list), "top": {desc: (values, rows)}, "distinct": count}"""
    want = select_expected(h, name)
    assert tuple(int(v) for v in got["median"]) == want["median"], (name, "median", got["median"], want["median"])
    for w in (0, 1):
        assert [int(v) for v in got["quantiles"][w]] == want["quantiles"][w], (name, "quantiles", w, got["quantiles"][w], want["quantiles"][w])
    assert int(got["distinct"]) == want["distinct"], (name, "count distinct", got["distinct"], want["distinct"])
    for desc in (False, True):
        vals, rows = (np.asarray(a).astype(np.int64) for a in got["top"][desc])
        assert vals.tolist() == want["top"][desc], (name, "top", desc, vals.tolist())
        assert rows.max() < h.n and np.array_equal(src.at(col, rows), vals), (name, "top-k rows do not hold the values", desc)
        for v in np.unique(vals):                                            # equal values: distinct positions, ascending
            r = rows[vals == v]
            assert np.all(np.diff(r) > 0), (name, "top-k ties", desc, r.tolist())


# ---- joins ------------------------------------------------------------------------------------------------------------------------------
def join_build(rng_seed=4):
    """100 build keys: a permutation of 1..100 but for 7 of them, replaced by keys no probe row holds"""
    rng = np.random.default_rng(rng_seed)
    key = rng.permutation(np.arange(1, K + 1, dtype=np.int32))
    miss = np.sort(rng.choice(K, 7, replace=False))
    key[miss] = 1000 + np.arange(7, dtype=np.int32)
    pos = np.full(K + 1, NONE, np.uint32)
    hit = key <= K
    pos[key[hit]] = np.flatnonzero(hit).astype(np.uint32)
    return key, pos


def check_join(B, h, id1, look, count, what):
    """look[i] = the build row of probe row i (all n rows of id1), NONE where its key is not on the build side; count = matching pairs"""
    key, pos = join_build()
    want = B.gather(B.table(pos), id1)
    _all(B, B.cmp(EQ, look, want), h.n, what + " lookup")
    B.free(want)
    assert int(count) == int(h.id1[key[key <= K]].sum()), (what, "count", count)


# ---- the local families: probe slices against the family's own model ---------------------------------------------------------------------
# A slice [lo, hi) is rebuilt on the CPU from row lo - halo on; the model runs over halo + slice as one column and its first `halo`
# outputs are dropped.  A window family needs halo >= w - 1: every kept row's window then lies inside the rebuilt rows (or the rebuilt
# rows start at row 0, where the model clamps as the device does).
def halo_slices(n, halo):
    """(base, lo, hi): rebuild [base, hi), hold [lo, hi)"""
    return [(max(lo - halo, 0), lo, hi) for lo, hi in probes(n)]


WINQ = dict(w=21, nums=(1, 2, 3), den=4)


def check_winq(B, src, n, out, which, w=WINQ["w"], nums=WINQ["nums"], den=WINQ["den"]):
    """aqg_window_quantiles over price: plane j of `out` (elements [j n, (j + 1) n)) answers nums[j]"""
    import winq_model
    for base, lo, hi in halo_slices(n, w - 1):
        want, _ = winq_model.windows(src.rows(ck.GEN_PRICE, base, hi), w, nums, den, which)
        for j in range(len(nums)):
            got = B.rows(out, j * n + lo, j * n + hi)
            assert np.array_equal(got, want[j][lo - base:]), "window quantiles: plane %d differs in the slice at %d" % (j, lo)


PAIR_WINDOWS = {"reg": 8, "lds": 64, "prefix": 1000}
PAIR_COLS = (ck.GEN_PRICE, ck.GEN_ID1)


def check_pair(B, src, n, out, fam, w):
    """aqg_scan2 of (price, id1) under the family's accuracy contract (pair_moments.PairExact.check, what tests/test_gpu_pairwin.py
    holds).  The contract's range of a PREFIX-route window is the running range of the column up to the row; the slice's own, from the
    halo on, is never larger, so the bound held here is the contract's or tighter."""
    import pair_moments as pm
    for base, lo, hi in halo_slices(n, w - 1):
        ex = pm.PairExact(src.rows(PAIR_COLS[0], base, hi), src.rows(PAIR_COLS[1], base, hi))
        got, sel = np.full(hi - base, np.nan), np.zeros(hi - base, bool)
        got[lo - base:], sel[lo - base:] = B.rows(out, lo, hi), True
        ill = ex.check(got, fam, w, what="pair window fam %d w %d in the slice at %d" % (fam, w, lo), upto=sel)
        assert 100 * ill <= hi - lo, ("pair window: ill-conditioned positions", fam, w, lo, ill)


EMA_HALO = 4096
EMA_ALPHA = 0.25


def check_ema(B, src, n, out, mode, hold, alpha=EMA_ALPHA):
    """aqg_scan_ema of price with a constant alpha under the family's bound (`hold` of tests/test_gpu_ema.py, at the rows' true
    positions).  The rows in front of the halo weigh (1 - alpha)^4096 < 1e-500 of a value below 2^9: nothing in a double.  M, the
    running maximum of |x|, is taken from the halo on: never larger than the column's, so the bound is the contract's or tighter."""
    import ema_model as em
    for base, lo, hi in halo_slices(n, EMA_HALO):
        ref = em.reference_ema(src.rows(ck.GEN_PRICE, base, hi), None, mode, alpha=alpha)
        k = lo - base
        sub = em.Reference(ref.y[k:], ref.M[k:], ref.poisoned[k:], np.arange(lo, hi, dtype=np.int64), ref.err[k:])
        hold(B.rows(out, lo, hi), sub, mode, "ema mode %d in the slice at %d" % (mode, lo))


TW_SPAN, TW_HALO = 10.0, 64


class _Col:
    def __init__(self, x):
        self.x = x


def check_timewin(B, src, n, bounds, outs, frame, hold, span=TW_SPAN):
    """aqg_rangew over (TIMESTAMP as uint32, price): `bounds` the first position of every window, outs[op] the aggregates; `hold` of
    tests/test_gpu_timewin.py"""
    import timewin_model as tm
    for base, lo, hi in halo_slices(n, TW_HALO):
        t, x = src.rows(ck.GEN_TIMESTAMP, base, hi), src.rows(ck.GEN_PRICE, base, hi)
        fp, st = tm.stamps(t)
        lo_loc = tm.search_bounds(fp, st, None, span, frame)
        k = lo - base
        assert base == 0 or lo_loc[k:].min() > 0, "the halo does not cover a window"
        w = tm.search_windows(x, lo_loc)
        sub = tm.Windows(x[k:], lo_loc[k:], w.S[k:], w.A[k:], w.emin, w.nnan[k:], w.npinf[k:], w.nninf[k:], w.mn[k:], w.mx[k:])
        sub.len = w.len[k:]
        assert np.array_equal(B.rows(bounds, lo, hi).astype(np.int64), lo_loc[k:] + base), "time windows: bounds differ in the slice at %d" % lo
        for op, out in outs.items():
            hold(_Col(x), sub, op, B.rows(out, lo, hi), "time windows op %d in the slice at %d" % (op, lo))


# ---- as-of join and window join: the build side is the whole table (on = TIMESTAMP = row + 1 as uint32, payload v1) -------------------------
ASOF_MODES = ((False, False), (False, True), (True, False), (True, True))                     # (forward, strict)
WJ_BEFORE, WJ_AFTER, WJ_FILL = 5, 3, 77
TOP = 2**32 - 1


def join_probes(n):
    """about 10,000 probe stamps (uint32, in no order): 0, 1, every threshold - 1 / + 0 / + 1, n, n + 1, the end of the type, 600 stamps
    beside every threshold and the column's end, the rest anywhere in [0, n + 5000]"""
    rng = np.random.default_rng(11)
    ths = thresholds(n)
    special = [0, 1, 2, n - 1, n, n + 1, n + 2, TOP - 1, TOP] + [t + d for t in ths for d in (-1, 0, 1)]
    near = np.concatenate([t + rng.integers(-HALF, HALF, 600) for t in ths + [n]])
    wide = rng.integers(0, min(n + 5000, TOP) + 1, 10_000 - len(special) - len(near))
    s = np.clip(np.concatenate([special, near, wide]).astype(np.int64), 0, TOP)
    return rng.permutation(s).astype(np.uint32)


def asof_expected(n, stamps, forward, strict):
    """the build row whose stamp row + 1 is nearest at or before / after the probe's (strictly: before / after)"""
    s = np.asarray(stamps, np.int64)
    if forward:
        on = np.maximum(s + (1 if strict else 0), 1)
        none = on > n
    else:
        on = np.minimum(s - (1 if strict else 0), n)
        none = on < 1
    return np.where(none, NONE, on - 1).astype(np.uint32)


def check_asof(n, stamps, got, forward, strict):
    want = asof_expected(n, stamps, forward, strict)
    bad = np.flatnonzero(np.asarray(got) != want)
    assert len(bad) == 0, "as-of forward=%s strict=%s: %d probes differ, first stamp %d: got %d, expected %d" % (
        forward, strict, len(bad), stamps[bad[0]], got[bad[0]], want[bad[0]])


def wj_rows(n, stamps, before=WJ_BEFORE, after=WJ_AFTER):
    """(first row, row count) of every probe's window: the stamps within `before` below and `after` above, both ends closed"""
    s = np.asarray(stamps, np.int64)
    lo_on, hi_on = np.maximum(s - before, 1), np.minimum(s + after, n)
    return lo_on - 1, np.maximum(hi_on - lo_on + 1, 0)


def check_wj(src, n, stamps, outs, hold, fill=WJ_FILL):
    """outs[op] = aqg_join_window's answer per probe; the windows' rows of v1 come from the generator, concatenated into one short
    column; `hold` of tests/test_gpu_wj.py holds every aggregate to wj_model.interval_windows over it"""
    import wj_model as wm
    first, cnt = wj_rows(n, stamps)
    x = np.concatenate([src.rows(ck.GEN_V1, f, f + c) for f, c in zip(first.tolist(), cnt.tolist()) if c] + [np.zeros(0, np.int32)])
    hi = np.cumsum(cnt)
    ref = wm.interval_windows(x, hi - cnt, hi)
    for op, got in outs.items():
        hold(x, ref, op, np.asarray(got), fill, "window join op %d" % op)


# ---- aqg_groupby_build(id1) and what sits on it -------------------------------------------------------------------------------------------
GROUP_W = 7


def group_order(src):
    """id1's values in the order of their first rows: the group order of a build"""
    a = src.rows(ck.GEN_ID1, 0, 1 << 16)
    _, first = np.unique(a, return_index=True)
    keys = a[np.sort(first)]
    assert len(keys) == K
    return keys.astype(np.int64)


def group_layout(src, h):
    """(keys in group order, offsets[G + 1]) of the flat layout"""
    keys = group_order(src)
    return keys, np.concatenate([[0], np.cumsum(h.id1[keys])])


def check_group_table(src, h, keys, counts, sums, agg_keys, agg_sums):
    """the build's groups in first-occurrence order with the histogram's sizes; grouped_reduce's SUM(v1) bit for bit groupby_agg's"""
    want, _ = group_layout(src, h)
    assert np.array_equal(np.asarray(keys, np.int64), want), "groups are not in first-occurrence order"
    assert np.array_equal(np.asarray(counts, np.int64), h.id1[want]), "group sizes differ from the histogram"
    assert np.array_equal(np.asarray(agg_keys, np.int64), want) and np.asarray(sums).tobytes() == np.asarray(agg_sums).tobytes(), "grouped_reduce SUM differs from groupby_agg"
    assert [int(v) for v in ck.i128_to_int(np.asarray(sums))] == [int((h.pair[g] * np.arange(6)).sum()) for g in want]


def check_flat_keys(B, src, h, ts, key_flat):
    """grouped_flatten(id1): position p holds the key of the group whose range [offsets[g], offsets[g + 1]) holds p"""
    keys, off = group_layout(src, h)
    first, last = np.zeros(K + 1, np.uint32), np.zeros(K + 1, np.uint32)
    first[keys], last[keys] = off[:-1] + 1, off[1:]
    lo = B.gather(B.table(first), key_flat)
    _all(B, B.cmp(LE, lo, ts), h.n, "flat layout: group starts")
    B.free(lo)
    hi = B.gather(B.table(last), key_flat)
    _all(B, B.cmp(LE, ts, hi), h.n, "flat layout: group ends")
    B.free(hi)


def check_flat_stamps(B, src, h, ts_flat):
    """grouped_flatten(TIMESTAMP): strictly descending inside every group (ht_postproc order), so ts_flat[p] >= ts_flat[p - 1] happens at
    row 0 (the shift's own first row) and at exactly the group starts where the stamps read back rise; every row once: the sum"""
    keys, off = group_layout(src, h)
    p = B.prev(ts_flat)
    rises = B.count(B.cmp(LE, p, ts_flat))
    B.free(p)
    edge = off[1:-1].astype(np.int64)
    before, after = B.at(ts_flat, edge - 1).astype(np.int64), B.at(ts_flat, edge).astype(np.int64)
    assert rises == 1 + int((after >= before).sum()), "flat layout: %d rises, the group starts explain %d" % (rises - 1, int((after >= before).sum()))
    for g in (0, K // 2, K - 1):                                         # a group runs from its last row down to its first
        got = B.at(ts_flat, np.array([off[g], off[g + 1] - 1], np.int64)).astype(np.int64).tolist()
        assert got == [src.last_row_of(ck.GEN_ID1, keys[g]) + 1, src.first_row_of(ck.GEN_ID1, keys[g]) + 1], ("flat layout: group", g, got)
    assert B.total(ts_flat) == h.n * (h.n + 1) // 2, "flat layout: the stamps do not sum to n (n + 1) / 2"


def check_group_medians(src, h, lower, upper):
    keys, _ = group_layout(src, h)
    assert [int(v) for v in lower] == [median_of(h.pair[g]) for g in keys], "grouped median (lower)"
    assert [int(v) for v in upper] == [median_of(h.pair[g], True) for g in keys], "grouped median (upper)"


GROUP_QUANT = ((1, 2, 3, 4), 5)             # v1 is uniform over 1..5: these ranks fall beside the run boundaries, the answers differ from group to group


def check_group_quantiles(src, h, got, upper):
    keys, _ = group_layout(src, h)
    nums, den = GROUP_QUANT
    want = [quantiles_of(h.pair[g], nums, den, upper) for g in keys]
    assert np.asarray(got).astype(np.int64).tolist() == want, "grouped quantiles (%s)" % ("upper" if upper else "lower")


def comb_table(h, method, desc=False):
    """rank of value v inside group `key`, indexed by key * 6 + v"""
    tab = np.zeros((K + 1) * 6, np.uint32)
    for g in range(1, K + 1):
        tab[g * 6:g * 6 + 6] = dict(zip(("min", "max", "dense"), rank_tables(h.pair[g], desc)))[method]
    return tab


def check_group_rank(B, h, comb_flat, got, method, desc=False):
    """grouped rank of v1 in the flat layout against a gather from the 606-entry table over comb = id1 * 6 + v1, flattened"""
    want = B.gather(B.table(comb_table(h, method, desc)), comb_flat)
    _all(B, B.cmp(EQ, got, want), h.n, "grouped rank %s" % method)
    B.free(want)


def group_tail(src, key, rows):
    """v1 of the LAST `rows` positions of the group in the flat layout: its first rows of the column, highest row id first"""
    a, v = src.rows(ck.GEN_ID1, 0, 1 << 16), src.rows(ck.GEN_V1, 0, 1 << 16)
    at = np.flatnonzero(a == key)[:rows]
    assert len(at) == rows
    return v[at[::-1]]


def group_head(src, key, rows):
    """v1 of the FIRST `rows` positions of the group in the flat layout: its last rows of the column, highest row id first"""
    lo = max(src.n - (1 << 16), 0)
    a, v = src.rows(ck.GEN_ID1, lo, src.n), src.rows(ck.GEN_V1, lo, src.n)
    at = np.flatnonzero(a == key)[-rows:]
    assert len(at) == rows
    return v[at[::-1]]


def check_group_window(B, src, h, out, oracle, w=GROUP_W):
    """grouped SUMW(w) of v1 at both ends of every group: the first w positions (the window restarts at the group start and grows)
    and the last w (against the oracle's scan of the group's last 2 w - 1 elements)"""
    keys, off = group_layout(src, h)
    for g, key in enumerate(keys.tolist()):
        assert h.id1[key] >= 2 * w
        want = oracle.scan(ck.SCAN_SUMW, np.ascontiguousarray(group_head(src, key, w)), w)
        got = B.rows(out, off[g], off[g] + w)
        assert got.tobytes() == want.tobytes(), "grouped window sum: the start of group %d (position %d)" % (g, off[g])
        want = oracle.scan(ck.SCAN_SUMW, np.ascontiguousarray(group_tail(src, key, 2 * w - 1)), w)[-w:]
        got = B.rows(out, off[g + 1] - w, off[g + 1])
        assert got.tobytes() == want.tobytes(), "grouped window sum: the end of group %d (positions up to %d)" % (g, off[g + 1])


def pair_build(rng_seed=5):
    """a two-column build side: 460 of the 500 (id1, v1) pairs in a shuffled order and 9 pairs no probe row holds"""
    rng = np.random.default_rng(rng_seed)
    allp = np.array([(g, v) for g in range(1, K + 1) for v in range(1, 6)], np.int32)
    keep = rng.permutation(len(allp))[:460]
    rows = np.concatenate([allp[keep], np.array([(g, 9) for g in range(1, 10)], np.int32)])
    rows = rows[rng.permutation(len(rows))]
    pos = np.full((K + 1) * 6, NONE, np.uint32)
    real = rows[:, 1] <= 5
    pos[rows[real, 0] * 6 + rows[real, 1]] = np.flatnonzero(real).astype(np.uint32)
    return np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1]), pos


def check_pair_join(B, h, comb, look, counts):
    """the composite-key join: look[i] against a gather from the 606-entry position table over comb = id1 * 6 + v1; counts: the output
    rows of the INNER, LEFT, SEMI and ANTI joins (every build tuple is there once)"""
    kg, kv, pos = pair_build()
    want = B.gather(B.table(pos), comb)
    _all(B, B.cmp(EQ, look, want), h.n, "composite-key lookup")
    B.free(want)
    hit = int(sum(h.pair[g, v] for g, v in zip(kg.tolist(), kv.tolist()) if v <= 5))
    assert [int(c) for c in counts] == [hit, h.n, hit, h.n - hit], ("composite-key join counts", counts, hit)


# ---- device memory a family's test holds at its peak -----------------------------------------------------------------------------------------
def _sort_ws(n):                              # sort.hip: six planes of row ids / images, chunk counts, the histogram's partials
    return 6 * 4 * n + 256 * (n // 8192 + 1) * 4 + (1 << 24)


NEED = {
    # v1, ts, order + gathered values, one bounds column, a mask
    "sort": lambda n: 5 * 4 * n + n + _sort_ws(n),
    # the sort's planes, the order and the marks rank keeps in the pool (5 n); first, order, ts, the gathered ranks, a mask
    "rank": lambda n: 4 * 4 * n + n + 5 * n + _sort_ws(n),
    # one column, count distinct's pair list (a row id and an image per row, kept by the context), the selection's scratch (a few MB)
    "select": lambda n: 4 * n + 8 * n + (1 << 28),
    # id1, the lookup, the gathered table, a mask; the probe rows' flags and the tail's offsets in the workspace
    "join": lambda n: 3 * 4 * n + n + 8 * n + (1 << 28),
}
NEED.update({
    # price, three planes of quantiles; the rank table in the workspace is a few KB
    "winq": lambda n: 4 * n + 3 * 4 * n + (1 << 20),
    # price, id1, n doubles; covw's prefix (three doubles a row) and 72 bytes per tile of 2048 rows
    "pair": lambda n: 2 * 4 * n + 8 * n + 3 * 8 * n + 72 * (n // 2048 + 1) + (1 << 20),
    # the same with corrw's prefix: five doubles a row
    "pair_wide": lambda n: 2 * 4 * n + 8 * n + 5 * 8 * n + 72 * (n // 2048 + 1) + (1 << 20),
    # price, n doubles, an aggregate per tile
    "ema": lambda n: 4 * n + 8 * n + 64 * (n // 2048 + 1) + (1 << 20),
    # stamps, price, the bounds, the widest result (16-byte sums), the block tree (three 16-byte entries per 64 rows and level)
    "timewin": lambda n: 3 * 4 * n + 16 * n + 4 * n + n + (1 << 24),
    # id1, v1, id1 * 6 + v1, the lookup, the gathered table, a mask; the probe rows' flags and the tail's offsets in the workspace
    "join_pair": lambda n: 5 * 4 * n + n + 8 * n + (1 << 28),
    # the stamps and their images, v1 and its copy in the window order, the order, the fold's tree
    "asof_wj": lambda n: 5 * 4 * n + n + (1 << 24),
    # id1, v1 or the stamps, the build's group ids, one flattened column with its shifted copy and a mask, the flat group ids
    "grouped": lambda n: 6 * 4 * n + n + (1 << 28),
    # the grouped window sum: id1, v1, the group ids, v1 flattened in the workspace, 16-byte sums
    "grouped_scan": lambda n: 4 * 4 * n + 16 * n + (1 << 28),
    # id1 * 6 + v1 in both layouts, the group ids in both layouts, ranks and their expectation, a mask; the sort's planes, the order
    # and the marks
    "grouped_rank": lambda n: 7 * 4 * n + n + 5 * n + 4 * n + _sort_ws(n),
})


def distinct_all_need(n):
    """count(distinct) over an all-distinct column (TIMESTAMP) of n rows: the column, the pair list -- every row is left as a
    (group, image) pair, 8 bytes -- and the group-by of the second phase over n pairs in n groups.  With no hint that group-by ends
    on the hashed plan (partition plans stop at a hint of 2^25, groupby.hip), whose table has next_pow2(2 hint) + 1 slots, hint >= the
    group count, of a 16-byte record and 12 bytes of slot id, first row and count (agg_workspace)"""
    slots = 1 << (2 * n - 1).bit_length()
    return 4 * n + 8 * n + (slots + 1) * (16 + 12)


def size_of(family):
    return LIMIT if NEED[family](LIMIT) < BUDGET else PAST31
