"""The checker of the row-limit tests, checked on the CPU (no GPU needed).  At n = 100,003 every closed form and check function of
tests/row_limit_cases.py must agree with the family's own numpy model run over the whole column; fed the pattern a 32-bit wrap leaves
behind -- rows past a threshold replaced by the rows at i mod threshold -- every check must refuse."""
import copy

import numpy as np
import pytest

import checker as ck
import distinct_model
import join_model
import median_model
import quantile_model
import rank_model as rm
import row_limit_cases as rl
import topk_model

N = rl.SMALL
B = rl.HostBackend()
WRAP = rl.thresholds(N)[3]                   # the stand-in of 2^31 at this size


class World:
    def __init__(self, oracle):
        self.src = rl.Source(oracle, N)
        self.v1, self.id1, self.price, self.ts = (self.src.rows(c, 0, N) for c in (ck.GEN_V1, ck.GEN_ID1, ck.GEN_PRICE, ck.GEN_TIMESTAMP))
        self.h = rl.Hist.of_columns(self.v1, self.id1, self.price)
        self.order = {d: np.argsort(-self.v1 if d else self.v1, kind="stable").astype(np.uint32) for d in (False, True)}


@pytest.fixture(scope="module")
def w(oracle):
    return World(oracle)


def refused(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_sizes_probes_and_memory():
    assert rl.LIMIT == 2**32 - 2**20 - 1 and rl.LIMIT % 4 == 3 and 2**31 < rl.PAST31 < 2**31 + 2**21
    for n, want in ((rl.LIMIT, [(2**28, 16), (2**29, 8), (2**30, 4), (2**31, 2), (2**31 + 2**30, 4)]), (rl.PAST31, [(2**28, 16), (2**29, 8), (2**30, 4), (2**31, 2)])):
        assert rl.straddles(n) == want
        pr = rl.probes(n)
        for t, b in want:
            lo, hi = next(p for p in pr if p[0] <= t < p[1])
            assert lo == t - rl.HALF and hi == t + rl.HALF                            # rows on both sides of the threshold
            assert (t * b) % 2**32 == 0 and lo * b < t * b <= (hi - 1) * b                 # the 32-bit byte offset wraps inside the slice
        assert pr[-1] == (n - rl.HALF, n)
    assert len(rl.probes(N)) == 6 and all(0 <= lo < hi <= N for lo, hi in rl.probes(N))
    for fam, need in rl.NEED.items():
        n = rl.size_of(fam)
        assert n in (rl.LIMIT, rl.PAST31) and need(n) < rl.BUDGET, fam
        assert n == rl.PAST31 or need(rl.LIMIT) < rl.BUDGET, fam
        assert need(n) > 8 * n, fam                                                    # at least two 4-byte columns: the figure is not a placeholder
    # count(distinct) over the all-distinct TIMESTAMP column passes the budget at either size (its second phase is an n-group group-by)
    assert rl.distinct_all_need(rl.LIMIT) > 288e9 and rl.distinct_all_need(rl.LIMIT) > rl.distinct_all_need(rl.PAST31) > rl.BUDGET


def test_source_slices_are_the_column(w):
    for lo, hi in rl.probes(N):
        assert np.array_equal(w.src.rows(ck.GEN_PRICE, lo, hi), w.price[lo:hi])
    assert np.array_equal(w.ts, np.arange(1, N + 1, dtype=np.uint32))
    assert np.array_equal(w.src.at(ck.GEN_ID1, [0, 77, N - 1]), w.id1[[0, 77, N - 1]])
    for v in range(1, 6):
        rows = np.flatnonzero(w.v1 == v)
        assert (w.src.first_row_of(ck.GEN_V1, v), w.src.last_row_of(ck.GEN_V1, v)) == (rows[0], rows[-1])
    big = rl.Source(w.src.oracle, rl.LIMIT)                                          # past 2^31 the stamps keep ascending as uint32
    assert big.rows(ck.GEN_TIMESTAMP, 2**31 - 2, 2**31 + 2).tolist() == [2**31 - 1, 2**31, 2**31 + 1, 2**31 + 2]


def test_hist_from_group_tables_equals_bincount(w, oracle):
    def table(col):
        o = oracle.groupby([col])
        return col[o["first_rows"]], o["counts"]
    o = oracle.groupby([w.id1, w.v1])
    h = rl.Hist.of_tables(table(w.v1), table(w.id1), table(w.price), (w.id1[o["first_rows"]], w.v1[o["first_rows"]], o["counts"]))
    for name in ("v1", "id1", "price", "pair"):
        assert np.array_equal(getattr(h, name), getattr(w.h, name)), name


@pytest.mark.parametrize("desc", [False, True])
def test_sort(w, desc):
    order = w.order[desc]
    first, last = rl.runs(w.h.v1, desc)
    s = w.v1[order]
    for v in range(1, 6):
        assert np.all(s[first[v]:last[v] + 1] == v) and last[v] - first[v] + 1 == w.h.v1[v]
    rl.check_sort(B, w.src, w.h, w.v1, w.ts, order, desc)
    # a wrap re-processes low rows: positions past the threshold hold what belongs at i mod threshold
    refused(rl.check_sort, B, w.src, w.h, w.v1, w.ts, rl.wrapped(order, WRAP), desc)
    swap = order.copy()                                                              # an unstable sort: one pair swapped inside a run
    p = int(first[3]) + 10
    swap[[p, p + 1]] = swap[[p + 1, p]]
    refused(rl.check_sort, B, w.src, w.h, w.v1, w.ts, swap, desc)
    dup = order.copy()                                                               # one id lost to a duplicate
    dup[int(first[2]) + 5] = dup[int(first[2]) + 4]
    refused(rl.check_sort, B, w.src, w.h, w.v1, w.ts, dup, desc)
    hh = copy.copy(w.h)                                                              # the closed form itself off by one row
    hh.v1 = w.h.v1.copy()
    hh.v1[2] += 1
    hh.v1[3] -= 1
    refused(rl.check_sort, B, w.src, hh, w.v1, w.ts, order, desc)


@pytest.mark.parametrize("desc", [False, True])
def test_rank(w, desc):
    o = rm.DESC if desc else rm.ASC
    got = {m: rm.rank(w.v1, [0], code, o, k=rl.RANK_K) for m, code in (("min", rm.MIN), ("max", rm.MAX), ("dense", rm.DENSE), ("first", rm.FIRST), ("ntile", rm.NTILE))}
    for m in ("min", "max", "dense"):
        rl.check_rank_values(B, w.h, w.v1, got[m], m, desc)
        refused(rl.check_rank_values, B, w.h, w.v1, rl.wrapped(got[m], WRAP), m, desc)
    rl.check_row_number(B, w.h, w.ts, w.order[desc], got["first"])
    refused(rl.check_row_number, B, w.h, w.ts, w.order[desc], rl.wrapped(got["first"], WRAP))
    rl.check_ntile(B, w.h, got["first"], got["ntile"])
    refused(rl.check_ntile, B, w.h, got["first"], rl.wrapped(got["ntile"], WRAP))
    for k in (1, 2, 7, 100, N, N + 5):                                               # the closed form of NTILE is the model's
        assert np.array_equal(rl.ntile_of(got["first"].astype(np.int64) - 1, N, k), rm.rank(w.v1, [0], rm.NTILE, o, k=k))


def model_select(w, name):
    x = getattr(w, name)
    nums, den = rl.QUANT
    out = {"median": tuple(median_model.flat(x, which)[0] for which in (0, 1)),
           "quantiles": tuple(quantile_model.flat(x, nums, den, which)[0] for which in (0, 1)),
           "distinct": distinct_model.flat(x), "top": {}}
    for desc in (False, True):
        vals, pos, _ = topk_model.topk(x, [0, N], rl.TOPK, topk_model.ORDER_DESC if desc else topk_model.ORDER_ASC)
        out["top"][desc] = (vals[0], pos[0])
    return out


@pytest.mark.parametrize("name,col", rl.SELECT_COLS)
def test_select(w, name, col):
    got = model_select(w, name)
    rl.check_select(w.src, w.h, name, col, got)
    for key, bad in (("median", (got["median"][0] + 1, got["median"][1])), ("distinct", got["distinct"] - 1),
                     ("quantiles", (got["quantiles"][0], np.roll(got["quantiles"][1], 1)))):
        refused(rl.check_select, w.src, w.h, name, col, dict(got, **{key: bad}))
    vals, rows = got["top"][True]
    refused(rl.check_select, w.src, w.h, name, col, dict(got, top={False: got["top"][False], True: (vals, rows[::-1].copy())}))
    refused(rl.check_select, w.src, w.h, name, col, dict(got, top={False: got["top"][False], True: (vals, (rows + 1) % N)}))
    cnt, s = getattr(w.h, name), np.sort(getattr(w, name))                            # the closed form is the sorted column, at the run boundaries too
    le, _ = rl.le_lt(cnt)
    for r in [0, 1, N // 2, N - 1] + [int(le[v]) - 1 for v in np.flatnonzero(cnt)] + [int(le[v]) for v in np.flatnonzero(cnt)[:-1]]:
        assert rl.value_at(cnt, r) == s[r] and rl.value_at(cnt, r, desc=True) == s[N - 1 - r]
    hh = copy.copy(w.h)                                                              # a histogram off by ONE row: a row of the median's value
    off = cnt.copy()                                                                 # counted below the least value moves the minimum, the k
    off[int(got["median"][0])] -= 1                                                  # smallest and the distinct count
    off[int(np.flatnonzero(cnt)[0]) - 1] += 1
    setattr(hh, name, off)
    refused(rl.check_select, w.src, hh, name, col, got)


def test_joins(w):
    key, pos = rl.join_build()
    look = join_model.lookup(key, w.id1)
    assert np.array_equal(look, pos[w.id1]) and (look == rl.NONE).sum() == w.h.id1[np.setdiff1d(np.arange(1, 101), key)].sum() > 0
    count = join_model.count(key, w.id1)
    rl.check_join(B, w.h, w.id1, look, count, "join")
    refused(rl.check_join, B, w.h, w.id1, look, count + 1, "join")
    bad = rl.wrapped(look, WRAP)
    assert (bad != look).any()
    refused(rl.check_join, B, w.h, w.id1, bad, count, "join")


# ---- the local families: slice + halo against the whole-column model, and the wrap pattern refused at the slice it lands in ----------------
def refused_at(slice_lo, fn, *args):
    """the probe-slice comparison fails, and it fails AT the slice the wrap reaches first"""
    with pytest.raises(AssertionError, match=r"slice at %d\b" % slice_lo):
        fn(*args)


WRAP_SLICE = WRAP - rl.HALF                    # the slice around the stand-in of 2^31: its rows past WRAP hold rows 0 ..


def test_the_wrap_lands_in_the_slice_of_its_threshold():
    lows = [lo for lo, _ in rl.probes(N)]
    assert WRAP_SLICE in lows and all(lo + rl.HALF <= WRAP for lo in lows if lo < WRAP_SLICE)   # every earlier slice ends before the wrap


@pytest.mark.parametrize("which", [0, 1])
def test_window_quantiles(w, which):
    import winq_model
    full, _ = winq_model.windows(w.price, rl.WINQ["w"], rl.WINQ["nums"], rl.WINQ["den"], which)
    rl.check_winq(B, w.src, N, full.reshape(-1), which)
    bad = np.stack([rl.wrapped(p, WRAP) for p in full])
    refused_at(WRAP_SLICE, rl.check_winq, B, w.src, N, bad.reshape(-1), which)
    refused(rl.check_winq, B, w.src, N, np.roll(full, 1, axis=0).reshape(-1), which)           # planes at the wrong offset


@pytest.mark.parametrize("route", sorted(rl.PAIR_WINDOWS))
def test_pair_windows(w, route):
    import pair_moments as pm
    import pairwin_cases as pc
    ww = rl.PAIR_WINDOWS[route]
    assert pc.route_of(ww, rl.LIMIT) == pc.route_of(ww, N) == {"reg": pc.ROUTE_REG, "lds": pc.ROUTE_LDS, "prefix": pc.ROUTE_PREFIX}[route]
    ex = pm.PairExact(*(w.src.rows(c, 0, N) for c in rl.PAIR_COLS))
    m = ex.moments(ww)
    for fam, key in ((pm.COV, "C"), (pm.CORR, "corr"), (pm.BETA, "beta")):
        rl.check_pair(B, w.src, N, m[key], fam, ww)
        refused_at(WRAP_SLICE, rl.check_pair, B, w.src, N, rl.wrapped(m[key], WRAP), fam, ww)


@pytest.mark.parametrize("mode", [0, 1])
def test_ema(w, mode):
    import ema_model as em
    from test_gpu_ema import hold
    full = em.reference_ema(w.price, None, mode, alpha=rl.EMA_ALPHA).y.astype(np.float64)
    rl.check_ema(B, w.src, N, full, mode, hold)
    with pytest.raises(AssertionError, match=r"slice at %d\b" % WRAP_SLICE):
        rl.check_ema(B, w.src, N, rl.wrapped(full, WRAP), mode, hold)


@pytest.mark.parametrize("frame", [0, 1])
def test_time_windows(w, frame):
    import timewin_model as tm
    from test_gpu_timewin import OPS, hold
    from aquery2_amd.capi import RANGEW_AVG, RANGEW_COUNT, RANGEW_MAX, RANGEW_MIN, RANGEW_SUM
    fp, st = tm.stamps(w.ts)
    lo = tm.search_bounds(fp, st, None, rl.TW_SPAN, frame)
    win = tm.search_windows(w.price, lo)
    assert win.len.max() == (11 if frame else 10)                                              # row + 1 stamps: a closed span of 10 holds 11 rows
    outs = {RANGEW_COUNT: win.len.astype(np.uint32), RANGEW_SUM: tm.exact_int_sum(win), RANGEW_AVG: tm.exact_int_avg(win), RANGEW_MIN: win.mn, RANGEW_MAX: win.mx}
    assert set(outs) == set(OPS)
    rl.check_timewin(B, w.src, N, lo.astype(np.uint32), outs, frame, hold)
    refused_at(WRAP_SLICE, rl.check_timewin, B, w.src, N, rl.wrapped(lo, WRAP).astype(np.uint32), outs, frame, hold)
    for op in OPS:
        bad = dict(outs)
        bad[op] = rl.wrapped(outs[op], WRAP)
        if op == RANGEW_COUNT:                                                                 # (the counts of two full windows are equal: move one instead)
            bad[op] = outs[op].copy()
            bad[op][WRAP + 5] -= 1
        with pytest.raises(AssertionError):
            rl.check_timewin(B, w.src, N, lo.astype(np.uint32), bad, frame, hold)


# ---- as-of join, window join ---------------------------------------------------------------------------------------------------------------
def test_probe_stamps_straddle_what_they_claim():
    for n in (N, rl.PAST31, rl.LIMIT):
        s = rl.join_probes(n).astype(np.int64)
        assert 9_990 <= len(s) <= 10_000 and s.min() == 0 and s.max() == rl.TOP
        have = set(s.tolist())
        for t in rl.thresholds(n) + [n]:
            assert {t - 1, t, t + 1} <= have and ((s > t - rl.HALF) & (s < t)).sum() > 200 and ((s > t) & (s < t + rl.HALF)).sum() > 200
        assert {0, 1, n, n + 1, rl.TOP} <= have and np.any(np.diff(s) < 0)                   # ... and the probe side is not sorted


@pytest.mark.parametrize("forward,strict", rl.ASOF_MODES)
def test_asof(w, forward, strict):
    import asof_model as am
    s = rl.join_probes(N)
    got = am.asof_rows_sorted([], w.ts, [], s, am.FORWARD if forward else am.BACKWARD, strict)
    few = np.concatenate([s[:150], s[s.astype(np.int64) >= N - 2][:50]])                       # the brute-force statement on a few of them
    assert np.array_equal(am.asof_rows([], w.ts, [], few, am.FORWARD if forward else am.BACKWARD, strict), rl.asof_expected(N, few, forward, strict))
    rl.check_asof(N, s, got, forward, strict)
    bad = got.copy()                                                                         # a search that wrapped: rows past the threshold answer i mod threshold
    past = (bad != rl.NONE) & (bad >= WRAP)
    bad[past] = bad[past] % WRAP
    assert past.any()
    refused(rl.check_asof, N, s, bad, forward, strict)
    refused(rl.check_asof, N, s, am.asof_rows_sorted([], w.ts, [], s, am.FORWARD if forward else am.BACKWARD, not strict), forward, strict)


def wj_model_outs(w, s):
    import timewin_model as tm
    import wj_model as wm
    order, lo, hi = wm.window_bounds([], w.ts, [], s, rl.WJ_BEFORE, rl.WJ_AFTER, 0)
    assert np.array_equal(order, np.arange(N))
    first, cnt = rl.wj_rows(N, s)
    assert np.array_equal(hi.astype(np.int64) - lo, cnt) and np.array_equal(lo[cnt > 0].astype(np.int64), first[cnt > 0])   # the windows by arithmetic are the model's
    ne, win = wm.interval_windows(w.v1, lo, hi)
    outs = {wm.COUNT: np.zeros(len(s), np.uint32), wm.SUM: np.zeros(len(s), ck.I128), wm.AVG: np.full(len(s), float(rl.WJ_FILL)),
            wm.MIN: np.full(len(s), rl.WJ_FILL, np.int32), wm.MAX: np.full(len(s), rl.WJ_FILL, np.int32)}
    outs[wm.COUNT][ne] = win.len
    ex = tm.exact_int_sum(win)
    outs[wm.SUM]["lo"][ne], outs[wm.SUM]["hi"][ne] = ex["lo"], ex["hi"].view(np.int64)
    outs[wm.AVG][ne], outs[wm.MIN][ne], outs[wm.MAX][ne] = tm.exact_int_avg(win), win.mn, win.mx
    return outs


def test_window_join(w):
    import wj_model as wm
    from test_gpu_wj import hold
    s = rl.join_probes(N)
    outs = wj_model_outs(w, s)
    assert (outs[wm.COUNT] == 0).sum() > 100 and (outs[wm.COUNT] == 9).sum() > 5000 and len(set(outs[wm.COUNT].tolist())) >= 8
    rl.check_wj(w.src, N, s, outs, hold)
    shifted = wj_model_outs(w, np.where(s.astype(np.int64) >= WRAP, s.astype(np.int64) % WRAP, s).astype(np.uint32))   # windows read at i mod threshold
    for op in (wm.SUM, wm.AVG, wm.MIN, wm.MAX):
        refused(rl.check_wj, w.src, N, s, {**outs, op: shifted[op]}, hold)
    off = outs[wm.COUNT].copy()
    off[int(np.argmax(off == 9))] = 8
    refused(rl.check_wj, w.src, N, s, {**outs, wm.COUNT: off}, hold)


# ---- aqg_groupby_build(id1) and what sits on it --------------------------------------------------------------------------------------------------
class Grouped:
    """the build of id1 by the models: groups in first-occurrence order, a group's rows in descending row id"""

    def __init__(self, w, oracle):
        self.gid, self.G = median_model.first_occurrence_ids(w.id1)
        first = np.array([np.flatnonzero(self.gid == g)[0] for g in range(self.G)])
        self.keys = w.id1[first]
        self.counts = np.bincount(self.gid, minlength=self.G)
        self.perm = np.concatenate([np.flatnonzero(self.gid == g)[::-1] for g in range(self.G)])
        self.starts = np.concatenate([[0], np.cumsum(self.counts)[:-1]])
        self.sums = oracle.grouped_reduce(ck.RED_SUM, w.v1, oracle.groupby([w.id1]))


@pytest.fixture(scope="module")
def grouped(w, oracle):
    return Grouped(w, oracle)


def test_group_table_and_flat_layout(w, grouped, oracle):
    g = grouped
    rl.check_group_table(w.src, w.h, g.keys, g.counts, g.sums, g.keys, g.sums)
    refused(rl.check_group_table, w.src, w.h, g.keys, np.roll(g.counts, 1), g.sums, g.keys, g.sums)
    refused(rl.check_group_table, w.src, w.h, g.keys, g.counts, np.roll(g.sums, 1), g.keys, g.sums)
    key_flat, ts_flat = w.id1[g.perm], w.ts[g.perm]
    rl.check_flat_keys(B, w.src, w.h, w.ts, key_flat)
    rl.check_flat_stamps(B, w.src, w.h, ts_flat)
    refused(rl.check_flat_keys, B, w.src, w.h, w.ts, rl.wrapped(key_flat, WRAP))
    refused(rl.check_flat_stamps, B, w.src, w.h, rl.wrapped(ts_flat, WRAP))
    up = np.concatenate([np.sort(ts_flat[a:a + c]) for a, c in zip(g.starts, g.counts)])       # ascending inside the groups: the wrong direction
    refused(rl.check_flat_stamps, B, w.src, w.h, up)
    swap = ts_flat.copy()
    swap[[500, 501]] = swap[[501, 500]]
    refused(rl.check_flat_stamps, B, w.src, w.h, swap)


def test_group_medians_and_ranks(w, grouped):
    g = grouped
    lower, upper = (median_model.grouped(w.v1, g.gid, g.G, which)[0] for which in (0, 1))
    rl.check_group_medians(w.src, w.h, lower, upper)
    refused(rl.check_group_medians, w.src, w.h, lower + 1, upper)
    nums, den = rl.GROUP_QUANT
    for which in (0, 1):
        q = quantile_model.grouped(w.v1, g.gid, g.G, nums, den, which)[0]
        assert len({tuple(r) for r in q.tolist()}) > 3                                          # the answers do differ between groups
        rl.check_group_quantiles(w.src, w.h, q, bool(which))
        refused(rl.check_group_quantiles, w.src, w.h, np.roll(q, 1, axis=0), bool(which))
    comb_flat = (w.id1 * 6 + w.v1)[g.perm]
    for method, code in (("min", rm.MIN), ("dense", rm.DENSE), ("max", rm.MAX)):
        got = rm.rank(w.v1[g.perm], g.starts, code, rm.ASC)
        rl.check_group_rank(B, w.h, comb_flat, got, method)
        refused(rl.check_group_rank, B, w.h, comb_flat, rl.wrapped(got, WRAP), method)
    got = rm.rank(w.v1[g.perm], g.starts, rm.MIN, rm.DESC)
    rl.check_group_rank(B, w.h, comb_flat, got, "min", True)
    refused(rl.check_group_rank, B, w.h, comb_flat, got, "min", False)


def test_group_window(w, grouped, oracle):
    g = grouped
    x = w.v1[g.perm]
    out = np.concatenate([oracle.scan(ck.SCAN_SUMW, np.ascontiguousarray(x[a:a + c]), rl.GROUP_W) for a, c in zip(g.starts, g.counts)])
    rl.check_group_window(B, w.src, w.h, out, oracle)
    refused(rl.check_group_window, B, w.src, w.h, rl.wrapped(out, WRAP), oracle)
    refused(rl.check_group_window, B, w.src, w.h, oracle.scan(ck.SCAN_SUMW, x, rl.GROUP_W), oracle)   # windows that run across the group starts


def test_composite_key_join(w):
    import join_keys_model as jkm
    kg, kv, pos = rl.pair_build()
    comb = w.id1 * 6 + w.v1
    look = pos[comb]
    hit = look != rl.NONE
    assert 0.85 < hit.mean() < 0.97 and np.array_equal(kg[look[hit]], w.id1[hit]) and np.array_equal(kv[look[hit]], w.v1[hit])
    btab = {(int(a), int(b)): r for r, (a, b) in enumerate(zip(kg, kv))}
    assert len(btab) == len(kg) and look[:2000].tolist() == [btab.get((int(a), int(b)), rl.NONE) for a, b in zip(w.id1[:2000], w.v1[:2000])]
    counts = [int(hit.sum()), N, int(hit.sum()), N - int(hit.sum())]
    rl.check_pair_join(B, w.h, comb, look, counts)
    refused(rl.check_pair_join, B, w.h, comb, rl.wrapped(look, WRAP), counts)
    refused(rl.check_pair_join, B, w.h, comb, look, [counts[0], N, counts[2] - 1, counts[3]])
