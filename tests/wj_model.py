"""The model of the window join (include/aqg.h: aqg_join_window, aqg_join_window_bounds, aqg_interval_fold).

The reference has no window join, so the contract is the library's own and this file states it twice in plain Python / numpy.  A side
is a list of 0..8 key columns in the (tag, data) format of tests/join_keys_model.py, whose tuple equality is used as it stands
(-0.0 == +0.0, a row holding a NaN key matches nothing), plus one numeric `on` column.

With B(i) = the build rows whose key tuple equals probe row i's, build row j of B(i) is in the window of probe row i iff neither `on`
is NaN and  b_j == p_i,  or  b_j < p_i and p_i - b_j is within `before`,  or  b_j > p_i and b_j - p_i is within `after`.
Distances: integers exactly (Python ints), floating values by the one rounded subtraction in double.  Within: d <= span on a closed
side, d < span on an open one (OPEN_LO / OPEN_HI).  PREVAILING adds the one row of B(i) directly in front of the window in (on, row)
order.  Inside a window the rows run in ascending (on, row id).

window_rows     brute force: per probe row, every build row of its tuple is asked the sentences above; no order, no search.
window_bounds   the way a device does it: the build rows ordered by (group, image of on, row), two searches per probe row in its
                group's segment -> (order, lo, hi), window i = order[lo[i]:hi[i]].  `mutant` plants one deliberate mistake.
interval_windows / loop_windows   the exact aggregates of the intervals [lo, hi) of a column, by prefix sums and a sparse table / by a
                loop per interval (tests/timewin_model.py's exact arithmetic: dyadic rationals).
tree_fold       the radix-64 block tree restated (suffix walk, S / P up the levels, direct loop, prefix walk); `mutant` likewise.
tests/test_wj_model.py holds the two forms equal and pins them to recorded answers of pandas (tests/golden/wj_pandas.json)."""
import math

import numpy as np

import asof_model as am
import timewin_model as tm

NONE = 0xFFFFFFFF
OPEN_LO, OPEN_HI, PREVAILING = 1, 2, 4
LDS, HBM, NOKEYS, PRESORTED = am.LDS, am.HBM, am.NOKEYS, am.PRESORTED
FOLD_STAGED, FOLD_INPLACE = 16, 32
COUNT, SUM, AVG, MIN, MAX = range(5)
U64 = 2 ** 64 - 1
RX = 64

BOUND_MUTANTS = ("lo_minus_1", "hi_plus_1", "segment_end_plus_1", "open_closed_swapped", "span_wraps", "nan_tail_included",
                 "prevailing_from_neighbour")
TREE_MUTANTS = ("suffix_prefix_swapped", "level_skipped", "empty_as_identity")


def span_ok(before, after, flags):
    """closed sides need span >= 0, open ones span > 0; NaN fails both; no unknown flag bits"""
    if flags & ~(OPEN_LO | OPEN_HI | PREVAILING):
        return False
    return bool((before > 0.0 if flags & OPEN_LO else before >= 0.0) and (after > 0.0 if flags & OPEN_HI else after >= 0.0))


def dmax_of(span, is_open):
    """the one exact limit of an integer distance: within <=> d <= dmax"""
    if math.isinf(span):
        return U64
    return min(math.ceil(span) - 1 if is_open else math.floor(span), U64)


def _vals(on):
    """exact Python values of an `on` column: ints, or floats (float32 widened, which is exact)"""
    on = np.asarray(on)
    if on.dtype.kind == "f":
        return True, [float(v) for v in on.astype(np.float64)]
    return False, [int(v) for v in on]


def _within(fp, big, small, span, is_open):
    if fp:
        d = big - small                                          # one rounded subtraction in double
        return d < span if is_open else d <= span
    return big - small <= dmax_of(span, is_open)


# ---- brute force -------------------------------------------------------------------------------------------------------------------
def window_rows(build_cols, build_on, probe_cols, probe_on, before, after, flags):
    """per probe row the np.int64 array of the build rows of its window, in (on, row) order, the prevailing row first: no order, no
    search -- every build row of the probe row's tuple is asked the three sentences above.  Integer distances are the differences of
    the (affine) uint64 images, larger minus smaller: exact; floating ones the rounded difference of the values."""
    assert span_ok(before, after, flags)
    bon, pon = np.asarray(build_on), np.asarray(probe_on)
    assert bon.dtype == pon.dtype
    fp = bon.dtype.kind == "f"
    bimg, pimg = am.image(bon), am.image(pon)
    bval, pval = bon.astype(np.float64) if fp else None, pon.astype(np.float64) if fp else None
    open_lo, open_hi = bool(flags & OPEN_LO), bool(flags & OPEN_HI)
    dl, dh = np.uint64(dmax_of(before, open_lo)), np.uint64(dmax_of(after, open_hi))
    table = {}
    for r, t in enumerate(am._tuples(build_cols, len(bon))):
        if t is not None and not (fp and np.isnan(bon[r])):
            table.setdefault(t, []).append(r)
    table = {t: np.array(r, np.int64) for t, r in table.items()}
    out = []
    for i, t in enumerate(am._tuples(probe_cols, len(pon))):
        rows = table.get(t) if t is not None and not (fp and np.isnan(pon[i])) else None
        if rows is None:
            out.append(np.zeros(0, np.int64))
            continue
        im, k = bimg[rows], pimg[i]
        eq, lt, gt = im == k, im < k, im > k
        with np.errstate(invalid="ignore", over="ignore"):
            if fp:
                d_lo, d_hi = pval[i] - bval[rows], bval[rows] - pval[i]
                in_lo = d_lo < before if open_lo else d_lo <= before
                in_hi = d_hi < after if open_hi else d_hi <= after
            else:
                in_lo, in_hi = (k - im) <= dl, (im - k) <= dh           # (only read where im < k / im > k: no wrap there)
        inside = eq | (lt & in_lo) | (gt & in_hi)
        front = lt & ~in_lo
        r_in, i_in = rows[inside], im[inside]
        win = r_in[np.lexsort((r_in, i_in))]
        if flags & PREVAILING and front.any():
            rf, imf = rows[front], im[front]
            win = np.concatenate([[rf[imf == imf.max()].max()], win])
        out.append(win.astype(np.int64))
    return out


# ---- images, segments, two searches ------------------------------------------------------------------------------------------------------
def _bisect(lo, hi, pred):
    """the first position of [lo, hi) at which pred turns false (pred is true on a prefix)"""
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid + 1
        else:
            hi = mid
    return lo


def window_bounds(build_cols, build_on, probe_cols, probe_on, before, after, flags, mutant=None):
    """(order, lo, hi) as uint32 arrays: order = the build rows by (group, on, row); window i = order[lo[i]:hi[i]]"""
    assert span_ok(before, after, flags) and (mutant is None or mutant in BOUND_MUTANTS)
    bon, pon = np.asarray(build_on), np.asarray(probe_on)
    nb, npr = len(bon), len(pon)
    lo, hi = np.zeros(npr, np.uint32), np.zeros(npr, np.uint32)
    if nb == 0 or npr == 0:
        return np.zeros(nb, np.uint32), lo, hi
    fp = bon.dtype.kind == "f"
    gb, G, gp = am.group_ids(build_cols, nb, probe_cols, npr)
    bimg, key = am.image(bon), am.image(pon)
    order = np.lexsort((np.arange(nb), bimg, gb))
    simg = bimg[order]
    off = np.searchsorted(gb[order], np.arange(G + 1))
    open_lo, open_hi = bool(flags & OPEN_LO), bool(flags & OPEN_HI)
    if mutant == "open_closed_swapped":
        open_lo, open_hi = not open_lo, not open_hi
    live = gp >= 0
    if fp:
        live &= key != am.NAN_IMAGE
    def finish(i, b, e, l, h):
        if mutant == "lo_minus_1":
            l = max(l - 1, b)
        if mutant == "hi_plus_1":
            h = min(h + 1, e)
        if flags & PREVAILING and l > (0 if mutant == "prevailing_from_neighbour" else b):
            l -= 1
        lo[i], hi[i] = l, h
    if fp:
        _, sval = _vals(bon[order])
        _, pval = _vals(pon)
    else:                                                        # images are affine in the value: thresholds by saturating adds
        dl, dh = np.uint64(dmax_of(before, open_lo)), np.uint64(dmax_of(after, open_hi))
        with np.errstate(over="ignore"):
            tl = key - dl if mutant == "span_wraps" else np.where(key >= dl, key - dl, np.uint64(0))
            th = key + dh if mutant == "span_wraps" else np.where(key <= np.uint64(U64) - dh, key + dh, np.uint64(U64))
    for g in np.unique(gp[live]):
        at = np.flatnonzero(live & (gp == g))
        b, e = int(off[g]), int(off[g + 1])
        if mutant == "segment_end_plus_1":
            e = min(e + 1, nb)
        if not fp:
            ls = b + np.searchsorted(simg[b:e], tl[at], "left")
            hs = np.maximum(b + np.searchsorted(simg[b:e], th[at], "right"), ls)
            for i, l, h in zip(at, ls, hs):
                finish(i, b, e, int(l), int(h))
            continue
        for i in at:
            p = pval[i]
            l = _bisect(b, e, lambda j: sval[j] < p and not _within(True, p, sval[j], before, open_lo))
            h = _bisect(b, e, lambda j: not (math.isnan(sval[j]) or (sval[j] > p and not _within(True, sval[j], p, after, open_hi))))
            if mutant == "nan_tail_included" and math.isinf(after):
                h = e
            finish(i, b, e, l, h)
    return order.astype(np.uint32), lo, hi


def rows_of(order, lo, hi):
    return [np.asarray(order[int(a):int(b)], np.int64) for a, b in zip(lo, hi)]


def routes(build_cols, build_on, npr, on_itemsize=None):
    """the AQG_ASOF_ROUTE_* bits of the search: LDS when the ordered build side (nb images of 4 or 8 bytes, nb row ids, G + 1 offsets)
    fits 48 KB under at least 2^16 probe rows"""
    bon = np.asarray(build_on)
    nb = len(bon)
    G = am.group_ids(build_cols, nb, [], 0)[1] if build_cols else 1
    w = 8 if bon.dtype.itemsize == 8 else 4
    lds = nb * w + nb * 4 + (G + 1) * 4 <= 48 * 1024 and npr >= 1 << 16
    return (LDS if lds else HBM) | (0 if build_cols else NOKEYS) | (PRESORTED if am.presorted(bon) else 0)


def fold_route(x, n, m):
    """the AQG_WJ_FOLD_* bit: STAGED when the column and its level 1 (accumulators: 8 bytes, 16 for sums of 8-byte integers, the
    element itself for MIN / MAX -- given here as x = (element bytes, accumulator bytes)) fit 48 KB under at least 2^16 queries"""
    esz, asz = x
    return FOLD_STAGED if n * esz + -(-n // RX) * asz <= 48 * 1024 and m >= 1 << 16 else FOLD_INPLACE


def acc_bytes(dtype, op):
    dtype = np.dtype(dtype)
    if op in (MIN, MAX):
        return dtype.itemsize
    return 16 if dtype.kind in "iu" and dtype.itemsize == 8 else 8


# ---- the aggregates of intervals [lo, hi) of a column --------------------------------------------------------------------------------------
def _windows(x, lo, ln, S, A, emin, nnan, npinf, nninf, mn, mx):
    w = tm.Windows(x, np.asarray(lo, np.int64), S, A, emin, nnan, npinf, nninf, mn, mx)
    w.len = np.asarray(ln, np.int64)
    return w


def clamp(lo, hi, n):
    """(lo, hi) as int64 with hi clamped to n and empty intervals as lo == hi"""
    lo, hi = np.asarray(lo, np.int64), np.minimum(np.asarray(hi, np.int64), n)
    return lo, np.where(hi > lo, hi, lo)


def interval_windows(x, lo, hi):
    """(nonempty, w): the mask of the non-empty intervals and tm.Windows over THOSE (in order), by prefix sums and a sparse table"""
    x = np.asarray(x)
    lo, hi = clamp(lo, hi, len(x))
    ne = hi > lo
    lo, hi = lo[ne], hi[ne]
    ints, emin = tm.dyadic(x)
    PS, PA = [0] * (len(x) + 1), [0] * (len(x) + 1)
    for i, v in enumerate(ints):
        PS[i + 1] = PS[i] + v
        PA[i + 1] = PA[i] + abs(v)
    S = [PS[int(b)] - PS[int(a)] for a, b in zip(lo, hi)]
    A = [PA[int(b)] - PA[int(a)] for a, b in zip(lo, hi)]

    def cnt(mask):
        c = np.concatenate([[0], np.cumsum(mask)])
        return c[hi] - c[lo]
    if x.dtype.kind == "f":
        nnan, npinf, nninf = cnt(np.isnan(x)), cnt(x == np.inf), cnt(x == -np.inf)
    else:
        nnan = npinf = nninf = np.zeros(len(lo), np.int64)
    ln = hi - lo
    lg = np.maximum(0, np.floor(np.log2(np.maximum(ln, 1))).astype(np.int64))
    lg = np.where((1 << lg) > ln, lg - 1, lg)
    mn, mx = np.empty(len(lo), x.dtype), np.empty(len(lo), x.dtype)
    with np.errstate(invalid="ignore"):
        for tabs, dst, fn in ((tm._sparse(x, np.minimum), mn, np.minimum), (tm._sparse(x, np.maximum), mx, np.maximum)):
            for k in np.unique(lg):
                sel = lg == k
                dst[sel] = fn(tabs[k][lo[sel]], tabs[k][hi[sel] - (1 << k)])
    return ne, _windows(x, lo, ln, S, A, emin, nnan, npinf, nninf, mn, mx)


def loop_windows(x, lo, hi):
    """the same by one loop per interval"""
    x = np.asarray(x)
    lo, hi = clamp(lo, hi, len(x))
    ne = hi > lo
    ints, emin = tm.dyadic(x)
    S, A, nn, npi, nni, mn, mx = [], [], [], [], [], [], []
    for a, b in zip(lo[ne], hi[ne]):
        s = t = c0 = c1 = c2 = 0
        lo_v = hi_v = None
        for j in range(int(a), int(b)):
            v = x[j]
            if x.dtype.kind == "f" and not np.isfinite(v):
                c0 += bool(np.isnan(v)); c1 += bool(v == np.inf); c2 += bool(v == -np.inf)
            else:
                s += ints[j]; t += abs(ints[j])
            lo_v = v if lo_v is None or v < lo_v else lo_v
            hi_v = v if hi_v is None or v > hi_v else hi_v
        S.append(s); A.append(t); nn.append(c0); npi.append(c1); nni.append(c2); mn.append(lo_v); mx.append(hi_v)
    return ne, _windows(x, lo[ne], (hi - lo)[ne], S, A, emin, np.array(nn, np.int64), np.array(npi, np.int64), np.array(nni, np.int64),
                        np.array(mn, x.dtype), np.array(mx, x.dtype))


# ---- the block tree, restated ----------------------------------------------------------------------------------------------------------
def tree_fold(x, lo, hi, op, fill=0, mutant=None):
    """list of Python values: op (SUM / MIN / MAX / COUNT; AVG = SUM / len) over x[lo:min(hi, n)] by the device's decomposition.
    Values are Python ints or floats, so integer sums are exact.  Empty: 0 for COUNT / SUM, `fill` otherwise."""
    assert mutant is None or mutant in TREE_MUTANTS
    x = np.asarray(x)
    n = len(x)
    v0 = [float(v) for v in x] if x.dtype.kind == "f" else [int(v) for v in x]
    if op in (SUM, AVG, COUNT):
        ident, f = 0, (lambda a, b: a + b)
    elif op == MIN:
        ident, f = None, (lambda a, b: b if a is None else a if b is None else (b if b < a else a))
    else:
        ident, f = None, (lambda a, b: b if a is None else a if b is None else (b if b > a else a))
    T, P, S = [v0], [None], [None]
    while len(T[-1]) > 1 or len(T) < 2:
        cur, nt, npre, nsuf = T[-1], [], [], []
        for b0 in range(0, len(cur), RX):
            blk = cur[b0:b0 + RX]
            acc = ident
            for v in blk:
                acc = f(acc, v)
            nt.append(acc)
        T.append(nt)
        for lvl in (nt,):
            pre, suf = [None] * len(lvl), [None] * len(lvl)
            for b0 in range(0, len(lvl), RX):
                acc = ident
                for q in range(b0, min(b0 + RX, len(lvl))):
                    acc = f(acc, lvl[q]); pre[q] = acc
                acc = ident
                for q in range(min(b0 + RX, len(lvl)) - 1, b0 - 1, -1):
                    acc = f(lvl[q], acc); suf[q] = acc
            if mutant == "suffix_prefix_swapped":
                pre, suf = suf, pre
            P.append(pre); S.append(suf)
    out = []
    for a, e in zip(lo, hi):
        a, e = int(a), min(int(e), n)
        if a >= e:
            out.append(0 if op in (COUNT, SUM) else (ident if mutant == "empty_as_identity" else fill))
            continue
        if op == COUNT:
            out.append(e - a)
            continue
        b, ln = e - 1, e - a
        left = mid = right = ident
        if a >> 6 == b >> 6:
            for q in range(a, b + 1):
                mid = f(mid, v0[q])
        else:
            for q in range(a, (a | 63) + 1):
                left = f(left, v0[q])
            for q in range(b & ~63, b + 1):
                right = f(right, v0[q])
            a, b = (a >> 6) + 1, (b >> 6) - 1
            k = 1
            while a <= b:
                if a >> 6 == b >> 6:
                    for q in range(a, b + 1):
                        mid = f(mid, T[k][q])
                    break
                if not (mutant == "level_skipped" and k == 1):
                    left = f(left, S[k][a])
                    right = f(P[k][b], right)
                a, b = (a >> 6) + 1, (b >> 6) - 1
                k += 1
        acc = f(f(left, mid), right)
        out.append(float(acc) / float(ln) if op == AVG else acc)     # (an exact integer sum rounds to double once)
    return out
