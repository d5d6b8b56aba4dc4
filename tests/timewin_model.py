"""The exact model of the time-range windows (include/aqg.h, time-range windows section), stated twice:

  loop_*     a plain loop per row that walks back from i while the predicate holds and folds the rows it passes;
  search_*   bisection on the stamps per slice plus exact integer prefix sums and a sparse table for min / max.

Values are dyadic rationals m 2^e (every finite double and every integer is one), so exact sums are integer arithmetic in units of
2^emin.  Non-finite rows are counted per window, never added.  A window is described by lo (its first position), and its aggregates
by `Windows`: the exact sum S and the sum of magnitudes A in those units, the counts of NaN / +Inf / -Inf rows, min and max."""
import bisect
import math
from fractions import Fraction

import numpy as np

OPEN, CLOSED = 0, 1
COUNT, SUM, AVG, MIN, MAX = range(5)
U64 = 2 ** 64 - 1


# ---- stamps ----------------------------------------------------------------------------------------------------------------------------
def date_col(ymd):
    """(n, 4) uint8 rows of the reference's date_t: day, month, int16 year"""
    a = np.zeros((len(ymd), 4), np.uint8)
    for i, (y, m, d) in enumerate(ymd):
        a[i, 0], a[i, 1] = d, m
        a[i, 2:4] = np.frombuffer(np.int16(y).tobytes(), np.uint8)
    return a


def time_col(hmsms):
    """(n, 8) uint8 rows of the reference's time_t: uint32 ms, seconds, minutes, hours, pad"""
    a = np.zeros((len(hmsms), 8), np.uint8)
    for i, (h, m, s, ms) in enumerate(hmsms):
        a[i, 0:4] = np.frombuffer(np.uint32(ms).tobytes(), np.uint8)
        a[i, 4], a[i, 5], a[i, 6] = s, m, h
    return a


def days_from_civil(y, m, d):
    y -= m <= 2
    era = (y if y >= 0 else y - 399) // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    return era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy


def stamps(t, kind=None):
    """(fp, list): exact Python ints for integer / 'date' / 'time' columns, Python floats (doubles) for floating ones"""
    t = np.asarray(t)
    if kind == "date":
        return False, [days_from_civil(int(np.frombuffer(r[2:4].tobytes(), np.int16)[0]), int(r[1]), int(r[0])) for r in t]
    if kind == "time":
        return False, [((int(r[6]) * 60 + int(r[5])) * 60 + int(r[4])) * 1000 + int(np.frombuffer(r[0:4].tobytes(), np.uint32)[0]) for r in t]
    if t.dtype.kind == "f":
        return True, [float(v) for v in t.astype(np.float64)]
    return False, [int(v) for v in t]


def span_ok(span, frame):
    return (span >= 0.0) if frame == CLOSED else (span > 0.0)              # (NaN fails both)


def dmax_of(span, frame):
    """the one exact limit of integer stamps: in window <=> d <= dmax"""
    if math.isinf(span):
        return U64
    return min(math.floor(span) if frame == CLOSED else math.ceil(span) - 1, U64)


def within(fp, ti, tj, span, frame):
    if fp:
        d = abs(ti - tj)                                                    # one rounded subtraction in double
        return d <= span if frame == CLOSED else d < span
    return abs(ti - tj) <= dmax_of(span, frame)


def slice_starts(n, starts):
    """start position of the slice of every row; starts: ascending first positions of the slices (None: one slice)"""
    if starts is None:
        return np.zeros(n, np.int64)
    s = np.asarray(starts, np.int64)
    return s[np.searchsorted(s, np.arange(n), side="right") - 1]


def loop_bounds(fp, st, starts, span, frame, rows=None):
    n = len(st)
    ss = slice_starts(n, starts)
    rows = range(n) if rows is None else rows
    lo = {}
    for i in rows:
        j = i
        while j > ss[i] and within(fp, st[i], st[j - 1], span, frame):
            j -= 1
        lo[i] = j
    return lo


def search_bounds(fp, st, starts, span, frame):
    n = len(st)
    lo = np.zeros(n, np.int64)
    edges = [0] if starts is None else [int(s) for s in starts]
    edges = edges + [n]
    dm = None if fp else dmax_of(span, frame)
    for a, b in zip(edges[:-1], edges[1:]):
        if b <= a:
            continue
        seg = st[a:b]
        if seg[-1] < seg[0]:
            seg = [-v for v in seg]                                         # descending: the image that ascends
        for k in range(b - a):
            if fp:
                c = bisect.bisect_left(seg, seg[k] - span, 0, k + 1)
                while c > 0 and within(True, seg[k], seg[c - 1], span, frame):
                    c -= 1
                while c < k and not within(True, seg[k], seg[c], span, frame):
                    c += 1
            else:
                c = bisect.bisect_left(seg, seg[k] - dm, 0, k + 1)
            lo[a + k] = a + c
    return lo


# ---- values ----------------------------------------------------------------------------------------------------------------------------
def dyadic(x):
    """(ints, emin): finite x[i] == ints[i] * 2^emin exactly; non-finite rows are 0 there"""
    x = np.asarray(x)
    if x.dtype.kind != "f":
        return [int(v) for v in x], 0
    xd = x.astype(np.float64)
    fin = np.isfinite(xd)
    m, e = np.frexp(np.where(fin, xd, 0.0))
    mi = (m * 2.0 ** 53).astype(np.int64)                                  # exact: |m| < 1 with 53 bits
    ee = e.astype(np.int64) - 53
    nz = mi != 0
    emin = int(ee[nz].min()) if nz.any() else 0
    return [int(a) << int(b - emin) if a else 0 for a, b in zip(mi, ee)], emin


class Windows:
    """the aggregates of the windows [lo[i], i]: everything a check needs, exact"""

    def __init__(self, x, lo, S, A, emin, nnan, npinf, nninf, mn, mx):
        self.x, self.lo, self.S, self.A, self.emin = x, lo, S, A, emin
        self.nnan, self.npinf, self.nninf, self.mn, self.mx = nnan, npinf, nninf, mn, mx
        self.len = np.arange(len(lo)) - lo + 1


def loop_windows(x, lo, rows=None):
    x = np.asarray(x)
    ints, emin = dyadic(x)
    out = {}
    for i in (range(len(x)) if rows is None else rows):
        S = A = nn = npi = nni = 0
        mn = mx = None
        for j in range(int(lo[i]), i + 1):
            v = x[j]
            if x.dtype.kind == "f" and not np.isfinite(v):
                nn += bool(np.isnan(v)); npi += bool(v == np.inf); nni += bool(v == -np.inf)
            else:
                S += ints[j]; A += abs(ints[j])
            mn = v if mn is None or v < mn else mn
            mx = v if mx is None or v > mx else mx
        out[i] = (S, A, nn, npi, nni, mn, mx)
    return out, emin


def _sparse(x, fn):
    tabs = [x]
    k = 1
    while 2 * k <= len(x):
        p = tabs[-1]
        tabs.append(fn(p[:-k], p[k:]))
        k *= 2
    return tabs


def search_windows(x, lo):
    x = np.asarray(x)
    lo = np.asarray(lo, np.int64)
    n = len(x)
    ints, emin = dyadic(x)
    PS, PA = [0] * (n + 1), [0] * (n + 1)
    for i, v in enumerate(ints):
        PS[i + 1] = PS[i] + v
        PA[i + 1] = PA[i] + abs(v)
    S = [PS[i + 1] - PS[int(lo[i])] for i in range(n)]
    A = [PA[i + 1] - PA[int(lo[i])] for i in range(n)]
    idx = np.arange(n)

    def cnt(mask):                                                          # counts are integers: their prefix difference is exact
        c = np.concatenate([[0], np.cumsum(mask)])
        return c[idx + 1] - c[lo]
    if x.dtype.kind == "f":
        nnan, npinf, nninf = cnt(np.isnan(x)), cnt(x == np.inf), cnt(x == -np.inf)
    else:
        nnan = npinf = nninf = np.zeros(n, np.int64)
    ln = idx - lo + 1
    lg = np.maximum(0, np.floor(np.log2(np.maximum(ln, 1))).astype(np.int64))
    lg = np.where((1 << lg) > ln, lg - 1, lg)
    mn, mx = np.empty_like(x), np.empty_like(x)
    with np.errstate(invalid="ignore"):
        for tabs, dst, fn in ((_sparse(x, np.minimum), mn, np.minimum), (_sparse(x, np.maximum), mx, np.maximum)):
            for k in np.unique(lg):
                sel = lg == k
                dst[sel] = fn(tabs[k][lo[sel]], tabs[k][idx[sel] + 1 - (1 << k)])
    return Windows(x, lo, S, A, emin, nnan, npinf, nninf, mn, mx)


# ---- what a device answer is held to ------------------------------------------------------------------------------------------------------
def expected_class(w, i):
    """the non-finite class of window i's floating sum: 'nan', '+inf', '-inf' or None (finite)"""
    if w.nnan[i] or (w.npinf[i] and w.nninf[i]):
        return "nan"
    if w.npinf[i]:
        return "+inf"
    if w.nninf[i]:
        return "-inf"
    return None


def sum_share(w, got, avg=False):
    """worst |got - exact| / bound over the finite windows of a floating SUM (AVG); raises on a window of the wrong non-finite class
    or beyond its bound.  bound = m u / (1 - m u) sum|x|, m = len - 1 (AVG: over len, plus u |avg|); windows whose sum|x| reaches
    2^1023 are outside the contract.  Windows far inside the bound are accepted in double arithmetic (with the roundings of that
    comparison charged to them), the others go through exact fractions."""
    got = np.asarray(got, np.float64)
    n = len(got)
    den, mul = 1 << max(0, -w.emin), 1 << max(0, w.emin)

    def tof(v):
        try:
            return (v * mul) / den                                          # int / int: correctly rounded
        except OverflowError:
            return math.inf if v > 0 else -math.inf
    Sf, Af = np.array([tof(v) for v in w.S]), np.array([tof(v) for v in w.A])
    nan = (w.nnan > 0) | ((w.npinf > 0) & (w.nninf > 0))
    pinf, ninf = ~nan & (w.npinf > 0), ~nan & (w.nninf > 0)
    assert np.isnan(got[nan]).all(), ("a window that holds a NaN (or both Infs) is not NaN", np.flatnonzero(nan & ~np.isnan(got))[:5])
    assert np.all(got[pinf] == np.inf) and np.all(got[ninf] == -np.inf), "a window that holds one kind of Inf is not that Inf"
    fin = ~(nan | pinf | ninf) & (Af < 2.0 ** 1023)
    assert np.isfinite(got[fin]).all(), ("a finite window came out non-finite", np.flatnonzero(fin & ~np.isfinite(got))[:5])
    ln = w.len.astype(np.float64)
    m = ln - 1.0
    with np.errstate(over="ignore", invalid="ignore"):
        bound = m / (2.0 ** 53 - m) * Af
        exact = Sf
        if avg:
            exact, bound = Sf / ln, bound / ln + np.abs(Sf / ln) * 2.0 ** -53
        err = np.abs(got - exact)
        fast = fin & (err + 2.0 * np.spacing(np.abs(exact)) <= bound * (1.0 - 1e-9))
        worst = float(np.max(err[fast] / bound[fast])) if fast.any() else 0.0
    scale = Fraction(2) ** w.emin
    for i in np.flatnonzero(fin & ~fast):
        mi, li = int(w.len[i]) - 1, int(w.len[i])
        ex, mag = w.S[i] * scale, w.A[i] * scale
        bd = Fraction(mi, 2 ** 53 - mi) * mag
        if avg:
            ex, bd = ex / li, bd / li + abs(ex / li) / 2 ** 53
        e = abs(Fraction(float(got[i])) - ex)
        if e == 0:
            continue
        assert bd > 0 and e <= bd, ("window %d: |got - exact| = %.3g beyond the bound %.3g" % (i, float(e), float(bd)))
        worst = max(worst, float(e / bd))
    return worst


def exact_int_sum(w):
    """integer column: the exact sums as (lo, hi) uint64 words of the 128-bit two's complement value"""
    out = np.zeros(len(w.S), np.dtype([("lo", "<u8"), ("hi", "<u8")]))
    for i, s in enumerate(w.S):
        s &= (1 << 128) - 1
        out[i] = (s & U64, s >> 64)
    return out


def exact_int_avg(w):
    """integer column: the exact sum rounded to double, divided by len"""
    return np.array([float(s) / float(ln) for s, ln in zip(w.S, w.len)], np.float64)
