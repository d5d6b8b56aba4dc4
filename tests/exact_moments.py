"""Exact running and windowed variances of a column laid out by group offsets (host only): the truth the variance scans are measured
against.  Every finite double is k / 2^m, so the column is brought to Python integers (scaled by a common 2^m), prefix sums of x and
x^2 are taken in Python ints (object arrays), and every result (w Q - S^2) / w^2 is one exact rational, rounded once to double
(int / int is correctly rounded).  O(n) for any window.

Windows are clamped at the group's start and give the population variance, as the oracle defines varw (oracle/aq_oracle.c, D9)."""
import numpy as np


def _as_ints(x):
    """(python ints as an object array, m) with x = ints / 2^m exactly"""
    x = np.asarray(x)
    if x.dtype.kind in "iub":
        return x.astype(object), 0
    ratios = [v.as_integer_ratio() for v in x.astype(np.float64).tolist()]
    m = max((d.bit_length() - 1 for _, d in ratios), default=0)
    return np.array([num << (m - (d.bit_length() - 1)) for num, d in ratios], dtype=object), m


def _offsets(n, offsets):
    off = np.asarray([0, n] if offsets is None else offsets, dtype=np.int64)
    if off[-1] != n:
        off = np.concatenate([off, [n]])
    return off


def pos_in_group(n, offsets=None):
    """predecessors of every position inside its group"""
    off = _offsets(n, offsets)
    counts = np.diff(off)
    return np.arange(n, dtype=np.int64) - np.repeat(off[:-1], counts)


class Exact:
    """the column's prefix sums of x and x^2 in Python ints, made once; var(w) per window length"""

    def __init__(self, x, offsets=None):
        self.x, self.offsets = np.asarray(x), offsets
        self.n = n = len(self.x)
        v, self.m = _as_ints(self.x)
        zero = np.array([0], dtype=object)
        self.S = np.concatenate([zero, np.cumsum(v)]) if n else zero
        self.Q = np.concatenate([zero, np.cumsum(v * v)]) if n else zero
        self.pos = pos_in_group(n, offsets)
        self._rr = None

    def var(self, w=None):
        """population variance of the last min(w, position in group + 1) elements of every position's group; w=None: the whole
        group so far (the running variance, vars)"""
        if self.n == 0:
            return np.zeros(0)
        length = self.pos + 1 if w is None else np.minimum(self.pos + 1, int(w))
        hi = np.arange(1, self.n + 1)
        lo = hi - length
        s, q = self.S[hi] - self.S[lo], self.Q[hi] - self.Q[lo]
        L = length.astype(object)
        return ((L * q - s * s) / (L * L * (1 << (2 * self.m)))).astype(np.float64)

    def running_range(self):
        if self._rr is None:
            self._rr = running_range(self.x, self.offsets)
        return self._rr

    def check(self, got, T, w=None, sd=False, what=""):
        check(got, self.x, T, w, self.offsets, sd, what, rr=None if (w is not None and int(w) <= SHORT_W) else self.running_range())


def window_var(x, w, offsets=None):
    return Exact(x, offsets).var(w)


def running_var(x, offsets=None):
    return Exact(x, offsets).var(None)


def running_range(x, offsets=None):
    """max - min of each group's values up to every position (in double)"""
    a = np.asarray(x).astype(np.float64)
    pos = pos_in_group(len(a), offsets)
    hi, lo = a.copy(), a.copy()
    k = 1
    while k < len(a):
        ok = pos[k:] >= k
        hi[k:] = np.where(ok, np.maximum(hi[k:], hi[:-k]), hi[k:])
        lo[k:] = np.where(ok, np.minimum(lo[k:], lo[:-k]), lo[k:])
        k *= 2
    return hi - lo


def window_range(x, w, offsets=None):
    """max - min of every clamped window's values (O(n w): short windows)"""
    a = np.asarray(x).astype(np.float64)
    pos = pos_in_group(len(a), offsets)
    hi, lo = a.copy(), a.copy()
    for k in range(1, min(int(w), len(a))):
        ok = pos[k:] >= k
        hi[k:] = np.where(ok, np.maximum(hi[k:], a[:-k]), hi[k:])
        lo[k:] = np.where(ok, np.minimum(lo[k:], a[:-k]), lo[k:])
    return hi - lo


SHORT_W = 64


def bound(x, T, w=None, offsets=None, rr=None):
    """the accuracy contract of the variance scans: |got - T| <= 1e-9 T + c R^2 -- c = 1e-12 with R the window's range for vars and
    windows of up to 64, c = 1e-10 with R the group's range so far for longer windows"""
    if w is not None and int(w) <= SHORT_W:
        R, c = window_range(x, w, offsets), 1e-12
    else:
        R, c = running_range(x, offsets) if rr is None else rr, 1e-12 if w is None else 1e-10
    return 1e-9 * T + c * R * R, R


def check(got, x, T, w=None, offsets=None, sd=False, what="", rr=None):
    """assert the contract for a var (sd=False) or stddev (sd=True) result against the exact variance T"""
    b, R = bound(x, T, w, offsets, rr)
    got = np.asarray(got, dtype=np.float64)
    want = np.sqrt(T) if sd else T
    tol = np.sqrt(b) if sd else b
    err = np.abs(got - want)
    bad = ~(err <= tol)
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(got)} positions out of bounds; first at {i}: got {got[i]!r}, "
                             f"exact {want[i]!r}, bound {tol[i]!r}")
    assert np.all(got[R == 0] == 0), f"{what}: a constant range must give exactly 0"
