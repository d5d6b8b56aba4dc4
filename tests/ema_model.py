"""The exact model of the exponential moving averages (include/aqg.h, exponential moving averages section): the recurrences
evaluated over the rationals and rounded once.

Every input is a double, hence a dyadic rational m * 2^e, and the recurrences only multiply and add: all values stay dyadic, so the
model carries (m, e) pairs of Python integers -- the same numbers fractions.Fraction would hold, without a gcd per step -- and makes
one correctly rounded division at the end.  The doubles alpha,
d = fl(1 - alpha), decay[i] and fl(1 - decay[i]) are taken as the exact rationals they are, x as the double it converts to.

    exact_ema(x, starts, mode, alpha=..., decay=...)  ->  EmaResult(y, M, poisoned)

`starts`: ascending positions at which a slice (group) starts, position 0 included; None = one slice.  `decay` is in the layout of x.
y[i] is the correctly rounded exact value (NaN from a slice's first non-finite row on), M[i] = max |x_j| over the slice's rows up to i,
poisoned[i] = row i lies at or behind its slice's first non-finite row (x NaN / +-Inf, or a decay that is NaN or outside [0, 1]; a
slice's first decay is never read).

An exact value of row i of a slice has about 53 i bits, so the model is quadratic in the slice length: fine for the thousands of rows a
tile edge needs, hopeless for millions.  For those, `wide_ema` evaluates the same recurrences in numpy's extended precision (64-bit
significand), blocked so that it is vector code; it is one more bracketing of the same maps, so the derived bound holds for it with
2^-64 in place of 2^-53, which `wide_err` returns -- the tests subtract that from the bound they allow the device.  Finite data only.
"""
from collections import namedtuple
import math

import numpy as np

RECURSIVE, ADJUSTED = 0, 1
U = 2.0 ** -53
C_BOUND = {RECURSIVE: 4.0, ADJUSTED: 9.0}

EmaResult = namedtuple("EmaResult", "y M poisoned")


def to_double(x):
    """the column as the doubles the device converts it to (round to nearest: exact but for 64-bit integers)"""
    return np.ascontiguousarray(np.asarray(x)).astype(np.float64)


def bound(mode, M, pos):
    """the asserted error bound of a finite row at position `pos` of its slice: 4 (i + 2) u M_i resp. 9 (i + 2) u M_i"""
    return C_BOUND[mode] * (np.asarray(pos, np.float64) + 2.0) * U * np.asarray(M, np.float64)


def slice_positions(n, starts):
    """position of every row inside its slice"""
    s = np.zeros(n, np.int64)
    st = np.asarray([0] if starts is None else starts, np.int64)
    s[st] = st
    return np.arange(n, dtype=np.int64) - np.maximum.accumulate(s)


def coefficients(n, alpha=None, decay=None):
    """(a, b) as doubles: a_i = fl(1 - alpha), b_i = alpha, or a_i = decay[i], b_i = fl(1 - decay[i])"""
    if decay is not None:
        a = np.asarray(decay, np.float64)
        with np.errstate(invalid="ignore"):
            return a, 1.0 - a
    return np.full(n, 1.0 - float(alpha)), np.full(n, float(alpha))


# ---- dyadic rationals as (m, e) = m * 2^e ------------------------------------------------------------------------------------
def _dy(f):
    num, den = float(f).as_integer_ratio()
    return num, 1 - den.bit_length()                      # den = 2^k


def _mul(p, q):
    return p[0] * q[0], p[1] + q[1]


def _add(p, q):
    if p[1] < q[1]:
        p, q = q, p
    return (p[0] << (p[1] - q[1])) + q[0], q[1]


def _ratio(p, q):
    """p / q (q > 0) correctly rounded.  The leading 192 bits of both decide it almost always: the quotients of the truncations
    bracket the true one, int / int rounds correctly and monotonically, so when both ends round to the same double that is the
    answer; otherwise the whole integers are divided.  The power of two left over is exact while the result is a normal double."""
    (m, e), (d, f) = p, q
    if m == 0:
        return 0.0
    sign, m = (-1.0, -m) if m < 0 else (1.0, m)
    sm, sd = max(0, m.bit_length() - 192), max(0, d.bit_length() - 192)
    mlo, dlo = m >> sm, d >> sd
    lo, hi = mlo / (dlo + (1 if sd else 0)), (mlo + (1 if sm else 0)) / dlo
    if lo == hi:
        return sign * math.ldexp(lo, e + sm - f - sd)
    sh = m.bit_length() - d.bit_length()
    return sign * math.ldexp((m << max(0, -sh)) / (d << max(0, sh)), e - f + sh)


def _to_float(p):
    return _ratio(p, (1, 0))


def exact_ema(x, starts, mode, alpha=None, decay=None):
    xd = to_double(x)
    n = len(xd)
    a, b = coefficients(n, alpha, decay)
    st = set([0] if starts is None else [int(s) for s in starts])
    y = np.empty(n, np.float64)
    M = np.empty(n, np.float64)
    poisoned = np.zeros(n, bool)
    ONE = (1, 0)
    num = den = None
    m_run, bad = 0.0, False
    for i in range(n):
        first = i in st
        if first:
            m_run, bad = 0.0, False
        xi = float(xd[i])
        ok = np.isfinite(xi) and (first or (0.0 <= a[i] <= 1.0))
        if not ok:
            bad = True
        if bad:
            poisoned[i], y[i], M[i] = True, np.nan, m_run
            continue
        m_run = max(m_run, abs(xi))
        M[i] = m_run
        if mode == RECURSIVE:
            num = _dy(xi) if first else _add(_mul(_dy(a[i]), num), _mul(_dy(b[i]), _dy(xi)))
            y[i] = _to_float(num)
        else:
            if first:
                num, den = _dy(xi), ONE
            else:
                ai = _dy(a[i])
                num, den = _add(_mul(ai, num), _dy(xi)), _add(_mul(ai, den), ONE)
            y[i] = _ratio(num, den)
    return EmaResult(y, M, poisoned)


# ---- extended precision, for slices too long for the exact model ---------------------------------------------------------------------
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "wide_ema needs a 64-bit significand"
U_WIDE = 2.0 ** -64


def _linrec(a, c, L=2048):
    """z[i] = a[i] z[i-1] + c[i] (z[-1] = 0) in extended precision: blocks of L rows advance side by side, then take their carries"""
    n = len(a)
    B = -(-n // L)
    A = np.ones(B * L, LD); A[:n] = a
    Cc = np.zeros(B * L, LD); Cc[:n] = c
    A = np.ascontiguousarray(A.reshape(B, L).T)            # [L, B]: one step of every block is one contiguous row
    Cc = np.ascontiguousarray(Cc.reshape(B, L).T)
    Z = np.empty_like(Cc); P = np.empty_like(A)
    Z[0], P[0] = Cc[0], A[0]
    for j in range(1, L):
        Z[j] = A[j] * Z[j - 1] + Cc[j]
        P[j] = A[j] * P[j - 1]
    carry = np.zeros(B, LD)
    z = LD(0)
    for k in range(B):
        carry[k] = z
        z = P[L - 1, k] * z + Z[L - 1, k]
    Z += P * carry[None, :]
    return np.ascontiguousarray(Z.T).reshape(-1)[:n]


def wide_ema(x, starts, mode, alpha=None, decay=None):
    """EmaResult with y in extended precision (within wide_err of the exact value); finite rows and good decays only"""
    xd = to_double(x)
    n = len(xd)
    a, b = coefficients(n, alpha, decay)
    st = np.asarray([0] if starts is None else starts, np.int64)
    assert np.isfinite(xd).all() and ((a >= 0) & (a <= 1)).all()
    a = a.astype(LD); a[st] = 0
    xl = xd.astype(LD)
    if mode == RECURSIVE:
        w = b.astype(LD); w[st] = 1
        y = _linrec(a, w * xl)
    else:
        y = _linrec(a, xl) / _linrec(a, np.ones(n, LD))
    pos = slice_positions(n, starts)
    M = np.abs(xd)
    for lo, hi in zip(st, list(st[1:]) + [n]):
        M[lo:hi] = np.maximum.accumulate(M[lo:hi])
    return EmaResult(y, M, np.zeros(n, bool)), pos


def wide_err(mode, M, pos):
    return C_BOUND[mode] * (np.asarray(pos, np.float64) + 2.0) * U_WIDE * np.asarray(M, np.float64)


# ---- the reference the tests hold the device to --------------------------------------------------------------------------------------
EXACT_MAX = 1600                                           # rows of a slice up to which the exact model is affordable
Reference = namedtuple("Reference", "y M poisoned pos err")


def reference_ema(x, starts, mode, alpha=None, decay=None, exact_max=EXACT_MAX):
    """slice by slice: the exact model (err = 0: y is the correctly rounded exact value), or, for a finite slice of more than
    `exact_max` rows, the extended-precision evaluation with err = wide_err.  y is returned in extended precision either way;
    a test allows the device  bound - err."""
    xd = to_double(x)
    n = len(xd)
    st = [0] if starts is None else [int(v) for v in starts]
    y, M, poisoned, err = np.empty(n, LD), np.empty(n, np.float64), np.zeros(n, bool), np.zeros(n, np.float64)
    for lo, hi in zip(st, st[1:] + [n]):
        dec = None if decay is None else np.asarray(decay, np.float64)[lo:hi]
        tame = np.isfinite(xd[lo:hi]).all() and (dec is None or ((dec[1:] >= 0) & (dec[1:] <= 1)).all())
        if hi - lo > exact_max and tame:
            if dec is not None:
                dec = dec.copy(); dec[0] = 1.0             # (never read; wide_ema wants it valid)
            r, pos = wide_ema(xd[lo:hi], None, mode, alpha=alpha, decay=dec)
            err[lo:hi] = wide_err(mode, r.M, pos)
        else:
            r = exact_ema(xd[lo:hi], None, mode, alpha=alpha, decay=dec)
        y[lo:hi], M[lo:hi], poisoned[lo:hi] = r.y, r.M, r.poisoned
    return Reference(y, M, poisoned, slice_positions(n, starts), err)


# ---- the tiled composition in doubles, with planted mistakes -----------------------------------------------------------------------
FAULTS = ("tile_carry_dropped", "carry_across_group", "op_swapped", "alpha_for_d", "first_decay_read", "den_not_restarted",
          "decay_row_layout", "divide_before_carry")


def tiled_ema(x, starts, mode, alpha=None, decay=None, tile=2048, fault=None, decay_row=None):
    """the reduce-then-scan composition restated in doubles: every tile composes its rows' maps from the identity, then takes the map
    of everything before it as carry-in.  `fault` plants one of FAULTS (decay_row: the decay column in ROW layout, for the fault that
    reads it where the flat one was meant).  Finite rows only."""
    xd = to_double(x)
    n = len(xd)
    if fault == "decay_row_layout" and decay is not None and decay_row is not None:
        decay = decay_row
    a, b = coefficients(n, alpha, decay)
    if fault == "alpha_for_d" and decay is None:
        a = b.copy()
    st = np.zeros(n, bool)
    st[[0] if starts is None else list(starts)] = True
    if fault == "carry_across_group":
        st[1:] = False
    adj = mode == ADJUSTED
    y = np.empty(n, np.float64)
    if fault == "den_not_restarted" and adj:               # the numerator restarts at a group start, the denominator runs on
        num = den = 0.0
        for i in range(n):
            num = xd[i] if st[i] else a[i] * num + xd[i]
            den = 1.0 if i == 0 else a[i] * den + 1.0
            y[i] = num / den
        return y
    ca, cn, cd = 1.0, 0.0, 0.0                              # the map of everything before the tile: y -> ca y + cn (cd: denominator)
    for t0 in range(0, n, tile):
        la, ln, ld = 1.0, 0.0, 0.0                          # the tile's own map so far
        if fault == "tile_carry_dropped":
            ca, cn, cd = 1.0, 0.0, 0.0
        for i in range(t0, min(n, t0 + tile)):
            xi = xd[i]
            if st[i]:
                ra = 0.0
                if fault == "first_decay_read" and decay is not None:
                    rn, rd = (xi, 1.0) if adj else (b[i] * xi, 0.0)
                else:
                    rn, rd = xi, 1.0
            else:
                ra = a[i]
                rn, rd = (xi, 1.0) if adj else (b[i] * xi, 0.0)
            la, ln, ld = la * ra, ra * ln + rn, ra * ld + rd
            if fault == "op_swapped":
                fa, fn, fd = la * ca, ca * ln + cn, ca * ld + cd        # carry applied AFTER the tile's map
            else:
                fa, fn, fd = ca * la, la * cn + ln, la * cd + ld
            if fault == "divide_before_carry" and adj:
                y[i] = ln / ld + (la * (cn / cd) if cd else 0.0)
            else:
                y[i] = fn / fd if adj else fn
        ca, cn, cd = ca * la, la * cn + ln, la * cd + ld
    return y

