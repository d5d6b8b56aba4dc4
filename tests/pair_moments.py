"""Exact moving and running cov / corr / beta of two columns laid out by group offsets (host only): the truth the pair windows
(aqg_scan2 / aqg_grouped_scan2 / aqg_grouped_scan2_flat) are measured against, built on exact_moments.py.

Both columns are brought to Python integers (x = ints / 2^mx, y = ints / 2^my), prefix sums of x, y, x^2, y^2 and xy are taken in Python
ints, and with L the window's length every
    C = (L Sxy - Sx Sy) / L^2,   Vx = (L Sxx - Sx^2) / L^2,   Vy = (L Syy - Sy^2) / L^2
is one exact rational, rounded once to double (int / int is correctly rounded).  beta = C / Vx is a ratio of two integers, rounded once
as well; corr = C / sqrt(Vx Vy) is the integer square root of the rational rho^2 scaled by 2^160 -- 80 bits, rounded once to double.

The accuracy contract generalises exact_moments.bound.  Rx, Ry: the window's ranges on the short routes (the clamped window is at most
SHORT_W rows), the group's ranges so far on the prefix route; c = 1e-12 for the short routes and the running ops, 1e-10 for longer windows.
    cov   |got - C| <= bC = 1e-9 |C| + c Rx Ry                       (bVx = 1e-9 Vx + c Rx^2, bVy alike: the variance contract)
    corr  tol = bC / sqrt(Vx Vy) + |rho| (bVx / Vx + bVy / Vy) / 2 + 4 * 2^-52
    beta  tol = bC / Vx + |beta| bVx / Vx + 4 * 2^-52 |beta|
A position with tol > ILL_TOL (or an exact variance of 0 over a range that is not 0) is ILL-CONDITIONED: there a corr must be NaN or lie
in [-1, 1], and a beta is not held to a value.  Where the exact variance is 0 AND the range is 0 (every difference the kernel takes is
exactly 0), corr / beta must be exactly NaN."""
import math

import numpy as np

from exact_moments import _as_ints, pos_in_group, window_range, running_range

COV, CORR, BETA = 0, 1, 2
SHORT_W = 64
ILL_TOL = 1e-6
EPS4 = 4 * 2.0 ** -52


def short_route(w, n):
    """does the window op with window w over n rows take one of the two short routes (the window is clamped by the column)"""
    return w is not None and min(int(w), n) <= SHORT_W


def _prefix(v):
    zero = np.array([0], dtype=object)
    return np.concatenate([zero, np.cumsum(v)]) if len(v) else zero


def _round_ratio(num, den):
    """the object arrays num / den as float64, every element rounded once (den > 0)"""
    return np.array([a / b for a, b in zip(num.tolist(), den.tolist())], dtype=np.float64)


def _corr_exact(cn, vxn, vyn):
    out = np.full(len(cn), np.nan)
    for i, (c, a, b) in enumerate(zip(cn.tolist(), vxn.tolist(), vyn.tolist())):
        d = a * b
        if d > 0:
            r = math.isqrt((c * c << 160) // d)
            out[i] = math.copysign(r / (1 << 80), c) if c else 0.0
    return out


def _shifted(num, den, e):
    """num / den * 2^e for python ints"""
    return (num << e) / den if e >= 0 else num / (den << -e)


class PairExact:
    """the prefix sums of the two columns, made once; moments(w) per window length (w=None: the running ops)"""

    def __init__(self, x, y, offsets=None):
        self.x, self.y, self.offsets = np.asarray(x), np.asarray(y), offsets
        assert len(self.x) == len(self.y)
        self.n = len(self.x)
        vx, self.mx = _as_ints(self.x)
        vy, self.my = _as_ints(self.y)
        self.S = {"x": _prefix(vx), "y": _prefix(vy), "xx": _prefix(vx * vx), "yy": _prefix(vy * vy), "xy": _prefix(vx * vy)}
        self.pos = pos_in_group(self.n, offsets)
        self._rr = None
        self._cache = {}

    def length(self, w):
        return self.pos + 1 if w is None else np.minimum(self.pos + 1, int(w))

    def moments(self, w=None):
        """{"C", "Vx", "Vy", "corr", "beta"} as float64 arrays (corr / beta NaN where the exact Vx Vy / Vx is 0) and the exact-zero masks
        "vx0", "vy0\""""
        key = None if w is None else min(int(w), max(self.n, 1))
        if key in self._cache:
            return self._cache[key]
        n = self.n
        if n == 0:
            z = np.zeros(0)
            return {"C": z, "Vx": z, "Vy": z, "corr": z, "beta": z, "vx0": z.astype(bool), "vy0": z.astype(bool)}
        length = self.length(w)
        hi = np.arange(1, n + 1)
        lo = hi - length
        d = {k: s[hi] - s[lo] for k, s in self.S.items()}
        L = length.astype(object)
        cn, vxn, vyn = L * d["xy"] - d["x"] * d["y"], L * d["xx"] - d["x"] * d["x"], L * d["yy"] - d["y"] * d["y"]
        LL = L * L
        out = {"C": _round_ratio(cn, LL * (1 << (self.mx + self.my))), "Vx": _round_ratio(vxn, LL * (1 << (2 * self.mx))),
               "Vy": _round_ratio(vyn, LL * (1 << (2 * self.my)))}
        out["vx0"] = np.array([v == 0 for v in vxn.tolist()])
        out["vy0"] = np.array([v == 0 for v in vyn.tolist()])
        out["corr"] = _corr_exact(cn, vxn, vyn)
        e = self.mx - self.my                                    # beta = cn / vxn * 2^(mx - my)
        out["beta"] = np.array([_shifted(c, v, e) if v > 0 else np.nan for c, v in zip(cn.tolist(), vxn.tolist())], dtype=np.float64)
        self._cache[key] = out
        return out

    def ranges(self, w):
        """(Rx, Ry, c) of the contract for the window op w (None: running)"""
        if short_route(w, self.n):
            return window_range(self.x, w, self.offsets), window_range(self.y, w, self.offsets), 1e-12
        if self._rr is None:
            self._rr = running_range(self.x, self.offsets), running_range(self.y, self.offsets)
        return self._rr[0], self._rr[1], 1e-12 if w is None else 1e-10

    def tolerances(self, fam, w=None):
        """(want, tol, ill, must_nan): the exact values, the contract's bound (inf where ill-conditioned), the ill-conditioned positions
        and the positions that must be exactly NaN"""
        m = self.moments(w)
        Rx, Ry, c = self.ranges(w)
        bC = 1e-9 * np.abs(m["C"]) + c * Rx * Ry
        if fam == COV:
            none = np.zeros(self.n, bool)
            return m["C"], bC, none, none
        bVx, bVy = 1e-9 * m["Vx"] + c * Rx * Rx, 1e-9 * m["Vy"] + c * Ry * Ry
        with np.errstate(divide="ignore", invalid="ignore"):
            if fam == CORR:
                want = m["corr"]
                zero = m["vx0"] | m["vy0"]
                must_nan = (m["vx0"] & (Rx == 0)) | (m["vy0"] & (Ry == 0))
                tol = bC / np.sqrt(m["Vx"] * m["Vy"]) + np.abs(want) * (bVx / m["Vx"] + bVy / m["Vy"]) / 2 + EPS4
            else:
                want = m["beta"]
                zero = m["vx0"]
                must_nan = m["vx0"] & (Rx == 0)
                tol = bC / m["Vx"] + np.abs(want) * bVx / m["Vx"] + EPS4 * np.abs(want)
        ill = (zero & ~must_nan) | (~zero & ~(tol <= ILL_TOL))
        tol = np.where(ill | zero, np.inf, tol)
        return want, tol, ill, must_nan

    def check(self, got, fam, w=None, what="", upto=None):
        """assert the contract over positions [0, upto) (None: all); returns the number of ill-conditioned positions among them"""
        got = np.asarray(got, dtype=np.float64)
        want, tol, ill, must_nan = self.tolerances(fam, w)
        if isinstance(upto, np.ndarray):                         # (a mask of the positions to hold)
            sel = upto.astype(bool)
        else:
            sel = np.zeros(self.n, bool)
            sel[:self.n if upto is None else upto] = True
        held = sel & ~ill & ~must_nan
        bad = held & ~(np.abs(got - want) <= tol)
        if bad.any():
            i = int(np.argmax(bad))
            raise AssertionError(f"{what}: {int(bad.sum())} of {int(held.sum())} positions out of bounds; first at {i}: got {got[i]!r}, "
                                 f"exact {want[i]!r}, bound {tol[i]!r}")
        nn = sel & must_nan & ~np.isnan(got)
        assert not nn.any(), f"{what}: a constant range must give exactly NaN; first at {int(np.argmax(nn))}: got {got[int(np.argmax(nn))]!r}"
        if fam == CORR:
            loose = sel & ill & ~(np.isnan(got) | (np.abs(got) <= 1.0))
            assert not loose.any(), f"{what}: an ill-conditioned corr must be NaN or lie in [-1, 1]; first at {int(np.argmax(loose))}"
        return int((sel & ill).sum())


def direct(x, y, offsets, fam, w=None):
    """the model stated a second way: an O(n w) double loop over Fractions (small cases); corr as (rho^2, sign)"""
    from fractions import Fraction
    x, y = np.asarray(x), np.asarray(y)
    n = len(x)
    fx, fy = [Fraction(v) for v in x.tolist()], [Fraction(v) for v in y.tolist()]
    pos = pos_in_group(n, offsets)
    out = []
    for i in range(n):
        L = int(pos[i]) + 1 if w is None else min(int(pos[i]) + 1, int(w))
        xs, ys = fx[i + 1 - L:i + 1], fy[i + 1 - L:i + 1]
        mx, my = sum(xs) / L, sum(ys) / L
        c = sum((a - mx) * (b - my) for a, b in zip(xs, ys)) / L
        vx, vy = sum((a - mx) ** 2 for a in xs) / L, sum((b - my) ** 2 for b in ys) / L
        if fam == COV:
            out.append(float(c))
        elif fam == BETA:
            out.append(float(c / vx) if vx else math.nan)
        else:
            out.append(math.copysign(math.sqrt(c * c / (vx * vy)), c) if vx * vy else math.nan)
    return np.array(out, dtype=np.float64)
