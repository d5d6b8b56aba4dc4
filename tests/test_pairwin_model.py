"""The exact model of the pair windows (tests/pair_moments.py) without a GPU: stated a second way, held to pandas' recorded answers, the
ill-conditioned cap over the whole case list, and planted mistakes in a numpy restatement of the kernels' arithmetic, each of which at
least one case must refuse."""
import json
import os

import numpy as np
import pytest

import pair_moments as pm
import pairwin_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
FAMS = (pm.COV, pm.CORR, pm.BETA)


def small_cases():
    rng = np.random.default_rng(99)
    out = []
    for (tx, ty), fam, sizes in (((np.int32, np.int32), "centred", [150]), ((np.float64, np.float32), "offset", [1, 2, 40, 3, 80]),
                                 ((np.uint8, np.int64), "centred", [70, 1, 66]), ((np.int16, np.int16), "constant", [90, 5])):
        n = sum(sizes)
        x, y = pc.pair_columns(rng, fam, tx, ty, n)
        out.append((x, y, np.concatenate([[0], np.cumsum(sizes)])))
    return out


def test_the_model_stated_a_second_way():
    for x, y, off in small_cases():
        ex = pm.PairExact(x, y, off)
        for w in (None, 1, 2, 3, 9, 65, 150):
            m = ex.moments(w)
            for fam, key in ((pm.COV, "C"), (pm.BETA, "beta")):
                want = pm.direct(x, y, off, fam, w)
                assert np.array_equal(m[key], want, equal_nan=True), (fam, w)      # both are one exact rational rounded once
            want = pm.direct(x, y, off, pm.CORR, w)                                # (two roundings in the second statement)
            assert np.array_equal(np.isnan(m["corr"]), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.all(np.abs(m["corr"][ok] - want[ok]) <= 4 * 2.0 ** -53), w


def test_pandas_golden():
    with open(os.path.join(HERE, "golden", "pairwin_pandas.json")) as f:
        gold = json.load(f)
    held = 0
    for c in gold["cases"]:
        x, y = np.array(c["x"], np.int64), np.array(c["y"], np.int64)
        ex = pm.PairExact(x, y, np.concatenate([[0], np.cumsum(c["sizes"])]))
        m = ex.moments(c["w"])
        for key, mine in (("cov", m["C"]), ("corr", m["corr"]), ("beta", m["beta"])):
            for i, v in enumerate(c[key]):
                if v is not None:
                    assert abs(v - mine[i]) <= 1e-9 * (1 + abs(v)), (c["name"], c["w"], key, i, v, mine[i])
                    held += 1
    assert held > 5000


ALL = pc.flat_cases() + [c for _, c in pc.linear_cases()] + pc.grouped_cases()


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_ill_conditioned_cap(case):
    """at most 1 % of a case's positions are ill-conditioned, for every op and window it is run with: a condition on the inputs"""
    n = len(case.x)
    ex = pm.PairExact(case.x, case.y, pc.offsets_of(case))
    for w in [None] + list(case.windows):
        for fam in (pm.CORR, pm.BETA):
            if not case.long_ok and pc.route_of(w, n) == pc.ROUTE_PREFIX:
                continue
            ill = int(ex.tolerances(fam, w)[2].sum())
            assert 100 * ill <= n, (case.name, fam, w, ill, n)


# ---- the kernels' arithmetic in numpy, with mistakes to plant ---------------------------------------------------------------------------
def diff(col, i, k):
    """x[i] - x[k] as the kernels take it: exact for integers, in double otherwise"""
    if col.dtype.kind in "iu":
        return float(int(col[i]) - int(col[k]))
    return float(col[i]) - float(col[k])


def finish(fam, cxy, cxx, cyy, L, bug):
    div = L - 1 if bug == "sample divisor" and L > 1 else L
    if fam == pm.COV:
        return cxy / div
    if fam == pm.CORR:
        if not (cxx > 0 and cyy > 0):
            return 0.0 if bug == "no NaN at zero variance" else np.nan
        return min(1.0, max(-1.0, cxy / (np.sqrt(cxx) * np.sqrt(cyy))))
    if not cxx > 0:
        return 0.0 if bug == "no NaN at zero variance" else np.nan
    return cxy / cxx


def restated(x, y, off, fam, w, bug=None, tile=pc.TS):
    """what pair_window.hip computes, route by route (w=None: running); `bug` plants one mistake"""
    n = len(x)
    start = np.repeat(off[:-1], np.diff(off))
    out = np.empty(n)
    short = w is not None and min(w, n) <= pc.LDS_W
    if short:
        for i in range(n):
            lo = max(i - w + 1, 0 if bug == "no clamp at the group start" else start[i])
            if bug == "halo one row short" and i - lo + 1 == w and w > 1 and (i % tile) < w - 1:
                lo += 1                                              # the oldest row of a window that reaches into the halo is missing
            rows = range(lo, i + 1)
            L = len(rows)
            dx, dy = np.array([diff(x, e, lo) for e in rows]), np.array([diff(y, e, lo) for e in rows])
            a, b = dx - dx.sum() / L, dy - dy.sum() / L
            out[i] = finish(fam, (a * b).sum(), (a * a).sum(), (b * b).sum(), L, bug)
        return out
    # prefix route: anchored sums per group, combined tile by tile
    P = np.zeros((n + 1, 5))
    for g in range(len(off) - 1):
        a0, b0 = int(off[g]), int(off[g + 1])
        run = np.zeros(5)
        for t0 in range(a0 - a0 % tile, b0, tile):
            lo, hi = max(t0, a0), min(t0 + tile, b0)
            if bug == "raw sums":
                dx, dy = x[lo:hi].astype(np.float64), y[lo:hi].astype(np.float64)
                shift_x = shift_y = 0.0
            else:
                dx, dy = np.array([diff(x, e, lo) for e in range(lo, hi)]), np.array([diff(y, e, lo) for e in range(lo, hi)])
                shift_x, shift_y = (0.0, 0.0) if bug == "no anchor shift in the combine" else (diff(x, lo, a0), diff(y, lo, a0))
            dx, dy = dx + shift_x, dy + shift_y                      # (the combine's shift, applied to the rows: the same sums)
            part = np.cumsum(np.stack([dx, dy, dx * dy, dx * dx, dy * dy], axis=1), axis=0)
            P[lo + 1:hi + 1] = run + part
            run = P[hi].copy()
    for i in range(n):
        d = i if bug == "no clamp at the group start" else i - start[i]
        L = d + 1 if w is None else min(d + 1, w)
        lo = i + 1 - L                                              # the window's first row
        if bug == "halo one row short" and w is not None and L == w:
            lo, L = lo + 1, L - 1
        s = P[i + 1] - (P[lo] if lo != start[i] else 0)             # (the prefix restarts with every group)
        cxy, cxx, cyy = s[2] - s[0] * s[1] / L, s[3] - s[0] * s[0] / L, s[4] - s[1] * s[1] / L
        out[i] = finish(fam, cxy, cxx, cyy, L, bug)
    return out


def planted_cases():
    rng = np.random.default_rng(7)
    sizes = [40, 1, 700, 3, pc.TS + 60, 25]
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    out = []
    for tx, ty, fam in ((np.int64, np.int64, "offset"), (np.float64, np.int32, "centred")):
        x, y = pc.pair_columns(rng, fam, tx, ty, n)
        out.append((x, y, off))
    x = np.full(n, 7, np.int16)
    out.append((x, x.copy(), off))                                   # constant: the exact-NaN rule
    return out


def refused(x, y, off, bug):
    ex = pm.PairExact(x, y, off)
    for w in (None, 3, 9, 64, 100):
        for fam in FAMS:
            try:
                ex.check(restated(x, y, off, fam, w, bug), fam, w)
            except AssertionError:
                return True
    return False


BUGS = ["sample divisor", "no clamp at the group start", "halo one row short", "raw sums", "no anchor shift in the combine", "no NaN at zero variance"]
PLANTED = planted_cases()


def test_the_restatement_passes():
    for x, y, off in PLANTED:
        assert not refused(x, y, off, None)


@pytest.mark.parametrize("bug", BUGS)
def test_planted_mistakes_are_refused(bug):
    assert any(refused(x, y, off, bug) for x, y, off in PLANTED), bug
