"""The model of the time-range windows (tests/timewin_model.py) on the CPU: its two statements agree on every case of
tests/timewin_cases.py, it meets pandas' recorded answers bit for bit, and the cases refuse eight planted mistakes, each by name."""
import bisect
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import timewin_cases as tc
import timewin_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = tc.flat_cases() + tc.grouped_cases()
BY_NAME = {c.name: c for c in ALL}


def test_case_names_are_unique_and_cover_the_grid():
    assert len(BY_NAME) == len(ALL)
    rx, tile = tc.geometry()
    ns = {c.n for c in tc.flat_cases()}
    for n in (1, 2, 63, 64, 65, rx * rx - 1, rx * rx, rx * rx + 1, tile - 1, tile, tile + 1):
        assert n in ns
    L, blocks = tc.levels(tc.big_case().n)
    assert L == 4 and tc.big_case().n >= 3 * blocks[2]          # two whole top elements fit between the ends of one window


@pytest.mark.parametrize("chunk", range(8))
def test_the_two_statements_agree(chunk):
    for c in ALL[chunk::8]:
        fp, st = tm.stamps(c.t, c.kind)
        lo, w = tc.reference(c)
        assert np.all(lo >= tm.slice_starts(c.n, c.starts)) and np.all(lo <= np.arange(c.n)), c.name
        rows = range(c.n) if c.n <= 700 else sorted(set(np.random.default_rng(c.n).integers(0, c.n, size=120)) | {0, c.n - 1})
        lb = tm.loop_bounds(fp, st, c.starts, c.span, c.frame, rows)
        assert all(lb[i] == lo[i] for i in rows), c.name
        lw, emin = tm.loop_windows(c.x, lo, rows)
        assert emin == w.emin
        for i in rows:
            S, A, nn, npi, nni, mn, mx = lw[i]
            assert (S, A, nn, npi, nni) == (w.S[i], w.A[i], w.nnan[i], w.npinf[i], w.nninf[i]), (c.name, i)
            if not nn:
                assert mn == w.mn[i] and mx == w.mx[i], (c.name, i)


def test_big_case_statements_agree_on_a_sample():
    c = tc.big_case()
    fp, st = tm.stamps(c.t, c.kind)
    lo, w = tc.reference(c)
    rx = tc.geometry()[0]
    rows = [0, 1, 3 * rx ** 3 + 100, c.n - 1]
    lb = tm.loop_bounds(fp, st, None, c.span, c.frame, rows)
    assert all(lb[i] == lo[i] for i in rows)
    lw, _ = tm.loop_windows(c.x, lo, rows)
    for i in rows:
        assert lw[i][0] == w.S[i] and lw[i][5] == w.mn[i] and lw[i][6] == w.mx[i]
    i = rows[2]
    assert i // rx ** 3 - int(lo[i]) // rx ** 3 == 3          # elements 1 and 2 of the top level lie whole inside this window


def test_model_meets_pandas_bit_for_bit():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "timewin_pandas.json")))
    assert len(gold["cases"]) >= 32
    for g in gold["cases"]:
        t = np.array(g["t"], np.int64)
        x = np.array([float.fromhex(v) for v in g["x"]])
        frame = tm.CLOSED if g["closed"] == "both" else tm.OPEN
        fp, st = tm.stamps(t)
        for lo in (tm.search_bounds(fp, st, None, g["span"], frame), np.array([v for _, v in sorted(tm.loop_bounds(fp, st, None, g["span"], frame).items())])):
            w = tm.search_windows(x, lo)
            unit = Fraction(2) ** w.emin
            assert [int(v) for v in w.len] == g["count"], g["name"]
            for key, mine in (("sum", [float(s * unit) for s in w.S]), ("mean", [float(s * unit) / float(n) for s, n in zip(w.S, w.len)]), ("min", w.mn), ("max", w.mx)):
                assert [float(v).hex() for v in mine] == g[key], (g["name"], key)


# ---- planted mistakes: each is a wrong statement of the bounds or of the sum, and a named case tells it from the model ---------------------
def wrong_bounds(c, mistake):
    fp, st = tm.stamps(c.t, c.kind)
    n = c.n
    ss = tm.slice_starts(n, c.starts)
    starts = None if c.starts is None else [int(s) for s in c.starts]
    frame, span = c.frame, c.span
    if mistake == "frames-swapped":
        return tm.search_bounds(fp, st, c.starts, span, 1 - frame) if tm.span_ok(span, 1 - frame) else None
    if mistake == "peers-included":                               # the window's end moves to the last row with i's stamp: its length grows
        lo = tm.search_bounds(fp, st, c.starts, span, frame).copy()
        for i in range(n - 1):
            j = i
            while j + 1 < n and ss[j + 1] == ss[i] and st[j + 1] == st[i]:
                j += 1
            lo[i] -= j - i                                         # (what a length-preserving view of the mistake looks like)
        return lo
    if mistake == "no-group-clamp":
        return tm.search_bounds(fp, st, None, span, frame)
    if mistake == "previous-group-clamp":
        prev = dict(zip(starts, [0] + starts[:-1]))
        lo = np.zeros(n, np.int64)
        for i in range(n):
            j = i
            while j > prev[int(ss[i])] and tm.within(fp, st[i], st[j - 1], span, frame):
                j -= 1
            lo[i] = j
        return lo
    if mistake == "signed-difference":
        dm = None if fp else tm.dmax_of(span, frame)
        lo = np.zeros(n, np.int64)
        for i in range(n):
            j = i
            while j > ss[i] and ((st[i] - st[j - 1] <= span) if fp else (st[i] - st[j - 1] <= dm)):
                j -= 1
            lo[i] = j
        return lo
    if mistake == "wrapped-subtraction":                          # t[i] - dmax in the column's own 64 bits
        dm = tm.dmax_of(span, frame)
        lo = np.zeros(n, np.int64)
        for i in range(n):
            edge = (st[i] - dm + 2 ** 63) % 2 ** 64 - 2 ** 63
            lo[i] = bisect.bisect_left(st, edge, int(ss[i]), i + 1)
        return lo
    if mistake == "floor-for-open":
        dm = min(math.floor(span), tm.U64)
        return np.array([bisect.bisect_left(st, st[i] - dm, int(ss[i]), i + 1) for i in range(n)])
    raise KeyError(mistake)


PLANTED = [
    ("frames-swapped", "exact-s5-f0"),
    ("frames-swapped", "exact-fp-f1"),
    ("peers-included", "tie-runs"),
    ("no-group-clamp", "g-one-row-between"),
    ("previous-group-clamp", "g-one-row-between"),
    ("signed-difference", "descending"),
    ("wrapped-subtraction", "int64-ends-s9.22337e+18"),
    ("floor-for-open", "exact-unit-open3"),
]


@pytest.mark.parametrize("mistake,name", PLANTED)
def test_planted_bounds_mistake_is_refused(mistake, name):
    c = BY_NAME[name]
    lo, _ = tc.reference(c)
    bad = wrong_bounds(c, mistake)
    assert bad is not None and not np.array_equal(np.asarray(bad, np.int64), lo), (mistake, name)


def test_planted_prefix_difference_is_refused():
    """a sum taken as a difference of running sums lets the NaN (and the Inf) rows in front of a window through; the case's windows
    behind them are finite in the model, and sum_share refuses the NaN"""
    c = BY_NAME["nonfinite"]
    lo, w = tc.reference(c)
    run = np.concatenate([[0.0], np.cumsum(c.x)])
    with np.errstate(invalid="ignore"):
        bad = run[np.arange(c.n) + 1] - run[lo]
    finite_windows = [i for i in range(c.n) if tm.expected_class(w, i) is None]
    assert len(finite_windows) > c.n - 40 and np.isnan(bad[finite_windows]).any()
    with pytest.raises(AssertionError):
        tm.sum_share(w, bad)
    good = np.array([math.fsum(c.x[int(lo[i]):i + 1]) if tm.expected_class(w, i) is None else float(np.sum(c.x[int(lo[i]):i + 1])) for i in range(c.n)])
    assert tm.sum_share(w, good) <= 1.0


def test_large_value_leaving_the_window_is_told_apart():
    """add-and-remove keeps the rounding of a 1e30 that has left the window: beyond the bound of the ones' own windows"""
    c = BY_NAME["g-1e30-beside-ones"]
    lo, w = tc.reference(c)
    s = int(c.starts[1])
    assert np.all(lo[s:int(c.starts[2])] >= s) and all(w.A[i] == (i - int(lo[i]) + 1) * 2 ** -w.emin for i in range(s, s + 100))
    bad = np.array([float(x * Fraction(2) ** w.emin) for x in w.S], np.float64)
    bad[s + 5] = (1e30 + 6.0) - 1e30
    with pytest.raises(AssertionError):
        tm.sum_share(w, bad)


def test_span_rules():
    assert tm.dmax_of(2.5, tm.CLOSED) == 2 and tm.dmax_of(2.5, tm.OPEN) == 2 and tm.dmax_of(3, tm.OPEN) == 2 and tm.dmax_of(3, tm.CLOSED) == 3
    assert tm.dmax_of(0.5, tm.OPEN) == 0 and tm.dmax_of(1e30, tm.OPEN) == tm.U64 and tm.dmax_of(float("inf"), tm.CLOSED) == tm.U64
    assert tm.dmax_of(2.0 ** 64, tm.OPEN) == tm.U64 and tm.dmax_of(2.0 ** 64, tm.CLOSED) == tm.U64
    assert tm.span_ok(0, tm.CLOSED) and not tm.span_ok(0, tm.OPEN) and not tm.span_ok(float("nan"), tm.CLOSED) and not tm.span_ok(-1, tm.CLOSED)
    assert tm.days_from_civil(2024, 3, 1) - tm.days_from_civil(2024, 2, 28) == 2 and tm.days_from_civil(2025, 3, 1) - tm.days_from_civil(2025, 2, 28) == 1
