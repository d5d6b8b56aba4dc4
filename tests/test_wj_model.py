"""The model of the window join (tests/wj_model.py) held to itself and to pandas, on the CPU: its two statements agree on every named
case of tests/wj_cases.py and on 200 random seeds; it meets the recorded answers of pandas merge + filter + groupby
(tests/golden/wj_pandas.json, tools/gen_wj_golden.py); and every planted mistake is refused by a named case."""
import json
import os

import numpy as np
import pytest

import checker as ck
import wj_cases
import wj_model as wm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wj_pandas.json")


def same_windows(c, flags, mutant=None):
    want = wm.window_rows(c.bk, c.bo, c.pk, c.po, c.before, c.after, flags)
    order, lo, hi = wm.window_bounds(c.bk, c.bo, c.pk, c.po, c.before, c.after, flags, mutant=mutant)
    if sorted(order.tolist()) != list(range(len(c.bo))):
        return False
    return all(np.array_equal(a, b) for a, b in zip(wm.rows_of(order, lo, hi), want))


@pytest.mark.parametrize("name", sorted(wj_cases.cases()))
def test_two_statements_agree_on_every_case(name):
    c = wj_cases.cases()[name]
    heavy = len(c.po) > 20000 or len(c.bo) > 100000
    for flags in (c.flags[-1:] if heavy else c.flags):
        assert same_windows(c, flags), (name, flags)


@pytest.mark.parametrize("block", range(10))
def test_two_statements_agree_on_random_sides(block):
    for seed in range(20 * block, 20 * block + 20):
        c, flags = wj_cases.random_case(seed, 300)
        assert same_windows(c, flags), (seed, flags)


def aggregates_agree(x, lo, hi):
    ne, a = wm.interval_windows(x, lo, hi)
    ne2, b = wm.loop_windows(x, lo, hi)
    assert np.array_equal(ne, ne2) and a.S == b.S and a.A == b.A and a.emin == b.emin and np.array_equal(a.len, b.len)
    for f in ("nnan", "npinf", "nninf"):
        assert np.array_equal(getattr(a, f), getattr(b, f))
    ok = a.nnan == 0
    assert np.array_equal(a.mn[ok], b.mn[ok]) and np.array_equal(a.mx[ok], b.mx[ok])
    return ne, a


@pytest.mark.parametrize("name", ["edges_level2_f64", "edges_level1_i8", "one_row", "values_nonfinite", "inplace_u64_carry"])
def test_interval_aggregates_two_ways_and_through_the_tree(name):
    f = wj_cases.folds()[name]
    sel = np.arange(len(f.lo))[:: max(1, len(f.lo) // 150)]                     # (the loop form is quadratic in the interval length)
    lo, hi = f.lo[sel], f.hi[sel]
    ne, w = aggregates_agree(f.x, lo, hi)
    if f.x.dtype.kind != "f":
        scale = 1
        tree = wm.tree_fold(f.x, lo, hi, wm.SUM)
        assert [t for t, k in zip(tree, ne) if k] == [s * scale for s in w.S] and all(t == 0 for t, k in zip(tree, ne) if not k)
    for op, ref in ((wm.MIN, w.mn), (wm.MAX, w.mx)):
        tree = wm.tree_fold(f.x, lo, hi, op, fill=-7)
        got = np.array([t for t, k in zip(tree, ne) if k], f.x.dtype)
        ok = w.nnan == 0
        assert np.array_equal(got[ok], ref[ok]) and all(t == -7 for t, k in zip(tree, ne) if not k)
    assert wm.tree_fold(f.x, lo, hi, wm.COUNT) == [int(v) for v in np.where(ne, wm.clamp(lo, hi, len(f.x))[1] - wm.clamp(lo, hi, len(f.x))[0], 0)]


def test_model_meets_pandas():
    g = json.load(open(GOLDEN))
    assert len(g["sides"]) >= 12
    for s in g["sides"]:
        dt = np.dtype(s["dtype"])
        bo, po = np.array(s["build_on"], dt), np.array(s["probe_on"], dt)
        bk = [(ck.INT64, np.array(s["build_by"], np.int64))] if s["by"] else []
        pk = [(ck.INT64, np.array(s["probe_by"], np.int64))] if s["by"] else []
        xi, xf = np.array(s["xi"], np.int64), np.array(s["xf"], np.float64)
        for key, rec in s["answers"].items():
            flags = int(key)
            rows = wm.window_rows(bk, bo, pk, po, s["before"], s["after"], flags)
            order, lo, hi = wm.window_bounds(bk, bo, pk, po, s["before"], s["after"], flags)
            assert all(np.array_equal(a, b) for a, b in zip(wm.rows_of(order, lo, hi), rows))
            assert [len(r) for r in rows] == rec["count"]
            ne, wi = wm.interval_windows(xi[order], lo, hi)
            _, wf = wm.interval_windows(xf[order], lo, hi)
            at = np.flatnonzero(ne)
            assert [rec["isum"][i] for i in at] == wi.S and all(rec["isum"][i] is None for i in np.flatnonzero(~ne))
            fsum = [float(v) * 2.0 ** wf.emin for v in wf.S]                     # exact: small multiples of 1/8
            assert [rec["fsum"][i] for i in at] == fsum
            assert [rec["fmin"][i] for i in at] == wf.mn.tolist() and [rec["fmax"][i] for i in at] == wf.mx.tolist()
            assert [rec["fmean"][i] for i in at] == [a / float(n) for a, n in zip(fsum, wf.len)]


# ---- every planted mistake is refused by a named case ------------------------------------------------------------------------------------
REFUSED_BY = {"lo_minus_1": ("group_sizes", 0), "hi_plus_1": ("group_sizes", 0), "segment_end_plus_1": ("straddle", 0),
              "open_closed_swapped": ("d_eq_span_i32", wm.OPEN_LO), "span_wraps": ("ends_int64", 0), "nan_tail_included": ("inf_before_nan_tail", 0),
              "prevailing_from_neighbour": ("prevailing", wm.PREVAILING)}


@pytest.mark.parametrize("mutant", wm.BOUND_MUTANTS)
def test_planted_mistakes_in_the_bounds_are_refused(mutant):
    name, flags = REFUSED_BY[mutant]
    c = wj_cases.cases()[name]
    assert same_windows(c, flags)
    assert not same_windows(c, flags, mutant=mutant), mutant


def test_open_closed_swapped_is_refused_on_either_side_and_in_floating_stamps():
    for name in ("d_eq_span_i32", "d_eq_span_f64", "d_eq_span_f32", "d_eq_span_u16"):
        for flags in (wm.OPEN_LO, wm.OPEN_HI):
            assert not same_windows(wj_cases.cases()[name], flags, mutant="open_closed_swapped"), (name, flags)


@pytest.mark.parametrize("mutant", wm.TREE_MUTANTS)
def test_planted_mistakes_in_the_tree_are_refused(mutant):
    f = wj_cases.folds()["edges_level2_f64"]
    x = np.arange(len(f.x), dtype=np.int64) * 3 + 1                              # (integer values: the comparison is exact)
    ne, w = wm.interval_windows(x, f.lo, f.hi)
    good, bad = wm.tree_fold(x, f.lo, f.hi, wm.SUM), wm.tree_fold(x, f.lo, f.hi, wm.SUM, mutant=mutant)
    assert [t for t, k in zip(good, ne) if k] == w.S
    if mutant == "empty_as_identity":
        good, bad = wm.tree_fold(x, f.lo, f.hi, wm.MAX, fill=-1), wm.tree_fold(x, f.lo, f.hi, wm.MAX, fill=-1, mutant=mutant)
        assert (~ne).any() and all(t == -1 for t, k in zip(good, ne) if not k)
    assert good != bad, mutant
