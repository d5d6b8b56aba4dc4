"""aqg_rangew* (range_window.hip): time-range windows of a column and of every group of a build, through the C-ABI, held to the exact
model of tests/timewin_model.py on the cases of tests/timewin_cases.py.  Bounds, counts, integer sums / averages and min / max are
exact; floating sums and averages meet the derived bound m u / (1 - m u) sum|x| of include/aqg.h on finite windows and come out in
the specified non-finite class elsewhere.  The worst observed share of that bound is printed."""
import json
import os

import numpy as np
import pytest

import timewin_cases as tc
import timewin_model as tm
from aquery2_amd.capi import (DATE, TIME, INT32, STR, TIMESTAMP, RANGEW_AVG, RANGEW_CLOSED, RANGEW_COUNT, RANGEW_MAX, RANGEW_MIN,
                              RANGEW_OPEN, RANGEW_SUM)

pytestmark = pytest.mark.gpu
ERR_DTYPE, ERR_ARG = 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
assert (RANGEW_COUNT, RANGEW_SUM, RANGEW_AVG, RANGEW_MIN, RANGEW_MAX, RANGEW_OPEN, RANGEW_CLOSED) == (tm.COUNT, tm.SUM, tm.AVG, tm.MIN, tm.MAX, tm.OPEN, tm.CLOSED)
OPS = (RANGEW_COUNT, RANGEW_SUM, RANGEW_AVG, RANGEW_MIN, RANGEW_MAX)
WORST = {"share": 0.0}


@pytest.fixture(scope="module")
def dev():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    print("worst |got - exact| / bound of a floating sum or average in this module: %.3g" % WORST["share"])
    d.close()


def stamps_dev(dev, c):
    return dev.key_col(DATE if c.kind == "date" else TIME, c.t) if c.kind else dev.to_device(c.t)


def hold(c, w, op, got, what):
    """one aggregate of every window against the model"""
    isf = np.asarray(c.x).dtype.kind == "f"
    if op == RANGEW_COUNT:
        assert got.dtype == np.uint32 and np.array_equal(got, w.len), what
    elif op == RANGEW_SUM and not isf:
        ex = tm.exact_int_sum(w)
        assert np.array_equal(got["lo"], ex["lo"]) and np.array_equal(got["hi"].view(np.uint64), ex["hi"]), what
    elif op == RANGEW_AVG and not isf:
        assert got.dtype == np.float64 and np.array_equal(got, tm.exact_int_avg(w)), what
    elif op in (RANGEW_SUM, RANGEW_AVG):
        assert got.dtype == np.float64, what
        share = tm.sum_share(w, got, avg=op == RANGEW_AVG)
        WORST["share"] = max(WORST["share"], share)
        print("%s: worst |got - exact| / bound = %.3g" % (what, share))
        assert share <= 1.0, what
    else:
        ref = w.mn if op == RANGEW_MIN else w.mx
        ok = w.nnan == 0
        assert got.dtype == ref.dtype and np.array_equal(got[ok], ref[ok]), what          # (== : either zero passes)


def run_flat(dev, c):
    lo, w = tc.reference(c)
    td, xd = stamps_dev(dev, c), dev.to_device(c.x)
    lod = dev.rangew_bounds(td, c.span, c.frame, keep=True)
    assert np.array_equal(lod.to_host(), lo), c.name
    for op in OPS:
        x = None if op == RANGEW_COUNT else xd
        got = dev.rangew_fold(op, x, lod)
        hold(c, w, op, got, "%s/op%d" % (c.name, op))
        one = dev.rangew(op, td, c.span, x, c.frame)
        assert one.tobytes() == got.tobytes(), (c.name, op, "aqg_rangew is not bounds followed by fold")
        assert dev.rangew(op, td, c.span, x, c.frame).tobytes() == one.tobytes(), (c.name, op, "two calls differ")


FLAT = tc.flat_cases()
NCHUNK = 6


def test_geometry_is_what_the_cases_assume(dev):
    rx, tile = tc.geometry()
    for n in (1, rx, rx + 1, rx * rx, rx * rx + 1, rx ** 3 + 1):
        dev.rangew_fold(RANGEW_MAX, np.zeros(n, np.int8), np.zeros(n, np.uint32))
        nl, blocks, _, _ = dev.rangew_last()
        assert (nl, blocks) == tc.levels(n), n
    assert tile % (rx * rx) == 0 or (rx * rx) % tile == 0          # tiles and the blocks of level 1 nest: a staged tile pair holds whole blocks


@pytest.mark.parametrize("chunk", range(NCHUNK))
def test_flat_cases(dev, chunk):
    """every named case of the column form: bounds exact, every aggregate, aqg_rangew == bounds + fold, two calls bit-identical"""
    for c in FLAT[chunk::NCHUNK]:
        run_flat(dev, c)


def test_big_column(dev):
    """four levels; windows that hold two whole elements of the top level between their ends"""
    c = tc.big_case()
    lo, w = tc.reference(c)
    td, xd = dev.to_device(c.t), dev.to_device(c.x)
    lod = dev.rangew_bounds(td, c.span, c.frame, keep=True)
    assert np.array_equal(lod.to_host(), lo)
    assert dev.rangew_last()[2:] == (c.n - 1, 0)
    for op in (RANGEW_SUM, RANGEW_MIN, RANGEW_MAX, RANGEW_AVG):
        hold(c, w, op, dev.rangew_fold(op, xd, lod), "big/op%d" % op)
    assert dev.rangew_last()[:2] == tc.levels(c.n)
    xf = c.x.astype(np.float64) * 2.0 ** -7
    hold(tc.Case("big-float", c.t, xf, c.span, c.frame), tm.search_windows(xf, lo), RANGEW_SUM, dev.rangew_fold(RANGEW_SUM, xf, lod), "big/float-sum")


@pytest.mark.parametrize("c", tc.grouped_cases(), ids=lambda c: c.name)
def test_grouped(dev, c):
    """the flat grouped bounds, and the three grouped forms (row layout, flat layout, grouped bounds + fold) against the model; for a
    few groups also against the column form run on each group alone"""
    lo, w = tc.reference(c)
    keys, t_row, x_row = c.rows()
    gb = dev.groupby_build([keys])
    assert gb.ngroups == len(c.starts) and np.array_equal(dev.group_offsets(gb)[:len(c.starts)], c.starts)
    td, xd = dev.to_device(c.t), dev.to_device(c.x)
    lod = dev.rangew_bounds(td, c.span, c.frame, gb=gb, keep=True)
    assert np.array_equal(lod.to_host(), lo), c.name
    edges = [int(s) for s in c.starts] + [c.n]
    for op in OPS:
        forms = {"row": dev.grouped_rangew(gb, op, t_row, c.span, None if op == RANGEW_COUNT else x_row, c.frame),
                 "flat": dev.grouped_rangew(gb, op, td, c.span, None if op == RANGEW_COUNT else xd, c.frame, flat=True),
                 "bounds+fold": dev.rangew_fold(op, None if op == RANGEW_COUNT else xd, lod)}
        for k, got in forms.items():
            hold(c, w, op, got, "%s/%s/op%d" % (c.name, k, op))
        if len(c.starts) <= 8 and op != RANGEW_COUNT:
            for a, b in zip(edges[:-1], edges[1:]):
                alone = dev.rangew(op, c.t[a:b], c.span, c.x[a:b], c.frame)
                sub = tm.search_windows(c.x[a:b], lo[a:b] - a)
                hold(tc.Case("alone", c.t[a:b], c.x[a:b], c.span, c.frame), sub, op, alone, "%s/alone%d/op%d" % (c.name, a, op))
                if np.asarray(c.x).dtype.kind != "f":
                    assert alone.tobytes() == forms["flat"][a:b].tobytes()
    gb.destroy()


def test_fold_with_hand_made_bounds(dev):
    """the fold knows nothing of stamps: any lo <= i is a window, and lo[i] > i is clamped to i"""
    rx, tile = tc.geometry()
    n = 2 * tile + rx + 3
    r = np.random.default_rng(5)
    lo = (np.arange(n) * r.random(n)).astype(np.uint32)                     # not monotone
    lo[::7] = np.arange(n, dtype=np.uint32)[::7] + 5                        # beyond i: clamped
    lo[3] = 2 ** 32 - 1
    clamped = np.minimum(lo.astype(np.int64), np.arange(n))
    for x in (r.integers(-2 ** 62, 2 ** 62, size=n), r.standard_normal(n), r.integers(0, 255, size=n).astype(np.uint8)):
        w = tm.search_windows(x, clamped)
        c = tc.Case("hand", np.zeros(n, np.int64), x, 1, 0)
        for op in OPS:
            hold(c, w, op, dev.rangew_fold(op, None if op == RANGEW_COUNT else x, lo), "hand-made/%s/op%d" % (x.dtype.name, op))


def test_inf_span_is_the_running_scan(dev):
    """span = +Inf: the running sums / mins / maxs of aqg_scan"""
    rx, tile = tc.geometry()
    n = 2 * tile + 77
    r = np.random.default_rng(6)
    t = tc.asc(n, 6)
    # (positive doubles: the reference's maxs starts from the smallest positive normal, which a running max of these never meets)
    for x in (r.integers(-2 ** 40, 2 ** 40, size=n), r.integers(1, 100, size=n).astype(np.float64)):
        for op, sop in ((RANGEW_SUM, 0), (RANGEW_MIN, 2), (RANGEW_MAX, 3)):                # AQG_SCAN_SUMS / MINS / MAXS
            got = dev.rangew(op, t, float("inf"), x, RANGEW_OPEN)
            ref = dev.scan(sop, x)
            assert got.tobytes() == ref.tobytes(), (x.dtype.name, sop)         # (integer-valued doubles: every order of summation is exact)


def test_errors_write_nothing(dev):
    n = 100
    t, x = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.float64)
    td, xd = dev.to_device(t), dev.to_device(x)
    canary = np.full(4 * n, 0xA5, np.uint8)
    keys = np.arange(n, dtype=np.int32) % 3
    gb = dev.groupby_build([keys])
    agg = dev.groupby_agg([keys], [0], [x])                                 # not a handle of aqg_groupby_build
    L = dev.lib

    def refused(code, fn, *args):
        out = dev.to_device(canary.view(np.float64))
        rc = fn(*[out.ptr if a is OUT else a for a in args])
        assert rc == code, (rc, code, fn.__name__ if hasattr(fn, "__name__") else fn, args)
        dev.sync()
        assert np.array_equal(out.to_host().view(np.uint8), canary)
    OUT = object()
    inf, nan = float("inf"), float("nan")
    for span, frame in ((nan, 0), (nan, 1), (-1.0, 1), (0.0, 0), (-inf, 1), (1.0, 2), (1.0, -1)):
        refused(ERR_ARG, L.aqg_rangew_bounds, dev.ctx, td.tag, td.ptr, n, span, frame, OUT)
        refused(ERR_ARG, L.aqg_rangew, dev.ctx, RANGEW_SUM, td.tag, td.ptr, span, frame, xd.tag, xd.ptr, n, OUT)
        refused(ERR_ARG, L.aqg_grouped_rangew, dev.ctx, gb.h, RANGEW_SUM, td.tag, td.ptr, span, frame, xd.tag, xd.ptr, OUT)
        refused(ERR_ARG, L.aqg_grouped_rangew_flat, dev.ctx, gb.h, RANGEW_SUM, td.tag, td.ptr, span, frame, xd.tag, xd.ptr, OUT)
        refused(ERR_ARG, L.aqg_grouped_rangew_bounds_flat, dev.ctx, gb.h, td.tag, td.ptr, span, frame, OUT)
    for op in (-1, 5):
        refused(ERR_ARG, L.aqg_rangew, dev.ctx, op, td.tag, td.ptr, 1.0, 0, xd.tag, xd.ptr, n, OUT)
        refused(ERR_ARG, L.aqg_rangew_fold, dev.ctx, op, xd.tag, xd.ptr, n, td.ptr, OUT)
    for tag in (STR, TIMESTAMP, 6):
        refused(ERR_DTYPE, L.aqg_rangew_bounds, dev.ctx, tag, td.ptr, n, 1.0, 0, OUT)
        refused(ERR_DTYPE, L.aqg_rangew, dev.ctx, RANGEW_SUM, tag, td.ptr, 1.0, 0, xd.tag, xd.ptr, n, OUT)
    for tag in (DATE, TIME, STR):
        refused(ERR_DTYPE, L.aqg_rangew, dev.ctx, RANGEW_SUM, td.tag, td.ptr, 1.0, 0, tag, xd.ptr, n, OUT)
        refused(ERR_DTYPE, L.aqg_rangew_fold, dev.ctx, RANGEW_MAX, tag, xd.ptr, n, td.ptr, OUT)
    refused(ERR_ARG, L.aqg_rangew, dev.ctx, RANGEW_SUM, td.tag, None, 1.0, 0, xd.tag, xd.ptr, n, OUT)
    refused(ERR_ARG, L.aqg_rangew, dev.ctx, RANGEW_SUM, td.tag, td.ptr, 1.0, 0, xd.tag, None, n, OUT)
    refused(ERR_ARG, L.aqg_rangew_fold, dev.ctx, RANGEW_SUM, xd.tag, xd.ptr, n, None, OUT)
    refused(ERR_ARG, L.aqg_rangew_bounds, dev.ctx, td.tag, None, n, 1.0, 0, OUT)
    # out overlapping an input: the input itself is the canary
    for fn, args in ((L.aqg_rangew, lambda o: (dev.ctx, RANGEW_MAX, td.tag, td.ptr, 1.0, 0, xd.tag, o, n, o)),
                     (L.aqg_rangew, lambda o: (dev.ctx, RANGEW_COUNT, INT32, o, 1.0, 0, INT32, None, n, o)),
                     (L.aqg_rangew_bounds, lambda o: (dev.ctx, INT32, o, n, 1.0, 0, o)),
                     (L.aqg_rangew_fold, lambda o: (dev.ctx, RANGEW_COUNT, INT32, None, n, o, o))):
        out = dev.to_device(canary.view(np.float64))
        assert fn(*args(out.ptr)) == ERR_ARG
        dev.sync()
        assert np.array_equal(out.to_host().view(np.uint8), canary)
    refused(ERR_ARG, L.aqg_grouped_rangew, dev.ctx, agg.h, RANGEW_SUM, td.tag, td.ptr, 1.0, 0, xd.tag, xd.ptr, OUT)
    refused(ERR_ARG, L.aqg_grouped_rangew_flat, dev.ctx, agg.h, RANGEW_SUM, td.tag, td.ptr, 1.0, 0, xd.tag, xd.ptr, OUT)
    refused(ERR_ARG, L.aqg_grouped_rangew_bounds_flat, dev.ctx, agg.h, td.tag, td.ptr, 1.0, 0, OUT)
    # empty inputs are fine
    assert L.aqg_rangew(dev.ctx, RANGEW_SUM, td.tag, None, 1.0, 0, xd.tag, None, 0, None) == 0
    assert L.aqg_rangew_bounds(dev.ctx, td.tag, None, 0, 1.0, 0, None) == 0
    assert L.aqg_rangew_fold(dev.ctx, RANGEW_SUM, xd.tag, None, 0, None, None) == 0
    gb.destroy()


def test_step_counters(dev):
    n = 3 * tc.geometry()[1] + 5
    up = np.arange(n, dtype=np.int64) * 2
    up[10] = up[9]                                                          # one tie: neither a rising nor a falling step
    dev.rangew_bounds(up, 5, RANGEW_OPEN)
    assert dev.rangew_last()[2:] == (n - 2, 0)
    dev.rangew_bounds(up[::-1].astype(np.float64), 5, RANGEW_OPEN)
    assert dev.rangew_last()[2:] == (0, n - 2)
    sh = np.random.default_rng(1).permutation(n).astype(np.int32)
    lo = dev.rangew_bounds(sh, 5, RANGEW_OPEN)
    u, d = dev.rangew_last()[2:]
    assert u > 0 and d > 0 and u + d == n - 1 and np.all(lo <= np.arange(n))
    assert dev.rangew(RANGEW_SUM, sh, 5, sh).shape == (n,)
    # steps across a group start do not count
    keys = np.repeat(np.arange(3, dtype=np.int32), 100)
    gb = dev.groupby_build([keys])
    tf = np.concatenate([np.arange(100), np.arange(100), np.arange(100)]).astype(np.int64)
    dev.rangew_bounds(tf, 5, RANGEW_OPEN, gb=gb)
    assert dev.rangew_last()[2:] == (297, 0)
    gb.destroy()


def test_pandas_goldens_through_the_device(dev):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "timewin_pandas.json")))
    for g in gold["cases"]:
        t = np.array(g["t"], np.int64)
        x = np.array([float.fromhex(v) for v in g["x"]])
        frame = RANGEW_CLOSED if g["closed"] == "both" else RANGEW_OPEN
        td, xd = dev.to_device(t), dev.to_device(x)
        assert [int(v) for v in dev.rangew(RANGEW_COUNT, td, g["span"], None, frame)] == g["count"], g["name"]
        for key, op in (("sum", RANGEW_SUM), ("mean", RANGEW_AVG), ("min", RANGEW_MIN), ("max", RANGEW_MAX)):
            assert [float(v).hex() for v in dev.rangew(op, td, g["span"], xd, frame)] == g[key], (g["name"], key)


def test_emitted_group_loop(tmp_path):
    """tests/emitted/time_windows.cpp over host_main's synthetic dataset (2e5 rows): `sumr(40, t[vecs[g]], c[vecs[g]], col[g])`,
    `maxr(...)` and `countr(40, t[vecs[g]], col[g])` in the generated group loop cost ONE bounds search and ONE fold per aggregate, at
    1000 groups and at 10; `subvec(0, 2)` views take the per-group path and give the per-group answer"""
    import subprocess
    from test_gpu_emitted import EM, run
    from test_gpu_quantiles import _synthetic
    import quantile_model as qm
    subprocess.check_call(["make", "-C", EM, "build/time_windows.so", "build/host_main"], stdout=subprocess.DEVNULL)
    a, c = _synthetic()
    run("time_windows.so", "synthetic", "dll_tw_flat", "dll_tw_group", "dll_tw_group10", cwd=str(tmp_path))
    n = len(c)
    t = np.fromfile(tmp_path / "tw.t", np.int32)
    assert len(t) == n and np.all(np.diff(t) >= 1)
    c = np.asarray(c).astype(np.int32)
    i128 = np.dtype([("lo", "<u8"), ("hi", "<u8")])

    def check(t_, c_, starts, files, what):
        fp, st = tm.stamps(t_)
        lo = tm.search_bounds(fp, st, starts, 40, tm.OPEN)
        w = tm.search_windows(c_, lo)
        case = tc.Case(what, t_, c_, 40, tm.OPEN)
        for path, op, dt in zip(files, (RANGEW_SUM, RANGEW_MAX, RANGEW_COUNT), (i128, np.int32, np.uint32)):
            if path is not None:
                hold(case, w, op, np.fromfile(path, dt), what + "/op%d" % op)
    check(t, c, None, [tmp_path / ("twf.out.%d" % k) for k in range(3)], "emitted flat")
    for name, key, G in (("twg", a, 1000), ("twg10", a % 10, 10)):
        gid, ng = qm.first_occurrence_ids(key)
        assert ng == G
        # the group loop's row lists: groups in first-occurrence order, a group's rows in descending row id (the flat layout)
        order = np.lexsort((-np.arange(n), gid))
        starts = np.flatnonzero(np.diff(gid[order], prepend=-1))
        first = np.full(G, n, np.int64)
        np.minimum.at(first, gid, np.arange(n))
        assert np.array_equal(np.fromfile(tmp_path / (name + ".out.0"), np.int32), key[first])
        cf, tf = c[order], t[order]
        check(tf, cf, starts, [tmp_path / (name + ".out.%d" % k) for k in (1, 2, 3)], name)
        # the two-row views, one per group, each the per-group answer of its first two rows
        counts = np.diff(np.append(starts, n))
        take = np.concatenate([np.arange(s0, s0 + min(cnt, 2)) for s0, cnt in zip(starts, counts)])
        sub_starts = np.concatenate([[0], np.cumsum(np.minimum(counts, 2))[:-1]])
        check(tf[take], cf[take], sub_starts, [tmp_path / (name + ".out.4"), None, None], name + " subvec")
        bounds, folds, groups = (int(v) for v in (tmp_path / (name + ".calls")).read_text().split())
        assert groups == G and bounds == 1 and folds == 3, "one search and one fold per aggregate, whatever the number of groups"
