"""The per-group model (tests/groupagg_model.py) against the oracle's grouped reduction, on the value sets the GPU tests use
(tests/groupagg_cases.py) at one small shape: the oracle can then be trusted at the shapes tests/test_gpu_groupagg_extremes.py needs.  No GPU.

Integers: sum, min, max, count, avg, var, stddev bit for bit.  Floating columns: min and max bit for bit in EVERY group (the model folds
a group's rows in the order the reference visits them, NaN rows included); sum and avg within (n_g - 1) 2^-53 sum|x| of the exact sum
of the finite rows (the same infinity / NaN where a row is infinite or NaN); var against the formula over exactly summed squares --
the squares rounded in the column's type, as the reference multiplies them -- within the bound the GPU tests use."""
import math

import numpy as np
import pytest

import checker as ck
import extremes as ex
import groupagg_cases as gc
import groupagg_model as gm

N, G = 20_011, 500


def layouts():
    return {None: gc.Layout(N, G, 1), gc.I64: gc.carry_layout(N, G, 2, gc.I64), gc.U64: gc.carry_layout(N, G, 3, gc.U64)}


def group_rows(o):
    """the rows of every group in the order the reference's loop visits them (ht_postproc: descending row id)"""
    return [o["row_ids"][o["offsets"][g]: o["offsets"][g] + o["counts"][g]] for g in range(o["ngroups"])]


def test_the_layout_has_the_three_kinds_of_groups():
    for lay in layouts().values():
        c = np.bincount(lay.labels)
        assert c[0] == N // 3 and np.all(c[1:1 + gc.ONES] == 1) and len(np.unique(lay.labels)) > 300
    assert layouts()[gc.I64].probe_es == (53, 64) and layouts()[gc.U64].probe_es == (53, 64)      # (e = 77 needs 16 386 rows a group)


@pytest.mark.parametrize("dt", ex.INT_DTYPES, ids=ex.nm)
def test_integer_groups(oracle, dt):
    lays = layouts()
    done = 0
    for which, lay in lays.items():
        if which is not None and which != dt:
            continue
        o = oracle.groupby([lay.labels])
        rows = group_rows(o)
        for cname, x, ops in gc.columns(lay, [dt], seed=5, sets=("int_full", "carry", "narrow_at_end")):
            if (which is None) == (cname.startswith("carry") and dt.itemsize == 8 and bool(lays[dt].probe_es)):
                continue                                     # the carry columns of 8-byte types: on the layout that holds their probes
            want = {name: oracle.grouped_reduce(ck.RED_NAMES[name], x, o) for name in ("sum", "min", "max", "count", "avg", "var", "stddev")}
            sums = ck.i128_to_int(want["sum"])
            xl = x.tolist()
            for g, r in enumerate(rows):
                m = gm.int_group([xl[i] for i in r.tolist()], dt)
                assert sums[g] == m["sum"], (cname, g)
                assert int(want["min"][g]) == m["min"] and int(want["max"][g]) == m["max"] and int(want["count"][g]) == m["count"], (cname, g)
                for name in ("avg", "var", "stddev"):
                    assert ex.same(np.float64(want[name][g]), np.float64(m[name])), (cname, name, g, want[name][g], m[name])
            done += 1
            if cname.startswith("carry") and lay.probe_es:   # the probes: float(S - 1), float(S), float(S + 1) over their row counts
                k = 0
                for e in lay.probe_es:
                    _, probe_sums = ex.avg_probe_column(dt, e)
                    for j in range(3):
                        g = int(o["reversemap"][lay.sized_rows[k][0]])
                        assert sums[g] == probe_sums[j] and want["avg"][g] == float(probe_sums[j]) / len(lay.sized_rows[k]), (e, j)
                        k += 1
    assert done >= (3 if dt in (gc.I32, gc.U32) else 2 if dt.itemsize == 8 else 1)


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_floating_groups(oracle, dt):
    lay = layouts()[None]
    o = oracle.groupby([lay.labels])
    rows = group_rows(o)
    seen = set()
    for cname, x, ops in gc.columns(lay, [dt], seed=5, sets=("fp_finite", "fp_inf", "fp_nan")):
        want = {gc.RED_NAME[op]: oracle.grouped_reduce(op, x, o) for op in ops}
        xl = x.tolist()
        st = gc.group_stats(x, o)
        nan_groups = 0
        for g, r in enumerate(rows):
            vals = [xl[i] for i in r.tolist()]
            m = gm.fp_group(vals, dt)
            n = len(vals)
            nan_groups += m["nan"]
            assert bool(st["nan"][g]) == m["nan"] and st["n"][g] == n
            assert abs(st["sum_abs"][g] - m["sum_abs"]) <= 1e-12 * m["sum_abs"]
            if "min" in want:
                assert ex.same(want["min"][g], dt.type(m["min"])) and ex.same(want["max"][g], dt.type(m["max"])), (cname, g)
                assert int(want["count"][g]) == n
                for name, div in (("sum", 1.0), ("avg", float(n))):
                    got = float(want[name][g])
                    if m["nan"] or (m["pinf"] and m["ninf"]):
                        assert math.isnan(got), (cname, name, g)
                    elif m["pinf"] or m["ninf"]:
                        assert got == (math.inf if m["pinf"] else -math.inf), (cname, name, g)
                    else:
                        bound = (n - 1) * 2.0 ** -53 * m["sum_abs"] / div
                        assert abs(got - m["exact_sum"] / div) <= bound + np.spacing(abs(got)), (cname, name, g, got, m["exact_sum"], bound)
                        seen.add("finite")
                if m["pinf"] and not m["nan"]:
                    seen.add("+inf")
                if n > 1 and not m["nan"] and all(v == math.inf for v in vals):
                    assert want["min"][g] == np.finfo(dt).max          # the seed of min
                    seen.add("all +inf")
                if n > 1 and all(v < 0 for v in vals):
                    assert want["max"][g] == np.finfo(dt).tiny         # the seed of max
                    seen.add("all negative")
            else:
                got = float(want["var"][g])
                if m["nan"] or m["pinf"] or m["ninf"]:
                    assert math.isnan(got), (cname, "var", g)          # inf - inf * inf / (n + 1)
                    continue
                sq = [float(dt.type(v) * dt.type(v)) for v in vals]    # the squares in the column's type
                ssq, s = math.fsum(sq), math.fsum(vals)
                ref = (ssq - s * s / (n + 1)) / (n + 1)
                bound = 4 * n * 2.0 ** -52 * ssq / (n + 1)
                assert abs(got - ref) <= bound, (cname, "var", g, got, ref, bound)
                sd = float(want["stddev"][g])
                assert ex.same(np.float64(sd), np.float64(math.sqrt(got) if got >= 0 else math.nan)), (cname, "stddev", g)
        assert nan_groups <= 0.1 * o["ngroups"] and ("fp_nan" in cname) == (nan_groups > 0), (cname, nan_groups)
    assert seen == {"finite", "+inf", "all +inf", "all negative"}


def test_fold_seeds():
    assert gm.seeds(np.float32) == (float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny))
    assert gm.fold_min([math.inf, math.inf], np.float64) == np.finfo(np.float64).max
    assert gm.fold_max([-1.0, -math.inf], np.float32) == float(np.finfo(np.float32).tiny)
    assert gm.fold_max([-5, -7], np.int16) == -5 and gm.fold_min([], np.uint8) == 255
    # 65535 * 65535 wraps to -131071 in int; the unsigned 128-bit sum of squares takes that value sign-extended: about 2^128
    assert gm.int_var([65535], np.uint16) == (float(2 ** 128 - 131071) - float(65535 * 65535) / 2.0) / 2.0
    assert gm.int_var([-32768, 32767], np.int16) == (float(32768 ** 2 + 32767 ** 2) - 1.0 / 3.0) / 3.0
    assert gm.promoted(np.uint16) == (True, 32) and gm.promoted(np.uint32) == (False, 32)


def test_pack_calls_respects_the_budget():
    for dt in gc.ALL_DT:
        for budget in (1, 4, 7, 8):
            for call in gc.pack_calls(gc.INT_OPS, dt, budget):
                assert call and sum(gc.acc_count(op, dt) for op in call) <= budget
    assert gc.pack_calls(gc.INT_OPS, gc.I32, 1, count_ok=False) == [[gc.SUM], [gc.MIN], [gc.MAX]]
