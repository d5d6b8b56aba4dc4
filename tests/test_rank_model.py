"""The ranking contract on the CPU: the model of tests/rank_model.py equals pandas' recorded answers (tests/golden/rank_pandas.json,
written by tools/gen_rank_golden.py) bit for bit, its two statements agree on every case of tests/rank_cases.py, and those cases
refuse every planted mistake of rank_model.MISTAKES.  Also: aqg_rank_out_dtype for the eight methods and the bindings capi declares."""
import json
import os
import re

import numpy as np
import pytest

import rank_cases as rc
import rank_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "rank_pandas.json")))


def golden_column(case):
    dt = np.dtype(case["dtype"])
    bits = np.array(case["bits"], {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize])
    return bits.view(dt)


def test_model_equals_pandas():
    assert sum(len(case["sizes"]) for case in GOLDEN["cases"]) >= 36                       # slices: whole columns and groups
    checked = 0
    for case in GOLDEN["cases"]:
        x = golden_column(case)
        assert len(x) == case["n"] <= 40
        starts = np.concatenate([[0], np.cumsum(case["sizes"])[:-1]]).astype(np.int64)
        for order, oname in ((rm.ASC, "asc"), (rm.DESC, "desc")):
            want = case["results"][oname]
            for statement in (rm.five_sorted, rm.five_counting):
                five = statement(x, starts, order)
                for method in rm.METHODS:
                    name = rm.METHOD_NAMES[method]
                    for k in (GOLDEN["ks"] if method == rm.NTILE else [0]):
                        w = want[name][str(k)] if method == rm.NTILE else want[name]
                        w = np.array(w, np.float64) if rm.is_double(method) else np.array(w, np.uint32)
                        got = rm.finish(method, k, five)
                        assert rm.same_bits(got, w), (case["dtype"], case["sizes"], oname, name, k)
                        checked += 1
    assert checked > 1000


FIVES = {}


def five_of(c, order):
    """the first statement's five integers of a case (computed once, shared)"""
    key = (c.name, order)
    if key not in FIVES:
        FIVES[key] = rm.five_sorted(c.x, c.starts, order)
    return FIVES[key]


@pytest.mark.parametrize("order", [rm.ASC, rm.DESC], ids=["asc", "desc"])
def test_statements_agree(order):
    cases = rc.all_cases()
    assert len(cases) > 200
    for c in cases:
        a, b = five_of(c, order), rm.five_counting(c.x, c.starts, order)
        for name, u, v in zip(("min", "max", "dense", "first", "c"), a, b):
            assert np.array_equal(u, v), (c.name, name)
        assert (a[0] <= a[3]).all() and (a[3] <= a[1]).all() and (a[1] <= a[4]).all() and (a[2] <= a[0]).all() and (a[2] >= 1).all()


def test_cases_cover_the_edges():
    """what the issue asks the cases to hold, read back from them"""
    cases = rc.all_cases()
    sm, et = rc.SMALL_MAX, rc.ET
    sizes = [np.diff(np.append(c.starts, len(c.x))) for c in cases if c.keys_row is not None]
    seen = set(int(s) for a in sizes for s in a)
    assert {1, 2, 3, sm - 1, sm, sm + 1} <= seen
    assert any(len(a) == 1 for a in sizes) and any((a == 1).all() and len(a) > rc.TILE for a in sizes)
    assert {255, 256, 257} <= {len(a) for a in sizes}
    assert any(a.max() > 3 * et and (a == 1).sum() >= 4 for a in sizes)
    # SMALL groups that straddle a TILE-position tile; groups of both routes in one case
    assert any(((np.cumsum(a) - a) // rc.TILE != (np.cumsum(a) - 1) // rc.TILE)[a <= sm].any() for a in sizes)
    assert any((a <= sm).any() and (a > sm).any() for a in sizes)
    # tie runs that begin on, end on and span an emit-tile edge (in the sorted order of a one-slice case)
    c = next(c for c in cases if c.name == "flat-int32-edge_runs")
    mn, mx = five_of(c, rm.ASC)[:2]
    heads, ends = set((mn - 1).tolist()), set(mx.tolist())
    assert et in heads and 2 * et in heads and et in ends and any(h < 3 * et < e for h, e in zip(sorted(heads), sorted(ends)))
    # an all-equal and an all-distinct slice, both zeros and several NaNs, both infinities, the ends of the integer types, uint64 above 2^53
    assert any(len(np.unique(c.x)) == 1 and len(c.x) > et for c in cases) and any(len(np.unique(c.x)) == len(c.x) > et for c in cases)
    f = [c for c in cases if c.dtype.kind == "f" and c.name.endswith("special")]
    assert any(np.isnan(c.x).sum() > 3 and np.signbit(c.x[c.x == 0]).any() and (~np.signbit(c.x[c.x == 0])).any() and np.isposinf(c.x).any() and np.isneginf(c.x).any() for c in f)
    for dt in rc.ALL_DTYPES:
        if np.dtype(dt).kind in "iu":
            info = np.iinfo(dt)
            assert any(c.dtype == dt and (c.x == info.min).any() and (c.x == info.max).any() for c in cases), dt
    assert any(c.dtype == np.uint64 and (c.x > 2 ** 53).sum() > 2 and len(np.unique(c.x.astype(np.float64))) < len(np.unique(c.x)) for c in cases)
    assert any(c.dtype == np.bool_ for c in cases)
    c = next(c for c in cases if c.name.startswith("flat-int32-n%d-" % (et + 1)))
    n = len(c.x)
    assert {1, n - 1, n, n + 1, 7} <= set(c.ks) and n % 7


@pytest.mark.parametrize("bug", rm.MISTAKES)
def test_planted_mistake_is_refused(bug):
    """some case, method and order tells the mistaken model from the contract"""
    assert len(rm.MISTAKES) >= 10
    for c in rc.all_cases():
        for order in (rm.ASC, rm.DESC):
            good = five_of(c, order)
            bad = rm.five_sorted(c.x, c.starts, order, bug=bug, tile=rc.ET)
            for method in rm.METHODS:
                for k in (c.ks if method == rm.NTILE else [0]):
                    if not rm.same_bits(rm.finish(method, k, good), rm.finish(method, k, bad, bug=bug)):
                        return
    pytest.fail("no case refuses the planted mistake %r" % bug)


def test_big_case_is_consistent():
    """the many-tile column the GPU test runs (too long for the counting statement): the invariants of the five integers"""
    c = rc.big_case()
    mn, mx, dense, first, cc = rm.five_sorted(c.x, c.starts, rm.ASC)
    assert (cc == len(c.x)).all() and sorted(first.tolist()) == list(range(1, len(c.x) + 1))
    vals, counts = np.unique(c.x, return_counts=True)
    assert np.array_equal(dense, np.searchsorted(vals, c.x) + 1) and np.array_equal(mx - mn + 1, counts[dense - 1])


def test_out_dtype_and_bindings():
    from aquery2_amd import capi
    for name in ("aqg_rank_out_dtype", "aqg_rank", "aqg_grouped_rank", "aqg_grouped_rank_flat", "aqg_rank_last"):
        assert name in capi.RANK_PROTOTYPES, name
    assert [capi.RANK_MIN, capi.RANK_MAX, capi.RANK_DENSE, capi.RANK_FIRST, capi.RANK_AVERAGE, capi.RANK_PERCENT, capi.RANK_CUME_DIST, capi.RANK_NTILE] == list(rm.METHODS)
    hdr = open(os.path.join(ROOT, "include", "aqg.h")).read()
    for method, name in enumerate(("MIN", "MAX", "DENSE", "FIRST", "AVERAGE", "PERCENT", "CUME_DIST", "NTILE")):
        assert re.search(r"AQG_RANK_%s = %d\b" % (name, method), hdr), name
    lib = capi.load_library()
    for method in rm.METHODS:
        assert lib.aqg_rank_out_dtype(method) == (capi.DOUBLE if rm.is_double(method) else capi.UINT32)
        assert capi.TAG2NP[lib.aqg_rank_out_dtype(method)] == rm.out_dtype(method)
    assert lib.aqg_rank_out_dtype(-1) == -1 and lib.aqg_rank_out_dtype(8) == -1
