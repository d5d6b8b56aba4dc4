"""The pair windows on the device -- aqg_scan2, aqg_grouped_scan2, aqg_grouped_scan2_flat -- against the exact rational model
(tests/pair_moments.py) under its accuracy contract, over the case list of tests/pairwin_cases.py: every case through every entry, twice
and bit-identical, the route read back with aqg_scan2_last, the row-layout entry equal to flatten + the flat entry bit for bit."""
import numpy as np
import pytest

import exact_moments as em
import pair_moments as pm
import pairwin_cases as pc
from aquery2_amd import capi as P

pytestmark = pytest.mark.gpu

WOPS = {pm.COV: P.SCAN2_COVW, pm.CORR: P.SCAN2_CORRW, pm.BETA: P.SCAN2_BETAW}
SOPS = {pm.COV: P.SCAN2_COVS, pm.CORR: P.SCAN2_CORRS, pm.BETA: P.SCAN2_BETAS}
ERR_DTYPE, ERR_ARG = 2, 3
FLAT, LINEAR, NONFINITE, GROUPED = pc.flat_cases(), pc.linear_cases(), pc.nonfinite_cases(), pc.grouped_cases()


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run_op(d, case, gb, fam, w, cols=None):
    """one op of one case through every entry of its layout, each twice; returns the result (the entries agree bit for bit)"""
    op, ww = (SOPS[fam], 0) if w is None else (WOPS[fam], int(w))
    x, y = cols if cols is not None else (case.x, case.y)
    what = (case.name, fam, w)
    if gb is None:
        got = d.scan2(op, x, y, ww)
        assert d.scan2_last() == (pc.route_of(w, len(case.x)), pc.TS), what
        assert same_bits(got, d.scan2(op, x, y, ww)), what
        return got
    flat = d.grouped_scan2(gb, op, x, y, ww, flat=True)
    assert d.scan2_last() == (pc.route_of(w, len(case.x)), pc.TS), what
    assert same_bits(flat, d.grouped_scan2(gb, op, x, y, ww, flat=True)), what
    row = d.grouped_scan2(gb, op, case.x_row, case.y_row, ww)
    assert d.scan2_last() == (pc.route_of(w, len(case.x)), pc.TS), what
    assert same_bits(row, flat), (what, "row layout against flatten + flat")
    assert same_bits(row, d.grouped_scan2(gb, op, case.x_row, case.y_row, ww)), what
    return flat


def hold_case(d, case, gb=None):
    """every op and window of a case against the model; returns the routes taken"""
    n = len(case.x)
    ex = pm.PairExact(case.x, case.y, pc.offsets_of(case))
    xd, yd = d.to_device(case.x), d.to_device(case.y)
    routes = 0
    for w in [None] + list(case.windows):
        for fam in (pm.COV, pm.CORR, pm.BETA):
            if fam != pm.COV and not case.long_ok and pc.route_of(w, n) == pc.ROUTE_PREFIX:
                continue
            got = run_op(d, case, gb, fam, w, cols=(xd, yd))
            ill = ex.check(got, fam, w, "%s/fam%d/w%s" % (case.name, fam, w))
            assert 100 * ill <= n, (case.name, fam, w, ill)
            routes |= pc.route_of(w, n)
    return routes


@pytest.mark.parametrize("case", FLAT, ids=[c.name for c in FLAT])
def test_flat(gpu, case):
    hold_case(gpu, case)


@pytest.mark.parametrize("case", GROUPED, ids=[c.name for c in GROUPED])
def test_grouped(gpu, case):
    gb = gpu.groupby_build([case.keys_row])
    try:
        assert gb.ngroups == len(case.starts)
        hold_case(gpu, case, gb)
    finally:
        gb.destroy()


def test_every_route_flat_and_grouped(gpu):
    c = next(c for c in GROUPED if c.name.startswith("grouped-halo3"))
    gb = gpu.groupby_build([c.keys_row])
    seen = {"flat": 0, "grouped": 0}
    for w in (None, 8, 9, 64, 65):
        gpu.scan2(P.SCAN2_COVS if w is None else P.SCAN2_COVW, c.x, c.y, w or 0)
        seen["flat"] |= gpu.scan2_last()[0]
        gpu.grouped_scan2(gb, P.SCAN2_CORRS if w is None else P.SCAN2_CORRW, c.x, c.y, w or 0, flat=True)
        seen["grouped"] |= gpu.scan2_last()[0]
    gb.destroy()
    assert seen == {"flat": 7, "grouped": 7}, seen


@pytest.mark.parametrize("dt", [np.int32, np.float64, np.uint64])
def test_cov_of_a_column_with_itself_is_varw(gpu, dt):
    x = pc.family(np.random.default_rng(5), "offset", dt, 2049)
    ex = em.Exact(x)
    for w in (None, 2, 8, 9, 64, 65, 1000):
        got = gpu.scan2(P.SCAN2_COVS if w is None else P.SCAN2_COVW, x, x, w or 0)
        ex.check(got, ex.var(w), w, what="cov(x, x)/%s/w%s" % (np.dtype(dt).name, w))


@pytest.mark.parametrize("a,case", LINEAR, ids=[c.name for _, c in LINEAR])
def test_linear_dependence(gpu, a, case):
    ex = pm.PairExact(case.x, case.y)
    for w in [None] + list(case.windows):
        m = ex.moments(w)
        ok = ~m["vx0"]
        assert np.all(m["beta"][ok] == a) and np.all(m["corr"][ok] == np.sign(a)), "the model itself"
        for fam in (pm.CORR, pm.BETA):
            ex.check(run_op(gpu, case, None, fam, w), fam, w, "%s/fam%d/w%s" % (case.name, fam, w))


def test_swapping_the_columns(gpu):
    for case in FLAT[10:14]:                                             # the four mixed dtype pairs
        ex = pm.PairExact(case.x, case.y)
        for w in (None, 3, 64, 1000):
            for fam in (pm.COV, pm.CORR):
                got = gpu.scan2(SOPS[fam] if w is None else WOPS[fam], case.y, case.x, w or 0)
                ex.check(got, fam, w, "%s/swapped/fam%d/w%s" % (case.name, fam, w))


@pytest.mark.parametrize("case", NONFINITE, ids=[c.name for c in NONFINITE])
def test_non_finite_rows(gpu, case):
    """rows before the first non-finite row against the model of the truncated column; on the short routes also the windows behind it
    that no longer hold it, against the model of the column with that row replaced (those windows do not see the replacement)"""
    n, cut = len(case.x), case.cut
    head = pm.PairExact(case.x[:cut], case.y[:cut])
    xr, yr = case.x.copy(), case.y.copy()
    xr[cut], yr[cut] = 1.0, 2.0
    whole = pm.PairExact(xr, yr)
    for w in [None] + list(case.windows):
        for fam in (pm.COV, pm.CORR, pm.BETA):
            got = run_op(gpu, case, None, fam, w)
            what = "%s/fam%d/w%s" % (case.name, fam, w)
            head.check(got[:cut], fam, w, what)
            if pc.route_of(w, n) != pc.ROUTE_PREFIX:
                whole.check(got, fam, w, what + "/behind", upto=np.arange(n) >= cut + int(w))


def raw_call(d, entry, gbh, op, tx, ty, w, n=100):
    """an entry called with a poisoned output; returns (status, output untouched)"""
    x = d.to_device(np.arange(n, dtype=np.float64))
    out = d.to_device(np.full(n, 7.25))
    if gbh is None:
        rc = d.lib.aqg_scan2(d.ctx, op, tx, x.ptr, ty, x.ptr, n, w, out.ptr)
    else:
        rc = getattr(d.lib, entry)(d.ctx, gbh, op, tx, x.ptr, ty, x.ptr, w, out.ptr)
    d.sync()
    return rc, bool(np.all(out.to_host() == 7.25))


def test_errors_write_nothing(gpu):
    d = gpu
    keys = (np.arange(100) % 7).astype(np.int32)
    gb = d.groupby_build([keys])
    agg = d.groupby_agg([keys], [0], [np.arange(100, dtype=np.int32)])
    for entry, h in (("aqg_scan2", None), ("aqg_grouped_scan2", gb.h), ("aqg_grouped_scan2_flat", gb.h)):
        for op in (P.SCAN2_COVW, P.SCAN2_CORRW, P.SCAN2_BETAW):
            assert raw_call(d, entry, h, op, P.DOUBLE, P.DOUBLE, 0) == (ERR_ARG, True), (entry, op, "w == 0")
        assert raw_call(d, entry, h, P.SCAN2_COVS, P.DOUBLE, P.DOUBLE, 0)[0] == 0, (entry, "w is ignored by the running ops")
        for tx, ty in ((P.INT128, P.DOUBLE), (P.DOUBLE, P.UINT128), (P.STR, P.DOUBLE), (P.DOUBLE, 99)):
            assert raw_call(d, entry, h, P.SCAN2_COVW, tx, ty, 5) == (ERR_DTYPE, True), (entry, tx, ty)
        for op in (-1, 6, 99):
            assert raw_call(d, entry, h, op, P.DOUBLE, P.DOUBLE, 5) == (ERR_ARG, True), (entry, op)
    for entry in ("aqg_grouped_scan2", "aqg_grouped_scan2_flat"):
        assert raw_call(d, entry, agg.h, P.SCAN2_COVW, P.DOUBLE, P.DOUBLE, 5) == (ERR_ARG, True), (entry, "a handle of aqg_groupby_agg")
    # n == 0: AQG_OK, nothing written
    out = d.to_device(np.full(4, 7.25))
    assert d.lib.aqg_scan2(d.ctx, P.SCAN2_CORRW, P.DOUBLE, None, P.DOUBLE, None, 0, 3, out.ptr) == 0
    d.sync()
    assert np.all(out.to_host() == 7.25)
    gb.destroy()
    agg.destroy()


def test_emitted_group_loop(tmp_path):
    """tests/emitted/pair_windows.cpp over host_main's synthetic dataset (2e5 rows): `corrw(20, c[vecs[g]], a[vecs[g]], col[g])`,
    `covs(...)` and `betaw(100, ...)` in the generated group loop cost ONE aqg_grouped_scan2_flat per (op, x, y, w), at 100 groups and at
    10; the flat forms go through aqg_scan2; everything is held to the model"""
    import subprocess
    from test_gpu_emitted import EM, run
    from test_gpu_quantiles import _synthetic
    import quantile_model as qm
    subprocess.check_call(["make", "-C", EM, "build/pair_windows.so", "build/host_main"], stdout=subprocess.DEVNULL)
    a, c = _synthetic()
    run("pair_windows.so", "synthetic", "dll_pair_flat", "dll_pair_group100", "dll_pair_group10", cwd=str(tmp_path))
    n = len(c)
    ops = ((pm.CORR, 20), (pm.COV, None), (pm.BETA, 100))
    ex = pm.PairExact(c, a)
    for j, (fam, w) in enumerate(ops):
        ex.check(np.fromfile(tmp_path / ("pairf.out.%d" % j), np.float64), fam, w, "emitted flat %d" % j)
    for name, key, G in (("pairg100", a % 100, 100), ("pairg10", a % 10, 10)):
        gid, ng = qm.first_occurrence_ids(key)
        assert ng == G
        # the group loop's row lists: groups in first-occurrence order, a group's rows in descending row id (the flat layout)
        order = np.lexsort((-np.arange(n), gid))
        starts = np.flatnonzero(np.diff(gid[order], prepend=-1))
        first = np.full(G, n, np.int64)
        np.minimum.at(first, gid, np.arange(n))
        assert np.array_equal(np.fromfile(tmp_path / (name + ".out.0"), np.int32), key[first])
        exg = pm.PairExact(c[order], a[order], np.append(starts, n))
        for j, (fam, w) in enumerate(ops, start=1):
            exg.check(np.fromfile(tmp_path / ("%s.out.%d" % (name, j)), np.float64), fam, w, "%s %d" % (name, j))
        assert (tmp_path / (name + ".out.4")).read_bytes() == (tmp_path / (name + ".out.1")).read_bytes()
        calls, groups = (int(v) for v in (tmp_path / (name + ".calls")).read_text().split())
        assert groups == G and calls == 3, "one grouped call per (op, x, y, w), whatever the number of groups"
