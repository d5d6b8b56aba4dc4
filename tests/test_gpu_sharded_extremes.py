"""The row-range-sharded layer at the numeric extremes: aqg_reduce_sharded, aqg_corr_sharded, aqg_scan_sharded (csrc/sharded.hip) and
aqg_groupby_agg_sharded through both merge paths of csrc/exchange.hip, against the oracle's answer for the WHOLE column or table -- and
the flat aqg_corr, which had only met 5000 rows of small integers.  Ranks are threads of one process on one GPU (aquery2_amd.ThreadRanks,
as tests/test_gpu_sharded.py), at most five of them.  The cuts, the inputs and the comparisons are tests/sharded_cases.py; what they are
worth is tests/test_sharded_cases.py: every way this layer's folds could be wrong is refused there by a case of the lists run here.

What is compared, and how -- the standards are those of tests/test_gpu_extremes.py's module docstring, applied through its own helpers:

  reductions   every op of checker.RED_NAMES on every dtype, over every cut of 70 001 rows and of 5 rows.  Integers (full range with the type's
               ends planted; 8-byte columns whose 128-bit sum carries or borrows in the fold ACROSS shards; avg probes whose rows up to the
               sums S - 1, S, S + 1 lie in different shards): bit for bit.  Floating columns (finite, +Inf, +-Inf): sum within
               n 2^-52 sum|finite x|, avg that over n, var / stddev within test_reduce_var_stddev_floating's bound, min / max / first / last
               bit for bit.  Seeds (strictly negative, all +Inf, such shards in front of and behind tame ones), a column of -0.0 only and one of
               subnormals only: the same.  Every rank must return the same bits.
  corr         groupagg_cases.CORR_PAIRS at full range, the full product of two pools, constant columns: bit for bit (NaN where the oracle
               has NaN, the same infinity); aqg_corr on one device at 1, 2, 2047, 2049 and 70 001 rows, operands 0 and 1 element past alignment
  scans        every op aqg_scan_sharded offers on every dtype, over every cut, the ranks' rows laid end to end.  Integers bit for bit, and equal
               to aqg_scan of the whole column on one device (csrc/sharded.hip: "integer results are bit-identical to the single-GPU call");
               avgw of integers the exact window mean to one ulp; floating mins / maxs / minw / maxw / shifts / ratiow bit for bit; floating
               sums / avgs / sumw / avgw under check_fp_sums' bound against the oracle, and sumw / avgw also against the sum of the rows the
               device's route adds -- per call: a shard behind the column's start is computed by two aqg_scan calls (sharded_cases.check_window_rows);
               varw / stddevw against the exact variance (tests/exact_moments.py: the contract of test_gpu_variance.py)
  group-by     groupagg_cases' group shapes and value sets at 60 011 rows, every rank's result against the oracle's group-by of the whole
               table: group count, global first rows, keys, every aggregate through groupagg_cases.compare

The largest |got - want| / bound of every floating sum family is printed by the test that measured it (DESIGN.md section 2 records them).

What is left out, and why -- nothing else is skipped, and nothing is skipped depending on the data:

  case                                              out of contract because
  ------------------------------------------------  ------------------------------------------------------------------------------
  vars / stddevs over shards                        include/aqg.h: "vars / stddevs are not offered" -- AQG_ERR_DTYPE on every rank (asserted)
  sumw / avgw / varw / stddevw with w == 0          DESIGN.md 2: "`sumw/avgw` with `w == 0` read `ret[-1]` (rejected with `AQG_ERR_ARG`)" (asserted)
  avgw on uint32 / uint64 columns                   DESIGN.md 2: "`avgw` on unsigned 4/8-byte inputs wraps `arr[i]-arr[i-w]` ...; the
                                                    device returns the true mean"
  avgw on int32 / int64 columns at full range       the same expression overflows a signed type there: halved columns (test_gpu_extremes.int_column)
  a NaN in a column of the min / max or the         DESIGN.md 2, "NaN and signed zeros": every output row strictly before the column's first NaN row is
  floating sum family                               held to the standards above, every rank's call succeeds; reductions: count / first / last
  sumw / avgw rows from the reference's first       same sentence: when an Inf row leaves the window the reference's recurrence computes
  NaN OUTPUT on                                     Inf - Inf and stays NaN
  floating sumw / avgw through HBM: the rows        DESIGN.md 2: "Floating sums: any re-ordered summation is bounded by ..." -- prefix_diff_kernel
  the route adds                                    sums the whole prefix of the call's column: the oracle's prefix-wide bound is the standard
  corr of floating or uint64 columns                csrc/reduce.hip: floating inputs are refused with AQG_ERR_DTYPE (asserted); uint64 has no kernel
  nine avg-probe groups in the group-by             the three groups of e = 77 take 49 161 rows, more than 60 011 rows leave beside a group of a third
                                                    of them: six probe groups (e = 53, 64) there, e = 77 under aqg_reduce_sharded
  the merge path read back                          no handle or communicator exposes it.  csrc/exchange.hip takes the one-launch merge when
                                                    `gmax && nkeys == 1 && nparts <= XS_MAXCOL (6) && gcap * world <= XS_ROWS (1024)`, the key is a
                                                    non-floating type of at most 8 bytes and every payload column is an integer SUM / MIN / MAX or a
                                                    double SUM; a floating MIN / MAX, gmax == 0, a second key column or more groups than that send the
                                                    call through concatenate + re-aggregate.  (A float32 SUM travels as a double: it alone does not
                                                    change the path; float32 columns are run on both sides.)  sharded_cases.takes_small_merge restates
                                                    the condition and every test asserts it for each of its calls: the one-launch test makes a call
                                                    of their own of a floating column's MIN / MAX, so its SUM / COUNT / AVG stay on that merge
"""
import numpy as np
import pytest

import checker as ck
import extremes as ex
import groupagg_cases as gc
import sharded_cases as sc
from test_gpu_edges import view

pytestmark = pytest.mark.gpu
RED = ck.RED_NAMES


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def run_ranks(world, body):
    import aquery2_amd
    tr = aquery2_amd.ThreadRanks(world)
    try:
        return tr.run(body)
    finally:
        tr.close()


def status_of(call):
    import aquery2_amd
    try:
        call()
        return 0
    except aquery2_amd.capi.AqgError as e:
        return e.code


class Ratios(dict):
    def note(self, key, r):
        self[key] = max(self.get(key, 0.0), r)

    def show(self, what):
        if self:
            print(f"{what}: largest |got - want| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.items())), flush=True)
        assert all(v <= 1.0 for v in self.values()), self


# ---- reductions ------------------------------------------------------------------------------------------------------------------------------
_WHOLE = {}


def whole_column(oracle, case):
    """oracle.reduce of the whole column, once per case"""
    if case["name"] not in _WHOLE or _WHOLE[case["name"]][0] is not case["x"]:
        _WHOLE[case["name"]] = (case["x"], {name: oracle.reduce(op, case["x"]) for name, op in RED.items()})
    return _WHOLE[case["name"]][1]


def reduce_over(sh_of, cases):
    """{case name: {op: result}} per rank; sh_of(case): its cut (every case of one call has the same number of ranks)"""
    world = len(sh_of(cases[0]))

    def body(rank, dev, comm):
        out = {}
        for case in cases:
            lo, hi = sh_of(case)[rank]
            xs = dev.to_device(np.ascontiguousarray(case["x"][lo:hi]))
            out[case["name"]] = {name: comm.reduce_sharded(op, xs) for name, op in RED.items()}
        return out
    return run_ranks(world, body)


def check_reductions(oracle, cases, res, what):
    ratios = Ratios()
    for case in cases:
        want = whole_column(oracle, case)
        for r, out in enumerate(res):
            got = out[case["name"]]
            for name in RED:
                ratio = sc.check_reduce(case, name, got[name], want[name], wv=want["var"], gv=got["var"])
                if case["kind"] != "int" and name in ("sum", "avg", "var"):
                    ratios.note(f"{name}({case['x'].dtype.name})", ratio)
            if case["kind"] == "int":
                assert got["sum"] == sc.exact_sum_fast(case["x"]), (case["name"], r)
            if case["kind"] != "nan":
                assert all(ex.same(np.asarray(got[name]), np.asarray(res[0][case["name"]][name])) if not isinstance(got[name], int) else got[name] == res[0][case["name"]][name]
                           for name in RED), (case["name"], "rank", r, "differs from rank 0")
    ratios.show(what)


@pytest.mark.parametrize("cut", sc.cut_names(sc.N))
def test_reductions_over_shards(oracle, cut):
    cases = sc.reduce_cases()
    sh = sc.shards(cut, sc.N)
    check_reductions(oracle, cases, reduce_over(lambda case: sh, cases), f"aqg_reduce_sharded {cut}")


@pytest.mark.parametrize("cut", sc.cut_names(sc.N_TINY))
def test_reductions_over_more_ranks_than_rows(oracle, cut):
    cases = sc.reduce_cases(sc.N_TINY)
    sh = sc.shards(cut, sc.N_TINY)
    check_reductions(oracle, cases, reduce_over(lambda case: sh, cases), f"aqg_reduce_sharded {cut} (5 rows)")


@pytest.mark.parametrize("cut", ["even3", "last-rows-apart", "one-row-last"])
def test_avg_rounds_the_128_bit_total_once(oracle, cut):
    """ex.avg_probe_column's rows up to S - 1, S and S + 1, the probe rows in different shards: avg is float(total) / float(rows), from the
    exact 128-bit total of the shards' sums"""
    cases = [dict(name=name, x=x, kind="int", s=s) for name, x, s in sc.probe_cases()]
    res = reduce_over(lambda case: sc.probe_cuts(len(case["x"]))[cut], cases)
    check_reductions(oracle, cases, res, f"avg probes {cut}")
    for case in cases:
        for out in res:
            assert out[case["name"]]["sum"] == case["s"]
            assert np.float64(out[case["name"]]["avg"]).tobytes() == np.float64(float(case["s"]) / float(len(case["x"]))).tobytes(), case["name"]


# ---- corr --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", sc.cut_names(sc.N))
def test_corr_over_shards(oracle, cut):
    cases = [c for c in sc.corr_cases() if cut in sc.cut_names(len(c[1]))]
    world = len(sc.shards(cut, sc.N))

    def body(rank, dev, comm):
        out = []
        for name, x, y in cases:
            lo, hi = sc.shards(cut, len(x))[rank]
            out.append(comm.corr_sharded(np.ascontiguousarray(x[lo:hi]), np.ascontiguousarray(y[lo:hi])))
        return out
    res = run_ranks(world, body)
    for k, (name, x, y) in enumerate(cases):
        want = oracle.corr(x, y)
        for r in range(world):
            assert ex.same(np.float64(res[r][k]), np.float64(want)), (name, cut, r, res[r][k], want)


@pytest.mark.parametrize("n", [1, 2, 2047, 2049, 70_001])
def test_corr_on_one_device(gpu, oracle, n):
    """aqg_corr itself: full-range pairs, the full product of two pools (its own length), constant columns; operands 0 and 1 element past alignment"""
    for name, x, y in sc.corr_cases(n):
        for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            got, want = gpu.corr(view(gpu, x, ox), view(gpu, y, oy)), oracle.corr(x, y)
            assert ex.same(np.float64(got), np.float64(want)), (name, n, ox, oy, got, want)


def test_corr_refuses_floating_operands(gpu):
    i, f = np.arange(10, dtype=np.int32), np.arange(10, dtype=np.float32)
    for x, y in ((f, i), (i, f), (f.astype(np.float64), f)):
        assert status_of(lambda: gpu.corr(x, y)) == 2                 # AQG_ERR_DTYPE (include/aqg.h)

    def body(rank, dev, comm):
        return [status_of(lambda: comm.corr_sharded(x[rank * 5:rank * 5 + 5], y[rank * 5:rank * 5 + 5])) for x, y in ((f, i), (i, f))]
    assert run_ranks(2, body) == [[2, 2], [2, 2]]


# ---- scans, windows and shifts -------------------------------------------------------------------------------------------------------------------
_SCAN_REF = {}


def scan_refs(gpu, oracle, dt, name, label, x, w):
    """(oracle.scan, aqg_scan on one device -- for the integer results that are bit for bit) of the whole column, kept while the tests of one dtype run"""
    if _SCAN_REF.get("dt") != (dt.name, len(x)):
        _SCAN_REF.clear()
        _SCAN_REF["dt"] = (dt.name, len(x))
    key = (name, label, w)
    if key not in _SCAN_REF or _SCAN_REF[key][0] is not x:             # (a label names one column: the entry holds it)
        op = ck.SCAN_NAMES[name]
        one = gpu.scan(op, x, w) if dt.kind != "f" and name in sc.BITWISE_INT else None
        _SCAN_REF[key] = (x, oracle.scan(op, x, w) if name not in sc.gsc.VAR_OPS else None, one)
    return _SCAN_REF[key][1:]


def scan_over(sh, plan):
    def body(rank, dev, comm):
        lo, hi = sh[rank]
        up, out = {}, []
        for name, label, x, w in plan:
            if id(x) not in up:
                up[id(x)] = dev.to_device(np.ascontiguousarray(x[lo:hi]))
            out.append(comm.scan_sharded(ck.SCAN_NAMES[name], up[id(x)], w))
        return out
    return run_ranks(len(sh), body)


def check_scans(gpu, oracle, dt, sh, plan, res, what, first_nan=None):
    ratios = Ratios()
    for k, (name, label, x, w) in enumerate(plan):
        got = np.concatenate([res[r][k] for r in range(len(sh))])
        assert got.size == len(x) and all(len(res[r][k]) == hi - lo for r, (lo, hi) in enumerate(sh)), (what, name, w)
        want, one = scan_refs(gpu, oracle, dt, name, label, x, w)
        ratio = sc.check_scan(name, x, w, got, want, sh=sh, one_device=one, first_nan=first_nan, what=f"{what} {label}")
        if dt.kind == "f" and name in sc.gsc.SUM_OPS:
            ratios.note(f"{name}({dt.name})", ratio)
    ratios.show(what)


@pytest.mark.parametrize("dt,cut", [(dt, cut) for dt in ex.NUM_DTYPES for cut in sc.cut_names(sc.N)], ids=lambda v: getattr(v, "name", v))
def test_scans_over_shards(gpu, oracle, dt, cut):
    sh = sc.shards(cut, sc.N)
    plan = sc.scan_plan(dt, sc.N)
    check_scans(gpu, oracle, dt, sh, plan, scan_over(sh, plan), f"aqg_scan_sharded {cut}")


@pytest.mark.parametrize("cut", sc.cut_names(sc.N_TINY))
def test_scans_over_more_ranks_than_rows(gpu, oracle, cut):
    sh = sc.shards(cut, sc.N_TINY)
    for dt in ex.NUM_DTYPES:
        plan = sc.scan_plan(dt, sc.N_TINY)
        check_scans(gpu, oracle, dt, sh, plan, scan_over(sh, plan), f"aqg_scan_sharded {cut} (5 rows)")


def test_scans_that_are_not_offered_fail_on_every_rank():
    x = np.arange(1, 31, dtype=np.int32)

    def body(rank, dev, comm):
        mine = x[rank * 10: rank * 10 + 10]
        return ([status_of(lambda: comm.scan_sharded(ck.SCAN_NAMES[name], mine)) for name in ("vars", "stddevs")],
                [status_of(lambda: comm.scan_sharded(ck.SCAN_NAMES[name], mine, 0)) for name in ("sumw", "avgw", "varw", "stddevw")],
                comm.scan_sharded(ck.SCAN_MAXS, mine)[-1])            # the communicator stays usable
    res = run_ranks(3, body)
    assert [r[0] for r in res] == [[2, 2]] * 3 and [r[1] for r in res] == [[3, 3, 3, 3]] * 3          # AQG_ERR_DTYPE, AQG_ERR_ARG
    assert [int(r[2]) for r in res] == [10, 20, 30]


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("cut", ["even3", "tiny_middle", "empty_middle_then_tiny"])
def test_negative_zero_as_the_last_row_of_a_shard(gpu, oracle, dt, cut):
    sh = sc.shards(cut, sc.N)
    x = sc.zero_border_column(dt, sh)
    assert all(np.signbit(x[hi - 1]) and x[hi - 1] == 0 for lo, hi in sh if hi > lo) and np.count_nonzero(x == 0) == sum(hi > lo for lo, hi in sh)
    plan = [(name, f"-0.0 at the borders of {cut}", x, 0) for name in ("prev", "deltas", "mins", "maxs", "aggnext")]
    check_scans(gpu, oracle, dt, sh, plan, scan_over(sh, plan), f"-0.0 borders {cut}")


NAN_CUTS = {"first shard": "even3", "tiny shard": "tiny_middle", "last row of a shard": "even3"}


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("where", list(sc.NAN_PLACES))
def test_nan_rows_over_shards(gpu, oracle, dt, where):
    """one NaN row -- in the first shard, in the three-row shard, as the last row of a shard: every output row strictly before it is held to the usual
    standards, every rank's call succeeds (what comes back behind a NaN is unspecified: DESIGN.md section 2)"""
    x = sc.nan_column(dt, where)
    first = sc.NAN_PLACES[where]
    sh = sc.shards(NAN_CUTS[where], sc.N)
    assert np.isnan(x[first]) and np.count_nonzero(np.isnan(x)) == 1 and any(lo <= first < hi for lo, hi in sh)
    if where == "tiny shard": assert sh[1][0] <= first < sh[1][1] and sh[1][1] - sh[1][0] == 3
    if where == "last row of a shard": assert first == sh[0][1] - 1
    plan = [(name, f"NaN in the {where}", x, 0) for name in ("mins", "maxs", "sums", "avgs")] + \
           [(name, f"NaN in the {where}", x, w) for name in ("minw", "maxw", "sumw", "avgw") for w in (5, 1000, 50_000, sc.N)]
    check_scans(gpu, oracle, dt, sh, plan, scan_over(sh, plan), f"NaN {where}", first_nan=first)


# ---- the sharded group-by -------------------------------------------------------------------------------------------------------------------------
def groupby_over(sh, keys, calls, gmax, hint):
    """calls: [(ops, column)]; per rank a list of dict(G, keys, first, res) in call order"""
    def body(rank, dev, comm):
        lo, hi = sh[rank]
        k = [dev.to_device(np.ascontiguousarray(c[lo:hi])) for c in keys]
        up, out, gb = {}, [], None
        for ops, x in calls:
            if id(x) not in up:
                up[id(x)] = dev.to_device(np.ascontiguousarray(x[lo:hi]))
            gb = comm.groupby_agg_sharded(k, list(ops), [up[id(x)]] * len(ops), row_base=lo, hint=hint, gmax=gmax, handle=gb)
            out.append(dict(G=gb.ngroups, keys=[gb.keys(i, c.dtype) for i, c in enumerate(keys)], first=gb.first_rows64(),
                            res=[gb.result(j, op, ck.tag_of(x)) for j, op in enumerate(ops)]))
        if gb is not None:
            gb.destroy()
        return out
    return run_ranks(len(sh), body)


def check_groupby(oracle, o, keys, calls, res, what, ratios):
    stats, share = {}, 1.0
    for c, (ops, x) in enumerate(calls):
        for r, out in enumerate(res):
            got = out[c]
            assert got["G"] == o["ngroups"], (what, r, got["G"], o["ngroups"])
            assert np.array_equal(got["first"], o["first_rows"].astype(np.int64)), (what, r, "global first rows")
            for i, col in enumerate(keys):
                assert np.array_equal(got["keys"][i], col[o["first_rows"]]), (what, r, "key column", i)
            for j, op in enumerate(ops):
                key = (id(x), op)
                if key not in stats:
                    st = stats.get((id(x), None))
                    if st is None and x.dtype.kind == "f":
                        st = stats[(id(x), None)] = gc.group_stats(x, o)
                    if st is not None and op == gc.STDDEV:
                        st["oracle_var"] = oracle.grouped_reduce(gc.VAR, x, o)
                    stats[key] = (oracle.grouped_reduce(op, x, o), st)
                want, st = stats[key]
                share = min(share, gc.compare(op, x, got["res"][j], want, o, f"{what} rank {r} [{c}.{j}] {ex.nm(x.dtype)}", st))
                if x.dtype.kind == "f" and op in (gc.SUM, gc.AVG):
                    ratios.note(f"{gc.RED_NAME[op]}({x.dtype.name})", gc.fp_sum_ratio(op, got["res"][j], want, st))
    assert share >= 0.9


def groupby_calls(lay, dtypes, sets, max_cols, minmax_apart):
    calls = []
    for cname, x, ops in gc.columns(lay, dtypes, seed=lay.G, sets=sets):
        calls += [(tuple(call), x) for call in sc.pack_exchange_calls(ops, x.dtype, max_cols, minmax_apart)]
    return calls


ALL_SETS = ("int_full", "carry", "narrow_at_end", "fp_finite", "fp_inf", "fp_nan")


def run_groupby(oracle, G, key_of, cut, gmax, hint, dtypes=gc.ALL_DT, max_cols=6, small=False, what=""):
    """every value set under the layout of ~G groups; the carry sets under the layouts whose reserved groups hold the avg probes.  small: the test is
    about the one-launch merge -- MIN / MAX of a floating column go into a call of their own, and every other call must meet the condition of
    csrc/exchange.hip for that merge (sharded_cases.takes_small_merge); not small: no call may meet it"""
    lays = {None: sc.groupby_layout(G), sc.I64: sc.groupby_carry_layout(G, "int64"), sc.U64: sc.groupby_carry_layout(G, "uint64")}
    ncalls, on_small, ratios = 0, 0, Ratios()
    for which, lay in lays.items():
        if which is not None and which not in [np.dtype(t) for t in dtypes]:
            continue
        keys = key_of(lay.labels)
        o = oracle.groupby(keys)
        assert o["counts"].max() == lay.n // 3 and np.count_nonzero(o["counts"] == 1) >= 50
        sh = sc.groupby_cuts(lay)[cut]
        sets = tuple(s for s in ALL_SETS if s != "carry") if which is None else ("carry",)
        calls = groupby_calls(lay, dtypes if which is None else [which], sets, max_cols, small)
        for ops, x in calls:
            fp_minmax = x.dtype.kind == "f" and any(op in (gc.MIN, gc.MAX) for op in ops)
            takes = sc.takes_small_merge(ops, x.dtype, len(keys), gmax, len(sh), keys[0].dtype)
            assert takes == (small and not fp_minmax), (what, cut, ex.nm(x.dtype), [gc.RED_NAME[op] for op in ops])
            on_small += takes
        if small:                                            # floating sums, counts and means of both widths are among the calls of the one-launch merge
            for dt in ex.FP_DTYPES:
                assert any(x.dtype == dt and {gc.SUM, gc.COUNT, gc.AVG} <= set(ops) and sc.takes_small_merge(ops, dt, 1, gmax, len(sh)) for ops, x in calls) or which is not None
        if gmax:
            assert max(oracle.groupby([c[lo:hi] for c in keys])["ngroups"] for lo, hi in sh if hi > lo) <= gmax
        check_groupby(oracle, o, keys, calls, groupby_over(sh, keys, calls, gmax, hint), f"{what} {cut}", ratios)
        ncalls += len(calls)
    print(f"{what} {cut}: {ncalls} calls, {on_small} of them by the condition of the one-launch merge", flush=True)
    ratios.show(f"{what} {cut}")


GROUPBY_CUTS = ("even3", "tiny_middle", "empty_rank", "split")


@pytest.mark.parametrize("cut", GROUPBY_CUTS)
def test_group_by_through_the_one_launch_merge(oracle, cut):
    """one int32 key, three ranks, gmax = 341 (3 * 341 <= 1024), about 300 groups, at most six payload columns a call: the condition of
    xmerge_small_kernel (module docstring), asserted for every call.  MIN / MAX of a floating column -- which send a whole call through the
    concatenation -- go into a call of their own, so SUM / COUNT / AVG of float32 and float64 columns (finite, +-Inf groups, NaN groups beside
    tame ones) and the sums, squares and counts of VAR / STDDEV meet the kernel's double atomic add"""
    run_groupby(oracle, 300, gc.k_i32, cut, sc.GMAX_SMALL, 341, small=True, what="one-launch merge")


@pytest.mark.parametrize("cut", GROUPBY_CUTS)
def test_group_by_through_the_concatenation_gmax_0(oracle, cut):
    """the same shapes with gmax = 0: the group counts are exchanged first, the shard tables concatenated and re-aggregated"""
    run_groupby(oracle, 300, gc.k_i32, cut, 0, 341, max_cols=8, what="concatenation, gmax 0")


@pytest.mark.parametrize("cut", GROUPBY_CUTS)
def test_group_by_two_key_columns(oracle, cut):
    run_groupby(oracle, 300, gc.k_2xi32, cut, sc.GMAX_SMALL, 341, dtypes=[np.int16, np.uint32, np.int64, np.uint64, np.float32, np.float64], max_cols=8, what="two keys")


@pytest.mark.parametrize("cut", GROUPBY_CUTS)
def test_group_by_more_groups_than_the_one_launch_merge_holds(oracle, cut):
    """about 5000 groups (above XS_ROWS): gmax is a bound on the shard tables only"""
    run_groupby(oracle, 5000, gc.k_i32, cut, 5200, 5200, dtypes=[np.int8, np.uint16, np.int32, np.int64, np.uint64, np.float32, np.float64], max_cols=8, what="5000 groups")
