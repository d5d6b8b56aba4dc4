"""The scratch-memory catalogue: one small call per entry of include/aqg.h and per route / plan, run by tests/scratch_child.py in a
process of its own -- unguarded, and under AQG_WS_GUARD = 0x00, 0xFF, 0xA5 (tests/test_gpu_scratch_guard.py; DESIGN.md "Scratch
memory").  Every call is built from the family's case module and checked by the helper the family's own test file uses, or -- where
no case module exists -- on the sizes the family's test names, against the oracle.  A call names the entries it drives and the
route / plan bits it expects; tests/test_scratch_catalogue.py holds the list to the header without a GPU.

A call is `fn(env)`: env.dev is a fresh Device whose library handle records every entry called, every status, and every byte
copied back from the device (the digest); env.oracle is the checker.  It may return {"out": [arrays / scalars that came back through
host pointers], "plan": AQG_PLAN_* bits}."""
import numpy as np

from aquery2_amd import capi as P

# ---- what the completeness test subtracts from the header: one reason per name -------------------------------------------------------
EXEMPT = {
    # type rules: pure host functions
    "aqg_dtype_size": "type rule, host only", "aqg_long_type": "type rule, host only", "aqg_fp_type": "type rule, host only",
    "aqg_coercion": "type rule, host only", "aqg_ewise_out_dtype": "type rule, host only", "aqg_reduce_out_dtype": "type rule, host only",
    "aqg_scan_out_dtype": "type rule, host only", "aqg_rank_out_dtype": "type rule, host only", "aqg_rangew_out_dtype": "type rule, host only",
    "aqg_version": "a constant string",
    # context and memory management
    "aqg_device_count": "context management", "aqg_ctx_create": "context management (every call runs it)", "aqg_ctx_destroy": "context management",
    "aqg_last_error": "context management", "aqg_ctx_stream": "context management", "aqg_sync": "context management",
    "aqg_reserve_workspace": "sizes the arena itself; under the guard it would hide an entry's own sizing",
    "aqg_malloc": "user memory, not scratch", "aqg_free": "user memory", "aqg_h2d": "copy", "aqg_d2h": "copy", "aqg_d2d": "copy", "aqg_memset": "fill",
    # column pinning
    "aqg_col_pin": "column pinning: host registration and DMA, no device scratch", "aqg_col_pin_last": "reporter",
    "aqg_col_fetch": "column pinning", "aqg_col_fetch_wait": "column pinning", "aqg_col_unpin": "column pinning", "aqg_col_unpin_all": "column pinning",
    # timers
    "aqg_timer_start": "timer", "aqg_timer_stop_ms": "timer", "aqg_last_kernel_ms": "timer",
    # reporters of the last call and accessors of a handle (read by the child after every call)
    "aqg_sort_last_passes": "reporter", "aqg_select_last_routes": "reporter", "aqg_window_quantiles_last": "reporter", "aqg_rank_last": "reporter",
    "aqg_rangew_last": "reporter", "aqg_distinct_last": "reporter", "aqg_str_encode_last": "reporter", "aqg_join_last": "reporter",
    "aqg_join_asof_last": "reporter", "aqg_join_window_last": "reporter", "aqg_groupby_plan": "reporter",
    "aqg_groupby_destroy": "handle management", "aqg_groupby_ngroups": "handle accessor", "aqg_groupby_nrows": "handle accessor",
    "aqg_groupby_reversemap": "handle accessor", "aqg_groupby_counts": "handle accessor", "aqg_groupby_first_rows": "handle accessor",
    "aqg_groupby_first_rows64": "handle accessor", "aqg_groupby_agg_result": "handle accessor",
    "aqg_join_tuple_slots": "host code, no GPU",
    # RCCL communicators
    "aqg_comm_unique_id": "RCCL communicator", "aqg_comm_init_rccl": "RCCL communicator", "aqg_comm_init_custom": "communicator set-up (the sharded calls run over it)",
    "aqg_comm_destroy": "communicator", "aqg_comm_rank": "communicator", "aqg_comm_world": "communicator",
    # the guard's own hooks
    "aqg_debug_ws_check": "test aid", "aqg_debug_ws_info": "test aid",
}

# route / plan bits nothing in the catalogue can reach, with the reason
UNREACHABLE = {
    ("str", P.STR_ROUTE_HOST): "AQG_STR_HOST is an env switch and the host map uses no device scratch (below 2^16 rows the default route, reported but not required)",
}

# the switch sets of tests/test_gpu_plans.py: plans the default thresholds do not reach run in children of their own (pattern 0xA5 only)
SWITCH_SETS = {
    "": {},
    "p1_max": {"AQG_P1_MAX": "1"},
    "no_p1": {"AQG_DISABLE_P1": "1"},
    "sorted_tail": {"AQG_SORTED_TAIL_MIN": "1"},
    "no_pw_defer": {"AQG_DISABLE_PW_DEFER": "1"},
    "no_build_partition": {"AQG_DISABLE_BUILD_PARTITION": "1"},
}

SORT_SMALL, SORT_CHUNK = 4096, 131072          # sort.hip SMALL / CHUNK (tests/test_gpu_sort.py)
SCAN_TILE = 2048                               # scan_dev.hpp: rows per tile


class Call:
    def __init__(self, name, entries, fn, expect=None, switches="", family="misc", d2h=True):
        self.name, self.entries, self.fn, self.expect, self.switches, self.family = name, tuple(entries), fn, dict(expect or {}), switches, family
        self.d2h = d2h          # False: the binding copies back more than the entry wrote (never-written user memory); only what the call returns is digested


CALLS = []


def call(name, entries, expect=None, switches="", family="misc", d2h=True):
    def deco(fn):
        CALLS.append(Call(name, entries, fn, expect, switches, family, d2h=d2h))
        return fn
    return deco


def rng(seed):
    return np.random.default_rng(seed)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- element-wise, reductions, scans, gather / filter: the sizes of tests/test_gpu_basic.py and the scan tile ------------------------------
N_EW = 3 * SCAN_TILE + 5


@call("ewise", ["aqg_ewise", "aqg_unary", "aqg_gen_column"], family="basic")
def _ewise(env):
    import checker as ck
    d, o = env.dev, env.oracle
    r = rng(1)
    a, b = r.integers(-1000, 1000, N_EW).astype(np.int32), r.integers(1, 99, N_EW).astype(np.int32)
    for op in (ck.OP_ADD, ck.OP_MUL, ck.OP_DIV, ck.OP_LT):
        assert same(d.ewise(op, a, b), o.ewise(op, a, b)), op
    assert same(d.ewise(ck.OP_SUB, a, np.int32(7)), o.ewise(ck.OP_SUB, a, np.int32(7)))
    x = r.integers(0, 10 ** 6, N_EW).astype(np.int64)
    assert same(d.unary(0, x), o.unary(0, x))
    g = d.gen_column(ck.GEN_V1, 42, 0, N_EW, N_EW, 100).to_host()
    assert same(g, o.gen_column(ck.GEN_V1, 42, 0, N_EW, N_EW, 100))


@call("reduce", ["aqg_reduce", "aqg_reduce_dev", "aqg_corr"], family="basic")
def _reduce(env):
    import ctypes as C
    import checker as ck
    d, o = env.dev, env.oracle
    r = rng(2)
    outs = []
    for dt in (np.int32, np.float64, np.int8):
        x = (r.normal(size=N_EW) * 100).astype(dt)
        for name in ("sum", "min", "max", "count", "avg", "var", "stddev", "first", "last"):
            got, want = d.reduce(ck.RED_NAMES[name], x), o.reduce(ck.RED_NAMES[name], x)
            if np.dtype(dt).kind == "f" and name in ("sum", "avg", "var", "stddev"):
                assert abs(float(got) - float(want)) <= 1e-9 * max(1.0, abs(float(want))), (dt, name, got, want)
            else:
                assert got == want, (dt, name, got, want)
            outs.append(np.float64(got) if isinstance(got, (float, np.floating)) else str(got))
    x = r.integers(-10 ** 6, 10 ** 6, N_EW).astype(np.int32)
    xd, out = d.to_device(x), d.empty(2, np.uint64)
    d._chk(d.lib.aqg_reduce_dev(d.ctx, ck.RED_SUM, xd.tag, C.c_void_p(xd.ptr), C.c_uint32(xd.n), C.c_void_p(out.ptr)), "aqg_reduce_dev")
    d.sync()
    assert int(out.to_host()[0].astype(np.int64)) == int(x.astype(np.int64).sum())
    y = (x * 3 + r.integers(-5, 5, N_EW)).astype(np.int32)
    got, want = d.corr(x, y), o.corr(x, y)
    assert got == want, (got, want)
    outs.append(np.float64(got))
    return {"out": outs}


@call("scan_at_the_tile", ["aqg_scan", "aqg_scan_resume"], family="basic")
def _scan(env):
    import checker as ck
    d, o = env.dev, env.oracle
    r = rng(3)
    outs = []
    for n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 3 * SCAN_TILE + 5):
        x = r.integers(-1000, 1000, n).astype(np.int32)
        # the scans the existing tests hold to bit equality on integer columns (sharded_cases.BITWISE_INT) ...
        for name, w in (("sums", 0), ("avgs", 0), ("mins", 0), ("maxs", 0), ("sumw", 100), ("minw", 10), ("maxw", 2500), ("ratiow", 3),
                        ("deltas", 0), ("prev", 0), ("aggnext", 0)):
            op = ck.SCAN_NAMES[name]
            assert same(d.scan(op, x, w), o.scan(op, x, w)), (n, name)
        # ... and the ones they hold to a bound (tests/test_gpu_variance.py, grouped_scan_cases.int_avgw_bad): here for their scratch and digest
        for name, w in (("avgw", 7), ("varw", 40), ("varw", 2500), ("vars", 0)):
            outs.append(d.scan(ck.SCAN_NAMES[name], x, w))
        # avgw against the exact window mean (integer window sums are exact; len = min(w, i + 1)).  Bound: the reference's recurrence
        # avg += (x[i] - x[i-w]) / w makes three roundings a row, each at most 2^-53 of an operand below 2 max|x| = 2000, over at most n
        # rows: 3 n 2000 2^-53.  A direct sum / len is one rounding and far inside it.
        cs = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
        i = np.arange(n)
        lo = np.maximum(i - 6, 0)
        exact = (cs[i + 1] - cs[lo]) / (i + 1 - lo)
        assert outs[-4].dtype == np.float64 and np.all(np.abs(outs[-4] - exact) <= 3 * n * 2000 * 2.0 ** -53), (n, "avgw")
    x = r.integers(-1000, 1000, 2 * SCAN_TILE + 3).astype(np.int64)
    whole, cut = o.scan(ck.SCAN_NAMES["sums"], x, 0), SCAN_TILE + 1
    got = d.scan_resume(ck.SCAN_NAMES["sums"], x[cut:], int(x[:cut].sum()), cut)
    assert same(got, whole[cut:])
    return {"out": outs}


@call("gather_compact_around_a_tile", ["aqg_gather", "aqg_gather_fill", "aqg_compact", "aqg_mask_to_index"], family="basic", d2h=False)
def _gather(env):
    """(Device.compact / mask_to_index copy the whole n-element output buffer back and cut it at m: the rows behind m are user memory that
    nothing wrote, so the digest is taken over the returned arrays)"""
    d, o = env.dev, env.oracle
    r = rng(4)
    outs = []
    for n in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 5 * SCAN_TILE + 77):
        x = r.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)
        mask = r.random(n) < 0.4
        idx = r.integers(0, n, n // 2).astype(np.uint32)
        got = [d.compact(x, mask), d.mask_to_index(mask), d.gather(x, idx)]
        assert same(got[0], x[mask]) and same(got[1], np.flatnonzero(mask).astype(np.uint32)) and same(got[2], o.gather(x, idx)), n
        idx[::5] = 0xFFFFFFFF
        want = np.where(idx == 0xFFFFFFFF, np.int64(-7), x[np.minimum(idx, n - 1)])
        got.append(d.gather_fill(x, idx, np.int64(-7)))
        assert same(got[3], want), n
        outs += got
    return {"out": outs}


# ---- sort: SMALL +- 1 and CHUNK + 1, digit passes 0 / 1 / more on both paths ---------------------------------------------------------------
def _sort_one(env, n, kind):
    import test_gpu_sort as ts
    d = env.dev
    r = rng(5 + n)
    if kind == 0:
        keys = [np.full(n, 7, np.int32)]                       # one value: every digit pass is skipped
    elif kind == 1:
        keys = [r.integers(0, 200, n).astype(np.int32)]         # one byte varies
    else:
        keys = [r.integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32), r.normal(size=n).astype(np.float32)]
    orders = [P.ORDER_ASC, P.ORDER_DESC][:len(keys)]
    got = d.sort_rows(keys, orders)
    passes = d.sort_last_passes()
    assert same(got, ts.want_order(keys, orders).astype(np.uint32)), (n, kind)
    assert (passes == 0, passes == 1, passes > 1)[kind], (n, kind, passes)


for _n in (SORT_SMALL - 1, SORT_SMALL, SORT_SMALL + 1, SORT_CHUNK + 1):
    for _k in (0, 1, 2):
        call("sort_n%d_passes%s" % (_n, ("0", "1", "many")[_k]), ["aqg_sort_rows"],
             expect={"sort": ["%s:%d" % ("wg" if _n <= SORT_SMALL else "multi", _k)]}, family="sort")(lambda env, n=_n, k=_k: _sort_one(env, n, k))


# ---- ranking -----------------------------------------------------------------------------------------------------------------------------
def _smallest(cases, pred):
    ok = [c for c in cases if pred(c)]
    assert ok
    return min(ok, key=lambda c: len(c.x))


@call("rank_flat_small", ["aqg_rank"], expect={"rank": P.RANK_ROUTE_SMALL}, family="rank")
def _rank_small(env):
    import rank_cases as rc
    import test_gpu_rank as tr
    c = _smallest(rc.flat_cases(), lambda c: 1 < len(c.x) <= rc.SMALL_MAX and c.dtype == np.dtype(np.float64))
    assert tr.hold_case(env.dev, c) == P.RANK_ROUTE_SMALL


@call("rank_flat_sorted", ["aqg_rank"], expect={"rank": P.RANK_ROUTE_SORTED}, family="rank")
def _rank_sorted(env):
    import rank_cases as rc
    import test_gpu_rank as tr
    c = _smallest(rc.flat_cases(), lambda c: len(c.x) > rc.SMALL_MAX and c.dtype == np.dtype(np.int32))
    assert tr.hold_case(env.dev, c) == P.RANK_ROUTE_SORTED


@call("rank_grouped_mixed", ["aqg_grouped_rank", "aqg_grouped_rank_flat", "aqg_groupby_build"], expect={"rank": P.RANK_ROUTE_SMALL | P.RANK_ROUTE_SORTED}, family="rank")
def _rank_grouped(env):
    import rank_cases as rc
    import test_gpu_rank as tr
    c = _smallest(rc.grouped_cases(), lambda c: c.name.split("-")[1] == "mixed")
    gb = env.dev.groupby_build([c.keys_row])
    assert tr.hold_case(env.dev, c, gb) == tr.expected_routes(c) == P.RANK_ROUTE_SMALL | P.RANK_ROUTE_SORTED
    return {"plan": gb.plan}


# ---- exponential moving averages ---------------------------------------------------------------------------------------------------------
@call("ema_flat", ["aqg_scan_ema", "aqg_decay_from_times"], family="ema")
def _ema_flat(env):
    import ema_cases as ec
    import test_gpu_ema as te
    flat = ec.flat_cases()
    big = max(len(c.x) for c in flat)
    for pick in (lambda c: c.decay is None, lambda c: c.decay is not None):
        c = _smallest(flat, lambda c: pick(c) and len(c.x) == big)
        te.hold(te.run_case(env.dev, c)["flat"], ec.reference(c), c.mode, c.name)
    t = np.cumsum(rng(6).integers(0, 50, 3 * SCAN_TILE + 1)).astype(np.int64)
    got = env.dev.decay_from_times(t, 10.0)
    te.hold_decay(got, te.decay_exact([int(v) for v in t], 10.0), "decay_from_times")


@call("ema_grouped", ["aqg_grouped_ema", "aqg_grouped_ema_flat", "aqg_grouped_decay_from_times_flat", "aqg_groupby_build"], family="ema")
def _ema_grouped(env):
    import ema_cases as ec
    import test_gpu_ema as te
    grouped = ec.grouped_cases()
    for pick in (lambda c: c.decay is None, lambda c: c.decay is not None):
        c = _smallest(grouped, lambda c: pick(c) and len(c.starts) > 2 and len(c.x) > 2 * SCAN_TILE)
        gb = env.dev.groupby_build([c.keys_row])
        ref = ec.reference(c)
        for entry, got in te.run_case(env.dev, c, gb).items():
            te.hold(got, ref, c.mode, c.name + "/" + entry)
    t = np.cumsum(rng(7).integers(0, 50, len(c.x))).astype(np.int64)
    got = env.dev.decay_from_times(t, 10.0, gb=gb)
    want = te.decay_exact([int(v) for v in t], 10.0)
    for s_ in c.starts:
        want[int(s_)] = want[0]
    te.hold_decay(got, want, "grouped_decay_from_times_flat")
    return {"plan": gb.plan}


# ---- time-range windows ------------------------------------------------------------------------------------------------------------------
@call("rangew_flat", ["aqg_rangew_bounds", "aqg_rangew_fold", "aqg_rangew"], family="timewin")
def _rangew_flat(env):
    import timewin_cases as tc
    import test_gpu_timewin as tt
    flat = tc.flat_cases()
    rx, tile = tc.geometry()
    for kind in ("i", "f"):
        c = _smallest(flat, lambda c: len(c.x) > tile and np.asarray(c.x).dtype.kind == kind)
        tt.run_flat(env.dev, c)


@call("rangew_grouped", ["aqg_grouped_rangew_bounds_flat", "aqg_grouped_rangew", "aqg_grouped_rangew_flat", "aqg_rangew_fold", "aqg_groupby_build"], family="timewin")
def _rangew_grouped(env):
    import timewin_cases as tc
    import test_gpu_timewin as tt
    d = env.dev
    c = min(tc.grouped_cases(), key=lambda c: (len(c.starts) < 3, c.n))
    lo, w = tc.reference(c)
    keys, t_row, x_row = c.rows()
    gb = d.groupby_build([keys])
    td, xd = d.to_device(c.t), d.to_device(c.x)
    lod = d.rangew_bounds(td, c.span, c.frame, gb=gb, keep=True)
    assert np.array_equal(lod.to_host(), lo), c.name
    for op in tt.OPS:
        forms = {"row": d.grouped_rangew(gb, op, t_row, c.span, None if op == P.RANGEW_COUNT else x_row, c.frame),
                 "flat": d.grouped_rangew(gb, op, td, c.span, None if op == P.RANGEW_COUNT else xd, c.frame, flat=True),
                 "bounds+fold": d.rangew_fold(op, None if op == P.RANGEW_COUNT else xd, lod)}
        for k, got in forms.items():
            tt.hold(c, w, op, got, "%s/%s/op%d" % (c.name, k, op))
    return {"plan": gb.plan}


# ---- window join, as-of join --------------------------------------------------------------------------------------------------------------
def _wj(env, name, flags=0):
    import wj_cases
    import test_gpu_wj as tw
    tw.run_case(env.dev, wj_cases.cases()[name], flags, (name, flags))


def _asof(env, name):
    import asof_cases
    import test_gpu_asof as ta
    bk, bo, pk, po, routes = asof_cases.cases()[name]
    for d_, s in ta.MODES:
        rc_, got, intact = ta.asof_raw(env.dev, bk, bo, pk, po, d_, ta.STRICT if s else 0)
        assert rc_ == 0 and intact
        assert np.array_equal(got, ta.want_of(name, d_, s)), (name, d_, s)
        assert env.dev.join_asof_last()[0] == routes
    return routes


def _asof_and_wj_calls():
    """one as-of and one window-join call per route mask the case tables reach, the smallest case of each"""
    import asof_cases
    import asof_model as am
    import wj_cases
    import wj_model as wm
    by_route = {}
    for name, (bk, bo, pk, po, routes) in sorted(asof_cases.cases().items()):
        if routes and (routes not in by_route or len(bo) + len(po) < by_route[routes][1]):
            by_route[routes] = (name, len(bo) + len(po))
    for routes, (name, _) in sorted(by_route.items()):
        call("asof_%s" % name, ["aqg_join_asof"], expect={"asof": routes}, family="asof")(lambda env, name=name: _asof(env, name) and None)
    seen = {}
    for name, c in sorted(wj_cases.cases().items()):
        r = wm.routes(c.bk, c.bo, len(c.po))
        if len(c.bo) == 0 or len(c.po) == 0:
            continue
        fr = wm.fold_route((np.asarray(c.x).dtype.itemsize, wm.acc_bytes(np.asarray(c.x).dtype, wm.SUM)), len(c.bo), len(c.po))
        key = (r, fr)
        if key not in seen or len(c.bo) + len(c.po) < seen[key][1]:
            seen[key] = (name, len(c.bo) + len(c.po))
    for (r, fr), (name, _) in sorted(seen.items()):
        call("wj_%s" % name, ["aqg_join_window_bounds", "aqg_join_window", "aqg_interval_fold", "aqg_gather"], expect={"wj": r | fr}, family="wj")(
            lambda env, name=name: _wj(env, name))
    for name, f in sorted(wj_cases.folds().items()):
        fr = wm.fold_route((f.x.dtype.itemsize, wm.acc_bytes(f.x.dtype, wm.SUM)), len(f.x), len(f.lo))
        if ("fold", fr) in seen:
            continue
        seen[("fold", fr)] = name
        call("interval_fold_%s" % name, ["aqg_interval_fold"], expect={"wj": fr}, family="wj")(lambda env, name=name: _fold(env, name))


def _fold(env, name):
    import wj_cases
    import wj_model as wm
    import test_gpu_wj as tw
    f = wj_cases.folds()[name]
    ref = wm.interval_windows(f.x, f.lo, f.hi)
    for op in tw.OPS:
        rc_, got, intact = tw.fold_raw(env.dev, op, f.x, f.lo, f.hi)
        assert rc_ == 0 and intact, (name, op)
        tw.hold(f.x, ref, op, got, tw.FILL, "fold/%s/op%d" % (name, op))


_asof_and_wj_calls()


# ---- the radix selections: median, top-k, quantiles, moving quantiles, count distinct ------------------------------------------------------
def _selection(env, pick):
    """the shapes of selection_family_cases through the three families, as tests/test_gpu_selection_family.py's child does"""
    import selection_family_cases as sf
    d = env.dev
    done = 0
    for name, dt, counts, x in sf.generate():
        if not pick(name, dt, counts):
            continue
        gb = d.groupby_build([sf.keys_of(counts)])
        xd = d.to_device(x)
        x_row = x                                                  # (sorted keys: the flat layout is the column)
        for (what, arg), answers in sf.models(x, counts).items():
            if what == "median":
                got = {"quantiles": d.grouped_quantiles(gb, xd, [1], 2, arg, flat=True)[:, 0], "median": d.grouped_median(gb, xd, arg, flat=True)}
            else:
                got = {"quantiles": d.grouped_quantiles(gb, xd, [0 if what == "min" else 1], 1, flat=True)[:, 0], "topk": d.grouped_topk(gb, xd, 1, arg, flat=True)[:, 0]}
            for family, (want, flags) in answers.items():
                assert got[family].tobytes() == want.tobytes(), (name, str(dt), what, arg, family)
        done += 1
        gb.destroy()
    assert done
    return None


@call("selection_flat_layout", ["aqg_grouped_median_flat", "aqg_grouped_topk_flat", "aqg_grouped_quantiles_flat", "aqg_groupby_build"],
      expect={"select": P.ROUTE_SMALL | P.ROUTE_GROUP}, family="select")
def _sel_flat(env):
    return _selection(env, lambda name, dt, counts: np.dtype(dt) in (np.dtype(np.int64), np.dtype(np.float32)))


@call("selection_row_layout_and_flat_column", ["aqg_median", "aqg_topk", "aqg_quantiles", "aqg_grouped_median", "aqg_grouped_topk", "aqg_grouped_quantiles",
                                               "aqg_groupby_build"], expect={"select": P.ROUTE_SMALL | P.ROUTE_GROUP}, family="select")
def _sel_row(env):
    d = env.dev
    r = rng(8)
    n = 3 * 4096 + 17
    x = r.integers(-500, 500, n).astype(np.int32)
    keys = np.concatenate([np.repeat(np.arange(40, dtype=np.int32), 100), np.full(n - 4000, 40, np.int32)])      # 40 SMALL groups and one long one
    r.shuffle(keys)
    gb = d.groupby_build([keys])
    off, rows = gb.postproc()
    G = gb.ngroups
    outs = []
    med = d.grouped_median(gb, x)
    top = d.grouped_topk(gb, x, 3)
    qs = d.grouped_quantiles(gb, x, [0, 1, 2, 4], 4)
    routes = d.select_last_routes()[0]
    for g in range(G):
        s = np.sort(x[rows[off[g]:off[g + 1]]])
        c = len(s)
        assert med[g] == s[(c - 1) // 2], g
        assert top[g].tolist() == s[::-1][:3].tolist(), g
        assert qs[g].tolist() == [s[0], s[(c - 1) // 4], s[(c - 1) // 2], s[-1]], g
    s = np.sort(x)
    m = d.median(x)
    assert m == s[(n - 1) // 2]
    t = d.topk(x, 5)
    assert np.asarray(t).tolist() == s[::-1][:5].tolist()
    q = d.quantiles(x, [0, 1, 2], 2)
    assert np.asarray(q).tolist() == [s[0], s[(n - 1) // 2], s[-1]]
    outs += [np.asarray(m), np.asarray(t), np.asarray(q)]
    return {"out": outs, "plan": gb.plan}


@call("selection_split", ["aqg_grouped_median_flat", "aqg_median", "aqg_groupby_build"], expect={"select": P.ROUTE_SPLIT}, family="select")
def _sel_split(env):
    """one group of 2^20 + 3 rows: the SPLIT route's own threshold (AQG_SELECT_SPLIT_MIN = 2^20), the smallest shape that takes it"""
    d = env.dev
    n = (1 << 20) + 3
    x = rng(9).integers(-10 ** 6, 10 ** 6, n).astype(np.int32)
    gb = d.groupby_build([np.zeros(n, np.int32)])
    got = d.grouped_median(gb, x[::-1].copy(), flat=True)
    assert d.select_last_routes()[0] & P.ROUTE_SPLIT
    s = np.sort(x)
    assert got[0] == s[(n - 1) // 2]
    m = d.median(x)
    assert m == s[(n - 1) // 2]
    return {"out": [np.asarray(m)], "plan": gb.plan}


@call("window_quantiles", ["aqg_window_quantiles", "aqg_grouped_window_quantiles", "aqg_grouped_window_quantiles_flat", "aqg_groupby_build"], family="select")
def _winq(env):
    d = env.dev
    r = rng(10)
    n, w = 2 * 4096 + 9, 21
    x = r.integers(-100, 100, n).astype(np.int32)

    def model(col, starts):
        out = np.empty((2, len(col)), col.dtype)
        edges = list(starts) + [len(col)]
        for a, b in zip(edges[:-1], edges[1:]):
            for i in range(a, b):
                s = np.sort(col[max(a, i - w + 1):i + 1])
                out[0, i], out[1, i] = s[(len(s) - 1) // 2], s[-1]
        return out
    got = d.window_quantiles(x, [1, 2], 2, w)
    assert same(np.asarray(got).reshape(2, n), model(x, [0]))
    keys = np.repeat(np.arange(5, dtype=np.int32), -(-n // 5))[:n]
    gb = d.groupby_build([keys])
    off, rows = gb.postproc()
    want = model(x[rows], off[:-1])
    assert same(np.asarray(d.grouped_window_quantiles(gb, x, [1, 2], 2, w)).reshape(2, n), want)
    assert same(np.asarray(d.grouped_window_quantiles(gb, x[rows], [1, 2], 2, w, flat=True)).reshape(2, n), want)
    return {"plan": gb.plan}


@call("count_distinct", ["aqg_count_distinct", "aqg_grouped_count_distinct", "aqg_grouped_count_distinct_flat", "aqg_groupby_build", "aqg_groupby_postproc"], family="select")
def _distinct(env):
    d = env.dev
    r = rng(11)
    n = 5 * 4096 + 3
    x = r.integers(0, 300, n).astype(np.int32)
    keys = r.integers(0, 7, n).astype(np.int32)                  # seven long groups: every one crosses tile edges and leaves pairs
    gb = d.groupby_build([keys])
    off, rows = gb.postproc()
    want = np.array([len(np.unique(x[rows[off[g]:off[g + 1]]])) for g in range(gb.ngroups)], np.uint32)
    assert same(d.grouped_count_distinct(gb, x), want)
    assert same(d.grouped_count_distinct(gb, x[rows], layout="flat"), want)
    c = d.count_distinct(x)
    assert c == len(np.unique(x))
    return {"out": [np.uint32(c)], "plan": gb.plan}


# ---- strings --------------------------------------------------------------------------------------------------------------------------
def _str(env, name, n, route):
    import strdict_cases as sc
    import strdict_model as sm
    import test_gpu_strdict as tsd
    case = sc.case(name, n)
    col = tsd.Column(case.pool, case.idx)
    want, want_nd, _ = sm.codes(col.strs)
    out, nd, last = tsd.encode(env.dev, col)
    assert np.array_equal(out.to_host(), want) and nd == want_nd
    assert last == sm.expected_route(n, case.collides) and last[0] & route, (last, route)
    return {"out": [np.uint32(nd)]}


@call("str_encode_device", ["aqg_str_encode"], expect={"str": P.STR_ROUTE_DEVICE}, family="str")
def _str_device(env):
    return _str(env, "word_edges", 65_536, P.STR_ROUTE_DEVICE)


@call("str_encode_fallback", ["aqg_str_encode"], expect={"str": P.STR_ROUTE_FALLBACK}, family="str")
def _str_fallback(env):
    import strdict_cases as sc
    name = next(c.name for c in sc.cases(sc.MIN_ROWS) if c.collides)
    return _str(env, name, 65_536, P.STR_ROUTE_FALLBACK)


# ---- joins ----------------------------------------------------------------------------------------------------------------------------
@call("join_single_key", ["aqg_join_count", "aqg_join_pairs", "aqg_join_lookup"], family="join")
def _join1(env):
    d, o = env.dev, env.oracle
    r = rng(12)
    build = r.permutation(40_003).astype(np.int32)[:5000]
    probe = r.integers(0, 40_003, 9001).astype(np.int32)
    pr, br = d.join_pairs(build, probe)
    wp, wb = o.join_pairs(build, probe)
    order = np.lexsort((br, pr))
    worder = np.lexsort((wb, wp))
    assert np.array_equal(pr[order], wp[worder]) and np.array_equal(br[order], wb[worder])
    cnt = d.join_count(build, probe)
    assert cnt == len(wp)
    look = d.join_lookup(build, probe)
    pos = {int(v): i for i, v in enumerate(build)}
    assert look.tolist() == [pos.get(int(v), 0xFFFFFFFF) for v in probe]
    return {"out": [np.uint64(cnt)]}


def _join_keys(env, spec, nb, npr, want):
    import test_gpu_join_keys as tj
    build, probe = tj.sides(rng(71), tj.SPECS[spec][0], nb, npr)
    r = tj.check_all(env.dev, build, probe)
    assert r == want, (r, want)


for _spec, _npr, _bits in (("i32_i32", 70_001, P.JOIN_ROUTE_PACKED | P.JOIN_ROUTE_LDS), ("i32_i32", 5000, P.JOIN_ROUTE_PACKED | P.JOIN_ROUTE_HBM),
                           ("i64_i32", 70_001, P.JOIN_ROUTE_WIDE | P.JOIN_ROUTE_LDS), ("i64_i32", 5000, P.JOIN_ROUTE_WIDE | P.JOIN_ROUTE_HBM)):
    call("join_keys_%s_npr%d" % (_spec, _npr), ["aqg_join_keys_count", "aqg_join_keys_pairs", "aqg_join_keys_lookup"], expect={"join": _bits}, family="join")(
        lambda env, spec=_spec, npr=_npr, bits=_bits: _join_keys(env, spec, 1000, npr, bits))


def _star(env, nb):
    """the fused star join + group-by at 40 003 fact rows, as tests/test_gpu_configs.py models it: look-up, unmatched rows dropped, exact
    products, sums in first-occurrence order among the joined rows"""
    import checker as ck
    d = env.dev
    r = rng(13 + nb)
    n = 40_003
    fk = r.integers(0, nb + 20, n).astype(np.int32)               # some keys have no partner
    gkey = r.integers(-40, 40, n).astype(np.int32)
    val = r.integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32)
    dim_key = r.permutation(np.arange(0, nb, dtype=np.int32))
    dim_w = r.integers(-8, 7, nb).astype(np.int32)
    gb = d.join_groupby_sum(dim_key, dim_w, fk, gkey, val)
    first = {}
    for row, k in enumerate(dim_key.tolist()):
        first.setdefault(k, row)
    look = np.array([first.get(k, -1) for k in fk.tolist()], dtype=np.int64)
    rows = np.nonzero(look >= 0)[0]
    order, sums = {}, []
    for i in rows.tolist():
        g = int(gkey[i])
        if g not in order:
            order[g] = len(order)
            sums.append(0)
        sums[order[g]] += int(val[i]) * int(dim_w[look[i]])
    assert gb.ngroups == len(order)
    assert gb.keys(0, np.int32).tolist() == list(order)
    assert ck.i128_to_int(gb.result(0, ck.RED_SUM, ck.INT64)) == sums
    return {"plan": gb.plan}


for _nb in (8, 4096):
    call("star_join_nb%d" % _nb, ["aqg_join_groupby_sum", "aqg_groupby_keys"], family="join")(lambda env, nb=_nb: _star(env, nb))


# ---- group-by: every plan ----------------------------------------------------------------------------------------------------------------
def _agg(env, n, G, keyfn, hint, bits, forbid=0, dts=(np.int32, np.float64), seed=0, ops=None, narrow=False):
    import checker as ck
    import groupagg_cases as gc
    r = rng(100 + seed)
    labels = r.integers(0, G, n).astype(np.int64)
    labels[:G] = np.arange(G)
    keys = keyfn(labels)
    o = env.oracle.groupby(keys)
    plan = 0
    for dt in dts:
        x = (r.integers(0, 200, n) + (2 ** 31 - 300 if narrow else -100)).astype(dt)      # narrow: a narrow range at the top of int32 (the packed-values field)
        for call_ops in (ops or ([gc.SUM, gc.MIN, gc.MAX], [gc.COUNT, gc.AVG])):
            plan |= gc.check(env.dev, env.oracle, keys, list(call_ops), [x] * len(call_ops), hint, bits, forbid, "catalogue", ogb=o)
    return {"plan": plan}


def _plans():
    import groupagg_cases as gc
    A = ["aqg_groupby_agg", "aqg_groupby_keys"]
    # the LDS plans: the shapes of groupagg_cases.PLANS at a tenth of their rows (the planner looks at hint and key shape, not at n, here)
    call("agg_fast_lds", A, expect={"plan": P.PLAN_FAST_LDS}, family="agg")(lambda env: _agg(env, 20_003, 100, gc.k_i32, 100, P.PLAN_FAST_LDS))
    call("agg_small_lds", A, expect={"plan": P.PLAN_SMALL_LDS}, family="agg")(lambda env: _agg(env, 20_003, 100, gc.k_i16, 100, P.PLAN_SMALL_LDS))
    call("agg_hbm_table", A, expect={"plan": P.PLAN_HBM_TABLE}, family="agg")(lambda env: _agg(env, 60_003, 20_000, gc.k_i32, 20_000, P.PLAN_HBM_TABLE))
    # The partition plans, DENSE and BIG_LDS.  make_agg_plan (groupby.hip) takes none of them below 2^20 rows (`n >= (1u << 20)` in plan_dense's
    # and the big table's conditions, in use_part, use_wpart, build_part),
    # and ROW_EMIT needs a partition plan with G == n: N20 is the smallest n that reaches them.  The planner's sampled key ranges
    # (RANGE_PARTITIONS, PACKED_VALUES), the look-up build (BUILD_LOOKUP) and the partition on the group id (GID_PARTITION, grouped_reduce.hip)
    # start at 2^22 rows: N22.  Nothing here copies the multi-million-row sizes of tests/test_gpu_plans.py beyond these two thresholds.
    N20, N22 = (1 << 20) + 7, (1 << 22) + 5
    one = ([gc.SUM, gc.MIN, gc.MAX, gc.COUNT],)
    i32 = (np.int32,)
    call("agg_dense", A, expect={"plan": P.PLAN_DENSE}, family="plans")(lambda env: _agg(env, N20, 8000, gc.k_dense, 8000, P.PLAN_DENSE, dts=i32))
    call("agg_big_lds", A, expect={"plan": P.PLAN_BIG_LDS}, family="plans")(lambda env: _agg(env, N20, 6000, gc.k_strided, 6000, P.PLAN_BIG_LDS, dts=i32))
    call("agg_row_emit", A, expect={"plan": P.PLAN_ROW_EMIT}, family="plans")(
        lambda env: _agg(env, N20, N20, lambda L: [(np.random.default_rng(7).permutation(len(L)) - 500).astype(np.int32)], N20 + 1000, P.PLAN_ROW_EMIT, dts=i32, ops=one))
    call("agg_part_one", A, expect={"plan": P.PLAN_PART_ONE}, family="plans")(
        lambda env: _agg(env, N20, 300_000, gc.k_hashed, 400_000, P.PLAN_PART_ONE, P.PLAN_RANGE_PARTITIONS, dts=i32, ops=one))
    call("agg_part_two", A, expect={"plan": P.PLAN_PART_TWO}, switches="p1_max", family="plans")(
        lambda env: _agg(env, N20, 300_000, gc.k_hashed, 400_000, P.PLAN_PART_TWO, dts=i32, ops=one))
    call("agg_part_round1", A, expect={"plan": P.PLAN_PART_ROUND1}, switches="no_p1", family="plans")(
        lambda env: _agg(env, N20, 300_000, gc.k_hashed, 400_000, P.PLAN_PART_ROUND1, dts=i32, ops=one))
    call("agg_sorted_tail", A, expect={"plan": P.PLAN_PART_ONE | P.PLAN_SORTED_TAIL}, switches="sorted_tail", family="plans")(
        lambda env: _agg(env, N20, 300_000, gc.k_hashed, 400_000, P.PLAN_PART_ONE | P.PLAN_SORTED_TAIL, dts=i32, ops=one))
    # four int32 key columns and a hint above 2^20 (use_wpart: `hint > (1u << 20)`): 1.2e6 tuples need 1.2e6 rows and more
    wide = dict(n=1_500_007, G=1_200_000, keyfn=gc.k_wide, hint=1_300_000, bits=P.PLAN_PART_WIDE, dts=i32, ops=([gc.SUM, gc.MIN, gc.MAX],))
    call("agg_part_wide", A, expect={"plan": P.PLAN_PART_WIDE}, family="plans")(lambda env: _agg(env, **wide))
    # (the tuple is packed into one word from 2^22 rows and three key columns on: partition_wide.hip, `n < (1u << 22) || ks.nkeys < 3`)
    call("agg_part_wide_packed_keys", A, expect={"plan": P.PLAN_PART_WIDE | P.PLAN_PACKED_KEYS}, family="plans_bitmap")(lambda env: _agg(env, **dict(wide, n=N22)))
    call("agg_part_wide_no_defer", A, expect={"plan": P.PLAN_PART_WIDE}, switches="no_pw_defer", family="plans")(lambda env: _agg(env, **wide))
    call("agg_part_one_ranged", A, expect={"plan": P.PLAN_PART_ONE | P.PLAN_RANGE_PARTITIONS}, family="plans_big")(
        lambda env: _agg(env, N22, 400_000, gc.k_dense, 500_000, P.PLAN_PART_ONE | P.PLAN_RANGE_PARTITIONS, dts=i32, ops=one))
    call("agg_packed_values", A, expect={"plan": P.PLAN_PART_TWO | P.PLAN_PACKED_VALUES}, switches="p1_max", family="plans_big")(
        lambda env: _agg(env, N22, 400_000, gc.k_dense, 500_000, P.PLAN_PART_TWO | P.PLAN_PACKED_VALUES, dts=i32, ops=([gc.SUM, gc.MIN, gc.MAX],), narrow=True))

    def build(env, n, G, want, reduce_plan=0):
        import checker as ck
        r = rng(200 + n % 97)
        labels = r.integers(0, G, n).astype(np.int64)
        labels[:G] = np.arange(G)
        key = gc.k_dense(labels) if want & P.PLAN_BUILD_LOOKUP else gc.k_hashed(labels)
        o = env.oracle.groupby(key)
        gb = env.dev.groupby_build(key, hint=G + G // 4)
        plan = gb.plan
        assert plan & want == want, (hex(plan), hex(want))
        assert gb.ngroups == o["ngroups"] and np.array_equal(gb.reversemap(), o["reversemap"]) and np.array_equal(gb.first_rows(), o["first_rows"])
        assert np.array_equal(gb.counts(), o["counts"])
        if reduce_plan:
            x = r.integers(-1000, 1000, n).astype(np.int32)
            got = env.dev.grouped_reduce(gb, ck.RED_SUM, x)
            assert gb.plan & reduce_plan == reduce_plan, hex(gb.plan)
            plan |= gb.plan
            assert same(got, env.oracle.grouped_reduce(ck.RED_SUM, x, o))
        return {"plan": plan}
    B = ["aqg_groupby_build"]
    call("build_partitioned", B, expect={"plan": P.PLAN_BUILD_PARTITIONED}, family="plans")(lambda env: build(env, N20, 300_000, P.PLAN_BUILD_PARTITIONED))
    call("build_not_partitioned", B, switches="no_build_partition", family="plans")(lambda env: build(env, N20, 300_000, 0))
    call("build_lookup_and_gid_partition", B + ["aqg_grouped_reduce"], expect={"plan": P.PLAN_BUILD_PARTITIONED | P.PLAN_BUILD_LOOKUP | P.PLAN_GID_PARTITION}, family="plans_big")(
        lambda env: build(env, N22, 400_000, P.PLAN_BUILD_PARTITIONED | P.PLAN_BUILD_LOOKUP, P.PLAN_GID_PARTITION))


_plans()


@call("agg_sparse_rank_bitmap", ["aqg_groupby_agg", "aqg_groupby_keys"], family="plans_bitmap")
def _sparse_rank(env):
    """the context's all-zero ranking bitmap: hint > 4096 and 64 * hint < n / 32 (sparse_rank, make_agg_plan) -- 8.4e6 rows at the least,
    the smallest n at which a stale bit of the bitmap could show"""
    import groupagg_cases as gc
    n, G = 8_400_007, 4097
    key = ((np.arange(n, dtype=np.int64) * 7919) % G * 3 - 11).astype(np.int32)
    x = (np.arange(n, dtype=np.int64) % 1013 - 500).astype(np.int32)
    out = {"plan": 0}
    for _ in range(2):                                           # twice on one context: the second call meets the bitmap the first one left
        out["plan"] |= gc.check(env.dev, env.oracle, [key], [gc.SUM, gc.COUNT], [x, x], G, 0, 0, "sparse_rank")
    assert env.dev.debug_ws_info()["rank_bm_bytes"] >= n // 8, "the ranking bitmap was not taken"
    return out


@call("grouped_reduce_scan_ewise", ["aqg_groupby_build", "aqg_groupby_postproc", "aqg_grouped_reduce", "aqg_grouped_reduce_flat", "aqg_grouped_flatten",
                                     "aqg_grouped_scan", "aqg_grouped_scan_flat", "aqg_grouped_corr", "aqg_grouped_ewise", "aqg_groupby_offsets"], family="grouped")
def _grouped(env):
    import checker as ck
    d, o = env.dev, env.oracle
    r = rng(14)
    n, G = 3 * SCAN_TILE + 11, 37
    keys = r.integers(0, G, n).astype(np.int32)
    x = r.integers(-1000, 1000, n).astype(np.int32)
    y = (x * 2 + r.integers(-9, 9, n)).astype(np.int32)
    gb = d.groupby_build([keys])
    og = o.groupby([keys])
    off, rows = gb.postproc()
    assert gb.ngroups == og["ngroups"] and np.array_equal(gb.reversemap(), og["reversemap"])
    assert np.array_equal(d.group_offsets(gb)[:gb.ngroups + 1], off)
    flat = d.grouped_flatten(gb, x)
    assert same(flat, x[rows])
    for name in ("sum", "min", "max", "avg", "count"):
        op = ck.RED_NAMES[name]
        want = o.grouped_reduce(op, x, og)
        assert same(d.grouped_reduce(gb, op, x), want), name
        assert same(d.grouped_reduce_flat(gb, op, flat), want), name
    for name, w in (("sums", 0), ("mins", 0), ("sumw", 5), ("maxw", 100), ("prev", 0)):
        op = ck.SCAN_NAMES[name]
        want = np.concatenate([o.scan(op, flat[off[g]:off[g + 1]], w) for g in range(gb.ngroups)])
        assert same(d.grouped_scan(gb, op, x, w), want), name
        assert same(d.grouped_scan(gb, op, flat, w, flat=True), want), name
    got = d.grouped_corr(gb, x, y)
    want = np.array([o.corr(x[rows[off[g]:off[g + 1]]], y[rows[off[g]:off[g + 1]]]) for g in range(gb.ngroups)])
    assert same(got, want)
    s = d.grouped_reduce(gb, ck.RED_NAMES["max"], x)
    got = d.grouped_ewise(gb, ck.OP_SUB, x, s)
    assert same(got, o.ewise(ck.OP_SUB, x, s[og["reversemap"]]))
    return {"plan": gb.plan}


# ---- sharded entries on one device: several contexts in one process (tests/test_gpu_sharded.py) ----------------------------------------------
@call("sharded_world3", ["aqg_reduce_sharded", "aqg_corr_sharded", "aqg_scan_sharded", "aqg_groupby_agg_sharded", "aqg_groupby_exchange", "aqg_groupby_agg",
                         "aqg_str_encode_sharded"], family="sharded")
def _sharded(env):
    import checker as ck
    o = env.oracle
    r = rng(15)
    n = 3 * SCAN_TILE + 100
    x = r.integers(-1000, 1000, n).astype(np.int32)
    y = (3 * x + r.integers(-7, 7, n)).astype(np.int32)
    keys = r.integers(0, 50, n).astype(np.int32)
    cuts = [0, SCAN_TILE + 1, SCAN_TILE + 4, n]
    strs = [b"s%d" % (i % 97) for i in range(300)]
    og = o.groupby([keys])
    want_sum = ck.i128_to_int(o.grouped_reduce(ck.RED_SUM, x, og))
    ranks = env.ranks(3)

    def body(rank, dev, comm):
        a, b = cuts[rank], cuts[rank + 1]
        out = {"sum": comm.reduce_sharded(ck.RED_SUM, x[a:b]), "corr": comm.corr_sharded(x[a:b], y[a:b]),
               "sums": comm.scan_sharded(ck.SCAN_NAMES["sums"], x[a:b]), "minw": comm.scan_sharded(ck.SCAN_NAMES["minw"], x[a:b], 100)}
        gb = comm.groupby_agg_sharded([keys[a:b]], [ck.RED_SUM], [x[a:b]], a, hint=64)
        out["ngroups"], out["gsum"], out["first"] = gb.ngroups, ck.i128_to_int(gb.result(0, ck.RED_SUM, ck.INT32)), gb.first_rows64()
        local = dev.groupby_agg([keys[a:b]], [ck.RED_SUM], [x[a:b]], hint=64)
        ex = comm.groupby_exchange(local, [ck.RED_SUM], a)
        out["xsum"] = ck.i128_to_int(ex.result(0, ck.RED_SUM, ck.INT32))
        codes, nd = comm.str_encode_sharded(strs[rank * 100:(rank + 1) * 100])
        out["codes"], out["nd"] = codes.to_host(), nd
        return out
    res = ranks.run(body)
    outs = []
    for rank, got in enumerate(res):
        a, b = cuts[rank], cuts[rank + 1]
        assert got["sum"] == int(x.astype(np.int64).sum()) and got["corr"] == o.corr(x, y)
        assert same(got["sums"], o.scan(ck.SCAN_NAMES["sums"], x, 0)[a:b]) and same(got["minw"], o.scan(ck.SCAN_NAMES["minw"], x, 100)[a:b])
        assert got["ngroups"] == og["ngroups"] and got["gsum"] == want_sum and got["xsum"] == want_sum
        assert np.array_equal(got["first"], og["first_rows"].astype(np.int64))
        assert got["nd"] == 97
        outs += [np.float64(got["corr"]), np.uint32(got["nd"])]
    return {"out": outs}


@call("pack_and_merge", ["aqg_groupby_pack", "aqg_groupby_merge_packed", "aqg_groupby_agg", "aqg_groupby_keys"], family="sharded")
def _pack_merge(env):
    """three row-range shards packed into the buffer an all-gather would fill and merged (tests/test_gpu_configs.py), at both merge sizes:
    world * gmax within the one-workgroup merge (2048) and beyond it"""
    import checker as ck
    d, o = env.dev, env.oracle
    r = rng(16)
    plan = 0
    for G, n in ((50, 3000), (1500, 9000)):
        key = r.integers(0, G, n).astype(np.int32)
        val = r.integers(-1000, 1000, n).astype(np.int64)
        og = o.groupby([key])
        world, gmax = 3, G
        gathered = d.to_device(np.zeros(world * (gmax + 1) * 2, np.int64))
        bounds = [0, n // 3, n // 3 + 7, n]
        for rk in range(world):
            lo, hi = bounds[rk], bounds[rk + 1]
            gb = d.groupby_agg([key[lo:hi]], [ck.RED_SUM], [val[lo:hi]])
            d.groupby_pack(gb, 0, gmax, gathered.ptr + rk * (gmax + 1) * 2 * 8)
            gb.destroy()
        merged = d.groupby_merge_packed(gathered.ptr, world, gmax, ck.INT32, ck.RED_SUM)
        assert merged.ngroups == og["ngroups"]
        assert np.array_equal(merged.keys(0, key.dtype), key[og["first_rows"]])
        assert ck.i128_to_int(merged.result(0, ck.RED_SUM, ck.INT64)) == ck.i128_to_int(o.grouped_reduce(ck.RED_SUM, val, og))
        plan |= merged.plan
    return {"plan": plan}


def by_name(name):
    return next(c for c in CALLS if c.name == name)
