"""Every family added since test_maximum_row_count, run at the row limit: n = AQG_MAX_ROWS - 1 = 4,293,918,719 rows (or PAST31 = 2^31 +
2^20 + 3 where tests/row_limit_cases.py says the family's buffers do not fit).  One test per family; each runs the SAME check function
of row_limit_cases.py twice -- at n = 100,003, where tests/test_row_limit_cases.py has shown the closed forms equal the numpy models,
and at the large size.  Whole-column comparisons stay on the device (gather from a small table, compare, reduce: the primitives
test_maximum_row_count holds at the limit); only scalars, probe slices and boundary elements come to the host.

A case skips only when the device's free memory, asked once, is below the need the case states."""
import ctypes as C
import time

import numpy as np
import pytest
import torch  # noqa: F401  (at collection: torch opens the device only where its runtime is loaded before the library's first context)

import aquery2_amd
import checker as ck
import row_limit_cases as rl
from aquery2_amd import capi as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def free_bytes():
    """free device memory, asked once through torch; None (no case skips) where torch cannot open the device in this process"""
    try:
        return int(torch.cuda.mem_get_info(0)[0])
    except RuntimeError as e:
        print("row limit: free device memory unknown (%s): no case skips" % e)
        return None


class DeviceBackend:
    """the backend of row_limit_cases over device columns (DevBuf)"""

    def __init__(self, dev):
        self.dev = dev

    def table(self, a):
        return self.dev.to_device(np.ascontiguousarray(a))

    def gather(self, tab, idx):
        d = self.dev
        out = d.empty(idx.n, tab.dtype)
        d._chk(d.lib.aqg_gather(d.ctx, tab.tag, C.c_void_p(tab.ptr), C.c_void_p(idx.ptr), C.c_uint32(idx.n), C.c_void_p(out.ptr)), "aqg_gather")
        return out

    def cmp(self, op, a, b):
        return self.dev.ewise(op, a, b, keep=True)

    def count(self, mask):
        return int(self.dev.reduce(ck.RED_SUM, mask))

    def total(self, x):
        return int(self.dev.reduce(ck.RED_SUM, x))

    def prev(self, x):
        return self.dev.scan(ck.SCAN_PREV, x, keep=True)

    def rows(self, x, lo, hi):
        return P.DevBuf(self.dev, x.ptr + int(lo) * x.dtype.itemsize, x.dtype, int(hi) - int(lo), owned=False).to_host()

    def at(self, x, idx):
        return self.dev.gather(x, np.ascontiguousarray(idx, dtype=np.uint32))

    def free(self, *cols):
        for c in cols:
            c.free()


class World:
    """the device's columns of an n-row table (made on first use, freed by name), the oracle's slices of the same table, and the
    histograms the closed forms start from"""

    GEN = {"v1": ck.GEN_V1, "id1": ck.GEN_ID1, "price": ck.GEN_PRICE, "ts": ck.GEN_TIMESTAMP}

    def __init__(self, dev, oracle, n):
        self.dev, self.n, self.src, self.B, self.cols = dev, n, rl.Source(oracle, n), DeviceBackend(dev), {}

    def col(self, name):
        if name not in self.cols:
            c = self.dev.gen_column(self.GEN[name], rl.SEED, 0, self.n, self.n, rl.K)
            if name == "ts":                                           # row + 1 as uint32: ascending past 2^31
                raw = c
                c = P.DevBuf(self.dev, raw.ptr, np.uint32, self.n, owned=False)
                c._owner = raw
            self.cols[name] = c
        return self.cols[name]

    def drop(self, *names):
        for name in names:
            c = self.cols.pop(name, None)
            if c is not None:
                (getattr(c, "_owner", None) or c).free()

    def table(self, *names):
        """(keys..., counts) of a count per value (tuple) of the named columns, from aqg_groupby_agg"""
        cols = [self.col(nm) for nm in names]
        gb = self.dev.groupby_agg(cols, [ck.RED_COUNT], [cols[0]], hint=1024)
        out = tuple(gb.keys(k, np.int32) for k in range(len(cols))) + (gb.counts(),)
        gb.destroy()
        return out

    def hist(self, *names):
        kw = {nm: self.table(*(("id1", "v1") if nm == "pair" else (nm,))) for nm in names}
        h = rl.Hist.of_tables(**kw)
        assert h.n == self.n
        return h


class TrackingDevice(aquery2_amd.Device):
    """a context that remembers the columns allocated through it and frees them before it goes (device columns are not the context's:
    what a failing body left behind would otherwise stay allocated for the rest of the process)"""

    def __init__(self):
        super().__init__(0)
        self.made = []

    def empty(self, n, dtype):
        self.made.append(super().empty(n, dtype))
        return self.made[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for buf in self.made:
            buf.free()
        self.close()


def at_both_sizes(family, oracle, free_bytes, body):
    for n in (rl.SMALL, rl.size_of(family)):
        need = rl.NEED[family](n)
        if free_bytes is not None and need > free_bytes:
            pytest.skip("%s at %d rows needs %.1f GB of device memory, %.1f GB are free" % (family, n, need / 1e9, free_bytes / 1e9))
        t0 = time.perf_counter()
        with TrackingDevice() as dev:                                  # a context of its own: its workspace goes with it
            body(World(dev, oracle, n))
        print("row limit: %s at %d rows (%.1f GB stated): %.1f s" % (family, n, need / 1e9, time.perf_counter() - t0))


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
def test_sort(oracle, free_bytes, desc):
    """aqg_sort_rows by v1, stable, ascending and descending: rows_out, the scatter's 32-bit positions and the six n-row planes of the
    workspace at the limit"""
    def body(w):
        h = w.hist("v1")
        v1, ts = w.col("v1"), w.col("ts")
        order = w.dev.sort_rows([v1], [P.ORDER_DESC if desc else P.ORDER_ASC], keep=True)
        assert w.dev.sort_last_passes() == 1                           # 1..5: one digit position varies
        rl.check_sort(w.B, w.src, h, v1, ts, order, desc)
    at_both_sizes("sort", oracle, free_bytes, body)


def test_rank(oracle, free_bytes):
    """aqg_rank over v1: min and dense against the six-entry table over the whole column (ascending; max and descending too), the row
    number against the stable order, NTILE on the probe slices from the row number"""
    def body(w):
        h = w.hist("v1")
        v1 = w.col("v1")
        for method, code, desc in (("min", P.RANK_MIN, False), ("dense", P.RANK_DENSE, False), ("max", P.RANK_MAX, True), ("min", P.RANK_MIN, True)):
            got = w.dev.rank(v1, code, P.ORDER_DESC if desc else P.ORDER_ASC, keep=True)
            assert w.dev.rank_last()[0] == P.RANK_ROUTE_SORTED
            rl.check_rank_values(w.B, h, v1, got, method, desc)
            got.free()
        first = w.dev.rank(v1, P.RANK_FIRST, P.ORDER_ASC, keep=True)
        ntile = w.dev.rank(v1, P.RANK_NTILE, P.ORDER_ASC, k=rl.RANK_K, keep=True)
        rl.check_ntile(w.B, h, first, ntile)
        ntile.free()
        order = w.dev.sort_rows([v1], [P.ORDER_ASC], keep=True)
        w.drop("v1")
        rl.check_row_number(w.B, h, w.col("ts"), order, first)
    at_both_sizes("rank", oracle, free_bytes, body)


def run_select(dev, x):
    nums, den = rl.QUANT
    return {"median": (dev.median(x, P.SEL_LOWER), dev.median(x, P.SEL_UPPER)),
            "quantiles": (dev.quantiles(x, nums, den, P.SEL_LOWER), dev.quantiles(x, nums, den, P.SEL_UPPER)),
            "distinct": dev.count_distinct(x),
            "top": {desc: dev.topk(x, rl.TOPK, P.ORDER_DESC if desc else P.ORDER_ASC, rows=True) for desc in (False, True)}}


def test_select(oracle, free_bytes):
    """aqg_median, aqg_quantiles, aqg_topk and aqg_count_distinct over v1 and price: the values from the histogram, the top-k rows from
    the generator"""
    def body(w):
        for name, col in rl.SELECT_COLS:
            h = w.hist(name)
            rl.check_select(w.src, h, name, col, run_select(w.dev, w.col(name)))
            w.drop(name)
        assert w.dev.count_distinct(w.col("id1")) == rl.K
    at_both_sizes("select", oracle, free_bytes, body)


def test_joins(oracle, free_bytes):
    """a 100-row build side, all n rows of id1 as the probe side: aqg_join_lookup / aqg_join_count and the typed-key forms"""
    def body(w):
        h = w.hist("id1")
        id1 = w.col("id1")
        key, _ = rl.join_build()
        d = w.dev
        for what in ("join", "join_keys"):
            out = d.empty(w.n, np.uint32)
            if what == "join":
                kd = d.to_device(key)
                d._chk(d.lib.aqg_join_lookup(d.ctx, kd.tag, C.c_void_p(kd.ptr), C.c_uint32(kd.n), C.c_void_p(id1.ptr), C.c_uint32(w.n), C.c_void_p(out.ptr)), "aqg_join_lookup")
                count = d.join_count(kd, id1)
            else:
                kd, dts, bp = d._keyargs([key])
                pp = (C.c_void_p * 1)(id1.ptr)
                d._chk(d.lib.aqg_join_keys_lookup(d.ctx, 1, dts, bp, kd[0].n, pp, w.n, out.ptr), "aqg_join_keys_lookup")
                count = d.join_keys_count([key], [id1])
            rl.check_join(w.B, h, id1, out, count, what)
            out.free()
    at_both_sizes("join", oracle, free_bytes, body)


def test_composite_key_join(oracle, free_bytes):
    """a 469-row build side of (id1, v1) tuples, all n rows of (id1, v1) as the probe side: aqg_join_keys_lookup over the whole column,
    aqg_join_keys_count for the inner, left, semi and anti joins"""
    def body(w):
        d = w.dev
        h = w.hist("pair")
        id1, v1 = w.col("id1"), w.col("v1")
        kg, kv, _ = rl.pair_build()
        kd, dts, bp = d._keyargs([kg, kv])
        pp = (C.c_void_p * 2)(id1.ptr, v1.ptr)
        look = d.empty(w.n, np.uint32)
        d._chk(d.lib.aqg_join_keys_lookup(d.ctx, 2, dts, bp, kd[0].n, pp, w.n, look.ptr), "aqg_join_keys_lookup")
        counts = [d.join_keys_count(kd, [id1, v1], kind) for kind in (P.JOIN_INNER, P.JOIN_LEFT, P.JOIN_SEMI, P.JOIN_ANTI)]
        six = d.ewise(ck.OP_MUL, id1, np.int32(6), ot=ck.INT32, keep=True)
        w.drop("id1")
        comb = d.ewise(ck.OP_ADD, six, v1, ot=ck.INT32, keep=True)
        six.free()
        rl.check_pair_join(w.B, h, comb, look, counts)
    at_both_sizes("join_pair", oracle, free_bytes, body)


def test_window_quantiles(oracle, free_bytes):
    """aqg_window_quantiles of price, w = 21, three ranks: the planes start at j n elements, the tiles read a 20-row halo"""
    def body(w):
        price = w.col("price")
        for which in (P.SEL_LOWER, P.SEL_UPPER):
            out = w.dev.window_quantiles(price, rl.WINQ["nums"], rl.WINQ["den"], rl.WINQ["w"], which, keep=True)
            assert w.dev.window_quantiles_last()[1] == rl.WINQ["w"] - 1
            rl.check_winq(w.B, w.src, w.n, out, which)
            out.free()
    at_both_sizes("winq", oracle, free_bytes, body)


def pair_body(routes, fams):
    import pair_moments as pm
    import pairwin_cases as pc
    ops = {pm.COV: P.SCAN2_COVW, pm.CORR: P.SCAN2_CORRW, pm.BETA: P.SCAN2_BETAW}

    def body(w):
        x, y = w.col("price"), w.col("id1")
        out = w.dev.empty(w.n, np.float64)
        for route in routes:
            ww = rl.PAIR_WINDOWS[route]
            for fam in fams:
                w.dev.scan2(ops[fam], x, y, ww, keep=True, out=out)
                assert w.dev.scan2_last() == (pc.route_of(ww, w.n), pc.TS), (route, fam)
                rl.check_pair(w.B, w.src, w.n, out, fam, ww)
    return body


def test_pair_windows(oracle, free_bytes):
    """aqg_scan2 of (price, id1): covw / corrw / betaw on the REG and LDS routes and covw on the PREFIX route, whose difference kernel
    strides by exactly 2^20 rows on 256 compute units -- all the slack AQG_MAX_ROWS leaves"""
    import pair_moments as pm
    at_both_sizes("pair", oracle, free_bytes, lambda w: (pair_body(("reg", "lds"), (pm.COV, pm.CORR, pm.BETA))(w), pair_body(("prefix",), (pm.COV,))(w)))


def test_pair_windows_wide_prefix(oracle, free_bytes):
    """corrw and betaw on the PREFIX route: five and four doubles a row of workspace"""
    import pair_moments as pm
    at_both_sizes("pair_wide", oracle, free_bytes, pair_body(("prefix",), (pm.CORR, pm.BETA)))


def test_ema(oracle, free_bytes):
    """aqg_scan_ema of price, alpha = 1/4, both modes: the tile aggregates' chunked scan over two million tiles"""
    from test_gpu_ema import hold

    def body(w):
        price = w.col("price")
        out = w.dev.empty(w.n, np.float64)
        for mode in (P.EMA_RECURSIVE, P.EMA_ADJUSTED):
            w.dev.ema(price, alpha=rl.EMA_ALPHA, mode=mode, keep=True, out=out)
            rl.check_ema(w.B, w.src, w.n, out, mode, hold)
    at_both_sizes("ema", oracle, free_bytes, body)


def test_time_windows(oracle, free_bytes):
    """aqg_rangew over (TIMESTAMP as uint32, price), span 10, both frames: bounds by binary search over stamps past 2^31, the block
    tree of the fold, 16-byte sums"""
    import timewin_cases as tc
    from test_gpu_timewin import OPS, hold

    def body(w):
        ts, price = w.col("ts"), w.col("price")
        for frame in (P.RANGEW_OPEN, P.RANGEW_CLOSED):
            bounds = w.dev.rangew_bounds(ts, rl.TW_SPAN, frame, keep=True)
            for op in OPS:
                x = None if op == P.RANGEW_COUNT else price
                out = w.dev.rangew_fold(op, x, bounds, keep=True)
                assert w.dev.rangew_last()[:2] == tc.levels(w.n)
                rl.check_timewin(w.B, w.src, w.n, bounds, {op: out}, frame, hold)
                out.free()
            one = w.dev.rangew(P.RANGEW_MAX, ts, rl.TW_SPAN, price, frame, keep=True)        # the fused entry: bounds in workspace
            rl.check_timewin(w.B, w.src, w.n, bounds, {P.RANGEW_MAX: one}, frame, hold)
            one.free()
            bounds.free()
    at_both_sizes("timewin", oracle, free_bytes, body)


def test_asof_and_window_join(oracle, free_bytes):
    """the whole table as the build side of aqg_join_asof / aqg_join_window (on = TIMESTAMP as uint32: ascending past 2^31; no key
    columns), about 10,000 probe stamps at and beside every threshold, the column's end and the ends of the type"""
    import wj_model as wm
    from test_gpu_wj import OPS, hold

    def body(w):
        d = w.dev
        ts, stamps = w.col("ts"), rl.join_probes(w.n)
        sd = d.to_device(stamps)
        for forward, strict in rl.ASOF_MODES:
            got = d.join_asof([], ts, [], sd, P.ASOF_FORWARD if forward else P.ASOF_BACKWARD, strict)
            assert d.join_asof_last()[0] & (P.ASOF_ROUTE_NOKEYS | P.ASOF_ROUTE_PRESORTED) == P.ASOF_ROUTE_NOKEYS | P.ASOF_ROUTE_PRESORTED
            rl.check_asof(w.n, stamps, got, forward, strict)
        v1 = w.col("v1")
        outs = {op: d.join_window(op, [], ts, [], sd, rl.WJ_BEFORE, rl.WJ_AFTER, x=None if op == wm.COUNT else v1,
                                  fill=None if op in (wm.COUNT, wm.SUM) else rl.WJ_FILL) for op in OPS}
        assert d.join_window_last()[0] & P.ASOF_ROUTE_PRESORTED
        rl.check_wj(w.src, w.n, stamps, outs, hold)
    at_both_sizes("asof_wj", oracle, free_bytes, body)


def test_groupby_build(oracle, free_bytes):
    """aqg_groupby_build(id1): the group table, grouped_reduce against groupby_agg bit for bit, grouped medians and quantiles of v1
    from the 500-group table, and the flat layout -- grouped_flatten of id1 and of the stamps over the whole column"""
    def body(w):
        d = w.dev
        h = w.hist("id1", "pair")
        id1, v1 = w.col("id1"), w.col("v1")
        agg = d.groupby_agg([id1], [ck.RED_SUM], [v1], hint=128)
        agg_keys, agg_sums = agg.keys(0, np.int32), agg.result(0, ck.RED_SUM, ck.INT32)
        agg.destroy()
        gb = d.groupby_build([id1], hint=128)
        rl.check_group_table(w.src, h, gb.keys(0, np.int32), gb.counts(), d.grouped_reduce(gb, ck.RED_SUM, v1), agg_keys, agg_sums)
        rl.check_group_medians(w.src, h, d.grouped_median(gb, v1, P.SEL_LOWER), d.grouped_median(gb, v1, P.SEL_UPPER))
        nums, den = rl.GROUP_QUANT
        for which in (P.SEL_LOWER, P.SEL_UPPER):
            rl.check_group_quantiles(w.src, h, d.grouped_quantiles(gb, v1, nums, den, which), bool(which))
        w.drop("v1")
        ts = w.col("ts")
        key_flat = d.grouped_flatten(gb, id1, keep=True)
        rl.check_flat_keys(w.B, w.src, h, ts, key_flat)
        key_flat.free()
        ts_flat = d.grouped_flatten(gb, ts, keep=True)
        w.drop("ts")
        rl.check_flat_stamps(w.B, w.src, h, ts_flat)
        ts_flat.free()
        gb.destroy()
    at_both_sizes("grouped", oracle, free_bytes, body)


def test_grouped_window_scan(oracle, free_bytes):
    """aqg_grouped_scan SUMW(7) of v1 over the build of id1: 16-byte sums in the flat layout, held at both ends of every group"""
    def body(w):
        h = w.hist("id1")
        gb = w.dev.groupby_build([w.col("id1")], hint=128)
        out = w.dev.grouped_scan(gb, ck.SCAN_SUMW, w.col("v1"), rl.GROUP_W, keep=True)
        rl.check_group_window(w.B, w.src, h, out, oracle)
        out.free()
        gb.destroy()
    at_both_sizes("grouped_scan", oracle, free_bytes, body)


def test_grouped_rank(oracle, free_bytes):
    """aqg_grouped_rank of v1 inside the groups of id1 (min, dense, max ascending; min descending) over the whole flat layout, against
    a gather from the 606-entry table over id1 * 6 + v1 brought into the flat layout"""
    def body(w):
        d = w.dev
        h = w.hist("id1", "pair")
        id1, v1 = w.col("id1"), w.col("v1")
        six = d.ewise(ck.OP_MUL, id1, np.int32(6), ot=ck.INT32, keep=True)
        comb = d.ewise(ck.OP_ADD, six, v1, ot=ck.INT32, keep=True)
        six.free()
        gb = d.groupby_build([id1], hint=128)
        comb_flat = d.grouped_flatten(gb, comb, keep=True)
        comb.free()
        for method, code, desc in (("min", P.RANK_MIN, False), ("dense", P.RANK_DENSE, False), ("max", P.RANK_MAX, False), ("min", P.RANK_MIN, True)):
            got = d.grouped_rank(gb, v1, code, P.ORDER_DESC if desc else P.ORDER_ASC, keep=True)
            assert d.rank_last()[0] == P.RANK_ROUTE_SORTED
            rl.check_group_rank(w.B, h, comb_flat, got, method, desc)
            got.free()
        comb_flat.free()
        gb.destroy()
    at_both_sizes("grouped_rank", oracle, free_bytes, body)
