"""aqg_topk / aqg_grouped_topk / aqg_grouped_topk_flat (topk.hip): the k largest or smallest elements with their positions.
Everything goes through the C-ABI and is held to tests/topk_model.py: `check` demands every property of the contract (values bitwise
the elements at their positions, positions inside the group, distinct, ascending among equal images, every slot the image of its
rank, exact padding) and leaves open only WHICH of the rows tied on the k-th image are taken.  The seeded cases assert on the model
that no slot is flagged (a NaN, or a zero of a group with both zeros) before the device is asked; only the cases written for zeros
and NaNs compare such slots by value.

Passes reported by aqg_select_last_routes for these calls: SMALL 1; GROUP / SPLIT the digit passes of the threshold search, at most
one per byte of the dtype, plus the one collecting pass -- a group of at most k rows needs no search and reports 1."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import extremes as ex
import median_model as mm
import topk_model as tk
from aquery2_amd.capi import (BOOL, I128, INT32, INT128, ORDER_ASC, ORDER_DESC, ORDER_NEG, ROUTE_GROUP, ROUTE_SMALL, ROUTE_SPLIT, TOPK_MAX, U128,
                              UINT128, AqgError, DevBuf)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL_MAX = 256          # AQG_SELECT_SMALL_MAX default
SMALL_CAP = 512
SPLIT_MIN = 1 << 20      # AQG_SELECT_SPLIT_MIN default
CHUNK = 8192             # topk.hip / select_radix.hpp: rows per chunk of a SPLIT group
TILE = 2048              # ... flat positions per workgroup of the SMALL route
DTYPES = ex.NUM_DTYPES + [np.dtype(np.bool_)]
ORDERS = (ORDER_ASC, ORDER_DESC)
SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, SPLIT_MIN - 1, SPLIT_MIN, SPLIT_MIN + 1]
KS = [1, 2, 3, 64, 65, 256, 257, 1024]
assert TOPK_MAX == 1024


@pytest.fixture(scope="module")
def dev():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def upload(dev, a, shift=0):
    """the column on the device, `shift` elements off an aligned base; bool columns tagged BOOL"""
    a = np.ascontiguousarray(a)
    host = a.astype(np.uint8) if a.dtype == np.bool_ else a
    base = dev.to_device(np.concatenate([np.zeros(shift, host.dtype), host]))
    buf = DevBuf(dev, base.ptr + shift * host.itemsize, host.dtype, host.size, owned=False)
    buf._base = base
    if a.dtype == np.bool_:
        buf._tag = BOOL
    return buf


def as_model(a):
    return a.astype(np.uint8) if a.dtype == np.bool_ else a


def flat_inputs(rng, dt, n):
    r = ex.full_range(rng, dt, n)
    two = ex.full_range(rng, dt, 2)
    yield "random", r
    yield "equal", np.repeat(ex.full_range(rng, dt, 1), n)
    yield "two", two[rng.integers(0, 2, n)]
    yield "ascending", np.sort(r)
    yield "descending", np.sort(r)[::-1].copy()


def flat_route(n):
    return 0 if n == 0 else ROUTE_SMALL if n <= SMALL_MAX else ROUTE_GROUP if n < SPLIT_MIN else ROUTE_SPLIT


@pytest.mark.parametrize("order", ORDERS, ids=["asc", "desc"])
@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
def test_flat_every_size_k_and_input(dev, dt, order):
    rng = np.random.default_rng(2000 + DTYPES.index(dt))
    case = 0
    for n in SIZES:
        for name, col in flat_inputs(rng, dt, n):
            col = as_model(col)
            off = [0, n]
            model = tk.topk(col, off, max(KS), order)                     # one sort for every k: the first k slots of the first 1024
            assert not model[2].any(), "seeded flat inputs hold no NaN and no mixed zeros among their extremes"
            for shift in ((0, 1, 3) if n <= SMALL_MAX + 1 else ((0, 1, 3)[case % 3],)):
                x = upload(dev, col, shift)
                for k in KS:
                    vals, rows = dev.topk(x, k, order, rows=True)
                    tk.check(vals[None, :], rows[None, :], col, off, k, order, model=model)
                    routes, passes = dev.select_last_routes()
                    assert routes == flat_route(n), (n, k, routes)
                    assert passes <= col.dtype.itemsize + 1 and (passes >= 1) == (n > 0), (n, k, passes)
                    if k in (3, 257):                                     # and without positions
                        tk.check(dev.topk(x, k, order)[None, :], None, col, off, k, order, model=model)
                assert np.array_equal(x.to_host().view(np.uint8), col.view(np.uint8)), "the input column was modified"
            case += 1


def grouped_case(dev, keys, x, ks, orders=ORDERS, expect_routes=None, by_value=False):
    """both layouts, with and without positions, against the flat layout the build defines (x[row_ids], offsets of postproc)"""
    gid, G = mm.first_occurrence_ids(*keys)
    xm = as_model(x)
    gb = dev.groupby_build(keys)
    assert gb.ngroups == G
    off, row_ids = gb.postproc()
    xd = upload(dev, x)
    xf = dev.grouped_flatten(gb, xd, keep=True)
    if x.dtype == np.bool_:
        xf._tag = BOOL
    xflat = xf.to_host()
    assert np.array_equal(xflat.view(np.uint8), xm[row_ids].view(np.uint8)) and np.array_equal(gid[row_ids], np.repeat(np.arange(G), np.diff(off.astype(np.int64))))
    out = {}
    for order in orders:
        for k in ks:
            model = tk.topk(xflat, off, k, order)
            assert by_value or not model[2].any(), "seeded inputs leave no flagged slot"
            for flat in (False, True):
                vals, pos = dev.grouped_topk(gb, xf if flat else xd, k, order, flat=flat, pos=True)
                tk.check(vals, pos, xflat, off, k, order, model=model)
                routes, passes = dev.select_last_routes()
                assert 1 <= passes <= xm.dtype.itemsize + 1, passes
                if expect_routes is not None:
                    assert routes == expect_routes, (routes, expect_routes)
                tk.check(dev.grouped_topk(gb, xf if flat else xd, k, order, flat=flat), None, xflat, off, k, order, model=model)
            out[order, k] = vals
    assert np.array_equal(xd.to_host().view(np.uint8), xm.view(np.uint8)), "x was modified"
    assert np.array_equal(xf.to_host().view(np.uint8), xflat.view(np.uint8)), "xflat was modified"
    gb.destroy()
    return out


def mixed_sizes(k):
    """group sizes around k and around both thresholds, a run of 300 groups of exactly 256 rows (every 2048-row tile border is straddled),
    one group above the SPLIT threshold and a band of 5000-row groups"""
    return [1, 2, 3, k - 1, k, k + 1, 255, 256, 257] + [256] * 300 + [SPLIT_MIN + 5] + [5000] * 6


@pytest.mark.parametrize("dt", [np.dtype(np.float32), np.dtype(np.int64), np.dtype(np.uint8), np.dtype(np.int16)], ids=ex.nm)
def test_grouped_all_three_routes_in_one_call(dev, dt):
    rng = np.random.default_rng(3100 + dt.itemsize)
    for k in (4, 100):
        sizes = [s for s in mixed_sizes(k) if s > 0]
        keys = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
        grouped_case(dev, [keys], ex.full_range(rng, dt, len(keys)), [k], expect_routes=ROUTE_SMALL | ROUTE_GROUP | ROUTE_SPLIT)


def test_grouped_two_key_columns_and_bool(dev):
    rng = np.random.default_rng(3200)
    n = 200_003
    k1, k2 = rng.integers(0, 30, n).astype(np.int16), rng.integers(-5, 5, n).astype(np.int64)
    grouped_case(dev, [k1, k2], ex.full_range(rng, np.dtype(np.float64), n), [2, 700])
    grouped_case(dev, [k1, k2], rng.integers(0, 2, n).astype(np.bool_), [3, 1024])


def test_ties_on_the_kth_value(dev):
    """the k-th value is shared by many more rows than there are slots left (`need` < ties) in every route; the tied rows lie on both
    sides of an 8192-row chunk border of the SPLIT group and of a 2048-row tile border of the SMALL groups; all-equal groups larger than k"""
    rng = np.random.default_rng(3300)
    big = SPLIT_MIN + 3 * CHUNK + 11
    sizes = [big, 9000, 9000] + [200] * 40 + [7, 300, 5000]
    gid = np.repeat(np.arange(len(sizes)), sizes)
    x = rng.integers(0, 1000, len(gid)).astype(np.int32)
    top = np.int32(5000)
    # SPLIT group: three rows above the tie, then rows tied on `top` around the first chunk borders (and many elsewhere)
    x[[17, CHUNK + 5, 2 * CHUNK - 1]] = [7000, 7001, 7000]
    x[CHUNK - 3:CHUNK + 3] = top
    x[rng.integers(0, big, 500)] = top
    x[[17, CHUNK + 5, 2 * CHUNK - 1]] = [7000, 7001, 7000]
    # GROUP groups: one with a few rows above a wide tie, one all equal
    g1 = big
    x[g1:g1 + 9000:2] = top
    x[g1 + 1] = 6000
    x[g1 + 9000:g1 + 18000] = 42
    # SMALL groups of 200 rows cross the 2048-row tile borders; every second row ties on the top value, some are all equal
    s0 = g1 + 18000
    x[s0:s0 + 8000:2] = top
    x[s0 + 2000:s0 + 2400] = 77
    x[-5000:] = 9                                                           # an all-equal GROUP group larger than k
    x[-5300:-5000] = 3                                                      # an all-equal 300-row group
    # rows are given in flat order through keys that are already grouped: the flat layout is each group's rows in descending row order
    for dtype in (np.int32, np.float32):
        grouped_case(dev, [gid.astype(np.int32)], x.astype(dtype), [1, 4, 130], expect_routes=ROUTE_SMALL | ROUTE_GROUP | ROUTE_SPLIT)


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_zeros_nans_and_infinities(dev, dt):
    """written to exercise the flagged slots: compared by value (check still demands bitwise elements at the reported positions)"""
    rng = np.random.default_rng(3400)
    pool = np.array([0.0, -0.0, np.nan, ex._neg_nan(dt), np.inf, -np.inf, 1.5, -2.5], dtype=dt)
    sizes = [SPLIT_MIN + 9, 40_000, 300, 300, 5, 70_000, 100]
    gid = np.repeat(np.arange(len(sizes)), sizes)
    x = pool[rng.integers(0, len(pool), len(gid))]
    x[gid == 2] = np.where(rng.integers(0, 2, 300) == 1, ex._neg_nan(dt), dt.type(np.nan))       # all NaN, both signs
    x[gid == 5] = np.where(rng.integers(0, 2, 70_000) == 1, ex._neg_nan(dt), dt.type(np.nan))
    x[gid == 6] = np.where(rng.integers(0, 2, 100) == 1, dt.type(-0.0), dt.type(0.0))
    p = rng.permutation(len(gid))
    out = grouped_case(dev, [gid[p].astype(np.int32)], x[p].astype(dt), [3, 200], by_value=True)
    assert np.isnan(out[ORDER_DESC, 3]).any() and np.isinf(out[ORDER_ASC, 3]).any()
    for n in (5, 300, 70_000, SPLIT_MIN + 7):                                # an only -0.0 column returns -0.0, in every route
        col = np.full(n, -0.0, dt)
        for order in ORDERS:
            vals, rows = dev.topk(col, 4, order, rows=True)
            tk.check(vals[None, :], rows[None, :], col, [0, n], 4, order)
            assert np.all(np.signbit(vals)) and np.all(vals == 0)
        mixed = np.where(np.arange(n) % 3 == 0, dt.type(0.0), dt.type(-0.0))
        mixed[n // 2] = np.nan
        for order in ORDERS:
            vals, rows = dev.topk(mixed, 4, order, rows=True)
            tk.check(vals[None, :], rows[None, :], mixed, [0, n], 4, order)
            assert np.isnan(vals[0]) == (order == ORDER_DESC)


PRELUDE = r'''
import hashlib
import sys
import numpy as np
sys.path.insert(0, "tests")
import aquery2_amd, extremes as ex, median_model as mm, topk_model as tk
gpu = aquery2_amd.Device(0)
rng = np.random.default_rng(91)
res = []
for dt in (np.int8, np.uint16, np.int32, np.float32, np.uint64, np.float64):
    keys = rng.integers(0, 37, N).astype(np.int32)
    keys[:LONG] = 5
    x = ex.full_range(rng, np.dtype(dt), N)
    x[LONG - 40:LONG] = x[0]                                # an all-equal run inside the long group
    gb = gpu.groupby_build([keys])
    off, row_ids = gb.postproc()
    xflat = x[row_ids]
    for order in (0, 1):
        for k in KS:
            vals, pos = gpu.grouped_topk(gb, x, k, order, pos=True)
            assert gpu.select_last_routes()[0] == WANT, gpu.select_last_routes()
            assert not tk.topk(xflat, off, k, order)[2].any()
            tk.check(vals, pos, xflat, off, k, order)
            v1, r1 = gpu.topk(x[:FLAT], k, order, rows=True)
            assert gpu.select_last_routes()[0] == WANT, gpu.select_last_routes()
            tk.check(v1[None, :], r1[None, :], x[:FLAT], [0, FLAT], k, order)
            res += [vals.tobytes().hex(), v1.tobytes().hex()]
print("OK", hashlib.sha256("".join(res).encode()).hexdigest(), flush=True)
'''


def run_pinned(want, env, n, long_group, flat_n, ks):
    head = f"WANT, N, LONG, FLAT, KS = {want}, {n}, {long_group}, {flat_n}, {ks}\n"
    out = subprocess.run([sys.executable, "-c", head + PRELUDE], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env), cwd=ROOT)
    assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
    return out.stdout.split()[-1]


def test_every_route_alone_gives_the_same_values():
    """the same input through one route alone (mask exactly 1, 2, 4), in fresh processes because the thresholds are read once: equal
    digests of the values, positions held to `check` in each.  SMALL cannot take a group above its 512-row cap, so it is compared on
    an input whose groups fit; GROUP and SPLIT are compared on a 30,011-row column with a 9,000-row group"""
    group = {"AQG_SELECT_SMALL_MAX": "0", "AQG_SELECT_SPLIT_MIN": "4000000000"}
    split = {"AQG_SELECT_SMALL_MAX": "0", "AQG_SELECT_SPLIT_MIN": "1"}
    small = {"AQG_SELECT_SMALL_MAX": str(SMALL_CAP)}
    ks = [1, 3, 257, 1024]
    assert run_pinned(ROUTE_GROUP, group, 30_011, 9000, 30_011, ks) == run_pinned(ROUTE_SPLIT, split, 30_011, 9000, 30_011, ks), "GROUP and SPLIT disagree"
    fits = (ROUTE_SMALL, small, 9_011, 150, 300, ks), (ROUTE_GROUP, group, 9_011, 150, 300, ks), (ROUTE_SPLIT, split, 9_011, 150, 300, ks)
    a, b, c = (run_pinned(*args) for args in fits)
    assert a == b == c, "SMALL, GROUP and SPLIT disagree"


def test_errors_leave_the_outputs_alone(dev):
    import checker as ck
    lib = dev.lib
    keys = np.arange(10, dtype=np.int32) % 3
    gb = dev.groupby_build([keys])
    sv, sp = np.full(64, 0x5A5A5A5A5A5A5A5A, np.uint64), np.full(64, 0x5A5A5A5A, np.uint32)
    vals, pos = dev.to_device(sv), dev.to_device(sp)
    x = dev.to_device(np.arange(10, dtype=np.int32))

    def calls(order, tag, xp, k, vp, pp, ctx=dev.ctx, h=gb.h, whole=True):
        if whole:
            yield lib.aqg_topk(ctx, order, tag, xp, 10, k, vp, pp)
        yield lib.aqg_grouped_topk(ctx, h, order, tag, xp, k, vp, pp)
        yield lib.aqg_grouped_topk_flat(ctx, h, order, tag, xp, k, vp, pp)
    ARG, DTYPE = 3, 2
    for k in (0, TOPK_MAX + 1, 0xFFFFFFFF):
        assert list(calls(ORDER_DESC, INT32, x.ptr, k, vals.ptr, pos.ptr)) == [ARG] * 3, k
    for order in (ORDER_NEG, 3, -1):
        assert list(calls(order, INT32, x.ptr, 2, vals.ptr, pos.ptr)) == [ARG] * 3, order
    for tag, npdt in ((INT128, I128), (UINT128, U128)):
        wide = dev.to_device(np.zeros(10, npdt))
        assert list(calls(ORDER_ASC, tag, wide.ptr, 2, vals.ptr, pos.ptr)) == [DTYPE] * 3
    assert list(calls(ORDER_ASC, INT32, None, 2, vals.ptr, pos.ptr)) == [ARG] * 3          # null column
    assert list(calls(ORDER_ASC, INT32, x.ptr, 2, None, pos.ptr)) == [ARG] * 3             # null values
    assert list(calls(ORDER_ASC, INT32, x.ptr, 2, vals.ptr, pos.ptr, ctx=None)) == [ARG] * 3
    assert list(calls(ORDER_ASC, INT32, x.ptr, 2, vals.ptr, pos.ptr, h=None, whole=False)) == [ARG] * 2
    agg = dev.groupby_agg([keys], [ck.RED_SUM], [np.arange(10, dtype=np.int32)])        # a fused group-by handle: rejected like the median rejects it
    assert list(calls(ORDER_ASC, INT32, x.ptr, 2, vals.ptr, pos.ptr, h=agg.h, whole=False)) == [ARG] * 2
    with pytest.raises(AqgError) as e:
        dev.grouped_topk(agg, x, 2)
    assert e.value.code == ARG
    dev.sync()
    assert np.array_equal(vals.to_host(), sv) and np.array_equal(pos.to_host(), sp), "an output was written by a refused call"
    # padding is exactly zero / 0xFFFFFFFF, and nothing past G * k is touched
    got = lib.aqg_grouped_topk(dev.ctx, gb.h, ORDER_DESC, INT32, x.ptr, 5, vals.ptr, pos.ptr)
    assert got == 0
    v, p = vals.to_host().view(np.int32), pos.to_host()
    assert v[:15].reshape(3, 5).tolist() == [[9, 6, 3, 0, 0], [7, 4, 1, 0, 0], [8, 5, 2, 0, 0]]
    real = np.arange(5)[None, :] < np.array([4, 3, 3])[:, None]                     # group 0 holds rows 0, 3, 6, 9: its fourth slot is the element 0
    assert np.all(p[:15].reshape(3, 5)[~real] == 0xFFFFFFFF) and np.all(p[:15].reshape(3, 5)[real] < 10)
    assert np.all(v[15:] == 0x5A5A5A5A) and np.all(p[15:] == 0x5A5A5A5A)
    # empty inputs
    v0, r0 = dev.topk(np.zeros(0, np.float64), 3, rows=True)
    assert not v0.view(np.uint64).any() and np.all(r0 == 0xFFFFFFFF) and dev.select_last_routes() == (0, 0)
    gb0 = dev.groupby_build([np.zeros(0, np.int32)])
    assert gb0.ngroups == 0 and dev.grouped_topk(gb0, np.zeros(0, np.int32), 3).shape == (0, 3)


def _synthetic():
    """host_main's `synthetic` dataset: columns a and c of its LCG"""
    x, a, c = 12345, [], []
    for _ in range(200000):
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        a.append((x >> 33) % 1000)
        c.append((x >> 20) % 97)
    return np.array(a, np.int32), np.array(c, np.int32)


@pytest.mark.parametrize("dataset,suffix,G", [("trade_small", "", 300), ("synthetic", "_c", 1000)])
def test_emitted_group_loop_q8(tmp_path, dataset, suffix, G):
    """the generated group loop `col[g] = maxk(2, v[vecs[g]])` and `mink(3, v[vecs[g]] + k[vecs[g]])` (tests/emitted/topk_q8.cpp): a table
    column goes through aqg_grouped_topk, an expression over gathers through aqg_grouped_topk_flat -- ONE grouped call per aggregate
    for all groups, and every group's vector is its slots of that call's result"""
    from test_gpu_emitted import EM, _trade, run
    subprocess.check_call(["make", "-C", EM, "build/topk_q8.so", "build/host_main"], stdout=subprocess.DEVNULL)
    key, v = _trade(50_000, 300) if dataset == "trade_small" else _synthetic()
    gid, ng = mm.first_occurrence_ids(key)
    assert ng == G
    first = np.full(G, len(key), np.int64)
    np.minimum.at(first, gid, np.arange(len(key)))
    by_group = np.argsort(gid, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(gid, minlength=G))])
    run("topk_q8.so", dataset, "dll_q8_top" + suffix, "dll_q8_expr" + suffix, cwd=str(tmp_path))

    def dumped(col, k, order):
        vals, pos, flags = tk.topk(col[by_group], off, k, order)
        assert not flags.any()
        return vals[pos != tk.MISSING]
    for out in ("q8t", "q8e"):
        assert np.array_equal(np.fromfile(tmp_path / f"{out}.out.0", np.int32), key[first])
        calls, groups = (int(t) for t in (tmp_path / f"{out}.calls").read_text().split())
        assert groups == G and calls == 1, "one grouped call for all groups"
    assert np.fromfile(tmp_path / "q8t.out.1", np.int32).tobytes() == dumped(v, 2, ORDER_DESC).tobytes()
    raw = (tmp_path / "q8e.out.1").read_bytes()
    count = int(np.minimum(np.diff(off), 3).sum())
    edt = {4 * count: np.int32, 8 * count: np.int64}[len(raw)]                      # the element-wise operators' own result type
    assert raw == dumped(v.astype(edt) + key.astype(edt), 3, ORDER_ASC).tobytes()
