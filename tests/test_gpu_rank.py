"""aqg_rank / aqg_grouped_rank / aqg_grouped_rank_flat / aqg_rank_last (rank.hip): where every row stands in its slice.  Everything goes
through the C-ABI and is compared BIT FOR BIT with the model of tests/rank_model.py -- integer ranks exact, doubles equal as bit
patterns.  The cases live in tests/rank_cases.py on the geometry read from the code; tests/test_rank_model.py shows on the CPU that the
model equals pandas' recorded answers and that the cases refuse every planted mistake."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rank_cases as rc
import rank_model as rm
from aquery2_amd.capi import (BOOL, DATE, INT128, ORDER_ASC, ORDER_DESC, ORDER_NEG, RANK_ROUTE_SMALL, RANK_ROUTE_SORTED, UINT64, UINT128)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_DTYPE, ERR_ARG = 2, 3
assert (ORDER_ASC, ORDER_DESC) == (rm.ASC, rm.DESC)


@pytest.fixture(scope="module")
def dev():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def upload(dev, x):
    """the column on the device; bool columns tagged BOOL"""
    buf = dev.to_device(x)
    if np.asarray(x).dtype == np.bool_:
        buf._tag = BOOL
    return buf


def calls_of(c):
    """every (method, k) a case is asked: each method once, NTILE with every k of the case"""
    return [(m, 0) for m in rm.METHODS if m != rm.NTILE] + [(rm.NTILE, k) for k in c.ks]


def hold_case(dev, c, gb=None):
    """every method and both orders of one case against the model, through the flat entry or both grouped entries; the routes it took"""
    n = len(c.x)
    xd = upload(dev, c.x)
    xr = upload(dev, c.x_row) if gb is not None else None
    outs = {np.dtype(np.uint32): dev.empty(n, np.uint32), np.dtype(np.float64): dev.empty(n, np.float64)}
    routes = 0
    for order in (ORDER_ASC, ORDER_DESC):
        five = rm.five_sorted(c.x, c.starts, order)
        for method, k in calls_of(c):
            want = rm.finish(method, k, five)
            out = outs[rm.out_dtype(method)]
            if gb is None:
                got = {"flat": dev.rank(xd, method, order, k, keep=True, out=out).to_host()}
            else:
                got = {"row": dev.grouped_rank(gb, xr, method, order, k, keep=True, out=out).to_host(),
                       "flat": dev.grouped_rank(gb, xd, method, order, k, flat=True, keep=True, out=out).to_host()}
            r, tile = dev.rank_last()
            assert tile == rc.ET
            routes |= r
            for entry, g in got.items():
                if not rm.same_bits(g, want):
                    bad = np.flatnonzero(g.view(np.uint64 if g.dtype.itemsize == 8 else np.uint32) != want.view(np.uint64 if g.dtype.itemsize == 8 else np.uint32))
                    pytest.fail("%s/%s %s order %d k %d: %d rows differ, first at %d: got %r want %r" % (
                        c.name, entry, rm.METHOD_NAMES[method], order, k, len(bad), bad[0], g[bad[0]], want[bad[0]]))
    assert np.array_equal(xd.to_host().view(np.uint8), c.x.view(np.uint8)), (c.name, "the input was modified")
    return routes


FLAT = rc.flat_cases()
GROUPED = rc.grouped_cases()


@pytest.mark.parametrize("dt", sorted({c.dtype.name for c in FLAT}))
def test_flat_grid(dev, dt):
    """every n of the grid (the SMALL threshold, emit-tile edges, the one-workgroup sort's last size), ties / distinct / equal / special
    values, every method, both orders"""
    cases = [c for c in FLAT if c.dtype.name == dt]
    assert cases
    for c in cases:
        routes = hold_case(dev, c)
        assert routes == (RANK_ROUTE_SMALL if len(c.x) <= rc.SMALL_MAX else RANK_ROUTE_SORTED), c.name


def expected_routes(c):
    sizes = np.diff(np.append(c.starts, len(c.x)))
    return (RANK_ROUTE_SMALL if (sizes <= rc.SMALL_MAX).any() else 0) | (RANK_ROUTE_SORTED if (sizes > rc.SMALL_MAX).any() else 0)


@pytest.mark.parametrize("layout", sorted({c.name.split("-")[1] for c in GROUPED}))
def test_grouped(dev, layout):
    """group sizes on both sides of the SMALL switch, SMALL groups across the staging tiles, one group over three emit tiles beside groups
    of one row, every row its own group, one group, G on both sides of 256, group starts and tie runs on emit-tile edges, SMALL and SORTED
    groups in one call -- through both grouped entries, with the route mask read back"""
    cases = [c for c in GROUPED if c.name.split("-")[1] == layout]
    assert cases
    for c in cases:
        gb = dev.groupby_build([c.keys_row])
        assert gb.ngroups == len(c.starts)
        assert np.array_equal(dev.group_offsets(gb)[:len(c.starts)], c.starts)
        assert hold_case(dev, c, gb) == expected_routes(c), c.name
        gb.destroy()
    if layout == "mixed":
        assert expected_routes(cases[0]) == RANK_ROUTE_SMALL | RANK_ROUTE_SORTED


def test_many_tiles_and_reproducible(dev):
    """70 000 rows (35 emit tiles, the sort's digit passes), flat and as groups of 1000; the same call twice into different buffers is
    byte-equal"""
    c = rc.big_case()
    n = len(c.x)
    xd = dev.to_device(c.x)
    keys = np.repeat(np.arange(-(-n // 1000), dtype=np.int32), 1000)[:n]
    gb = dev.groupby_build([keys])
    starts = np.arange(0, n, 1000)
    x_row = np.empty_like(c.x)                                       # the flat layout lists a group's rows by descending row id
    perm = np.concatenate([np.arange(min(s + 1000, n) - 1, s - 1, -1) for s in starts])
    x_row[perm] = c.x
    xr = dev.to_device(x_row)
    for order in (ORDER_ASC, ORDER_DESC):
        five, gfive = rm.five_sorted(c.x, c.starts, order), rm.five_sorted(c.x, starts, order)
        for method, k in [(m, 0) for m in rm.METHODS if m != rm.NTILE] + [(rm.NTILE, 7), (rm.NTILE, n - 1)]:
            a, b = dev.rank(xd, method, order, k), dev.rank(xd, method, order, k)
            assert rm.same_bits(a, rm.finish(method, k, five)), (method, order, k)
            assert a.tobytes() == b.tobytes()
            a, b = dev.grouped_rank(gb, xr, method, order, k), dev.grouped_rank(gb, xd, method, order, k, flat=True)
            assert rm.same_bits(a, rm.finish(method, k, gfive)), (method, order, k)
            assert a.tobytes() == b.tobytes()
    assert dev.rank_last() == (RANK_ROUTE_SORTED, rc.ET)
    gb.destroy()


# ---- one route alone: the switch is read once per process ------------------------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path.insert(0, "tests")
import numpy as np
import aquery2_amd, rank_cases as rc, rank_model as rm
want_routes, layouts = int(sys.argv[1]), sys.argv[2].split(",")
dev = aquery2_amd.Device(0)
seen = 0
for c in rc.grouped_cases():
    if c.name.split("-")[1] not in layouts or c.dtype not in (np.dtype(np.int32), np.dtype(np.float64)):
        continue
    gb = dev.groupby_build([c.keys_row])
    for order in (rm.ASC, rm.DESC):
        five = rm.five_sorted(c.x, c.starts, order)
        for method, k in [(m, 0) for m in rm.METHODS if m != rm.NTILE] + [(rm.NTILE, k) for k in c.ks]:
            for flat, x in ((True, c.x), (False, c.x_row)):
                got = dev.grouped_rank(gb, x, method, order, k, flat=flat)
                assert rm.same_bits(got, rm.finish(method, k, five)), (c.name, method, order, k, flat)
                assert dev.rank_last()[0] == want_routes, (c.name, dev.rank_last())
                seen += 1
    gb.destroy()
assert dev.rank(np.arange(300, dtype=np.int32)[::-1].copy(), rm.FIRST).tolist() == list(range(300, 0, -1)) and dev.rank_last()[0] == want_routes
assert seen > 50
print("OK", seen)
"""


@pytest.mark.parametrize("small_max,routes,layouts", [("0", RANK_ROUTE_SORTED, "threshold,singletons,small_sizes,straddle"),
                                                       (str(rc.SMALL_CAP), RANK_ROUTE_SMALL, "threshold,small_sizes,straddle,g257")],
                         ids=["all_sorted", "all_small"])
def test_one_route_alone(small_max, routes, layouts):
    """AQG_SELECT_SMALL_MAX = 0 sends every group, groups of one row included, through the sort and the emit pass; = 512 sends groups of
    up to 512 rows through the LDS route.  Fresh child processes: the switch is read once.  Both give the model's answers."""
    out = subprocess.run([sys.executable, "-c", CHILD, str(routes), layouts], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, AQG_SELECT_SMALL_MAX=small_max), cwd=ROOT)
    assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])


# ---- the recorded answers of pandas, on the device ---------------------------------------------------------------------------------------
def test_pandas_golden(dev):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "rank_pandas.json")))
    for case in golden["cases"]:
        dt = np.dtype(case["dtype"])
        x = np.array(case["bits"], {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize]).view(dt)
        sizes = case["sizes"]
        if len(sizes) > 1:
            g = rc.grouped_case("golden", sizes, x)
            gb = dev.groupby_build([g.keys_row])
        for order, oname in ((ORDER_ASC, "asc"), (ORDER_DESC, "desc")):
            for method in rm.METHODS:
                for k in (golden["ks"] if method == rm.NTILE else [0]):
                    w = case["results"][oname][rm.METHOD_NAMES[method]]
                    w = w[str(k)] if method == rm.NTILE else w
                    w = np.array(w, np.float64) if rm.is_double(method) else np.array(w, np.uint32)
                    got = dev.rank(upload(dev, x), method, order, k) if len(sizes) == 1 else dev.grouped_rank(gb, upload(dev, g.x_row), method, order, k)
                    assert rm.same_bits(got, w), (case["dtype"], sizes, oname, method, k)
        if len(sizes) > 1:
            gb.destroy()


# ---- errors --------------------------------------------------------------------------------------------------------------------------
CANARY = 0x5EEDFACECAFEBEEF


def canary(dev, n):
    return dev.to_device(np.full(n, CANARY, np.uint64))


def untouched(buf):
    return bool((buf.to_host() == np.uint64(CANARY)).all())


def test_errors_write_nothing(dev):
    n = 1000
    x = dev.to_device(np.arange(n, dtype=np.int32))
    keys = dev.to_device((np.arange(n) % 7).astype(np.int32))
    gb = dev.groupby_build([keys])
    agg = dev.groupby_agg([keys], [0], [x])
    out = canary(dev, n)
    lib, ctx = dev.lib, dev.ctx

    def flat(method, order, k, t, xp, nn, op):
        return lib.aqg_rank(ctx, method, order, k, t, xp, nn, op)

    def grouped(h, method, order, k, t, xp, op):
        return [fn(ctx, h, method, order, k, t, xp, op) for fn in (lib.aqg_grouped_rank, lib.aqg_grouped_rank_flat)]

    for method in (-1, 8, 100):
        assert flat(method, ORDER_ASC, 1, x.tag, x.ptr, n, out.ptr) == ERR_ARG
        assert grouped(gb.h, method, ORDER_ASC, 1, x.tag, x.ptr, out.ptr) == [ERR_ARG, ERR_ARG]
    for order in (ORDER_NEG, -1, 3):
        assert flat(rm.MIN, order, 0, x.tag, x.ptr, n, out.ptr) == ERR_ARG
        assert grouped(gb.h, rm.MIN, order, 0, x.tag, x.ptr, out.ptr) == [ERR_ARG, ERR_ARG]
    assert flat(rm.NTILE, ORDER_ASC, 0, x.tag, x.ptr, n, out.ptr) == ERR_ARG                      # NTILE needs k >= 1 ...
    assert grouped(gb.h, rm.NTILE, ORDER_ASC, 0, x.tag, x.ptr, out.ptr) == [ERR_ARG, ERR_ARG]
    for t in (INT128, UINT128, DATE):
        assert flat(rm.MIN, ORDER_ASC, 0, t, x.ptr, n, out.ptr) == ERR_DTYPE
        assert grouped(gb.h, rm.MIN, ORDER_ASC, 0, t, x.ptr, out.ptr) == [ERR_DTYPE, ERR_DTYPE]
    assert grouped(agg.h, rm.MIN, ORDER_ASC, 0, x.tag, x.ptr, out.ptr) == [ERR_ARG, ERR_ARG]     # not a handle of aqg_groupby_build
    assert flat(rm.MIN, ORDER_ASC, 0, x.tag, None, n, out.ptr) == ERR_ARG
    assert flat(rm.MIN, ORDER_ASC, 0, x.tag, x.ptr, n, None) == ERR_ARG
    assert untouched(out)
    # out overlapping x: the column itself, its tail (4-byte and 8-byte results)
    xd = canary(dev, n)
    for method in (rm.MIN, rm.AVERAGE):
        assert flat(method, ORDER_ASC, 0, UINT64, xd.ptr, n, xd.ptr) == ERR_ARG
        assert flat(method, ORDER_ASC, 0, UINT64, xd.ptr, n, xd.ptr + 8 * (n - 1)) == ERR_ARG
        assert grouped(gb.h, method, ORDER_ASC, 0, UINT64, xd.ptr, xd.ptr) == [ERR_ARG, ERR_ARG]
    assert untouched(xd)
    # nothing to do
    assert flat(rm.MIN, ORDER_ASC, 0, x.tag, None, 0, None) == 0
    empty = dev.groupby_build([np.zeros(0, np.int32)])
    assert grouped(empty.h, rm.DENSE, ORDER_DESC, 0, x.tag, None, None) == [0, 0]
    assert untouched(out)
    # ... and every other method ignores k; BOOL ranks as 0 < 1
    assert np.array_equal(dev.rank(x, rm.MIN, k=0), dev.rank(x, rm.MIN, k=12345))
    b = np.array([True, False, True, False, False])
    bd = upload(dev, b)
    assert bd.tag == BOOL and dev.rank(bd, rm.MIN).tolist() == [4, 1, 4, 1, 1] and dev.rank(bd, rm.FIRST, ORDER_DESC).tolist() == [1, 3, 2, 4, 5]
    for h in (gb, agg, empty):
        h.destroy()


def test_one_host_read_per_handle(dev):
    """a handle's first grouped call reads the SORTED route's row count; later calls through it give the same answers from the cached
    count, and a rebuild through a fresh handle of another shape reads its own"""
    c = next(c for c in GROUPED if c.name == "grouped-mixed-int32-ties")
    gb = dev.groupby_build([c.keys_row])
    want = rm.rank(c.x, c.starts, rm.DENSE)
    for _ in range(3):
        assert rm.same_bits(dev.grouped_rank(gb, c.x, rm.DENSE, flat=True), want)
        assert dev.rank_last()[0] == RANK_ROUTE_SMALL | RANK_ROUTE_SORTED
    c2 = next(c for c in GROUPED if c.name == "grouped-small_sizes-int32-ties")
    gb2 = dev.groupby_build([c2.keys_row])
    assert rm.same_bits(dev.grouped_rank(gb2, c2.x, rm.DENSE, flat=True), rm.rank(c2.x, c2.starts, rm.DENSE))
    assert dev.rank_last()[0] == RANK_ROUTE_SMALL
    assert rm.same_bits(dev.grouped_rank(gb, c.x, rm.MAX, flat=True), rm.rank(c.x, c.starts, rm.MAX))
    gb.destroy()
    gb2.destroy()


def test_emitted_group_loop(tmp_path):
    """tests/emitted/ranks.cpp over host_main's synthetic dataset (2e5 rows): `rankof(c[vecs[g]], col[g])`, `dense_rank(..., true)`,
    `percent_rank(...)` and `ntile(4, ...)` in the generated group loop cost ONE aqg_grouped_rank_flat per (column, method, order), at
    1000 groups and at 10; a `subvec(0, 2)` view of the temporary takes the per-group path and gives the per-group answer"""
    from test_gpu_emitted import EM, run
    from test_gpu_quantiles import _synthetic
    import quantile_model as qm
    subprocess.check_call(["make", "-C", EM, "build/ranks.so", "build/host_main"], stdout=subprocess.DEVNULL)
    a, c = _synthetic()
    run("ranks.so", "synthetic", "dll_rank_flat", "dll_rank_group", "dll_rank_group10", cwd=str(tmp_path))
    n = len(c)
    whole = np.zeros(1, np.int64)
    for j, (method, order, k) in enumerate(((rm.MIN, rm.ASC, 0), (rm.AVERAGE, rm.ASC, 0), (rm.NTILE, rm.ASC, 7), (rm.FIRST, rm.DESC, 0))):
        got = np.fromfile(tmp_path / ("rankf.out.%d" % j), rm.out_dtype(method))
        assert rm.same_bits(got, rm.rank(c, whole, method, order, k)), ("emitted flat", j)
    for name, key, G in (("rankg", a, 1000), ("rankg10", a % 10, 10)):
        gid, ng = qm.first_occurrence_ids(key)
        assert ng == G
        # the group loop's row lists: groups in first-occurrence order, a group's rows in descending row id (the flat layout)
        order = np.lexsort((-np.arange(n), gid))
        starts = np.flatnonzero(np.diff(gid[order], prepend=-1))
        first = np.full(G, n, np.int64)
        np.minimum.at(first, gid, np.arange(n))
        assert np.array_equal(np.fromfile(tmp_path / (name + ".out.0"), np.int32), key[first])
        cf = c[order]
        for j, (method, o, k) in enumerate(((rm.MIN, rm.ASC, 0), (rm.DENSE, rm.DESC, 0), (rm.PERCENT, rm.ASC, 0), (rm.NTILE, rm.ASC, 4)), start=1):
            got = np.fromfile(tmp_path / ("%s.out.%d" % (name, j)), rm.out_dtype(method))
            assert rm.same_bits(got, rm.rank(cf, starts, method, o, k)), (name, j)
        assert np.array_equal(np.fromfile(tmp_path / (name + ".out.6"), np.uint32), np.fromfile(tmp_path / (name + ".out.1"), np.uint32))
        # the two-row views, one per group, each the per-group answer of its first two rows
        sub = np.fromfile(tmp_path / (name + ".out.5"), np.uint32)
        counts = np.diff(np.append(starts, n))
        want = []
        for s0, cnt in zip(starts, counts):
            want += [1] if cnt < 2 else [1 + int(cf[s0 + 1] < cf[s0]), 1 + int(cf[s0] < cf[s0 + 1])]
        assert np.array_equal(sub, np.array(want, np.uint32))
        calls, groups = (int(v) for v in (tmp_path / (name + ".calls")).read_text().split())
        assert groups == G and calls == 4, "one grouped call per (column, method, order), whatever the number of groups"
