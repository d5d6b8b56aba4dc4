"""The string dictionary (aqg_str_encode, aqg_str_encode_sharded: aquery2_amd/csrc/strdict.hip) against its model
(tests/strdict_model.py) over the case table of tests/strdict_cases.py, at the row counts either side of 2^16 where the host map
hands over to the device dictionary.  Every case asserts the codes, the distinct count AND the route aqg_str_encode_last reports:
HOST below 2^16 rows, DEVICE from there on, FALLBACK (with the verify kernel's mismatch flag) exactly where the column holds two
different strings under one 64-bit hash and length -- pairs made by inverting the hash (strdict_model.collision).  Should the kernel's
hash change without the model, those pairs stop colliding and their cases fail on the route, not silently pass.
Then the codes through their consumers (group-by, build, join through codes) and through the sharded dictionary exchange with shards
on the device path, on the host map, empty, and falling back."""
import ctypes as C

import numpy as np
import pytest

import checker as ck
import join_keys_model as jkm
import strdict_cases as sc
import strdict_model as sm

pytestmark = pytest.mark.gpu
AQG_ERR_ARG = 3
HOST, DEVICE, FALLBACK = sm.ROUTE_HOST, sm.ROUTE_DEVICE, sm.ROUTE_FALLBACK
N = 70_003


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def ranks():
    import aquery2_amd
    tr = aquery2_amd.ThreadRanks(3)
    yield tr
    tr.close()


class Column:
    """the row pointers of a column: ONE buffer per pool entry (address 0 for None, a NULL pointer) and the n addresses picked by idx"""

    def __init__(self, pool, idx):
        self.bufs = [None if s is None else C.create_string_buffer(s) for s in pool]
        addrs = np.array([0 if b is None else C.addressof(b) for b in self.bufs], dtype=np.uint64)
        self.ptrs = np.ascontiguousarray(addrs[np.asarray(idx, dtype=np.int64)], dtype=np.uint64)
        self.n = int(self.ptrs.size)
        self.strs = [pool[i] for i in np.asarray(idx).tolist()]

    def contents(self):
        return [sm.content(s) for s in self.strs]


def encode(dev, col):
    """aqg_str_encode of a Column: (DevBuf of codes, ndistinct, (route, mismatch))"""
    out = dev.empty(col.n, np.uint32)
    nd = C.c_uint32(0xDEAD)
    dev._chk(dev.lib.aqg_str_encode(dev.ctx, C.c_void_p(col.ptrs.ctypes.data), C.c_uint32(col.n), C.c_void_p(out.ptr), C.byref(nd)), "aqg_str_encode")
    return out, nd.value, dev.str_encode_last()


# ---- the diagnostic itself -------------------------------------------------------------------------------------------------------------
def test_route_diagnostic_is_zero_before_a_call_and_after_an_argument_error():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    try:
        assert d.str_encode_last() == (0, 0)
        col = Column([b"x", b"y"], [0, 1, 0])
        out, nd, last = encode(d, col)
        assert out.to_host().tolist() == [0, 1, 0] and nd == 2 and last == (HOST, 0)
        assert d.lib.aqg_str_encode(d.ctx, None, C.c_uint32(3), C.c_void_p(out.ptr), None) == AQG_ERR_ARG
        assert d.str_encode_last() == (0, 0)
        assert d.lib.aqg_str_encode(d.ctx, C.c_void_p(col.ptrs.ctypes.data), C.c_uint32(3), None, None) == AQG_ERR_ARG
        assert d.str_encode_last() == (0, 0)
        assert d.lib.aqg_str_encode_last(d.ctx, None, None) == AQG_ERR_ARG
        _, nd, last = encode(d, Column([], []))                       # no rows: the host map, no strings
        assert nd == 0 and last == (HOST, 0)
    finally:
        d.close()


# ---- the case table: codes, distinct count and route at every size --------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.SIZES)
@pytest.mark.parametrize("name", sc.NAMES)
def test_codes_and_route_over_the_case_table(gpu, name, n):
    case = sc.case(name, n)
    col = Column(case.pool, case.idx)
    want, want_nd, _ = sm.codes(col.strs)
    out, nd, last = encode(gpu, col)
    got = out.to_host()
    print(name, n, "route", last, "ndistinct", nd, "want", want_nd, "rows that differ", int(np.count_nonzero(got != want)))
    assert np.array_equal(got, want)
    assert nd == want_nd
    assert last == sm.expected_route(n, case.collides)


def test_total_bytes_zero_on_the_device_path(gpu):
    """only empty strings and NULL pointers from 2^16 rows on: nothing to upload, one group, every code 0 -- and the next call on the
    same context is an ordinary one"""
    for pool in ([b""], [None], [None, b""]):
        col = Column(pool, np.arange(sc.SIZES[1]) % len(pool))
        out, nd, last = encode(gpu, col)
        assert nd == 1 and last == (DEVICE, 0) and not out.to_host().any()
    case = sc.case("word_edges", sc.SIZES[1])
    out, nd, last = encode(gpu, Column(case.pool, case.idx))
    want, want_nd, _ = sm.codes(case.strs())
    assert np.array_equal(out.to_host(), want) and nd == want_nd and last == (DEVICE, 0)


# ---- through the consumers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["word_edges", "collision_pair_among_1000"])
def test_groupby_over_the_codes(gpu, oracle, name):
    """Device.key_col(STR) feeding aqg_groupby_agg and aqg_groupby_build beside an int16 key, against the oracle's typed group-by of
    (string, int16): group count, first rows, row-to-group map, exact sums and counts"""
    case = sc.case(name, N)
    strs = case.strs()
    rng = np.random.default_rng(21)
    k2 = rng.integers(-2, 2, N).astype(np.int16)
    v = rng.integers(-1000, 1000, N).astype(np.int32)
    codes = gpu.key_col(ck.STR, strs)
    last = gpu.str_encode_last()
    want_codes, want_nd, _ = sm.codes(strs)
    assert codes.ndistinct == want_nd and np.array_equal(codes.to_host(), want_codes)
    assert last == sm.expected_route(N, case.collides)
    o = oracle.groupby_typed([(ck.STR, strs), (ck.INT16, k2)])
    rev = o["reversemap"].astype(np.int64)
    want_sum = np.bincount(rev, weights=v.astype(np.float64), minlength=o["ngroups"]).astype(np.int64)
    want_cnt = np.bincount(rev, minlength=o["ngroups"])
    kd = [codes, gpu.to_device(k2)]
    for hint in (0, 64):
        gb = gpu.groupby_agg(kd, [ck.RED_SUM, ck.RED_COUNT], [v, v], hint=hint)
        assert gb.ngroups == o["ngroups"]
        assert np.array_equal(gb.first_rows(), o["first_rows"])
        assert ck.i128_to_int(gb.result(0, ck.RED_SUM, ck.INT32)) == want_sum.tolist()
        assert np.array_equal(gb.result(1, ck.RED_COUNT, ck.INT32), want_cnt.astype(np.uint64))
        assert np.array_equal(gb.keys(0, np.uint32), want_codes[o["first_rows"]]) and np.array_equal(gb.keys(1, np.int16), k2[o["first_rows"]])
        gb.destroy()
    b = gpu.groupby_build(kd)
    assert b.ngroups == o["ngroups"]
    assert np.array_equal(b.reversemap(), o["reversemap"])
    assert np.array_equal(b.first_rows(), o["first_rows"])
    assert np.array_equal(b.counts(), want_cnt.astype(np.uint32))
    b.destroy()


@pytest.mark.parametrize("collides", [True, False], ids=["collision", "control"])
def test_join_through_codes(gpu, collides):
    """strings join through the codes of ONE aqg_str_encode over the build rows followed by the probe rows (include/aqg.h): the pairs
    are those of content equality (tests/join_keys_model.py).  The empty string is a key on both sides -- a NULL pointer on the probe
    side -- and of a colliding pair A is on the build side only and B on the probe side only: they do not join."""
    from aquery2_amd import capi
    rng = np.random.default_rng(31)
    nb, npr = 30_001, 40_003                                           # together past 2^16; the probe half starts 4 bytes off a 16-byte line
    (a, b), = sc.pairs(1)
    if not collides:
        b = sm.ordinary16(rng, [a, b])
    common = sc.word_edge_pool() + sc._ordinary(10_000, b"k")
    assert common[0] == b""
    bpool = common + [a]
    ppool = common + [None, b] + sc._ordinary(3_000, b"miss")
    bidx, pidx = sc._cover(rng, nb, len(bpool)), sc._cover(rng, npr, len(ppool))
    build, probe = Column(bpool, bidx), Column(ppool, pidx)
    ptrs = np.ascontiguousarray(np.concatenate([build.ptrs, probe.ptrs]))
    out = gpu.empty(nb + npr, np.uint32)
    nd = C.c_uint32()
    gpu._chk(gpu.lib.aqg_str_encode(gpu.ctx, C.c_void_p(ptrs.ctypes.data), C.c_uint32(nb + npr), C.c_void_p(out.ptr), C.byref(nd)), "aqg_str_encode")
    last = gpu.str_encode_last()
    want_codes, want_nd, _ = sm.codes(build.strs + probe.strs)
    assert nd.value == want_nd and np.array_equal(out.to_host(), want_codes)
    assert last == sm.expected_route(nb + npr, collides)
    bc = capi.DevBuf(gpu, out.ptr, np.uint32, nb, owned=False)
    pc = capi.DevBuf(gpu, out.ptr + 4 * nb, np.uint32, npr, owned=False)
    bside, pside = [(ck.STR, build.contents())], [(ck.STR, probe.contents())]
    m = jkm.matches(bside, pside)
    assert a in build.strs and all(m[i] == [] for i in np.flatnonzero(pidx == ppool.index(b)))           # B finds no partner: A is not B
    assert all(m[i] for i in np.flatnonzero(pidx == ppool.index(None)))                                   # NULL on the probe side meets b"" on the build side
    for kind in (jkm.INNER, jkm.LEFT, jkm.SEMI, jkm.ANTI):
        want_p, want_b = jkm.pairs(kind, bside, pside, m)
        assert gpu.join_keys_count([bc], [pc], kind) == len(want_p)
        pr, br = gpu.join_keys_pairs([bc], [pc], kind)
        assert np.array_equal(pr, want_p), kind
        assert br is None if want_b is None else np.array_equal(br, want_b), kind
    want_p, want_b = jkm.pairs(jkm.INNER, bside, pside, m)
    pr, br = gpu.join_pairs(bc, pc)
    assert np.array_equal(pr, want_p) and np.array_equal(br, want_b)
    assert np.array_equal(gpu.join_keys_lookup([bc], [pc]), jkm.lookup(bside, pside, m))


# ---- the sharded dictionary exchange --------------------------------------------------------------------------------------------------------
def run_sharded(ranks, oracle, shards, want_routes):
    """shards: one (pool, idx) per rank.  Every rank encodes its rows (aqg_str_encode_sharded) and groups the whole table by the codes
    (aqg_groupby_agg_sharded); asserts per rank the codes of the model's ONE dictionary, the global distinct count, the route of the
    rank's local encode, and the sharded group-by against the oracle's group-by of the whole table."""
    cols = [Column(pool, idx) for pool, idx in shards]
    base = np.cumsum([0] + [c.n for c in cols])
    total = int(base[-1])
    v = np.random.default_rng(total).integers(-1000, 1000, total).astype(np.int32)

    def body(rank, dev, comm):
        col = cols[rank]
        out = dev.empty(col.n, np.uint32)
        nd = C.c_uint32(0xDEAD)
        dev._chk(dev.lib.aqg_str_encode_sharded(comm.h, C.c_void_p(col.ptrs.ctypes.data) if col.n else None, C.c_uint32(col.n), C.c_void_p(out.ptr), C.byref(nd)),
                 "aqg_str_encode_sharded")
        last = dev.str_encode_last()
        vd = dev.to_device(np.ascontiguousarray(v[base[rank]:base[rank + 1]]))
        gb = comm.groupby_agg_sharded([out], [ck.RED_SUM, ck.RED_COUNT], [vd, vd], row_base=int(base[rank]), hint=0)
        res = (out.to_host(), nd.value, last, gb.ngroups, gb.first_rows64(), gb.keys(0, np.uint32), gb.result(0, ck.RED_SUM, ck.INT32), gb.result(1, ck.RED_COUNT, ck.INT32))
        gb.destroy()
        return res

    res = ranks.run(body)
    want, want_nd = sm.codes_sharded([c.strs for c in cols])
    o = oracle.groupby_typed([(ck.STR, [s for c in cols for s in c.contents()])])
    assert o["ngroups"] == want_nd and np.array_equal(o["reversemap"], np.concatenate(want))
    rev = o["reversemap"].astype(np.int64)
    want_sum = np.bincount(rev, weights=v.astype(np.float64), minlength=want_nd).astype(np.int64)
    want_cnt = np.bincount(rev, minlength=want_nd)
    for rank, (codes, nd, last, G, first, keys, sums, cnts) in enumerate(res):
        print("rank", rank, "rows", cols[rank].n, "route", last, "ndistinct", nd, "want", want_nd)
        assert np.array_equal(codes, want[rank]), rank
        assert nd == want_nd, rank
        assert last == want_routes[rank], rank
        assert G == want_nd
        assert np.array_equal(first, o["first_rows"].astype(np.int64))
        assert np.array_equal(keys, np.arange(want_nd, dtype=np.uint32))             # the codes ARE the global first-occurrence ids
        assert ck.i128_to_int(sums) == want_sum.tolist()
        assert np.array_equal(cnts, want_cnt.astype(np.uint64))
    return res


def shard_pool():
    return [b"", None] + sc.word_edge_pool()[1:] + sc._ordinary(300, b"sh")


BIG = 66_001                                                            # a shard on the device path


def test_sharded_device_empty_and_host_ranks(ranks, oracle):
    """(66,001, 0, 900) rows: rank 0 builds its dictionary on the device (its first rows come down from the build handle), rank 1 has
    no rows and an empty dictionary, rank 2 takes the host map and holds strings nobody else has"""
    pool = shard_pool()
    late = [b"seen-on-the-last-rank-only-%d" % i for i in range(7)]
    rng = np.random.default_rng(41)
    run_sharded(ranks, oracle, [(pool, sc._cover(rng, BIG, len(pool))), (pool, np.zeros(0, np.int64)), (pool + late, sc._cover(rng, 900, len(pool) + 7))],
                [(DEVICE, 0), (HOST, 0), (HOST, 0)])


def test_sharded_first_occurrence_decided_by_a_host_rank(ranks, oracle):
    """(500, 66,001, 66,001) rows: the global order starts with what the 500 rows of rank 0 hold (host map); most of the device-built
    dictionaries of ranks 1 and 2 are remapped onto it, and the last rank brings strings of its own"""
    pool = shard_pool()
    late = [b"seen-on-the-last-rank-only-%d" % i for i in range(7)]
    rng = np.random.default_rng(42)
    run_sharded(ranks, oracle, [(pool, rng.integers(0, len(pool), 500)), (pool, sc._cover(rng, BIG, len(pool))), (pool + late, sc._cover(rng, BIG, len(pool) + 7))],
                [(HOST, 0), (DEVICE, 0), (DEVICE, 0)])


def test_sharded_colliding_pair_on_two_ranks(ranks, oracle):
    """A on rank 0 only, B on rank 1 only, both on the device path: neither local dictionary sees a collision (DEVICE), and the merge
    -- by content -- gives the two their own global codes"""
    (a, b), = sc.pairs(1)
    pool = sc._ordinary(40, b"sh")
    rng = np.random.default_rng(43)
    res = run_sharded(ranks, oracle, [(pool + [a], sc._cover(rng, BIG, 41)), (pool + [b], sc._cover(rng, BIG, 41)), (pool, sc._cover(rng, 900, 40))],
                      [(DEVICE, 0), (DEVICE, 0), (HOST, 0)])
    assert res[0][1] == 42


def test_sharded_colliding_pair_on_one_rank(ranks, oracle):
    """both strings of the pair on rank 0: its device dictionary is rejected and the host map refills the first rows its dictionary
    is shipped from (FALLBACK); the other ranks are untouched and the merged dictionary is exact"""
    (a, b), = sc.pairs(1)
    pool = sc._ordinary(40, b"sh")
    rng = np.random.default_rng(44)
    res = run_sharded(ranks, oracle, [(pool + [a, b], sc._cover(rng, BIG, 42)), (pool + [b], sc._cover(rng, BIG, 41)), (pool + [a], sc._cover(rng, 900, 41))],
                      [(FALLBACK, 1), (DEVICE, 0), (HOST, 0)])
    assert res[0][1] == 42


def test_sharded_rank_of_empty_strings_only(ranks, oracle):
    """rank 1 holds nothing but b"" on the device path (no bytes to upload; its dictionary is the one NUL byte) and is the first to
    hold it; rank 2 holds nothing but NULL pointers, the same string"""
    pool = sc._ordinary(40, b"sh")
    rng = np.random.default_rng(45)
    run_sharded(ranks, oracle, [(pool, sc._cover(rng, BIG, 40)), ([b""], np.zeros(BIG, np.int64)), ([None], np.zeros(700, np.int64))],
                [(DEVICE, 0), (DEVICE, 0), (HOST, 0)])


def test_sharded_one_string_everywhere(ranks, oracle):
    res = run_sharded(ranks, oracle, [([b"the-only-one"], np.zeros(BIG, np.int64)), ([b"the-only-one"], np.zeros(900, np.int64)), ([b"the-only-one"], np.zeros(BIG, np.int64))],
                      [(DEVICE, 0), (HOST, 0), (DEVICE, 0)])
    assert all(r[1] == 1 and not r[0].any() for r in res)
