"""The hash joins pinned to tests/join_model.py: aqg_join_lookup, aqg_join_count / aqg_join_pairs (join.hip) and the fused
aqg_join_groupby_sum (groupby_starjoin.hip) -- keys equal to the tables' empty marks, collision chains that wrap past the last
slot, duplicate build keys, every table route and size step, unaligned column views, the accumulators at their limits and the
error returns.  Every result is an integer, a row id or a status: everything is compared for equality."""
import ctypes as C

import numpy as np
import pytest

import checker as ck
import join_model as jm

pytestmark = pytest.mark.gpu
KEY_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64]
NONE = jm.NONE
M32 = 0xFFFFFFFF
FIB = 0x9E3779B1
FIB_INV = pow(FIB, -1, 1 << 32)
AQG_OK, AQG_ERR_DTYPE, AQG_ERR_ARG, AQG_ERR_OVERFLOW = 0, 2, 3, 6
nm = lambda d: np.dtype(d).name


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def full_range(rng, dt, n):
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def distinct_keys(rng, dt, n, exclude=()):
    """n distinct keys from the whole range of the type, in random order"""
    info = np.iinfo(dt)
    span = int(info.max) - int(info.min) + 1
    assert n + len(exclude) <= span
    if span <= 1 << 16:
        k = np.arange(int(info.min), int(info.max) + 1).astype(dt)
    else:
        k = np.unique(full_range(rng, dt, n + n // 8 + 64))
    k = k[~np.isin(k, np.array(list(exclude), dtype=dt))] if len(exclude) else k
    assert len(k) >= n
    return rng.permutation(k)[:n]


def mixed_probe(rng, build, n, dt):
    """about two thirds of the probes hit, the rest are drawn from the whole range (misses for every wide type)"""
    p = full_range(rng, dt, n)
    if len(build):
        hit = rng.random(n) < 0.67
        p[hit] = build[rng.integers(0, len(build), int(hit.sum()))]
    return p


# ---- aqg_join_lookup ------------------------------------------------------------------------------------------------------
# the key whose 64-bit image equals the table's empty mark (every signed -1, the uint64 maximum), and the all-ones keys of the
# narrower unsigned types, which are ordinary keys
ALL_ONES = [(np.int8, -1), (np.int16, -1), (np.int32, -1), (np.int64, -1), (np.uint64, 2**64 - 1), (np.uint8, 255), (np.uint16, 65535), (np.uint32, 2**32 - 1)]


@pytest.mark.parametrize("npr", [70_001, 5000], ids=["lds", "hbm"])
@pytest.mark.parametrize("dt,special", ALL_ONES, ids=[nm(d) for d, _ in ALL_ONES])
def test_lookup_all_ones_key(gpu, dt, special, npr):
    rng = np.random.default_rng(31)
    nb = 2000
    info = np.iinfo(dt)
    others = np.array([v for v in range(int(info.min), int(info.max) + 1) if v != special], dtype=dt) if info.bits == 8 else None
    base = rng.choice(others, nb) if others is not None else distinct_keys(rng, dt, nb, exclude=(special,))
    probe = mixed_probe(rng, base, npr, dt)
    probe[probe == dt(special)] = base[0]
    at = np.concatenate([[0, 1, 7, 8, npr - 1, npr - 2], rng.integers(0, npr, 40)])          # vector body and scalar tail rows
    probe[at] = dt(special)
    for rows, want in (((1234,), 1234), ((nb - 1, 700, 3), 3), ((), NONE)):
        build = base.copy()
        build[list(rows)] = dt(special)
        got = gpu.join_lookup(build, probe)
        assert np.all(got[at] == want), (dt, rows, got[at])
        assert np.array_equal(got, jm.lookup(build, probe)), (dt, rows)


@pytest.mark.parametrize("dt", KEY_DTYPES, ids=nm)
def test_lookup_duplicate_build_keys_lowest_row_wins(gpu, dt):
    rng = np.random.default_rng(32)
    nb, info = 5000, np.iinfo(dt)
    keys = distinct_keys(rng, dt, 700 if info.bits > 8 else 200)
    keys[:2] = [info.min, info.max]
    if info.min < 0:
        keys[2] = -1
    keys = np.unique(keys)
    build = rng.choice(keys, nb)
    assert len(np.unique(build)) < nb // 5
    for npr in (20_000, 70_001):
        probe = mixed_probe(rng, build, npr, dt)
        assert np.array_equal(gpu.join_lookup(build, probe), jm.lookup(build, probe)), (dt, npr)


TABLE_NB = [0, 1, 7, 8, 9, 512, 513, 2047, 2048, 2049, 100_003, 1_000_003]


@pytest.mark.parametrize("nb", TABLE_NB)
@pytest.mark.parametrize("dt", [np.int32, np.int64], ids=nm)
def test_lookup_table_steps_and_routes(gpu, dt, nb):
    """the table sizes at which the LDS copy changes its occupancy (513) or gives way to the HBM table (2049), the probe counts at
    which the LDS route starts (65,536) -- distinct keys over the whole range, a third of the probes miss"""
    rng = np.random.default_rng(33 + nb)
    build = distinct_keys(rng, dt, nb)
    sizes = [1, 65_535, 65_536, 65_543]
    probes = [mixed_probe(rng, build, n, dt) for n in sizes]
    want = np.split(jm.lookup(build, np.concatenate(probes)), np.cumsum(sizes)[:-1])
    bd = gpu.to_device(build)
    for p, w in zip(probes, want):
        got = gpu.join_lookup(bd, p)
        assert np.array_equal(got, w), (dt, nb, len(p))
        if nb == 0:
            assert np.all(got == NONE)


def jslot(keys, bits):
    """join.hip's jslot, restated: the home slot of a key's 64-bit image in a table of 2^bits slots"""
    k = np.asarray(keys).astype(np.int64).view(np.uint64) if np.asarray(keys).dtype.kind == "i" else np.asarray(keys).astype(np.uint64)
    lo, hi = k & np.uint64(M32), k >> np.uint64(32)
    h = ((lo ^ ((hi * np.uint64(0x85EBCA6B)) & np.uint64(M32))) * np.uint64(FIB)) & np.uint64(M32)
    return (h >> np.uint64(32 - bits)).astype(np.int64)


def fib_slot(keys, bits):
    """groupby_dev.hpp's fib_slot, restated"""
    return (((np.asarray(keys).astype(np.uint64) * np.uint64(FIB)) & np.uint64(M32)) >> np.uint64(32 - bits)).astype(np.int64)


def keys_with_home(slot, bits, j):
    """32-bit keys whose Fibonacci-hash home in a table of 2^bits slots is `slot`: the hash is a multiplication by an odd constant
    modulo 2^32, so its inverse maps the wanted products back to keys (j < 2^(32-bits) picks the key within the slot)"""
    j = np.asarray(j, dtype=np.uint64)
    assert j.max() < 1 << (32 - bits)
    return (((np.uint64(slot << (32 - bits)) + j) * np.uint64(FIB_INV)) & np.uint64(M32)).astype(np.uint32)


@pytest.mark.parametrize("nb", [12, 1500, 3000], ids=["lds_small", "lds_large", "hbm"])
@pytest.mark.parametrize("dt", [np.uint32, np.int64], ids=nm)
def test_lookup_collision_chain_wraps_past_the_last_slot(gpu, dt, nb):
    """WHITE BOX on jslot (join.hip): every build key has the LAST slot of the table as its home, so the chain of nb keys wraps
    to slot 0 and runs on to slot nb - 2.  Misses with the same home, and misses whose home lies inside the chain, must walk to
    the first empty slot and come back with NONE.  The 8-byte keys carry several high words (a negative one too), folded out of
    the low word the way jslot folds them in."""
    rng = np.random.default_rng(34)
    cap = 16
    while cap < 2 * nb:                                                  # pow2_at_least(2 * nb) of make_table
        cap <<= 1
    bits, last = cap.bit_length() - 1, cap - 1
    low = keys_with_home(last, bits, np.arange(nb + 400))
    inside = np.concatenate([keys_with_home(s, bits, np.arange(3)) for s in (0, 1, nb // 2, max(nb - 2, 0))])
    if dt == np.uint32:
        same_home, inside_miss = low, inside
    else:
        def widen(lo32, hi_words):
            hi = np.asarray(hi_words, dtype=np.uint64)[np.arange(len(lo32)) % len(hi_words)]
            lo = lo32.astype(np.uint64) ^ ((hi * np.uint64(0x85EBCA6B)) & np.uint64(M32))
            return ((hi << np.uint64(32)) | lo).view(np.int64)
        same_home, inside_miss = widen(low, [0, 0x12345, M32, 0x80000000, 7]), widen(inside, [M32, 3])
        assert -1 not in same_home.tolist() and -1 not in inside_miss.tolist()
    build, miss = rng.permutation(same_home[:nb]), np.concatenate([same_home[nb:], inside_miss])
    # the premise, visible: one home slot for the whole build side and the first group of misses, homes inside the chain for the rest
    assert np.all(jslot(build, bits) == last) and np.all(jslot(same_home[nb:], bits) == last)
    assert set(jslot(inside_miss, bits).tolist()) <= set(range(0, max(nb - 1, 1)))
    assert len(np.unique(build)) == nb and not np.isin(miss, build).any()
    npr = 70_001
    probe = np.concatenate([build, miss, rng.choice(np.concatenate([build, miss]), npr - nb - len(miss))]).astype(dt)
    got = gpu.join_lookup(build.astype(dt), probe)
    assert np.all(got[nb:nb + len(miss)] == NONE)
    assert np.array_equal(got, jm.lookup(build.astype(dt), probe))


def test_lookup_keys_that_differ_in_the_high_word_only(gpu):
    rng = np.random.default_rng(35)
    c = 0x5EED
    build = rng.permutation(c + (np.arange(200_000, dtype=np.int64) << 32))
    probe = np.concatenate([build[:40_000], c + (np.arange(200_000, 215_000, dtype=np.int64) << 32), build[:15_001] + 1])
    probe = rng.permutation(probe)
    assert len(probe) == 70_001
    assert np.array_equal(gpu.join_lookup(build, probe), jm.lookup(build, probe))


@pytest.mark.parametrize("npr", [15, 16, 17, 65_541])
@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.int32, np.int64], ids=nm)
def test_lookup_offset_views(gpu, dt, npr):
    """probe and output pointers advanced by one element: off the vector width, so the rows take the scalar loop"""
    rng = np.random.default_rng(36)
    build = distinct_keys(rng, dt, 300 if np.iinfo(dt).bits > 8 else 100)
    probe = mixed_probe(rng, build, npr + 1, dt)
    bd, pd = gpu.to_device(build), gpu.to_device(probe)
    fill = np.full(npr + 2, 0xA5A5A5A5, np.uint32)
    for poff, ooff in ((1, 1), (1, 0), (0, 1)):
        od = gpu.to_device(fill)
        rc = gpu.lib.aqg_join_lookup(gpu.ctx, bd.tag, C.c_void_p(bd.ptr), C.c_uint32(bd.n), C.c_void_p(pd.ptr + poff * probe.itemsize), C.c_uint32(npr),
                                     C.c_void_p(od.ptr + 4 * ooff))
        assert rc == AQG_OK
        got = od.to_host()
        assert np.array_equal(got[ooff:ooff + npr], jm.lookup(build, probe[poff:poff + npr])), (dt, npr, poff, ooff)
        assert np.all(got[:ooff] == 0xA5A5A5A5) and np.all(got[ooff + npr:] == 0xA5A5A5A5)      # nothing written around the view


# ---- aqg_join_count / aqg_join_pairs --------------------------------------------------------------------------------------
def check_pairs(gpu, build, probe):
    want_p, want_b = jm.pairs(build, probe)
    assert gpu.join_count(build, probe) == jm.count(build, probe) == len(want_p)
    pr, br = gpu.join_pairs(build, probe)
    assert np.array_equal(pr, want_p) and np.array_equal(br, want_b)
    return pr, br


@pytest.mark.parametrize("nb,distinct", [(300_000, 200_000), (1_100_000, 500_000)], ids=["hashed_build", "partitioned_build"])
@pytest.mark.parametrize("dt", [np.int32, np.int64], ids=nm)
def test_pairs_many_distinct_build_keys(gpu, dt, nb, distinct):
    """the build side grouped by aqg_groupby_build beyond its smallest plan.  The build's handle stays inside join_core, so its route is
    not read back here; it is inferred from make_agg_plan: a build of n >= 2^20 rows takes the partition plans once its hint passes
    3072, which the un-hinted call reaches on its first retry (1024 -> 16384) with 5e5 distinct keys."""
    rng = np.random.default_rng(37)
    keys = distinct_keys(rng, dt, distinct)
    build = keys[rng.integers(0, distinct, nb)]
    probe = mixed_probe(rng, build, 100_003, dt)
    check_pairs(gpu, build, probe)


@pytest.mark.parametrize("dt,special", [(np.int64, -1), (np.uint64, 2**64 - 1)], ids=["int64", "uint64"])
def test_pairs_all_ones_key_with_duplicates_and_one_heavy_key(gpu, dt, special):
    rng = np.random.default_rng(38)
    nb, npr, heavy = 60_000, 10_000, dt(424242)
    others = distinct_keys(rng, dt, nb, exclude=(special, 424242))
    build = others.copy()
    build[rng.permutation(nb)[:50_000]] = heavy                           # one ordinary key on 50,000 of the 60,000 rows
    build[[59_999, 31_000, 12, 4000, 4001]] = dt(special)
    probe = mixed_probe(rng, others, npr, dt)
    assert not np.isin(probe, np.array([heavy, dt(special)])).any()
    probe[[0, 5000, npr - 1]] = dt(special)
    probe[[1, 17, 4096, npr - 2]] = heavy
    pr, br = check_pairs(gpu, build, probe)
    assert br[pr == 0].tolist() == br[pr == 5000].tolist() == br[pr == npr - 1].tolist() == [12, 4000, 4001, 31_000, 59_999]
    for row in (1, 17, 4096, npr - 2):
        assert np.array_equal(br[pr == row], np.nonzero(build == heavy)[0])
    assert int((build == heavy).sum()) >= 49_995
    same = pr[1:] == pr[:-1]
    assert np.all(br[1:][same] > br[:-1][same])                           # ascending build rows within every probe row


def raw_pairs(gpu, bd, pd, out_p, out_b, capacity):
    m = C.c_uint64(0xDEAD)
    rc = gpu.lib.aqg_join_pairs(gpu.ctx, bd.tag, C.c_void_p(bd.ptr), C.c_uint32(bd.n), C.c_void_p(pd.ptr), C.c_uint32(pd.n),
                                C.c_void_p(out_p.ptr) if out_p is not None else None, C.c_void_p(out_b.ptr) if out_b is not None else None,
                                C.c_uint64(capacity), C.byref(m))
    return rc, m.value


def _count_int16_duplicates(rng):
    return rng.integers(0, 40, 500).astype(np.int16), rng.integers(-5, 45, 2000).astype(np.int16)


def _count_all_ones_int64(rng):
    build = rng.choice(distinct_keys(rng, np.int64, 900, exclude=(-1,)), 3000)
    probe = mixed_probe(rng, build, 5003, np.int64)
    build[[2999, 1500, 12]] = -1
    probe[[0, 2500, 5002]] = -1
    return build, probe


def _count_hashed_build(rng):
    build = distinct_keys(rng, np.int32, 200_000)[rng.integers(0, 200_000, 300_000)]
    return build, mixed_probe(rng, build, 100_003, np.int32)


COUNT_CASES = {"int16_duplicates": _count_int16_duplicates, "all_ones_int64": _count_all_ones_int64, "hashed_build": _count_hashed_build}


@pytest.mark.parametrize("name", list(COUNT_CASES))
def test_count_without_pairs(gpu, name):
    """aqg_join_count builds no row lists (no aqg_groupby_postproc): its count is the model's and the m_host of aqg_join_pairs on the same
    columns, and the context it leaves behind still groups -- no handle or buffer of the count-only call is left in the way"""
    rng = np.random.default_rng(50)
    build, probe = COUNT_CASES[name](rng)
    gk, gv = rng.integers(0, 50, 100_000).astype(np.int32), rng.integers(-1000, 1000, 100_000).astype(np.int32)
    bd, pd = gpu.to_device(build), gpu.to_device(probe)
    want = jm.count(build, probe)
    assert want > 0 and gpu.join_count(bd, pd) == want
    gb = gpu.groupby_agg([gk], [ck.RED_SUM], [gv])
    keys, first = np.unique(gk, return_index=True)
    by_first = np.argsort(first)
    assert gb.keys(0, np.int32).tolist() == keys[by_first].tolist() and gb.first_rows().tolist() == first[by_first].tolist()
    assert ck.i128_to_int(gb.result(0, ck.RED_SUM, ck.INT32)) == [int(gv[gk == k].sum()) for k in keys[by_first]]
    gb.destroy()
    op, ob = gpu.empty(want, np.uint32), gpu.empty(want, np.uint32)
    assert raw_pairs(gpu, bd, pd, op, ob, want) == (AQG_OK, want)
    assert gpu.join_count(bd, pd) == want


def test_join_returns(gpu, oracle):
    rng = np.random.default_rng(39)
    # a group-by and a join to be repeated at the end, on the same context
    gk, gv = rng.integers(0, 50, 100_000).astype(np.int32), rng.integers(-1000, 1000, 100_000).astype(np.int32)
    def group_sums():
        gb = gpu.groupby_agg([gk], [ck.RED_SUM], [gv])
        res = (gb.keys(0, np.int32).tolist(), gb.first_rows().tolist(), ck.i128_to_int(gb.result(0, ck.RED_SUM, ck.INT32)))
        gb.destroy()
        return res
    build = rng.integers(0, 40, 500).astype(np.int16)
    probe = rng.integers(-5, 45, 2000).astype(np.int16)
    before = (group_sums(), *gpu.join_pairs(build, probe), gpu.join_lookup(build, probe))
    opr, obr = oracle.join_pairs(build, probe)
    assert np.array_equal(before[1], opr) and np.array_equal(before[2], obr)
    bd, pd = gpu.to_device(build), gpu.to_device(probe)
    m = jm.count(build, probe)
    fill = np.full(m + 8, 0xA5A5A5A5, np.uint32)
    # a capacity one below the count: refused with the true count, nothing written
    op, ob = gpu.to_device(fill), gpu.to_device(fill)
    assert raw_pairs(gpu, bd, pd, op, ob, m - 1) == (AQG_ERR_OVERFLOW, m)
    assert np.array_equal(op.to_host(), fill) and np.array_equal(ob.to_host(), fill)
    # the exact capacity: written, and nothing beyond the count
    assert raw_pairs(gpu, bd, pd, op, ob, m) == (AQG_OK, m)
    want_p, want_b = jm.pairs(build, probe)
    assert np.array_equal(op.to_host()[:m], want_p) and np.array_equal(ob.to_host()[:m], want_b)
    assert np.all(op.to_host()[m:] == 0xA5A5A5A5) and np.all(ob.to_host()[m:] == 0xA5A5A5A5)
    # no matches, outputs given
    op, ob = gpu.to_device(fill), gpu.to_device(fill)
    miss = gpu.to_device((probe.astype(np.int16) + 1000).astype(np.int16))
    assert raw_pairs(gpu, bd, miss, op, ob, len(fill)) == (AQG_OK, 0)
    assert np.array_equal(op.to_host(), fill) and np.array_equal(ob.to_host(), fill)
    # empty sides
    e = gpu.to_device(np.zeros(0, np.int16))
    for b_, p_ in ((e, pd), (bd, e), (e, e)):
        assert raw_pairs(gpu, b_, p_, op, ob, len(fill)) == (AQG_OK, 0)
        assert raw_pairs(gpu, b_, p_, None, None, 0) == (AQG_OK, 0)
    assert np.array_equal(op.to_host(), fill)
    assert gpu.join_count(np.zeros(0, np.int16), probe) == 0 and gpu.join_count(build, np.zeros(0, np.int16)) == 0
    assert np.all(gpu.join_lookup(np.zeros(0, np.int16), probe) == NONE) and len(gpu.join_lookup(build, np.zeros(0, np.int16))) == 0
    # AQG_BOOL keys
    import aquery2_amd.capi as capi
    bb, pb = rng.random(300) < 0.3, rng.random(1000) < 0.5
    bbd, pbd = gpu.to_device(bb), gpu.to_device(pb)
    bbd._tag = pbd._tag = capi.BOOL
    assert bbd.tag == capi.BOOL
    pr, br = gpu.join_pairs(bbd, pbd)
    want_p, want_b = jm.pairs(bb, pb)
    assert np.array_equal(pr, want_p) and np.array_equal(br, want_b)
    assert gpu.join_count(bbd, pbd) == jm.count(bb, pb)
    assert np.array_equal(gpu.join_lookup(bbd, pbd), jm.lookup(bb, pb))
    only_true = gpu.to_device(np.ones(5, np.bool_))
    only_true._tag = capi.BOOL
    assert np.array_equal(gpu.join_lookup(only_true, pbd), np.where(pb, 0, NONE).astype(np.uint32))
    # floating keys: refused by all three
    for fdt in (np.float32, np.float64):
        fb, fp = np.arange(10, dtype=fdt), np.arange(20, dtype=fdt)
        for call in (gpu.join_lookup, gpu.join_count, gpu.join_pairs):
            with pytest.raises(capi.AqgError) as err:
                call(fb, fp)
            assert err.value.code == AQG_ERR_DTYPE
        fbd, fpd = gpu.to_device(fb), gpu.to_device(fp)
        assert raw_pairs(gpu, fbd, fpd, op, ob, len(fill))[0] == AQG_ERR_DTYPE
    assert np.array_equal(op.to_host(), fill)
    # the context is as it was: the same group-by and the same joins give the same answers
    after = (group_sums(), *gpu.join_pairs(build, probe), gpu.join_lookup(build, probe))
    assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1:], after[1:]))


# ---- aqg_join_groupby_sum -------------------------------------------------------------------------------------------------
def star(gpu, dim_key, dim_w, fk, gkey, val, hint=0, handle=None, offs=(0, 0, 0), dev=None):
    """one call of aqg_join_groupby_sum through the C-ABI, compared with the model: keys, first rows (fact row ids), exact sums.
    offs: fk / gkey / val are passed as views that start `off` elements into a larger column; dev: device columns already uploaded
    (dim_key, dim_w, fk, gkey, val order, None = upload)"""
    import aquery2_amd.capi as capi
    host = [np.ascontiguousarray(a) for a in (dim_key, dim_w, fk, gkey, val)]
    pad = [0, 0, *offs]
    bufs = []
    for i, (a, off) in enumerate(zip(host, pad)):
        if dev is not None and dev[i] is not None:
            bufs.append(dev[i])
        else:
            bufs.append(gpu.to_device(np.concatenate([np.full(off, 0x5A5A5A5A, dtype=np.uint32).astype(a.dtype), a]) if off else a))
    ptr = [C.c_void_p(b.ptr + 4 * off) for b, off in zip(bufs, pad)]
    h = handle.h if handle is not None else C.c_void_p()
    rc = gpu.lib.aqg_join_groupby_sum(gpu.ctx, bufs[0].tag, ptr[0], bufs[1].tag, ptr[1], C.c_uint32(len(host[0])), ptr[2], bufs[3].tag, ptr[3],
                                      bufs[4].tag, ptr[4], C.c_uint32(len(host[2])), C.c_uint32(hint), C.byref(h))
    if rc != AQG_OK:
        return rc, None
    gb = handle if handle is not None else capi.GroupBy(gpu, h)
    gb._keep = bufs
    keys, rows, sums = jm.star_sum(*host)
    assert gb.ngroups == len(keys), (gb.ngroups, len(keys))
    if len(keys):
        signed = host[1].dtype.kind == "i" or host[4].dtype.kind == "i"
        assert np.array_equal(gb.keys(0, host[3].dtype), keys)
        assert np.array_equal(gb.first_rows(), rows)
        assert ck.i128_to_int(gb.result(0, ck.RED_SUM, ck.INT64 if signed else ck.UINT64)) == sums
    if handle is None:
        gb.destroy()
    return rc, len(keys)


def star_inputs(rng, n, nb, gkeys, kdt=np.int32, vdt=np.int32, wdt=np.int32, partner=0.8):
    """a dimension side of nb distinct keys from the whole range, fact rows of which `partner` have one, group keys from gkeys"""
    dim_key = distinct_keys(rng, kdt, nb)
    fk = full_range(rng, kdt, n)
    if nb:
        hit = rng.random(n) < partner
        fk[hit] = dim_key[rng.integers(0, nb, int(hit.sum()))]
    gk = np.asarray(gkeys)[rng.integers(0, len(gkeys), n)] if n else np.asarray(gkeys)[:0]
    return dim_key, full_range(rng, wdt, nb), fk, gk, full_range(rng, vdt, n)


def plant(rng, cols, keys):
    """every group key on at least one row that has a partner"""
    dim_key, _, fk, gk, _ = cols
    rows = rng.permutation(len(fk))[:len(keys)]
    gk[rows] = keys
    fk[rows] = dim_key[rng.integers(0, len(dim_key), len(keys))]
    return cols


EMPTY32 = {np.int32: -2**31, np.uint32: 2**31}


@pytest.mark.parametrize("gdt", [np.int32, np.uint32], ids=nm)
def test_star_group_key_equal_to_the_empty_mark(gpu, gdt):
    """0x80000000 as a GROUP key (slot `lcap` of the LDS table): the only group, one of 51, the group of row 0, and in the last
    three rows only -- rows past the last block of 8, which go to the global table directly"""
    rng = np.random.default_rng(40)
    e = EMPTY32[gdt]
    others = np.array([k for k in distinct_keys(rng, gdt, 51).tolist() if k != e][:50], dtype=gdt)
    n = 40_003                                                            # n % 8 == 3
    # the only group
    dk, dw, fk, gk, val = star_inputs(rng, n, 64, np.array([e], dtype=gdt))
    assert star(gpu, dk, dw, fk, gk, val) == (AQG_OK, 1)
    # among 50 others
    dk, dw, fk, gk, val = star_inputs(rng, n, 64, np.concatenate([others, np.array([e], dtype=gdt)]))
    assert star(gpu, dk, dw, fk, gk, val) == (AQG_OK, 51)
    # the group of row 0, which has a partner
    gk[0], fk[0] = e, dk[3]
    assert star(gpu, dk, dw, fk, gk, val) == (AQG_OK, 51)
    # in the three tail rows only, all joined
    gk = others[rng.integers(0, 50, n)]
    gk[-3:], fk[-3:] = e, dk[:3]
    assert star(gpu, dk, dw, fk, gk, val) == (AQG_OK, 51)
    # ... and as the only group that exists at all: nothing but the tail rows has a partner
    fk[:-3] = np.array([k for k in range(100) if k not in dk.tolist()][:1], dtype=np.int32)[0]
    assert star(gpu, dk, dw, fk, gk, val) == (AQG_OK, 1)


_GROUP_CASES = {}


def group_case(G):
    """n = 200,003 rows in G groups whose keys come from the whole 32-bit range (the empty mark and both ends among them)"""
    if G not in _GROUP_CASES:
        rng = np.random.default_rng(41 + G)
        keys = distinct_keys(rng, np.uint32, G, exclude=(0, 2**31, 2**32 - 1, 2**31 - 1))
        special = np.array([2**31, 0, 2**32 - 1, 2**31 - 1], dtype=np.uint32)[:min(4, G)]
        keys[:len(special)] = special
        _GROUP_CASES[G] = plant(rng, star_inputs(rng, 200_003, 100, keys, partner=0.9), keys)
    return _GROUP_CASES[G]


@pytest.mark.parametrize("G", [1, 64, 3071, 3072])
def test_star_group_counts_whatever_the_hint(gpu, G):
    """up to 3072 groups with no hint, a hint far too small, the exact one and the largest: the same answer"""
    cols = group_case(G)
    assert len(jm.star_sum(*cols)[0]) == G
    for hint in sorted({0, 1, G, 3072}):
        assert star(gpu, *cols, hint=hint) == (AQG_OK, G), hint


def test_star_more_groups_than_the_limit(gpu):
    cols = group_case(3073)
    assert len(jm.star_sum(*cols)[0]) == 3073
    for hint in (0, 3073):
        assert star(gpu, *cols, hint=hint) == (AQG_ERR_ARG, None)
    assert star(gpu, *group_case(64)) == (AQG_OK, 64)                     # the context still answers


def test_star_groups_count_among_the_joined_rows_only(gpu):
    """10,000 distinct group keys in the column, 100 of them on rows with a partner: the library answers (its limit counts the groups
    of the JOINED rows -- rows without a partner never reach the group table)"""
    rng = np.random.default_rng(42)
    n = 200_003
    keys = distinct_keys(rng, np.int32, 10_000)
    dk, dw, fk, gk, val = star_inputs(rng, n, 50, keys[:100])
    rows = rng.permutation(n)
    joined, lonely = rows[:80_000], rows[80_000:]
    fk[joined] = dk[rng.integers(0, 50, len(joined))]
    gk[joined] = keys[:100][rng.integers(0, 100, len(joined))]
    gk[joined[:100]] = keys[:100]
    fk[lonely] = np.array([k for k in range(60) if k not in dk.tolist()][:1], dtype=np.int32)[0]    # a key of no dimension row
    gk[lonely] = keys[100:][rng.integers(0, 9900, len(lonely))]
    gk[lonely[:9900]] = keys[100:]
    assert len(np.unique(gk)) == 10_000 and len(jm.star_sum(dk, dw, fk, gk, val)[0]) == 100
    for hint in (0, 100):
        assert star(gpu, dk, dw, fk, gk, val, hint=hint) == (AQG_OK, 100)


@pytest.mark.parametrize("vdt,wdt", [(np.uint32, np.int32), (np.int32, np.uint32)], ids=["u32_val_i32_w", "i32_val_u32_w"])
def test_star_mixed_signedness(gpu, vdt, wdt):
    """an unsigned column times a signed one: the products are signed 64-bit values, the result a signed 128-bit sum"""
    rng = np.random.default_rng(43)
    n, nb = 300_000, 64
    ext = lambda d: np.array([0, 1, np.iinfo(d).max, np.iinfo(d).min, np.iinfo(d).max - 1], dtype=d)
    dk, dw, fk, gk, val = star_inputs(rng, n, nb, (np.arange(9, dtype=np.int64) * 500_000_000).astype(np.uint32), vdt=vdt, wdt=wdt)
    at = rng.random(n) < 0.5
    val[at] = ext(vdt)[rng.integers(0, 5, int(at.sum()))]
    dw[:40] = ext(wdt)[rng.integers(0, 5, 40)]
    dw[:5] = ext(wdt)
    assert star(gpu, dk, dw, fk, gk, val) == (AQG_OK, 9)
    # every product at its largest magnitude, one sign: nothing cancels
    val[:] = np.iinfo(vdt).max if vdt == np.uint32 else np.iinfo(vdt).min
    dw[:] = np.iinfo(wdt).min if wdt == np.int32 else np.iinfo(wdt).max
    assert star(gpu, dk, dw, fk, gk, val) == (AQG_OK, 9)


ACC_SWEEPS = {
    "min_times_negative": (np.int32, -2**31, np.int32, [-(1 << k) for k in range(32)]),
    "min_times_positive": (np.int32, -2**31, np.int32, [1 << k for k in range(31)]),
    "max_times_negative": (np.int32, 2**31 - 1, np.int32, [-(1 << k) for k in range(32)]),
    "unsigned_max": (np.uint32, 2**32 - 1, np.uint32, [1 << k for k in range(32)] + [2**32 - 1]),
}


@pytest.mark.parametrize("name", list(ACC_SWEEPS))
def test_star_accumulators_at_their_limits(gpu, name):
    """one group, every value at one extreme, every weight +-2^k for every k: the sweep crosses the switch between one 64-bit
    accumulator per workgroup and the two halves wherever the grid puts it; n * val * w as a Python int"""
    vdt, v, wdt, ws = ACC_SWEEPS[name]
    n = (1 << 20) + 5
    dim_key = np.array([5, 6, 7], dtype=np.int32)
    fk, gk, val = np.full(n, 5, np.int32), np.full(n, -77, np.int32), np.full(n, v, dtype=vdt)
    dev = [gpu.to_device(dim_key), None, gpu.to_device(fk), gpu.to_device(gk), gpu.to_device(val)]
    import aquery2_amd.capi as capi
    for w in ws:
        dw = gpu.to_device(np.full(3, w, dtype=wdt))
        h = C.c_void_p()
        gpu._chk(gpu.lib.aqg_join_groupby_sum(gpu.ctx, dev[0].tag, C.c_void_p(dev[0].ptr), dw.tag, C.c_void_p(dw.ptr), C.c_uint32(3), C.c_void_p(dev[2].ptr),
                                              dev[3].tag, C.c_void_p(dev[3].ptr), dev[4].tag, C.c_void_p(dev[4].ptr), C.c_uint32(n), C.c_uint32(0), C.byref(h)),
                 "aqg_join_groupby_sum")
        gb = capi.GroupBy(gpu, h)
        assert gb.ngroups == 1 and gb.keys(0, np.int32).tolist() == [-77] and gb.first_rows().tolist() == [0]
        got = ck.i128_to_int(gb.result(0, ck.RED_SUM, ck.INT64 if vdt == np.int32 else ck.UINT64))
        assert got == [n * v * w], (name, w, got, n * v * w)
        gb.destroy()


@pytest.mark.parametrize("nb", [0, 1, 7, 8, 9, 4095, 4096])
def test_star_dimension_sizes(gpu, nb):
    rng = np.random.default_rng(44 + nb)
    cols = star_inputs(rng, 20_011, nb, np.arange(-20, 20, dtype=np.int32), partner=0.7)
    rc, G = star(gpu, *cols)
    assert rc == AQG_OK and G == (40 if nb else 0)


def test_star_dimension_side_too_large(gpu):
    rng = np.random.default_rng(45)
    assert star(gpu, *star_inputs(rng, 1000, 4097, np.arange(5, dtype=np.int32))) == (AQG_ERR_ARG, None)
    assert star(gpu, *star_inputs(rng, 1000, 4096, np.arange(5, dtype=np.int32)))[0] == AQG_OK


def test_star_duplicate_and_empty_mark_dimension_keys(gpu):
    rng = np.random.default_rng(46)
    dk, dw, fk, gk, val = star_inputs(rng, 50_001, 3000, np.arange(30, dtype=np.int32), partner=0.5)
    dup_rows = rng.permutation(3000)[:40]
    dk[dup_rows] = dk[dup_rows[0]]                                        # 40 copies of one key at scattered rows
    e_rows = [2999, 1500, 17]
    dk[e_rows] = -2**31                                                   # the LDS empty mark as a dimension key, three times
    dw[:] = np.arange(3000, dtype=np.int32) + 1                           # w names its row: the lowest row must win
    fk[rng.permutation(50_001)[:20_000]] = rng.choice(np.array([dk[dup_rows[0]], -2**31], dtype=np.int32), 20_000)
    assert star(gpu, dk, dw, fk, gk, val) == (AQG_OK, 30)
    # the mark probed while no dimension row holds it
    dk[e_rows] = [11, 12, 13]
    assert len(np.unique(dk)) == 3000 - 39
    assert star(gpu, dk, dw, fk, gk, val) == (AQG_OK, 30)


@pytest.mark.parametrize("nb", [5, 100, 3000])
def test_star_dimension_chain_wraps_past_the_last_slot(gpu, nb):
    """WHITE BOX on fib_slot (groupby_dev.hpp) and the dimension table of starjoin_kernel (dcap = the power of two >= 2 * max(nb, 8)):
    every dimension key has the last slot as its home; fact keys that miss share that home or have theirs inside the chain"""
    rng = np.random.default_rng(47)
    dcap = 1
    while dcap < 2 * max(nb, 8):
        dcap <<= 1
    bits, last = dcap.bit_length() - 1, dcap - 1
    same_home = keys_with_home(last, bits, np.arange(nb + 60))
    inside = np.concatenate([keys_with_home(s, bits, np.arange(3)) for s in (0, 1, nb // 2, nb - 2)])
    dk, miss = rng.permutation(same_home[:nb]), np.concatenate([same_home[nb:], inside])
    assert np.all(fib_slot(same_home, bits) == last) and set(fib_slot(inside, bits).tolist()) <= set(range(nb - 1))
    assert 2**31 not in dk.tolist() + miss.tolist() and not np.isin(miss, dk).any()
    n = 30_005
    fk = np.concatenate([dk, miss, rng.choice(np.concatenate([dk, miss]), n - nb - len(miss))]).astype(np.uint32)
    gk = rng.integers(0, 12, n).astype(np.int32)
    rc, G = star(gpu, dk, full_range(rng, np.int32, nb), fk, gk, full_range(rng, np.int32, n))
    assert rc == AQG_OK and G == 12


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049, 65_537])
def test_star_fact_sizes_and_column_views(gpu, n):
    """fact sizes around the 8-row step, and fk / gkey / val as views 1, 2 and 3 elements into their columns: 4-byte but not 16-byte
    aligned, which the row loop must take through its 4-byte loads"""
    rng = np.random.default_rng(48 + n)
    cols = star_inputs(rng, n, 37, np.array([-2**31, -1, 0, 1, 2**31 - 1, 12345], dtype=np.int32), partner=0.8)
    if n:
        cols[2][0] = cols[0][0]                                           # row 0 joins
    want = len(jm.star_sum(*cols)[0])
    views = [(0, 0, 0), (1, 2, 3), (2, 2, 2)] + [tuple(o if c == col else 0 for c in range(3)) for col in range(3) for o in (1, 2, 3)]
    for offs in views:                                                    # each column alone at 1, 2 and 3 elements, and all three together
        assert star(gpu, *cols, offs=offs) == (AQG_OK, want), (n, offs)


def test_star_handle_reuse(gpu):
    import aquery2_amd.capi as capi
    rng = np.random.default_rng(49)
    gb = None
    for G in (5, 3000, 2):
        keys = distinct_keys(rng, np.int32, G)
        cols = plant(rng, star_inputs(rng, 100_003, 200, keys, partner=0.9), keys)
        if gb is None:
            gb = capi.GroupBy(gpu, C.c_void_p())
        assert star(gpu, *cols, handle=gb) == (AQG_OK, G)
    gb.destroy()
