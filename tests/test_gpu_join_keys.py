"""The joins on composite and typed keys (aqg_join_keys_count / _pairs / _lookup, aqg_join_last, aqg_gather_fill) against their model
(tests/join_keys_model.py) and, for the equality rule, against the group ids the REAL reference produced
(tests/golden/ref_golden_keys.json).  Everything goes through the C-ABI; every result is an integer, a row id or a status and is
compared for equality."""
import ctypes as C

import numpy as np
import pytest

import checker as ck
import join_keys_model as jkm
import join_model as jm
import keycases
from test_join_keys_model import GOLD, golden_self_join

pytestmark = pytest.mark.gpu
NONE = jkm.NONE
KINDS = (jkm.INNER, jkm.LEFT, jkm.SEMI, jkm.ANTI)
AQG_OK, AQG_ERR_DTYPE, AQG_ERR_ARG, AQG_ERR_OVERFLOW = 0, 2, 3, 6
PACKED, WIDE, LDS, HBM = 1, 2, 4, 8
CANARY = 0xA5A5A5A5


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def dev_cols(gpu, cols):
    return [gpu.key_col(tag, data) if tag in (ck.DATE, ck.TIME, ck.TIMESTAMP, ck.STR) else gpu.to_device(data) for tag, data in cols]


# ---- seeded sides: tuple number j -> a tuple, injectively, so that "present" and "absent" are decided by numbers ---------------------
INT = {"i8": (ck.INT8, np.int8), "i16": (ck.INT16, np.int16), "i32": (ck.INT32, np.int32), "i64": (ck.INT64, np.int64),
       "u8": (ck.UINT8, np.uint8), "u16": (ck.UINT16, np.uint16), "u32": (ck.UINT32, np.uint32), "u64": (ck.UINT64, np.uint64)}
DOMAIN = {"bool": 2, "i8": 256, "u8": 256, "i16": 1 << 16, "u16": 1 << 16}
STRIDE = 0x9E3779B97F4A7C15                 # odd: d -> d * STRIDE + offset is one-to-one modulo every power of two


def column(rng, kind, digit, c):
    """the values of one key column for the digits `digit` (distinct digits, distinct values)"""
    n = len(digit)
    d = digit.astype(np.uint64)
    if kind == "bool":
        return ck.BOOL, digit.astype(np.bool_)
    if kind in INT:
        tag, dt = INT[kind]
        return tag, (d * np.uint64(STRIDE) + np.uint64(0x1234567 * (c + 1))).astype(dt)          # wraps: one-to-one below the type's width
    if kind == "f64":
        return ck.DOUBLE, digit.astype(np.float64) * 0.5 - 3.0
    if kind == "f32":
        return ck.FLOAT, digit.astype(np.float32) * np.float32(0.5) - np.float32(3.0)
    if kind == "i128":
        a = np.zeros(n, ck.I128)
        a["lo"] = d * np.uint64(0x8000000000000001)
        a["hi"] = digit % 3 - 1
        return ck.INT128, a
    w = {"date": 4, "time": 8, "ts": 12}[kind]
    a = np.zeros((n, w), np.uint8)
    a[:, 0:4] = digit.astype("<u4").view(np.uint8).reshape(n, 4)
    if kind == "ts":
        a[:, 4:8] = (digit * 7 + 1).astype("<u4").view(np.uint8).reshape(n, 4)
    if kind in ("time", "ts"):
        a[:, w - 1] = rng.integers(0, 256, n)            # junk in the padding byte, different on every row and side
    return {"date": ck.DATE, "time": ck.TIME, "ts": ck.TIMESTAMP}[kind], a


def tuples(rng, spec, j, total):
    """the key columns of the tuples numbered j (an int64 array of numbers below `total`): mixed-radix digits, the column of the
    largest domain taking what the small radices of the others leave"""
    dom = [DOMAIN.get(k, 1 << 62) for k in spec]
    big = int(np.argmax(dom))
    radix = [min(d, 13) for d in dom]
    rest = int(np.prod([r for c, r in enumerate(radix) if c != big]))
    radix[big] = -(-total // rest)
    assert radix[big] <= dom[big]
    q = j.copy()
    digits = [None] * len(spec)
    for c in [c for c in range(len(spec)) if c != big] + [big]:
        digits[c], q = q % radix[c], q // radix[c]
    assert not q.any()
    return [column(rng, k, digits[c], c) for c, k in enumerate(spec)]


def sides(rng, spec, nb, npr, miss=1 / 3):
    """build: every tuple present 1-4 times, shuffled; probe: about `miss` of the rows without a partner"""
    D = max(1, nb // 2)
    j = rng.permutation(np.repeat(np.arange(D, dtype=np.int64), rng.integers(1, 5, D)))[:nb]
    if nb == 0:
        j, D = np.zeros(0, np.int64), 0
    p = D + rng.integers(0, max(D, 50), npr)
    hit = rng.random(npr) >= miss
    if nb:
        p[hit] = j[rng.integers(0, nb, int(hit.sum()))]
    total = 2 * max(D, 50) + 1
    return tuples(rng, spec, j, total), tuples(rng, spec, p, total)


def check_all(gpu, build, probe, form=None, route=None):
    """all four kinds, the counts and the look-up of one pair of sides against the model; returns the routes of the probe"""
    m = jkm.matches(build, probe)
    bd, pd = dev_cols(gpu, build), dev_cols(gpu, probe)
    routes = set()
    for kind in KINDS:
        want_p, want_b = jkm.pairs(kind, build, probe, m)
        assert gpu.join_keys_count(bd, pd, kind) == jkm.count(kind, build, probe, m) == len(want_p), kind
        pr, br = gpu.join_keys_pairs(bd, pd, kind)
        routes.add(gpu.join_last())
        assert np.array_equal(pr, want_p), kind
        assert br is None if want_b is None else np.array_equal(br, want_b), kind
    assert np.array_equal(gpu.join_keys_lookup(bd, pd), jkm.lookup(build, probe, m))
    routes.add(gpu.join_last())
    nb, npr = len(build[0][1]), len(probe[0][1])
    if nb and npr:
        assert len(routes) == 1
        r, G, slots = routes.pop()
        assert (G, slots) == jkm.distinct(build)
        assert form is None or r & 3 == form
        assert route is None or r & 12 == route
        return r
    assert routes == {(0, 0, 0)}                 # an empty side: no probe ran
    return 0


# ---- the equality rule, against the reference's ids --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLD))
def test_self_join_against_reference_ids(gpu, name):
    cols = dict(keycases.cases())[name]
    want, cnt = golden_self_join(name, cols)
    dk = dev_cols(gpu, cols)                     # strings: the codes of one dictionary serve both sides
    assert np.array_equal(gpu.join_keys_lookup(dk, dk), want)
    assert gpu.join_keys_count(dk, dk, jkm.INNER) == cnt


# ---- kinds x forms x routes --------------------------------------------------------------------------------------------------------
SPECS = {"i32_i32": (("i32", "i32"), PACKED), "i8_i16_i32": (("i8", "i16", "i32"), PACKED), "bool_u16": (("bool", "u16"), PACKED),
         "i64_i32": (("i64", "i32"), WIDE), "f64_i32": (("f64", "i32"), WIDE), "date_i32": (("date", "i32"), PACKED), "ts_i32": (("ts", "i32"), WIDE),
         "i128_i32": (("i128", "i32"), WIDE), "i64x8": (("i64",) * 8, WIDE)}


def expected_route(spec, nb, npr, build):
    """today's rule: the table (8 bytes a slot) and the group keys (8 bytes a word) within 48 KB under at least 2^16 probe rows"""
    G, slots = jkm.distinct(build)
    words = 1 if SPECS[spec][1] == PACKED else sum(2 if k in ("ts", "i128") else 1 for k in SPECS[spec][0])
    return LDS if slots * 8 + words * G * 8 <= 48 * 1024 and npr >= 1 << 16 else HBM


@pytest.mark.parametrize("npr", [70_001, 5000])
@pytest.mark.parametrize("nb", [1000, 40_000])
@pytest.mark.parametrize("spec", sorted(SPECS))
def test_kinds_forms_routes(gpu, spec, nb, npr):
    rng = np.random.default_rng(71)
    build, probe = sides(rng, SPECS[spec][0], nb, npr)
    check_all(gpu, build, probe, form=SPECS[spec][1], route=expected_route(spec, nb, npr, build))


def test_every_form_and_route_runs(gpu):
    rng = np.random.default_rng(72)
    seen = set()
    for spec in ("i32_i32", "i64_i32"):
        for npr in (70_001, 5000):
            build, probe = sides(rng, SPECS[spec][0], 1000, npr)
            seen.add(check_all(gpu, build, probe))
    assert seen == {PACKED | LDS, PACKED | HBM, WIDE | LDS, WIDE | HBM}


# ---- no key value is a sentinel ----------------------------------------------------------------------------------------------------
ALL_ONES = {"i32_i32": ("i32", "i32"), "u8_u16_u32": ("u8", "u16", "u32"), "u64": ("u64",), "i64": ("i64",), "i64_i64": ("i64", "i64"), "u64_i32": ("u64", "i32")}


def put_all_ones(cols, rows):
    for _, a in cols:
        a[list(rows)] = -1 if a.dtype.kind == "i" else np.iinfo(a.dtype).max


@pytest.mark.parametrize("npr", [70_001, 5000], ids=["lds", "hbm"])
@pytest.mark.parametrize("spec", sorted(ALL_ONES))
def test_all_ones_tuples_are_ordinary_keys(gpu, spec, npr):
    rng = np.random.default_rng(73)
    nb = 2000
    base, probe = sides(rng, ALL_ONES[spec], nb, npr)
    at = np.concatenate([[0, 1, 7, 8, npr - 1, npr - 2], rng.integers(0, npr, 40)])          # vector body and scalar tail rows
    put_all_ones(probe, at)
    pd = dev_cols(gpu, probe)
    for rows, want in (((1234,), 1234), ((nb - 1, 700, 3), 3), ((), NONE)):
        build = [(t, a.copy()) for t, a in base]
        put_all_ones(build, rows)
        m = jkm.matches(build, probe)
        model = jkm.lookup(build, probe, m)
        assert np.all(model[at] == want)
        bd = dev_cols(gpu, build)
        got = gpu.join_keys_lookup(bd, pd)
        assert np.all(got[at] == want) and np.array_equal(got, model), (spec, rows)
        for kind in (jkm.INNER, jkm.ANTI):
            pr, br = gpu.join_keys_pairs(bd, pd, kind)
            wp, wb = jkm.pairs(kind, build, probe, m)
            assert np.array_equal(pr, wp) and (wb is None or np.array_equal(br, wb)), (spec, rows, kind)


# ---- collision chains that wrap at the last slot -----------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,form", [(("i32", "i32"), PACKED), (("i64", "i32"), WIDE)], ids=["packed", "wide"])
def test_chains_wrap_at_the_last_slot(gpu, spec, form):
    rng = np.random.default_rng(74)
    N, G, SLOTS = 200_000, 1000, 2048
    pool = tuples(rng, spec, np.arange(N, dtype=np.int64), N)
    slot = gpu.join_tuple_slots([a for _, a in pool], SLOTS)
    tail = np.nonzero(slot >= SLOTS - 3)[0]
    assert len(tail) >= 80
    inb, absent = tail[:40], tail[40:80]                          # 40 tuples start in the last three slots: the chain runs on at slot 0
    rest = np.setdiff1d(np.arange(N), tail)
    bj = rng.permutation(np.concatenate([inb, rng.choice(rest, G - len(inb), replace=False)]))
    take = lambda j: [(t, a[j]) for t, a in pool]
    build = take(bj)
    for npr, route in ((5000, HBM), (70_001, LDS)):
        pj = np.concatenate([inb, absent, rng.choice(bj, npr - 80 - npr // 4), rng.choice(rest, npr // 4)])
        probe = take(rng.permutation(pj))
        check_all(gpu, build, probe, form=form, route=route)
        assert gpu.join_last()[1:] == (G, SLOTS)


# ---- tuples that differ in one column ----------------------------------------------------------------------------------------------
def test_near_misses(gpu):
    rng = np.random.default_rng(75)
    n = 5003
    a, b, c = rng.integers(-2**62, 2**62, n), rng.integers(-2**30, 2**30, n).astype(np.int32), rng.integers(-2**62, 2**62, n)
    wide = [(ck.INT64, a), (ck.INT32, b), (ck.INT64, c)]
    packed = [(ck.INT32, b), (ck.INT32, (b * 3).astype(np.int32))]
    single = [(ck.INT64, a)]
    def changed(cols, k, f):
        return [(t, f(x) if i == k else x) for i, (t, x) in enumerate(cols)]
    cases = [(wide, changed(wide, 0, lambda x: x + 1)), (wide, changed(wide, 2, lambda x: x + 1)), (wide, changed(wide, 1, lambda x: x ^ np.int32(1 << 20))),
             (wide, changed(wide, 0, lambda x: x ^ (1 << 40))), (wide, changed(wide, 2, lambda x: x ^ (1 << 63 - 1))),       # only the high 32 bits
             (packed, changed(packed, 0, lambda x: x + np.int32(1))), (packed, changed(packed, 1, lambda x: x ^ np.int32(1 << 31 - 1))),
             (single, changed(single, 0, lambda x: x ^ (1 << 32))), (single, changed(single, 0, lambda x: x ^ (1 << 62)))]
    for build, probe in cases:
        bd, pd = dev_cols(gpu, build), dev_cols(gpu, probe)
        assert jkm.count(jkm.INNER, build, probe) == 0
        assert np.all(gpu.join_keys_lookup(bd, pd) == NONE)
        assert gpu.join_keys_count(bd, pd, jkm.INNER) == 0 and gpu.join_keys_count(bd, pd, jkm.ANTI) == n
        assert gpu.join_keys_count(bd, bd, jkm.SEMI) == n         # and the sides match themselves


# ---- floating keys -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", [None, "i64"], ids=["packed", "wide"])
@pytest.mark.parametrize("dt,tag", [(np.float64, ck.DOUBLE), (np.float32, ck.FLOAT)], ids=["f64", "f32"])
def test_floating_keys(gpu, dt, tag, second):
    rng = np.random.default_rng(76)
    n = 203
    plain = lambda: (rng.integers(1, 30, n) * 0.25).astype(dt)
    special = plain()
    special[[0, 5, 9, n - 1]] = np.nan                            # NaN at the SAME rows on both sides
    special[[1, 6, n - 2]] = -np.nan
    special[[2, 7]] = -0.0
    special[[3, 8]] = 0.0
    other = special.copy()
    other[[2, 7]] = 0.0
    other[[3, 8]] = -0.0
    zeros = plain(); zeros[[4, 40]] = 0.0                         # a side with neither a NaN nor a negative zero
    k = rng.integers(0, 2, n).astype(np.int64)
    def cols(f):
        return [(tag, f)] + ([(ck.INT64, k)] if second else [])
    for build, probe in ((special, special), (special, other), (special, zeros), (zeros, special), (plain(), special), (special, plain())):
        m = jkm.matches(cols(build), cols(probe))
        assert all(not b for b, v in zip(m, probe) if np.isnan(v))
        check_all(gpu, cols(build), cols(probe), form=WIDE if second else PACKED)
    got = gpu.join_keys_lookup(dev_cols(gpu, cols(special)), dev_cols(gpu, cols(other)))
    assert np.all(got[[0, 5, 9, n - 1, 1, 6, n - 2]] == NONE) and np.all(got[[2, 7, 3, 8]] != NONE)


def test_time_padding_byte_is_ignored(gpu):
    rng = np.random.default_rng(77)
    for spec in (("time",), ("time", "i32"), ("ts",)):
        build, probe = sides(rng, spec, 600, 4001)
        build[0][1][:, -1], probe[0][1][:, -1] = 0x11, 0xEE       # the padding bytes differ between the sides on every row
        assert check_all(gpu, build, probe) & (PACKED if spec == ("time",) else WIDE)
        assert jkm.count(jkm.SEMI, build, probe) > 2000


# ---- edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [("i32", "i16"), ("i64", "f64")], ids=["packed", "wide"])
def test_edges(gpu, spec):
    rng = np.random.default_rng(78)
    for nb, npr in ((0, 0), (0, 9), (0, 70_001), (9, 0), (1, 1), (40, 1), (1, 40), (5, 70_001)):
        build, probe = sides(rng, spec, nb, npr, miss=0.5)
        check_all(gpu, build, probe)
    build, probe = sides(rng, spec, 3000, 999)
    build = [(t, np.repeat(a[:1], 3000, axis=0)) for t, a in build]           # G == 1: a build side of all-equal tuples
    probe[0][1][::3], probe[1][1][::3] = build[0][1][0], build[1][1][0]
    check_all(gpu, build, probe)
    assert gpu.join_last()[1:] == (1, 16)
    # a SEMI call with build_rows_out == NULL, written into a canary-filled output
    bd, pd = dev_cols(gpu, build), dev_cols(gpu, probe)
    _, dts, bp = gpu._keyargs(bd)
    _, _, pp = gpu._keyargs(pd)
    want, _ = jkm.pairs(jkm.SEMI, build, probe)
    out = gpu.to_device(np.full(len(want) + 8, CANARY, np.uint32))
    m = C.c_uint64()
    assert gpu.lib.aqg_join_keys_pairs(gpu.ctx, jkm.SEMI, 2, dts, bp, 3000, pp, 999, out.ptr, None, len(want), C.byref(m)) == AQG_OK
    got = out.to_host()
    assert m.value == len(want) >= 333 and np.array_equal(got[:len(want)], want) and np.all(got[len(want):] == CANARY)
    assert gpu.lib.aqg_join_keys_pairs(gpu.ctx, jkm.LEFT, 2, dts, bp, 3000, pp, 999, out.ptr, None, 1 << 40, C.byref(m)) == AQG_ERR_ARG


# ---- views off the vector width ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npr", [17, 65_541])
@pytest.mark.parametrize("spec", [("i16", "i32"), ("i32", "i64"), ("ts", "u8")], ids=["packed", "wide", "timestamp"])
def test_offset_views(gpu, spec, npr):
    """key columns and outputs advanced by one element: off the vector width, so the rows take the scalar loop"""
    rng = np.random.default_rng(79)
    nb = 300
    build, probe = sides(rng, spec, nb + 1, npr + 1)
    bd, pd = dev_cols(gpu, build), dev_cols(gpu, probe)
    esz = [np.asarray(a).reshape(len(a), -1).view(np.uint8).reshape(len(a), -1).shape[1] for _, a in build]
    dts = (C.c_int * 2)(*[b.tag for b in bd])
    cut = lambda cols, o, n: [(t, a[o:o + n]) for t, a in cols]
    for boff, poff, ooff in ((1, 1, 1), (0, 1, 0), (0, 0, 1)):
        bp = (C.c_void_p * 2)(*[b.ptr + boff * e for b, e in zip(bd, esz)])
        pp = (C.c_void_p * 2)(*[p.ptr + poff * e for p, e in zip(pd, esz)])
        b, p = cut(build, boff, nb), cut(probe, poff, npr)
        m = jkm.matches(b, p)
        od = gpu.to_device(np.full(npr + 2, CANARY, np.uint32))
        assert gpu.lib.aqg_join_keys_lookup(gpu.ctx, 2, dts, bp, nb, pp, npr, od.ptr + 4 * ooff) == AQG_OK
        got = od.to_host()
        assert np.array_equal(got[ooff:ooff + npr], jkm.lookup(b, p, m)), (boff, poff, ooff)
        assert np.all(got[:ooff] == CANARY) and np.all(got[ooff + npr:] == CANARY)                  # nothing written around the view
        wp, wb = jkm.pairs(jkm.LEFT, b, p, m)
        o1, o2 = gpu.to_device(np.full(len(wp) + 2, CANARY, np.uint32)), gpu.to_device(np.full(len(wp) + 2, CANARY, np.uint32))
        cnt = C.c_uint64()
        assert gpu.lib.aqg_join_keys_pairs(gpu.ctx, jkm.LEFT, 2, dts, bp, nb, pp, npr, o1.ptr + 4 * ooff, o2.ptr + 4 * ooff, len(wp), C.byref(cnt)) == AQG_OK
        g1, g2 = o1.to_host(), o2.to_host()
        assert cnt.value == len(wp) and np.array_equal(g1[ooff:ooff + len(wp)], wp) and np.array_equal(g2[ooff:ooff + len(wp)], wb)
        assert np.all(g1[:ooff] == CANARY) and np.all(g1[ooff + len(wp):] == CANARY) and np.all(g2[:ooff] == CANARY) and np.all(g2[ooff + len(wp):] == CANARY)


# ---- one integer key: the existing joins' answers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_one_integer_key_equals_the_integer_joins(gpu, dt):
    rng = np.random.default_rng(80)
    info = np.iinfo(dt)
    keys = np.unique(np.concatenate([rng.integers(info.min, info.max, 150, dtype=dt, endpoint=True), np.array([info.min, info.max, 0], dtype=dt)]))
    for nb, npr in ((900, 20_000), (900, 70_001)):
        build = rng.choice(keys, nb)
        probe = rng.integers(info.min, info.max, npr, dtype=dt, endpoint=True)
        hit = rng.random(npr) < 0.67
        probe[hit] = rng.choice(build, int(hit.sum()))
        pr, br = gpu.join_keys_pairs([build], [probe], jkm.INNER)
        opr, obr = gpu.join_pairs(build, probe)
        assert np.array_equal(pr, opr) and np.array_equal(br, obr)
        assert np.array_equal(pr, jm.pairs(build, probe)[0]) and np.array_equal(br, jm.pairs(build, probe)[1])
        assert np.array_equal(gpu.join_keys_lookup([build], [probe]), gpu.join_lookup(build, probe))


@pytest.mark.parametrize("nb,npr,route,slots", [(2048, 65_536, LDS, 4096), (2049, 65_536, HBM, 8192), (2048, 65_535, HBM, 4096)],
                         ids=["48KB_table_2^16_rows", "one_build_row_more", "one_probe_row_fewer"])
def test_one_int32_key_lookup_reports_the_route_it_ran(gpu, nb, npr, route, slots):
    """aqg_join_keys_lookup on one plain integer key runs join.hip's probe, and aqg_join_last says what THAT launcher decided: the edges
    of the LDS rule (a table of 12-byte slots within 48 KB under at least 2^16 probe rows).  No other test reads the route of this path."""
    rng = np.random.default_rng(82)
    build = rng.permutation((np.arange(nb, dtype=np.int64) * 1_000_003 - 2**31).astype(np.int32))
    probe = rng.integers(-2**31, 2**31, npr).astype(np.int32)
    hit = rng.random(npr) < 0.67
    probe[hit] = build[rng.integers(0, nb, int(hit.sum()))]
    got = gpu.join_keys_lookup([build], [probe])
    assert gpu.join_last() == (PACKED | route, 0, slots)
    assert np.array_equal(got, jm.lookup(build, probe))


# ---- limits and errors -------------------------------------------------------------------------------------------------------------
def test_counts_beyond_32_bits_and_overflow(gpu):
    n = 70_000
    cols = [gpu.to_device(np.full(n, 7, np.int32)), gpu.to_device(np.full(n, -1, np.int64))]
    assert gpu.join_keys_count(cols, cols, jkm.LEFT) == gpu.join_keys_count(cols, cols, jkm.INNER) == 4_900_000_000
    assert gpu.join_keys_count(cols, cols, jkm.SEMI) == n and gpu.join_keys_count(cols, cols, jkm.ANTI) == 0
    _, dts, ptrs = gpu._keyargs(cols)
    o1, o2 = gpu.to_device(np.full(4096, CANARY, np.uint32)), gpu.to_device(np.full(4096, CANARY, np.uint32))
    m = C.c_uint64()
    rc = gpu.lib.aqg_join_keys_pairs(gpu.ctx, jkm.LEFT, 2, dts, ptrs, n, ptrs, n, o1.ptr, o2.ptr, 1 << 62, C.byref(m))
    assert rc == AQG_ERR_OVERFLOW and m.value == 4_900_000_000
    assert np.all(o1.to_host() == CANARY) and np.all(o2.to_host() == CANARY)                       # nothing written
    # capacity one too small
    rng = np.random.default_rng(81)
    build, probe = sides(rng, ("i32", "i32"), 500, 2000)
    bd, pd = dev_cols(gpu, build), dev_cols(gpu, probe)
    _, dts, bp = gpu._keyargs(bd)
    _, _, pp = gpu._keyargs(pd)
    for kind in KINDS:
        want = jkm.count(kind, build, probe)
        rc = gpu.lib.aqg_join_keys_pairs(gpu.ctx, kind, 2, dts, bp, 500, pp, 2000, o1.ptr, o2.ptr, want - 1, C.byref(m))
        assert rc == AQG_ERR_OVERFLOW and m.value == want
        assert np.all(o1.to_host() == CANARY) and np.all(o2.to_host() == CANARY)
        rc = gpu.lib.aqg_join_keys_pairs(gpu.ctx, kind, 2, dts, bp, 500, pp, 2000, None, None, 0, C.byref(m))      # NULL outputs: the count alone
        assert rc == AQG_OK and m.value == want


def test_argument_errors(gpu):
    x = gpu.to_device(np.arange(100, dtype=np.int64))
    ts = gpu.to_device(np.zeros(12 * 100, np.uint8))
    out = gpu.to_device(np.full(128, CANARY, np.uint32))
    m = C.c_uint64()
    ptrs = (C.c_void_p * 9)(*[x.ptr] * 9)
    tsp = (C.c_void_p * 9)(*[ts.ptr] * 9)
    def calls(nkeys, dts, bp, pp, kind=0):
        d = (C.c_int * 9)(*(list(dts) + [ck.INT64] * (9 - len(dts))))
        return (gpu.lib.aqg_join_keys_count(gpu.ctx, kind, nkeys, d, bp, 100, pp, 100, C.byref(m)),
                gpu.lib.aqg_join_keys_pairs(gpu.ctx, kind, nkeys, d, bp, 100, pp, 100, out.ptr, out.ptr, 64, C.byref(m)),
                gpu.lib.aqg_join_keys_lookup(gpu.ctx, nkeys, d, bp, 100, pp, 100, out.ptr))
    assert calls(1, [ck.STR], ptrs, ptrs) == (AQG_ERR_DTYPE,) * 3
    assert calls(2, [ck.INT64, ck.LDOUBLE], ptrs, ptrs) == (AQG_ERR_DTYPE,) * 3
    assert calls(0, [], ptrs, ptrs) == (AQG_ERR_ARG,) * 3
    assert calls(9, [ck.INT64] * 9, ptrs, ptrs) == (AQG_ERR_ARG,) * 3
    null = (C.c_void_p * 9)(x.ptr, None, *[x.ptr] * 7)
    assert calls(2, [ck.INT64, ck.INT64], null, ptrs) == (AQG_ERR_ARG,) * 3
    assert calls(2, [ck.INT64, ck.INT64], ptrs, null) == (AQG_ERR_ARG,) * 3
    assert calls(5, [ck.TIMESTAMP] * 5, tsp, tsp) == (AQG_ERR_ARG,) * 3          # ten normalised columns
    assert np.all(out.to_host() == CANARY) and m.value == 0                     # nothing written
    assert calls(1, [ck.INT64], ptrs, ptrs, kind=4)[:2] == (AQG_ERR_ARG,) * 2    # (the look-up has no kind: it runs)
    assert calls(1, [ck.INT64], ptrs, ptrs, kind=-1)[:2] == (AQG_ERR_ARG,) * 2
    d4 = (C.c_int * 4)(*[ck.TIMESTAMP] * 4)                                      # eight normalised columns: accepted
    assert gpu.lib.aqg_join_keys_count(gpu.ctx, 0, 4, d4, tsp, 100, tsp, 100, C.byref(m)) == AQG_OK and m.value == 10_000
    assert gpu.lib.aqg_join_keys_lookup(gpu.ctx, 4, d4, tsp, 100, tsp, 100, out.ptr) == AQG_OK
    got = out.to_host()
    assert np.all(got[:100] == 0) and np.all(got[100:] == CANARY)


# ---- aqg_gather_fill ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.int8, np.uint16, np.float32, np.int64, ck.I128], ids=["1", "2", "4", "8", "16"])
def test_gather_fill(gpu, dt):
    rng = np.random.default_rng(82)
    n, m = 3001, 70_001
    dt = np.dtype(dt)
    x = rng.integers(0, 256, n * dt.itemsize).astype(np.uint8).view(dt)
    if dt.kind == "f":
        x = rng.integers(-1000, 1000, n).astype(dt)
    idx = rng.integers(0, n, m).astype(np.uint32)
    miss = np.zeros(m, bool)
    miss[[0, 1, 7, 8, m - 2, m - 1]] = True
    miss[rng.integers(0, m, m // 5)] = True
    idx[miss] = NONE
    safe = np.where(miss, 0, idx)
    fill = x[5:6].copy()
    fill.view(np.uint8)[:] = np.arange(1, dt.itemsize + 1) * 17 % 251 + 1            # no zero byte, no byte of a neighbour
    for f, fv in ((None, np.zeros(1, dt)), (fill[0], fill)):
        want = x[safe]
        want[miss] = fv[0]
        got = gpu.gather_fill(x, idx, f)
        assert got.tobytes() == want.tobytes()
    xd, idd = gpu.to_device(x), gpu.to_device(idx)
    canary = np.full((m + 2) * dt.itemsize, 0xA5, np.uint8)
    for ioff, ooff in ((0, 1), (1, 0), (1, 1)):                                     # index and output views off the vector width
        od = gpu.to_device(canary)
        rc = gpu.lib.aqg_gather_fill(gpu.ctx, xd.tag, xd.ptr, idd.ptr + 4 * ioff, m - 1, fill.ctypes.data, od.ptr + ooff * dt.itemsize)
        assert rc == AQG_OK
        got = od.to_host().view(dt)
        want = x[safe[ioff:ioff + m - 1]]
        want[miss[ioff:ioff + m - 1]] = fill[0]
        assert got[ooff:ooff + m - 1].tobytes() == want.tobytes()
        assert np.all(got[:ooff].view(np.uint8) == 0xA5) and np.all(got[ooff + m - 1:].view(np.uint8) == 0xA5)
    assert gpu.lib.aqg_gather_fill(gpu.ctx, ck.TIMESTAMP, xd.ptr, idd.ptr, 4, None, xd.ptr) == AQG_ERR_DTYPE
    assert gpu.lib.aqg_gather_fill(gpu.ctx, xd.tag, xd.ptr, None, 4, None, xd.ptr) == AQG_ERR_ARG


def test_left_join_then_gather_fill(gpu):
    """an outer join's build columns end to end: LEFT pairs, then the build side's value column with a fill for the missing rows"""
    rng = np.random.default_rng(83)
    build, probe = sides(rng, ("i32", "i16"), 3000, 20_001)
    val = rng.integers(-10**9, 10**9, 3000).astype(np.int64)
    pr, br = gpu.join_keys_pairs(dev_cols(gpu, build), dev_cols(gpu, probe), jkm.LEFT)
    wp, wb = jkm.pairs(jkm.LEFT, build, probe)
    assert np.array_equal(pr, wp) and np.array_equal(br, wb) and (wb == NONE).sum() > 3000
    want = np.where(wb == NONE, np.int64(-77), val[np.where(wb == NONE, 0, wb)])
    assert np.array_equal(gpu.gather_fill(val, br, -77), want)
