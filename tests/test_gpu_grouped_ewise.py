"""aqg_grouped_ewise: out[i] = v[i] OP s[group of i] (or s[group of i] OP v[i]) for all groups of a build in one launch -- the device form of
the generated loop's `x[val] OP agg(x[val])`.  The expected value is the composition the reference runs: the oracle's element-wise
operator with a HOST scalar, applied group by group to the gathered slice, compared bit for bit (floating results: the bit patterns of
the non-NaN elements and the NaN positions).  The flat layout holds the same elements in the order of the row lists, so its expected
column is the row-order one taken through the row lists."""
import ctypes as C
import os

import numpy as np
import pytest

import checker as ck
from aquery2_amd.capi import AqgError, DevBuf, LAYOUT_FLAT, LAYOUT_ROW

pytestmark = pytest.mark.gpu

# (vt, st, ot): every compute class (int32, uint32, int64, uint64, float, double) and every store width
# (elements per 16-byte store: 16, 8, 4, 2, 1)
TRIPLES = [
    (np.int8, np.int8, ck.INT8),        # int32 arithmetic, 16 elements per store
    (np.int16, np.int32, ck.INT64),     # int32 arithmetic, 2 per store
    (np.uint32, np.int32, ck.UINT32),   # uint32 arithmetic
    (np.int64, np.int64, ck.INT64),     # int64 arithmetic
    (np.uint64, np.uint64, ck.DOUBLE),  # uint64 arithmetic, converted to double
    (np.float32, np.float64, ck.DOUBLE),
    (np.int32, np.float64, ck.DOUBLE),
    (np.int32, np.int32, ck.BOOL),      # 16 per store
    (np.int32, np.int64, ck.INT128),    # 1 per store
    (np.int16, np.float32, ck.FLOAT),   # float arithmetic
    (np.int32, np.int32, ck.INT32),
]
OPS = [ck.OP_SUB, ck.OP_DIV, ck.OP_MOD, ck.OP_LT, ck.OP_GE, ck.OP_ADD, ck.OP_MUL, ck.OP_AND, ck.OP_EQ]
KINDS = [ck.VEC_SCALAR, ck.SCALAR_VEC]


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def fp_class(vt, st):
    return np.dtype(vt).kind == "f" or np.dtype(st).kind == "f"


def refused(op, vt, st):
    """aqg_ewise refuses bitwise operators and % on floating operands; so does the grouped form"""
    return fp_class(vt, st) and op in (ck.OP_MOD, ck.OP_AND, ck.OP_OR, ck.OP_XOR)


def values(rng, dt, n, edges=True):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return np.round(rng.uniform(-100, 100, n), 4).astype(dt)
    info = np.iinfo(dt)
    x = rng.integers(max(info.min, -20000), min(info.max, 20000), n, endpoint=True).astype(dt)
    if edges and n:                                        # the ends of the type: INT_MIN / -1, wrap-around of + - *
        pos = rng.integers(0, n, max(1, n // 50))
        x[pos] = rng.choice(np.array([info.min, info.max, 0], dtype=dt), pos.size)
    return x


def scalars(rng, dt, G):
    """one scalar per group; groups 0 / 1 / 2 (where they exist) get 0 (x / 0, x % 0), -1 (INT_MIN / -1) and the type's minimum"""
    s = values(rng, dt, G, edges=False)
    dt = np.dtype(dt)
    if dt.kind != "f":
        s[s == 0] = 3
        for g, val in enumerate((0, -1 if dt.kind == "i" else np.iinfo(dt).max, np.iinfo(dt).min)):
            if g < G:
                s[g] = val
    return s


class Grouping:
    """a build over n rows and its row-order group ids / flat order, made once per shape"""

    def __init__(self, gpu, keys):
        self.gb = gpu.groupby_build([keys])
        self.G = self.gb.ngroups
        self.n = keys.size
        self.gid = self.gb.reversemap() if self.n else np.zeros(0, np.uint32)
        self.rows = self.gb.postproc()[1] if self.n else np.zeros(0, np.uint32)      # flat position -> row


def make_keys(rng, n, G, skew=False):
    if n == 0:
        return np.zeros(0, np.int32)
    if G >= n:
        return rng.permutation(n).astype(np.int32)                                  # every row a group of its own
    if skew:                                                                        # one group holds 90 % of the rows
        return np.where(rng.random(n) < 0.9, 0, rng.integers(0, G, n)).astype(np.int32)
    return rng.integers(0, G, n).astype(np.int32)


def expected_rows(oracle, op, kind, v, s, gid, G, ot):
    """the reference's composition in row order: oracle ewise with the HOST scalar s[g] over group g's rows"""
    out = np.zeros(v.size, dtype=ck.TAG2NP[ot])
    order = np.argsort(gid, kind="stable")
    bounds = np.searchsorted(gid[order], np.arange(G + 1))
    vs = v[order]
    tmp = np.zeros(v.size, dtype=ck.TAG2NP[ot])
    for g in range(G):
        a, b = int(bounds[g]), int(bounds[g + 1])
        if a == b:
            continue
        sc = s[g]
        tmp[a:b] = oracle.ewise(op, vs[a:b], sc, ot=ot) if kind == ck.VEC_SCALAR else oracle.ewise(op, sc, vs[a:b], ot=ot)
    out[order] = tmp
    return out


def same(got, want):
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        return np.array_equal(gn, wn) and got[~gn].tobytes() == want[~wn].tobytes()
    return got.tobytes() == want.tobytes()


def run(gpu, grp, layout, op, kind, v, s, ot, misaligned=False):
    vin = v[grp.rows] if layout == LAYOUT_FLAT else v
    if not misaligned:
        return gpu.grouped_ewise(grp.gb, op, vin, s, kind=kind, layout=layout, ot=ot)
    # v and out one element past a 16-byte boundary: the element-at-a-time path of the same kernel
    odt = ck.TAG2NP[ot]
    base = gpu.to_device(np.concatenate([vin[:1], vin]))
    obase = gpu.empty(vin.size + 1, odt)
    vv = DevBuf(gpu, base.ptr + vin.dtype.itemsize, vin.dtype, vin.size, owned=False)
    ov = DevBuf(gpu, obase.ptr + odt.itemsize, odt, vin.size, owned=False)
    return gpu.grouped_ewise(grp.gb, op, vv, s, kind=kind, layout=layout, ot=ot, out=ov, keep=True).to_host()


def check(gpu, oracle, grp, rng, triple, op, kind, layouts=(LAYOUT_ROW, LAYOUT_FLAT), misaligned=False):
    vt, st, ot = triple
    v, s = values(rng, vt, grp.n), scalars(rng, st, max(grp.G, 1))[:grp.G]
    if refused(op, vt, st):
        if grp.n:
            with pytest.raises(AqgError) as e:
                run(gpu, grp, LAYOUT_ROW, op, kind, v, s, ot)
            assert e.value.code == 2
        return
    want = expected_rows(oracle, op, kind, v, s, grp.gid, grp.G, ot)
    for layout in layouts:
        got = run(gpu, grp, layout, op, kind, v, s, ot, misaligned)
        w = want[grp.rows] if layout == LAYOUT_FLAT else want
        assert same(got, w), (triple, op, kind, layout, grp.n, grp.G, misaligned)


@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: f"{np.dtype(t[0]).name}-{np.dtype(t[1]).name}-{t[2]}")
def test_every_type_triple_op_kind_and_layout(gpu, oracle, triple):
    """4 * 256 + 3 rows in 7 groups (a vector tail behind one full workgroup of int32 vectors) and 70 001 rows in 300 groups (several
    workgroups, a ragged end): every operator of the list, both operand orders, both layouts, integer edge scalars (0, -1, minimum)"""
    rng = np.random.default_rng(1234 + TRIPLES.index(triple))
    for n, G in ((4 * 256 + 3, 7), (70_001, 300)):
        grp = Grouping(gpu, make_keys(rng, n, G))
        for op in OPS:
            for kind in KINDS:
                check(gpu, oracle, grp, rng, triple, op, kind)


SHAPES = [(n, G, False) for n in (0, 1, 3, 4 * 256 + 3, 70_001) for G in sorted({1, 7, 300, n}) if G <= max(n, 1)] + [(70_001, 300, True), (4 * 256 + 3, 7, True)]


@pytest.mark.parametrize("n,G,skew", SHAPES)
def test_shapes(gpu, oracle, n, G, skew):
    """below one vector, a vector tail, several workgroups with a ragged end; one group, a few, many, every row its own group; one group
    with 90 % of the rows -- for store widths 16, 4, 2 and 1, in both layouts and operand orders"""
    rng = np.random.default_rng(n * 31 + G + skew)
    grp = Grouping(gpu, make_keys(rng, n, G, skew))
    assert grp.G == (n if G >= n else grp.G) <= min(max(G, 0), n)
    many = grp.G > 5000                                                  # (a host-scalar oracle call per group: keep those few)
    for i, triple in enumerate([TRIPLES[10], TRIPLES[0], TRIPLES[6], TRIPLES[8]]):
        for op in ((ck.OP_SUB,) if many else (ck.OP_SUB, ck.OP_DIV)):
            for kind in (KINDS if not many or i == 0 else KINDS[i % 2:i % 2 + 1]):      # (many: the other store widths in one operand order each)
                check(gpu, oracle, grp, rng, triple, op, kind)


@pytest.mark.parametrize("triple", [TRIPLES[0], TRIPLES[10], TRIPLES[6], TRIPLES[8], TRIPLES[7]], ids=lambda t: f"{np.dtype(t[0]).name}-{t[2]}")
def test_misaligned_operands(gpu, oracle, triple):
    """v and out offset by one element from a 16-byte boundary"""
    rng = np.random.default_rng(77)
    grp = Grouping(gpu, make_keys(rng, 4 * 256 + 3, 7))
    for op in (ck.OP_SUB, ck.OP_DIV, ck.OP_LT):
        for kind in KINDS:
            check(gpu, oracle, grp, rng, triple, op, kind, misaligned=True)


def test_integer_edge_scalars(gpu, oracle):
    """a group whose scalar is 0 under DIV / MOD (defined as 0), INT32_MIN over -1 (wraps), in both operand orders"""
    keys = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 2], np.int32)
    grp = Grouping(gpu, keys)
    lo = np.iinfo(np.int32).min
    v = np.array([lo, lo, lo, 7, 7, 7, -1, -1, 0, 0], np.int32)
    s = np.array([0, -1, lo], np.int32)
    for op in (ck.OP_DIV, ck.OP_MOD):
        for kind in KINDS:
            want = expected_rows(oracle, op, kind, v, s, grp.gid, grp.G, ck.INT32)
            for layout in (LAYOUT_ROW, LAYOUT_FLAT):
                got = gpu.grouped_ewise(grp.gb, op, v[grp.rows] if layout else v, s, kind=kind, layout=layout, ot=ck.INT32)
                assert np.array_equal(got, want[grp.rows] if layout else want), (op, kind, layout)
    got = gpu.grouped_ewise(grp.gb, ck.OP_DIV, v, s, ot=ck.INT32)
    assert got[0] == 0 and got[3] == 0 and got[1] == lo and got[4] == -7            # x / 0 = 0; INT32_MIN / -1 wraps to INT32_MIN


def test_errors_and_empty(gpu):
    lib = gpu.lib
    keys = np.arange(10, dtype=np.int32) % 3
    x = gpu.to_device(np.arange(10, dtype=np.int32))
    s = gpu.to_device(np.arange(3, dtype=np.int32))
    s128 = gpu.to_device(np.zeros(3, ck.I128))
    sentinel = np.full(10, -7, np.int32)
    out = gpu.to_device(sentinel)
    gb = gpu.groupby_build([keys])

    def call(h, layout, op, kind, vt, v, st, sp, ot, o, ctx=gpu.ctx):
        return lib.aqg_grouped_ewise(ctx, h, layout, op, kind, vt, C.c_void_p(v), st, C.c_void_p(sp), ot, C.c_void_p(o))
    ok = (gb.h, LAYOUT_ROW, ck.OP_SUB, ck.VEC_SCALAR, ck.INT32, x.ptr, ck.INT32, s.ptr, ck.INT32, out.ptr)
    assert call(*ok[:3], ck.VEC_VEC, *ok[4:]) == 3                                   # kind
    assert call(*ok[:2], 14, *ok[3:]) == 3 and call(ok[0], 2, *ok[2:]) == 3          # op, layout
    assert call(*ok[:5], None, *ok[6:]) == 3 and call(*ok[:7], None, *ok[8:]) == 3 and call(*ok[:9], None) == 3      # null operands
    assert call(*ok, ctx=None) == 3
    assert call(*ok[:6], ck.INT128, s128.ptr, *ok[8:]) == 2                          # 128-bit scalar column
    assert call(*ok[:4], ck.INT128, *ok[5:]) == 2 and call(*ok[:4], ck.STR, *ok[5:]) == 2
    assert call(*ok[:6], ck.DOUBLE, *ok[7:8], ck.INT128, ok[9]) == 2                 # what aqg_ewise refuses: 128-bit result of floating arithmetic
    assert call(*ok[:2], ck.OP_MOD, ok[3], *ok[4:6], ck.DOUBLE, *ok[7:]) == 2
    assert call(*ok[:8], 99, ok[9]) == 2                                             # no such result dtype
    assert np.array_equal(out.to_host(), sentinel)
    # a fused group-by handle has neither reversemap nor row lists
    agg = gpu.groupby_agg([keys], [ck.RED_SUM], [np.arange(10, dtype=np.int32)])
    with pytest.raises(AqgError) as e:
        gpu.grouped_ewise(agg, ck.OP_SUB, x, s)
    assert e.value.code == 3
    # no groups: AQG_OK, nothing written
    gb0 = gpu.groupby_build([np.zeros(0, np.int32)])
    assert gb0.ngroups == 0
    assert call(gb0.h, *ok[1:]) == 0 and call(gb0.h, LAYOUT_FLAT, *ok[2:]) == 0
    assert np.array_equal(out.to_host(), sentinel)
    assert len(gpu.grouped_ewise(gb0, ck.OP_SUB, np.zeros(0, np.int32), np.zeros(0, np.int32))) == 0


@pytest.mark.parametrize("seed", range(int(os.environ.get("AQG_FUZZ_SEEDS", "40"))))
def test_random_cases(gpu, oracle, seed):
    rng = np.random.default_rng(int(os.environ.get("AQG_FUZZ_BASE", "9000")) + seed)
    n = int(rng.choice([1, 5, 255, 1024, 4099, 65_537, 200_000]))
    G = int(rng.choice([1, 2, 33, 300, 2000]))
    grp = Grouping(gpu, make_keys(rng, n, min(G, n), skew=bool(rng.random() < 0.25)))
    for _ in range(3):
        triple = TRIPLES[rng.integers(len(TRIPLES))]
        op = int(rng.integers(0, 14))
        kind = KINDS[rng.integers(2)]
        layout = (LAYOUT_ROW, LAYOUT_FLAT)[rng.integers(2)]
        check(gpu, oracle, grp, rng, triple, op, kind, layouts=(layout,), misaligned=bool(rng.random() < 0.2))
