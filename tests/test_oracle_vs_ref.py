"""Pins the C restatement (oracle/aq_oracle.c) against the REAL reference library on seeded random inputs, bit for bit: against
the digests of its answers recorded in tests/golden/ref_digests.json (oracle/gen_ref_digests.py) everywhere, and against the library
itself (oracle/_ref/libaqref.so, built by oracle/Makefile) where it is built."""
import numpy as np
import pytest

import checker as ck

NUM_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64]
BIN_DTYPES = [np.int16, np.int32, np.int64, np.uint32, np.float32, np.float64]


def rand(rng, dt, n, small=False):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return (rng.uniform(-100, 100, n)).astype(dt)
    hi = 12 if small else min(np.iinfo(dt).max, 20000)
    lo = 1 if (dt.kind == "u" or small) else max(np.iinfo(dt).min, -20000)
    return rng.integers(lo, hi, n, endpoint=True).astype(dt)


def nm(dt):
    return np.dtype(dt).name


@pytest.mark.parametrize("dt", NUM_DTYPES)
def test_type_rules(oracle, ref_answers, dt):
    R = ref_answers.check
    t = ck.NP2TAG[np.dtype(dt)]
    k = f"type_rules/{nm(dt)}"
    R(f"{k}/long_type", oracle.long_type(t), lambda r: r.long_type(t))
    R(f"{k}/fp_type", oracle.fp_type(t), lambda r: r.fp_type(t))
    for dt2 in NUM_DTYPES:
        t2 = ck.NP2TAG[np.dtype(dt2)]
        R(f"{k}/coercion/{nm(dt2)}", oracle.coercion(t, t2), lambda r: r.coercion(t, t2))
    for op in range(9):
        R(f"{k}/reduce_out/{op}", oracle.reduce_out_dtype(op, t), lambda r: r.reduce_out_dtype(op, t))
    for op in range(12):
        R(f"{k}/scan_out/{op}", oracle.scan_out_dtype(op, t), lambda r: r.scan_out_dtype(op, t))


@pytest.mark.parametrize("dt", NUM_DTYPES)
@pytest.mark.parametrize("n", [0, 1, 2, 7, 1000])
def test_reduce(oracle, ref_answers, dt, n):
    rng = np.random.default_rng(n * 31 + np.dtype(dt).num)
    x = rand(rng, dt, n)
    for name, op in ck.RED_NAMES.items():
        if n == 0 and name in ("avg",):
            continue  # 0/0 = NaN on both sides
        ref_answers.check(f"reduce/{nm(dt)}/{n}/{name}", oracle.reduce(op, x), lambda r: r.reduce(op, x))


@pytest.mark.parametrize("dt", NUM_DTYPES)
@pytest.mark.parametrize("n", [0, 1, 5, 257])
def test_scan(oracle, ref_answers, dt, n):
    rng = np.random.default_rng(n * 17 + np.dtype(dt).num)
    x = rand(rng, dt, n)
    x[x == 0] = 1
    for name, op in ck.SCAN_NAMES.items():
        if name in ("vars", "stddevs", "varw", "stddevw"):
            continue  # not callable in the reference (printf in loop / out-of-bounds read)
        for w in (0, 1, 2, 3, 10, 256, 257, 1000):
            if w == 0 and name in ("ratiow", "sumw", "avgw"):
                continue  # undefined in the reference (reads ret[-1] / divides by zero)
            ref_answers.check(f"scan/{nm(dt)}/{n}/{name}/{w}", oracle.scan(op, x, w), lambda r: r.scan(op, x, w))


@pytest.mark.parametrize("lt", BIN_DTYPES)
@pytest.mark.parametrize("rt", BIN_DTYPES)
def test_ewise_free_ops(oracle, ref_answers, lt, rt):
    R = ref_answers.check
    rng = np.random.default_rng(np.dtype(lt).num * 100 + np.dtype(rt).num)
    n = 301
    l, r = rand(rng, lt, n), rand(rng, rt, n)
    r[r == 0] = 3
    l[l == 0] = 5
    tl, tr = ck.NP2TAG[np.dtype(lt)], ck.NP2TAG[np.dtype(rt)]
    for op in (ck.OP_ADD, ck.OP_SUB, ck.OP_MUL, ck.OP_DIV, ck.OP_GT):
        k = f"ewise/{nm(lt)}/{nm(rt)}/{op}"
        R(f"{k}/out", oracle.ewise_out_dtype(op, tl, tr), lambda ref: ref.ewise_out_dtype(op, tl, tr))
        R(f"{k}/vv", oracle.ewise(op, l, r), lambda ref: ref.ewise(op, l, r))
        R(f"{k}/vs", oracle.ewise(op, l, r[7]), lambda ref: ref.ewise(op, l, r[7]))
        R(f"{k}/sv", oracle.ewise(op, l[9], r), lambda ref: ref.ewise(op, l[9], r))


@pytest.mark.parametrize("lt", BIN_DTYPES)
@pytest.mark.parametrize("rt", BIN_DTYPES)
def test_ewise_aqop(oracle, ref_answers, lt, rt):
    R = ref_answers.check
    rng = np.random.default_rng(np.dtype(lt).num * 7 + np.dtype(rt).num)
    n = 130
    l, r = rand(rng, lt, n, small=True), rand(rng, rt, n, small=True)
    for op in (ck.OP_LT, ck.OP_GE, ck.OP_LE, ck.OP_EQ, ck.OP_NE):
        R(f"aqop/{nm(lt)}/{nm(rt)}/{op}", oracle.ewise(op, l, r, ot=ck.BOOL), lambda ref: ref.ewise(op, l, r, ot=ck.BOOL))
    if np.dtype(lt).kind != "f" and np.dtype(rt).kind != "f":
        for op in (ck.OP_AND, ck.OP_OR, ck.OP_XOR):
            R(f"aqop/{nm(lt)}/{nm(rt)}/{op}", oracle.ewise(op, l, r, ot=ck.INT32), lambda ref: ref.ewise(op, l, r, ot=ck.INT32))


@pytest.mark.parametrize("dt", [np.int32, np.int64, np.float32, np.float64, np.uint8])
def test_unary(oracle, ref_answers, dt):
    R = ref_answers.check
    rng = np.random.default_rng(5)
    x = np.abs(rand(rng, dt, 100))
    R(f"unary/{nm(dt)}/sqrt", oracle.unary(ck.UN_SQRT, x), lambda r: r.unary(ck.UN_SQRT, x))
    if np.dtype(dt).kind == "f":
        for p in (0, 2, 6, 7, 20):
            R(f"unary/{nm(dt)}/truncate/{p}", oracle.unary(ck.UN_TRUNCATE, x, p), lambda r: r.unary(ck.UN_TRUNCATE, x, p))


@pytest.mark.parametrize("lt", BIN_DTYPES)
@pytest.mark.parametrize("rt", BIN_DTYPES)
def test_corr(oracle, ref_answers, lt, rt):
    rng = np.random.default_rng(11)
    x, y = rand(rng, lt, 500, small=True), rand(rng, rt, 500, small=True)
    ref_answers.check(f"corr/{nm(lt)}/{nm(rt)}", np.float64(oracle.corr(x, y)), lambda r: np.float64(r.corr(x, y)))


@pytest.mark.parametrize("dt", NUM_DTYPES)
def test_gather_compact(oracle, ref_answers, dt):
    R = ref_answers.check
    rng = np.random.default_rng(3)
    x = rand(rng, dt, 400)
    idx = rng.integers(0, 400, 1000).astype(np.uint32)
    R(f"gather/{nm(dt)}", oracle.gather(x, idx), lambda r: r.gather(x, idx))
    mask = rng.integers(0, 2, 400).astype(np.uint8)
    R(f"compact/{nm(dt)}", oracle.compact(x, mask), lambda r: r.compact(x, mask))
    assert oracle.compact(x, np.zeros(400, np.uint8)).size == 0


def test_hash_kats(oracle, ref_answers):
    R = ref_answers.check
    # SURVEY 8c a16
    assert oracle.hash_scalar(np.int32(7)) == 6018027440424182935
    assert oracle.hash_tuple([np.int32(3), np.int32(4)]) == 11708105269577805707
    R("hash/kat_scalar_7", oracle.hash_scalar(np.int32(7)), lambda r: r.hash_scalar(np.int32(7)))
    R("hash/kat_tuple_3_4", oracle.hash_tuple([np.int32(3), np.int32(4)]), lambda r: r.hash_tuple([np.int32(3), np.int32(4)]))
    rng = np.random.default_rng(1)
    for i, v in enumerate(rng.integers(-2**31, 2**31 - 1, 50)):
        R(f"hash/scalar/{i}", oracle.hash_scalar(np.int32(v)), lambda r: r.hash_scalar(np.int32(v)))
    for i in range(20):
        vals = [np.int32(v) for v in rng.integers(-1000, 1000, 6)]
        for k in (1, 2, 3, 6):
            R(f"hash/tuple/{i}/{k}", oracle.hash_tuple(vals[:k]), lambda r: r.hash_tuple(vals[:k]))


GB_CASES = [
    (1, 1000, 10), (1, 5000, 100), (1, 3000, 3000), (2, 4000, 20), (3, 4000, 8), (6, 3000, 3), (1, 1, 1), (2, 17, 2),
]


@pytest.mark.parametrize("nk,n,card", GB_CASES)
def test_groupby(oracle, ref_answers, nk, n, card):
    R = ref_answers.check
    rng = np.random.default_rng(nk * 1000 + n + card)
    keys = [rng.integers(-card, card, n).astype(np.int32) for _ in range(nk)]
    a = oracle.groupby(keys)
    k = f"groupby/{nk}/{n}/{card}"
    R(f"{k}/ngroups", a["ngroups"], lambda r: r.groupby(keys)["ngroups"])
    for f in ("reversemap", "counts", "first_rows", "offsets", "row_ids"):
        R(f"{k}/{f}", a[f], lambda r: r.groupby(keys)[f])
    for vdt in (np.int32, np.float32, np.int64, np.float64):
        v = rand(rng, vdt, n, small=True)
        for name in ("sum", "min", "max", "count", "avg", "first", "last", "var"):
            op = ck.RED_NAMES[name]
            R(f"{k}/{nm(vdt)}/{name}", oracle.grouped_reduce(op, v, a), lambda r: r.grouped_reduce(op, v, r.groupby(keys)))


def test_groupby_int64_key(oracle, ref_answers):
    rng = np.random.default_rng(8)
    k = (rng.integers(0, 50, 2000).astype(np.int64) << 33) - 7
    a = oracle.groupby([k])
    for f in ("reversemap", "counts", "first_rows", "offsets", "row_ids"):
        ref_answers.check(f"groupby_int64_key/{f}", a[f], lambda r: r.groupby([k])[f])
