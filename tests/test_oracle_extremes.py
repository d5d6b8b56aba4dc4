"""The oracle at the numeric extremes (CPU only): against a model of the C++ rules that does not come from it (tests/extremes.py),
against the real reference where C++ defines the answer, and against exact python arithmetic where a 128-bit sum has to be rounded
to a double.

Oracle vs model: all 11 x 11 operand type pairs, every operation the pair accepts (14 for integer pairs, 10 where an operand is
floating), the three kinds, over the full product of the two types' pools; the result type is the reference's default where it has
one (the expression's own type otherwise), and on one pair per compute type every other result type the call accepts.  Integer and
bool results bit for bit; floating results bit for bit where finite or infinite, NaN where NaN.

Oracle vs the real reference (`ref_answers`, keys under `x/`; related questions are recorded as one digest, see Bundle): the reference is built without -fwrapv and traps on integer
division, so a row of a question reaches it only if `extremes.defined_in_cxx` says C++ defines it (no zero divisor, no
INT_MIN / -1, no signed overflow in the compute type; computed in python int).  Over the 36 pairs of the reference's six binary
types that predicate removes 7342 of 349547 rows (REMOVED_ROWS / ASKED_ROWS below, asserted by
test_defined_predicate_counts) and leaves at least one row to every (pair, operation, kind).  Reductions and scans of all ten
types run over a pool + 500 full-range values column; `deltas` and `avgw` of int32 / int64 take that column halved, because
`arr[i] - arr[i-1]` must not overflow there either (asserted by scan_defined).
"""
import numpy as np
import pytest

import checker as ck
import extremes as ex
import golden_util as gu

REMOVED_ROWS, ASKED_ROWS = 7342, 349547                # rows the predicate removes / rows before it (test_defined_predicate_counts)

PAIRS = [(lt, rt) for lt in ex.OPERAND_DTYPES for rt in ex.OPERAND_DTYPES]
BIN_PAIRS = [(lt, rt) for lt in ex.BIN_DTYPES for rt in ex.BIN_DTYPES]
pair_id = lambda p: f"{ex.nm(p[0])}-{ex.nm(p[1])}"


class Bundle:
    """Many questions to the reference recorded as ONE digest (the digests of the parts, joined): the recorded file grows by a line per
    bundle, not per question.  Where the reference is built every part is compared on its own first, so a failure names the part."""

    def __init__(self):
        self.parts = []

    def add(self, name, got, ask):
        self.parts.append((name, ex.canon_nan(got), lambda ref, ask=ask: ex.canon_nan(ask(ref))))

    def check(self, ref_answers, key):
        assert self.parts, key
        if ref_answers.live is not None:
            for name, got, ask in self.parts:
                assert gu.digest(got) == gu.digest(ask(ref_answers.live)), f"{key}: {name}: the oracle differs from the live reference"
        join = lambda vals: "".join(gu.digest(v) for v in vals).encode()
        ref_answers.check(key, join(g for _, g, _ in self.parts), lambda ref: join(a(ref) for _, _, a in self.parts))


def check_model(oracle, op, l, r, kind, ot, what):
    got, want = oracle.ewise(op, l, r, ot=ot), ex.model_ewise(op, l, r, kind, ot)
    if not ex.same(got, want):
        i = ex.first_diff(got, want)
        la, ra = np.atleast_1d(l), np.atleast_1d(r)
        raise AssertionError(f"{what}: row {i}: {la[i % len(la)]!r} {ex.OP_NAME[op]} {ra[i % len(ra)]!r} -> oracle {got[i]!r}, model {want[i]!r}")


def kinds_of(l, r, lt, rt):
    """(kind, l, r) over the product columns and over the pool against each scalar of the other type"""
    yield "vv", l, r
    for s in ex.scalars(rt):
        yield "vs", ex.pool(lt), s
    for s in ex.scalars(lt):
        yield "sv", s, ex.pool(rt)


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_oracle_vs_model(oracle, pair):
    lt, rt = pair
    l, r = ex.product_columns(lt, rt)
    for op in ex.ops_for(lt, rt):
        ot = ex.default_ot(oracle, op, lt, rt)
        for kind, a, b in kinds_of(l, r, lt, rt):
            check_model(oracle, op, a, b, kind, ot, f"{ex.nm(lt)} {ex.nm(rt)} {kind} -> {ex.OT_NAME[ot]}")
    if ex.compute_type(lt, rt)[0] == "f":
        for op in ex.INT_ONLY_OPS:                       # rejected, not computed
            with pytest.raises(ck.CheckerError):
                oracle.ewise(op, l, r, ot=ck.INT32)


@pytest.mark.parametrize("ctype", list(ex.OT_SWEEP_PAIRS), ids=lambda c: f"{c[0]}{c[1]}")
def test_oracle_vs_model_every_result_type(oracle, ctype):
    lt, rt = (np.dtype(t) for t in ex.OT_SWEEP_PAIRS[ctype])
    assert ex.compute_type(lt, rt) == ctype
    l, r = ex.product_columns(lt, rt)
    for op in ex.ops_for(lt, rt):
        for ot in ex.accepted_ots(op, lt, rt):
            check_model(oracle, op, l, r, "vv", ot, f"vv -> {ex.OT_NAME[ot]}")
            check_model(oracle, op, ex.pool(lt), ex.scalars(rt)[1], "vs", ot, f"vs -> {ex.OT_NAME[ot]}")
            check_model(oracle, op, ex.scalars(lt)[2], ex.pool(rt), "sv", ot, f"sv -> {ex.OT_NAME[ot]}")


def test_model_rejects_what_cxx_leaves_undefined():
    f, i = np.array([1.5e300]), np.array([3], np.int32)
    with pytest.raises(ValueError):
        ex.model_ewise(ck.OP_MUL, f, i, "vv", ck.INT32)          # floating value to an integer result
    with pytest.raises(ValueError):
        ex.model_ewise(ck.OP_MOD, f, i, "vv", ck.DOUBLE)
    with pytest.raises(ValueError):
        ex.model_ewise(ck.OP_GT, f, i, "vv", ck.INT128)
    assert ex.model_ewise(ck.OP_GT, f, i, "vv", ck.INT8).tolist() == [1]     # a comparison's 0 / 1 may go anywhere


def test_compute_type_is_the_cxx_one():
    C = ex.compute_type
    assert C(np.int8, np.uint8) == ("i", 32) and C(np.uint16, np.bool_) == ("i", 32)
    assert C(np.int32, np.uint32) == ("u", 32) and C(np.int64, np.uint32) == ("i", 64)
    assert C(np.int64, np.uint64) == ("u", 64) and C(np.uint64, np.float32) == ("f", 32) and C(np.float32, np.float64) == ("f", 64)


# ---- oracle vs the real reference --------------------------------------------------------------------------------------------------
REF_FREE_OPS = (ck.OP_ADD, ck.OP_SUB, ck.OP_MUL, ck.OP_DIV, ck.OP_GT)      # the reference's free operators: all three kinds
REF_CMP_OPS = (ck.OP_LT, ck.OP_GE, ck.OP_LE, ck.OP_EQ, ck.OP_NE)           # aqop_*: vec-vec only, the caller names the result type
REF_BIT_OPS = (ck.OP_AND, ck.OP_OR, ck.OP_XOR)


def ref_ewise_questions(lt, rt):
    """(key, op, kind, l, r, ot, rows before the predicate) of one pair: operands already cut down to the rows C++ defines"""
    l, r = ex.binary_columns(lt, rt, len(ex.pool(lt)) * len(ex.pool(rt)) + 500, 900 + ex.tag(lt) * 31 + ex.tag(rt))
    base = f"x/ewise/{ex.nm(lt)}/{ex.nm(rt)}"
    integer = ex.compute_type(lt, rt)[0] != "f"
    for op in REF_FREE_OPS + REF_CMP_OPS + (REF_BIT_OPS if integer else ()):
        ot = None if op in REF_FREE_OPS else (ck.BOOL if op in REF_CMP_OPS else ck.INT64)
        m = ex.defined_rows(op, l, r, "vv")
        yield f"{base}/{ex.OP_NAME[op]}/vv", op, "vv", l[m], r[m], ot, len(m)
        if op not in REF_FREE_OPS:
            continue
        for i, s in enumerate(ex.scalars(rt)):
            a = ex.pool(lt)
            m = ex.defined_rows(op, a, s, "vs")
            yield f"{base}/{ex.OP_NAME[op]}/vs/{i}", op, "vs", a[m], s, ot, len(m)
        for i, s in enumerate(ex.scalars(lt)):
            b = ex.pool(rt)
            m = ex.defined_rows(op, s, b, "sv")
            yield f"{base}/{ex.OP_NAME[op]}/sv/{i}", op, "sv", s, b[m], ot, len(m)


@pytest.mark.parametrize("pair", BIN_PAIRS, ids=pair_id)
def test_ref_ewise(oracle, ref_answers, pair):
    lt, rt = pair
    tl, tr = ex.tag(lt), ex.tag(rt)
    left, bundles = {}, {}
    for key, op, kind, l, r, ot, _ in ref_ewise_questions(lt, rt):
        n = np.size(l) if kind != "sv" else np.size(r)
        left[(op, kind)] = left.get((op, kind), 0) + n
        if n == 0:
            continue                                     # this scalar leaves no defined row (a zero divisor); others do, see below
        b = bundles.setdefault("free" if op in REF_FREE_OPS else "aqop", Bundle())
        if ot is None and kind == "vv":
            b.add(f"{key}: result type", oracle.ewise_out_dtype(op, tl, tr), lambda ref, op=op: ref.ewise_out_dtype(op, tl, tr))
        b.add(key, oracle.ewise(op, l, r, ot=ot), lambda ref, op=op, l=l, r=r, ot=ot: ref.ewise(op, l, r, ot=ot))
    assert all(v > 0 for v in left.values()), left       # a defined question for every (pair, operation, kind)
    for group, b in bundles.items():                     # two recorded digests per pair: the free operators (three kinds, every scalar), aqop_*
        b.check(ref_answers, f"x/ewise/{ex.nm(lt)}/{ex.nm(rt)}/{group}")


def test_defined_predicate_counts():
    asked = kept = 0
    for lt, rt in BIN_PAIRS:
        for _, op, kind, l, r, _, before in ref_ewise_questions(lt, rt):
            asked += before
            kept += np.size(l) if kind != "sv" else np.size(r)
    assert (asked - kept, asked) == (REMOVED_ROWS, ASKED_ROWS)


def test_defined_predicate():
    D = ex.defined_in_cxx
    i32, i64, u32, i16 = np.int32, np.int64, np.uint32, np.int16
    assert not D(ck.OP_DIV, i32, i32, 5, 0) and not D(ck.OP_DIV, i32, i32, -2**31, -1) and D(ck.OP_DIV, i32, i32, -2**31 + 1, -1)
    assert not D(ck.OP_ADD, i32, i32, 2**31 - 1, 1) and D(ck.OP_ADD, i32, u32, 2**31 - 1, 1)       # unsigned compute type wraps by definition
    assert D(ck.OP_MUL, i16, i16, -2**15, 2**15 - 1)                                   # int16 * int16 is computed in int: fits
    assert not D(ck.OP_MUL, i64, i32, 2**62, 2) and D(ck.OP_SUB, i64, i32, -2**63, 0) and not D(ck.OP_SUB, i64, i32, -2**63, 1)
    assert D(ck.OP_DIV, np.float32, i32, 1.0, 0) and D(ck.OP_GT, i32, i32, -2**31, 2**31 - 1)


def scan_defined(name, x, w):
    """whether C++ defines the reference's loop for this scan: `deltas` and `avgw` subtract two elements in the promoted element type"""
    dt = x.dtype
    if dt.kind != "i" or dt.itemsize < 4 or name not in ("deltas", "avgw"):
        return True
    v, d = x.tolist(), (1 if name == "deltas" else w)
    lim = 1 << (dt.itemsize * 8 - 1)
    return all(-lim <= v[i] - v[i - d] < lim for i in range(d, len(v)))


def mixed_column(dt, seed=77):
    return ex.unary_column(dt, len(ex.pool(dt)) + 500, seed + ex.tag(dt))


@pytest.mark.parametrize("dt", ex.NUM_DTYPES, ids=ex.nm)
def test_ref_reduce_and_scan(oracle, ref_answers, dt):
    x = mixed_column(dt)
    half = x >> 1 if dt.kind == "i" and dt.itemsize >= 4 else x
    k = f"x/col/{ex.nm(dt)}"
    b = Bundle()
    for name, op in ck.RED_NAMES.items():
        if name in ("var", "stddev"):
            continue                                     # squares of full-range values overflow: not defined in the reference
        b.add(name, oracle.reduce(op, x), lambda r, op=op: r.reduce(op, x))
    b.check(ref_answers, f"{k}/reduce")
    b = Bundle()
    for name, op in ck.SCAN_NAMES.items():
        if name in ("vars", "stddevs", "varw", "stddevw"):
            continue
        for w in (1, 3, 100, 600):
            col = x if scan_defined(name, x, w) else half
            assert scan_defined(name, col, w), (name, w)
            b.add(f"{name} w={w}", oracle.scan(op, col, w), lambda r, op=op, col=col, w=w: r.scan(op, col, w))
    b.check(ref_answers, f"{k}/scan")


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_ref_floating_columns_with_nans_and_both_zeros(oracle, ref_answers, dt):
    rng = np.random.default_rng(5)
    x = rng.uniform(-10, 10, 300).astype(dt)
    x[rng.integers(0, 300, 40)] = 0.0
    x[rng.integers(0, 300, 40)] = -0.0
    y = x.copy()
    y[[0, 17, 150, 299]] = np.nan
    for tagname, col in (("zeros", x), ("nans", y)):
        b = Bundle()
        for name in ("min", "max", "sum", "avg", "first", "last"):
            b.add(name, oracle.reduce(ck.RED_NAMES[name], col), lambda r, op=ck.RED_NAMES[name], col=col: r.reduce(op, col))
        for name, op in ck.SCAN_NAMES.items():
            if name in ("vars", "stddevs", "varw", "stddevw"):
                continue
            b.add(name, oracle.scan(op, col, 5), lambda r, op=op, col=col: r.scan(op, col, 5))
        b.check(ref_answers, f"x/fp/{ex.nm(dt)}/{tagname}")


@pytest.mark.parametrize("dt", ex.NUM_DTYPES, ids=ex.nm)
def test_ref_sqrt_truncate(oracle, ref_answers, dt):
    x = mixed_column(dt, 91)
    b = Bundle()
    b.add("sqrt", oracle.unary(ck.UN_SQRT, x), lambda r: r.unary(ck.UN_SQRT, x))
    if dt.kind == "f":
        for p in ex.TRUNC_P:
            t = ex.truncate_column(dt, p)
            b.add(f"truncate p={p}", oracle.unary(ck.UN_TRUNCATE, t, p), lambda r, t=t, p=p: r.unary(ck.UN_TRUNCATE, t, p))
    b.check(ref_answers, f"x/unary/{ex.nm(dt)}")


@pytest.mark.parametrize("dt", [np.dtype(np.int64), np.dtype(np.uint64)], ids=ex.nm)
def test_ref_large_sums(oracle, ref_answers, dt):
    """4097 rows of the type's maximum, then rounding probes: the 128-bit sum carries 4096 times and avg / avgs round it"""
    x = np.concatenate([np.full(4097, np.iinfo(dt).max, dtype=dt), np.array([1, 1, 1023, 1, 2**40, 1], dtype=dt)])
    b = Bundle()
    for name in ("sum", "avg"):
        b.add(name, oracle.reduce(ck.RED_NAMES[name], x), lambda r, op=ck.RED_NAMES[name]: r.reduce(op, x))
    assert oracle.reduce(ck.RED_SUM, x) == ex.exact_sum(x)
    for name in ("sums", "avgs"):
        b.add(name, oracle.scan(ck.SCAN_NAMES[name], x), lambda r, op=ck.SCAN_NAMES[name]: r.scan(op, x))
    b.check(ref_answers, f"x/large/{ex.nm(dt)}")


@pytest.mark.parametrize("dt", [np.dtype(np.int64), np.dtype(np.uint64)], ids=ex.nm)
def test_ref_avgs_first_row_a_double_cannot_hold(oracle, ref_answers, dt):
    """`s = ret[0] = arr[0]`: the reference's avgs (and the growing part of avgw) sums from the first row rounded to double"""
    b = Bundle()
    for k, first in enumerate(ex.unrepresentable_first_rows(dt)):
        x = ex.unary_column(dt, 300, 55 + k)
        x[0] = first
        assert int(np.float64(first)) != int(first)
        b.add(f"first row {first}", oracle.scan(ck.SCAN_AVGS, x), lambda r, x=x: r.scan(ck.SCAN_AVGS, x))
        assert oracle.scan(ck.SCAN_AVGS, x)[1] == (int(np.float64(first)) + int(x[1])) / 2.0
    b.check(ref_answers, f"x/first/{ex.nm(dt)}")


# ---- avg / avgs where the 128-bit sum has to be rounded ---------------------------------------------------------------------------------
AVG_PROBES = [(dt, e, odd, neg) for dt in (np.int64, np.uint64) for e in (53, 54, 62, 63, 64, 65, 77, 84) for odd in (False, True)
              for neg in ((False, True) if dt is np.int64 else (False,))]


@pytest.mark.parametrize("dt,e,odd,neg", AVG_PROBES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_avg_rounds_the_128_bit_sum_once(oracle, dt, e, odd, neg):
    """running sums S - 1, S, S + 1 around an exact tie S at the bit a double rounds at, 2^53 <= S < 2^85: avg and avgs are
    float(sum) / float(count), the sum rounded to nearest-even once (python's int -> float is correctly rounded)"""
    x, sums = ex.avg_probe_column(dt, e, odd=odd, negative=neg)
    n = len(x)
    assert ex.exact_sum(x) == sums[2] and ex.exact_sum(x[:n - 2]) == sums[0]
    assert float(sums[0]) != float(sums[2]) or e == 53                       # the three sums straddle a rounding boundary
    running = oracle.scan(ck.SCAN_AVGS, x)
    for j, s in enumerate(sums):
        cnt = n - 2 + j
        want = np.float64(float(s) / float(cnt))
        assert np.float64(oracle.reduce(ck.RED_AVG, x[:cnt])).tobytes() == want.tobytes(), (j, s)
        assert running[cnt - 1].tobytes() == want.tobytes(), (j, s)
        assert oracle.reduce(ck.RED_SUM, x[:cnt]) == s
