"""Inputs at the numeric extremes of every column type, and a model of aqg_ewise that does not come from the oracle.

Three things live here (a plain module: tests import it, pytest collects nothing from it):

  * per-type POOLS: the ends of each type and their neighbours, zero, small values of both signs; for floating types also both
    zeros, +-max, the smallest normal, subnormals (largest, smallest-normal / 4), +-Inf, NaNs of both signs, 0.1, 1e10 and the
    neighbours of 2^24 and 2^53 (where float / double stop holding every integer);
  * COLUMN BUILDERS: a column starts with the pool (unary) or the full product of two pools (binary), goes on with full-range
    random values and has the pool planted again over its last rows and around every multiple of 1024 -- so the first and the
    last 16-byte vector of a kernel, its element-at-a-time tail and the borders between workgroup spans all see special values;
  * model_ewise: `l OP r` from the C++ rules themselves -- integer promotion, the usual arithmetic conversions, arithmetic of
    the compute type (integers in python `int`, wrapped; floats in numpy float32 / float64), the library's defined results where
    C++ traps or is undefined (x / 0 = 0, x % 0 = 0, INT_MIN / -1 wraps to INT_MIN, x % -1 = 0), then the conversion to the
    result type (wrap; sign or zero extension into the 128-bit pair; `!= 0` for bool).  A floating VALUE converted to an integer
    result type is undefined in C++ once out of range: the model rejects that combination.
"""
import itertools

import numpy as np

import checker as ck

INT_DTYPES = [np.dtype(t) for t in (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64)]
FP_DTYPES = [np.dtype(np.float32), np.dtype(np.float64)]
NUM_DTYPES = INT_DTYPES + FP_DTYPES
OPERAND_DTYPES = NUM_DTYPES + [np.dtype(np.bool_)]              # the 11 operand types of aqg_ewise
BIN_DTYPES = [np.dtype(t) for t in (np.int16, np.int32, np.int64, np.uint32, np.float32, np.float64)]   # the reference harness's

ARITH_OPS = (ck.OP_ADD, ck.OP_SUB, ck.OP_MUL, ck.OP_DIV)
INT_ONLY_OPS = (ck.OP_MOD, ck.OP_AND, ck.OP_OR, ck.OP_XOR)
CMP_OPS = (ck.OP_GT, ck.OP_LT, ck.OP_GE, ck.OP_LE, ck.OP_EQ, ck.OP_NE)
ALL_OPS = ARITH_OPS + INT_ONLY_OPS + CMP_OPS
KINDS = ("vv", "vs", "sv")
OP_NAME = {v: k for k, v in ck.OP_NAMES.items()}


def nm(dt):
    return np.dtype(dt).name


def tag(dt):
    return ck.NP2TAG[np.dtype(dt)]


# ---- pools -------------------------------------------------------------------------------------------------------------------
def _neg_nan(dt):
    dt = np.dtype(dt)
    return np.array([0xFFC00000], np.uint32).view(np.float32)[0] if dt.itemsize == 4 else np.array([0xFFF8 << 48], np.uint64).view(np.float64)[0]


def _dedup_bits(a):
    """drop repeated bit patterns, keep the order (0.0 and -0.0, NaN and -NaN stay apart)"""
    bits = a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    _, first = np.unique(bits, return_index=True)
    return a[np.sort(first)]


def pool(dt, nan=True, inf=True):
    """the special values of one type; nan / inf = False leave NaNs / infinities out (columns of order-dependent operations)"""
    dt = np.dtype(dt)
    if dt.kind == "b":
        return np.array([False, True])
    if dt.kind in "iu":
        ii = np.iinfo(dt)
        vals = [ii.min, ii.min + 1, ii.max, ii.max - 1, 0, 1, 2, 3, 7]
        if dt.kind == "i":
            vals += [-1, -2, -3]
        return _dedup_bits(np.array(vals, dtype=dt))
    fi = np.finfo(dt)
    tiny = dt.type(fi.tiny)                                          # smallest normal
    sub_hi = np.nextafter(tiny, dt.type(0))                          # largest subnormal
    vals = [0.0, -0.0, 1, -1, 2, -2, 3, -3, 7, fi.max, -fi.max, tiny, -tiny, tiny / dt.type(4), sub_hi, -sub_hi, 0.1, 1e10,
            16777215, 16777216, 16777217, 16777218, 2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2, np.nextafter(fi.max, dt.type(0))]
    if inf:
        vals += [np.inf, -np.inf]
    with np.errstate(all="ignore"):
        a = np.array(vals, dtype=dt)
    if nan:
        a = np.concatenate([a, np.array([np.nan], dt), np.array([_neg_nan(dt)], dt)])
    return _dedup_bits(a)


def scalars(dt):
    """the scalar operands of the vs / sv kinds: zero, -1 (the largest value of an unsigned type), the type's minimum, its
    maximum, two ordinary values; NaN, an infinity, -0.0 and a subnormal for floating types"""
    dt = np.dtype(dt)
    if dt.kind == "b":
        return [np.bool_(False), np.bool_(True)]
    if dt.kind in "iu":
        ii = np.iinfo(dt)
        return [dt.type(v) for v in dict.fromkeys([0, -1 if dt.kind == "i" else ii.max, ii.min, ii.max, 1, 7])]
    fi = np.finfo(dt)
    return [dt.type(v) for v in (0.0, -1.0, -fi.max, fi.max, 7.0, np.nan, -np.inf, -0.0, fi.tiny / 4)]


def full_range(rng, dt, n):
    """n values drawn from every bit pattern of an integer type; floating types: every finite bit pattern (any exponent, both
    signs, subnormals), NaNs and infinities replaced by ordinary values"""
    dt = np.dtype(dt)
    if dt.kind == "b":
        return rng.integers(0, 2, n).astype(np.bool_)
    raw = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize])
    a = raw.view(dt).copy()
    if dt.kind == "f":
        bad = ~np.isfinite(a)
        a[bad] = rng.uniform(-1000, 1000, int(bad.sum())).astype(dt)
    return a


def _plant(col, special):
    """`special` again over the last 40 rows and around every multiple of 1024 (rows the first copy does not already hold)"""
    n, m = len(col), len(special)
    if n == 0 or m == 0:
        return col
    for k, i in enumerate(range(max(0, n - 40), n)):
        col[i] = special[k % m]
    for b in range(1024, n, 1024):
        for k, i in enumerate(range(max(0, b - 4), min(n, b + 4))):
            col[i] = special[(b // 1024 * 8 + k) % m]
    return col


def unary_column(dt, n, seed, nan=True, inf=True):
    """pool, then full-range random values, the pool planted again (see _plant); exactly n rows"""
    rng = np.random.default_rng(seed)
    p = pool(dt, nan=nan, inf=inf)
    col = np.concatenate([p, full_range(rng, dt, max(0, n - len(p)))])[:n].copy()
    return _plant(col, p[rng.permutation(len(p))])


def binary_columns(lt, rt, n, seed):
    """two columns of n rows: the full product of the two pools first (as far as n reaches), full-range random pairs after
    it, pool pairs planted again over the last rows and around every multiple of 1024"""
    rng = np.random.default_rng(seed)
    pl, pr = pool(lt), pool(rt)
    L, R = np.repeat(pl, len(pr)), np.tile(pr, len(pl))
    if n < len(L):                                    # a short column takes a random sample of the product, not its first rows
        pick = rng.permutation(len(L))[:n]
        L, R = L[pick], R[pick]
    l = np.concatenate([L, full_range(rng, lt, max(0, n - len(L)))])[:n].copy()
    r = np.concatenate([R, full_range(rng, rt, max(0, n - len(R)))])[:n].copy()
    pick = rng.permutation(len(pl) * len(pr))
    return _plant(l, np.repeat(pl, len(pr))[pick]), _plant(r, np.tile(pr, len(pl))[pick])


def product_columns(lt, rt):
    """exactly the full product of the two pools"""
    pl, pr = pool(lt), pool(rt)
    return np.repeat(pl, len(pr)), np.tile(pr, len(pl))


# ---- the C++ rules --------------------------------------------------------------------------------------------------------------
# a compute type is (kind, bits): kind "i" signed / "u" unsigned / "f" floating
def _promoted(dt):
    """integer promotion [conv.prom]: bool and every integer type narrower than int become int"""
    dt = np.dtype(dt)
    if dt.kind == "f":
        return ("f", dt.itemsize * 8)
    if dt.kind == "b" or dt.itemsize < 4:
        return ("i", 32)
    return (dt.kind, dt.itemsize * 8)


def compute_type(lt, rt):
    """usual arithmetic conversions [expr.arith.conv] of the promoted operand types"""
    a, b = _promoted(lt), _promoted(rt)
    if a[0] == "f" or b[0] == "f":
        return ("f", max(x[1] for x in (a, b) if x[0] == "f"))
    if a[0] == b[0]:
        return (a[0], max(a[1], b[1]))
    u, s = (a, b) if a[0] == "u" else (b, a)
    if u[1] >= s[1]:                                   # the unsigned type's rank is not lower: unsigned wins
        return u
    return s                                           # the signed type holds every value of the narrower unsigned one


def _wrap(v, kind, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if kind == "i" and v >> (bits - 1) else v


def _int_op(op, kind, bits):
    """python-int function of two values of the compute type (kind, bits) -> value of the expression's C++ type"""
    def tdiv(a, b):                                    # C++ division truncates towards zero
        q = abs(a) // abs(b)
        return -q if (a < 0) != (b < 0) else q

    def f(a, b):
        if op == ck.OP_ADD: return _wrap(a + b, kind, bits)
        if op == ck.OP_SUB: return _wrap(a - b, kind, bits)
        if op == ck.OP_MUL: return _wrap(a * b, kind, bits)
        if op == ck.OP_DIV:
            if b == 0: return 0                                          # defined result: the C++ expression traps
            return _wrap(tdiv(a, b), kind, bits)                         # INT_MIN / -1 = 2^(bits-1) wraps back to INT_MIN
        if op == ck.OP_MOD:
            if b == 0: return 0                                          # defined result
            if kind == "i" and b == -1: return 0                         # defined result (INT_MIN % -1 traps; x % -1 is 0 anyway)
            return a - tdiv(a, b) * b
        if op == ck.OP_AND: return _wrap(a & b, kind, bits)
        if op == ck.OP_OR: return _wrap(a | b, kind, bits)
        if op == ck.OP_XOR: return _wrap(a ^ b, kind, bits)
        if op == ck.OP_GT: return int(a > b)
        if op == ck.OP_LT: return int(a < b)
        if op == ck.OP_GE: return int(a >= b)
        if op == ck.OP_LE: return int(a <= b)
        if op == ck.OP_EQ: return int(a == b)
        if op == ck.OP_NE: return int(a != b)
        raise ValueError(op)
    return f


_NPINT = {("i", 32): np.int32, ("u", 32): np.uint32, ("i", 64): np.int64, ("u", 64): np.uint64}
_NPFP = {32: np.float32, 64: np.float64}


def _as_py_ints(x, kind, bits):
    """integer / bool operand -> object array of python ints converted to the integer compute type (value-preserving or modular)"""
    a = np.atleast_1d(np.asarray(x))
    return np.array([_wrap(int(v), kind, bits) for v in a.tolist()], dtype=object)


def _out_dtype(ot):
    return ck.TAG2NP[ot]


def model_ewise(op, l, r, kind, ot):
    """`l OP r` element by element; kind "vv": two columns, "vs": r is a scalar, "sv": l is a scalar; `ot`: dtype tag of the result.
    Returns an array of the result's element type (128-bit results as the (lo, hi) structured types of checker.py)."""
    la, ra = np.atleast_1d(np.asarray(l)), np.atleast_1d(np.asarray(r))
    n = len(la) if kind != "sv" else len(ra)
    ckind, bits = compute_type(la.dtype, ra.dtype)
    is_cmp = op in CMP_OPS
    if ckind == "f":
        if op in INT_ONLY_OPS:
            raise ValueError("% & | ^ have no floating form")
        if ot in (ck.INT128, ck.UINT128):
            raise ValueError("no 128-bit result from floating operands")
        F = _NPFP[bits]
        with np.errstate(all="ignore"):
            a, b = np.broadcast_to(la.astype(F), n), np.broadcast_to(ra.astype(F), n)      # int -> float: one rounding, as in C++
            if op == ck.OP_ADD: v = a + b
            elif op == ck.OP_SUB: v = a - b
            elif op == ck.OP_MUL: v = a * b
            elif op == ck.OP_DIV: v = a / b
            elif op == ck.OP_GT: v = a > b
            elif op == ck.OP_LT: v = a < b
            elif op == ck.OP_GE: v = a >= b
            elif op == ck.OP_LE: v = a <= b
            elif op == ck.OP_EQ: v = a == b
            else: v = a != b
            if is_cmp:
                v = v.astype(np.int32)                                              # the comparison's value: int 0 / 1
            elif ot not in (ck.FLOAT, ck.DOUBLE, ck.BOOL):
                raise ValueError("floating value to an integer result type: undefined in C++ when out of range")
            assert is_cmp or v.dtype == F
            if ot == ck.BOOL:
                return (v != 0).astype(np.uint8)
            return v.astype(_out_dtype(ot))
    # integer compute type
    a, b = _as_py_ints(la, ckind, bits), _as_py_ints(ra, ckind, bits)
    if len(a) != n: a = np.repeat(a, n)
    if len(b) != n: b = np.repeat(b, n)
    v = np.frompyfunc(_int_op(op, ckind, bits), 2, 1)(a, b) if n else np.array([], dtype=object)
    vk, vb = (("i", 32) if is_cmp else (ckind, bits))                              # C++ type of the expression's value
    vals = v.tolist()
    if ot == ck.BOOL:
        return np.array([x != 0 for x in vals], dtype=np.uint8)
    if ot in (ck.INT128, ck.UINT128):                                                # sign extension of a signed value, zero extension of an unsigned one
        out = np.zeros(n, dtype=_out_dtype(ot))
        out["lo"] = np.array([x & 0xFFFFFFFFFFFFFFFF for x in vals], dtype=np.uint64)
        hi = [(x >> 64) & 0xFFFFFFFFFFFFFFFF for x in vals]
        out["hi"] = np.array(hi, dtype=np.uint64).view(out.dtype["hi"])
        return out
    odt = _out_dtype(ot)
    if odt.kind == "f":                                                              # integer -> floating: one rounding from the exact value
        return np.array(vals, dtype=_NPINT[(vk, vb)]).astype(odt)
    return np.array([_wrap(x, odt.kind, odt.itemsize * 8) for x in vals], dtype=odt)  # modular narrowing / value-preserving widening


def defined_in_cxx(op, lt, rt, a, b):
    """whether C++ defines `a OP b` for scalars of types lt, rt (what may be put to a reference built without -fwrapv that traps on
    integer division): no zero divisor, no INT_MIN / -1, no signed overflow in the compute type -- decided in python int"""
    ckind, bits = compute_type(lt, rt)
    if ckind == "f":
        return True
    x, y = _wrap(int(a), ckind, bits), _wrap(int(b), ckind, bits)
    if op in (ck.OP_DIV, ck.OP_MOD):
        if y == 0:
            return False
        return not (ckind == "i" and y == -1 and x == -(1 << (bits - 1)))
    if ckind == "i" and op in (ck.OP_ADD, ck.OP_SUB, ck.OP_MUL):
        exact = x + y if op == ck.OP_ADD else x - y if op == ck.OP_SUB else x * y
        return -(1 << (bits - 1)) <= exact < (1 << (bits - 1))
    return True


def defined_rows(op, l, r, kind):
    """boolean mask over the rows of an ewise question: True where defined_in_cxx"""
    la, ra = np.atleast_1d(np.asarray(l)), np.atleast_1d(np.asarray(r))
    n = len(la) if kind != "sv" else len(ra)
    if compute_type(la.dtype, ra.dtype)[0] == "f" or op not in ARITH_OPS + (ck.OP_MOD,):
        return np.ones(n, dtype=bool)
    lv, rv = la.tolist(), ra.tolist()
    if kind == "vs": rv = rv * n
    if kind == "sv": lv = lv * n
    return np.array([defined_in_cxx(op, la.dtype, ra.dtype, x, y) for x, y in zip(lv, rv)], dtype=bool)


# ---- comparing ----------------------------------------------------------------------------------------------------------------
def canon_nan(a):
    """floating arrays / scalars with every NaN replaced by the one canonical quiet NaN (sign and payload are not part of any contract)"""
    if isinstance(a, int):                            # a 128-bit sum comes back as a python int
        return a
    a = np.array(a, copy=True)
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a


def same(got, want):
    """bit for bit; floating values: bit for bit where finite or infinite, NaN where NaN"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype.itemsize != want.dtype.itemsize or got.shape != want.shape:
        return False
    if want.dtype.kind == "f" and got.dtype.kind == "f":
        return canon_nan(got).tobytes() == canon_nan(want).tobytes()
    return got.tobytes() == want.tobytes()


def first_diff(got, want):
    """index of the first row where `same` fails (for assertion messages)"""
    got, want = canon_nan(np.atleast_1d(got)), canon_nan(np.atleast_1d(want))
    w = got.dtype.itemsize
    g = np.frombuffer(got.tobytes(), np.uint8).reshape(-1, w)
    b = np.frombuffer(want.tobytes(), np.uint8).reshape(-1, w)
    bad = np.nonzero((g != b).any(axis=1))[0]
    return int(bad[0]) if len(bad) else -1


# ---- result types ---------------------------------------------------------------------------------------------------------------
NATURAL_TAG = {("i", 32): ck.INT32, ("u", 32): ck.UINT32, ("i", 64): ck.INT64, ("u", 64): ck.UINT64, ("f", 32): ck.FLOAT, ("f", 64): ck.DOUBLE}
INT_TAGS = [ck.INT8, ck.INT16, ck.INT32, ck.INT64, ck.UINT8, ck.UINT16, ck.UINT32, ck.UINT64]
ALL_OTS = INT_TAGS + [ck.INT128, ck.UINT128, ck.FLOAT, ck.DOUBLE, ck.BOOL]
OT_NAME = {ck.INT8: "int8", ck.INT16: "int16", ck.INT32: "int32", ck.INT64: "int64", ck.UINT8: "uint8", ck.UINT16: "uint16",
           ck.UINT32: "uint32", ck.UINT64: "uint64", ck.INT128: "int128", ck.UINT128: "uint128", ck.FLOAT: "float", ck.DOUBLE: "double",
           ck.BOOL: "bool"}
# one operand pair per compute type on which every result type the call accepts is exercised
OT_SWEEP_PAIRS = {("i", 32): (np.int8, np.uint16), ("u", 32): (np.int32, np.uint32), ("i", 64): (np.uint32, np.int64),
                  ("u", 64): (np.int64, np.uint64), ("f", 32): (np.int64, np.float32), ("f", 64): (np.float32, np.float64)}


def ops_for(lt, rt):
    """the operations aqg_ewise accepts for an operand pair"""
    return ARITH_OPS + CMP_OPS if compute_type(lt, rt)[0] == "f" else ALL_OPS


def accepted_ots(op, lt, rt):
    """every result type the call accepts and C++ defines for (op, pair): no 128-bit result from floating operands; a floating VALUE
    (not a comparison's 0 / 1) goes to floating or bool results only"""
    if compute_type(lt, rt)[0] != "f":
        return list(ALL_OTS)
    if op in CMP_OPS:
        return INT_TAGS + [ck.FLOAT, ck.DOUBLE, ck.BOOL]
    return [ck.FLOAT, ck.DOUBLE, ck.BOOL]


def default_ot(oracle, op, lt, rt):
    """the reference's result type where it has one (ewise_out_dtype); else -- uint64 mixed with another type, bool with a number --
    the expression's own C++ type (bool for comparisons)"""
    t = oracle.ewise_out_dtype(op, tag(lt), tag(rt))
    if t != ck.ERROR and t in ck.TAG2NP:
        return t
    return ck.BOOL if op in CMP_OPS else NATURAL_TAG[compute_type(lt, rt)]


def ewise_cases():
    """(lt, rt, op, kind) over all 11 x 11 operand pairs, every operation the pair accepts and the three kinds"""
    for lt, rt in itertools.product(OPERAND_DTYPES, OPERAND_DTYPES):
        for op in ops_for(lt, rt):
            for kind in KINDS:
                yield lt, rt, op, kind


# ---- truncate ---------------------------------------------------------------------------------------------------------------------
TRUNC_P = (0, 2, 6, 7, 15, 16, 20)


def truncate_column(dt, p):
    """+-max, the values just below and above max / 10^p (where truncate stops rounding), Inf, NaN, subnormals, ordinary values"""
    dt = np.dtype(dt)
    fi = np.finfo(dt)
    edge = dt.type(float(fi.max) / 10.0 ** p)
    with np.errstate(all="ignore"):
        vals = [fi.max, -fi.max, edge, np.nextafter(edge, dt.type(0)), np.nextafter(edge, dt.type(np.inf)), -edge, np.inf, -np.inf, np.nan,
                fi.tiny, fi.tiny / dt.type(4), -fi.tiny / dt.type(4), 0.0, -0.0, 0.5, 1.5, 2.5, -2.5, 0.125, 1234.56789, -0.000123456, 1e10 / 3, 16777217]
        return np.concatenate([np.array(vals, dtype=dt), pool(dt)])


# ---- columns for reductions and scans ----------------------------------------------------------------------------------------------
def one_sign_zeros(x):
    """min / max family: the reference keeps the LAST of two equal values, a parallel fold may keep the other, and 0.0 == -0.0 --
    so a column handed to that family holds zeros of one sign only (-0.0 becomes 0.0); asserted, not assumed"""
    x = x.copy()
    if x.dtype.kind == "f":
        x[(x == 0) & np.signbit(x)] = 0.0
        z = x[x == 0]
        assert not np.signbit(z).any()
    return x


def sum_safe(x):
    """floating column for the sum family: finite rows scaled so that |x| <= max / (2 n) -- no summation order of the finite
    rows overflows; infinities stay"""
    if x.dtype.kind != "f":
        return x
    x = x.copy()
    lim = np.finfo(x.dtype).max / (2 * max(len(x), 1))
    fin = np.isfinite(x)
    big = fin & (np.abs(x) > lim)
    with np.errstate(all="ignore"):
        x[big] = np.ldexp(np.frexp(x[big])[0], int(np.floor(np.log2(lim))) - 1).astype(x.dtype)
    assert np.all(np.abs(x[fin]) <= lim)
    return x


def square_safe(x):
    """full-exponent floating column scaled so that the squares, their sum AND the square of the sum (s * s <= n * ssq) stay finite in the
    column's type: |x| <= sqrt(max / 2) / n"""
    x = x.copy()
    lim = np.sqrt(float(np.finfo(x.dtype).max) / 2) / max(len(x), 1)
    big = np.abs(x) > lim
    x[big] = (np.sign(x[big]) * np.ldexp(np.frexp(x[big])[0], int(np.floor(np.log2(lim))))).astype(x.dtype)
    assert np.all(np.abs(x) <= lim)
    return x


def exact_sum(x):
    return sum(int(v) for v in x.tolist())


def unrepresentable_first_rows(dt):
    """8-byte integers a double cannot hold: the reference's `avgs` starts its running sum from the first row rounded to double
    (`s = ret[0] = arr[0]`, aggregations.h:224), so these first rows shift every later mean's sum by up to 2^10"""
    dt = np.dtype(dt)
    ii = np.iinfo(dt)
    vals = [ii.max, ii.max - 1, 2**53 + 1, 2**62 + 1, 2**63 - 513]
    if dt.kind == "i":
        vals += [ii.min + 1, -(2**53 + 1), -(2**62 + 3)]
    else:
        vals += [2**63 + 1, 2**64 - 1025]
    return [dt.type(v) for v in vals]


def avg_probe_column(dt, e, odd=False, negative=False):
    """int64 / uint64 column whose running sums reach S - 1, S and S + 1 over its last three rows, S = 2^e + 2^(e-53) (odd: 2^e + 3 * 2^(e-53)):
    S is an exact tie at the bit a double rounds at, its neighbours lie just below and just above it.  The first row is 0: the
    reference's `avgs` starts its sum from the first element ROUNDED to double (`s = ret[0] = arr[0]`), which is exact for 0.
    Returns (column, [S-1, S, S+1])."""
    dt = np.dtype(dt)
    big = int(np.iinfo(dt).max)
    S = (1 << e) + (3 if odd else 1) * (1 << (e - 53))
    q, rem = divmod(S - 1, big)
    x = np.array([0] + [big] * q + [rem, 1, 1], dtype=dt)
    sums = [S - 1, S, S + 1]
    if negative:
        assert dt.kind == "i"
        x, sums = -x, [-s for s in sums]
    return x, sums
