"""Named cases of the window join (aqg_join_window*, aqg_interval_fold), each the smallest shape at which its mistake shows, shared by
the model's tests (tests/test_wj_model.py) and the device's (tests/test_gpu_wj.py).

A join case is Case(bk, bo, pk, po, before, after, x, flags): key columns in the (tag, data) format of tests/join_keys_model.py, the
`on` columns as numpy arrays of one dtype, the two spans, a value column x over the build rows, and the flag combinations the spans
are valid under (a span of 0 needs a closed side).  A fold case is Fold(x, lo, hi): m intervals over a column, for aqg_interval_fold
alone.  The route bits a call must report are derived from the shapes by wj_model.routes / wj_model.fold_route."""
from collections import namedtuple

import numpy as np

import asof_cases
import checker as ck
from wj_model import OPEN_HI, OPEN_LO, PREVAILING

Case = namedtuple("Case", "bk bo pk po before after x flags")
Fold = namedtuple("Fold", "x lo hi")
ALL_FLAGS = tuple(range(8))
CLOSED_ONLY = (0, PREVAILING)
_CASES = _FOLDS = None


def _key(a, dtype=np.int32):
    a = np.asarray(a, dtype=dtype)
    return (ck.NP2TAG[a.dtype], a)


def _x(n, seed, dtype=np.int32):
    rng = np.random.default_rng(900 + seed)
    if np.dtype(dtype).kind == "f":
        return (rng.normal(0, 100, n)).astype(dtype)
    return rng.integers(-1000, 1000, n).astype(dtype)


def _from_asof(name, before, after, seed, xdtype=np.int32, flags=ALL_FLAGS):
    bk, bo, pk, po, _ = asof_cases.cases()[name]
    return Case(bk, bo, pk, po, before, after, _x(len(bo), seed, xdtype), flags)


def _d_eq_span(dtype):
    """one symbol beside a decoy; the probe row sits exactly `before` behind one build row and `after` in front of another: the open
    side drops that row, the closed side keeps it.  Floating: distances 0.5 and 0.25, exact in binary"""
    s = 1 if np.dtype(dtype).kind in "iu" else 0.125
    on = np.array([0, 4, 6, 10, 10, 12, 14, 20], np.float64) * s
    bk = np.concatenate([np.zeros(8), np.ones(8)])
    bo = np.concatenate([on, on + s]).astype(dtype)
    po = (np.array([10, 10, 9, 11, 0, 20, 13], np.float64) * s).astype(dtype)
    return Case([_key(bk)], bo, [_key(np.zeros(len(po)))], po, 4 * s, 2 * s, _x(16, 1), ALL_FLAGS)


def _prevailing():
    """group 0 in front of group 1 in the order; probes of group 1 whose window starts at the segment start (no prevailing row: a row
    taken from the neighbour is group 0's last), probes in front of an empty window, and a prevailing row among three ties (the
    highest row id)"""
    bk = np.array([0] * 6 + [1] * 7)
    bo = np.array([0, 10, 20, 30, 40, 50, 5, 10, 10, 10, 20, 30, 40], np.int32)
    pk = np.array([1, 1, 1, 1, 1, 0, 0, 1])
    po = np.array([5, 7, 20, 15, 100, 0, 45, 4], np.int32)
    return Case([_key(bk)], bo, [_key(pk)], po, 5, 1, _x(13, 2), ALL_FLAGS)


def _values_case(kind):
    """two symbols, `on` = 0 .. 199 each, windows of about 20 rows; values: a segment of 1e30s beside a segment of ones / NaN and Inf
    rows among ones / int64 and uint64 values whose window sums carry into the upper 64 bits"""
    rng = np.random.default_rng(31)
    n = 200
    bk = np.repeat([0, 1], n)
    bo = np.tile(np.arange(n), 2).astype(np.int32)
    pk = rng.integers(0, 2, 300)
    po = rng.integers(-5, n + 5, 300).astype(np.int32)
    if kind == "1e30":
        x = np.concatenate([np.full(n, 1e30), np.ones(n)])
    elif kind == "nonfinite":
        x = rng.normal(0, 1, 2 * n)
        x[[7, 130, 390]] = np.nan
        x[[40, 250]] = np.inf
        x[[41, 300]] = -np.inf
    elif kind == "i64":
        x = np.concatenate([np.full(n, np.iinfo(np.int64).max - 3), np.full(n, np.iinfo(np.int64).min + 5)]).astype(np.int64)
    else:
        x = np.full(2 * n, np.iinfo(np.uint64).max - 1, np.uint64)
    sh = rng.permutation(2 * n)
    return Case([_key(bk[sh])], bo[sh], [_key(pk)], po, 12, 7, x[sh], ALL_FLAGS)


def _level3(before):
    """one presorted keyless build side of 262144 + 130 rows (a tree with three levels above the rows); windows (closed behind, after
    = 0) that end on, one before and one after 64, 4096 and 262144, and start at row 0 (before = 300000) or 70 rows earlier"""
    n = 262144 + 130
    bo = np.arange(n, dtype=np.int64)
    po = np.array([0, 1, 62, 63, 64, 65, 4094, 4095, 4096, 4097, 262142, 262143, 262144, 262145, n - 1], np.int64)
    return Case([], bo, [], po, before, 0, _x(n, 3), (0, OPEN_LO, OPEN_LO | PREVAILING))


def cases():
    global _CASES
    if _CASES is None:
        big = 2.0 ** 64
        c = {"group_sizes": _from_asof("group_sizes", 15, 10, 10), "group_sizes_f64x": _from_asof("group_sizes", 25, 0.5, 11, np.float64),
             "straddle": _from_asof("straddle", 4, 4, 12), "all_ties": _from_asof("all_ties", 1, 1, 13),
             "zero_spans": _from_asof("group_sizes", 0, 0, 14, flags=CLOSED_ONLY), "zero_spans_ties": _from_asof("all_ties", 0, 0, 15, flags=CLOSED_ONLY),
             "inf_spans": _from_asof("straddle", np.inf, np.inf, 16), "inf_spans_f64": _from_asof("ends_float64", np.inf, np.inf, 17),
             "inf_before_nan_tail": _from_asof("build_nan_last", 3, np.inf, 18, np.float32),
             "ends_int8": _from_asof("ends_int8", 255, 127, 19, np.int8), "ends_int8_sat": _from_asof("ends_int8", 1e30, big, 20),
             "ends_int64": _from_asof("ends_int64", 2.0 ** 63, 1, 21, np.int64), "ends_int64_sat": _from_asof("ends_int64", big, 1e300, 22),
             "ends_uint64": _from_asof("ends_uint64", 2.0 ** 63, 2, 23, np.uint64), "ends_uint64_sat": _from_asof("ends_uint64", np.inf, big, 24),
             "ends_uint8": _from_asof("ends_uint8", 128, 1.5, 25, np.uint8),
             "ends_float64": _from_asof("ends_float64", 1.0, 2.0, 26, np.float64), "ends_float32": _from_asof("ends_float32", 1.0, 1e38, 27, np.float32),
             "d_eq_span_i32": _d_eq_span(np.int32), "d_eq_span_f64": _d_eq_span(np.float64), "d_eq_span_f32": _d_eq_span(np.float32),
             "d_eq_span_u16": _d_eq_span(np.uint16),
             "prevailing": _prevailing(),
             "absent_keys": _from_asof("absent_keys", 6, 2, 28, np.int16), "nan_keys": _from_asof("tuple3_wide_f64", 9, 4, 29, np.uint16),
             "tuple2_packed": _from_asof("tuple2_packed", 5, 5, 30), "tuple2_wide": _from_asof("tuple2_wide", 3, 8, 31, np.uint32),
             "nokeys": _from_asof("nokeys", 1.25, 0.5, 32, np.float64), "nokeys_presorted": _from_asof("nokeys_presorted", 2.0, 1.0, 33, np.float32),
             "build_sorted": _from_asof("build_sorted", 4, 2, 34), "build_swapped": _from_asof("build_swapped", 4, 2, 35),
             "build_nan_middle": _from_asof("build_nan_middle", 4, 2, 36), "build_nan_last": _from_asof("build_nan_last", 4, 2, 37),
             "lds_i64": _from_asof("lds_i64", 7, 3, 38), "lds_i32": _from_asof("lds_i32", 7, 3, 39, np.float64),
             "hbm_big": _from_asof("hbm_big", 2.0 ** 33, 2.0 ** 31, 40),
             "values_1e30": _values_case("1e30"), "values_nonfinite": _values_case("nonfinite"), "values_i64_carry": _values_case("i64"),
             "values_u64_carry": _values_case("u64"), "level3_nokeys": _level3(300000), "level3_nokeys_short": _level3(70)}
        for n in (1, 2, 3, 5):
            c["np_%d" % n] = _from_asof("np_%d" % n, 20, 9, 41 + n)
        _CASES = c
    return _CASES


# ---- the fold alone ------------------------------------------------------------------------------------------------------------------
def _edges(n, dtype, seed):
    """intervals with their ends on, one before and one after 64, 4096 and 262144; both ends in one block, in adjacent blocks,
    block-aligned; one row; the whole column; lo > hi; hi > n"""
    x = _x(n, seed, dtype)
    marks = [m for m in (64, 4096, 262144) if m + 1 < n]
    pts = sorted({0, 1, n - 1, n} | {m + d for m in marks for d in (-1, 0, 1)})
    lo, hi = [], []
    for a in pts:
        for b in pts:
            lo.append(a); hi.append(b)                            # (a >= b: empty)
    extra = [(5, 9), (64, 128), (63, 65), (128, 192), (100, 101), (0, n), (70, 3), (n - 3, n + 1000), (0, 0xFFFFFFFF), (n, n + 5),
             (4096, 8192), (4095, 8193), (1, n - 1)]
    lo += [a for a, _ in extra]; hi += [b for _, b in extra]
    return Fold(x, np.array(lo, np.uint32), np.array(hi, np.uint32))


def _random_fold(n, m, dtype, seed, x=None):
    rng = np.random.default_rng(700 + seed)
    a, b = rng.integers(0, n + 1, m), rng.integers(0, n + 1, m)
    short = rng.random(m) < 0.5
    b = np.where(short, np.minimum(a + rng.integers(0, 200, m), n), b)
    return Fold(_x(n, seed, dtype) if x is None else x, a.astype(np.uint32), b.astype(np.uint32))


def folds():
    """name -> Fold.  STAGED needs the column with its level 1 under 48 KB and at least 2^16 queries"""
    global _FOLDS
    if _FOLDS is None:
        rng = np.random.default_rng(77)
        m16 = (1 << 16) + 5
        xf = rng.normal(0, 1, 3000)
        xf[1000:2000] = 1e30
        xn = rng.normal(0, 1, 3000)
        xn[[5, 64, 1999]] = np.nan
        xn[[700, 2500]] = np.inf
        xn[701] = -np.inf
        _FOLDS = {"edges_level3_i32": _edges(262144 + 130, np.int32, 1), "edges_level2_f64": _edges(4096 * 2 + 130, np.float64, 2),
                  "edges_level1_i8": _edges(64 * 3 + 5, np.int8, 3), "one_row": Fold(np.array([7], np.int64), np.array([0, 0, 1], np.uint32), np.array([1, 0, 1], np.uint32)),
                  "staged_i32": _random_fold(5000, m16, np.int32, 4), "staged_f64": _random_fold(4000, m16, np.float64, 5),
                  "staged_i64_carry": _random_fold(2500, m16, np.int64, 6, np.full(2500, np.iinfo(np.int64).max, np.int64)),
                  "inplace_wide_column": _random_fold(20000, m16, np.int32, 7), "inplace_few_queries": _random_fold(5000, 1000, np.int32, 8),
                  "inplace_u64_carry": _random_fold(9000, 500, np.uint64, 9, np.full(9000, np.iinfo(np.uint64).max, np.uint64)),
                  "values_1e30": _random_fold(3000, 2000, np.float64, 10, xf), "values_nonfinite": _random_fold(3000, 2000, np.float64, 11, xn),
                  "staged_1e30": _random_fold(3000, m16, np.float64, 12, xf), "f32": _random_fold(7000, 3000, np.float32, 13)}
    return _FOLDS


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------------
def random_case(seed, max_n):
    """(Case, flags): random sides of tests/asof_cases.random_sides with spans from the `on` domain (integral, half-integral, 0, +Inf)"""
    bk, bo, pk, po, _, _ = asof_cases.random_sides(seed, max_n)
    rng = np.random.default_rng(5000 + seed)
    flags = int(rng.integers(0, 8))
    pick = lambda: float(rng.choice([0.0, 0.5, 1.0, 2.0, 3.5, 7.0, np.inf]))
    before, after = pick(), pick()
    if before == 0.0:
        flags &= ~OPEN_LO
    if after == 0.0:
        flags &= ~OPEN_HI
    xdt = (np.int32, np.float64, np.int64, np.uint8, np.float32)[seed % 5]
    return Case(bk, bo, pk, po, before, after, _x(len(bo), seed, xdt), (flags,)), flags
