"""Inputs and the `check` routine of tests/test_gpu_groupagg_extremes.py: the group-by aggregates at the numeric extremes, plan by plan.

A plain module (pytest collects nothing from it).  The pytest file calls `run_plan` in-process for the plans the default switches
reach, and inside a child process (test_gpu_plans.run_forced: the switches are read once per process) for the plans behind a switch.

GROUP SHAPES -- every case, through its key column: one group that holds a third of the rows (same-address atomics, the
wavefront-level combining), 60 groups of exactly one row, a few groups of an exact size reserved for planted values, the rest random.
The layout is made of group LABELS; a plan's key columns are an injective map of the labels, so every plan at one shape groups the rows
the same way and the oracle's `reversemap` tells which rows form a group.

VALUE SETS -- all from the pools and builders of tests/extremes.py:
  int_full       ex.unary_column: full-range values of the eight integer types with the ends of the type planted
  carry          int64 / uint64 columns whose per-group low word carries or borrows on most rows, and nine groups made of
                 ex.avg_probe_column: their 128-bit sums lie on, just below and just above a rounding tie of `avg` (e = 53, 64, 77)
  narrow_at_end  int32 / uint32 values in [max - 4, max], [min, min + 4], and a column that is narrow but for min, max and 0xFFFFFFFF
                 in three of its last ten rows (the packed value fields and their late-row escape)
  fp_finite      every finite exponent, both signs, subnormals, zeros of one sign; scaled so that no order of summation overflows
                 (ex.sum_safe; ex.square_safe for var / stddev)
  fp_inf         fp_finite with +Inf rows in 5 % of the groups, infinities of both signs in 2 %, a multi-row and a one-row group of
                 all +Inf, the same of all -Inf, and of strictly negative finite values (the seeds of min and max)
  fp_nan         fp_inf with NaNs of both signs in some rows of at most 10 % of the groups -- chosen by GROUP; the dominant group is among
                 them in one column and not in the other

WHAT IS COMPARED (check): group count, first rows, key columns, counts -- always, every group.  The plan read back.  Integer results
bit for bit (128-bit sums included).  Floating min / max bit for bit, floating sum / avg / var / stddev inside the bounds below, for
every group without a NaN row: DESIGN.md section 2 -- "a NaN voids only what is behind it", and in a group that is everything the
group holds.  At least 90 % of the groups are compared in every call (asserted here, and on the input by the builders).

  sum     equal where the oracle's value is infinite, NaN where it is NaN (Inf - Inf), else |got - want| <= 2 n_g 2^-53 sum|x_g| over
          the group's finite rows plus one ulp of the result: include/aqg.h's (n_g - 1) 2^-53 sum|x| from the exact sum, for both sides
  avg     that bound over n_g
  var     |got - want| <= 4 n_g 2^-52 sum x_g^2 / (n_g + 1) (derived in test_gpu_extremes.py::test_reduce_var_stddev_floating: both sides
          round the same squares and differ by the order of two sums); stddev: that over sqrt(var - bound), or -- a variance within its
          own error of zero -- either side may take the root of a negative number.  A non-finite variance: the same infinity, or a NaN
"""
import numpy as np

import checker as ck
import extremes as ex
from aquery2_amd import capi

ONES = 60                      # groups of exactly one row
FP_SIZED = (7, 7, 7)           # reserved multi-row groups of the floating sets: all +Inf, all -Inf, strictly negative
PROBE_E = (53, 64, 77)
I64, U64 = np.dtype(np.int64), np.dtype(np.uint64)
I32, U32 = np.dtype(np.int32), np.dtype(np.uint32)
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
NARROW4 = [I32, U32, F32]
TINY_AND_WIDE = [np.dtype(t) for t in (np.int8, np.uint8, np.int16, np.uint16, np.int64, np.uint64, np.float64)]
ALL_DT = ex.INT_DTYPES + ex.FP_DTYPES
SUM, MIN, MAX, COUNT, AVG, VAR, STDDEV = ck.RED_SUM, ck.RED_MIN, ck.RED_MAX, ck.RED_COUNT, ck.RED_AVG, ck.RED_VAR, ck.RED_STDDEV
RED_NAME = {v: k for k, v in ck.RED_NAMES.items()}


# ---- group shapes --------------------------------------------------------------------------------------------------------------
def probe_sizes(dt, es=PROBE_E):
    """the sizes of the groups that hold ex.avg_probe_column(dt, e)'s rows up to the sums S - 1, S and S + 1: three groups for every e"""
    return [len(ex.avg_probe_column(dt, e)[0]) - 2 + j for e in es for j in range(3)]


class Layout:
    """labels[i]: the group of row i.  Label 0 holds rows [n // 7, n // 7 + n // 3); labels 1 .. ones are one row each; the next
    len(sized) labels have exactly the sizes asked for; the rest of the rows draw from the remaining labels up to G.  `big`: the size
    of group 0 where a plan refuses a third of the rows by design"""

    def __init__(self, n, G, seed, sized=FP_SIZED, ones=ONES, big=None):
        rng = np.random.default_rng(seed)
        lo, big = n // 7, n // 3 if big is None else big
        self.big = big
        rest = rng.permutation(np.concatenate([np.arange(0, lo), np.arange(lo + big, n)]))
        assert ones + sum(sized) < len(rest)
        self.n, self.labels = n, np.zeros(n, np.int64)
        self.ones_rows = rest[:ones]
        self.labels[self.ones_rows] = 1 + np.arange(ones)
        pos, self.sized_rows = ones, []
        for k, sz in enumerate(sized):
            rows = np.sort(rest[pos:pos + sz])
            self.labels[rows] = 1 + ones + k
            self.sized_rows.append(rows)
            pos += sz
        self.first_free = 1 + ones + len(sized)
        self.G = max(G, self.first_free + 1)
        self.labels[rest[pos:]] = rng.integers(self.first_free, self.G, len(rest) - pos)
        self.probe_es = ()
        self._memo = {}
        assert np.count_nonzero(self.labels == 0) == big and all(np.count_nonzero(self.labels == 1 + k) == 1 for k in range(ones))

    def first_flags(self):
        """True at the first row of every group"""
        if "first" in self._memo:
            return self._memo["first"]
        order = np.argsort(self.labels, kind="stable")
        sl = self.labels[order]
        f = np.zeros(self.n, bool)
        f[order[np.concatenate([[True], sl[1:] != sl[:-1]])]] = True
        self._memo["first"] = f
        return f

    def rows_of(self, groups):
        """True at the rows of the given groups"""
        m = np.zeros(self.G, bool)
        m[groups] = True
        return m[self.labels]

    def memo(self, key, make):
        """a column built once per layout (the floating sets build on one another); callers copy before they write"""
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]


# ---- value sets ----------------------------------------------------------------------------------------------------------------
def int_full(dt, lay, seed):
    return ex.unary_column(dt, lay.n, seed)


def carry(dt, lay, seed):
    """uint64: every row all ones; int64: INT64_MIN, -1, INT64_MAX, 1 in turn -- the low word of a group's sum carries or borrows on most
    rows.  A layout whose reserved groups have probe_sizes(dt) gets the avg probes planted into them."""
    dt = np.dtype(dt)
    n = lay.n
    if dt == U64:
        x = np.full(n, np.iinfo(np.uint64).max, dtype=dt)
    else:
        x = np.array([np.iinfo(np.int64).min, -1, np.iinfo(np.int64).max, 1], dtype=dt)[np.arange(n) % 4]
    if lay.probe_es:
        assert [len(r) for r in lay.sized_rows] == probe_sizes(dt, lay.probe_es)
        k = 0
        for e in lay.probe_es:
            col, _ = ex.avg_probe_column(dt, e)
            for j in range(3):
                rows = lay.sized_rows[k]
                x[rows] = col[:len(rows)]
                k += 1
    return x


def narrow_at_end(dt, lay, seed, which):
    dt = np.dtype(dt)
    ii, n = np.iinfo(dt), lay.n
    rng = np.random.default_rng(seed)
    if which == "hi":
        return rng.integers(ii.max - 4, ii.max, n, endpoint=True).astype(dt)
    if which == "lo":
        return rng.integers(ii.min, ii.min + 4, n, endpoint=True).astype(dt)
    assert which == "late"
    x = rng.integers(1, 6, n).astype(dt)                        # narrow over the first 2^20 rows (and all the others but three)
    x[n - 9], x[n - 5] = ii.min, ii.max
    x[n - 2] = np.array([0xFFFFFFFF], np.uint32).view(dt)[0]
    return x


def fp_finite(dt, lay, seed, safe="sum"):
    dt = np.dtype(dt)
    base = lay.memo(("base", dt, seed), lambda: ex.one_sign_zeros(ex.unary_column(dt, lay.n, seed, nan=False, inf=False)))
    x = ex.sum_safe(base) if safe == "sum" else ex.square_safe(base)
    assert np.isfinite(x).all()
    return x


def fp_inf(dt, lay, seed, safe="sum"):
    dt = np.dtype(dt)
    return lay.memo(("inf", dt, seed, safe), lambda: _fp_inf(dt, lay, seed, safe)).copy()


def _fp_inf(dt, lay, seed, safe):
    x = fp_finite(dt, lay, seed, safe)
    rng = np.random.default_rng(seed + 1)
    free = rng.permutation(np.arange(lay.first_free, lay.G))
    a, b = free[: max(1, len(free) // 20)], free[max(1, len(free) // 20): max(1, len(free) // 20) + max(1, len(free) // 50)]
    in_a, in_b = lay.rows_of(a), lay.rows_of(b)
    first, coin = lay.first_flags(), rng.random(lay.n) < 0.5
    x[in_a & (first | coin)] = np.inf
    x[in_b & first] = np.inf
    x[in_b & ~first & coin] = -np.inf                          # (a group of b with one row only is a +Inf group)
    if len(lay.sized_rows) >= 3 and len(lay.ones_rows) >= 3:
        tiny = dt.type(np.finfo(dt).tiny)
        x[lay.sized_rows[0]], x[lay.ones_rows[0]] = np.inf, np.inf
        x[lay.sized_rows[1]], x[lay.ones_rows[1]] = -np.inf, -np.inf
        for rows in (lay.sized_rows[2], lay.ones_rows[2:3]):
            x[rows] = -np.abs(x[rows]) - tiny
            assert np.all(x[rows] < 0) and np.isfinite(x[rows]).all()
    return x


def fp_nan(dt, lay, seed, dominant, safe="sum"):
    """fp_inf with NaNs of both signs in about a third of the rows of 8 % of the groups (the dominant group among them or not)"""
    dt = np.dtype(dt)
    x = fp_inf(dt, lay, seed, safe)
    rng = np.random.default_rng(seed + 2)
    present = np.unique(lay.labels)
    free = present[present >= lay.first_free]
    chosen = rng.permutation(free)[: max(1, int(len(present) * 0.08))]
    if dominant:
        chosen = np.concatenate([chosen[:-1], [0]])
    assert len(chosen) <= 0.1 * len(present), "the input recipe keeps 90 % of the groups free of NaN"
    hit = lay.rows_of(chosen) & (lay.first_flags() | (rng.random(lay.n) < 0.3))
    rows = np.nonzero(hit)[0]
    x[rows[0::2]] = np.nan
    x[rows[1::2]] = ex._neg_nan(dt)
    return x


# ---- the comparison ------------------------------------------------------------------------------------------------------------
def acc_count(op, dt):
    """accumulators one aggregate takes (groupby.hip aqg_make_plan): 8-byte integer sums take two"""
    wide = np.dtype(dt) in (I64, U64)
    if op in (MIN, MAX):
        return 1
    if op == COUNT:
        return 0
    return (2 if wide else 1) * (2 if op in (VAR, STDDEV) else 1)


def pack_calls(ops, dt, max_acc, count_ok=True):
    """`ops` over one column cut into calls of at most max_acc accumulators (count_ok False: the ops that need the group sizes are left
    out -- the LDS budget of that shape has no room for them)"""
    calls, cur, used = [], [], 0
    for op in ops:
        if not count_ok and op in (COUNT, AVG, VAR, STDDEV):
            continue
        a = acc_count(op, dt)
        if a > max_acc:
            continue
        if used + a > max_acc or len(cur) == 8:
            calls.append(cur)
            cur, used = [], 0
        cur.append(op)
        used += a
    return calls + ([cur] if cur else [])


def group_stats(x, o):
    """per group of the oracle's numbering: rows, whether a row is NaN, sum |x| and sum x^2 over the finite rows (double)"""
    rev, G = o["reversemap"], o["ngroups"]
    with np.errstate(all="ignore"):
        x64 = x.astype(np.float64)
        fin = np.isfinite(x64)
        ax = np.where(fin, np.abs(x64), 0.0)
        return dict(n=o["counts"].astype(np.float64), nan=np.bincount(rev, weights=np.isnan(x64), minlength=G) > 0,
                    sum_abs=np.bincount(rev, weights=ax, minlength=G), sum_sq=np.bincount(rev, weights=ax * ax, minlength=G))


def _fail(what, op, bad, got, want, extra=""):
    g = int(np.nonzero(bad)[0][0])
    raise AssertionError(f"{what}: {RED_NAME[op]}: group {g} (of {int(bad.sum())} wrong): device {got[g]!r}, oracle {want[g]!r} {extra}")


def fp_sum_bound(op, st, want):
    """the bound of a floating SUM / AVG per group (module docstring): 2 n_g 2^-53 sum|x_g| (over n_g for AVG) plus one ulp of the result"""
    ng = st["n"]
    bound = 2 * ng * 2.0 ** -53 * st["sum_abs"]
    if op == AVG:
        bound = bound / ng
    return bound + np.spacing(np.abs(np.where(np.isfinite(want), want, 0.0)))


def fp_sum_ratio(op, got, want, st):
    """largest |got - want| / fp_sum_bound over the groups compare() holds to that bound (no NaN row, a finite oracle value): what a test reports"""
    with np.errstate(all="ignore"):
        live = ~st["nan"] & np.isfinite(want) & np.isfinite(got)
        r = np.abs(got - want)[live] / fp_sum_bound(op, st, want)[live]
    return float(r.max()) if len(r) else 0.0


def compare(op, x, got, want, o, what, stats=None):
    """one result column against the oracle's (module docstring); returns the share of the groups that were compared"""
    G = o["ngroups"]
    assert got.shape == want.shape == (G,) and got.dtype == want.dtype, (what, got.dtype, want.dtype, got.shape, G)
    if x.dtype.kind != "f" or op == COUNT:
        if not ex.same(got, want):
            i = ex.first_diff(got, want)
            raise AssertionError(f"{what}: {RED_NAME[op]}: group {i}: device {got[i]!r}, oracle {want[i]!r}")
        return 1.0
    st = stats if stats is not None else group_stats(x, o)
    keep = ~st["nan"]
    assert keep.sum() >= 0.9 * G, (what, "groups without a NaN row", int(keep.sum()), G)
    ng = st["n"]
    with np.errstate(all="ignore"):
        if op in (MIN, MAX):
            bad = keep & (got.view(np.uint32 if x.dtype.itemsize == 4 else np.uint64) != want.view(np.uint32 if x.dtype.itemsize == 4 else np.uint64))
            if bad.any():
                _fail(what, op, bad, got, want)
        elif op in (SUM, AVG):
            bound = fp_sum_bound(op, st, want)
            fin, inf, nan = np.isfinite(want), np.isinf(want), np.isnan(want)
            bad = keep & ((fin & ~(np.abs(got - want) <= bound)) | (inf & (got != want)) | (nan & ~np.isnan(got)))
            if bad.any():
                g = int(np.nonzero(bad)[0][0])
                _fail(what, op, bad, got, want, f"bound {bound[g]!r}, rows {int(ng[g])}")
        else:
            bound = 4 * ng * 2.0 ** -52 * st["sum_sq"] / (ng + 1)
            fin, inf, nan = np.isfinite(want), np.isinf(want), np.isnan(want)
            if op == VAR:
                bad = keep & ((fin & ~(np.abs(got - want) <= bound)) | (inf & (got != want)) | (nan & ~np.isnan(got)))
            else:
                var = st["oracle_var"]                       # stddev is judged next to the oracle's variance of the same group
                safe = np.isfinite(var) & (var > bound)
                tol = bound / np.sqrt(np.where(safe, var - bound, 1.0)) + 2.0 ** -52 * np.where(fin, want, 0.0)
                near0 = np.isfinite(var) & ~safe            # a variance within its own error of zero
                ok_safe = np.abs(got - want) <= tol
                ok_near = np.isnan(got) | (np.abs(got - np.where(fin, want, 0.0)) <= np.sqrt(2 * bound))
                ok_rest = np.where(np.isinf(want), got == want, np.isnan(got))          # the variance itself is not finite
                bad = keep & ~np.where(safe, ok_safe, np.where(near0, ok_near, ok_rest))
            if bad.any():
                g = int(np.nonzero(bad)[0][0])
                _fail(what, op, bad, got, want, f"bound (of the variance) {bound[g]!r}, rows {int(ng[g])}")
    return float(keep.sum()) / G


def check(gpu, oracle, keys, ops, vals, hint, want_plan_bits, forbid_bits=0, what="", ogb=None):
    """one aqg_groupby_agg call against the oracle (module docstring)"""
    o = ogb if ogb is not None else oracle.groupby(keys)
    gb = gpu.groupby_agg(keys, ops, vals, hint=hint)                 # (a status other than AQG_OK raises)
    plan = gb.plan
    print(f"{what}: plan {plan:#x} (asserted: has {want_plan_bits:#x}, has none of {forbid_bits:#x}); {gb.ngroups} groups; "
          f"{[RED_NAME[op] for op in ops]}", flush=True)
    assert plan & want_plan_bits == want_plan_bits and not plan & forbid_bits, (what, "plan", hex(plan), hex(want_plan_bits), hex(forbid_bits))
    assert gb.ngroups == o["ngroups"], (what, gb.ngroups, o["ngroups"])
    assert np.array_equal(gb.first_rows(), o["first_rows"]), what
    for k, c in enumerate(keys):
        assert np.array_equal(gb.keys(k, c.dtype), c[o["first_rows"]]), (what, "key column", k)
    cnt = gb.counts()
    if any(op in (COUNT, AVG, VAR, STDDEV) for op in ops):
        assert cnt is not None, (what, "counts")
    if cnt is not None:                                              # (the handle has them whenever an op or the plan needed the group sizes)
        assert np.array_equal(cnt, o["counts"]), (what, "counts")
    stats = {}
    for j, (op, v) in enumerate(zip(ops, vals)):
        got, want = gb.result(j, op, ck.tag_of(v)), oracle.grouped_reduce(op, v, o)
        st = None
        if v.dtype.kind == "f" and op != COUNT:
            st = stats.get(id(v))
            if st is None:
                st = stats[id(v)] = group_stats(v, o)
            if op == STDDEV:
                st["oracle_var"] = oracle.grouped_reduce(VAR, v, o)
        share = compare(op, v, got, want, o, f"{what} [{j}] {ex.nm(v.dtype)}", st)
        assert share >= 0.9
    gb.destroy()
    return plan


# ---- the columns of one shape ----------------------------------------------------------------------------------------------------
INT_OPS = (SUM, MIN, MAX, COUNT, AVG, VAR, STDDEV)
NARROW_OPS = (SUM, MIN, MAX, AVG, VAR)
FP_SUM_OPS = (SUM, MIN, MAX, COUNT, AVG)
FP_SQ_OPS = (VAR, STDDEV)


def columns(lay, dtypes, seed=0, sets=("int_full", "carry", "narrow_at_end", "fp_finite", "fp_inf", "fp_nan"), late=True):
    """(name, column, ops) of every value set that has columns of the given types"""
    out = []
    for dt in (np.dtype(t) for t in dtypes):
        s = seed + 17 * dt.num
        if dt.kind in "iu":
            if "int_full" in sets:
                out.append((f"int_full({dt.name})", int_full(dt, lay, s), INT_OPS))
            if "carry" in sets and dt in (I64, U64):
                out.append((f"carry({dt.name})", carry(dt, lay, s), INT_OPS))
            if "narrow_at_end" in sets and dt in (I32, U32):
                for which in ("hi",) + (("lo",) if dt == I32 else ()) + (("late",) if late else ()):
                    out.append((f"narrow_at_end({dt.name}, {which})", narrow_at_end(dt, lay, s, which), NARROW_OPS))
        else:
            if "fp_finite" in sets:
                out.append((f"fp_finite({dt.name})", fp_finite(dt, lay, s), FP_SUM_OPS))
                out.append((f"fp_finite({dt.name}, squares)", fp_finite(dt, lay, s, "square"), FP_SQ_OPS))
            if "fp_inf" in sets:
                out.append((f"fp_inf({dt.name})", fp_inf(dt, lay, s), FP_SUM_OPS))
                out.append((f"fp_inf({dt.name}, squares)", fp_inf(dt, lay, s, "square"), FP_SQ_OPS))
            if "fp_nan" in sets and len(np.unique(lay.labels)) >= 20:       # (fewer than 20 groups: one NaN group is more than 10 %)
                for dom in (False, True):
                    out.append((f"fp_nan({dt.name}, dominant group {'in' if dom else 'out'})", fp_nan(dt, lay, s, dom), FP_SUM_OPS))
                out.append((f"fp_nan({dt.name}, squares)", fp_nan(dt, lay, s, False, "square"), FP_SQ_OPS))
    return out


def carry_layout(n, G, seed, dt, big=None):
    """a layout whose reserved groups hold the avg probes of `dt`: every e whose three groups take less than a quarter of the rows"""
    es = tuple(e for e in PROBE_E if 3 * len(ex.avg_probe_column(dt, e)[0]) < n // 4)
    lay = Layout(n, G, seed, sized=probe_sizes(dt, es), big=big)
    lay.probe_es = es
    return lay


# ---- the plans of aqg_groupby_agg ----------------------------------------------------------------------------------------------------
P = capi
N_SMALL, N_MID, N_WIDE, N_PACK = 200_003, 1_050_007, 3_200_011, 4_700_023

k_i32 = lambda L: [(L * 7 - 1000).astype(np.int32)]
k_2xi32 = lambda L: [(L % 97).astype(np.int32), (L // 97 - 5).astype(np.int32)]
k_i64 = lambda L: [(L << 33) | 5]
k_i16 = lambda L: [(L - 2000).astype(np.int16)]
k_dense = lambda L: [(L + 5).astype(np.int32)]
k_strided = lambda L: [(L * 104_729).astype(np.int32)]             # (6000 groups: up to 6.3e8, no dense domain)
k_hashed = lambda L: [(L * 5003).astype(np.int32)]
k_wide = lambda L: [(L % 100 + 1).astype(np.int32), (L // 100 % 1000).astype(np.int32), (L // 100_000 + 7).astype(np.int32), ((L * 7) % 13).astype(np.int32)]

# name -> list of shapes: n, G, key map, hint (None: G), plan bits wanted / forbidden, accumulators per call, whether the LDS budget of the
# shape has room for the group sizes, value types, value sets (None: all).  The budgets restate make_agg_plan (groupby.hip): an LDS
# table of next_pow2(hint * 4 / 3 + 1) slots of 8 + 8 * accumulators (+ 4 with counts, + 4 beside a key wider than 4 bytes) bytes must fit 76 KiB.
PLANS = {
    # one aligned int32 key, 4-byte values, 1 .. 4 accumulators.  G = 3000 fits the LDS budget with ONE accumulator and no counts only
    # (4097 slots of 16 bytes); two accumulators stop at 1535 groups, four with counts at 767 -- so the full calls run at G = 100 and 700
    "few_lds": [dict(n=N_SMALL, G=100, key=k_i32, bits=P.PLAN_FAST_LDS, acc=4, dtypes=NARROW4),
                dict(n=N_SMALL, G=700, key=k_i32, bits=P.PLAN_FAST_LDS, acc=4, dtypes=NARROW4, sets=("int_full", "narrow_at_end", "fp_nan")),
                dict(n=N_SMALL, G=3000, key=k_i32, bits=P.PLAN_FAST_LDS, acc=1, count_ok=False, dtypes=NARROW4, sets=("int_full", "fp_inf"))],
    # the VW = 8 instantiation: 1-, 2- and 8-byte values; one int32 key, two int32 keys, one int64 key (an 8-byte key: 4 bytes more per slot)
    "fast_v8": [dict(n=N_SMALL, G=100, key=k_i32, bits=P.PLAN_FAST_LDS, acc=4, dtypes=TINY_AND_WIDE, probes=True),
                dict(n=N_SMALL, G=700, key=k_2xi32, bits=P.PLAN_FAST_LDS, acc=4, dtypes=TINY_AND_WIDE, sets=("int_full", "fp_inf")),
                dict(n=N_SMALL, G=100, key=k_i64, bits=P.PLAN_FAST_LDS, acc=4, dtypes=TINY_AND_WIDE, sets=("int_full", "carry", "fp_nan")),
                dict(n=N_SMALL, G=3000, key=k_i32, bits=P.PLAN_FAST_LDS, acc=1, count_ok=False, dtypes=TINY_AND_WIDE, sets=("int_full", "fp_inf"))],
    # RowPass::HASHED inside LDS: a key the fast kernels do not take (int16), and more accumulators than they take (five to seven) on an int32 key
    "small_lds": [dict(n=N_SMALL, G=100, key=k_i16, bits=P.PLAN_SMALL_LDS, acc=7, dtypes=ALL_DT, probes=True),
                  dict(n=N_SMALL, G=700, key=k_i32, bits=P.PLAN_SMALL_LDS, acc=7, min_acc=5, dtypes=ALL_DT, sets=("int_full", "carry", "fp_inf", "fp_nan"))],
    "hbm_table": [dict(n=N_SMALL, G=20_000, key=k_i32, bits=P.PLAN_HBM_TABLE, acc=8, dtypes=ALL_DT, probes=True)],
    # direct-indexed LDS tables over the key domain: 150 KiB / (8 * accumulators + 4 (+ 4 with counts)) slots a pass, four passes -- a domain
    # of 20 000 values fits with up to two accumulators, one of 8000 with all eight
    "dense": [dict(n=N_MID, G=8000, key=k_dense, bits=P.PLAN_DENSE, acc=8, dtypes=ALL_DT, probes=True),
              dict(n=N_MID, G=20_000, key=k_dense, bits=P.PLAN_DENSE, acc=2, dtypes=[I32, U64, F32], sets=("int_full", "carry", "fp_inf"))],
    # multi-pass hashed LDS table: 150 KiB / (16 + 8 * accumulators) slots, three quarters of them a pass, four passes: 9600 groups at four accumulators
    "big_lds": [dict(n=N_MID, G=6000, key=k_strided, bits=P.PLAN_BIG_LDS, acc=4, dtypes=ALL_DT, probes=True)],
    "part_one": [dict(n=N_MID, G=300_000, key=k_hashed, hint=400_000, bits=P.PLAN_PART_ONE, forbid=P.PLAN_RANGE_PARTITIONS, acc=8, dtypes=ALL_DT, probes=True),
                 dict(n=N_MID, G=300_000, key=k_i64, hint=400_000, bits=P.PLAN_PART_ONE, acc=8, dtypes=[I32, I64, F32], sets=("int_full", "carry", "fp_nan"))],
    "part_one_ranged": [dict(n=N_PACK, G=400_000, key=k_dense, hint=500_000, bits=P.PLAN_PART_ONE | P.PLAN_RANGE_PARTITIONS, acc=8,
                             dtypes=[np.dtype(np.uint16), I64, F32, F64], sets=("int_full", "carry", "fp_inf"))],
    "part_two": [dict(n=N_MID, G=300_000, key=k_hashed, hint=400_000, bits=P.PLAN_PART_TWO, acc=8, dtypes=ALL_DT, probes=True)],
    "part_round1": [dict(n=N_MID, G=300_000, key=k_hashed, hint=400_000, bits=P.PLAN_PART_ROUND1, acc=8, dtypes=ALL_DT, probes=True)],
    "sorted_tail": [dict(n=N_MID, G=300_000, key=k_hashed, hint=400_000, bits=P.PLAN_PART_ONE | P.PLAN_SORTED_TAIL, acc=8, dtypes=ALL_DT, probes=True)],
    # four int32 key columns, a hint above 2^20, at most four accumulators (the emit path is groupby_tail.hip's, as for every plan above:
    # the 1- and 2-byte types are left to them).  A tuple that holds a third of the rows is refused BY DESIGN (partition_wide.hip: the
    # partitions are sized by rows, ~1000 each, and the call falls back to the HBM table): the large group has 48 rows here, and the
    # e = 77 avg probes (16 386 rows a group) stay with the other plans.  One test per value width: the calls of all six types together
    # take longer than the slowest forced-plan test of test_gpu_plans.py
    "part_wide_int4": [dict(n=N_WIDE, G=1_400_000, key=k_wide, hint=1_300_000, bits=P.PLAN_PART_WIDE, acc=4, big=48, dtypes=[I32, U32],
                       sets=("int_full", "carry", "narrow_at_end", "fp_inf", "fp_nan"), late=False)],
    "part_wide_int8": [dict(n=N_WIDE, G=1_400_000, key=k_wide, hint=1_300_000, bits=P.PLAN_PART_WIDE, acc=4, big=48, dtypes=[I64, U64],
                       sets=("int_full", "carry", "narrow_at_end", "fp_inf", "fp_nan"), late=False)],
    "part_wide_fp": [dict(n=N_WIDE, G=1_400_000, key=k_wide, hint=1_300_000, bits=P.PLAN_PART_WIDE, acc=4, big=48, dtypes=[F32, F64],
                       sets=("int_full", "carry", "narrow_at_end", "fp_inf", "fp_nan"), late=False)],
}
# the switches a plan is forced with (read once per process: such a plan runs in a child process)
PLAN_ENV = {"part_two": {"AQG_P1_MAX": "1"}, "part_round1": {"AQG_DISABLE_P1": "1"}, "sorted_tail": {"AQG_SORTED_TAIL_MIN": "1"},
            "part_one_cursors_off": {"AQG_DISABLE_P1_CURSORS": "1"}, "part_one_ranged_cursors_off": {"AQG_DISABLE_P1_CURSORS": "1"},
            "packed_values": {"AQG_P1_MAX": "1", "AQG_DISABLE_RANGED": "1"}}
PLANS["part_one_cursors_off"] = [dict(PLANS["part_one"][0], dtypes=[I32, U32, I64, U64, F32, F64], sets=("int_full", "carry", "fp_inf"))]
PLANS["part_one_ranged_cursors_off"] = PLANS["part_one_ranged"]


def run_shape(gpu, oracle, name, sh):
    n, G = sh["n"], sh["G"]
    hint = sh.get("hint") or G
    big = sh.get("big")
    lays = {None: Layout(n, G, 100 + G, big=big)}
    if sh.get("probes"):                                       # the carry columns take a layout whose reserved groups fit the avg probes
        lays[I64], lays[U64] = carry_layout(n, G, 101 + G, I64, big), carry_layout(n, G, 102 + G, U64, big)
    sets = sh.get("sets") or ("int_full", "carry", "narrow_at_end", "fp_finite", "fp_inf", "fp_nan")
    ncalls = 0
    for which, lay in lays.items():
        keys = sh["key"](lay.labels)
        o = oracle.groupby(keys)
        assert np.array_equal(o["reversemap"], oracle.groupby([lay.labels], postproc=False)["reversemap"]), "the key map is injective"
        assert o["counts"].max() == lay.big and np.count_nonzero(o["counts"] == 1) >= 50
        cols = columns(lay, sh["dtypes"], seed=G, sets=sets, late=sh.get("late", True)) if which is None else \
            [c for c in columns(lay, [which], seed=G, sets=("carry",))]
        if which is None and sh.get("probes"):
            cols = [c for c in cols if not c[0].startswith("carry")]
        for cname, x, ops in cols:
            for call in pack_calls(ops, x.dtype, sh["acc"], sh.get("count_ok", True)):
                if sum(acc_count(op, x.dtype) for op in call) < sh.get("min_acc", 0):
                    continue                                   # (this shape is about calls the fast kernels do not take)
                check(gpu, oracle, keys, call, [x] * len(call), hint, sh["bits"], sh.get("forbid", 0), f"{name} n={n} G~{G} {cname}", ogb=o)
                ncalls += 1
    assert ncalls > 0, (name, "no call fits this shape")
    return ncalls


def run_plan(gpu, oracle, name):
    total = sum(run_shape(gpu, oracle, name, sh) for sh in PLANS[name])
    print(f"{name}: {total} calls", flush=True)


def run_row_emit(gpu, oracle, n=N_MID):
    """a unique key, hint = n + 1000: every row its own group, the result columns are a map of the input rows (emit_rows_kernel).  The
    group shape is the plan's own -- n groups of one row -- so NaN sets are left out (every NaN row would be a whole group, and the
    recipe allows 10 % of the groups) and the other sets come as they are."""
    rng = np.random.default_rng(7)
    key = (rng.permutation(n) - 500_000).astype(np.int32)
    o = oracle.groupby([key])
    assert o["ngroups"] == n
    lay = Layout(n, 1000, 8)                                    # (only the builders' row recipe is used; the key is the unique one)
    for cname, x, ops in columns(lay, ALL_DT, seed=3, sets=("int_full", "carry", "narrow_at_end", "fp_finite", "fp_inf")):
        for call in pack_calls(ops, x.dtype, 8):
            check(gpu, oracle, [key], call, [x] * len(call), n + 1000, P.PLAN_ROW_EMIT, 0, f"row_emit n={n} {cname}", ogb=o)


def run_packed_values(gpu, oracle, n=N_PACK, G=400_000):
    """the two-level plan at >= 2^22 rows packs narrow 4-byte integer columns into the spare bits of the key word as offsets from their
    sampled minimum: columns that sit at an end of their type (field arithmetic, the rebuilt count * vmin, the int squares that wrap), and the
    late rows -- min, max, 0xFFFFFFFF in the last ten rows -- that leave the field: that call must come back UNPACKED, and equal"""
    lay = Layout(n, G, 77)
    keys = k_dense(lay.labels)
    o = oracle.groupby(keys)
    PT, PK = P.PLAN_PART_TWO, P.PLAN_PACKED_VALUES
    for dt in (I32, U32):
        for which in ("hi",) + (("lo",) if dt == I32 else ()):
            x = narrow_at_end(dt, lay, 5, which)
            for call in ([SUM, MIN, MAX], [AVG, VAR]):
                check(gpu, oracle, keys, call, [x] * len(call), 500_000, PT | PK, 0, f"packed_values narrow_at_end({dt.name}, {which})", ogb=o)
        x = narrow_at_end(dt, lay, 5, "late")
        for call in ([SUM, MIN, MAX], [AVG, VAR]):
            check(gpu, oracle, keys, call, [x] * len(call), 500_000, PT, PK, f"packed_values narrow_at_end({dt.name}, late)", ogb=o)


# ---- aqg_grouped_reduce / _flat / aqg_grouped_corr -------------------------------------------------------------------------------------
REDUCE_OPS = ("sum", "min", "max", "avg", "var", "stddev", "first", "last", "count")


def check_reduce(gpu, oracle, gb, o, x, names, what, flat=False, want_plan=None):
    """aqg_grouped_reduce (flat: aqg_grouped_reduce_flat over x laid out by the oracle's row lists) of one column, op by op"""
    xin = x[o["row_ids"]] if flat else x
    st = group_stats(x, o) if x.dtype.kind == "f" else None
    for name in names:
        op = ck.RED_NAMES[name]
        got = gpu.grouped_reduce_flat(gb, op, xin) if flat else gpu.grouped_reduce(gb, op, x)
        want = oracle.grouped_reduce(op, x, o)
        if want_plan is not None and name not in ("first", "last"):
            print(f"{what}: {name}: plan {gb.plan:#x} (asserted: has {want_plan:#x})", flush=True)
            assert gb.plan & want_plan == want_plan, (what, name, hex(gb.plan))
        if name in ("first", "last"):                       # they move NaNs as they are: every group
            assert ex.same(got, want), (what, name, ex.first_diff(got, want))
            continue
        if st is not None and name == "stddev":
            st["oracle_var"] = oracle.grouped_reduce(VAR, x, o)
        compare(op, x, got, want, o, f"{what} {ex.nm(x.dtype)}", st)


def reduce_columns(lay, dtypes, seed, sets):
    """the columns of `columns`, one per name, each with the ops of aqg_grouped_reduce that its recipe is safe for"""
    out = []
    for cname, x, ops in columns(lay, dtypes, seed=seed, sets=sets):
        names = [RED_NAME[op] for op in ops] + ([] if "squares" in cname else ["first", "last"])
        out.append((cname, x, names))
    return out


def run_grouped_reduce(gpu, oracle, n, G, seed=0):
    """a build handle's aqg_grouped_reduce through the ordinary plans: G about 1000 at 200 003 rows (LDS), about 300 000 at 1.05e6 (partitions)"""
    lays = {None: Layout(n, G, 200 + seed), I64: carry_layout(n, G, 201 + seed, I64), U64: carry_layout(n, G, 202 + seed, U64)}
    for which, lay in lays.items():
        key = k_i32(lay.labels)
        o = oracle.groupby(key)
        gb = gpu.groupby_build(key)
        assert gb.ngroups == o["ngroups"] and np.array_equal(gb.reversemap(), o["reversemap"])
        cols = reduce_columns(lay, ALL_DT, G, ("int_full", "narrow_at_end", "fp_finite", "fp_inf", "fp_nan")) if which is None else \
            reduce_columns(lay, [which], G, ("carry",))
        for cname, x, names in cols:
            check_reduce(gpu, oracle, gb, o, x, names, f"grouped_reduce n={n} G~{G} {cname}")
        gb.destroy()


def run_gid_partition(gpu, oracle, part, n=4_200_000):
    """aqg_grouped_reduce partitioned on the dense group id (n >= 2^22 rows, more than 2^16 groups): nearly every row its own group"""
    lay = Layout(n, n, 300)
    key = k_dense(lay.labels)
    o = oracle.groupby(key)
    gb = gpu.groupby_build(key)
    assert gb.ngroups == o["ngroups"] > (1 << 16) and o["counts"].max() == n // 3      # (more than 2^16 groups: the plan's own threshold)
    GP = P.PLAN_GID_PARTITION
    cols = reduce_columns(lay, [I32], 1, ("int_full", "narrow_at_end")) + reduce_columns(lay, [np.dtype(np.uint16)], 1, ("int_full",)) if part == "int" else \
        reduce_columns(lay, [F32], 1, ("fp_inf", "fp_nan"))
    for cname, x, names in cols:
        names = [nm_ for nm_ in names if nm_ != "count"]
        check_reduce(gpu, oracle, gb, o, x, names, f"gid_partition {cname}", want_plan=GP)
    if part == "int":
        x = int_full(I64, lay, 2)                              # (8-byte integer sums keep the hashed plans: min and max only)
        check_reduce(gpu, oracle, gb, o, x, ["min", "max"], "gid_partition int_full(int64)", want_plan=GP)
    gb.destroy()


def run_reduce_flat(gpu, oracle, n, G):
    ones = ONES if G > 200 else 0
    lays = {None: Layout(n, G, 400 + G, ones=ones)}
    if n > 100_000:
        lays[I64], lays[U64] = carry_layout(n, G, 401, I64), carry_layout(n, G, 402, U64)
    for which, lay in lays.items():
        key = k_i32(lay.labels)
        o = oracle.groupby(key)
        gb = gpu.groupby_build(key)
        assert gb.ngroups == o["ngroups"]
        sets = ("int_full", "carry", "narrow_at_end", "fp_finite", "fp_inf", "fp_nan")
        cols = reduce_columns(lay, ALL_DT, G, sets) if which is None else reduce_columns(lay, [which], G, ("carry",))
        for cname, x, names in cols:
            check_reduce(gpu, oracle, gb, o, x, names, f"grouped_reduce_flat n={n} G~{G} {cname}", flat=True)
        gb.destroy()


CORR_PAIRS = [(np.int32, np.int32), (np.uint32, np.int32), (np.int8, np.uint16), (np.int16, np.int16)]


def run_corr(gpu, oracle, n, G):
    """aqg_grouped_corr of full-range columns, bit for bit against the oracle's corr of every group's rows (products in the operands' C++
    type, five 128-bit sums); one group's x is constant: a zero denominator, the oracle's answer whatever it is"""
    lay = Layout(n, G, 500 + G, sized=(3,), ones=ONES if G > 200 else 0)
    key = k_i32(lay.labels)
    o = oracle.groupby(key)
    gb = gpu.groupby_build(key)
    assert gb.ngroups == o["ngroups"]
    for tx, ty in CORR_PAIRS:
        x, y = ex.unary_column(tx, n, 31), ex.unary_column(ty, n, 32)
        x[lay.sized_rows[0]] = 7
        got = gpu.grouped_corr(gb, x, y)
        want = np.empty(o["ngroups"], np.float64)
        for g in range(o["ngroups"]):
            rows = o["row_ids"][o["offsets"][g]: o["offsets"][g] + o["counts"][g]]
            want[g] = oracle.corr(x[rows], y[rows])
        const = int(o["reversemap"][lay.sized_rows[0][0]])
        assert ex.same(got[const:const + 1], want[const:const + 1]), ("constant x", got[const], want[const])
        assert ex.same(got, want), (np.dtype(tx).name, np.dtype(ty).name, n, G, ex.first_diff(got, want))
    gb.destroy()
