"""The flat column operations at the numeric extremes: aqg_ewise, aqg_unary, aqg_reduce, aqg_scan and aqg_grouped_scan through the
C-ABI against the oracle (and, for aqg_ewise up to 4096 rows, against the independent model of tests/extremes.py) -- full-range
values of every type, the ends of each type and their neighbours, zero divisors, INT_MIN / -1, wrapping sums and differences, 128-bit
sums that carry and have to be rounded, +-Inf, -0.0, subnormals and NaNs, at sizes around the vector / tile / chain-link borders and
with operands that are aligned to their element size only.

How results are compared: integer, index and bool outputs bit for bit; min / max family and shifts of floating columns bit for bit;
floating sums within DESIGN.md section 2's bound k * 2^-52 * sum|x| over the k rows that contribute where the oracle's value is
finite, the same infinity / a NaN where it is not (the bound divided by the row count for means).  For sum / avg / sums / avgs the
rows that contribute are rows 0 ... i.  A window's rows are the window's: `sumw / avgw` of floating columns are held to a window sum
computed here in numpy over exactly the rows the device's route adds -- the window itself on the direct route (w <= 64), the tile and
its halo on the prefix-difference route, see the table -- with the bound over those rows; the oracle's recurrence, whose own error
grows with the whole prefix, is compared under the prefix-wide bound next to it.  `avgw` of integer columns is the exact window sum
(python int) rounded to double and divided by the window's length, to one ulp.

What is left out, and why -- nothing else is skipped, and nothing is skipped depending on the data:

  case                                              out of contract because
  ------------------------------------------------  ------------------------------------------------------------------------------
  avgw on uint32 / uint64 columns                   DESIGN.md 2: "`avgw` on unsigned 4/8-byte inputs wraps `arr[i]-arr[i-w]` ...; the
                                                    device returns the true mean"
  avgw on int32 / int64 columns at full range       the same expression overflows a signed type there (undefined in the reference): these
                                                    columns are halved for avgw, which keeps arr[i] - arr[i-w] inside the type
  a floating VALUE into an integer result type      include/aqg.h, aqg_ewise: "evaluated in the C++ usual-arithmetic-conversion type ... then
                                                    converted to `ot`" -- that conversion is undefined in C++ once out of range
  default result type of uint64 with another type   DESIGN.md 2: "`Coercion<uint64, other>` is `const char*`" (aqg_ewise_out_dtype: AQG_ERROR);
                                                    the pairs are run with the expression's own C++ type as result type instead
  sumw / avgw with w == 0                           DESIGN.md 2: "`sumw/avgw` with `w == 0` read `ret[-1]` (rejected with `AQG_ERR_ARG`)"
  floating sumw / avgw, 64 < w: rounding of the     DESIGN.md 2: "Floating sums: any re-ordered summation is bounded by ..." -- these routes
  tile + halo (hbm route: of the whole prefix)      take the difference of two prefixes (scan_window.hpp window_sum_kernel: over the 2048-row tile and
  instead of the window's rows alone                its halo; prefix_diff_kernel: over the column), so that is the summation the bound is about
  NaN in a column of min / max / mins / maxs /      DESIGN.md 2, "NaN and signed zeros": the reference's folds forget what came before a NaN and
  minw / maxw or of the floating sum family         its window sums stay NaN: every output row strictly before the first NaN row is held to the
                                                    standards above, the call succeeds, nothing more (test_nan_rows_*)
  sumw / avgw rows from the reference's first       same sentence: when an Inf row leaves the window the reference's recurrence computes
  NaN OUTPUT on                                     Inf - Inf and stays NaN, the device goes back to the window's own sum
"""
import functools

import numpy as np
import pytest

import checker as ck
import extremes as ex
from test_gpu_edges import view
from test_gpu_grouped_scan import compose

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 17, 1023, 1025, 4095, 4097, 8197, 1_000_003)
OFFS = (0, 1, 3)
MODEL_MAX_N = 4096


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


# ---- element-wise -------------------------------------------------------------------------------------------------------------
def _plan():
    """every (pair, op, kind) once; its size and the three offsets (l, r, out) drawn with a fixed seed, the largest size given to one case of
    every (compute type, op, kind).  test_ewise_plan_covers checks what the draw has to guarantee."""
    rng = np.random.default_rng(20240)
    cases = [dict(lt=lt, rt=rt, op=op, kind=kind) for lt, rt, op, kind in ex.ewise_cases()]
    by, rot = {}, {}
    for i, c in enumerate(cases):
        c["n"] = int(SIZES[rng.integers(len(SIZES) - 1)])
        c["offs"] = tuple(int(v) for v in rng.choice(OFFS, 3))
        c["seed"] = 5000 + i
        side = c["rt"] if c["kind"] == "vs" else c["lt"]
        turn = rot.setdefault((c["kind"], c["op"], side), []); turn.append(i)       # the scalars of a type in rotation over the other operand's 11 types
        c["scalar"] = (len(turn) - 1) % len(ex.scalars(side)) if c["kind"] != "vv" else None
        by.setdefault((ex.compute_type(c["lt"], c["rt"]), c["op"], c["kind"]), []).append(i)
    for idx in by.values():
        cases[idx[rng.integers(len(idx))]]["n"] = SIZES[-1]
    return cases


PLAN = _plan()
PAIRS = [(lt, rt) for lt in ex.OPERAND_DTYPES for rt in ex.OPERAND_DTYPES]
pair_id = lambda p: f"{ex.nm(p[0])}-{ex.nm(p[1])}"


def test_ewise_plan_covers():
    kinds_n = {(c["kind"], c["n"]) for c in PLAN}
    assert kinds_n == {(k, n) for k in ex.KINDS for n in SIZES}
    assert {(ex.compute_type(c["lt"], c["rt"]), c["n"]) for c in PLAN} >= {(ct, n) for ct in ex.NATURAL_TAG for n in SIZES}
    assert {(c["op"], c["n"]) for c in PLAN} == {(op, n) for op in ex.ALL_OPS for n in SIZES}
    for k in ex.KINDS:                                    # vec_ok on and off for each operand and for the output
        assert {c["offs"] for c in PLAN if c["kind"] == k} == {(a, b, o) for a in OFFS for b in OFFS for o in OFFS}
    for k in ("vs", "sv"):                                # every scalar of the pool (0, -1, the minimum, the maximum, NaN, ...) of every operand type, as divisor too
        for dt in ex.OPERAND_DTYPES:
            for op in ex.ops_for(dt, dt):
                drawn = {c["scalar"] for c in PLAN if c["kind"] == k and c["op"] == op and c["rt" if k == "vs" else "lt"] == dt}
                assert drawn == set(range(len(ex.scalars(dt)))), (k, dt, op, drawn)
    big = [c for c in PLAN if c["n"] == SIZES[-1]]
    assert {c["lt"] for c in big} == set(ex.OPERAND_DTYPES) and {c["rt"] for c in big} == set(ex.OPERAND_DTYPES)
    assert {(c["lt"], c["rt"]) for c in PLAN} == set(PAIRS) and len(PAIRS) == 121


@functools.lru_cache(maxsize=8)
def _columns(lt, rt, n, seed):
    return ex.binary_columns(lt, rt, n, seed)


def run_ewise(gpu, oracle, op, kind, l, r, ot, offs, what):
    n = len(l) if kind != "sv" else len(r)
    dl = view(gpu, l, offs[0]) if kind != "sv" else l
    dr = view(gpu, r, offs[1]) if kind != "vs" else r
    out = view(gpu, np.zeros(n, ck.TAG2NP[ot]), offs[2])
    got = gpu.ewise(op, dl, dr, ot=ot, out=out)
    for name, want in (("oracle", oracle.ewise(op, l, r, ot=ot)),) + ((("model", ex.model_ewise(op, l, r, kind, ot)),) if n <= MODEL_MAX_N else ()):
        if not ex.same(got, want):
            i = ex.first_diff(got, want)
            la, ra = np.atleast_1d(l), np.atleast_1d(r)
            raise AssertionError(f"{what} n={n} offs={offs} -> {ex.OT_NAME[ot]}: row {i}: {la[i % len(la)]!r} {ex.OP_NAME[op]} {ra[i % len(ra)]!r}: "
                                 f"device {got[i]!r}, {name} {want[i]!r}")


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_ewise(gpu, oracle, pair):
    lt, rt = pair
    tl, tr = ex.tag(lt), ex.tag(rt)
    for c in (c for c in PLAN if (c["lt"], c["rt"]) == pair):
        op, kind, n = c["op"], c["kind"], c["n"]
        assert gpu.lib.aqg_ewise_out_dtype(op, tl, tr) == oracle.ewise_out_dtype(op, tl, tr)
        l, r = _columns(lt, rt, n, 40 + tl * 32 + tr)
        if kind == "vs":
            r = ex.scalars(rt)[c["scalar"]]
        if kind == "sv":
            l = ex.scalars(lt)[c["scalar"]]
        run_ewise(gpu, oracle, op, kind, l, r, ex.default_ot(oracle, op, lt, rt), c["offs"], f"{ex.nm(lt)} {ex.nm(rt)} {kind}")


@pytest.mark.parametrize("ctype", list(ex.OT_SWEEP_PAIRS), ids=lambda c: f"{c[0]}{c[1]}")
def test_ewise_every_result_type(gpu, oracle, ctype):
    """the (compute type, result type) kernels that no default result type reaches: every result type the call accepts, on one pair per
    compute type, the three kinds, sizes and offsets in rotation"""
    lt, rt = (np.dtype(t) for t in ex.OT_SWEEP_PAIRS[ctype])
    k = 0
    for op in ex.ops_for(lt, rt):
        for ot in ex.accepted_ots(op, lt, rt):
            for kind in ex.KINDS:
                n = SIZES[k % (len(SIZES) - 1)]
                offs = (OFFS[k % 3], OFFS[k // 3 % 3], OFFS[k // 9 % 3])
                k += 1
                l, r = _columns(lt, rt, n, 7)
                if kind == "vs":                         # the scalars in rotation: each of them meets every result type
                    r = ex.scalars(rt)[k % len(ex.scalars(rt))]
                if kind == "sv":
                    l = ex.scalars(lt)[k % len(ex.scalars(lt))]
                run_ewise(gpu, oracle, op, kind, l, r, ot, offs, f"{ex.nm(lt)} {ex.nm(rt)} {kind}")


def test_ewise_rejects_what_it_does_not_compute(gpu):
    import aquery2_amd
    f, i = np.array([1.5, 2.5], np.float32), np.array([3, 4], np.int32)
    for op in ex.INT_ONLY_OPS:
        with pytest.raises(aquery2_amd.AqgError):
            gpu.ewise(op, f, i, ot=ck.INT32)
    with pytest.raises(aquery2_amd.AqgError):
        gpu.ewise(ck.OP_ADD, f, i, ot=ck.INT128)
    with pytest.raises(aquery2_amd.AqgError):
        gpu.ewise(ck.OP_ADD, np.array([1], np.uint64), i)           # no default result type (table above)


# ---- sqrt / truncate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ex.NUM_DTYPES, ids=ex.nm)
def test_sqrt(gpu, oracle, dt):
    for n, off in ((1, 0), (17, 1), (4097, 3), (100_003, 0), (100_003, 1)):
        x = ex.unary_column(dt, n, 300 + n + off)
        got, want = gpu.unary(ck.UN_SQRT, view(gpu, x, off)), oracle.unary(ck.UN_SQRT, x)
        assert ex.same(got, want), (n, off, ex.first_diff(got, want))


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("p", ex.TRUNC_P)
def test_truncate(gpu, oracle, dt, p):
    t = ex.truncate_column(dt, p)
    for n, off in ((len(t), 0), (len(t), 1), (20_001, 3)):
        x = np.concatenate([t, ex.unary_column(dt, n - len(t), 400 + p)]) if n > len(t) else t
        got, want = gpu.unary(ck.UN_TRUNCATE, view(gpu, x, off), p), oracle.unary(ck.UN_TRUNCATE, x, p)
        assert ex.same(got, want), (n, off, ex.first_diff(got, want), x[ex.first_diff(got, want)])


# ---- reductions ------------------------------------------------------------------------------------------------------------------------
RED_N = (1, 3, 100_003, 3_000_001)
INT_REDS = ("sum", "min", "max", "count", "avg", "var", "stddev", "first", "last")
FP_REDS = ("sum", "min", "max", "count", "avg", "first", "last")


def exact_sum_fast(x):
    """exact sum of an integer column as a python int (32-bit halves summed in 64 bits)"""
    if x.dtype.itemsize < 8:
        return int(x.astype(np.int64).sum())
    lo = int((x.view(np.uint64) & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))
    hi = int((x >> x.dtype.type(32)).astype(np.int64 if x.dtype.kind == "i" else np.uint64).sum())
    return (hi << 32) + lo


def fp_sum_ok(got, want, bound):
    got, want = float(got), float(want)
    if np.isfinite(want):
        return abs(got - want) <= bound
    return got == want if np.isinf(want) else np.isnan(got)


@pytest.mark.parametrize("dt", ex.INT_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("n", RED_N)
def test_reduce_integers(gpu, oracle, dt, n):
    for off in (0, 1):
        x = ex.unary_column(dt, n, 600 + n + off)
        d = view(gpu, x, off)
        for name in INT_REDS:
            op = ck.RED_NAMES[name]
            got, want = gpu.reduce(op, d), oracle.reduce(op, x)
            assert (got == want) if isinstance(want, int) else ex.same(np.asarray(got), np.asarray(want)), (name, off, got, want)
        assert gpu.reduce(ck.RED_SUM, d) == exact_sum_fast(x)


@pytest.mark.parametrize("dt", [np.dtype(np.int64), np.dtype(np.uint64)], ids=ex.nm)
@pytest.mark.parametrize("n", RED_N[2:])
def test_reduce_accumulator_carries_and_borrows(gpu, oracle, dt, n):
    """the 128-bit sum of an 8-byte column carries into its high word and borrows from it again and again: a random walk over the type's
    ends; then runs of one sign, which carry (or borrow) on every row"""
    ii = np.iinfo(dt)
    rng = np.random.default_rng(n + dt.num)
    ends = np.array([ii.max, ii.max - 1, ii.min, ii.min + 1, 1, 0] + ([-1] if dt.kind == "i" else []), dtype=dt)
    walk = ends[rng.integers(0, len(ends), n)]
    up = np.full(n, ii.max, dtype=dt)
    cols = [walk, up] + ([np.full(n, ii.min, dtype=dt), np.concatenate([up[: n // 2], np.full(n - n // 2, ii.min, dtype=dt)])] if dt.kind == "i" else [])
    for x in cols:
        for off in (0, 1):
            d = view(gpu, x, off)
            s = exact_sum_fast(x)
            assert gpu.reduce(ck.RED_SUM, d) == s == oracle.reduce(ck.RED_SUM, x)
            got = gpu.reduce(ck.RED_AVG, d)
            assert np.float64(got).tobytes() == np.float64(oracle.reduce(ck.RED_AVG, x)).tobytes() == np.float64(float(s) / float(n)).tobytes()


AVG_PROBES = [(dt, e, odd, neg) for dt in (np.int64, np.uint64) for e in (53, 63, 64, 77, 84) for odd in (False, True)
              for neg in ((False, True) if dt is np.int64 else (False,))]


@pytest.mark.parametrize("dt,e,odd,neg", AVG_PROBES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_avg_rounds_the_128_bit_sum_once(gpu, oracle, dt, e, odd, neg):
    """sums S - 1, S, S + 1 around an exact tie at the bit a double rounds at (tests/extremes.py avg_probe_column): avg, and avgs over
    the same rows, are float(sum) / float(count)"""
    import aquery2_amd
    x, sums = ex.avg_probe_column(dt, e, odd=odd, negative=neg)
    n = len(x)
    d = gpu.to_device(x)
    running = gpu.scan(ck.SCAN_AVGS, d)
    assert ex.same(running, oracle.scan(ck.SCAN_AVGS, x)), ex.first_diff(running, oracle.scan(ck.SCAN_AVGS, x))
    for j, s in enumerate(sums):
        cnt = n - 2 + j
        head = aquery2_amd.DevBuf(gpu, d.ptr, x.dtype, cnt, owned=False)
        want = np.float64(float(s) / float(cnt))
        assert gpu.reduce(ck.RED_SUM, head) == s
        assert np.float64(gpu.reduce(ck.RED_AVG, head)).tobytes() == want.tobytes(), (j, s)
        assert running[cnt - 1].tobytes() == want.tobytes(), (j, s)


@pytest.mark.parametrize("dt", [np.dtype(np.int64), np.dtype(np.uint64)], ids=ex.nm)
def test_avgs_sums_from_the_first_row_rounded_to_double(gpu, oracle, dt):
    """`s = ret[0] = arr[0]` (aggregations.h:224): the reference's running mean starts from the first row as a DOUBLE; where a double cannot
    hold that row, every later sum carries the difference -- whole columns and every group of a grouped scan"""
    for k, first in enumerate(ex.unrepresentable_first_rows(dt)):
        for n in (1, 5, 2049, 70_001):
            x = ex.unary_column(dt, n, 650 + k)
            x[0] = first
            got, want = gpu.scan(ck.SCAN_AVGS, view(gpu, x, k % 2)), oracle.scan(ck.SCAN_AVGS, x)
            assert ex.same(got, want), (first, n, ex.first_diff(got, want))


@pytest.mark.parametrize("dt", [np.dtype(np.int64), np.dtype(np.uint64)], ids=ex.nm)
def test_sharded_avgs_sums_from_the_columns_first_row_rounded(oracle, dt):
    """aqg_scan_sharded: one column, one definition of avgs -- the shards behind the first add the rounding of the COLUMN's first row to
    their carry, so the shards together equal aqg_scan of the whole column (the oracle's answer), an empty leading shard included"""
    import aquery2_amd
    n = 60_013
    cols = []
    for k, first in enumerate(ex.unrepresentable_first_rows(dt)[:4]):
        x = ex.unary_column(dt, n, 670 + k)
        x[0] = first
        cols.append(x)
    for cuts in ([(0, 20_000), (20_000, 20_003), (20_003, n)], [(0, 0), (0, 41_000), (41_000, n)]):
        tr = aquery2_amd.ThreadRanks(len(cuts))
        def body(rank, dev, comm):
            lo, hi = cuts[rank]
            return [comm.scan_sharded(ck.SCAN_AVGS, dev.to_device(np.ascontiguousarray(x[lo:hi]))) for x in cols]
        try:
            res = tr.run(body)
        finally:
            tr.close()
        for ci, x in enumerate(cols):
            got, want = np.concatenate([res[r][ci] for r in range(len(cuts))]), oracle.scan(ck.SCAN_AVGS, x)
            assert ex.same(got, want), (cuts, int(x[0]), ex.first_diff(got, want))


def fp_columns(dt, n, seed):
    """(name, column) for the floating reductions and prefix sums: finite and safe to sum in any order; the same with +Inf rows; with
    infinities of both signs (the sum is NaN from the second sign on)"""
    rng = np.random.default_rng(seed)
    fin = ex.sum_safe(ex.one_sign_zeros(ex.unary_column(dt, n, seed, nan=False, inf=False)))
    pinf, both = fin.copy(), fin.copy()
    at = rng.integers(0, n, 3)
    pinf[at] = np.inf
    both[at] = np.inf
    both[rng.integers(0, n, 2)] = -np.inf
    return (("finite", fin), ("+inf", pinf), ("+-inf", both))


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("n", RED_N)
def test_reduce_floating(gpu, oracle, dt, n):
    for cname, x in fp_columns(dt, n, 700 + n):
        for off in (0, 1):
            d = view(gpu, x, off)
            finite_abs = np.abs(x[np.isfinite(x)].astype(np.float64)).sum()
            for name in FP_REDS:
                op = ck.RED_NAMES[name]
                got, want = gpu.reduce(op, d), oracle.reduce(op, x)
                if name in ("sum", "avg"):
                    bound = n * 2.0 ** -52 * finite_abs / (n if name == "avg" else 1)
                    assert fp_sum_ok(got, want, bound), (cname, name, off, got, want, bound)
                else:
                    assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), (cname, name, off, got, want)


def var_bound(x):
    """4 n 2^-52 ssq / (n + 1): the bound of test_reduce_var_stddev_floating's docstring for a column whose squares stay finite"""
    n = len(x)
    with np.errstate(over="ignore"):
        return 4 * n * 2.0 ** -52 * float(np.sum(x.astype(np.float64) ** 2)) / (n + 1)


def check_var_stddev_safe(gv, wv, gs, ws, bound, what=()):
    """var and stddev of a square_safe column (device gv / gs, oracle wv / ws) under `bound` = var_bound of the column"""
    gv, wv, gs, ws = float(gv), float(wv), float(gs), float(ws)
    assert np.isfinite(wv) and abs(gv - wv) <= bound, ("var",) + tuple(what) + (gv, wv, bound)
    if wv > bound:
        assert abs(gs - ws) <= bound / np.sqrt(wv - bound) + 2.0 ** -52 * ws, ("stddev",) + tuple(what) + (gs, ws)
    else:                                            # a variance within its own error of zero: either side may take the root of a negative number
        assert np.isnan(gs) or abs(gs - (ws if np.isfinite(ws) else 0.0)) <= np.sqrt(2 * bound), ("stddev",) + tuple(what) + (gs, ws)


def check_var_stddev_any(name, got, want, x, what=()):
    """var / stddev of a column whose squares may overflow: inside var_bound where the oracle's value is finite, else the same infinity, or also a NaN"""
    got, want = float(got), float(want)
    if np.isfinite(want):                            # (short columns: nothing overflowed)
        tol = var_bound(x)
        assert abs(got - want) <= (tol if name == "var" else max(np.sqrt(tol), tol / max(want, 1e-300))), tuple(what) + (name, got, want)
    else:
        assert got == want if np.isinf(want) else np.isnan(got), tuple(what) + (name, got, want)


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("n", RED_N)
def test_reduce_var_stddev_floating(gpu, oracle, dt, n):
    """var = (ssq - s * s / (n + 1)) / (n + 1), the squares in the column's type, the sums in double (aggregations.h:332-348).  Squares that stay
    finite: both sides round the same products and differ by the order of two sums -- |d ssq| <= n 2^-53 ssq, |d (s s)| <= 2 |s| n 2^-53 sum|x|
    <= 2 n^2 2^-53 ssq (Cauchy-Schwarz), so |d var| <= 4 n 2^-52 ssq / (n + 1) with room for the three last roundings; stddev: that over
    sqrt(var).  Full range: the squares overflow on both sides -- the same infinity, or also a NaN."""
    fin = ex.one_sign_zeros(ex.unary_column(dt, n, 750 + n, nan=False, inf=False))
    sq = ex.square_safe(fin)
    bound = var_bound(sq)
    for off in (0, 1):
        d = view(gpu, sq, off)
        check_var_stddev_safe(gpu.reduce(ck.RED_VAR, d), oracle.reduce(ck.RED_VAR, sq), gpu.reduce(ck.RED_STDDEV, d), oracle.reduce(ck.RED_STDDEV, sq), bound, (off,))
        for cname, x in (("full range", fin),) + fp_columns(dt, n, 760 + n):
            dx = view(gpu, x, off)
            for name in ("var", "stddev"):
                check_var_stddev_any(name, gpu.reduce(ck.RED_NAMES[name], dx), oracle.reduce(ck.RED_NAMES[name], x), x, (cname, off))


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_reduce_minmax_seeds(gpu, oracle, dt):
    """the reference seeds max with numeric_limits<T>::min() -- the smallest positive normal -- and min with max(): the max of an
    all-negative column is that seed, the min of an all-+Inf column is the largest finite value"""
    fi = np.finfo(dt)
    for n in (3, 100_003):
        neg = -np.abs(ex.unary_column(dt, n, 800 + n, nan=False)) - dt.type(fi.tiny)
        assert np.all(neg < 0)
        inf = np.full(n, np.inf, dtype=dt)
        for off in (0, 1):
            assert oracle.reduce(ck.RED_MAX, neg) == dt.type(fi.tiny) and oracle.reduce(ck.RED_MIN, inf) == dt.type(fi.max)
            assert gpu.reduce(ck.RED_MAX, view(gpu, neg, off)).tobytes() == dt.type(fi.tiny).tobytes()
            assert gpu.reduce(ck.RED_MIN, view(gpu, inf, off)).tobytes() == dt.type(fi.max).tobytes()
            assert gpu.reduce(ck.RED_MIN, view(gpu, neg, off)).tobytes() == oracle.reduce(ck.RED_MIN, neg).tobytes()
            assert gpu.reduce(ck.RED_MAX, view(gpu, -inf, off)).tobytes() == oracle.reduce(ck.RED_MAX, -inf).tobytes()


# ---- scans -------------------------------------------------------------------------------------------------------------------------------
SCAN_N = (2047, 2049, 70_001, 3_000_001)
PREFIX_OPS = ("sums", "avgs", "mins", "maxs", "deltas", "prev", "aggnext")
TS = 2048                                                    # rows per tile (scan_dev.hpp)
HALO_MAX_BYTES = 96 * 1024


# The two functions below restate the dispatch of aqg_scan (scan.hip, `case AQG_SCAN_MINW: case AQG_SCAN_MAXW:` -- the ww == n test and the
# van Herk candidates `for (int cand : {9, 7, 5, 3})` / `{5, 7, 9, 11}`) and of window_scan (scan_window.hpp: `lds <= HALO_MAX_BYTES` for both
# families, `ww <= DIRECT_MAX_W` (64) for floating sums; scan_dev.hpp: TS, HALO_MAX_BYTES).  A change of those constants has to be made here too:
# the names only label the test ids and choose window_reference's span, every window length is compared with the oracle whatever its route.
def minmax_route(dt, n, w, aligned):
    """the route aqg_scan takes for minw / maxw (scan.hip, case AQG_SCAN_MINW)"""
    sz = np.dtype(dt).itemsize
    ww = n if (w == 0 or w > n) else w
    if ww == n:
        return "w-ge-n"
    if ww >= 128 and aligned and n >= 64:
        V = 16 // sz
        hp = (ww - 1 + V - 1) // V * V
        cands = [c for c in (3, 5, 7, 9, 11) if (sz <= 4 or c <= 7) and c * 2048 * sz <= 150 * 1024 and c * 1024 >= 2 * hp + V]
        if cands:
            return "van-herk"
    return "doubling" if (TS + (ww - 1 + 7) // 8 * 8) * sz * 2 <= HALO_MAX_BYTES else "hbm"


def sum_route(dt, n, w):
    """the route aqg_scan takes for sumw / avgw (scan.hip, case AQG_SCAN_SUMW)"""
    dt = np.dtype(dt)
    ww = min(w, n)
    if dt.kind == "f" and ww <= 64:
        return "direct"
    acc = 8 if dt.kind == "f" or dt.itemsize <= 4 else 16
    return "lds" if (TS + (ww - 1 + 7) // 8 * 8) * acc <= HALO_MAX_BYTES else "hbm"


# (id, w, minw / maxw route at 3 000 001 aligned rows, sumw / avgw route there); w None: n + 3
ROUTES = [("short-doubling-w5", 5, "doubling", "lds"), ("doubling-w100", 100, "doubling", "lds"), ("van-herk-w128", 128, "van-herk", "lds"),
          ("van-herk-w1000", 1000, "van-herk", "lds"), ("hbm-fallback-w50000", 50_000, "hbm", "hbm"), ("w-ge-n", None, "w-ge-n", "hbm")]


def test_routes_are_the_ones_named():
    for rid, w, mm, sm in ROUTES:
        for dt in ex.NUM_DTYPES:
            n = SCAN_N[-1]
            ww = n + 3 if w is None else w
            assert minmax_route(dt, n, ww, True) == mm, (rid, dt)
            if w is not None:
                assert sum_route(dt, n, ww) == ("direct" if dt.kind == "f" and ww <= 64 else sm), (rid, dt)
    assert minmax_route(np.int32, SCAN_N[-1], 1000, False) == "doubling"        # a misaligned column cannot take van Herk
    assert sum_route(np.int64, SCAN_N[-1], 5000) == "hbm" and sum_route(np.int32, SCAN_N[-1], 5000) == "lds"


def link_rows(dt):
    return (8 if np.dtype(dt).itemsize <= 4 else 4) * TS     # rows per chain link (scan.hip chain_m)


def inf_runs_column(dt, n, seed, sign=1.0):
    """full-range finite values (zeros of one sign, no NaN) with runs of +Inf (sign = 1; -Inf for -1) and of the other infinity: at the
    start, at the end, over a whole 2048-row tile, across a chain link's border, and one of 60 000 rows -- longer than every window used"""
    x = ex.one_sign_zeros(ex.unary_column(dt, n, seed, nan=False, inf=False))
    a, b = dt.type(sign * np.inf), dt.type(-sign * np.inf)
    L = link_rows(dt)
    runs = [(0, min(700, n // 8), a), (n - min(300, n // 8), n, b), (n // 2, n // 2 + min(300, n // 8), b)]
    if n > 3 * TS + 64:
        runs.append((2 * TS - 10, 3 * TS + 10, b))
    if n > L + 4096:
        runs.append((L - 50, L + 50, a))
    if n > 200_000:
        runs += [(100_000, 160_000, a), (40 * L - 3, 40 * L + 2, b)]
    for lo, hi, v in runs:
        x[lo:hi] = v
    return x


def window_reference(x, w, route):
    """(sum over the last min(i + 1, w) rows, bound) computed over exactly the rows a route of aqg_scan adds, in double:
    direct -- the window's rows, oldest first; bound w 2^-52 sum|x| over the window.
    lds    -- the difference of two prefixes over the row's 2048-row tile and its halo of w - 1 rows rounded up to 8 (scan_window.hpp window_sum_kernel);
              bound (halo + 2048) 2^-52 sum|x| over tile and halo.
    Rows whose span holds an infinity come out non-finite here and are left to the comparison with the oracle."""
    from numpy.lib.stride_tricks import sliding_window_view as swv
    n = len(x)
    x64 = x.astype(np.float64)
    ax = np.abs(x64)
    ax[~np.isfinite(ax)] = np.inf
    with np.errstate(all="ignore"):
        if route == "direct":
            pad = np.zeros(w - 1)
            return swv(np.concatenate([pad, x64]), w).sum(axis=1), w * (2.0 ** -52 * swv(np.concatenate([pad, ax]), w).sum(axis=1) + 5e-324)
        assert route == "lds", route
        H = (w - 1 + 7) // 8 * 8
        nt = (n + TS - 1) // TS
        tiles = lambda a: swv(np.concatenate([np.zeros(H), a, np.zeros(nt * TS - n)]), H + TS)[::TS][:nt]
        C = np.concatenate([np.zeros((nt, 1)), np.cumsum(tiles(x64), axis=1)], axis=1)          # C[t, p + 1] = prefix up to LDS position p
        i = np.arange(nt * TS).reshape(nt, TS)
        ln = np.minimum(i + 1, w)
        idx = H + np.arange(TS)[None, :]
        ref = np.take_along_axis(C, idx + 1, axis=1) - np.take_along_axis(C, idx + 1 - ln, axis=1)
        bound = np.broadcast_to(((H + TS) * (2.0 ** -52 * tiles(ax).sum(axis=1) + 5e-324))[:, None], ref.shape)     # (+ one subnormal step per row)
        return ref.reshape(-1)[:n], bound.reshape(-1)[:n]


def check_fp_sums(name, got, want, x, w=None, route=None):
    """the floating sum family row by row (module docstring).  Every row up to the oracle's first NaN output (windows) against the oracle
    under the prefix-wide bound -- its recurrence has touched every earlier row; window rows on the direct / lds routes also against
    window_reference under the bound over the rows that route adds."""
    n = len(x)
    i = np.arange(n, dtype=np.float64)
    absx = np.abs(x.astype(np.float64))
    absx[~np.isfinite(absx)] = 0.0
    eps = 2.0 ** -23 if (name == "avgw" and x.dtype == np.float32) else 2.0 ** -52     # (the reference subtracts arr[i] - arr[i-w] in float)
    bound = (i + 1) * eps * np.cumsum(absx)
    if name == "avgs":
        bound /= i + 1
    if name == "avgw":
        bound /= np.minimum(i + 1, w)
    got, want = got.astype(np.float64), want.astype(np.float64)
    stop = n
    if name in ("sumw", "avgw") and np.isnan(want).any():
        stop = int(np.nonzero(np.isnan(want))[0][0])
    g, t, b = got[:stop], want[:stop], bound[:stop]
    fin, inf, nan = np.isfinite(t), np.isinf(t), np.isnan(t)
    with np.errstate(invalid="ignore"):
        bad = (fin & ~(np.abs(g - t) <= b)) | (inf & (g != t)) | (nan & ~np.isnan(g))
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{name} w={w}: row {r}: device {g[r]!r}, oracle {t[r]!r}, bound {b[r]!r}")
    if name in ("sumw", "avgw") and route in ("direct", "lds"):
        check_window_route(name, g, x, w, route)


def check_window_route(name, g, x, w, route, first=0):
    """floating sumw / avgw rows `first` ... len(g) - 1 of `g` (double; the caller has cut it at the oracle's first NaN output) against window_reference:
    the sum of the rows the direct / lds route adds over the column `x`, under the bound over those rows"""
    stop = len(g)
    ref, rb = window_reference(x, w, route)
    if name == "avgw":
        ln = np.minimum(np.arange(len(x), dtype=np.float64) + 1, w)
        ref, rb = ref / ln, rb / ln
    with np.errstate(invalid="ignore"):
        bad = np.isfinite(ref[:stop]) & np.isfinite(rb[:stop]) & ~(np.abs(g - ref[:stop]) <= rb[:stop])
    bad[:first] = False
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{name} w={w} ({route} route): row {r}: device {g[r]!r}, sum of the route's rows {ref[r]!r}, bound {rb[r]!r}")


def check_int_avgw(got, x, w):
    """avgw of an integer column: the exact window sum (python int) rounded to double once, divided by the window's length -- to one ulp"""
    n = len(x)
    if x.dtype.itemsize < 8:
        c = np.concatenate([[0], np.cumsum(x.astype(np.int64))])
    else:
        c = np.concatenate([np.array([0], dtype=object), np.cumsum(x.astype(object))])
    ln = np.minimum(np.arange(n) + 1, w)
    hi = np.arange(n) + 1
    exact = (c[hi] - c[hi - ln]).astype(np.float64) / ln              # python int -> float: correctly rounded
    bad = ~(np.abs(got - exact) <= np.spacing(np.abs(exact)))
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"avgw w={w}: row {r}: device {got[r]!r}, exact mean {exact[r]!r}")


def int_column(dt, n, seed, name):
    """full range; halved for avgw of int32 / int64 (table in the module docstring)"""
    x = ex.unary_column(dt, n, seed)
    return x >> dt.type(1) if name == "avgw" and dt.kind == "i" and dt.itemsize >= 4 else x


@pytest.mark.parametrize("dt", ex.INT_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("n", SCAN_N)
def test_scan_prefix_and_shifts_integers(gpu, oracle, dt, n):
    """running sums that pass 64 bits (8-byte columns), negative carries, running extremes that sit at the type's ends, differences that
    wrap -- through the tiles, the aggregate scan (two levels from 3 000 001 rows) and hundreds of chain links"""
    for off in (0, 1):
        x = ex.unary_column(dt, n, 900 + n + off)
        d = view(gpu, x, off)
        for name in PREFIX_OPS:
            got, want = gpu.scan(ck.SCAN_NAMES[name], d), oracle.scan(ck.SCAN_NAMES[name], x)
            assert ex.same(got, want), (name, off, ex.first_diff(got, want))
    if dt.itemsize == 8:                                     # one sign only: the 128-bit running sum carries (borrows) on every row
        for v in (np.iinfo(dt).max,) + ((np.iinfo(dt).min,) if dt.kind == "i" else ()):
            x = np.full(n, v, dtype=dt)
            x[::7] = 1
            for name in ("sums", "avgs"):
                got, want = gpu.scan(ck.SCAN_NAMES[name], x), oracle.scan(ck.SCAN_NAMES[name], x)
                assert ex.same(got, want), (name, v, ex.first_diff(got, want))
            assert ck.i128_to_int(gpu.scan(ck.SCAN_SUMS, x)[-1:])[0] == exact_sum_fast(x)


@pytest.mark.parametrize("dt", ex.INT_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r[0])
def test_scan_windows_integers(gpu, oracle, dt, route):
    rid, w0, mm, sm = route
    for n in SCAN_N:
        w = n + 3 if w0 is None else w0
        for off in (0, 1):
            for name in ("sumw", "avgw", "minw", "maxw", "ratiow"):
                if name == "avgw" and dt.kind == "u" and dt.itemsize >= 4:
                    continue                                 # table in the module docstring
                x = int_column(dt, n, 1000 + n, name)
                got, want = gpu.scan(ck.SCAN_NAMES[name], view(gpu, x, off), w), oracle.scan(ck.SCAN_NAMES[name], x, w)
                if name == "avgw":
                    check_fp_sums(name, got, want, x, min(w, n))     # the oracle's recurrence, inside its own drift
                    check_int_avgw(got, x, min(w, n))
                else:
                    assert ex.same(got, want), (rid, name, n, off, ex.first_diff(got, want))
    for name in ("minw", "maxw"):                            # w == 0: the window never closes (the running form)
        x = ex.unary_column(dt, 70_001, 1100)
        assert ex.same(gpu.scan(ck.SCAN_NAMES[name], x, 0), oracle.scan(ck.SCAN_NAMES[name], x, 0)), name


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("n", SCAN_N)
def test_scan_prefix_and_shifts_floating(gpu, oracle, dt, n):
    for off in (0, 1):
        for sign in (1.0, -1.0):                             # mins over a column that starts with +Inf, maxs over one that starts with -Inf
            x = inf_runs_column(dt, n, 1200 + n, sign)
            d = view(gpu, x, off)
            for name in ("mins", "maxs"):
                got, want = gpu.scan(ck.SCAN_NAMES[name], d), oracle.scan(ck.SCAN_NAMES[name], x)
                assert ex.same(got, want), (name, sign, off, ex.first_diff(got, want))
        y = ex.unary_column(dt, n, 1300 + n)                 # shifts: NaNs, both zeros, subnormals, infinities move as bits
        d = view(gpu, y, off)
        for name in ("deltas", "prev", "aggnext"):
            got, want = gpu.scan(ck.SCAN_NAMES[name], d), oracle.scan(ck.SCAN_NAMES[name], y)
            assert ex.same(got, want), (name, off, ex.first_diff(got, want))
        for cname, z in fp_columns(dt, n, 1400 + n):
            d = view(gpu, z, off)
            for name in ("sums", "avgs"):
                check_fp_sums(name, gpu.scan(ck.SCAN_NAMES[name], d), oracle.scan(ck.SCAN_NAMES[name], z), z)


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r[0])
def test_scan_windows_floating(gpu, oracle, dt, route):
    rid, w0, mm, sm = route
    for n in SCAN_N:
        w = n + 3 if w0 is None else w0
        for off in (0, 1):
            for sign in (1.0, -1.0):
                x = inf_runs_column(dt, n, 1500 + n, sign)
                d = view(gpu, x, off)
                for name in ("minw", "maxw"):
                    got, want = gpu.scan(ck.SCAN_NAMES[name], d, w), oracle.scan(ck.SCAN_NAMES[name], x, w)
                    assert ex.same(got, want), (rid, name, n, sign, off, ex.first_diff(got, want))
                for name in ("sumw", "avgw"):                # an Inf run enters the window; rows up to the reference's first NaN output
                    z = ex.sum_safe(x)
                    check_fp_sums(name, gpu.scan(ck.SCAN_NAMES[name], view(gpu, z, off), w), oracle.scan(ck.SCAN_NAMES[name], z, w), z, min(w, n), sum_route(dt, n, w))
            y = ex.unary_column(dt, n, 1600 + n)             # ratiow: x / 0, 0 / 0, NaN operands
            got, want = gpu.scan(ck.SCAN_RATIOW, view(gpu, y, off), w), oracle.scan(ck.SCAN_RATIOW, y, w)
            assert ex.same(got, want), (rid, "ratiow", n, off, ex.first_diff(got, want))
            z = fp_columns(dt, n, 1700 + n)[0][1]            # finite everywhere: every row of sumw / avgw is checked
            for name in ("sumw", "avgw"):
                check_fp_sums(name, gpu.scan(ck.SCAN_NAMES[name], view(gpu, z, off), w), oracle.scan(ck.SCAN_NAMES[name], z, w), z, min(w, n), sum_route(dt, n, w))
    for name in ("minw", "maxw"):
        for sign in (1.0, -1.0):
            x = inf_runs_column(dt, 70_001, 1800, sign)
            assert ex.same(gpu.scan(ck.SCAN_NAMES[name], x, 0), oracle.scan(ck.SCAN_NAMES[name], x, 0)), (name, sign)


def test_scan_window_zero_is_rejected(gpu):
    import aquery2_amd
    for name in ("sumw", "avgw"):
        with pytest.raises(aquery2_amd.AqgError):
            gpu.scan(ck.SCAN_NAMES[name], np.arange(10, dtype=np.int32), 0)


# ---- NaN rows ----------------------------------------------------------------------------------------------------------------------------
NAN_N = 3_000_001


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
@pytest.mark.parametrize("where", ["three", "last"])
def test_nan_rows_in_order_dependent_operations(gpu, oracle, dt, where):
    """NaNs at rows 5000, 70 000 and n - 1 (or at the last row only) of 3 000 001 rows: every output row strictly before the first NaN row is
    held to the usual standards, the calls succeed (what comes back behind a NaN is unspecified: DESIGN.md section 2 records what was measured)."""
    x = ex.sum_safe(ex.one_sign_zeros(ex.unary_column(dt, NAN_N, 1900, nan=False, inf=False)))
    rows = [5000, 70_000, NAN_N - 1] if where == "three" else [NAN_N - 1]
    x[rows] = np.nan
    first = rows[0]
    d = gpu.to_device(x)
    for name, w in [("mins", 0), ("maxs", 0), ("sums", 0), ("avgs", 0)] + [(nm_, w) for nm_ in ("minw", "maxw", "sumw", "avgw") for w in (5, 1000, 50_000, NAN_N)]:
        got, want = gpu.scan(ck.SCAN_NAMES[name], d, w), oracle.scan(ck.SCAN_NAMES[name], x, w)
        if name in ("mins", "maxs", "minw", "maxw"):
            assert ex.same(got[:first], want[:first]), (name, w, ex.first_diff(got[:first], want[:first]))
        else:
            check_fp_sums(name, got[:first], want[:first], x[:first], min(w, NAN_N) if w else None, sum_route(dt, NAN_N, w) if w else None)
    for name in ("sum", "avg", "min", "max"):
        gpu.reduce(ck.RED_NAMES[name], d)


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_nan_rows_where_they_are_in_scope(gpu, oracle, dt):
    """first / last and the shifts move NaNs as they are; ratios divides them (NaN where the reference has NaN)"""
    x = ex.unary_column(dt, 100_003, 2000)
    x[[0, 5000, 70_000, len(x) - 1]] = np.nan
    for name in ("first", "last"):
        assert ex.same(np.asarray(gpu.reduce(ck.RED_NAMES[name], x)), np.asarray(oracle.reduce(ck.RED_NAMES[name], x))), name
    for name, w in (("deltas", 0), ("prev", 0), ("aggnext", 0), ("ratiow", 1), ("ratiow", 7)):
        got, want = gpu.scan(ck.SCAN_NAMES[name], x, w), oracle.scan(ck.SCAN_NAMES[name], x, w)
        assert ex.same(got, want), (name, w, ex.first_diff(got, want))


# ---- per-group scans ------------------------------------------------------------------------------------------------------------------------
def test_grouped_scan_at_the_extremes(gpu, oracle):
    """the same full-range integer columns and +-Inf columns under a 1000-group key: sums, avgs, mins, maxs, minw, maxw, sumw against the
    oracle's scan of every group's rows (w == 0: the window never closes -- the running form without a seed)"""
    n, G = 70_001, 1000
    rng = np.random.default_rng(2100)
    keys = rng.integers(0, G, n).astype(np.int32)
    keys[: n // 3] = keys[0]                                 # one long group: its scan crosses many tiles
    ogb = oracle.groupby([keys])
    gb = gpu.groupby_build([keys])
    assert gb.ngroups == ogb["ngroups"]

    def both(name, x, w):
        op = ck.SCAN_NAMES[name]
        ot = ck.TAG2NP[oracle.scan_out_dtype(op, ex.tag(x.dtype))]
        return gpu.grouped_scan(gb, op, x, w), compose(ogb, x, lambda v: oracle.scan(op, v, w), ot)

    for dt in ex.INT_DTYPES:
        x = ex.unary_column(dt, n, 2200)
        for name, w in (("sums", 0), ("avgs", 0), ("mins", 0), ("maxs", 0), ("minw", 3), ("maxw", 100), ("minw", 0), ("maxw", 0), ("sumw", 5), ("sumw", 100)):
            got, want = both(name, x, w)
            assert ex.same(got, want), (ex.nm(dt), name, w, ex.first_diff(got, want))
    for dt in ex.FP_DTYPES:
        for sign in (1.0, -1.0):
            x = ex.one_sign_zeros(ex.unary_column(dt, n, 2300, nan=False, inf=False))
            x[rng.random(n) < 0.15] = dt.type(sign * np.inf)
            x[rng.random(n) < 0.05] = dt.type(-sign * np.inf)
            for name, w in (("mins", 0), ("maxs", 0), ("minw", 3), ("maxw", 100), ("minw", 0), ("maxw", 0), ("minw", n), ("maxw", n)):
                got, want = both(name, x, w)
                assert ex.same(got, want), (ex.nm(dt), sign, name, w, ex.first_diff(got, want))
        z = fp_columns(dt, n, 2400)[0][1]
        absz = compose(ogb, np.abs(z.astype(np.float64)), np.cumsum, np.float64)
        pos = compose(ogb, np.ones(n), np.cumsum, np.float64)
        for name, w in (("sums", 0), ("sumw", 5), ("sumw", 100)):
            got, want = both(name, z, w)
            assert np.all(np.abs(got - want) <= pos * 2.0 ** -52 * absz), (ex.nm(dt), name, w)      # the oracle's recurrence has touched the group's earlier rows
        # a window's rows are the window's: against the sum of the rows the route adds, per group -- w = 5 the window itself (direct route), w = 100 the
        # group's rows inside the tile and its halo (window_sum_kernel over by_group restarts its prefix at every group start): at most 2048 + 104 of them
        trail = lambda a, k: np.lib.stride_tricks.sliding_window_view(np.concatenate([np.zeros(k - 1), a]), k).sum(axis=1)
        for w, span in ((5, 5), (100, TS + 104)):
            got = gpu.grouped_scan(gb, ck.SCAN_SUMW, z, w)
            ref = compose(ogb, z.astype(np.float64), lambda v: trail(v, w), np.float64)
            rb = span * 2.0 ** -52 * compose(ogb, np.abs(z.astype(np.float64)), lambda v: trail(v, span), np.float64)
            bad = ~(np.abs(got - ref) <= rb)
            assert not bad.any(), (ex.nm(dt), w, int(np.nonzero(bad)[0][0]))
    gb.destroy()
