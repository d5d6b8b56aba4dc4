"""The window join (aqg_join_window_bounds, aqg_interval_fold, aqg_join_window, aqg_join_window_last) against its model
(tests/wj_model.py; tests/test_wj_model.py holds that model to its brute-force form and to recorded answers of pandas).  Everything
goes through the C-ABI and every call writes between canary words.  The order, the bounds, counts, integer sums / averages and
min / max are exact; floating sums and averages meet the bound m u / (1 - m u) sum|x| of include/aqg.h on finite windows and come
out in the specified non-finite class elsewhere.  The worst observed share of that bound is printed."""
import ctypes as C
import functools

import numpy as np
import pytest

import asof_model as am
import checker as ck
import timewin_model as tm
import wj_cases
import wj_model as wm

pytestmark = pytest.mark.gpu
AQG_OK, AQG_ERR_DTYPE, AQG_ERR_ARG = 0, 2, 3
CANARY = 0xA5
OPS = (wm.COUNT, wm.SUM, wm.AVG, wm.MIN, wm.MAX)
FILL = 77
WORST = {"share": 0.0}
CASE_FLAGS = [(n, f) for n in sorted(wj_cases.cases()) for f in wj_cases.cases()[n].flags]


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    print("worst |got - exact| / bound of a floating sum or average in this module: %.3g" % WORST["share"])
    d.close()


# ---- calls between canaries -----------------------------------------------------------------------------------------------------------
class Out:
    """`n` elements of `dtype` inside a device allocation filled with canary bytes, `pad` elements on either side"""

    def __init__(self, gpu, n, dtype, pad=4):
        self.dtype, self.n, self.pad = np.dtype(dtype), n, pad
        self.buf = gpu.to_device(np.full((n + 2 * pad) * self.dtype.itemsize, CANARY, np.uint8))
        self.ptr = self.buf.ptr + pad * self.dtype.itemsize

    def read(self):
        """(the n elements, the canaries around them are intact)"""
        raw = self.buf.to_host()
        w, a = self.dtype.itemsize, self.pad * self.dtype.itemsize
        body = raw[a:a + self.n * w]
        return body.view(self.dtype).copy(), bool((raw[:a] == CANARY).all() and (raw[a + self.n * w:] == CANARY).all())

    def untouched(self):
        return bool((self.buf.to_host() == CANARY).all())


class Sides:
    """the columns of a case on the device, every one starting `shift` elements into its allocation"""

    def __init__(self, gpu, c, shift=0):
        self.keep = []

        def up(a):
            a = np.ascontiguousarray(a)
            buf = gpu.to_device(np.concatenate([np.zeros(shift, a.dtype), a]))
            self.keep.append(buf)
            return buf.ptr + shift * a.dtype.itemsize
        nk = len(c.bk)
        self.nk = nk
        self.dts = (C.c_int * max(1, nk))(*[t for t, _ in c.bk]) if nk else None
        self.bp = (C.c_void_p * max(1, nk))(*[up(a) for _, a in c.bk]) if nk else None
        self.pp = (C.c_void_p * max(1, nk))(*[up(a) for _, a in c.pk]) if nk else None
        self.bo, self.po, self.x = up(c.bo), up(c.po), up(c.x)
        self.nb, self.np, self.on_tag, self.x_tag = len(c.bo), len(c.po), ck.NP2TAG[np.asarray(c.bo).dtype], ck.NP2TAG[np.asarray(c.x).dtype]


def bounds_raw(gpu, s, c, flags, shift=0, **kw):
    """(status, order, lo, hi, canaries intact)"""
    order, lo, hi = Out(gpu, s.nb, np.uint32, 4 + shift), Out(gpu, s.np, np.uint32, 4 + shift), Out(gpu, s.np, np.uint32, 4 + shift)
    rc = gpu.lib.aqg_join_window_bounds(gpu.ctx, flags, kw.get("nkeys", s.nk), s.dts, s.bp, s.bo, s.nb, s.pp, s.po, s.np, kw.get("on_tag", s.on_tag),
                                        kw.get("before", c.before), kw.get("after", c.after), order.ptr, lo.ptr, hi.ptr)
    (o, i0), (l, i1), (h, i2) = order.read(), lo.read(), hi.read()
    return rc, o, l, h, i0 and i1 and i2


def out_dtype(gpu, op, x):
    return ck.TAG2NP[gpu.lib.aqg_rangew_out_dtype(op, ck.NP2TAG[np.asarray(x).dtype])]


def fill_ptr(dtype, fill):
    if fill is None:
        return None, None
    f = np.zeros(1, dtype)
    if dtype.names:
        f["lo"] = fill
    else:
        f[0] = fill
    return f, f.ctypes.data


def join_raw(gpu, s, c, op, flags, fill=FILL, shift=0, **kw):
    """(status, the np results, canaries intact)"""
    out = Out(gpu, s.np, out_dtype(gpu, op, c.x), 4 + shift)
    f, fp = fill_ptr(out.dtype, fill)
    rc = gpu.lib.aqg_join_window(gpu.ctx, kw.get("bad_op", op), flags, kw.get("nkeys", s.nk), s.dts, s.bp, s.bo, s.nb, s.pp, s.po, s.np, kw.get("on_tag", s.on_tag),
                                 kw.get("before", c.before), kw.get("after", c.after), kw.get("x_tag", s.x_tag), s.x, fp, out.ptr)
    got, intact = out.read()
    return rc, got, intact


def fold_raw(gpu, op, x, lo, hi, fill=FILL, shift=0, xd=None, ld=None, hd=None):
    x = np.asarray(x)
    keep = [gpu.to_device(np.concatenate([np.zeros(shift, a.dtype), a])) if d is None else d for a, d in ((x, xd), (lo, ld), (hi, hd))]
    ptr = [k.ptr + (shift * a.dtype.itemsize if d is None else 0) for k, a, d in zip(keep, (x, lo, hi), (xd, ld, hd))]
    out = Out(gpu, len(lo), out_dtype(gpu, op, x), 4 + shift)
    f, fp = fill_ptr(out.dtype, fill)
    rc = gpu.lib.aqg_interval_fold(gpu.ctx, op, ck.NP2TAG[x.dtype], ptr[0], len(x), ptr[1], ptr[2], len(lo), fp, out.ptr)
    gpu.sync()
    got, intact = out.read()
    return rc, got, intact


# ---- what an answer is held to ----------------------------------------------------------------------------------------------------------
def hold(x, ref, op, got, fill, what):
    """one aggregate of every interval against the exact aggregates ref = (nonempty, windows) of wj_model.interval_windows"""
    ne, w = ref
    isf = np.asarray(x).dtype.kind == "f"
    fv = np.zeros(1, got.dtype)
    if fill is not None and not got.dtype.names:
        fv[0] = fill
    if op == wm.COUNT:
        want = np.zeros(len(ne), np.uint32)
        want[ne] = w.len
        assert got.dtype == np.uint32 and np.array_equal(got, want), what
        return
    empty = got[~ne]
    if op == wm.SUM:
        assert empty.tobytes() == bytes(empty.nbytes), (what, "an empty window's sum is not zero")
    else:
        assert empty.tobytes() == np.repeat(fv, len(empty)).tobytes(), (what, "an empty window is not the fill")
    got = got[ne]
    if op == wm.SUM and not isf:
        ex = tm.exact_int_sum(w)
        assert np.array_equal(got["lo"], ex["lo"]) and np.array_equal(got["hi"].view(np.uint64), ex["hi"]), what
    elif op == wm.AVG and not isf:
        assert got.dtype == np.float64 and np.array_equal(got, tm.exact_int_avg(w)), what
    elif op in (wm.SUM, wm.AVG):
        assert got.dtype == np.float64, what
        share = tm.sum_share(w, got, avg=op == wm.AVG) if len(got) else 0.0
        WORST["share"] = max(WORST["share"], share)
        print("%s: worst |got - exact| / bound = %.3g" % (what, share))
        assert share <= 1.0, what
    else:
        r = w.mn if op == wm.MIN else w.mx
        ok = w.nnan == 0
        assert got.dtype == r.dtype and np.array_equal(got[ok], r[ok]), what          # (== : either zero passes)


def check_bounds(c, flags, order, lo, hi, what):
    """order: a permutation of the build rows; order[lo_i:hi_i] the model's rows of probe i element by element"""
    worder, wlo, whi = want_bounds(*what) if isinstance(what, tuple) else wm.window_bounds(c.bk, c.bo, c.pk, c.po, c.before, c.after, flags)
    assert np.array_equal(np.sort(order), np.arange(len(c.bo), dtype=np.uint32)), what
    assert np.array_equal(hi - lo, whi - wlo), what
    assert (hi <= len(c.bo)).all() and (lo <= hi).all(), what
    n = (hi - lo).astype(np.int64)
    pos = np.repeat(lo.astype(np.int64) - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
    wpos = np.repeat(wlo.astype(np.int64) - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
    assert np.array_equal(order[pos], worder[wpos]), what


@functools.lru_cache(maxsize=None)
def want_bounds(name, flags):
    c = wj_cases.cases()[name]
    return wm.window_bounds(c.bk, c.bo, c.pk, c.po, c.before, c.after, flags)


def groups_of(c):
    return am.group_ids(c.bk, len(c.bo), [], 0)[1] if c.bk else 1


def want_routes(c, op):
    r = wm.routes(c.bk, c.bo, len(c.po))
    if op != wm.COUNT:
        r |= wm.fold_route((np.asarray(c.x).dtype.itemsize, wm.acc_bytes(np.asarray(c.x).dtype, op)), len(c.bo), len(c.po))
    return r


def run_case(gpu, c, flags, what, shift=0, ops=OPS):
    s = Sides(gpu, c, shift)
    rc, order, lo, hi, intact = bounds_raw(gpu, s, c, flags, shift)
    assert rc == AQG_OK and intact, what
    check_bounds(c, flags, order, lo, hi, what)
    r, G, passes = gpu.join_window_last()
    assert r == wm.routes(c.bk, c.bo, len(c.po)) and G == groups_of(c), what
    if r & wm.PRESORTED:
        assert passes == am.sort_passes(c.bk, c.bo), what
    xs = np.asarray(c.x)[order]
    ref = wm.interval_windows(xs, lo, hi)
    gathered = gpu.gather(c.x, order)                                            # aqg_gather(x, order_out) materialises the build rows
    assert gathered.tobytes() == xs.tobytes(), what
    xd = gpu.to_device(gathered)
    ld, hd = gpu.to_device(lo), gpu.to_device(hi)
    for op in ops:
        rc, got, intact = join_raw(gpu, s, c, op, flags, shift=shift)
        assert rc == AQG_OK and intact, (what, op)
        hold(xs, ref, op, got, FILL, "%s/op%d" % (what, op))
        assert gpu.join_window_last() == (want_routes(c, op), G, passes), (what, op)
        rc, parts, intact = fold_raw(gpu, op, xs, lo, hi, xd=xd, ld=ld, hd=hd)
        assert rc == AQG_OK and intact and parts.tobytes() == got.tobytes(), (what, op, "aqg_join_window is not bounds + aqg_gather + fold")
        rc, again, intact = join_raw(gpu, s, c, op, flags, shift=shift)
        assert rc == AQG_OK and intact and again.tobytes() == got.tobytes(), (what, op, "two calls differ")


# ---- every named case under its flag combinations ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", CASE_FLAGS, ids=["%s-f%d" % nf for nf in CASE_FLAGS])
def test_case_equals_model(gpu, name, flags):
    run_case(gpu, wj_cases.cases()[name], flags, (name, flags))


@pytest.mark.parametrize("shift", [1, 3])
@pytest.mark.parametrize("name", ["np_1", "np_2", "np_3", "np_5", "lds_i64", "lds_i32", "ends_int8", "nokeys", "d_eq_span_f32"])
def test_unaligned_device_offsets(gpu, name, shift):
    c = wj_cases.cases()[name]
    for flags in (0, wm.OPEN_LO | wm.OPEN_HI | wm.PREVAILING):
        run_case(gpu, c, flags, (name, flags), shift=shift, ops=(wm.SUM, wm.MAX))


# ---- the fold alone ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wj_cases.folds()))
def test_interval_fold(gpu, name):
    f = wj_cases.folds()[name]
    ref = wm.interval_windows(f.x, f.lo, f.hi)
    xd, ld, hd = gpu.to_device(f.x), gpu.to_device(f.lo), gpu.to_device(f.hi)
    for op in OPS:
        rc, got, intact = fold_raw(gpu, op, f.x, f.lo, f.hi, xd=xd, ld=ld, hd=hd)
        assert rc == AQG_OK and intact, (name, op)
        hold(f.x, ref, op, got, FILL, "fold/%s/op%d" % (name, op))
        route = 0 if op == wm.COUNT else wm.fold_route((f.x.dtype.itemsize, wm.acc_bytes(f.x.dtype, op)), len(f.x), len(f.lo))
        assert gpu.join_window_last() == (route, 0, 0), (name, op)
        rc, again, intact = fold_raw(gpu, op, f.x, f.lo, f.hi, xd=xd, ld=ld, hd=hd)
        assert rc == AQG_OK and again.tobytes() == got.tobytes(), (name, op, "two calls differ")
    rc, got, intact = fold_raw(gpu, wm.MIN, f.x, f.lo, f.hi, fill=None, shift=1)
    assert rc == AQG_OK and intact
    hold(f.x, ref, wm.MIN, got, None, "fold/%s/null fill" % name)


def test_both_fold_routes_ran_and_agree(gpu):
    """the STAGED and the INPLACE route combine the same operands in the same order: one column, the same intervals, the same bits"""
    f = wj_cases.folds()["staged_f64"]
    few = slice(0, 5000)
    for op in (wm.SUM, wm.AVG, wm.MIN):
        _, staged, _ = fold_raw(gpu, op, f.x, f.lo, f.hi)
        assert gpu.join_window_last()[0] == wm.FOLD_STAGED
        _, inplace, _ = fold_raw(gpu, op, f.x, f.lo[few], f.hi[few])
        assert gpu.join_window_last()[0] == wm.FOLD_INPLACE
        assert staged[few].tobytes() == inplace.tobytes()


# ---- the Python binding ------------------------------------------------------------------------------------------------------------------
def test_python_binding(gpu):
    from aquery2_amd import capi
    assert (capi.WJ_OPEN_LO, capi.WJ_OPEN_HI, capi.WJ_PREVAILING, capi.WJ_FOLD_STAGED, capi.WJ_FOLD_INPLACE) == (wm.OPEN_LO, wm.OPEN_HI, wm.PREVAILING, wm.FOLD_STAGED, wm.FOLD_INPLACE)
    c = wj_cases.cases()["group_sizes_f64x"]
    flags = capi.WJ_OPEN_LO | capi.WJ_PREVAILING
    bk, pk = [a for _, a in c.bk], [a for _, a in c.pk]
    order, lo, hi = gpu.join_window_bounds(bk, c.bo, pk, c.po, c.before, c.after, flags=flags)
    check_bounds(c, flags, order, lo, hi, "binding")
    xs = c.x[order]
    ref = wm.interval_windows(xs, lo, hi)
    for op in OPS:
        x = None if op == wm.COUNT else c.x
        got = gpu.join_window(op, bk, c.bo, pk, c.po, c.before, c.after, x=x, flags=flags, fill=FILL)
        hold(xs, ref, op, got, FILL, "binding/op%d" % op)
        assert gpu.join_window_last()[:2] == (want_routes(c, op), groups_of(c))
        parts = gpu.interval_fold(op, None if op == wm.COUNT else gpu.gather(c.x, order), lo, hi, fill=FILL)
        assert parts.tobytes() == got.tobytes()


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_fuzz(gpu, seed):
    c, flags = wj_cases.random_case(seed, 5000)
    if len(c.bo) == 0:
        s = Sides(gpu, c)
        rc, got, intact = join_raw(gpu, s, c, wm.MAX, flags)
        assert rc == AQG_OK and intact and (got == FILL).all() and gpu.join_window_last() == (0, 0, 0)
        return
    run_case(gpu, c, flags, "fuzz%d" % seed, shift=seed % 2, ops=(OPS[seed % 5], wm.SUM))


# ---- empty sides, errors ----------------------------------------------------------------------------------------------------------------
def test_empty_sides(gpu):
    c = wj_cases.cases()["absent_keys"]
    nobuild = c._replace(bk=[(t, a[:0]) for t, a in c.bk], bo=c.bo[:0], x=c.x[:0])
    noprobe = c._replace(pk=[(t, a[:0]) for t, a in c.pk], po=c.po[:0])
    for flags in (0, 7):
        s = Sides(gpu, nobuild)
        rc, order, lo, hi, intact = bounds_raw(gpu, s, nobuild, flags)
        assert rc == AQG_OK and intact and len(order) == 0 and not lo.any() and not hi.any() and gpu.join_window_last() == (0, 0, 0)
        for op in OPS:
            rc, got, intact = join_raw(gpu, s, nobuild, op, flags)
            assert rc == AQG_OK and intact and gpu.join_window_last() == (0, 0, 0)
            want = np.zeros(len(c.po), got.dtype)
            if op in (wm.AVG, wm.MIN, wm.MAX):
                want[:] = FILL
            assert got.tobytes() == want.tobytes(), op
        s = Sides(gpu, noprobe)
        rc, order, lo, hi, intact = bounds_raw(gpu, s, noprobe, flags)
        assert rc == AQG_OK and intact and len(lo) == 0 and (order.view(np.uint8) == CANARY).all() and gpu.join_window_last() == (0, 0, 0)
        rc, got, intact = join_raw(gpu, s, noprobe, wm.SUM, flags)
        assert rc == AQG_OK and intact and len(got) == 0
    # the fold over no rows, and over no queries
    z = np.zeros(0, np.uint32)
    rc, got, intact = fold_raw(gpu, wm.MAX, np.zeros(0, np.int16), np.array([0, 3], np.uint32), np.array([5, 9], np.uint32))
    assert rc == AQG_OK and intact and (got == FILL).all()
    rc, got, intact = fold_raw(gpu, wm.SUM, np.arange(5.0), z, z)
    assert rc == AQG_OK and intact and len(got) == 0


def test_error_returns_leave_the_outputs_untouched(gpu):
    c = wj_cases.cases()["absent_keys"]
    s = Sides(gpu, c)
    assert join_raw(gpu, s, c, wm.SUM, 0)[0] == AQG_OK                           # a call that leaves routes behind

    def refused(code, flags=0, **kw):
        rc, order, lo, hi, intact = bounds_raw(gpu, s, c, flags, **kw)
        assert rc == code and intact and all((a.view(np.uint8) == CANARY).all() for a in (order, lo, hi)), kw
        assert gpu.join_window_last() == (0, 0, 0)
        rc, got, intact = join_raw(gpu, s, c, wm.AVG, flags, **kw)
        assert rc == code and intact and (got.view(np.uint8) == CANARY).all(), kw
        assert gpu.join_window_last() == (0, 0, 0)
    refused(AQG_ERR_ARG, flags=8)
    refused(AQG_ERR_ARG, flags=-1)
    refused(AQG_ERR_ARG, before=-1.0)
    refused(AQG_ERR_ARG, after=-0.5)
    refused(AQG_ERR_ARG, before=float("nan"))
    refused(AQG_ERR_ARG, after=float("nan"))
    refused(AQG_ERR_ARG, flags=wm.OPEN_LO, before=0.0)
    refused(AQG_ERR_ARG, flags=wm.OPEN_HI, after=0.0)
    for tag in (ck.BOOL, ck.INT128, ck.UINT128, ck.DATE, ck.TIME, ck.TIMESTAMP, ck.STR):
        refused(AQG_ERR_DTYPE, on_tag=tag)
    refused(AQG_ERR_ARG, nkeys=9)
    refused(AQG_ERR_ARG, nkeys=-1)
    # the join's own: a bad op, a value dtype that is not numeric
    for kw, code in ((dict(bad_op=5), AQG_ERR_ARG), (dict(bad_op=-1), AQG_ERR_ARG), (dict(x_tag=ck.STR), AQG_ERR_DTYPE), (dict(x_tag=ck.INT128), AQG_ERR_DTYPE)):
        rc, got, intact = join_raw(gpu, s, c, wm.MIN, 0, **kw)
        assert rc == code and intact and (got.view(np.uint8) == CANARY).all() and gpu.join_window_last() == (0, 0, 0), kw
    # null columns with rows, and outputs over inputs or over each other
    nb, npr, tag = len(c.bo), len(c.po), ck.NP2TAG[c.bo.dtype]
    out = Out(gpu, nb + 2 * npr + 64, np.uint32)
    o, l, h = out.ptr, out.ptr + 4 * (nb + 16), out.ptr + 4 * (nb + npr + 32)
    bounds = lambda b, p, oo, ll, hh: gpu.lib.aqg_join_window_bounds(gpu.ctx, 0, 0, None, None, b, nb, None, p, npr, tag, 1.0, 1.0, oo, ll, hh)
    for args in ((None, s.po, o, l, h), (s.bo, None, o, l, h), (s.bo, s.po, None, l, h), (s.bo, s.po, o, None, h), (s.bo, s.po, o, l, None),
                 (s.bo, s.po, o, l, l), (s.bo, s.po, o, o, h), (s.bo, l, o, l, h), (o, s.po, o, l, h)):
        assert bounds(*args) == AQG_ERR_ARG, args
    join = lambda b, p, x, oo: gpu.lib.aqg_join_window(gpu.ctx, wm.MAX, 0, 0, None, None, b, nb, None, p, npr, tag, 1.0, 1.0, s.x_tag, x, None, oo)
    for args in ((None, s.po, s.x, o), (s.bo, None, s.x, o), (s.bo, s.po, None, o), (s.bo, s.po, s.x, None), (s.bo, s.po, o, o), (o, s.po, s.x, o)):
        assert join(*args) == AQG_ERR_ARG, args
    fold = lambda op, t, x, ll, hh, oo: gpu.lib.aqg_interval_fold(gpu.ctx, op, t, x, nb, ll, hh, npr, None, oo)
    zeros = gpu.to_device(np.zeros(npr, np.uint32))
    for args in ((5, s.x_tag, s.x, zeros.ptr, zeros.ptr, o), (wm.SUM, s.x_tag, None, zeros.ptr, zeros.ptr, o), (wm.SUM, s.x_tag, s.x, None, zeros.ptr, o),
                 (wm.SUM, s.x_tag, s.x, zeros.ptr, None, o), (wm.SUM, s.x_tag, s.x, zeros.ptr, zeros.ptr, None), (wm.MIN, s.x_tag, o, zeros.ptr, zeros.ptr, o),
                 (wm.COUNT, s.x_tag, s.x, o, zeros.ptr, o)):
        assert fold(*args) == AQG_ERR_ARG, args
    assert fold(wm.SUM, ck.STR, s.x, zeros.ptr, zeros.ptr, o) == AQG_ERR_DTYPE
    # more than AQG_MAX_ROWS rows on either side
    too_many = 0xFFFFFFFF
    assert gpu.lib.aqg_join_window_bounds(gpu.ctx, 0, 0, None, None, s.bo, too_many, None, s.po, npr, tag, 1.0, 1.0, o, l, h) == AQG_ERR_ARG
    assert gpu.lib.aqg_join_window(gpu.ctx, wm.MAX, 0, 0, None, None, s.bo, nb, None, s.po, too_many, tag, 1.0, 1.0, s.x_tag, s.x, None, o) == AQG_ERR_ARG
    assert gpu.lib.aqg_interval_fold(gpu.ctx, wm.SUM, s.x_tag, s.x, too_many, zeros.ptr, zeros.ptr, npr, None, o) == AQG_ERR_ARG
    assert gpu.lib.aqg_interval_fold(gpu.ctx, wm.SUM, s.x_tag, s.x, nb, zeros.ptr, zeros.ptr, too_many, None, o) == AQG_ERR_ARG
    gpu.sync()
    assert out.untouched() and gpu.join_window_last() == (0, 0, 0)
    assert bounds(s.bo, s.po, o, l, h) == AQG_OK
    got = out.buf.to_host().view(np.uint32)
    keyless = c._replace(bk=[], pk=[], before=1.0, after=1.0)
    check_bounds(keyless, 0, got[4:4 + nb], got[4 + nb + 16:4 + nb + 16 + npr], got[4 + nb + npr + 32:4 + nb + 2 * npr + 32], "after the refusals")
