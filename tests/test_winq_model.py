"""tests/winq_model.py held to a brute-force sorted() of every window on tiny inputs of every dtype, to the recorded answers of pandas
rolling().quantile() (tests/golden/winq_pandas_rolling.json) and to tests/quantile_model.py where a window covers its slice; the kernel's
rule (rank tracking: csrc/window_quantile.hip) restated in numpy and held to the model with one writer per output; and the case list
of the GPU test (tests/winq_cases.py) held to the mistakes a kernel could make: for each, at least one of those cases refuses the wrong
answer.

One planted mistake cannot be refused by any comparison the contract allows: an order with -0.0 below +0.0 returns the same VALUES
everywhere and another zero only where the window holds both, which the contract leaves open (the flagged slots).  Its test shows
exactly that, instead of a refusal."""
import itertools
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import extremes as ex
import quantile_model as qm
import winq_cases as wc
import winq_model as wm
from test_quantile_model import brute_sorted, tiny_inputs

TS = wc.DEFAULT_TS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "winq_pandas_rolling.json")


@pytest.mark.parametrize("dt", wc.DTYPES, ids=ex.nm)
def test_model_equals_brute_force(dt):
    rng = np.random.default_rng(17 + wc.DTYPES.index(dt))
    offsets = [0, 1, 3, 6, 10, 23]
    gid = np.repeat(np.arange(5), np.diff(offsets))
    for x in tiny_inputs(rng, dt):
        xm = wc.as_model(x)
        for w, g in itertools.product((1, 2, 3, 5, 13, 23, 40), (None, gid)):
            for nums, den in wc.QLISTS + [([0, 7, 3, 7], 7)]:
                for which in wc.WHICH:
                    out, flags = wm.windows(x, w, nums, den, which, gid=g)
                    assert out.shape == flags.shape == (len(nums), 23) and out.dtype == xm.dtype
                    for i in range(23):
                        s = 0 if g is None else offsets[g[i]]
                        sl = xm[max(s, i - w + 1):i + 1]
                        order = brute_sorted(sl)
                        for j, num in enumerate(nums):
                            f = Fraction(num * (len(sl) - 1), den)
                            want = sl[order[math.floor(f) if which == wm.SEL_LOWER else math.ceil(f)]]
                            assert wm.same(out[j, i], want, flags[j, i]), (ex.nm(dt), w, nums, den, which, i, j)
                            if dt.kind != "f":
                                assert not flags.any() and out[j, i].tobytes() == want.tobytes()


def golden_cases():
    """(x, by or None, {(w, num, den, which): per-row answers}) of the recorded pandas answers"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    for c in doc["cases"]:
        x = np.array(c["x"], dtype=doc["dtype"])
        by = None if c["by"] is None else np.array(c["by"], dtype=np.int32)
        answers = {}
        for k, v in c["answers"].items():
            w, num, den, interp = k.split("_")
            answers[(int(w), int(num), int(den), {"lower": wm.SEL_LOWER, "higher": wm.SEL_UPPER}[interp])] = np.array(v, dtype=x.dtype)
        yield x, by, answers


def test_model_equals_pandas_rolling_quantile():
    seen = 0
    for x, by, answers in golden_cases():
        if by is None:
            order, gid = np.arange(len(x)), None
        else:
            order = np.argsort(by, kind="stable")               # every group's rows adjacent, in row order
            gid = by[order]
        for (w, num, den, which), want in answers.items():
            out, flags = wm.windows(x[order], w, [num], den, which, gid=gid)
            assert not flags.any()
            got = np.empty_like(want)
            got[order] = out[0]
            assert got.tobytes() == want.tobytes(), (w, num, den, which)
            seen += 1
    assert seen == 3 * 6 * 7 * 2


@pytest.mark.parametrize("dt", wc.DTYPES, ids=ex.nm)
def test_a_window_that_covers_its_slice_is_the_quantile_of_the_slice(dt):
    rng = np.random.default_rng(60 + wc.DTYPES.index(dt))
    n = 900
    gid = np.sort(rng.integers(0, 40, n))
    gid = np.unique(gid, return_inverse=True)[1].reshape(-1)
    G = int(gid.max()) + 1
    last = np.concatenate([np.nonzero(np.diff(gid))[0], [n - 1]])
    x = ex.full_range(rng, dt, n)
    for nums, den in wc.QLISTS:
        for which in wc.WHICH:
            want, wflags = qm.grouped(x, gid, G, nums, den, which)
            out, flags = wm.windows(x, n, nums, den, which, gid=gid)
            assert out[:, last].T.tobytes() == want.tobytes() and np.array_equal(flags[:, last].T, wflags)
            want1, _ = qm.flat(x, nums, den, which)
            assert wm.windows(x, n + 5, nums, den, which)[0][:, -1].tobytes() == want1.tobytes()
    assert wm.windows(x, 1, [0, 1, 2], 2)[0].tobytes() == np.tile(wc.as_model(x), 3).tobytes(), "w == 1 returns the input"


# ---- the kernel's rule, restated ---------------------------------------------------------------------------------------------------------------
def track(x, w, nums, den, which, gid=None, ts=TS, leave_strict=False, enter_le=False):
    """csrc/window_quantile.hip in numpy: a tile owns outputs [t0, t1); every row a of the tile and of the w - 1 rows in front of it is
    followed through the outputs of the tile whose window holds it -- the rank counted once, then moved by the row that enters and the
    row that leaves -- and writes its element where the rank is asked for.  Returns (out[nq][n], writers[nq][n]).
    leave_strict / enter_le: the two comparisons, planted wrong."""
    xm = wc.as_model(np.asarray(x))
    n, nq = len(xm), len(nums)
    img = wm.image(xm)
    ln = np.minimum(np.arange(n) - wm.slice_starts(n, gid) + 1, w)
    R = np.array([[qm.rank(num, den, c, which) for num in nums] for c in range(1, w + 1)], dtype=np.int64).reshape(w, nq)
    out, writers = np.zeros((nq, n), xm.dtype), np.zeros((nq, n), np.int64)
    for t0 in range(0, n, ts):
        t1 = min(t0 + ts, n)
        a = np.arange(max(t0 - (w - 1), 0), t1)
        q = np.maximum(a, t0)
        l = ln[q]
        keep = q - a < l
        a, q, l = a[keep], q[keep], l[keep]
        rank = np.zeros(len(a), np.int64)
        for k in range(w):                                     # the window of q, oldest row last
            b = q - k
            inside = (k < l) & (b != a)
            bb = np.where(inside, b, 0)
            rank += inside & np.where(bb < a, img[bb] <= img[a], img[bb] < img[a])
        while len(a):
            for j in range(nq):
                m = rank == R[l - 1, j]
                out[j, q[m]] = xm[a[m]]
                np.add.at(writers[j], q[m], 1)
            q2 = q + 1
            nl = ln[np.minimum(q2, n - 1)]
            alive = (q2 < t1) & (q2 - a < nl)
            qq = np.minimum(q2, n - 1)
            rank = rank + ((img[qq] <= img[a]) if enter_le else (img[qq] < img[a]))
            old = np.maximum(q2 - w, 0)
            rank = rank - ((l == w) & ((img[old] < img[a]) if leave_strict else (img[old] <= img[a])))
            a, q, l, rank = a[alive], q2[alive], nl[alive], rank[alive]
    return out, writers


def small_cases():
    """(x, w, gid, ts): inputs with many ties, several tiles, groups shorter and longer than the window"""
    rng = np.random.default_rng(3)
    for dt, n, w, ts in ((np.int32, 300, 7, 16), (np.float64, 257, 16, 64), (np.uint8, 400, 33, 32), (np.int16, 90, 1, 8), (np.int64, 200, 64, 64)):
        x = rng.integers(0, 6, n).astype(dt)
        yield x, w, None, ts
        yield x, w, np.sort(rng.integers(0, 12, n)), ts
        yield ex.full_range(rng, np.dtype(dt), n), w, np.sort(rng.integers(0, 40, n)), ts


def test_rank_tracking_is_the_model_with_one_writer_per_output():
    for x, w, gid, ts in small_cases():
        for (nums, den), which in itertools.product(wc.QLISTS, wc.WHICH):
            want, flags = wm.windows(x, w, nums, den, which, gid=gid)
            got, writers = track(x, w, nums, den, which, gid=gid, ts=ts)
            assert not flags.any() and got.tobytes() == want.tobytes(), (x.dtype, w, ts, nums, which)
            assert np.all(writers == 1)
    lay = wc.edges_layout(65, TS)
    x = wc.edges_column(lay, np.dtype(np.int32), np.random.default_rng(1))
    got, writers = track(x, 65, [1, 0, 2], 2, wm.SEL_UPPER, gid=lay.gid)
    assert got.tobytes() == wm.windows(x, 65, [1, 0, 2], 2, wm.SEL_UPPER, gid=lay.gid)[0].tobytes() and np.all(writers == 1)


# ---- planted mistakes: the model (or the restated kernel) with one thing wrong -> what a wrong kernel would have returned ------------------------
def image_zeros_apart(x):
    """mistake 9: -0.0 below +0.0"""
    im = wm.image(x)
    x = np.asarray(x)
    if x.dtype.kind == "f":
        im = im.copy()
        im[(x == 0) & np.signbit(x)] -= 1                       # just below the zero's image: above every negative value
    return im


def image_nan_first(x):
    """mistake 10: NaN below -inf"""
    im = wm.image(x)
    x = np.asarray(x)
    if x.dtype.kind == "f":
        im = im.copy()
        im[np.isnan(x)] = 0
    return im


def mistaken(name, x, w, gid, nums, den, which):
    if name == "window [i - w, i - 1]":
        return wm.Windows(x, w, gid, shift=1).quantiles(nums, den, which)[0]
    if name == "window not clamped at the group start":
        return wm.Windows(x, w, gid, clamp=False).quantiles(nums, den, which)[0]
    if name == "rank from w instead of len":
        return wm.Windows(x, w, gid).quantiles(nums, den, which, use_w=True)[0]
    if name == "leaving row compared with <":
        return track(x, w, nums, den, which, gid=gid, leave_strict=True)[0]
    if name == "entering row compared with <=":
        return track(x, w, nums, den, which, gid=gid, enter_le=True)[0]
    if name == "halo dropped at a tile edge":
        return wm.Windows(x, w, gid, tile=TS).quantiles(nums, den, which)[0]
    if name == "LOWER and UPPER swapped":
        return wm.Windows(x, w, gid).quantiles(nums, den, 1 - which)[0]
    if name == "planes transposed":
        out = wm.Windows(x, w, gid).quantiles(nums, den, which)[0]
        return np.ascontiguousarray(out.T).reshape(out.shape)
    if name == "-0.0 below +0.0":
        return wm.Windows(x, w, gid, image_fn=image_zeros_apart).quantiles(nums, den, which)[0]
    if name == "NaN below -inf":
        return wm.Windows(x, w, gid, image_fn=image_nan_first).quantiles(nums, den, which)[0]
    raise KeyError(name)


MISTAKES = ["window [i - w, i - 1]", "window not clamped at the group start", "rank from w instead of len", "leaving row compared with <",
            "entering row compared with <=", "halo dropped at a tile edge", "LOWER and UPPER swapped", "planes transposed", "NaN below -inf"]


def gpu_cases():
    """(x in flat order, w, gid) of the GPU test, the cheap ones first: the mixed zeros and NaNs, the grouped layouts, the flat grid"""
    for dt in ex.FP_DTYPES:
        x = wc.mixed_column(dt, 300)
        for w in (3, 64):
            yield x, w, None
            yield x, w, np.repeat(np.arange(6), 50)
    i32 = np.dtype(np.int32)
    for w in (2, 8):
        for lay, x in wc.grouped_cases(w, TS, i32):
            yield x, w, lay.gid
    for w, n, name, col, shift in wc.flat_grid(i32, TS, ws=(2, 3, 8)):
        yield col, w, None


@pytest.mark.parametrize("name", MISTAKES)
def test_the_gpu_cases_refuse(name):
    """the comparison the GPU test makes (wm.same against the model under its flags) over the GPU test's own cases and quantile lists:
    some case refuses the mistaken answer"""
    for x, w, gid in gpu_cases():
        s = wm.Windows(x, w, gid)
        for (nums, den), which in itertools.product(wc.QLISTS, wc.WHICH):
            out, flags = s.quantiles(nums, den, which)
            assert wm.same(out, out.copy(), flags)
            if not wm.same(mistaken(name, x, w, gid, nums, den, which), out, flags):
                return
    pytest.fail(f"no case refuses: {name}")


def test_zeros_apart_is_invisible_by_contract():
    """mistake 9, -0.0 below +0.0: a total order that agrees with the contract's on every VALUE.  Its answers differ from the model's in
    bits -- the mistake is real -- but only in the slots the model flags (the rank lands on a zero of a window that holds both zeros),
    and there by the zero's sign alone; the contract leaves that open, so no comparison may refuse it"""
    differs = 0
    for dt in ex.FP_DTYPES:
        x = wc.mixed_column(dt, 300)
        u = np.uint32 if dt.itemsize == 4 else np.uint64
        for w, gid in itertools.product((3, 64), (None, np.repeat(np.arange(6), 50))):
            for (nums, den), which in itertools.product(wc.QLISTS, wc.WHICH):
                out, flags = wm.windows(x, w, nums, den, which, gid=gid)
                bad = mistaken("-0.0 below +0.0", x, w, gid, nums, den, which)
                diff = bad.view(u) != out.view(u)
                assert not (diff & ~flags).any() and np.all(bad[diff] == 0) and np.all(out[diff] == 0)
                assert wm.same(bad, out, flags)
                differs += int(diff.sum())
    assert differs > 0


def test_general_cases_flag_nothing():
    for dt in (np.dtype(np.float32), np.dtype(np.float64)):
        for w, n, name, col, shift in wc.flat_grid(dt, TS, ws=(8,)):
            assert not wm.windows(col, w, [0, 1, 2], 2)[1].any(), (name, n)
    x = wc.mixed_column(np.dtype(np.float64), 300)
    assert wm.windows(x, 8, [0, 1, 2], 2)[1].mean() > 0.2
