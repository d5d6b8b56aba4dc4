"""tests/topk_model.py held to a brute-force sorted() on tiny inputs of every dtype, and its `check` held to the corruptions a kernel
could produce: each must be refused, and the model's own answer (and any other valid choice among tied rows) accepted."""
import functools
import math

import numpy as np
import pytest

import extremes as ex
import topk_model as tk

DTYPES = ex.NUM_DTYPES + [np.dtype(np.bool_)]
ORDERS = (tk.ORDER_ASC, tk.ORDER_DESC)


def brute(x, offsets, k, order):
    """positions of the first min(k, c) rows of every group under Python's own comparisons: NaN above everything, zeros equal, ties by
    ascending position"""
    def cmp(a, b):
        (va, pa), (vb, pb) = a, b
        na, nb = isinstance(va, float) and math.isnan(va), isinstance(vb, float) and math.isnan(vb)
        c = (na > nb) - (na < nb) if (na or nb) else (va > vb) - (va < vb)
        if order == tk.ORDER_DESC:
            c = -c
        return c if c else (pa > pb) - (pa < pb)
    out = []
    for g in range(len(offsets) - 1):
        rows = [(x[p].item(), p) for p in range(offsets[g], offsets[g + 1])]
        out.append([p for _, p in sorted(rows, key=functools.cmp_to_key(cmp))[:k]])
    return out


def tiny_inputs(rng, dt):
    yield ex.full_range(rng, dt, 23)
    yield rng.choice(ex.full_range(rng, dt, 3), 23)
    yield np.repeat(ex.full_range(rng, dt, 1), 23)
    if dt.kind == "f":
        pool = np.array([0.0, -0.0, np.nan, ex._neg_nan(dt), np.inf, -np.inf, 1.5, -1.5], dtype=dt)
        yield pool[rng.integers(0, len(pool), 23)]


@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
def test_model_equals_brute_force(dt):
    rng = np.random.default_rng(7 + DTYPES.index(dt))
    offsets = np.array([0, 1, 3, 3, 10, 23])
    for x in tiny_inputs(rng, dt):
        xm = x.astype(np.uint8) if dt == np.bool_ else x
        for order in ORDERS:
            for k in (1, 2, 3, 7, 13, 30):
                vals, pos, flags = tk.topk(x, offsets, k, order)
                want = brute(xm, offsets, k, order)
                for g, w in enumerate(want):
                    assert pos[g, :len(w)].tolist() == w, (ex.nm(dt), order, k, g)
                    assert np.all(pos[g, len(w):] == tk.MISSING) and not vals[g, len(w):].view(np.uint8).any()
                    assert vals[g, :len(w)].tobytes() == xm[w].tobytes()
                tk.check(vals, pos, x, offsets, k, order)
                tk.check(vals, None, x, offsets, k, order)
                if dt.kind != "f":
                    assert not flags.any()


def test_flags_mark_nans_and_mixed_zeros_only():
    x = np.array([0.0, -0.0, 1.0, np.nan, -0.0, -0.0, 2.0, 3.0], np.float32)
    vals, pos, flags = tk.topk(x, [0, 4, 8], 3, tk.ORDER_DESC)
    assert pos.tolist() == [[3, 2, 0], [7, 6, 4]]
    assert flags.tolist() == [[True, False, True], [False, False, False]]       # group 1 holds only -0.0: bit for bit
    assert np.signbit(vals[1, 2])


def refused(vals, pos, x, offsets, k, order):
    with pytest.raises(AssertionError):
        tk.check(vals, pos, x, offsets, k, order)
    return True


def test_check_refuses_every_corruption():
    #                  group 0: 7 rows, five tie on the top value 9      group 1: 2 rows
    x = np.array([9, 1, 9, 9, 5, 9, 9, 4, 8], np.int32)
    off, k, order = [0, 7, 9], 3, tk.ORDER_DESC
    vals, pos, _ = tk.topk(x, off, k, order)
    assert pos.tolist() == [[0, 2, 3], [8, 7, 0xFFFFFFFF]]
    tk.check(vals, pos, x, off, k, order)

    def variant(**slots):
        v, p = vals.copy(), pos.copy()
        for name, new in slots.items():
            g, j = int(name[1]), int(name[2])
            p[g, j] = new
            if new != 0xFFFFFFFF:
                v[g, j] = x[new]
        return v, p
    # another valid choice among the tied rows is accepted
    tk.check(*variant(s01=3, s02=6), x, off, k, order)
    # a dropped tie replaced by a smaller value
    assert refused(*variant(s02=4), x, off, k, order)
    # a duplicated position
    assert refused(*variant(s01=0), x, off, k, order)
    assert refused(*variant(s02=2), x, off, k, order)
    # a position from the neighbouring group
    assert refused(*variant(s02=8), x, off, k, order)
    assert refused(*variant(s11=6), x, off, k, order)
    # equal images with descending positions
    assert refused(*variant(s01=5, s02=2), x, off, k, order)
    # a non-zero padding slot, in the values and in the positions
    v, p = vals.copy(), pos.copy()
    v[1, 2] = 1
    assert refused(v, p, x, off, k, order)
    assert refused(v, None, x, off, k, order)
    v, p = vals.copy(), pos.copy()
    p[1, 2] = 7
    assert refused(v, p, x, off, k, order)
    # a value that is not bitwise the element at its position
    v, p = vals.copy(), pos.copy()
    v[0, 1] = 8
    assert refused(v, p, x, off, k, order)
    xf = np.array([0.0, -0.0, -1.0], np.float64)
    vf, pf, ff = tk.topk(xf, [0, 3], 2, tk.ORDER_DESC)
    assert pf.tolist() == [[0, 1]] and ff.all()
    tk.check(vf, pf, xf, [0, 3], 2, tk.ORDER_DESC)
    vf[0, 1] = 0.0                                                              # +0.0 where position 1 holds -0.0
    assert refused(vf, pf, xf, [0, 3], 2, tk.ORDER_DESC)
    # wrong order of the slots, a missing row marked as padding, the wrong dtype
    assert refused(*variant(s10=7, s11=8), x, off, k, order)
    assert refused(*variant(s02=0xFFFFFFFF), x, off, k, order)
    assert refused(vals.astype(np.int64), pos, x, off, k, order)
    # without positions the values alone are held to the model
    v = vals.copy()
    v[0, 2] = 5
    assert refused(v, None, x, off, k, order)
    tk.check(vals, None, x, off, k, order)


def test_full_range_inputs_leave_no_flagged_slot():
    """the seeded GPU cases assert this before the device is asked"""
    rng = np.random.default_rng(11)
    for dt in DTYPES:
        x = ex.full_range(rng, dt, 5000)
        for order in ORDERS:
            assert not tk.topk(x, [0, 100, 100, 2500, 5000], 64, order)[2].any()
