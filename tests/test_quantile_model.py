"""tests/quantile_model.py held to a brute-force sorted() on tiny inputs of every dtype, to tests/median_model.py at 1/2, to min and max
at 0 and 1, its rank arithmetic to fractions.Fraction -- and the case list of the GPU test (tests/quantile_cases.py) held to the
corruptions a kernel could produce: for each, at least one of those cases refuses the corrupted answer."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import extremes as ex
import median_model as mm
import quantile_cases as qc
import quantile_model as qm

DTYPES = qc.DTYPES


def brute_sorted(col):
    """the rows of a slice under Python's own comparisons: NaN above everything, zeros equal, ties by position"""
    def cmp(a, b):
        (va, pa), (vb, pb) = a, b
        na, nb = isinstance(va, float) and math.isnan(va), isinstance(vb, float) and math.isnan(vb)
        c = (na > nb) - (na < nb) if (na or nb) else (va > vb) - (va < vb)
        return c if c else (pa > pb) - (pa < pb)
    return [p for _, p in sorted([(col[p].item(), p) for p in range(len(col))], key=functools.cmp_to_key(cmp))]


def tiny_inputs(rng, dt):
    yield ex.full_range(rng, dt, 23)
    yield rng.choice(ex.full_range(rng, dt, 3), 23)
    yield np.repeat(ex.full_range(rng, dt, 1), 23)
    if dt.kind == "f":
        pool = np.array([0.0, -0.0, np.nan, ex._neg_nan(dt), np.inf, -np.inf, 1.5, -1.5], dtype=dt)
        yield pool[rng.integers(0, len(pool), 23)]


@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
def test_model_equals_brute_force(dt):
    rng = np.random.default_rng(11 + DTYPES.index(dt))
    offsets = [0, 1, 3, 6, 10, 23]
    gid = np.repeat(np.arange(5), np.diff(offsets))
    for x in tiny_inputs(rng, dt):
        xm = qc.as_model(x)
        for nums, den in qc.QLISTS + [([0, 7, 3, 7], 7)]:
            for which in qc.WHICH:
                out, flags = qm.grouped(x, gid, 5, nums, den, which)
                assert out.shape == flags.shape == (5, len(nums)) and out.dtype == xm.dtype
                for g in range(5):
                    sl = xm[offsets[g]:offsets[g + 1]]
                    order = brute_sorted(sl)
                    for j, num in enumerate(nums):
                        f = Fraction(num * (len(sl) - 1), den)
                        want = sl[order[math.floor(f) if which == qm.SEL_LOWER else math.ceil(f)]]
                        # by value where the model flags (mixed zeros, NaNs), else bit for bit
                        assert qm.same(out[g, j], want, flags[g, j]), (ex.nm(dt), nums, den, which, g, j)
                        if dt.kind != "f":
                            assert not flags.any() and out[g, j].tobytes() == want.tobytes()


@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
def test_half_is_the_median_and_the_ends_are_min_and_max(dt):
    rng = np.random.default_rng(40 + DTYPES.index(dt))
    n = 5000
    gid, G = mm.first_occurrence_ids(rng.integers(0, 300, n))
    for x in (ex.full_range(rng, dt, n), rng.choice(ex.full_range(rng, dt, 5), n)):
        s = qm.Sorted(x, gid, G)
        for which in qc.WHICH:
            want, wflags = mm.grouped(qc.as_model(x), gid, G, which)
            out, flags = s.quantiles([1], 2, which)
            assert out[:, 0].tobytes() == want.tobytes() and np.array_equal(flags[:, 0], wflags)
            for den in (1, 3, 100, 2 ** 32 - 1):
                out, flags = s.quantiles([0, den], den, which)
                im = mm.image(qc.as_model(x))
                lo, hi = np.full(G, im.max(), im.dtype), np.zeros(G, im.dtype)
                np.minimum.at(lo, gid, im)
                np.maximum.at(hi, gid, im)
                assert np.array_equal(mm.image(out[:, 0]), lo) and np.array_equal(mm.image(out[:, 1]), hi)


def test_rank_arithmetic_against_fractions():
    for c in (1, 2, 3, 2 ** 32 - 1):
        for den in (1, 2, 3, 100, 2 ** 32 - 1):
            for num in sorted({0, 1, den - 1, den}):
                if num > den:
                    continue
                f = Fraction(num * (c - 1), den)
                assert qm.rank(num, den, c, qm.SEL_LOWER) == math.floor(f) and qm.rank(num, den, c, qm.SEL_UPPER) == math.ceil(f)
                assert 0 <= qm.rank(num, den, c, qm.SEL_LOWER) <= qm.rank(num, den, c, qm.SEL_UPPER) <= c - 1
                # the device's form in unsigned 64-bit arithmetic: p fits, and the ceiling is p / den + (p % den != 0)
                p = num * (c - 1)
                assert p < 2 ** 64 and p // den + (p % den != 0) == math.ceil(f)


# ---- the corruptions: (out, flags) of the model -> what a wrong kernel would have returned ---------------------------------------------------
def _clip(r, c):
    return max(0, min(r, c - 1))


def corrupt(name, s, nums, den, which):
    if name == "rank off by one":
        return s.quantiles(nums, den, which, rank_fn=lambda num, d, c, w: _clip(qm.rank(num, d, c, w) + 1, c))[0]
    if name == "floor and ceil swapped":
        return s.quantiles(nums, den, 1 - which)[0]
    if name == "c in place of c - 1":
        return s.quantiles(nums, den, which, rank_fn=lambda num, d, c, w: _clip(qm.rank(num, d, c + 1, w), c))[0]
    out = s.quantiles(nums, den, which)[0]
    G, nq = out.shape
    if name == "laid out [nq][G]":
        return np.ascontiguousarray(out.T).reshape(G, nq)
    if name == "ascending rank order":
        r = s.ranks(nums, den, which)
        return np.take_along_axis(out, np.argsort(r, axis=1, kind="stable"), axis=1)
    if name == "repeats answered in the first slot only":
        bad = out.copy()
        for j, num in enumerate(nums):
            if num in nums[:j]:
                bad[:, j] = 0
        return bad
    if name == "the neighbour's slice":
        return np.roll(out, 1, axis=0)
    raise KeyError(name)


CORRUPTIONS = ["rank off by one", "floor and ceil swapped", "laid out [nq][G]", "ascending rank order", "repeats answered in the first slot only",
               "c in place of c - 1", "the neighbour's slice"]


@functools.lru_cache(maxsize=None)
def _sorted_case(i):
    name, build = list(qc.grouped_cases())[i]
    keys, x = build()
    gid, G = qm.first_occurrence_ids(*keys)
    return name, qm.Sorted(x, gid, G)


@pytest.mark.parametrize("name", CORRUPTIONS)
def test_the_gpu_cases_refuse(name):
    """the comparison the GPU test makes (qm.same against the model under its flags), over the GPU test's own cases and quantile
    lists: some case refuses the corrupted answer, and every case accepts the model's own"""
    for i in range(6):                                      # the cheap cases come first; they are enough
        case, s = _sorted_case(i)
        for nums, den in qc.QLISTS:
            for which in qc.WHICH:
                out, flags = s.quantiles(nums, den, which)
                assert qm.same(out, out.copy(), flags)
                if not qm.same(corrupt(name, s, nums, den, which), out, flags):
                    return
    pytest.fail(f"no case refuses: {name}")
