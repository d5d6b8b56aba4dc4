"""The median model (tests/median_model.py) against Python's statistics.median_low / median_high over sorted lists, and the
harness's declarations of the median entries.  No GPU."""
import ctypes as C
import statistics

import numpy as np
import pytest

import extremes as ex
import median_model as mm

DTYPES = ex.NUM_DTYPES + [np.dtype(np.bool_)]
COUNTS = [1, 2, 3, 4, 5, 8, 9, 64, 65, 100, 101]


def py_median(vals, which):
    """median_low / median_high of a list ordered like the model: NaNs last, the two zeros equal"""
    vals = sorted(vals, key=lambda v: (v != v, 0 if v != v else v))
    return (statistics.median_high if which == mm.SEL_UPPER else statistics.median_low)(vals) if all(v == v for v in vals) \
        else vals[len(vals) // 2 if which == mm.SEL_UPPER else (len(vals) - 1) // 2]


def agrees(got, want):
    return (got != got and want != want) or got == want


@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
@pytest.mark.parametrize("which", [mm.SEL_LOWER, mm.SEL_UPPER])
def test_flat_model_matches_statistics(dt, which):
    rng = np.random.default_rng(7)
    for c in COUNTS:
        for col in (ex.full_range(rng, dt, c), np.repeat(ex.full_range(rng, dt, 1), c), rng.choice(ex.full_range(rng, dt, 3), c)):
            got, flag = mm.flat(col, which)
            assert not flag
            assert got.dtype == col.dtype
            assert agrees(got.item(), py_median(col.tolist(), which)), (c, col)
            assert got.tobytes() in {v.tobytes() for v in col}            # an element of the input, bit for bit


@pytest.mark.parametrize("dt", DTYPES, ids=ex.nm)
def test_grouped_model_matches_statistics(dt):
    rng = np.random.default_rng(11)
    for G in (1, 2, 3, 10, 37):
        counts = rng.choice(COUNTS, G)
        gid = rng.permutation(np.repeat(np.arange(G), counts))
        x = rng.choice(ex.full_range(rng, dt, 50), len(gid))             # duplicates in every group
        for which in (mm.SEL_LOWER, mm.SEL_UPPER):
            got, flags = mm.grouped(x, gid, G, which)
            assert not flags.any()
            for g in range(G):
                assert agrees(got[g].item(), py_median(x[gid == g].tolist(), which)), (G, g)


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_infinities_are_ordinary_values(dt):
    x = np.array([np.inf, -np.inf, 1.0, np.inf, -np.inf, np.inf], dtype=dt)
    assert mm.flat(x, mm.SEL_LOWER) == (dt.type(1.0), False)
    assert mm.flat(x, mm.SEL_UPPER) == (dt.type(np.inf), False)
    assert mm.flat(np.array([-np.inf, -np.inf, 5.0], dtype=dt))[0] == -np.inf


@pytest.mark.parametrize("dt", ex.FP_DTYPES, ids=ex.nm)
def test_predicate_fires_on_mixed_zeros_and_nans(dt):
    nz, nan = dt.type(-0.0), dt.type(np.nan)
    # the rank lands on a zero of a group that holds both zeros
    got, flag = mm.flat(np.array([-1, 0.0, nz, 0.0, 1], dtype=dt))
    assert flag and got == 0
    # only one kind of zero: bit for bit
    got, flag = mm.flat(np.array([-1, nz, nz, nz, 1], dtype=dt))
    assert not flag and np.signbit(got)
    # both zeros present but the rank is elsewhere
    got, flag = mm.flat(np.array([0.0, nz, 5, 6, 7], dtype=dt))
    assert not flag and got == 5
    # NaNs sort above +inf, whatever their sign
    x = np.array([np.inf, nan, ex._neg_nan(dt), 1.0], dtype=dt)
    assert mm.flat(x, mm.SEL_LOWER) == (dt.type(np.inf), False)
    got, flag = mm.flat(x, mm.SEL_UPPER)
    assert flag and np.isnan(got)
    # grouped: one flag per group
    gid = np.array([0, 0, 0, 1, 1, 1, 2])
    got, flags = mm.grouped(np.array([0.0, nz, nz, nan, nan, 1, 3], dtype=dt), gid, 3)
    assert flags.tolist() == [True, True, False] and got[2] == 3
    assert mm.same(np.array([nz, -nan, 3], dtype=dt), got, flags)
    assert not mm.same(np.array([1, -nan, 3], dtype=dt), got, flags)
    assert not mm.same(np.array([nz, -nan, 4], dtype=dt), got, flags)


def test_pools_planted():
    for dt in DTYPES:
        col = ex.unary_column(dt, 3000, 5)
        for which in (mm.SEL_LOWER, mm.SEL_UPPER):
            got, flag = mm.flat(col, which)
            assert agrees(got.item(), py_median(col.tolist(), which))


def test_first_occurrence_ids():
    a = np.array([5, 3, 5, 9, 3, 3, 1])
    b = np.array([0, 0, 0, 1, 0, 1, 0])
    gid, G = mm.first_occurrence_ids(a)
    assert G == 4 and gid.tolist() == [0, 1, 0, 2, 1, 1, 3]
    gid, G = mm.first_occurrence_ids(a, b)
    assert G == 5 and gid.tolist() == [0, 1, 0, 2, 1, 3, 4]
    assert mm.first_occurrence_ids(a[:0])[1] == 0


def test_harness_declares_the_median_entries():
    from aquery2_amd import capi
    assert (capi.SEL_LOWER, capi.SEL_UPPER) == (0, 1) == (mm.SEL_LOWER, mm.SEL_UPPER)
    assert (capi.ROUTE_SMALL, capi.ROUTE_GROUP, capi.ROUTE_SPLIT) == (1, 2, 4)
    assert set(capi.MEDIAN_PROTOTYPES) == {"aqg_median", "aqg_grouped_median", "aqg_grouped_median_flat", "aqg_select_last_routes"}
    for name in ("median", "grouped_median", "select_last_routes"):
        assert callable(getattr(capi.Device, name))
    lib = capi.load_library()
    for name, argtypes in capi.MEDIAN_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is C.c_int
