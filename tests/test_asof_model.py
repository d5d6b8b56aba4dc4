"""The model of the as-of join (tests/asof_model.py) held to itself and to an independent implementation: its brute-force statement of
the contract equals its sort-and-search form on every named case and on seeded random sides; both equal recorded answers of pandas
merge_asof (tests/golden/asof_merge_asof.json, written by tools/gen_asof_golden.py); and every deliberate mistake a device
implementation is likely to make is told from the model by at least one named case.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import asof_cases
import asof_model as am
import checker as ck

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = [(d, s) for d in (am.BACKWARD, am.FORWARD) for s in (False, True)]


@pytest.fixture(scope="module")
def brute():
    """asof_rows of every named case and mode, computed once"""
    return {(name, d, s): am.asof_rows(c[0], c[1], c[2], c[3], d, s) for name, c in asof_cases.cases().items() for d, s in MODES}


@pytest.mark.parametrize("name", sorted(asof_cases.cases()))
def test_brute_force_equals_sorted_model(brute, name):
    bk, bo, pk, po, routes = asof_cases.cases()[name]
    for d, s in MODES:
        assert np.array_equal(brute[name, d, s], am.asof_rows_sorted(bk, bo, pk, po, d, s)), (d, s)
    assert bool(routes & am.PRESORTED) == am.presorted(bo)
    assert bool(routes & am.NOKEYS) == (not bk)
    G = am.group_ids(bk, len(bo), [], 0)[1] if bk else 1
    w = 8 if bo.dtype.itemsize == 8 else 4
    assert bool(routes & am.LDS) == (len(bo) * (w + 4) + (G + 1) * 4 <= 48 * 1024 and len(po) >= 1 << 16)
    assert bool(routes & am.HBM) != bool(routes & am.LDS)


def test_brute_force_equals_sorted_model_on_random_sides():
    for seed in range(200):
        bk, bo, pk, po, d, s = asof_cases.random_sides(seed, 40)
        assert np.array_equal(am.asof_rows(bk, bo, pk, po, d, s), am.asof_rows_sorted(bk, bo, pk, po, d, s)), seed


def test_cases_cover_what_they_name(brute):
    c = asof_cases.cases()
    assert {len(c[n][3]) for n in c} >= {1, 2, 3, 5, (1 << 16) + 3}
    assert {c[n][4] for n in c} >= {am.HBM, am.LDS, am.HBM | am.PRESORTED, am.HBM | am.NOKEYS, am.HBM | am.NOKEYS | am.PRESORTED}
    assert len(c["hbm_big"][1]) == 1 << 17
    sizes = np.bincount(c["group_sizes"][0][0][1])
    sizes = set(sizes[sizes > 0].tolist())
    assert sizes >= {1, 2} | {(1 << k) + d for k in range(2, 12) for d in (-1, 0, 1)}
    assert c["ends_uint64"][1].max() > 1 << 63 and c["ends_int64"][1].min() == -(1 << 63)
    for name in ("ends_float64", "ends_float32"):
        for col in (c[name][1], c[name][3]):
            assert np.isnan(col).any() and np.isinf(col).any() and np.signbit(col[col == 0]).any() and not np.signbit(col[col == 0]).all()
    # every mode of every case has rows with and (but for the one-row probe) without a partner
    for (name, d, s), r in brute.items():
        assert (r != am.NONE).any() or name == "np_1", (name, d, s)


# ---- an independent implementation ---------------------------------------------------------------------------------------------------
def test_model_equals_recorded_merge_asof():
    with open(os.path.join(HERE, "golden", "asof_merge_asof.json")) as f:
        gold = json.load(f)
    assert len(gold["sides"]) >= 10
    for k, side in enumerate(gold["sides"]):
        dt = np.dtype(side["dtype"])
        bo, po = np.array(side["build_on"], dt), np.array(side["probe_on"], dt)
        bk = [(ck.INT32, np.array(side["build_by"], np.int32))] if side["by"] else []
        pk = [(ck.INT32, np.array(side["probe_by"], np.int32))] if side["by"] else []
        assert len(np.unique(bo)) < len(bo) // 2                 # many duplicate times
        for d, dn in ((am.BACKWARD, "backward"), (am.FORWARD, "forward")):
            for s, sn in ((False, "exact"), (True, "strict")):
                want = np.array(side["answers"]["%s_%s" % (dn, sn)], np.int64)
                want = np.where(want < 0, am.NONE, want).astype(np.uint32)
                assert np.array_equal(am.asof_rows(bk, bo, pk, po, d, s), want), (k, dn, sn)
                assert np.array_equal(am.asof_rows_sorted(bk, bo, pk, po, d, s), want), (k, dn, sn)


# ---- the cases tell every likely mistake from the model -------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", am.MUTANTS)
def test_a_named_case_distinguishes_the_mutant(brute, mutant):
    killers = [(name, d, s) for name, c in asof_cases.cases().items() for d, s in MODES
               if not np.array_equal(am.asof_rows_sorted(c[0], c[1], c[2], c[3], d, s, mutant=mutant), brute[name, d, s])]
    assert killers, mutant


def test_straddling_neighbours_give_a_wrong_row_not_a_plausible_one(brute):
    """a segment bound off by one shows in the straddle case by itself"""
    bk, bo, pk, po, _ = asof_cases.cases()["straddle"]
    for mutant in ("segment_end_plus_1", "segment_start_minus_1"):
        assert any(not np.array_equal(am.asof_rows_sorted(bk, bo, pk, po, d, s, mutant=mutant), brute["straddle", d, s]) for d, s in MODES), mutant


# ---- the library exports the entries ---------------------------------------------------------------------------------------------------
def test_library_exports_the_entries():
    import aquery2_amd
    lib = C.CDLL(aquery2_amd.lib_path())
    for f in ("aqg_join_asof", "aqg_join_asof_last"):
        assert hasattr(lib, f), f
