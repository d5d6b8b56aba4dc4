"""The model of the exponential moving averages (tests/ema_model.py) and the case list (tests/ema_cases.py), on the CPU:
the model against answers recorded from pandas; every planted mistake of the tiled composition refused by some case; no case whose
bound is so wide that it hides a mistake it is counted as covering; the emitted-shape module compiles against the headers."""
import json
import os
import subprocess

import numpy as np
import pytest

import ema_cases as ec
import ema_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "ema_pandas.json")))


def unhex(a):
    return np.array([float.fromhex(v) for v in a], np.float64)


# ---- 1. the model against pandas -------------------------------------------------------------------------------------------------
def test_model_matches_pandas_alpha():
    """pandas evaluates sequentially in doubles -- one bracketing -- so it lies within the derived bounds of the exact model"""
    assert GOLDEN["pandas"] and len(GOLDEN["alpha_cases"]) >= 24
    for c in GOLDEN["alpha_cases"]:
        x, alpha = unhex(c["x"]), float.fromhex(c["alpha"])
        assert len(x) <= 64
        pos = np.arange(len(x))
        for mode, key in ((em.RECURSIVE, "recursive"), (em.ADJUSTED, "adjusted")):
            r = em.exact_ema(x, None, mode, alpha=alpha)
            assert np.all(np.abs(unhex(c[key]) - r.y) <= em.bound(mode, r.M, pos)), (key, alpha, len(x))


def test_model_matches_pandas_times():
    """halflife + times: pandas forms its weights its own way; 4 x the ratio the generator observed (the golden file's note)"""
    ratio = 4.0 * GOLDEN["times_ratio"]
    assert 0.0 < ratio < 9.0                     # still inside the derived bound of the adjusted form
    for c in GOLDEN["times_cases"]:
        x, decay = unhex(c["x"]), unhex(c["decay"])
        r = em.exact_ema(x, None, em.ADJUSTED, decay=decay)
        pos = np.arange(len(x))
        assert np.all(np.abs(unhex(c["adjusted"]) - r.y) <= ratio * em.U * (pos + 2) * r.M)


def test_model_semantics():
    """first rows, restarts, poison: the contract of include/aqg.h in small numbers"""
    x = np.array([4.0, 8.0, 16.0, 2.0, 6.0])
    r = em.exact_ema(x, [0, 3], em.RECURSIVE, alpha=0.5)
    assert r.y.tolist() == [4.0, 6.0, 11.0, 2.0, 4.0]
    r = em.exact_ema(x, [0, 3], em.ADJUSTED, alpha=0.5)
    assert r.y.tolist() == [4.0, (2 + 8) / 1.5, (1 + 4 + 16) / 1.75, 2.0, (1 + 6) / 1.5]
    dec = np.array([np.nan, 0.5, 0.0, 7.0, 1.0])          # a first row's decay is never read; 0 restarts; 1 keeps (b = 0)
    r = em.exact_ema(x, [0, 3], em.RECURSIVE, decay=dec)
    assert r.y.tolist() == [4.0, 6.0, 16.0, 2.0, 2.0] and not r.poisoned.any()
    bad = np.array([1.0, np.inf, 3.0, 4.0, 5.0])
    r = em.exact_ema(bad, [0, 3], em.ADJUSTED, alpha=0.25)
    assert r.poisoned.tolist() == [False, True, True, False, False] and np.isfinite(r.y[[0, 3, 4]]).all()
    r = em.exact_ema(x, [0, 3], em.RECURSIVE, decay=np.array([0.5, 1.5, 0.5, 0.5, -0.0]))
    assert r.poisoned.tolist() == [False, True, True, False, False]
    big = np.array([2 ** 63 - 1, 2 ** 62 + 1], np.int64)   # 64-bit integers convert by round-to-nearest first
    assert em.exact_ema(big, None, em.RECURSIVE, alpha=1.0).y.tolist() == [2.0 ** 63, 2.0 ** 62]


def test_wide_model_agrees_with_exact():
    """the extended-precision evaluation used for slices of millions of rows, against the exact model where both can run"""
    rng = np.random.default_rng(5)
    x = ec.column(rng, np.float64, em.EXACT_MAX + 77)
    dec = ec.decay_column(rng, "zeros", len(x))
    for mode in (em.RECURSIVE, em.ADJUSTED):
        for kw in ({"alpha": 2.0 ** -20}, {"alpha": 0.5}, {"decay": dec}):
            e = em.exact_ema(x, [0, 100], mode, **kw)
            w, pos = em.wide_ema(x, [0, 100], mode, **kw)
            assert np.array_equal(w.M, e.M)
            # the exact answer is rounded to a double once: half an ulp of it on top of the wide evaluation's own error
            assert np.all(np.abs(w.y - e.y.astype(np.longdouble)) <= em.wide_err(mode, e.M, pos) + em.U * np.abs(e.y))


# ---- 2. + 3. planted mistakes ------------------------------------------------------------------------------------------------------
_SEEN = {}


def applicable(case, fault):
    """whether the mistake can change this case's composition at all (the others are not even evaluated)"""
    grouped = case.starts is not None and len(case.starts) > 1
    return {"tile_carry_dropped": len(case.x) > ec.TS, "op_swapped": len(case.x) > ec.TS,
            "divide_before_carry": len(case.x) > ec.TS and case.mode == em.ADJUSTED,
            "carry_across_group": grouped, "den_not_restarted": grouped and case.mode == em.ADJUSTED,
            "alpha_for_d": case.decay is None, "first_decay_read": case.decay is not None,
            "decay_row_layout": case.decay_row is not None}[fault]


def fault_ratios(case):
    """{fault: max over rows of |faulted - reference| / (bound - reference error)} for the faults that change this case's composition;
    None for the poisoned cases (the restatement is for finite rows: those cases are the device tests')"""
    if case.name not in _SEEN:
        ref = ec.reference(case)
        if ref.poisoned.any():
            _SEEN[case.name] = None
            return None
        bd = em.bound(case.mode, ref.M, ref.pos) - ref.err
        kw = dict(alpha=case.alpha, decay=case.decay, tile=ec.TS)
        with np.errstate(all="ignore"):
            clean = em.tiled_ema(case.x, case.starts, case.mode, **kw)
            # the restatement itself is one bracketing: it has to pass before its corruptions mean anything
            assert np.all(np.abs(clean - ref.y) <= bd), case.name
            out = {}
            for f in em.FAULTS:
                if not applicable(case, f):
                    continue
                y = em.tiled_ema(case.x, case.starts, case.mode, fault=f, decay_row=case.decay_row, **kw)
                if not np.array_equal(y, clean, equal_nan=True):
                    err = np.abs(y - ref.y).astype(np.float64)
                    out[f] = float(np.max(np.where(np.isnan(err), np.inf, err) / np.maximum(bd, 1e-300)))
        _SEEN[case.name] = out
    return _SEEN[case.name]


CASES = ec.all_cases()


def test_case_names_are_unique():
    assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize("fault", em.FAULTS)
def test_every_planted_mistake_is_refused(fault):
    """at least one case puts the mistake beyond the asserted bound"""
    refused = [c.name for c in CASES if (fault_ratios(c) or {}).get(fault, 0.0) > 1.0]
    assert refused, fault


def test_no_case_hides_a_mistake_behind_its_bound():
    """for every case, the smallest error of a planted mistake that changes its composition exceeds the asserted bound by 2^10: a case
    whose alpha is so small, or whose slices are so long, that the bound swallows a dropped carry would not count as coverage"""
    weak, bare = [], []
    for c in CASES:
        r = fault_ratios(c)
        if r is None:
            continue
        if not r:
            bare.append(c.name)
        elif min(r.values()) < 2.0 ** 10:
            weak.append((c.name, min(r, key=r.get), min(r.values())))
    assert not weak, weak[:10]
    # a case none of the modelled mistakes changes covers none of them (it is there for a dtype, a size or a degenerate decay
    # against the device): only a column of one tile and one slice may be such a case
    assert all(c.kind == "flat" and len(c.x) <= ec.TS for c in CASES if c.name in bare), bare[:10]


# ---- 4. the emitted-shape module compiles against the headers ----------------------------------------------------------------------
def test_emitted_module_compiles():
    import aquery2_amd
    aquery2_amd.load_library()                                # the module links against the built library
    d = os.path.join(ROOT, "tests", "emitted")
    subprocess.check_call(["make", "-C", d, "build/ema.so"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(d, "build", "ema.so"))
