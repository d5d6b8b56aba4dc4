"""The count-distinct model (tests/distinct_model.py) against the answers recorded from the reference's headers
(tests/golden/ref_distinct.json), and the library's and the harness's declarations of the count-distinct entries.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import distinct_model as dm

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ref_distinct.json")) as f:
    CASES = json.load(f)["cases"]


def column(case):
    """the recorded bit patterns as a column of the recorded dtype"""
    dt = np.dtype(case["dtype"])
    u = np.dtype(f"u{dt.itemsize}")
    return np.array(case["bits"], dtype=u).view(dt) if dt != np.bool_ else np.array(case["bits"], dtype=np.uint8).astype(np.bool_)


def test_the_record_covers_what_the_rule_is_about():
    names = {c["name"] for c in CASES}
    for width in (8, 16, 32, 64):
        assert {f"dups_i{width}", f"dups_u{width}"} <= names
    for f in ("f32", "f64"):
        assert {f"zeros_{f}", f"nans_{f}", f"infs_{f}", f"empty_{f}", f"only_negzero_{f}", f"same_nan_thrice_{f}"} <= names
    for c in CASES:
        assert c["distinct"] == c["distinct_colref"], "vector_type and ColRef of the reference agree"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_equals_the_reference(case):
    x = column(case)
    assert len(x) == len(case["bits"])
    assert dm.flat(x) == case["distinct"]
    # the same rows as one group among others
    gid = np.concatenate([np.full(len(x), 1), [0, 2, 2]]).astype(np.int64)
    xs = np.concatenate([x, np.ones(3, dtype=x.dtype)])
    assert dm.grouped(xs, gid, 3).tolist() == [1, case["distinct"], 1]


def test_rule_in_words():
    for dt in (np.float32, np.float64):
        nz, nan = dt(-0.0), dt(np.nan)
        assert dm.flat(np.array([0.0, nz, nz], dtype=dt)) == 1
        assert dm.flat(np.array([nan, nan, -nan, 1.0, 1.0], dtype=dt)) == 4
        assert dm.flat(np.array([np.inf, -np.inf, np.inf], dtype=dt)) == 2
    assert dm.flat(np.array([], dtype=np.int16)) == 0
    assert dm.flat(np.array([True, False, True])) == 2
    assert dm.flat(np.array([-1, 255], dtype=np.int16)) == 2
    assert dm.grouped(np.array([5, 5, 5, 6]), np.array([0, 1, 1, 1]), 3).tolist() == [1, 2, 0]
    assert dm.grouped(np.zeros(0), np.zeros(0, dtype=np.int64), 0).dtype == np.uint32


def test_library_exports_the_count_distinct_entries():
    from aquery2_amd import capi
    names = {"aqg_count_distinct", "aqg_grouped_count_distinct", "aqg_grouped_count_distinct_flat", "aqg_distinct_last"}
    assert set(capi.DISTINCT_PROTOTYPES) == names
    for name in ("count_distinct", "grouped_count_distinct", "distinct_last"):
        assert callable(getattr(capi.Device, name))
    lib = capi.load_library()
    for name, argtypes in capi.DISTINCT_PROTOTYPES.items():
        fn = getattr(lib, name)                         # AttributeError: the library does not export it
        assert list(fn.argtypes) == argtypes and fn.restype is C.c_int
    with open(os.path.join(os.path.dirname(HERE), "include", "aqg.h")) as f:
        header = f.read()
    for name in names:
        assert f"int {name}(" in header
