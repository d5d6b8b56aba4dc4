"""The bits of the floating folds: aqg_rangew, aqg_grouped_rangew and aqg_interval_fold, SUM and AVG over float32 / float64 columns,
against the digests recorded in tests/golden/fold_digests.json (tools/gen_fold_digests.py).  The other modules hold these sums to
their error bound; this one holds the order in which the block tree combines its operands, which a bound cannot see."""
import json
import os

import pytest

import fold_digest_cases

pytestmark = pytest.mark.gpu
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fold_digests.json")


@pytest.fixture(scope="module")
def got():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    out = fold_digest_cases.outputs(d)
    d.close()
    return out


def test_every_recorded_case_is_computed_and_none_else(got):
    with open(PATH) as f:
        want = json.load(f)["digests"]
    assert sorted(got) == sorted(want)


def test_bits_of_the_floating_folds(got):
    with open(PATH) as f:
        want = json.load(f)["digests"]
    differ = [k for k in want if got[k][0] != want[k]]
    assert not differ, "the bracketing of these floating folds changed: %s" % differ
