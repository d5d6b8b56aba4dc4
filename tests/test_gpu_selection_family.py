"""The three radix selections on the shapes of tests/selection_family_cases.py, one route pinned per fresh process (the thresholds are
read once): for every group, bit for bit,
    grouped_quantiles([1], 2, which) == grouped_median(which),
    grouped_quantiles([0], 1) == grouped_topk(ASC, 1),    grouped_quantiles([1], 1) == grouped_topk(DESC, 1),
each equal to its numpy model, with the route mask the pinned switches imply.  The families share the load shape of a slice, the
routing, the SMALL kernel's body and the step after a digit (select_radix.hpp): a slip there that each family's own, aligned, cases
miss shows here as a disagreement with the model."""
import os
import subprocess
import sys

import pytest

import selection_family_cases as sf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, "tests")
import aquery2_amd, selection_family_cases as sf
gpu = aquery2_amd.Device(0)
checked = 0
for name, dt, counts, x in sf.generate():
    want_routes = sf.expected_routes(counts, PIN)
    gb = gpu.groupby_build([sf.keys_of(counts)])
    assert np.array_equal(gpu.group_offsets(gb), sf.offsets(counts)), "sorted keys: the flat layout is the column"
    xd = gpu.to_device(x)
    def routed(answer):
        assert gpu.select_last_routes()[0] == want_routes, (PIN, name, str(dt), gpu.select_last_routes(), want_routes)
        return answer

    for (what, arg), answers in sf.models(x, counts).items():
        if what == "median":
            got = {"quantiles": routed(gpu.grouped_quantiles(gb, xd, [1], 2, arg, flat=True))[:, 0],
                   "median": routed(gpu.grouped_median(gb, xd, arg, flat=True))}
        else:
            got = {"quantiles": routed(gpu.grouped_quantiles(gb, xd, [0 if what == "min" else 1], 1, flat=True))[:, 0],
                   "topk": routed(gpu.grouped_topk(gb, xd, 1, arg, flat=True))[:, 0]}
        a, b = got.values()
        assert a.tobytes() == b.tobytes(), (PIN, name, str(dt), what, arg, "the families disagree", np.flatnonzero(a != b)[:5])
        for family, (want, flags) in answers.items():
            g = got[family]
            assert not flags.any() and g.dtype == want.dtype
            assert g.tobytes() == want.tobytes(), (PIN, name, str(dt), what, arg, family, np.flatnonzero(g != want)[:5])
            checked += 1
    assert np.array_equal(xd.to_host().view(np.uint8), x.view(np.uint8)), "the column was modified"
    gb.destroy()
print("OK", checked, flush=True)
'''


@pytest.mark.parametrize("pin", list(sf.PINS))
def test_families_agree_on_shared_skeleton_shapes(pin):
    small_max, split_min = sf.PINS[pin]
    env = dict(os.environ, AQG_SELECT_SMALL_MAX=str(small_max), AQG_SELECT_SPLIT_MIN=str(split_min))
    out = subprocess.run([sys.executable, "-c", f"PIN = {pin!r}\n" + CHILD], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])
    assert int(out.stdout.split()[-1]) == len(sf.CASES) * len(sf.DTYPES) * 8
