"""TableInfo::order_by over device-typed columns (include/aquery/table.h): tests/emitted/orderby_device.cpp, built by the emitted
modules' pattern rule and run through host_main, sorts about 1e6 rows with order_by<-1, -2, 2>() over long / unsigned int / double
columns and materialises the result.  The expected order is numpy's stable sort under the header's exact key meaning: `-a` of a long
is descending order, `-b` of an unsigned int is (-b) mod 2^32 ascending, c ascending with -0.0 == +0.0; ties keep row order."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EM = os.path.join(HERE, "emitted")


@pytest.mark.gpu
def test_order_by_runs_on_the_device_and_is_stable(tmp_path):
    subprocess.check_call(["make", "-C", EM, "build/orderby_device.so", "build/host_main"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(EM, "build", "host_main"), os.path.join(EM, "build", "orderby_device.so"), "synthetic",
                          "dll_orderby_device"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().splitlines()
    n = 1000003
    assert lines[0] == f"rows {n}"
    passes = int(lines[1].split()[1])
    assert passes > 0, "order_by did not run on the device"
    assert lines[-1] == "done."
    a = np.fromfile(tmp_path / "orderby_in.0", dtype=np.int64)
    b = np.fromfile(tmp_path / "orderby_in.1", dtype=np.uint32)
    c = np.fromfile(tmp_path / "orderby_in.2", dtype=np.float64)
    ids = np.fromfile(tmp_path / "orderby_ids", dtype=np.uint32)
    assert len(a) == len(b) == len(c) == len(ids) == n
    assert np.any(b == 0) and np.any(b == 2**32 - 1) and np.any(np.signbit(c) & (c == 0))
    negb = np.zeros(1, np.uint32) - b                     # (-b) mod 2^32: 0 first, then descending
    c0 = np.where(c == 0, 0.0, c)
    want = np.lexsort((c0, negb, -a)).astype(np.uint32)
    assert np.array_equal(ids, want)
    rev = want[::-1].copy()                               # the module reverses the ids on the host and sets the first to row 7
    rev[0] = 7
    for k, col in enumerate((a, b, c)):
        got = np.fromfile(tmp_path / f"orderby_sorted.{k}", dtype=col.dtype)
        assert np.array_equal(got.view(np.uint8), col[want].view(np.uint8)), k
        got = np.fromfile(tmp_path / f"orderby_rev.{k}", dtype=col.dtype)
        assert np.array_equal(got.view(np.uint8), col[rev].view(np.uint8)), ("gather through ids rewritten on the host", k)
