"""The comparisons of the sum / average / variance scans against the oracle, shared by the tests that make them
(test_gpu_scan_join.py::test_scans_sums, test_gpu_grouped_scan.py, test_gpu_window_paths.py): one definition of every bound."""
import numpy as np

import exact_moments as em
import golden_util as gu


def ulp_close(a, b, ulps):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b))))


def column_sum_scan(name, w, x, a, b):
    """whole column, a = device, b = oracle.  sums/sumw on integers: bit-exact (128-bit).  avgs on integers: bit-exact (one division
    of an exact sum).  avgw on integers: the device rounds the exact window mean once; the reference accumulates a floating recurrence
    (aggregations.h:270-271), so both are compared with the exact rational.  Floating inputs: tree order vs sequential."""
    dt, n = x.dtype, len(x)
    is_int = np.dtype(dt).kind != "f"
    if is_int and name in ("sums", "sumw", "avgs"):
        assert gu.same_bits(a, b), (name, w, dt, n)
    elif is_int:  # avgw
        ww = min(w, n)
        xs = [int(v) for v in x]
        pref = np.concatenate([[0], np.cumsum(np.array(xs, dtype=object))])
        idx = np.arange(n)
        lens = np.minimum(idx + 1, ww)
        exact = np.array([float((pref[i + 1] - pref[i + 1 - l])) / float(l) for i, l in zip(idx, lens)])
        assert ulp_close(a, exact, 1), (name, w, dt)                       # device: <= 1 ulp of the exact mean
        if np.dtype(dt).kind == "u" and np.dtype(dt).itemsize >= 4:
            return     # reference quirk: (arr[i] - arr[i-w]) wraps for unsigned 4/8-byte inputs (aggregations.h:271)
        drift = 4.0 * np.spacing(float(np.max(np.abs(exact))) + 1.0) * (idx + 2)   # ~2 roundings per step at the largest magnitude
        assert np.all(np.abs(b - exact) <= drift), (name, w, dt)           # reference: inside its recurrence drift
        assert np.all(np.abs(a - b) <= drift)
    else:
        scale = np.maximum(1.0, np.abs(b.astype(np.float64)))
        # avgw: the reference subtracts arr[i]-arr[i-w] in T (float32 rounding per step), then drifts
        eps = float(np.finfo(dt).eps) if name == "avgw" else 2.0 ** -52
        sabs = float(np.sum(np.abs(x.astype(np.float64))))
        # any summation order: |err| <= (n-1) u sum|x| (both sides); avgw additionally carries the reference's per-step T rounding
        tol = 2 * n * 2.0 ** -52 * sabs + (100.0 * eps * float(np.max(np.abs(x))) * (np.arange(n) + 8) if name == "avgw" else 0)
        assert np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol), (name, w, dt)


def grouped_window(name, dt, got, want, absx, pos, what):
    """a window over the flat layout of a grouping against the oracle's composition: absx = |flat column| in double, pos = position
    of every row inside its group"""
    fp = np.dtype(dt).kind == "f"
    if name in ("minw", "maxw") or (name == "sumw" and not fp) or name == "ratiow":
        assert gu.same_bits(got, want), what
    else:
        eps_in = float(np.finfo(dt).eps) if fp else 2.0 ** -52
        bound = 4 * eps_in * float(np.max(absx)) * (pos + 2) + 1e-9
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound), what


def variance(exact, name, w, got, what, want=None):
    """the variance contract against the exact values (exact_moments.py; exact = em.Exact of the column, with the group offsets for a
    grouping), and against the oracle's result `want` where the caller could afford one"""
    win = None if name in ("vars", "stddevs") else w
    T = exact.var(win)
    sd = name.startswith("stddev")
    exact.check(got, T, win, sd=sd, what=what)
    if want is not None:
        b, _ = em.bound(exact.x, T, win, exact.offsets)
        tol = np.sqrt(b) if sd else b
        assert np.all(np.abs(got - want) <= 2 * tol + 1e-9 * np.abs(want)), what
