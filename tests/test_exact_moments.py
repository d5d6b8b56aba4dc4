"""The exact variance helper (tests/exact_moments.py) against the oracle's vars (the reference's recurrence with an exact LongType
running sum) and varw (a long-double two-pass, D9) on data with a large offset and a small spread: the truth the GPU variance tests
use and the parity target agree, so the GPU tolerances rest on both."""
import numpy as np
import pytest

import checker as ck
import exact_moments as em


def test_small_known_values():
    x = np.array([1, 2, 3, 4], np.int32)
    assert em.running_var(x).tolist() == [0.0, 0.25, 2 / 3, 1.25]
    assert em.window_var(x, 2).tolist() == [0.0, 0.25, 0.25, 0.25]
    assert em.window_var(x, 3, offsets=[0, 2]).tolist() == [0.0, 0.25, 0.0, 0.25]
    y = np.array([0.5, 0.25, -1.0], np.float64)
    assert em.running_var(y)[-1] == float(np.var(np.array(y, np.longdouble)))


def offset_data(rng, dt, n):
    if dt == np.int32:
        return (2**31 - 1001 + rng.integers(0, 1000, n)).astype(dt)
    if dt == np.uint32:
        return (2**32 - 1001 + rng.integers(0, 1000, n)).astype(dt)
    if dt == np.int64:
        return (1_700_000_000_000 + rng.integers(0, 1_000_000, n)).astype(dt)
    if dt == np.float64:
        return (60_000 + rng.integers(-6400, 6400, n) / 128).astype(dt)
    return (1000 + rng.integers(-64, 64, n) / 64).astype(dt)


@pytest.mark.parametrize("dt", [np.int32, np.uint32, np.int64, np.float64, np.float32])
def test_helper_agrees_with_the_oracle_on_offset_data(oracle, dt):
    rng = np.random.default_rng(5)
    n = 3000
    x = offset_data(rng, dt, n)
    T = em.running_var(x)
    got = oracle.scan(ck.SCAN_NAMES["vars"], x)
    assert np.all(np.abs(got - T) <= 1e-9 * T + 1e-12), dt
    for w in (1, 2, 3, 64, 65, 1000, n + 3):
        T = em.window_var(x, w)
        got = oracle.scan(ck.SCAN_NAMES["varw"], x, w)
        assert np.all(np.abs(got - T) <= 1e-12 * T), (dt, w)
        assert np.all(T[:1] == 0) and (w > 1 or np.all(T == 0))
    # grouped layout: the window clamps at every group's start
    off = [0, 1, 700, 701, 2500]
    T = em.window_var(x, 5, offsets=off)
    bounds = off + [n]
    want = np.concatenate([oracle.scan(ck.SCAN_NAMES["varw"], x[a:b], 5) for a, b in zip(bounds[:-1], bounds[1:])])
    assert np.all(np.abs(want - T) <= 1e-12 * T), dt
