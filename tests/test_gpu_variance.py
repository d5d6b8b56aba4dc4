"""vars / stddevs / varw / stddevw against the EXACT variance (tests/exact_moments.py), whole column (aqg_scan) and per group
(aqg_grouped_scan and the flat form aqg_grouped_scan_flat), on the data where E[x^2] - E[x]^2 cancels: a large offset with a small
spread (prices, timestamps, ids), full-range small integers, constant runs and slow drifts.  The contract (exact_moments.bound):
|got - T| <= 1e-9 T + 1e-12 R^2 for vars and windows of up to 64 (R: the window's range; for vars the group's range so far),
1e-9 T + 1e-10 R^2 for longer windows (R: the group's range so far), exactly 0 where R = 0; stddevs within the square root of that.
Every window length is accepted, however wide."""
import numpy as np
import pytest

import checker as ck
import exact_moments as em

pytestmark = pytest.mark.gpu
DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64]
FAMILIES = ["centred", "offset", "offset_low", "full", "constant", "ramp"]
SIZES = [1, 2, 2047, 2048, 2049, 300_001]
# the old LDS halo limits: 4097 / 4098 whole column, 3905 / 3906 grouped
WINDOWS = [1, 2, 3, 5, 8, 9, 64, 65, 100, 1000, 3905, 3906, 4097, 4098, 10_000]
WINDOWS_BIG_N = [3, 64, 65, 4098]
GROUPED_WINDOWS = [1, 2, 3, 8, 64, 65, 1000, 3905, 3906, 10_000]


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def family(rng, fam, dt, n):
    """test data; floating data is dyadic (k / 2^m), so the exact reference stays exact"""
    dt = np.dtype(dt)
    fp = dt.kind == "f"
    info = None if fp else np.iinfo(dt)
    if fam == "centred":
        if fp:
            return (rng.integers(-12800, 12800, n) / 128).astype(dt)
        return rng.integers(max(info.min, -1000), min(info.max, 1000), n, endpoint=True).astype(dt)
    if fam in ("offset", "offset_low"):
        low = fam == "offset_low"
        if dt == np.float64:
            return ((-60_000 if low else 60_000) + rng.integers(-6400, 6400, n) / 128).astype(dt)
        if dt == np.float32:
            return ((-1000 if low else 1000) + rng.integers(-64, 64, n) / 64).astype(dt)
        if dt == np.int64:
            return ((-1 if low else 1) * 1_700_000_000_000 + rng.integers(0, 1_000_000, n)).astype(dt)
        if dt == np.uint64:
            return (2**52 - 1_000_001 + rng.integers(0, 1_000_000, n)).astype(dt)
        spread = min(1000, (int(info.max) - int(info.min)) // 8)
        base = int(info.min) if low else int(info.max) - spread
        return (base + rng.integers(0, spread, n, endpoint=True)).astype(dt)
    if fam == "full":
        if fp:
            return (rng.integers(-2**20, 2**20, n) / 2**10).astype(dt)
        if dt.itemsize <= 2:
            return rng.integers(info.min, info.max, n, endpoint=True).astype(dt)
        lo, hi = (0, 2**52) if dt.kind == "u" else (-2**30, 2**30)
        return rng.integers(lo, hi, n).astype(dt)
    if fam == "constant":
        x = np.full(n, 7, dt) if fp or dt.itemsize < 8 else np.full(n, 2**40 + 3, dt)
        if n > 3000:
            x[n // 2:] = x[0] + 1                                # two constant runs
        return x
    # ramp: a slow drift with a little noise
    d = np.arange(n) // 64 + rng.integers(0, 2, n)
    if fp:
        return ((60_000 if dt == np.float64 else 500) + d / 4).astype(dt)
    if info.max < 2**15:
        return (info.min + d % (int(info.max) - int(info.min))).astype(dt)
    base = 1_700_000_000_000 if dt.itemsize == 8 else (2**31 - 100_000 if dt == np.int32 else (2**32 - 100_000 if dt == np.uint32 else 0))
    return (base + d).astype(dt)


def check_all(ex, T, got, w, what):
    ex.check(got[0], T, w, sd=False, what=what + " var")
    ex.check(got[1], T, w, sd=True, what=what + " stddev")


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dt", DTYPES)
def test_whole_column(gpu, dt, fam):
    rng = np.random.default_rng(10 * DTYPES.index(dt) + FAMILIES.index(fam))
    for n in SIZES:
        x = family(rng, fam, dt, n)
        ex = em.Exact(x)
        got = [gpu.scan(ck.SCAN_NAMES[nm], x) for nm in ("vars", "stddevs")]
        check_all(ex, ex.var(), got, None, f"vars {np.dtype(dt)} {fam} n={n}")
        for w in (WINDOWS if n < 10_000 else WINDOWS_BIG_N) + [n, n + 3]:
            got = [gpu.scan(ck.SCAN_NAMES[nm], x, w) for nm in ("varw", "stddevw")]
            check_all(ex, ex.var(w), got, w, f"varw {np.dtype(dt)} {fam} n={n} w={w}")


def test_whole_column_matches_the_oracle(gpu, oracle):
    """the parity target (the oracle) and the device agree on offset data as well"""
    rng = np.random.default_rng(11)
    for dt in (np.int32, np.int64, np.float64):
        x = family(rng, "offset", dt, 5000)
        a, b = gpu.scan(ck.SCAN_NAMES["vars"], x), oracle.scan(ck.SCAN_NAMES["vars"], x)
        assert np.all(np.abs(a - b) <= 2e-9 * b + 1e-12), dt
        ex = em.Exact(x)
        for w in (3, 100, 4098):
            a, b = gpu.scan(ck.SCAN_NAMES["varw"], x, w), oracle.scan(ck.SCAN_NAMES["varw"], x, w)
            bnd, _ = em.bound(x, ex.var(w), w)                  # the contract, plus the oracle's own long-double rounding
            assert np.all(np.abs(a - b) <= bnd + 1e-12 * b), (dt, w)


@pytest.mark.parametrize("dt", [np.int8, np.int16, np.int32, np.uint32])
def test_shift_invariance(gpu, dt):
    """vars(x + C) == vars(x) within the contract, for C up to the type's maximum minus max(x): needs no reference at all"""
    rng = np.random.default_rng(3)
    info = np.iinfo(dt)
    x = rng.integers(0, min(1000, int(info.max) // 4), 300_001).astype(dt)
    base = gpu.scan(ck.SCAN_NAMES["vars"], x)
    R = em.running_range(x)
    for C in (1, 1000, int(info.max) - int(x.max())):
        got = gpu.scan(ck.SCAN_NAMES["vars"], (x.astype(np.int64) + C).astype(dt))
        assert np.all(np.abs(got - base) <= 2e-9 * base + 2e-12 * R * R), (dt, C)
        for w in (5, 100):
            a = gpu.scan(ck.SCAN_NAMES["varw"], (x.astype(np.int64) + C).astype(dt), w)
            b = gpu.scan(ck.SCAN_NAMES["varw"], x, w)
            Rw, c = (em.window_range(x, w), 1e-12) if w <= em.SHORT_W else (R, 1e-10)   # both sides within the contract
            assert np.all(np.abs(a - b) <= 2e-9 * b + 2 * c * Rw * Rw), (dt, C, w)


def grouped_keys(rng, shape, n, G):
    if shape == "singletons":
        return rng.permutation(n).astype(np.int32)
    k = rng.integers(0, G, n).astype(np.int32)
    if shape == "long_front":
        k[: n // 2] = k[0]                                       # one long group in front: carries over many tiles
    elif shape == "runs":
        k = np.repeat(rng.integers(0, G, n // 37 + 1), 37)[:n].astype(np.int32)   # starts inside a window's halo
    return k


@pytest.mark.parametrize("shape,G", [("random", 1), ("random", 300), ("random", 70_000), ("long_front", 300), ("singletons", 0),
                                     ("runs", 300), ("interleaved", 300)])
@pytest.mark.parametrize("dt", DTYPES)
def test_grouped(gpu, oracle, dt, shape, G):
    n = 300_001 if shape == "long_front" else 100_001
    rng = np.random.default_rng(G + len(shape) + DTYPES.index(dt))
    keys = grouped_keys(rng, shape, n, G)
    fam = "ramp" if shape == "runs" else ("centred" if G == 70_000 else "offset")
    x = family(rng, fam, dt, n)
    if shape == "interleaved":                                  # symbols priced ~10 and ~60000 (type permitting) in the same tiles
        lowv = family(rng, "offset_low" if np.dtype(dt).kind in "if" else "centred", dt, n)
        x = np.where(keys % 2 == 0, x, lowv)
    ogb = oracle.groupby([keys])
    gb = gpu.groupby_build([keys])
    off = ogb["offsets"]
    xf = x[ogb["row_ids"]]
    xflat = gpu.grouped_flatten(gb, x, keep=True)
    ex = em.Exact(xf, off)
    got = [gpu.grouped_scan(gb, ck.SCAN_NAMES[nm], x) for nm in ("vars", "stddevs")]
    check_all(ex, ex.var(), got, None, f"grouped vars {np.dtype(dt)} {shape} G={G}")
    for w in GROUPED_WINDOWS + [n + 3]:
        got = [gpu.grouped_scan(gb, ck.SCAN_NAMES[nm], x, w) for nm in ("varw", "stddevw")]
        check_all(ex, ex.var(w), got, w, f"grouped varw {np.dtype(dt)} {shape} G={G} w={w}")
        if w in (3, 65, n + 3):
            flat = gpu.grouped_scan(gb, ck.SCAN_NAMES["varw"], xflat, w, flat=True)
            assert np.array_equal(flat, got[0]), ("flat form", w)


def test_wide_grouped_window_returns(gpu):
    """varw(5000, x[val]) per group, which the header layer's vcol_scan would turn into a process abort on any error status"""
    rng = np.random.default_rng(8)
    keys = rng.integers(0, 3, 50_000).astype(np.int32)
    x = family(rng, "offset", np.int32, 50_000)
    gb = gpu.groupby_build([keys])
    got = gpu.grouped_scan(gb, ck.SCAN_NAMES["varw"], x, 5000)
    assert got.shape == (50_000,) and np.all(np.isfinite(got))
