"""The cases tests/test_gpu_quantiles.py runs on the device, shared with tests/test_quantile_model.py, which shows on the CPU that this
very list refuses every corruption a kernel could produce.  Nothing here needs a GPU."""
import numpy as np

import extremes as ex

SMALL_MAX = 256          # select.hip: AQG_SELECT_SMALL_MAX default (groups ranked in LDS)
SMALL_CAP = 512          # ... and its largest value
SPLIT_MIN = 1 << 20      # select.hip: AQG_SELECT_SPLIT_MIN default (groups cut into chunks)
DTYPES = ex.NUM_DTYPES + [np.dtype(np.bool_)]
WHICH = (0, 1)
PERCENTILES = ([0, 1, 5, 25, 50, 75, 95, 100], 100)
# (nums, den): eight percentiles, the median, repeats out of order, and the widest denominator
QLISTS = [PERCENTILES, ([1], 2), ([3, 3, 0, 3], 3), ([1], 2 ** 32 - 1)]
FLAT_SIZES = [0, 1, 2, 3, 63, 64, 65, SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, SPLIT_MIN - 1, SPLIT_MIN, SPLIT_MIN + 1]
THRESHOLD_SIZES = [1, 2, 3, 64, 65, SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, 2047, 2048, 2049, SPLIT_MIN - 1, SPLIT_MIN, SPLIT_MIN + 1] * 2


def as_model(a):
    return a.astype(np.uint8) if a.dtype == np.bool_ else a


def flat_inputs(rng, dt, n):
    """random full-range values, an all-equal column, two distinct values, sorted both ways"""
    r = ex.full_range(rng, dt, n)
    two = ex.full_range(rng, dt, 2)
    yield "random", r
    yield "equal", np.repeat(ex.full_range(rng, dt, 1), n)
    yield "two", two[rng.integers(0, 2, n)]
    yield "ascending", np.sort(r)
    yield "descending", np.sort(r)[::-1].copy()


def threshold_case(dt, seed=78):
    """groups of every size at which the selection takes another path, twice, keys permuted: all three routes in one call"""
    rng = np.random.default_rng(seed)
    keys = rng.permutation(np.repeat(np.arange(len(THRESHOLD_SIZES)), THRESHOLD_SIZES)).astype(np.int32)
    return [keys], ex.full_range(rng, dt, len(keys))


def tile_border_case():
    """300 groups of exactly SMALL_MAX rows: every tile border is straddled"""
    rng = np.random.default_rng(81)
    keys = rng.permutation(np.repeat(np.arange(300), SMALL_MAX)).astype(np.int32)
    return [keys], ex.full_range(rng, np.dtype(np.int32), len(keys))


def two_keys_case(bool_values):
    rng = np.random.default_rng(79)
    n = 40_003
    k1, k2 = rng.integers(0, 30, n).astype(np.int16), rng.integers(-5, 5, n).astype(np.int64)
    return [k1, k2], rng.integers(0, 2, n).astype(np.bool_) if bool_values else ex.full_range(rng, np.dtype(np.float32), n)


SEEDS = range(10)


def seeded_case(seed):
    """one group, every row its own group, a few rows per group, sizes around SMALL_MAX, 100 groups, skewed sizes: at most 3e6 rows"""
    rng = np.random.default_rng(4300 + seed)
    dt = DTYPES[(seed * 3 + 1) % len(DTYPES)]
    n = [1, 2, 777, 5000, 70_001, 300_001, 1_000_003, 2_000_000, 3_000_000, 1_500_017][seed]
    kind = seed % 6
    if kind == 0:
        keys = np.zeros(n, np.int32)                                      # one group
    elif kind == 1:
        keys = rng.permutation(n).astype(np.int32)                        # every row its own group
    elif kind == 2:
        keys = rng.integers(0, max(1, n // 3), n).astype(np.int32)        # a few rows per group
    elif kind == 3:
        keys = rng.integers(0, max(1, n // 200), n).astype(np.int32)      # around the SMALL threshold
    elif kind == 4:
        keys = rng.integers(0, 100, n).astype(np.int32)
    else:
        keys = (rng.integers(0, 1000, n) ** 2 // 1000).astype(np.int32)   # skewed sizes
    x = ex.full_range(rng, dt, n) if seed % 2 else rng.choice(ex.full_range(rng, dt, 40), n)
    return [keys], x


def grouped_cases():
    """(name, builder) of every grouped case of the GPU test, the cheap ones first"""
    yield "two keys", lambda: two_keys_case(False)
    yield "two keys, bool values", lambda: two_keys_case(True)
    yield "tile borders", tile_border_case
    for seed in SEEDS:
        yield f"seeded {seed}", lambda seed=seed: seeded_case(seed)
    for dt in (np.dtype(np.float64), np.dtype(np.int16), np.dtype(np.uint32)):
        yield f"thresholds {ex.nm(dt)}", lambda dt=dt: threshold_case(dt)
