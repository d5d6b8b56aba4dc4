"""Cases for the skeleton the three radix selections share (select_radix.hpp: sweep_rows, classify_groups, small_tile, digit_step):
median, top-k and quantiles asked the same question about the same groups must give the same bits, on shapes where each family's own
cases happen to be aligned.  A case is a list of group sizes; the keys are sorted, so the flat layout is the column itself and group g is
the slice [off[g], off[g + 1]) with off = cumsum(counts) -- the start of every slice, in elements off a 16-byte boundary, is chosen here.

The values hold no NaN and no zero, so every answer is one bit pattern (ties are copies of the same bits): the models' ambiguity flags
are all False, which tests/test_selection_family_cases.py asserts together with the agreement of the three numpy models."""
import numpy as np

import median_model as mm
import quantile_model as qm
import topk_model as tm

TILE = 2048                 # select_radix.hpp: flat positions per workgroup of the SMALL route
SMALL_CAP = 512             # ... largest AQG_SELECT_SMALL_MAX
SPLIT_CHUNK = 8192          # ... rows per chunk of the SPLIT route
ROUTE_SMALL, ROUTE_GROUP, ROUTE_SPLIT = 1, 2, 4
NEVER = 4_000_000_000

DTYPES = [np.dtype(np.int8), np.dtype(np.uint16), np.dtype(np.float32), np.dtype(np.int64)]

# the switches of one child process: (AQG_SELECT_SMALL_MAX, AQG_SELECT_SPLIT_MIN)
PINS = {
    "small": (SMALL_CAP, NEVER),            # what fits goes SMALL, the rest GROUP
    "group": (0, NEVER),
    "split": (0, 1),
    "small+split": (SMALL_CAP, SMALL_CAP + 1),
}

CASES = {
    # slices that start 1, 2 and 3 elements off a 16-byte boundary (17 = 16 + 1 whatever the element size), short and long
    "misaligned starts": [17, 17, 17, 600, 1, 17, 2, 1029, 17, 3, 17, 17, 531],
    # slices shorter than one 16-byte vector of the narrowest dtype, at every start
    "shorter than a vector": list(range(1, 16)) + [15, 14, 1, 1, 2, 2, 7],
    # a SMALL group that straddles the border of a tile (rows 2000 .. 2099), then a group too long for SMALL, then SMALL groups again
    "tile border": [100] * 21 + [600] + [100] * 3,
}
# one slice of each length around the SPLIT route's chunk, off the boundary, between two short ones
for _len in (SPLIT_CHUNK - 1, SPLIT_CHUNK, SPLIT_CHUNK + 1, 2 * SPLIT_CHUNK + 1):
    CASES[f"chunk {_len}"] = [3, _len, 5]


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def keys_of(counts):
    return np.repeat(np.arange(len(counts), dtype=np.int32), counts)


def values(rng, dt, counts):
    """a column for the groups: full-range values, with every third group drawn from three values of its own (ties), never 0 or NaN"""
    n = int(np.sum(counts))
    if dt.kind == "f":
        x = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n)).astype(dt)
    else:
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    x[x == 0] = 1
    off = offsets(counts)
    for g in range(0, len(counts), 3):
        pool = x[off[g]:off[g] + 3].copy()
        x[off[g]:off[g + 1]] = pool[rng.integers(0, len(pool), counts[g])]
    return x


def expected_routes(counts, pin):
    small_max, split_min = PINS[pin]
    mask = 0
    for c in counts:
        mask |= ROUTE_SMALL if c <= small_max else ROUTE_GROUP if c < split_min else ROUTE_SPLIT
    return mask


def models(x, counts):
    """{question: (answer per group, flags per group)} of the three models, for the questions the families share"""
    gid, G, off = keys_of(counts).astype(np.int64), len(counts), offsets(counts)
    s = qm.Sorted(x, gid, G)
    res = {}
    for which in (mm.SEL_LOWER, mm.SEL_UPPER):
        q, qf = s.quantiles([1], 2, which)
        res["median", which] = {"quantiles": (q[:, 0], qf[:, 0]), "median": mm.grouped(x, gid, G, which)}
    for name, num, order in (("min", 0, tm.ORDER_ASC), ("max", 1, tm.ORDER_DESC)):
        q, qf = s.quantiles([num], 1, mm.SEL_LOWER)
        v, _, vf = tm.topk(x, off, 1, order)
        res[name, order] = {"quantiles": (q[:, 0], qf[:, 0]), "topk": (v[:, 0], vf[:, 0])}
    return res


def generate():
    """(case name, dtype, counts, column), seeded per case and dtype"""
    for ci, (name, counts) in enumerate(CASES.items()):
        for di, dt in enumerate(DTYPES):
            yield name, dt, counts, values(np.random.default_rng(7000 + 10 * ci + di), dt, counts)
