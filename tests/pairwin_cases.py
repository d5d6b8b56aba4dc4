"""The case list of the pair windows (covw / corrw / betaw and the running covs / corrs / betas), shared by the CPU test of the model
(tests/test_pairwin_model.py) and the GPU test (tests/test_gpu_pairwin.py).

A case is a pair of columns in the FLAT layout with its group starts (a flat case is one group) and the windows it is run with; a grouped
case also carries the row-layout columns and keys that produce that layout through aqg_groupby_build.  Data comes from the families of
tests/test_gpu_variance.py: "centred", "offset" and the dyadic floats are used for every op; "ramp" and "constant" only for cov, for
corr / beta on the short routes and for the exact-NaN rule (at long windows their windows are constant while the group is not: every
position would be ill-conditioned).  Ranges of x and y are kept within a factor of a few hundred of each other, so that beta's bound
(c Ry / Rx of its first term) stays under the ill-conditioned threshold.

The prefix pass of the pair windows keeps the scan of its tile aggregates in one workgroup (CHUNKED = false, pair_window.hip): it never
takes the chunked aggregate scan, so there is no case of more than 8192 tiles."""
from collections import namedtuple

import numpy as np

from test_gpu_variance import family

TS = 2048                                          # scan_dev.hpp: rows per tile
REG_W, LDS_W = 8, 64                               # the route switches (pair_route.hpp)
ROUTE_REG, ROUTE_LDS, ROUTE_PREFIX = 1, 2, 4
DIAGONAL = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64]
MIXED = [(np.int32, np.float64), (np.int64, np.float32), (np.uint8, np.int64), (np.uint64, np.int16)]
PAIRS = [(t, t) for t in DIAGONAL] + MIXED
SIZES = [1, 2, 2047, 2048, 2049, 6145]
BIG_N = 300_001

Case = namedtuple("Case", "name x y starts windows long_ok cut keys_row x_row y_row")


def windows_of(n):
    return sorted({1, 2, 3, 8, 9, 64, 65, 1000, n, n + 3})


def route_of(w, n):
    """the route a window op takes (w=None: a running op)"""
    if w is None:
        return ROUTE_PREFIX
    ww = min(int(w), n)
    return ROUTE_REG if ww <= REG_W else (ROUTE_LDS if ww <= LDS_W else ROUTE_PREFIX)


def pair_columns(rng, fam, tx, ty, n):
    """x from the family; y from a family of a comparable range (an 8-byte offset column beside a one-byte one would make beta's bound
    exceed the ill-conditioned threshold everywhere)"""
    tx, ty = np.dtype(tx), np.dtype(ty)

    def fam_of(t):                                             # (the 8-byte integer offset columns spread over 1e6, every other one over <= 1000)
        return "centred" if fam == "offset" and tx != ty and t.itemsize == 8 and t.kind in "iu" else fam
    return family(rng, fam_of(tx), tx, n), family(rng, fam_of(ty), ty, n)


def flat_case(name, x, y, windows=None, long_ok=True, cut=None):
    n = len(x)
    return Case(name, x, y, np.zeros(1, np.int64), windows if windows is not None else windows_of(n), long_ok, cut, None, None, None)


FAMS = ["centred", "offset"]


def flat_cases():
    rng = np.random.default_rng(20260)
    out = []
    for k, (tx, ty) in enumerate(PAIRS):                                        # every dtype pair at one tile + 1
        fam = FAMS[k % 2]
        x, y = pair_columns(rng, fam, tx, ty, 2049)
        out.append(flat_case("flat-%s-%s-%s-n2049" % (fam, np.dtype(tx).name, np.dtype(ty).name), x, y))
    for k, n in enumerate(SIZES):                                               # every size, the pairs in turn
        tx, ty = PAIRS[(3 * k + 1) % len(PAIRS)]
        fam = FAMS[(k + 1) % 2]
        x, y = pair_columns(rng, fam, tx, ty, n)
        out.append(flat_case("flat-%s-%s-%s-n%d" % (fam, np.dtype(tx).name, np.dtype(ty).name, n), x, y))
    x, y = pair_columns(rng, "offset", np.float64, np.float64, BIG_N)
    out.append(flat_case("flat-offset-float64-float64-n%d" % BIG_N, x, y, windows=[64, 65, 10_000]))
    for fam, dt in (("ramp", np.int32), ("ramp", np.float64), ("constant", np.int16), ("constant", np.float32)):
        x, y = family(rng, fam, dt, 2049), family(rng, fam, dt, 2049)
        out.append(flat_case("flat-%s-%s-n2049" % (fam, np.dtype(dt).name), x, y, long_ok=fam == "constant"))
    return out


def linear_cases():
    """y = a x + b with dyadic a, b: corr = +-1 and beta = a exactly"""
    rng = np.random.default_rng(20261)
    out = []
    for a, b, dt in ((0.75, -3.5, np.int32), (-2.5, 100.0, np.int16), (-0.125, 0.5, np.float32)):
        x = family(rng, "centred", dt, 2049)
        out.append((a, flat_case("linear-a%g-%s" % (a, np.dtype(dt).name), x, a * x.astype(np.float64) + b, windows=[2, 8, 9, 64, 65, 1000, 2052])))
    return out


def nonfinite_cases():
    """one NaN row, one Inf row, one 1e300 row whose products overflow: float64 columns, the bad row in y (x for the Inf)"""
    rng = np.random.default_rng(20262)
    out = []
    for what, v, col in (("nan", np.nan, 1), ("inf", np.inf, 0), ("1e300", 1e300, 1)):
        x, y = pair_columns(rng, "centred", np.float64, np.float64, 2 * TS + 100)
        cut = TS + 37
        (x, y)[col][cut] = v
        out.append(flat_case("nonfinite-%s" % what, x, y, windows=[3, 8, 9, 64, 65, 1000], cut=cut))
    return out


def layouts():
    """{name: group sizes}"""
    return {
        "ones": [1] * 70,
        "edges": [TS - 1, 1, 1, TS - 1, TS + 1, 300],                # starts at TS - 1, TS, TS + 1, 2 TS, 3 TS + 1
        "halo3": [2000, 20, 15, 30, 500],                            # the 63-row halo in front of row 2048 spans three groups and a fourth's tail
        "big-among-ones": [1] * 30 + [5000] + [1] * 30,
        "G1": [2 * TS + 5],
    }


def grouped_case(rng, name, sizes, tx, ty, fam):
    sizes = np.asarray(sizes, np.int64)
    n, G = int(sizes.sum()), len(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    # row layout: group g owns rows [starts[g], starts[g] + sizes[g]); the flat layout lists them by descending row id
    perm = np.concatenate([np.arange(s + c - 1, s - 1, -1) for s, c in zip(starts, sizes)]).astype(np.int64)      # flat position -> row
    keys_row = np.repeat((np.arange(G) * 7 + 3).astype(np.int32), sizes)
    x, y = pair_columns(rng, fam, tx, ty, n)
    x_row = np.empty_like(x); x_row[perm] = x
    y_row = np.empty_like(y); y_row[perm] = y
    return Case("grouped-%s-%s-%s-%s" % (name, fam, np.dtype(tx).name, np.dtype(ty).name), x, y, starts, windows_of(n), True, None, keys_row, x_row, y_row)


def grouped_cases():
    rng = np.random.default_rng(20263)
    out = []
    for k, (name, sizes) in enumerate(layouts().items()):
        for j in range(2):
            tx, ty = PAIRS[(5 * k + 7 * j + 2) % len(PAIRS)]
            out.append(grouped_case(rng, name, sizes, tx, ty, FAMS[(k + j) % 2]))
    return out


def offsets_of(case):
    return None if len(case.starts) == 1 else np.concatenate([case.starts, [len(case.x)]])
