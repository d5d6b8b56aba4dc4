"""The cases of the ranking tests (tests/test_rank_model.py on the CPU, tests/test_gpu_rank.py on the device), placed on geometry
read from the code: TILE flat positions per workgroup of the SMALL route and SMALL_CAP, its largest group (csrc/select_radix.hpp);
SMALL_MAX, the default of AQG_SELECT_SMALL_MAX (csrc/ctx.hip); ET = EB * EPT sorted entries per workgroup of the SORTED route's
kernels (csrc/rank.hip; the GPU tests hold aqg_rank_last's answer to it).

A case is a column in the layout scanned (x, slices from `starts`) and, for a grouped case, the row-layout column and keys that give
that flat layout: group g owns rows [starts[g], starts[g+1]) and the flat layout lists them by descending row id."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constants(path, names):
    src = open(os.path.join(ROOT, "aquery2_amd", "csrc", path)).read()
    env = {}
    for name in names:
        expr = re.search(r"constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*([^;]+);" % name, src).group(1)
        env[name] = int(eval(expr, {}, dict(env)))
    return [env[k] for k in names]


TILE, SMALL_CAP = _constants("select_radix.hpp", ["TILE", "SMALL_CAP"])
EB, EPT, ET = _constants("rank.hip", ["EB", "EPT", "ET"])
SMALL_MAX = int(re.search(r'unum\("AQG_SELECT_SMALL_MAX",\s*(\d+)\)', open(os.path.join(ROOT, "aquery2_amd", "csrc", "ctx.hip")).read()).group(1))
assert ET == EB * EPT and SMALL_MAX <= SMALL_CAP

Case = namedtuple("Case", "name dtype x starts keys_row x_row ks")

ALL_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.bool_, np.float32, np.float64]
WIDE_DTYPES = [np.int32, np.uint8, np.float64]                  # the dtypes that also take the sizes of several emit tiles
FLAT_N = [1, 2, 3, 64, 65, SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, ET - 1, ET, ET + 1]
FLAT_WIDE_N = [2 * ET - 1, 2 * ET, 2 * ET + 1, 3 * ET + 5]      # 2 ET: the one-workgroup sort's last size; beyond it the digit passes
BIG_N = 70_000                                                   # one column of many emit tiles (first statement only: c^2 is out of reach)


def column(rng, dtype, n, kind):
    """n values of `dtype`: "ties" (few distinct values, the type's ends among them), "distinct" (no two equal where the type has the
    room), "equal" (one value), "special" (floating: both zeros, NaNs of several payloads and both signs, both infinities among few values)"""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return np.ones(n, np.bool_) if kind == "equal" else rng.integers(0, 2, size=n).astype(np.bool_)
    if kind == "equal":
        return np.full(n, 3, dt)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        if kind == "distinct" and n <= int(info.max) - int(info.min):
            if dt.itemsize >= 4:                                # next to the type's end: 64-bit values above 2^53, one apart
                return (np.uint64(int(info.max) - n) + rng.permutation(n).astype(np.uint64)).astype(dt)
            return (int(info.min) + rng.permutation(int(info.max) - int(info.min) + 1)[:n]).astype(dt)
        pool = np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1, info.max // 2], dtype=dt)
        if dt.itemsize == 8:
            pool = np.concatenate([pool, np.array([2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2], dt)])      # equal as doubles, distinct as integers
        return pool[rng.integers(0, len(pool), size=n)]
    bits = np.uint32 if dt.itemsize == 4 else np.uint64
    if kind == "distinct":
        return rng.permutation(n).astype(dt) - dt.type(n // 2)
    pool = np.array([-1.5, 0.0, -0.0, 2.0, np.inf, -np.inf, 1e-30, -1e-30], dt)
    if kind == "special":
        hi = 0x7fc00000 if dt.itemsize == 4 else 0x7ff8000000000000
        sign = 1 << (dt.itemsize * 8 - 1)
        nans = np.array([hi, hi | 1, hi | sign, (hi | sign) + 5, (hi & (hi << 1)) | 7], bits).view(dt)      # the last: a signalling payload
        assert np.isnan(nans).all()
        pool = np.concatenate([pool, nans])
    return pool[rng.integers(0, len(pool), size=n)]


def runs_column(dtype, lengths, rng):
    """a column whose sorted order has tie runs of exactly `lengths` (ascending values 0, 1, ...), rows shuffled"""
    v = np.repeat(np.arange(len(lengths)), lengths)
    dt = np.dtype(dtype)
    if dt.kind in "iu" and dt.itemsize == 1:
        assert len(lengths) <= 127
    return rng.permutation(v).astype(dt)


def edge_runs(n):
    """tie runs that begin on, end on and span the emit-tile edges of a slice of n = 3 ET + 5 sorted entries"""
    assert n == 3 * ET + 5
    lengths = [ET - 2, 2, 5, ET - 5, ET + 3, 1, 1]             # heads at 0, ET - 2, ET (on the edge), ET + 5, 2 ET (on), 3 ET + 3, 3 ET + 4
    assert sum(lengths) == n
    return lengths


def _ks(sizes):
    c = int(max(sizes))
    ks = {1, 2, 7, c, c + 1}
    if c > 1:
        ks.add(c - 1)
    s = int(min(sizes))
    ks.update({s, s + 1})
    return tuple(sorted(k for k in ks if k >= 1))


def flat_case(name, x):
    return Case(name, x.dtype, x, np.zeros(1, np.int64), None, None, _ks([len(x)]))


def grouped_case(name, sizes, x):
    sizes = np.asarray(sizes, np.int64)
    n, G = int(sizes.sum()), len(sizes)
    assert len(x) == n
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    perm = np.concatenate([np.arange(s + c - 1, s - 1, -1) for s, c in zip(starts, sizes)]).astype(np.int64)      # flat position -> row
    keys_row = np.repeat((np.arange(G) * 7 + 3).astype(np.int32), sizes)
    x_row = np.empty_like(x)
    x_row[perm] = x
    return Case(name, x.dtype, x, starts, keys_row, x_row, _ks(sizes))


@functools.lru_cache(maxsize=None)
def flat_cases():
    rng = np.random.default_rng(1907)
    cases = []
    for dt in ALL_DTYPES:
        name = np.dtype(dt).name
        kinds = ["ties", "distinct", "equal"] + (["special"] if np.dtype(dt).kind == "f" else [])
        for n in FLAT_N + (FLAT_WIDE_N if dt in WIDE_DTYPES else []):
            for kind in kinds:
                if kind == "equal" and n not in (3, SMALL_MAX + 1, ET + 1, 3 * ET + 5):
                    continue
                cases.append(flat_case("flat-%s-n%d-%s" % (name, n, kind), column(rng, dt, n, kind)))
        if dt in WIDE_DTYPES:
            cases.append(flat_case("flat-%s-edge_runs" % name, runs_column(dt, edge_runs(3 * ET + 5), rng)))
    return cases


def layouts():
    sm = SMALL_MAX
    return {
        "small_sizes": [1, 2, 3, sm - 1, sm, 1, sm, 2, 3, 3, sm - 1, 1],                    # SMALL only
        "threshold": [1, 2, 3, sm - 1, sm, sm + 1, 2, sm + 1, sm, 1],                       # both sides of the switch
        "straddle": [100] * 45,                                                              # SMALL groups across the 2048-position tiles
        "three_tiles": [1, 1, 3 * ET + 5, 1, 1, 100],                                        # one group over three emit tiles beside groups of one row
        "singletons": [1] * (TILE + 52),                                                     # every row its own group
        "one_group": [ET + 450],
        "g255": [7] * 255, "g256": [7] * 256, "g257": [7] * 257,
        "big_on_edges": [ET, sm + 1, ET - (sm + 1), 2 * ET, sm + 44],                        # SORTED only: group starts on emit-tile edges
        "mixed": [sm + 1, 3, 2 * ET + 1, sm, 1, sm + 2, 2, ET, 50, 2 * sm],                  # both routes in one call
    }


GROUPED_DTYPES = [np.int32, np.float64, np.uint8, np.uint64, np.float32, np.int16]


@functools.lru_cache(maxsize=None)
def grouped_cases():
    rng = np.random.default_rng(1908)
    cases = []
    for lname, sizes in layouts().items():
        n = int(np.sum(sizes))
        for dt in GROUPED_DTYPES:
            if dt not in WIDE_DTYPES and lname not in ("threshold", "mixed"):
                continue
            kinds = ["ties", "distinct"] + (["special"] if np.dtype(dt).kind == "f" else [])
            for kind in kinds:
                cases.append(grouped_case("grouped-%s-%s-%s" % (lname, np.dtype(dt).name, kind), sizes, column(rng, dt, n, kind)))
        cases.append(grouped_case("grouped-%s-int32-equal" % lname, sizes, column(rng, np.int32, n, "equal")))
    # the big group of three_tiles with its tie runs on the emit-tile edges (it is the only SORTED group: its entries start at 0), and a
    # group whose last run ends exactly at the group's end, on an edge, before a group that opens with the same value
    sizes = layouts()["three_tiles"]
    for dt in (np.int32, np.float64):
        x = column(rng, dt, int(np.sum(sizes)), "ties")
        x[2:2 + 3 * ET + 5] = runs_column(dt, edge_runs(3 * ET + 5), rng)
        cases.append(grouped_case("grouped-three_tiles-%s-edge_runs" % np.dtype(dt).name, sizes, x))
    sizes = [ET, ET + 1]
    x = np.concatenate([runs_column(np.int32, [ET - 300, 300], rng), runs_column(np.int32, [0, 400, ET - 399], rng)])
    cases.append(grouped_case("grouped-run_ends_group-int32-runs", sizes, x))
    return cases


@functools.lru_cache(maxsize=None)
def big_case():
    rng = np.random.default_rng(1909)
    return flat_case("flat-int64-n%d-ties" % BIG_N, rng.integers(-500, 500, size=BIG_N).astype(np.int64))


def all_cases():
    return flat_cases() + grouped_cases()
