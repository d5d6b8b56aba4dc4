"""The cases of the exponential moving averages, shared by the CPU tests of the model (test_ema_model.py: every planted mistake is
refused by some case, and no case hides one behind its bound) and the GPU tests (test_gpu_ema.py: the device against the model).

The tile geometry is read from the code (csrc/scan_dev.hpp): TS = SB * IT rows per tile, IT rows per lane, CH tile aggregates per
chunk of launch_agg_scan.  A case is a column in the FLAT layout with its slice starts; a grouped case also carries the row-layout
columns and keys that aqg_groupby_build turns into exactly that layout (group g's rows are contiguous in the table, and the flat layout
lists them by DESCENDING row id, so the two layouts differ inside every group of more than one row).
"""
import os
import re
from collections import namedtuple

import numpy as np

import ema_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry():
    src = open(os.path.join(ROOT, "aquery2_amd", "csrc", "scan_dev.hpp")).read()
    env = {}
    for name in ("SB", "IT", "TS", "CH"):
        expr = re.search(r"constexpr\s+(?:int|uint32_t)\s+%s\s*=\s*([^;]+);" % name, src).group(1)
        env[name] = int(eval(expr, {}, dict(env)))
    return env["SB"], env["IT"], env["TS"], env["CH"]


SB, IT, TS, CH = _geometry()

Case = namedtuple("Case", "name kind dtype x starts mode alpha decay keys_row x_row decay_row")

FLAT_N = [1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097]
BIG_N = [CH * TS - 1, CH * TS, CH * TS + 1, 2 * CH * TS + 3]          # the aggregate scan's second round (wide_ema is their reference)
ALPHAS = [1.0, 0.5, 0.1, 2.0 ** -20]
ALPHA_TINY = 2.0 ** -52                                               # at the small n only
GRID_DTYPES = [np.int8, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64]
OTHER_DTYPES = [np.uint8, np.int16]                                   # the remaining numeric types, at three n
OTHER_N = [9, 2049, 4097]
DECAY_KINDS = ["uniform", "zeros", "ones", "denormal"]


def column(rng, dtype, n):
    """values over the type's whole range (64-bit integers beyond 2^53: the conversion rounds; floating: a few decades, both signs)"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, size=n)).astype(dt)
    info = np.iinfo(dt)
    if dt.itemsize == 8:
        lo, hi = (info.min // 2, info.max // 2) if dt.kind == "i" else (0, info.max // 2)
        v = rng.integers(lo, hi, size=n, dtype=dt, endpoint=True)
        return v if dt.kind == "i" else (v * np.uint64(2) + np.uint64(1)).astype(dt)       # uint64: beyond 2^63 too
    v = rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
    if n >= 2 and v[1] == v[0]:
        v[1] ^= 1                                                       # two equal rows average to themselves under any weights
    return v


def decay_column(rng, kind, n):
    if kind == "ones":
        return np.ones(n)
    if kind == "denormal":                                              # two factors make a denormal product, three underflow to 0
        return np.full(n, 1e-160)
    d = rng.uniform(0.0, 1.0, size=n)
    if kind == "zeros":                                                 # hard restarts inside a slice
        d[rng.uniform(size=n) < 0.05] = 0.0
    return d


def flat_case(rng, dtype, n, mode, alpha=None, kind=None, tag="flat"):
    x = column(rng, dtype, n)
    dec = decay_column(rng, kind, n) if kind else None
    what = ("alpha=%g" % alpha) if kind is None else kind
    return Case("%s-%s-n%d-m%d-%s" % (tag, np.dtype(dtype).name, n, mode, what), "flat", np.dtype(dtype), x, None, mode, alpha, dec, None, None, None)


def flat_cases():
    rng = np.random.default_rng(20240611)
    out, k = [], 0
    for dtype in GRID_DTYPES:
        for n in FLAT_N:
            for mode in (em.RECURSIVE, em.ADJUSTED):
                out.append(flat_case(rng, dtype, n, mode, alpha=ALPHAS[k % 4])); k += 1
                out.append(flat_case(rng, dtype, n, mode, kind=DECAY_KINDS[k % 4])); k += 1
    for dtype in OTHER_DTYPES:
        for n in OTHER_N:
            for mode in (em.RECURSIVE, em.ADJUSTED):
                out.append(flat_case(rng, dtype, n, mode, alpha=ALPHAS[k % 4])); k += 1
                out.append(flat_case(rng, dtype, n, mode, kind=DECAY_KINDS[k % 4])); k += 1
    # every alpha at one dtype and a few n, the tiny one at the small n
    for n in (9, 65, 513, 2049):
        for mode in (em.RECURSIVE, em.ADJUSTED):
            for alpha in ALPHAS + ([ALPHA_TINY] if n < TS else []):
                out.append(flat_case(rng, np.float64, n, mode, alpha=alpha, tag="alphas"))
                out.append(flat_case(rng, np.int32, n, mode, alpha=alpha, tag="alphas"))
    return out


# ---- grouped layouts -----------------------------------------------------------------------------------------------------------------
def _sizes_from_starts(starts, n):
    s = list(starts) + [n]
    return [s[i + 1] - s[i] for i in range(len(starts))]


def layouts():
    """{name: group sizes}: starts on tile borders, on lane-block borders (multiples of IT) and one row either side of them; a group
    over three tiles beside groups of one row; one group; every row its own; G on both sides of 256 (aqg_grouped_flatten's routes)"""
    rng = np.random.default_rng(7)
    edges = [0, IT - 1, IT, IT + 1, 2 * IT, 2 * IT + 1, TS - 1, TS, TS + 1, TS + IT, 2 * TS - 1, 2 * TS, 2 * TS + 1, 2 * TS + IT]
    lay = {
        "edges": _sizes_from_starts(edges, 2 * TS + 150),
        "three_tiles": [1, 1, 3 * TS + 5, 1, 1, 100],
        "one_group": [TS + 450],
        "singletons": [1] * (TS + 52),
    }
    for G in (255, 256, 257):
        lay["G%d" % G] = [int(v) for v in rng.integers(1, 20, size=G)]
    return lay


def grouped_case(rng, name, sizes, dtype, mode, alpha=None, kind=None, poison=None):
    sizes = np.asarray(sizes, np.int64)
    n, G = int(sizes.sum()), len(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    # row layout: group g owns rows [starts[g], starts[g] + sizes[g]); the flat layout lists them by descending row id
    perm = np.concatenate([np.arange(s + c - 1, s - 1, -1) for s, c in zip(starts, sizes)]).astype(np.int64)      # flat position -> row
    keys_row = np.repeat((np.arange(G) * 7 + 3).astype(np.int32), sizes)
    x = column(rng, dtype, n)
    dec = decay_column(rng, kind, n) if kind else None
    if poison:
        poison(x, dec, starts, sizes)
    x_row = np.empty_like(x); x_row[perm] = x
    dec_row = None
    if dec is not None:
        dec_row = np.empty_like(dec); dec_row[perm] = dec
    what = ("alpha=%g" % alpha) if kind is None else kind
    return Case("grouped-%s-%s-m%d-%s" % (name, np.dtype(dtype).name, mode, what), "grouped", np.dtype(dtype), x, starts, mode, alpha, dec, keys_row, x_row, dec_row)


def _poison_nan(x, dec, starts, sizes):
    x[starts[1] + 50] = np.nan


def _poison_inf(x, dec, starts, sizes):
    x[starts[1] + 3] = np.inf
    x[starts[1] + 600] = -np.inf


def _poison_decay(x, dec, starts, sizes):
    dec[starts[1]] = 7.0                       # a first row's decay is never read: this one poisons nothing
    dec[starts[1] + 20] = 1.5
    dec[starts[1] + 40] = -0.1
    dec[starts[1] + 60] = np.nan
    dec[starts[2]] = np.nan                    # nor does this one


def grouped_cases():
    rng = np.random.default_rng(977)
    out, k = [], 0
    dts = [np.float64, np.int32, np.int64, np.float32, np.uint8, np.uint64, np.int16]
    for name, sizes in layouts().items():
        for mode in (em.RECURSIVE, em.ADJUSTED):
            out.append(grouped_case(rng, name, sizes, dts[k % len(dts)], mode, alpha=[0.5, 0.1, 2.0 ** -20][k % 3])); k += 1
            out.append(grouped_case(rng, name, sizes, dts[k % len(dts)], mode, kind=DECAY_KINDS[k % 3])); k += 1
    # a poisoned group (it crosses a tile edge) between two tame ones
    tame = [TS - 548, 1000, 1500]
    for mode in (em.RECURSIVE, em.ADJUSTED):
        out.append(grouped_case(rng, "poison_nan", tame, np.float64, mode, alpha=0.1, poison=_poison_nan))
        out.append(grouped_case(rng, "poison_inf", tame, np.float32, mode, alpha=0.5, poison=_poison_inf))
        out.append(grouped_case(rng, "poison_inf_decay", tame, np.float64, mode, kind="zeros", poison=_poison_inf))
        out.append(grouped_case(rng, "poison_decay", tame, np.int32, mode, kind="uniform", poison=_poison_decay))
    return out


def all_cases():
    return flat_cases() + grouped_cases()


def reference(case):
    """ema_model.Reference of a case: exact for slices of up to EXACT_MAX rows and for poisoned ones, extended precision beyond"""
    return em.reference_ema(case.x, case.starts, case.mode, alpha=case.alpha, decay=case.decay)
