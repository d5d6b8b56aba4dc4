#!/usr/bin/env python3
"""Records the answers of pandas Series.rank / groupby().rank for tests/golden/rank_pandas.json (needs pandas and scipy; the tests
read only the JSON).

A few dozen slices of at most 40 rows, flat and by group, every method, both orders:
    MIN / MAX / DENSE / FIRST / AVERAGE   rank(method=..., ascending=..., na_option='bottom' (ASC) | 'top' (DESC))
    CUME_DIST                             rank(method='max', pct=True, ...)
    PERCENT, NTILE(k)                     pandas has neither: written from their formulas over pandas' own 'min' resp. 'first' ranks
                                          (NaN-free ascending slices are cross-checked with scipy.stats.rankdata first)
Columns are stored as the bit patterns of their elements, doubles in the answers as their shortest decimal form, which reads back exactly: the file holds
both bit for bit.  Nothing of the project's model enters the file.

    python tools/gen_rank_golden.py            # rewrites tests/golden/rank_pandas.json
"""
import json
import os

import numpy as np
import pandas as pd
from scipy.stats import rankdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "rank_pandas.json")
PANDAS_METHODS = ["min", "max", "dense", "first", "average"]
KS = [1, 3, 5, 40, 41]


def column(rng, dt, n):
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, size=n).astype(np.bool_)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        pool = [info.min, info.max, 0, 1, 2, info.max - 1]
        if dt.itemsize == 8:
            pool += [2 ** 53, 2 ** 53 + 1]
        return np.array(pool, dt)[rng.integers(0, len(pool), size=n)]
    bits = np.uint32 if dt.itemsize == 4 else np.uint64
    hi = 0x7fc00000 if dt.itemsize == 4 else 0x7ff8000000000000
    sign = 1 << (dt.itemsize * 8 - 1)
    pool = np.concatenate([np.array([-1.5, 0.0, -0.0, 2.0, np.inf, -np.inf, 0.25], dt), np.array([hi, hi | 1, hi | sign], bits).view(dt)])
    return pool[rng.integers(0, len(pool), size=n)]


def ntile(first, c, k):
    q, r, o = c // k, c % k, first - 1
    wide = r * (q + 1)
    return np.where(o < wide, o // (q + 1), r + (o - wide) // np.maximum(q, 1)) + 1


def record(x, sizes):
    n = len(x)
    gid = np.repeat(np.arange(len(sizes)), sizes)
    c = np.repeat(np.asarray(sizes, np.int64), sizes)
    xs = x.astype(np.uint8) if x.dtype == np.bool_ else x
    df = pd.DataFrame({"g": gid, "x": xs})
    res = {}
    for oname, asc in (("asc", True), ("desc", False)):
        na = "bottom" if asc else "top"
        r = {m: df.groupby("g")["x"].rank(method=m, ascending=asc, na_option=na).to_numpy() for m in PANDAS_METHODS}
        if len(sizes) == 1:                                  # the flat form answers the same
            for m in PANDAS_METHODS:
                assert np.array_equal(r[m], df["x"].rank(method=m, ascending=asc, na_option=na).to_numpy())
        ints = {m: r[m].astype(np.int64) for m in ("min", "max", "dense", "first")}
        for m in ints:
            assert np.array_equal(ints[m].astype(np.float64), r[m])
        if asc and x.dtype.kind != "f":                      # scipy's statement of the underlying ranks, where it has one
            for s, e in zip(np.cumsum([0] + list(sizes[:-1])), np.cumsum(sizes)):
                for m, sm in (("min", "min"), ("max", "max"), ("dense", "dense"), ("first", "ordinal"), ("average", "average")):
                    assert np.array_equal(rankdata(xs[s:e], method=sm), r[m][s:e]), (m, xs[s:e])
        cume = df.groupby("g")["x"].rank(method="max", ascending=asc, na_option=na, pct=True).to_numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            percent = np.where(c == 1, 0.0, (ints["min"] - 1).astype(np.float64) / (c - 1).astype(np.float64))
        res[oname] = {"min": ints["min"].tolist(), "max": ints["max"].tolist(), "dense": ints["dense"].tolist(), "first": ints["first"].tolist(),
                      "average": [float(v) for v in r["average"]], "percent": [float(v) for v in percent],
                      "cume_dist": [float(v) for v in cume],
                      "ntile": {str(k): ntile(ints["first"], c, k).tolist() for k in KS}}
    bits = x.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])
    return {"dtype": x.dtype.name, "bits": [int(v) for v in bits], "sizes": [int(s) for s in sizes], "n": n, "results": res}


def main():
    rng = np.random.default_rng(2024)
    layouts = [[1], [2], [17], [40], [1, 2, 3, 7, 1, 12], [5] * 6, [39, 1]]
    cases = []
    for dt in (np.float64, np.float32, np.int32, np.int8, np.uint64, np.int64, np.uint16, np.bool_):
        for sizes in layouts:
            if dt not in (np.float64, np.int32) and (len(sizes) != 6 and sizes != [17] or dt != np.float32 and sizes == [5] * 6):
                continue
            cases.append(record(column(rng, dt, int(sum(sizes))), sizes))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"pandas": pd.__version__, "ks": KS, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d slices, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
