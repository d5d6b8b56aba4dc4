#!/usr/bin/env python3
"""Records the answers of pandas for tests/golden/wj_pandas.json (needs pandas; the tests read only the JSON).

The window join stated independently: `merge` of the probe rows with the build rows on the key, a filter on the interval around the
probe row's `on`, `groupby(probe row).agg`.  A dozen pairs of sides, NaN-free, int64 or float64 `on` with many duplicate times, with
and without a key column; two spans and the four combinations of open and closed sides.  Per probe row: count and sum of an
int64 column and sum, min, max and mean of a float64 column whose values are small multiples of 1/8, so that every sum is exact in
double whatever order pandas adds in (its grouped sum is compensated, not the window order).  A probe row without rows in its window is absent from
the groupby: count 0, the other answers null.

    python tools/gen_wj_golden.py            # rewrites tests/golden/wj_pandas.json
"""
import json
import os

import numpy as np
import pandas as pd

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "wj_pandas.json")


def main():
    sides = []
    for seed in range(12):
        rng = np.random.default_rng(800 + seed)
        nb, npr = int(rng.integers(24, 40)), int(rng.integers(12, 20))
        dom = int(rng.integers(6, 14))
        fp = seed % 2 == 1
        bon, pon = rng.integers(-dom, dom, nb), rng.integers(-dom - 2, dom + 2, npr)
        if fp:
            bon, pon = bon / 4.0, pon / 4.0
        by = seed % 3 != 0
        bby, pby = (rng.integers(0, 4, nb), rng.integers(0, 5, npr)) if by else (np.zeros(nb, np.int64), np.zeros(npr, np.int64))
        xi, xf = rng.integers(-10 ** 6, 10 ** 6, nb), rng.integers(-400, 400, nb) / 8.0
        before, after = [(2.0, 1.0), (0.75, 2.5), (5.0, 0.5)][seed % 3]
        right = pd.DataFrame({"by": bby, "b_on": bon, "xi": xi, "xf": xf})
        left = pd.DataFrame({"by": pby, "p_on": pon, "probe": np.arange(npr)})
        pairs = left.merge(right, on="by")
        answers = {}
        for open_lo in (False, True):
            for open_hi in (False, True):
                d_lo, d_hi = pairs["p_on"] - pairs["b_on"], pairs["b_on"] - pairs["p_on"]
                front = (pairs["b_on"] < pairs["p_on"]) & ((d_lo < before) if open_lo else (d_lo <= before))
                behind = (pairs["b_on"] > pairs["p_on"]) & ((d_hi < after) if open_hi else (d_hi <= after))
                inside = pairs[(pairs["b_on"] == pairs["p_on"]) | front | behind]
                agg = inside.groupby("probe").agg(count=("xi", "size"), isum=("xi", "sum"), fsum=("xf", "sum"), fmin=("xf", "min"),
                                                  fmax=("xf", "max"), fmean=("xf", "mean"))
                agg = agg.reindex(np.arange(npr))
                rec = {"count": [int(c) if c == c else 0 for c in agg["count"].tolist()]}
                rec["isum"] = [int(v) if v == v else None for v in agg["isum"].tolist()]
                for col in ("fsum", "fmin", "fmax", "fmean"):                  # (repr of a double reads back to the same double)
                    rec[col] = [float(v) if v == v else None for v in agg[col].tolist()]
                answers["%d" % ((1 if open_lo else 0) | (2 if open_hi else 0))] = rec
        sides.append({"dtype": "float64" if fp else "int64", "by": by, "before": before, "after": after, "build_on": bon.tolist(),
                      "probe_on": pon.tolist(), "build_by": bby.tolist(), "probe_by": pby.tolist(), "xi": xi.tolist(), "xf": xf.tolist(),
                      "answers": answers})
    with open(OUT, "w") as f:
        json.dump({"pandas": pd.__version__, "sides": sides}, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
