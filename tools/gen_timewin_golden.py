#!/usr/bin/env python3
"""Records tests/golden/timewin_pandas.json: the answers of pandas' Series.rolling(Timedelta, closed="right" | "both") for
.sum() .mean() .min() .max() .count() on columns of at most 64 rows with ascending int64 nanosecond stamps that repeat.

The values are integer-valued doubles below 2^40, so that pandas' running add-and-remove is exact and its answers are the
mathematical ones.  Doubles are stored as float.hex().  Run from the repository root; needs pandas (recorded with 2.3.3)."""
import json
import os

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hexes(a):
    return [float(v).hex() for v in a]


def main():
    r = np.random.default_rng(20240229)
    cases = []
    for k, n in enumerate((1, 2, 3, 7, 16, 33, 63, 64)):
        for span in (1, 5, 17, 1000):
            steps = r.integers(0, 7, size=n) * (r.random(n) < 0.6)              # repeated stamps
            t = (10 ** 9 + np.cumsum(steps)).astype(np.int64)
            x = r.integers(-2 ** 39, 2 ** 39, size=n).astype(np.float64)
            s = pd.Series(x, index=pd.to_datetime(t, unit="ns"))
            for closed in ("right", "both"):
                roll = s.rolling(pd.Timedelta(span, unit="ns"), closed=closed)
                cases.append({"name": "n%d-s%d-%s" % (n, span, closed), "t": [int(v) for v in t], "x": hexes(x), "span": span, "closed": closed,
                              "sum": hexes(roll.sum().to_numpy()), "mean": hexes(roll.mean().to_numpy()), "min": hexes(roll.min().to_numpy()),
                              "max": hexes(roll.max().to_numpy()), "count": [int(v) for v in roll.count().to_numpy()]})
    out = os.path.join(ROOT, "tests", "golden", "timewin_pandas.json")
    with open(out, "w") as f:
        json.dump({"pandas": pd.__version__, "cases": cases}, f, indent=0)
    print(out, len(cases), "cases", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
