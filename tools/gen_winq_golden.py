#!/usr/bin/env python3
"""Records the answers of pandas rolling(w, min_periods=1).quantile(q, interpolation='lower' | 'higher') for
tests/golden/winq_pandas_rolling.json (needs pandas; the tests read only the JSON).

Small integers held in float64, NaN-free, a couple of hundred rows with many ties; with and without a groupby column.  Only dyadic q
(0, 1/8, 1/4, 1/2, 3/4, 7/8, 1): q (len - 1) is then exact in binary floating point, so pandas' position and the library's
floor / ceil of num (len - 1) / den name the same row.  Every answer is per ROW, in row order, whatever the groups are.

    python tools/gen_winq_golden.py            # rewrites tests/golden/winq_pandas_rolling.json
"""
import json
import os

import numpy as np
import pandas as pd

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "winq_pandas_rolling.json")
QS = [(0, 8), (1, 8), (2, 8), (4, 8), (6, 8), (7, 8), (8, 8)]                 # (num, den)
WS = [1, 2, 5, 8, 21, 64]


def main():
    cases = []
    for seed, (n, ngroups) in enumerate([(150, 0), (120, 4), (120, 50)]):
        rng = np.random.default_rng(900 + seed)
        x = rng.integers(-5, 10, n).astype(np.float64)
        by = rng.integers(0, ngroups, n) if ngroups else None
        s = pd.Series(x)
        answers = {}
        for w in WS:
            for num, den in QS:
                for interp in ("lower", "higher"):
                    if by is None:
                        r = s.rolling(w, min_periods=1).quantile(num / den, interpolation=interp)
                    else:
                        r = s.groupby(by).rolling(w, min_periods=1).quantile(num / den, interpolation=interp).droplevel(0).sort_index()
                    assert len(r) == n and not r.isna().any() and np.all(r.to_numpy() == np.round(r.to_numpy()))
                    answers["%d_%d_%d_%s" % (w, num, den, interp)] = [int(v) for v in r.tolist()]
        cases.append({"x": [int(v) for v in x.tolist()], "by": None if by is None else [int(v) for v in by.tolist()], "answers": answers})
    with open(OUT, "w") as f:
        json.dump({"pandas": pd.__version__, "dtype": "float64", "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
