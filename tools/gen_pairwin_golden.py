#!/usr/bin/env python3
"""Record pandas' answers for the pair windows into tests/golden/pairwin_pandas.json (needs pandas; the tests need only the file).

Columns of integers within +-1000, n <= 200, per group: rolling(w, min_periods=1).cov(ddof=0) / .corr() and expanding(1).cov(ddof=0) /
.corr(), beta as cov / var(ddof=0).  A value is recorded only where the exact Vx Vy > 0 (beta: Vx > 0) and is null elsewhere -- pandas
answers NaN, +-inf or rounding noise there.  While recording, every value is held to the exact model (tests/pair_moments.py) within
PANDAS_ERR (1 + |value|), just above pandas' own error on these inputs (online updates of raw sums in double), which is printed at the
end: 1.2e-12 with pandas 2.3.  The golden test allows a hundred times as much."""
import json
import os
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pair_moments as pm  # noqa: E402

PANDAS_ERR = 1e-11
WINDOWS = [1, 2, 3, 5, 64, 65, 150]


def columns():
    rng = np.random.default_rng(777)
    out = []
    for name, sizes in (("one-group", [200]), ("groups", [1, 2, 70, 3, 66, 58]), ("short", [5, 1, 1, 9])):
        n = sum(sizes)
        x = rng.integers(-1000, 1000, n, endpoint=True)
        y = (x * rng.integers(-2, 3) + rng.integers(-300, 300, n)).clip(-1000, 1000)
        out.append((name, sizes, x, y))
    return out


def pandas_answers(x, y, sizes, w):
    gid = np.repeat(np.arange(len(sizes)), sizes)
    df = pd.DataFrame({"g": gid, "x": x.astype(np.float64), "y": y.astype(np.float64)})
    res = {"cov": [], "corr": [], "beta": []}
    for _, grp in df.groupby("g", sort=False):
        roll = (lambda s: s.expanding(1)) if w is None else (lambda s: s.rolling(w, min_periods=1))
        cov = roll(grp["x"]).cov(grp["y"], ddof=0)
        res["cov"] += cov.tolist()
        res["corr"] += roll(grp["x"]).corr(grp["y"]).tolist()
        res["beta"] += (cov / roll(grp["x"]).var(ddof=0)).tolist()
    return res


def main():
    cases = []
    worst = 0.0
    for name, sizes, x, y in columns():
        off = np.concatenate([[0], np.cumsum(sizes)])
        ex = pm.PairExact(x, y, off)
        for w in [None] + WINDOWS:
            m = ex.moments(w)
            got = pandas_answers(x, y, sizes, w)
            keep = {"cov": ~(m["vx0"] | m["vy0"]), "corr": ~(m["vx0"] | m["vy0"]), "beta": ~m["vx0"]}
            want = {"cov": m["C"], "corr": m["corr"], "beta": m["beta"]}
            rec = {}
            for k in ("cov", "corr", "beta"):
                g = np.asarray(got[k], dtype=np.float64)
                err = np.abs(g - want[k])[keep[k]] / (1 + np.abs(want[k][keep[k]]))
                if len(err):
                    worst = max(worst, float(err.max()))
                    assert err.max() <= PANDAS_ERR, (name, w, k, float(err.max()))
                rec[k] = [float(v) if ok else None for v, ok in zip(g, keep[k])]
            cases.append({"name": name, "w": w, "sizes": list(map(int, sizes)), "x": x.tolist(), "y": y.tolist(), **rec})
    path = os.path.join(ROOT, "tests", "golden", "pairwin_pandas.json")
    with open(path, "w") as f:
        json.dump({"pandas": pd.__version__, "cases": cases}, f, separators=(",", ":"))
    print("wrote %s: %d cases, %d bytes, worst pandas error %.3g" % (path, len(cases), os.path.getsize(path), worst))


if __name__ == "__main__":
    main()
