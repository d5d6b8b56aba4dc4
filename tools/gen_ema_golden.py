#!/usr/bin/env python3
"""Records the answers of pandas ewm(...).mean() for tests/golden/ema_pandas.json (needs pandas; the tests read only the JSON).

Short float64 columns (at most 64 rows, NaN-free) with
    alpha cases:  ewm(alpha=a, adjust=False).mean()  and  ewm(alpha=a, adjust=True).mean()
    times cases:  ewm(halflife=h, times=t).mean()      (adjusted: pandas offers `times` with adjust=True only)
Doubles are stored as float.hex() strings, so the file holds them bit for bit.

pandas evaluates the alpha cases sequentially in doubles -- one bracketing of the recurrence -- so the model must agree with it within
the bounds of DESIGN.md section 4.15.  For the times cases pandas forms its weights its own way (0.5 ** (dt / halflife) folded into a
running weighted mean), so no derived bound covers the difference: this script records, as "times_ratio", the largest observed
|pandas - model| / (u (i + 2) M_i) over all times cases, u = 2^-53, with the model fed decay[i] = exp2(-(t[i] - t[i-1]) / halflife) as
recorded next to the answers; the test asserts 4 x that number.

    python tools/gen_ema_golden.py            # rewrites tests/golden/ema_pandas.json
"""
import json
import os
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ema_model as em  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ema_pandas.json")
ALPHAS = [1.0, 0.5, 0.25, 0.1, 2.0 / 11.0, 2.0 ** -20]


def hx(a):
    return [float(v).hex() for v in a]


def main():
    rng = np.random.default_rng(4242)
    alpha_cases, times_cases, worst = [], [], 0.0
    for k, n in enumerate([1, 2, 3, 8, 17, 33, 64, 64]):
        x = rng.normal(size=n) * 10.0 ** rng.integers(-2, 3, size=n)
        s = pd.Series(x)
        for a in ALPHAS:
            alpha_cases.append({"x": hx(x), "alpha": float(a).hex(),
                                "recursive": hx(s.ewm(alpha=a, adjust=False).mean().to_numpy()),
                                "adjusted": hx(s.ewm(alpha=a, adjust=True).mean().to_numpy())})
    for k, n in enumerate([1, 2, 5, 16, 40, 64, 64, 64]):
        x = rng.normal(size=n) * 10.0 ** rng.integers(-2, 3, size=n)
        t = np.cumsum(rng.integers(1, 5_000_000_000, size=n)).astype(np.int64)        # nanoseconds, ascending, up to 5 s apart
        h = int([1_000_000_000, 250_000_000, 7_000_000_000, 123_456_789][k % 4])
        got = pd.Series(x).ewm(halflife=pd.Timedelta(h, "ns"), times=pd.DatetimeIndex(t)).mean().to_numpy()
        decay = np.ones(n)
        decay[1:] = np.exp2(-(np.diff(t).astype(np.float64) / float(h)))
        r = em.exact_ema(x, None, em.ADJUSTED, decay=decay)
        pos = np.arange(n)
        worst = max(worst, float(np.max(np.abs(got - r.y) / (em.U * (pos + 2) * r.M))))
        times_cases.append({"x": hx(x), "t_ns": [int(v) for v in t], "halflife_ns": h, "decay": hx(decay), "adjusted": hx(got)})
    doc = {"pandas": pd.__version__,
           "note": "times_ratio: the largest |pandas - model| / (2^-53 (i + 2) M_i) this script observed over the times cases "
                   "(tools/gen_ema_golden.py); the test allows 4 x that",
           "times_ratio": worst, "alpha_cases": alpha_cases, "times_cases": times_cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes; times_ratio", worst)


if __name__ == "__main__":
    main()
