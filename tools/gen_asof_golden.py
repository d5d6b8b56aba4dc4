#!/usr/bin/env python3
"""Records the answers of pandas merge_asof for tests/golden/asof_merge_asof.json (needs pandas; the tests read only the JSON).

A dozen pairs of sides, sorted on `on` as merge_asof demands, NaN-free, int64 or float64, with many duplicate times; with and
without a `by` column.  For each pair the four answers direction x allow_exact_matches: per left row the right row id, -1 for none.

    python tools/gen_asof_golden.py            # rewrites tests/golden/asof_merge_asof.json
"""
import json
import os

import numpy as np
import pandas as pd

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "asof_merge_asof.json")


def main():
    sides = []
    for seed in range(12):
        rng = np.random.default_rng(500 + seed)
        nb, npr = int(rng.integers(150, 300)), int(rng.integers(150, 300))
        dom = int(rng.integers(15, 60))                          # far fewer times than rows: duplicates on both sides
        fp = seed % 2 == 1
        bon, pon = np.sort(rng.integers(-dom, dom, nb)), np.sort(rng.integers(-dom - 2, dom + 2, npr))
        if fp:
            bon, pon = bon / 4.0, pon / 4.0
        by = seed % 3 != 0
        bby, pby = rng.integers(0, 5, nb), rng.integers(0, 6, npr)
        right = pd.DataFrame({"on": bon, "by": bby, "row": np.arange(nb, dtype=np.int64)})
        left = pd.DataFrame({"on": pon, "by": pby})
        answers = {}
        for direction in ("backward", "forward"):
            for exact in (True, False):
                m = pd.merge_asof(left, right, on="on", by="by" if by else None, direction=direction, allow_exact_matches=exact)
                answers["%s_%s" % (direction, "exact" if exact else "strict")] = [int(r) if r == r else -1 for r in m["row"].tolist()]
        sides.append({"dtype": "float64" if fp else "int64", "by": by, "build_on": bon.tolist(), "probe_on": pon.tolist(),
                      "build_by": bby.tolist(), "probe_by": pby.tolist(), "answers": answers})
    with open(OUT, "w") as f:
        json.dump({"pandas": pd.__version__, "sides": sides}, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
