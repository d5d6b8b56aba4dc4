"""Quantiles at size: ms per call of the four shapes of DESIGN.md section 4.8, one JSON line per shape.

    python tools/quantile_probe.py [--n 1e9] [--mode quantiles|median] [--nq 1|8] [--shapes 1,2,3,4] [--reps 5]

Shapes (columns from aqg_gen_column), those of tools/median_probe.py:
  1  h2o Q6: v3 by (id4, id5), float32, 1e4 groups        2  the flat column v3
  3  v3 by id3, about n / 100 groups                      4  an int64 value column by id1, 100 groups
--mode quantiles  times aqg_grouped_quantiles / aqg_quantiles: --nq 1 asks for [1] / 2 (the median), --nq 8 for
                  [0, 1, 5, 25, 50, 75, 95, 100] / 100.
--mode median     times aqg_grouped_median / aqg_median.  Only entry points that older checkouts have are used in this mode, so the
                  same file measures them.
ms: HIP events around the whole call (aqg_timer_start / aqg_timer_stop_ms), the median of --reps timed calls after one warm-up call."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import INT64

GEN_ID1, GEN_ID3, GEN_ID4, GEN_ID5, GEN_V1, GEN_V2, GEN_V3 = 0, 2, 3, 4, 6, 7, 8
OP_MUL = 2
LISTS = {1: ([1], 2), 8: ([0, 1, 5, 25, 50, 75, 95, 100], 100)}


def timed(d, reps, call):
    call()                                   # warm-up: code objects, workspace, the flat layout of the build
    times = []
    for _ in range(reps):
        d.sync()
        d.timer_start()
        call()
        times.append(d.timer_stop_ms())
    return times


def grouped_shape(d, mode, nq, reps, keys, x):
    gb = d.groupby_build(keys)
    G = gb.ngroups
    extra = {"groups": G}
    if mode == "median":
        out = d.empty(G, x.dtype)
        times = timed(d, reps, lambda: d.grouped_median(gb, x, keep=True, out=out))
    else:
        nums, den = LISTS[nq]
        out = d.empty(G * nq, x.dtype)
        times = timed(d, reps, lambda: d.grouped_quantiles(gb, x, nums, den, keep=True, out=out))
    extra["routes"], extra["passes"] = d.select_last_routes()
    extra["checksum"] = float(np.nansum(out.to_host().astype(np.float64)))
    out.free()
    gb.destroy()
    return times, extra


def flat_shape(d, mode, nq, reps, x):
    extra = {"groups": 1}
    res = []
    if mode == "median":
        times = timed(d, reps, lambda: res.append(d.median(x)))
    else:
        nums, den = LISTS[nq]
        times = timed(d, reps, lambda: res.append(d.quantiles(x, nums, den)))
    extra["routes"], extra["passes"] = d.select_last_routes()
    extra["checksum"] = float(np.nansum(np.asarray(res[-1], dtype=np.float64)))
    return times, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--mode", choices=("quantiles", "median"), default="quantiles")
    ap.add_argument("--nq", type=int, choices=sorted(LISTS), default=8)
    ap.add_argument("--shapes", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    gen = lambda col, K: d.gen_column(col, 42, 0, n, n, K)
    for s in (int(t) for t in a.shapes.split(",")):
        if s in (1, 2, 3):
            x = gen(GEN_V3, 100)
        if s == 1:
            keys, name = [gen(GEN_ID4, 100), gen(GEN_ID5, 100)], "q6: v3 by id4, id5"
        elif s == 2:
            keys, name = [], "flat v3"
        elif s == 3:
            keys, name = [gen(GEN_ID3, 100)], "v3 by id3"
        else:
            v1, v2 = gen(GEN_V1, 100), gen(GEN_V2, 100)
            x = d.ewise(OP_MUL, v1, v2, ot=INT64, keep=True)          # v1 * v2 as an int64 column
            v1.free(); v2.free()
            keys, name = [gen(GEN_ID1, 100)], "int64 by id1"
        times, extra = grouped_shape(d, a.mode, a.nq, a.reps, keys, x) if keys else flat_shape(d, a.mode, a.nq, a.reps, x)
        print(json.dumps({"shape": s, "name": name, "mode": a.mode, "nq": 1 if a.mode == "median" else a.nq, "n": n, "ms": float(np.median(times)),
                          "times_ms": [round(t, 3) for t in times], **extra}), flush=True)
        for b in keys + [x]:
            b.free()
    d.close()


if __name__ == "__main__":
    main()
