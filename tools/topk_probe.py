"""Top-k at size: ms per call of the shapes of DESIGN.md section 4.11 next to the sort that could be composed before, one JSON line per shape.

    python tools/topk_probe.py [--n 1e9] [--shapes 1,2,3,4,5] [--reps 5]

Shapes (columns from aqg_gen_column; the values are v3's float32 bit patterns read as int32 -- positive floats order like their bits):
  1  h2o Q8: the largest 2 by id3, about n / 100 groups       2  k = 2 by (id4, id5), 1e4 groups       3  k = 100 by (id4, id5)
  4  flat, k = 10                                             5  flat, k = 1024
Per shape three calls alternate in one process, each timed by HIP events around the warmed call (aqg_timer_start / aqg_timer_stop_ms):
  flat   aqg_grouped_topk_flat over the column already in the flat layout (shapes 4, 5: aqg_topk)
  row    aqg_grouped_topk over the row-layout column: the flatten is part of the call (grouped shapes only)
  sort   the composition that existed before: aqg_sort_rows over (group id, value), ASC, DESC -- its time alone, without the pick
Reported: the median, and the spread (min, max) of --reps rounds; bytes: one read of the column per pass reported by
aqg_select_last_routes plus the outputs, and the share of `--hbm-gbs` that the flat call's time amounts to."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import DevBuf, ORDER_ASC, ORDER_DESC

GEN_ID3, GEN_ID4, GEN_ID5, GEN_V3 = 2, 3, 4, 8


def alternate(d, reps, calls):
    """{name: [ms, ...]}: one warm-up of every call, then `reps` rounds in which the calls take turns"""
    for call in calls.values():
        call()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            d.sync()
            d.timer_start()
            call()
            times[name].append(d.timer_stop_ms())
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--shapes", default="1,2,3,4,5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM bandwidth the share is taken of (MI355X: 8 TB/s peak)")
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    gen = lambda col: d.gen_column(col, 42, 0, n, n, 100)
    v3 = gen(GEN_V3)
    x = DevBuf(d, v3.ptr, np.int32, n, owned=False)
    shapes = {1: ("q8: largest 2 by id3", [GEN_ID3], 2), 2: ("largest 2 by id4, id5", [GEN_ID4, GEN_ID5], 2), 3: ("largest 100 by id4, id5", [GEN_ID4, GEN_ID5], 100),
              4: ("flat, largest 10", [], 10), 5: ("flat, largest 1024", [], 1024)}
    for s in (int(t) for t in a.shapes.split(",")):
        name, keycols, k = shapes[s]
        keys = [gen(c) for c in keycols]
        rows = d.empty(n, np.uint32)
        info = {}
        if keys:
            gb = d.groupby_build(keys)
            G = gb.ngroups
            xf = d.grouped_flatten(gb, x, keep=True)
            gid = DevBuf(d, d.lib.aqg_groupby_reversemap(gb.h), np.uint32, n, owned=False)
            vals = d.empty(G * k, np.int32)

            def flat_call():
                d._chk(d.lib.aqg_grouped_topk_flat(d.ctx, gb.h, ORDER_DESC, x.tag, xf.ptr, k, vals.ptr, None), "aqg_grouped_topk_flat")
                info["routes"], info["passes"] = d.select_last_routes() if "routes" not in info else (info["routes"], info["passes"])
            calls = {"flat": flat_call,
                     "row": lambda: d._chk(d.lib.aqg_grouped_topk(d.ctx, gb.h, ORDER_DESC, x.tag, x.ptr, k, vals.ptr, None), "aqg_grouped_topk"),
                     "sort": lambda: d.sort_rows([gid, x], [ORDER_ASC, ORDER_DESC], out=rows, keep=True)}
        else:
            G = 1
            vals = d.empty(k, np.int32)

            def flat_call():
                d._chk(d.lib.aqg_topk(d.ctx, ORDER_DESC, x.tag, x.ptr, n, k, vals.ptr, None), "aqg_topk")
                info["routes"], info["passes"] = d.select_last_routes() if "routes" not in info else (info["routes"], info["passes"])
            calls = {"flat": flat_call, "sort": lambda: d.sort_rows([x], [ORDER_DESC], out=rows, keep=True)}
        times = alternate(d, a.reps, calls)
        info["sort_passes"] = d.sort_last_passes()
        ms = {m: float(np.median(t)) for m, t in times.items()}
        nbytes = info["passes"] * n * 4 + G * k * 4
        print(json.dumps({"shape": s, "name": name, "n": n, "groups": G, "k": k, "ms": ms, "spread_ms": {m: [round(min(t), 3), round(max(t), 3)] for m, t in times.items()},
                          "sort_over_flat": ms["sort"] / ms["flat"], "bytes": nbytes, "share_of_hbm": nbytes / (ms["flat"] * 1e-3) / (a.hbm_gbs * 1e9),
                          "checksum": float(vals.to_host().astype(np.float64).sum()), **info}), flush=True)
        for b in keys + [rows, vals] + ([xf] if keys else []):
            b.free()
        if keys:
            gb.destroy()
    d.close()


if __name__ == "__main__":
    main()
