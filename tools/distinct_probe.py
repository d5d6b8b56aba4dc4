"""count(distinct x) under GROUP BY at size: ms per call of the four shapes of DESIGN.md section 4.9, one JSON line per shape and mode.

    python tools/distinct_probe.py [--n 1e9] [--mode both|distinct|compose] [--shapes 1,2,3,4] [--reps 5]

Shapes (columns from aqg_gen_column):
  1  v1 by id1            100 groups, 5 values                    2  v2 by (id4, id5)     1e4 groups, 15 values
  3  v3 by id3            about n / 100 groups of about 100 rows  4  v3 by id1            100 groups, nearly every value its own
--mode distinct  times aqg_grouped_count_distinct on a handle of aqg_groupby_build (the build itself is not timed: the generated loop
                 has it anyway); `kernel_ms` / `kernel_gbs` are the tile pass alone (aqg_last_kernel_ms; bytes = the flat column),
                 `crossing` and `pairs` what aqg_distinct_last reports.
--mode compose   times what a caller could do without it through the public C-ABI: aqg_groupby_agg over (keys..., x) with no
                 aggregates -- the distinct tuples -- then aqg_groupby_keys for the key columns of that table and a count-only
                 aqg_groupby_agg over them.  Both handles are reused from call to call.
--mode both      the two in ONE process, distinct first (the default: the acceptance compares them process by process).
ms: HIP events around the whole call (aqg_timer_start / aqg_timer_stop_ms), the median of --reps timed calls after one warm-up call.
`checksum` (the sum of the counts) must agree between the modes."""
import argparse
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A

GEN_ID1, GEN_ID3, GEN_ID4, GEN_ID5, GEN_V1, GEN_V2, GEN_V3 = 0, 2, 3, 4, 6, 7, 8
RED_COUNT = 3


def timed(d, reps, call):
    call()                                   # warm-up: code objects, workspace, the flat layout of the build, the pair list
    times = []
    for _ in range(reps):
        d.sync()
        d.timer_start()
        call()
        times.append(d.timer_stop_ms())
    return times


def run_distinct(d, reps, keys, x):
    gb = d.groupby_build(keys)
    out = d.empty(gb.ngroups, np.uint32)
    times = timed(d, reps, lambda: d.grouped_count_distinct(gb, x, keep=True, out=out))
    kms = d.last_kernel_ms()
    _, crossing, pairs = d.distinct_last()
    extra = {"groups": gb.ngroups, "kernel_ms": round(kms, 4), "kernel_gbs": round(x.n * x.dtype.itemsize / kms / 1e6, 1), "crossing": crossing,
             "pairs": pairs, "checksum": int(out.to_host().astype(np.int64).sum())}
    out.free()
    gb.destroy()
    return times, extra


def run_compose(d, reps, keys, x):
    state = {"h1": None, "h2": None, "kcols": None}

    def call():
        h1 = state["h1"] = d.groupby_agg(keys + [x], [], [], handle=state["h1"])
        if state["kcols"] is None or state["kcols"][0].n != h1.ngroups:
            state["kcols"] = [d.empty(h1.ngroups, k.dtype) for k in keys]
        for j, kc in enumerate(state["kcols"]):
            d._chk(d.lib.aqg_groupby_keys(h1.h, j, C.c_void_p(kc.ptr)), "aqg_groupby_keys")
        state["h2"] = d.groupby_agg(state["kcols"], [RED_COUNT], [None], handle=state["h2"])
    times = timed(d, reps, call)
    d.sync()
    h2 = state["h2"]
    counts = h2.result(0, RED_COUNT, 0)
    extra = {"groups": h2.ngroups, "tuples": state["h1"].ngroups, "checksum": int(np.asarray(counts).astype(np.int64).sum())}
    for b in state["kcols"]:
        b.free()
    state["h1"].destroy(); h2.destroy()
    return times, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--mode", choices=("both", "distinct", "compose"), default="both")
    ap.add_argument("--shapes", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    gen = lambda col, K: d.gen_column(col, 42, 0, n, n, K)
    for s in (int(t) for t in a.shapes.split(",")):
        if s == 1:
            keys, x, name = [gen(GEN_ID1, 100)], gen(GEN_V1, 100), "count(distinct v1) by id1"
        elif s == 2:
            keys, x, name = [gen(GEN_ID4, 100), gen(GEN_ID5, 100)], gen(GEN_V2, 100), "count(distinct v2) by id4, id5"
        elif s == 3:
            keys, x, name = [gen(GEN_ID3, 100)], gen(GEN_V3, 100), "count(distinct v3) by id3"
        else:
            keys, x, name = [gen(GEN_ID1, 100)], gen(GEN_V3, 100), "count(distinct v3) by id1"
        for mode in (("distinct", "compose") if a.mode == "both" else (a.mode,)):
            times, extra = (run_distinct if mode == "distinct" else run_compose)(d, a.reps, keys, x)
            print(json.dumps({"shape": s, "name": name, "mode": mode, "n": n, "ms": float(np.median(times)), "times_ms": [round(t, 3) for t in times], **extra}), flush=True)
        for b in keys + [x]:
            b.free()
    d.close()


if __name__ == "__main__":
    main()
