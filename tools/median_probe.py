"""The median at size: ms per call of the four shapes of DESIGN.md section 4.8, one JSON line per shape.

    python tools/median_probe.py [--n 1e9] [--mode select|sort] [--shapes 1,2,3,4] [--reps 5]

Shapes (columns from aqg_gen_column):
  1  h2o Q6: median(v3) by (id4, id5), float32, 1e4 groups        2  the flat median of v3
  3  median(v3) by id3, about n / 100 groups                      4  an int64 value column by id1, 100 groups
--mode select  times aqg_grouped_median / aqg_median.
--mode sort    times the composition that was available before them: aqg_sort_rows over (aqg_groupby_reversemap, value) with ASC, ASC,
               then two gathers at offsets[g] + (c - 1) / 2.  Only entry points that older checkouts have are used in this mode, so the
               same file measures them.
ms: HIP events around the whole call (aqg_timer_start / aqg_timer_stop_ms), the median of --reps timed calls after one warm-up call."""
import argparse
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import INT64, DevBuf, ORDER_ASC

GEN_ID1, GEN_ID3, GEN_ID4, GEN_ID5, GEN_V1, GEN_V2, GEN_V3 = 0, 2, 3, 4, 6, 7, 8
OP_MUL = 2


def timed(d, reps, call):
    call()                                   # warm-up: code objects, workspace, the flat layout of the build
    times = []
    for _ in range(reps):
        d.sync()
        d.timer_start()
        call()
        times.append(d.timer_stop_ms())
    return times


def grouped_shape(d, mode, reps, keys, x):
    gb = d.groupby_build(keys)
    G, n = gb.ngroups, x.n
    out = d.empty(G, x.dtype)
    extra = {"groups": G}
    if mode == "select":
        times = timed(d, reps, lambda: d.grouped_median(gb, x, keep=True, out=out))
        extra["routes"], extra["passes"] = d.select_last_routes()
    else:
        gid = DevBuf(d, d.lib.aqg_groupby_reversemap(gb.h), np.uint32, n, owned=False)
        counts = gb.counts().astype(np.int64)
        pos = d.to_device((np.concatenate([[0], np.cumsum(counts)[:-1]]) + (counts - 1) // 2).astype(np.uint32))
        rows, mid = d.empty(n, np.uint32), d.empty(G, np.uint32)

        def call():
            d.sort_rows([gid, x], [ORDER_ASC, ORDER_ASC], out=rows, keep=True)
            d._chk(d.lib.aqg_gather(d.ctx, 11, C.c_void_p(rows.ptr), C.c_void_p(pos.ptr), C.c_uint32(G), C.c_void_p(mid.ptr)), "aqg_gather")
            d._chk(d.lib.aqg_gather(d.ctx, x.tag, C.c_void_p(x.ptr), C.c_void_p(mid.ptr), C.c_uint32(G), C.c_void_p(out.ptr)), "aqg_gather")
        times = timed(d, reps, call)
        extra["passes"] = d.sort_last_passes()
        for b in (pos, rows, mid):
            b.free()
    extra["checksum"] = float(np.nansum(out.to_host().astype(np.float64)))
    out.free()
    gb.destroy()
    return times, extra


def flat_shape(d, mode, reps, x):
    n = x.n
    extra = {"groups": 1}
    if mode == "select":
        res = []
        times = timed(d, reps, lambda: res.append(d.median(x)))
        extra["routes"], extra["passes"] = d.select_last_routes()
        extra["checksum"] = float(res[-1])
    else:
        rows, out = d.empty(n, np.uint32), d.empty(1, x.dtype)
        pos = d.to_device(np.array([(n - 1) // 2], np.uint32))
        mid = d.empty(1, np.uint32)

        def call():
            d.sort_rows([x], [ORDER_ASC], out=rows, keep=True)
            d._chk(d.lib.aqg_gather(d.ctx, 11, C.c_void_p(rows.ptr), C.c_void_p(pos.ptr), C.c_uint32(1), C.c_void_p(mid.ptr)), "aqg_gather")
            d._chk(d.lib.aqg_gather(d.ctx, x.tag, C.c_void_p(x.ptr), C.c_void_p(mid.ptr), C.c_uint32(1), C.c_void_p(out.ptr)), "aqg_gather")
            return out.to_host()             # the flat median hands its result to the host: so does this
        times = timed(d, reps, call)
        extra["passes"] = d.sort_last_passes()
        extra["checksum"] = float(out.to_host()[0])
        for b in (rows, out, pos, mid):
            b.free()
    return times, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--mode", choices=("select", "sort"), default="select")
    ap.add_argument("--shapes", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    gen = lambda col, K: d.gen_column(col, 42, 0, n, n, K)
    for s in (int(t) for t in a.shapes.split(",")):
        if s in (1, 2, 3):
            x = gen(GEN_V3, 100)
        if s == 1:
            keys, name = [gen(GEN_ID4, 100), gen(GEN_ID5, 100)], "q6: median(v3) by id4, id5"
        elif s == 2:
            keys, name = [], "flat median(v3)"
        elif s == 3:
            keys, name = [gen(GEN_ID3, 100)], "median(v3) by id3"
        else:
            v1, v2 = gen(GEN_V1, 100), gen(GEN_V2, 100)
            x = d.ewise(OP_MUL, v1, v2, ot=INT64, keep=True)          # v1 * v2 as an int64 column
            v1.free(); v2.free()
            keys, name = [gen(GEN_ID1, 100)], "int64 median by id1"
        times, extra = grouped_shape(d, a.mode, a.reps, keys, x) if keys else flat_shape(d, a.mode, a.reps, x)
        print(json.dumps({"shape": s, "name": name, "mode": a.mode, "n": n, "ms": float(np.median(times)), "times_ms": [round(t, 3) for t in times], **extra}), flush=True)
        for b in keys + [x]:
            b.free()
    d.close()


if __name__ == "__main__":
    main()
