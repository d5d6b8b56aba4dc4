"""`x[val] OP agg(x[val])` for all groups at size: ms per call, one JSON line per (triple, layout).

    python tools/grouped_ewise_probe.py [--n 1e9] [--groups 100|1e5|1e7] [--mode fused|composed] [--reps 5]

The column operand is h2o's v1 (int32), the operator SUB; the per-group scalar column holds G int32 / double values.
--mode fused     times aqg_grouped_ewise.
--mode composed  times the composition that could be written before it: aqg_gather(st, s, gid, n) into a temporary, then
                 aqg_ewise(AQG_VEC_VEC).  gid is the build's reversemap (row layout) or that column brought into the flat layout by
                 aqg_grouped_flatten, once, outside the timed region (flat layout).  Only entry points that older checkouts have are
                 used in this mode, so the same file measures them.
Groups: 100 = id1 (K = 100), 1e5 = id1 (K = 1e5), 1e7 = id3 (n / 100 distinct values at 1e9 rows).
ms: HIP events around the whole call (aqg_timer_start / aqg_timer_stop_ms), the median of --reps timed calls after one warm-up call
(which also makes the handle's cached group ids of the flat layout).  Run every (groups, mode) in a fresh process, alternate the modes,
and take the median of the per-process medians."""
import argparse
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import DOUBLE, INT32, VEC_SCALAR, VEC_VEC, DevBuf

GEN_ID1, GEN_ID3, GEN_V1 = 0, 2, 6
OP_SUB = 1


def timed(d, reps, call):
    call()
    times = []
    for _ in range(reps):
        d.sync()
        d.timer_start()
        call()
        times.append(d.timer_stop_ms())
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--groups", type=float, default=100)
    ap.add_argument("--mode", choices=("fused", "composed"), default="fused")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, want_g, d = int(a.n), int(a.groups), A.Device(0)
    key = d.gen_column(GEN_ID3, 42, 0, n, n, 100) if want_g >= 10 ** 7 else d.gen_column(GEN_ID1, 42, 0, n, n, want_g)
    gb = d.groupby_build([key])
    key.free()
    G = gb.ngroups
    v = d.gen_column(GEN_V1, 42, 0, n, n, 100)
    vflat = d.grouped_flatten(gb, v, keep=True)
    gid = DevBuf(d, d.lib.aqg_groupby_reversemap(gb.h), np.uint32, n, owned=False)
    gid_flat = d.grouped_flatten(gb, gid, keep=True) if a.mode == "composed" else None
    rng = np.random.default_rng(7)
    for st, s_host, ot, odt in ((INT32, rng.integers(1, 6, G).astype(np.int32), INT32, np.int32), (DOUBLE, rng.uniform(1, 5, G), DOUBLE, np.float64)):
        s = d.to_device(s_host)
        out = d.empty(n, odt)
        tmp = d.empty(n, s_host.dtype) if a.mode == "composed" else None
        for layout, x, ids in ((0, v, gid), (1, vflat, gid_flat)):
            if a.mode == "fused":
                def call():
                    d._chk(d.lib.aqg_grouped_ewise(d.ctx, gb.h, layout, OP_SUB, VEC_SCALAR, INT32, C.c_void_p(x.ptr), st, C.c_void_p(s.ptr), ot,
                                                   C.c_void_p(out.ptr)), "aqg_grouped_ewise")
            else:
                def call():
                    d._chk(d.lib.aqg_gather(d.ctx, st, C.c_void_p(s.ptr), C.c_void_p(ids.ptr), C.c_uint32(n), C.c_void_p(tmp.ptr)), "aqg_gather")
                    d._chk(d.lib.aqg_ewise(d.ctx, OP_SUB, VEC_VEC, INT32, C.c_void_p(x.ptr), st, C.c_void_p(tmp.ptr), ot, C.c_void_p(out.ptr),
                                           C.c_uint32(n)), "aqg_ewise")
            times = timed(d, a.reps, call)
            head = out.to_host() if n <= 10 ** 6 else DevBuf(d, out.ptr, odt, 10 ** 6, owned=False).to_host()
            print(json.dumps({"mode": a.mode, "n": n, "groups": G, "layout": ("row", "flat")[layout], "scalar": ("int32", "double")[st == DOUBLE],
                              "ms": float(np.median(times)), "times_ms": [round(t, 3) for t in times],
                              "checksum": float(head.astype(np.float64).sum())}), flush=True)
        for b in (s, out, tmp):
            if b is not None:
                b.free()
    d.close()


if __name__ == "__main__":
    main()
