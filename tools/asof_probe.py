"""The as-of join at size: a quotes / trades shape, ms per call, one JSON line per call.

    python tools/asof_probe.py [--n 1e8] [--build 1e7] [--groups 1e4] [--reps 3]

Build side (quotes): --build rows, `sym` uint32 below --groups, `time` int64 non-decreasing; probe side (trades): --n rows of the same
columns over the same time range, both from seeded numpy (running sums of small steps: duplicate times on both sides).  Calls:
  aqg_join_keys_lookup on (sym)           the yardstick: the equi look-up does strictly less work (no ordering, no search)
  aqg_join_asof BACKWARD, build in time order   (PRESORTED: the ordering step sorts by the group id alone)
  aqg_join_asof BACKWARD, build side shuffled   (sorted by (group id, time))
ms: HIP events around the whole call, the median of --reps timed calls after one warm-up; `kernel_ms` the probe kernel alone
(aqg_last_kernel_ms).  `build_ms` is the same call over the first 16 probe rows -- grouping, ordering and imaging the build side,
what does not depend on the probe side -- and `build_share` its share of the call.  `bytes_per_row`: the algorithmic bytes of the
search kernel per probe row (4 group id + 8 time + 4 result); `roofline` their share of 8 TB/s at `kernel_ms`."""
import argparse
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd import capi

ROOF = 8e12


def timed(d, reps, call):
    call()                                   # warm-up: code objects, workspace, pooled buffers
    times = []
    for _ in range(reps):
        d.sync()
        d.timer_start()
        call()
        times.append(d.timer_stop_ms())
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--build", type=float, default=1e7)
    ap.add_argument("--groups", type=float, default=1e4)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    n, nb, G = int(a.n), int(a.build), int(a.groups)
    d = A.Device(0)
    rng = np.random.default_rng(42)
    step = max(1, 3 * n // nb)
    btime = np.cumsum(rng.integers(0, 2 * step, nb)).astype(np.int64)
    ptime = np.cumsum(rng.integers(0, 3, n)).astype(np.int64)
    bsym, psym = rng.integers(0, G, nb).astype(np.uint32), rng.integers(0, G, n).astype(np.uint32)
    pk, po, out = d.to_device(psym), d.to_device(ptime), d.empty(n, np.uint32)
    del psym, ptime
    dts = (C.c_int * 1)(capi.UINT32)
    pp = (C.c_void_p * 1)(pk.ptr)
    checksum = lambda: int(capi.DevBuf(d, out.ptr, np.uint32, min(n, 1 << 24), owned=False).to_host().astype(np.uint64).sum())

    def report(call, times, **extra):
        ms = float(np.median(times))
        print(json.dumps({"call": call, "n": n, "build": nb, "groups": G, "ms": round(ms, 4), "times_ms": [round(t, 4) for t in times],
                          "rows_per_s": round(n / ms * 1e3, 0), **extra}), flush=True)
        return ms
    for name, order in (("build in time order", None), ("build side shuffled", rng.permutation(nb))):
        bk, bo = d.to_device(bsym if order is None else bsym[order]), d.to_device(btime if order is None else btime[order])
        bp = (C.c_void_p * 1)(bk.ptr)
        if order is None:
            look = lambda: d._chk(d.lib.aqg_join_keys_lookup(d.ctx, 1, dts, bp, nb, pp, n, out.ptr), "aqg_join_keys_lookup")
            report("aqg_join_keys_lookup (sym)", timed(d, a.reps, look), kernel_ms=round(d.last_kernel_ms(), 4), checksum=checksum())
        asof = lambda rows: d._chk(d.lib.aqg_join_asof(d.ctx, capi.ASOF_BACKWARD, 0, 1, dts, bp, bo.ptr, nb, pp, po.ptr, rows, capi.INT64, out.ptr), "aqg_join_asof")
        build_ms = float(np.median(timed(d, a.reps, lambda: asof(min(n, 16)))))
        times = timed(d, a.reps, lambda: asof(n))
        kernel_ms, (routes, groups, passes) = d.last_kernel_ms(), d.join_asof_last()
        ms = float(np.median(times))
        report("aqg_join_asof BACKWARD, " + name, times, kernel_ms=round(kernel_ms, 4), routes=routes, presorted=bool(routes & capi.ASOF_ROUTE_PRESORTED),
               build_groups=groups, sort_passes=passes, build_ms=round(build_ms, 4), build_share=round(build_ms / ms, 3), bytes_per_row=16,
               roofline=round(n * 16 / (kernel_ms * 1e-3) / ROOF, 3), checksum=checksum())
        bk.free(); bo.free()
    d.close()


if __name__ == "__main__":
    main()
