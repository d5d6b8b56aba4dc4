"""The window join at size: a trades x quotes shape, ms per call, one JSON line per (build rows, symbols, window, dtype), with its two
yardsticks timed in the same process on the same build side.  No pass / fail threshold.

    python tools/wj_probe.py [--n 1e8] [--build 1e9,1e6] [--groups 100,1e5] [--windows 5,100,10000] [--dtypes int32,double] [--reps 7]

Build side (quotes): `sym` uint32 below --groups (seeded, uniform), `time` int64 = 0, 1, 2, ... (in time order, no ties), a value
column.  Probe side (trades): --n rows, `sym` likewise, `time` uniform over the build side's range.  A window of about w build rows of
one symbol is `before` = w * groups, `after` = 0, both sides closed.  Calls, HIP events around each, the median / least / greatest of
--reps timed calls after two warm-ups:
  bounds   aqg_join_window_bounds          gather   aqg_gather(x, order)          fold   aqg_interval_fold SUM over the gathered column
  whole    aqg_join_window SUM             kernel_ms: the fold kernel of that call alone (aqg_last_kernel_ms)
  asof     aqg_join_asof BACKWARD on the same sides: the yardstick of the search -- the same ordering step, one search instead of two
  self     probe == build, after = 0: aqg_join_window SUM against aqg_grouped_rangew SUM (CLOSED) over the same rows: the yardstick
           of the fold -- the same answers from the tile-staged fold (only where the build side has at most --self-max rows)
bytes_per_row of the two kernels, per probe row: bounds 4 gid + 8 time + 4 lo + 4 hi; fold 4 lo + 4 hi + the result."""
import argparse
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd import capi
from aquery2_amd.capi import RANGEW_CLOSED, RANGEW_SUM


def timed(d, reps, call):
    call()
    call()
    times = []
    for _ in range(reps):
        d.sync()
        d.timer_start()
        call()
        times.append(d.timer_stop_ms())
    return [round(float(np.median(times)), 3), round(min(times), 3), round(max(times), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--build", default="1e9,1e6")
    ap.add_argument("--groups", default="100,1e5")
    ap.add_argument("--windows", default="5,100,10000")
    ap.add_argument("--dtypes", default="int32,double")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--self-max", type=float, default=2e8)
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    rng = np.random.default_rng(42)
    dts = (C.c_int * 1)(capi.UINT32)
    chk = d._chk
    for nb in (int(float(s)) for s in a.build.split(",")):
        bo = d.to_device(np.arange(nb, dtype=np.int64))
        po = d.to_device(rng.integers(0, nb, n).astype(np.int64))
        order, lo, hi, rows = d.empty(nb, np.uint32), d.empty(n, np.uint32), d.empty(n, np.uint32), d.empty(n, np.uint32)
        for G in (int(float(s)) for s in a.groups.split(",")):
            bsym = rng.integers(0, G, nb).astype(np.uint32)
            bk, pk = d.to_device(bsym), d.to_device(rng.integers(0, G, n).astype(np.uint32))
            bp, pp = (C.c_void_p * 1)(bk.ptr), (C.c_void_p * 1)(pk.ptr)
            asof = timed(d, a.reps, lambda: chk(d.lib.aqg_join_asof(d.ctx, capi.ASOF_BACKWARD, 0, 1, dts, bp, bo.ptr, nb, pp, po.ptr, n, capi.INT64, rows.ptr), "aqg_join_asof"))
            asof_kernel = round(d.last_kernel_ms(), 3)
            gb = d.groupby_build([bk]) if nb <= a.self_max else None
            for dt in a.dtypes.split(","):
                x = d.to_device(rng.integers(-1000, 1000, nb).astype(np.int32) if dt == "int32" else rng.normal(0, 100, nb))
                xs, out, out_self = d.empty(nb, x.dtype), d.rangew_out(RANGEW_SUM, x, n), d.rangew_out(RANGEW_SUM, x, nb) if gb else None
                for w in (int(float(s)) for s in a.windows.split(",")):
                    before = float(w) * G
                    bounds = timed(d, a.reps, lambda: chk(d.lib.aqg_join_window_bounds(d.ctx, 0, 1, dts, bp, bo.ptr, nb, pp, po.ptr, n, capi.INT64, before, 0.0,
                                                                                       order.ptr, lo.ptr, hi.ptr), "aqg_join_window_bounds"))
                    bounds_kernel = round(d.last_kernel_ms(), 3)
                    gather = timed(d, a.reps, lambda: chk(d.lib.aqg_gather(d.ctx, x.tag, C.c_void_p(x.ptr), C.c_void_p(order.ptr), C.c_uint32(nb), C.c_void_p(xs.ptr)), "aqg_gather"))
                    fold = timed(d, a.reps, lambda: chk(d.lib.aqg_interval_fold(d.ctx, RANGEW_SUM, x.tag, xs.ptr, nb, lo.ptr, hi.ptr, n, None, out.ptr), "aqg_interval_fold"))
                    fold_kernel = round(d.last_kernel_ms(), 3)
                    whole = timed(d, a.reps, lambda: chk(d.lib.aqg_join_window(d.ctx, RANGEW_SUM, 0, 1, dts, bp, bo.ptr, nb, pp, po.ptr, n, capi.INT64, before, 0.0,
                                                                               x.tag, x.ptr, None, out.ptr), "aqg_join_window"))
                    routes, groups, passes = d.join_window_last()
                    mean_len = float(capi.DevBuf(d, hi.ptr, np.uint32, min(n, 1 << 22), owned=False).to_host().astype(np.int64).mean()
                                     - capi.DevBuf(d, lo.ptr, np.uint32, min(n, 1 << 22), owned=False).to_host().astype(np.int64).mean())
                    rec = {"n": n, "build": nb, "groups": groups, "dtype": dt, "window_rows": w, "mean_len": round(mean_len, 1), "routes": routes,
                           "sort_passes": passes, "bounds_ms": bounds, "bounds_kernel_ms": bounds_kernel, "gather_ms": gather, "fold_ms": fold,
                           "fold_kernel_ms": fold_kernel, "whole_ms": whole, "asof_ms": asof, "asof_kernel_ms": asof_kernel,
                           "bounds_over_asof": round(bounds[0] / asof[0], 2), "bounds_kernel_over_asof_kernel": round(bounds_kernel / asof_kernel, 2),
                           "bounds_kernel_GBps": round(n * 20 / (bounds_kernel * 1e-3) / 1e9, 1),
                           "fold_kernel_GBps": round(n * (8 + out.dtype.itemsize) / (fold_kernel * 1e-3) / 1e9, 1)}
                    if gb is not None:
                        selfj = timed(d, a.reps, lambda: chk(d.lib.aqg_join_window(d.ctx, RANGEW_SUM, 0, 1, dts, bp, bo.ptr, nb, bp, bo.ptr, nb, capi.INT64, before, 0.0,
                                                                                   x.tag, x.ptr, None, out_self.ptr), "aqg_join_window (self)"))
                        self_kernel = round(d.last_kernel_ms(), 3)
                        grouped = timed(d, a.reps, lambda: d.grouped_rangew(gb, RANGEW_SUM, bo, before, x, RANGEW_CLOSED, keep=True, out=out_self))
                        grouped_kernel = round(d.last_kernel_ms(), 3)
                        rec.update({"self_join_ms": selfj, "self_fold_kernel_ms": self_kernel, "grouped_rangew_ms": grouped, "grouped_rangew_fold_kernel_ms": grouped_kernel,
                                    "self_over_grouped": round(selfj[0] / grouped[0], 2), "fold_kernel_over_tile_staged": round(self_kernel / grouped_kernel, 2)})
                    print(json.dumps(rec), flush=True)
                for b in (x, xs, out, out_self):
                    if b is not None:
                        b.free()
            if gb is not None:
                gb.destroy()
            bk.free(); pk.free()
        for b in (bo, po, order, lo, hi, rows):
            b.free()
    d.close()


if __name__ == "__main__":
    main()
