"""Ranking at size: ms per call of aqg_rank / aqg_grouped_rank_flat, one JSON line per (shape, dtype, method), with what the SORTED route
is made of timed beside it on the same buffers in the same process: aqg_sort_rows over the same keys alone (the route's floor), the
emit kernel alone (aqg_last_kernel_ms of the rank call: the events bracket rank_emit_kernel), and a device copy that moves the bytes the
emit kernel moves.  No pass / fail threshold (DESIGN.md section 4.19 holds the numbers).

    python tools/rank_probe.py [--n 1e8] [--shapes flat,g100,g1e5,g1e7] [--dtypes int32,double] [--reps 7]

Columns from aqg_gen_column: the int32 column v1 (few distinct values: long tie runs); the double column is an ema of it (nearly all
distinct).  The grouped shapes time the call over columns already in the flat layout; the flatten is not part of it.  With n / G at or
below AQG_SELECT_SMALL_MAX rows per group (g1e7 at the default n) every group takes the SMALL route, and there is no sort to compare with.
ms: HIP events around the whole call (aqg_timer_start / aqg_timer_stop_ms): the median, the least and the greatest of --reps timed
calls after two warm-up calls.  emit_bytes: per sorted entry the order (4) and the marks (1) read, the result (4 or 8) scattered;
copy_ms: aqg_d2d of emit_bytes / 2 (a copy reads and writes every byte it is given)."""
import argparse
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import ORDER_ASC, RANK_AVERAGE, RANK_DENSE, RANK_MIN, RANK_ROUTE_SORTED

GEN_ID3, GEN_V1 = 2, 6


def timed(d, reps, call):
    call()
    call()
    times = []
    for _ in range(reps):
        d.sync()
        d.timer_start()
        call()
        times.append(d.timer_stop_ms())
    return times


def stats(times):
    return {"ms": round(float(np.median(times)), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--shapes", default="flat,g100,g1e5,g1e7")
    ap.add_argument("--dtypes", default="int32,double")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    xi = d.gen_column(GEN_V1, 42, 0, n, n, 100)
    xd = d.ema(xi, alpha=0.5, keep=True)
    scratch = (d.empty(n * 7, np.uint8), d.empty(n * 7, np.uint8))
    rows = d.empty(n, np.uint32)
    for shape in a.shapes.split(","):
        gb, kf = None, None
        if shape != "flat":
            G = int(float(shape[1:]))
            keys = d.gen_column(GEN_ID3, 42, 0, n, n, max(1, n // G))
            gb = d.groupby_build([keys])
            kf = d.grouped_flatten(gb, keys, keep=True)
        for dt in a.dtypes.split(","):
            x = xi if dt == "int32" else xd
            xf = x if gb is None else d.grouped_flatten(gb, x, keep=True)
            sort_ms = None
            for method, mname in ((RANK_MIN, "min"), (RANK_DENSE, "dense"), (RANK_AVERAGE, "average")):
                out = d.rank_out(method, n)
                osz = out.dtype.itemsize
                if gb is None:
                    times = timed(d, a.reps, lambda: d.rank(xf, method, ORDER_ASC, keep=True, out=out))
                else:
                    times = timed(d, a.reps, lambda: d.grouped_rank(gb, xf, method, ORDER_ASC, flat=True, keep=True, out=out))
                routes, tile = d.rank_last()
                rec = {"shape": shape, "groups": 1 if gb is None else gb.ngroups, "n": n, "dtype": dt, "method": mname, "routes": routes, **stats(times)}
                if routes & RANK_ROUTE_SORTED:
                    rec["emit_kernel_ms"] = round(d.last_kernel_ms(), 3)
                    if sort_ms is None:
                        skeys = [xf] if gb is None else [kf, xf]
                        sort_ms = stats(timed(d, a.reps, lambda: d.sort_rows(skeys, [ORDER_ASC] * len(skeys), out=rows, keep=True)))["ms"]
                    nbytes = n * (5 + osz)
                    copy = timed(d, a.reps, lambda: d._chk(d.lib.aqg_d2d(d.ctx, C.c_void_p(scratch[0].ptr), C.c_void_p(scratch[1].ptr), C.c_size_t(nbytes // 2)), "aqg_d2d"))
                    copy_ms = float(np.median(copy))
                    rec.update({"sort_rows_ms": sort_ms, "emit_bytes": nbytes, "copy_ms": round(copy_ms, 3), "emit_over_copy": round(rec["emit_kernel_ms"] / copy_ms, 2),
                                "rank_over_sort": round(rec["ms"] / sort_ms, 2)})
                print(json.dumps(rec), flush=True)
                del out
        if gb is not None:
            gb.destroy()
    d.close()


if __name__ == "__main__":
    main()
