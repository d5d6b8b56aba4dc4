"""Pair windows at size: ms per call of aqg_scan2 / aqg_grouped_scan2_flat, one JSON line per (shape, dtype, op, w), with the variance scan
of ONE of the two columns timed beside it at the same shape, in the same process and on the same buffers (varw for the windows, vars
for the running op).  No pass / fail threshold (DESIGN.md section 4.21 holds the numbers).

    python tools/pairwin_probe.py [--n 1e8] [--shapes flat,g100,g1e5] [--dtypes int32,double] [--reps 7] [--compose]

Columns from aqg_gen_column: x = the int32 column v1, y = v2; the double columns are emas of them.  The grouped shapes time the call over
columns already in the flat layout; the flatten is not part of it.
ms: HIP events around the whole call (aqg_timer_start / aqg_timer_stop_ms): the median, the least and the greatest of --reps timed
calls after two warm-up calls.  kernel_ms: aqg_last_kernel_ms of the last call (the short routes: the one kernel; the prefix route: every
pass).  gbs: bytes the call must move -- both columns read, one double a row written -- over kernel_ms.
--compose: once, at the flat double shape, what a user had to write before: three products through aqg_ewise and five sumw (w = 64),
every intermediate column allocated by the call that makes it, as the header layer would."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import SCAN2_CORRS, SCAN2_CORRW, SCAN2_COVW

GEN_ID3, GEN_V1, GEN_V2 = 2, 6, 7
SCAN_SUMW, SCAN_VARS, SCAN_VARW = 4, 12, 14
OP_MUL = 2


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
    ap.add_argument("--shapes", default="flat,g100,g1e5")
    ap.add_argument("--dtypes", default="int32,double")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--compose", action="store_true")
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    cols = {"int32": (d.gen_column(GEN_V1, 42, 0, n, n, 100), d.gen_column(GEN_V2, 42, 0, n, n, 100))}
    if "double" in a.dtypes:
        cols["double"] = tuple(d.ema(c, alpha=0.5, keep=True) for c in cols["int32"])
    out = d.empty(n, np.float64)
    for shape in a.shapes.split(","):
        gb = None
        if shape != "flat":
            G = int(float(shape[1:]))
            keys = d.gen_column(GEN_ID3, 42, 0, n, n, max(1, n // G))
            gb = d.groupby_build([keys])
            del keys
        for dt in a.dtypes.split(","):
            x, y = cols[dt] if gb is None else tuple(d.grouped_flatten(gb, c, keep=True) for c in cols[dt])
            esz = x.dtype.itemsize
            var_ms = {}
            for op, name, w in [(SCAN2_COVW, "covw", 5), (SCAN2_CORRW, "corrw", 5), (SCAN2_COVW, "covw", 64), (SCAN2_CORRW, "corrw", 64),
                                (SCAN2_COVW, "covw", 1000), (SCAN2_CORRW, "corrw", 1000), (SCAN2_CORRS, "corrs", 0)]:
                if gb is None:
                    times = timed(d, a.reps, lambda: d.scan2(op, x, y, w, keep=True, out=out))
                else:
                    times = timed(d, a.reps, lambda: d.grouped_scan2(gb, op, x, y, w, flat=True, keep=True, out=out))
                kms = d.last_kernel_ms()
                route = d.scan2_last()[0]
                if w not in var_ms:
                    vop = SCAN_VARW if w else SCAN_VARS
                    if gb is None:
                        vt = timed(d, a.reps, lambda: d.scan(vop, x, w, keep=True, out=out))
                    else:
                        vt = timed(d, a.reps, lambda: d.grouped_scan(gb, vop, x, w, flat=True, keep=True, out=out))
                    var_ms[w] = (stats(vt)["ms"], round(d.last_kernel_ms(), 3))
                rec = {"shape": shape, "groups": 1 if gb is None else gb.ngroups, "n": n, "dtype": dt, "op": name, "w": w, "route": route, **stats(times),
                       "kernel_ms": round(kms, 3), "gbs": round(n * (2 * esz + 8) / kms / 1e6, 1), "var_ms": var_ms[w][0], "var_kernel_ms": var_ms[w][1]}
                rec["over_var"] = round(rec["ms"] / rec["var_ms"], 2)
                print(json.dumps(rec), flush=True)
            if a.compose and gb is None and dt == "double":
                def compose():
                    for l, r in ((x, x), (y, y), (x, y)):
                        p = d.ewise(OP_MUL, l, r, keep=True)
                        d.scan(SCAN_SUMW, p, 64, keep=True)
                    d.scan(SCAN_SUMW, x, 64, keep=True)
                    d.scan(SCAN_SUMW, y, 64, keep=True)
                print(json.dumps({"shape": shape, "n": n, "dtype": dt, "op": "3 x ewise mul + 5 x sumw(64)", **stats(timed(d, a.reps, compose))}), flush=True)
            if gb is not None:
                del x, y
        if gb is not None:
            gb.destroy()
    d.close()


if __name__ == "__main__":
    main()
