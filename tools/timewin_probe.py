"""Time-range windows at size: ms per call of aqg_rangew_bounds, aqg_rangew_fold (SUM, MIN) and the whole aqg_rangew /
aqg_grouped_rangew_flat (SUM), one JSON line per (stamps, span, shape, dtype), with the fixed-width siblings -- aqg_scan(SUMW / MINW) and
aqg_grouped_scan_flat of the equal row count -- timed beside them on the same buffers in the same process.  No pass / fail threshold
(DESIGN.md section 4.17 holds the numbers).

    python tools/timewin_probe.py [--n 1e9] [--dtypes int32,double] [--shapes flat,g100,g1e5] [--spans 5,100,1000,1000000] [--reps 7]

Stamps: `regular` is 0, 1, 2, ... (a span of w holds exactly w rows); `irregular` is a walk with steps 0, 1 or 2 (mean 1, runs of
ties), both int32 and made on the host from a seed.  Values: the int32 column v1 of aqg_gen_column; the double column is an ema of it
(any doubles do).  The grouped shapes time the calls over columns already in the flat layout, stamps ascending along it.  ms: HIP
events around the whole call (aqg_timer_start / aqg_timer_stop_ms): the median, the least and the greatest of --reps timed calls after
two warm-up calls.  bytes_per_row: what the passes must move -- bounds: the stamp read, lo written; fold: lo and the value read, the
result written -- and frac_roofline is that over the time, against 8 TB/s."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import RANGEW_MIN, RANGEW_OPEN, RANGEW_SUM

GEN_ID1, GEN_ID3, GEN_V1 = 0, 2, 6
SCAN_SUMW, SCAN_MINW = 4, 6
HBM = 8e12


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
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--dtypes", default="int32,double")
    ap.add_argument("--shapes", default="flat,g100,g1e5")
    ap.add_argument("--spans", default="5,100,1000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    gen = lambda col, K: d.gen_column(col, 42, 0, n, n, K)
    xi = gen(GEN_V1, 100)
    xd = d.ema(xi, alpha=0.5, keep=True)
    stamps = {"regular": d.to_device(np.arange(n, dtype=np.int32))}
    walk = np.cumsum(np.random.default_rng(42).integers(0, 3, size=n, dtype=np.int8), dtype=np.int64)
    assert walk[-1] < 2 ** 31
    stamps["irregular"] = d.to_device(walk.astype(np.int32))
    del walk
    lo = d.empty(n, np.uint32)
    for shape in a.shapes.split(","):
        gb = None
        if shape != "flat":
            gb = d.groupby_build([gen(GEN_ID1, 100) if shape == "g100" else gen(GEN_ID3, max(1, n // 100_000))])
        for dt in a.dtypes.split(","):
            x = xi if dt == "int32" else xd
            esz = x.dtype.itemsize
            osum = d.rangew_out(RANGEW_SUM, x, n)
            omin = d.rangew_out(RANGEW_MIN, x, n)
            for w in (int(float(s)) for s in a.spans.split(",")):
                if gb is None:
                    sumw = timed(d, a.reps, lambda: d.scan(SCAN_SUMW, x, w, keep=True, out=osum))
                    minw = timed(d, a.reps, lambda: d.scan(SCAN_MINW, x, w, keep=True, out=omin))
                else:
                    sumw = timed(d, a.reps, lambda: d.grouped_scan(gb, SCAN_SUMW, x, w, flat=True, keep=True, out=osum))
                    minw = timed(d, a.reps, lambda: d.grouped_scan(gb, SCAN_MINW, x, w, flat=True, keep=True, out=omin))
                for sname, t in stamps.items():
                    if w >= 10 ** 5 and sname == "irregular":
                        continue
                    bounds = timed(d, a.reps, lambda: d.rangew_bounds(t, w, RANGEW_OPEN, gb=gb, keep=True, out=lo))
                    _, _, up, down = d.rangew_last()
                    fsum = timed(d, a.reps, lambda: d.rangew_fold(RANGEW_SUM, x, lo, keep=True, out=osum))
                    fmin = timed(d, a.reps, lambda: d.rangew_fold(RANGEW_MIN, x, lo, keep=True, out=omin))
                    if gb is None:
                        whole = timed(d, a.reps, lambda: d.rangew(RANGEW_SUM, t, w, x, RANGEW_OPEN, keep=True, out=osum))
                    else:
                        whole = timed(d, a.reps, lambda: d.grouped_rangew(gb, RANGEW_SUM, t, w, x, RANGEW_OPEN, flat=True, keep=True, out=osum))
                    bb, fb = 4 + 4, 4 + esz + osum.dtype.itemsize
                    print(json.dumps({"shape": shape, "groups": 1 if gb is None else gb.ngroups, "n": n, "dtype": dt, "stamps": sname, "span_rows": w,
                                      "steps_up": up, "steps_down": down, "bounds_ms": bounds, "fold_sum_ms": fsum, "fold_min_ms": fmin, "rangew_sum_ms": whole,
                                      "sumw_ms": sumw, "minw_ms": minw, "sum_ratio": round(whole[0] / sumw[0], 2), "min_ratio": round((bounds[0] + fmin[0]) / minw[0], 2),
                                      "bounds_frac_roofline": round(n * bb / (bounds[0] * 1e-3) / HBM, 3),
                                      "fold_sum_frac_roofline": round(n * fb / (fsum[0] * 1e-3) / HBM, 3)}), flush=True)
        if gb is not None:
            gb.destroy()
    d.close()


if __name__ == "__main__":
    main()
