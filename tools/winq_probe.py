"""Moving quantiles at size: ms per call and rows per second of aqg_window_quantiles / aqg_grouped_window_quantiles_flat, one JSON line per
(shape, w, nq), with maxw(w) over the same column beside it as context.  No pass / fail threshold: the kernel is bound by LDS reads and
VALU work that grow with w, not by HBM.

    python tools/winq_probe.py [--n 1e8] [--w 5,21,100,1000] [--shapes flat,g100,g1e5] [--nq 1,8] [--reps 7]

Shapes (columns from aqg_gen_column): the float32 column v3, flat; by id1 (100 groups); by id3 (about 1e5 groups at n = 1e8).  The grouped
shapes time the call over the column already in the flat layout (what the header layer holds); the flatten is not part of it.
ms: HIP events around the whole call (aqg_timer_start / aqg_timer_stop_ms): the median, the least and the greatest of --reps timed calls
after one warm-up call (code objects, workspace, the flat layout of the build)."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A

GEN_ID1, GEN_ID3, GEN_V3 = 0, 2, 8
SCAN_MAXW = 7
EIGHT = ([0, 1, 5, 25, 50, 75, 95, 100], 100)
MEDIAN = ([1], 2)


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
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--w", default="5,21,100,1000")
    ap.add_argument("--shapes", default="flat,g100,g1e5")
    ap.add_argument("--nq", default="1,8")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    gen = lambda col, K: d.gen_column(col, 42, 0, n, n, K)
    x = gen(GEN_V3, 100)
    out = d.empty(8 * n, x.dtype)
    mx = d.empty(n, x.dtype)
    for shape in a.shapes.split(","):
        gb = xf = None
        if shape != "flat":
            keys = gen(GEN_ID1, 100) if shape == "g100" else gen(GEN_ID3, max(1, n // 100_000))
            gb = d.groupby_build([keys])
            xf = d.grouped_flatten(gb, x, keep=True)
            keys.free()
        for w in (int(t) for t in a.w.split(",")):
            if gb is None:
                ctx = timed(d, a.reps, lambda: d.scan(SCAN_MAXW, x, w, keep=True, out=mx))
            else:
                ctx = timed(d, a.reps, lambda: d.grouped_scan(gb, SCAN_MAXW, xf, w, flat=True, keep=True, out=mx))
            for nq in (int(t) for t in a.nq.split(",")):
                nums, den = MEDIAN if nq == 1 else EIGHT
                if gb is None:
                    times = timed(d, a.reps, lambda: d.window_quantiles(x, nums, den, w, keep=True, out=out))
                else:
                    times = timed(d, a.reps, lambda: d.grouped_window_quantiles(gb, xf, nums, den, w, flat=True, keep=True, out=out))
                ms = float(np.median(times))
                print(json.dumps({"shape": shape, "groups": 1 if gb is None else gb.ngroups, "n": n, "w": w, "nq": len(nums), "ms": round(ms, 3),
                                  "ms_min": round(min(times), 3), "ms_max": round(max(times), 3), "rows_per_s": round(n / ms * 1e3),
                                  "maxw_ms": round(float(np.median(ctx)), 3), "tile_halo": d.window_quantiles_last()}), flush=True)
        if gb is not None:
            xf.free()
            gb.destroy()
    d.close()


if __name__ == "__main__":
    main()
