"""Exponential moving averages at size: ms per call of aqg_scan_ema / aqg_grouped_ema_flat, constant alpha and decay column, one JSON line
per (dtype, shape, form), with avgs -- aqg_scan(AVGS) / aqg_grouped_scan_flat(AVGS): the same three-kernel structure and, for the
constant-alpha form, the same bytes per row -- timed beside it on the same buffers in the same process.  No pass / fail threshold
(DESIGN.md section 4.15 holds the numbers).

    python tools/ema_probe.py [--n 1e9] [--dtypes int32,double] [--shapes flat,g100,g1e5] [--reps 21]

Columns from aqg_gen_column: the int32 column v1; the double column is an ema of it (any doubles do); the decay column is
aqg_decay_from_times of the id column.  The grouped shapes time the call over columns already in the flat layout; the flatten is not
part of it.  ms: HIP events around the whole call (aqg_timer_start / aqg_timer_stop_ms): the median, the least and the greatest of --reps
timed calls after two warm-up calls.  frac_roofline: the call's algorithmic bytes -- inputs read twice, result written once -- over its
time, against 8 TB/s."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import EMA_ADJUSTED, EMA_RECURSIVE

GEN_ID1, GEN_ID3, GEN_V1 = 0, 2, 6
SCAN_AVGS = 1
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
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--dtypes", default="int32,double")
    ap.add_argument("--shapes", default="flat,g100,g1e5")
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    gen = lambda col, K: d.gen_column(col, 42, 0, n, n, K)
    xi = gen(GEN_V1, 100)
    ids = gen(GEN_ID3, max(1, n // 100_000))
    dec = d.decay_from_times(ids, 1e4, keep=True)
    xd = d.ema(xi, alpha=0.5, keep=True)
    out = d.empty(n, np.float64)
    for shape in a.shapes.split(","):
        gb = None
        if shape != "flat":
            keys = gen(GEN_ID1, 100) if shape == "g100" else ids
            gb = d.groupby_build([keys])
        for dt in a.dtypes.split(","):
            x = xi if dt == "int32" else xd
            esz = x.dtype.itemsize
            if gb is None:
                base = timed(d, a.reps, lambda: d.scan(SCAN_AVGS, x, keep=True, out=out))
            else:
                base = timed(d, a.reps, lambda: d.grouped_scan(gb, SCAN_AVGS, x, flat=True, keep=True, out=out))
            base_ms = float(np.median(base))
            for mode, mname in ((EMA_RECURSIVE, "recursive"), (EMA_ADJUSTED, "adjusted")):
                for form, kw, nbytes in (("alpha", {"alpha": 0.1}, 2 * esz + 8), ("decay", {"decay": dec}, 2 * (esz + 8) + 8)):
                    if gb is None:
                        times = timed(d, a.reps, lambda: d.ema(x, mode=mode, keep=True, out=out, **kw))
                    else:
                        times = timed(d, a.reps, lambda: d.grouped_ema(gb, x, mode=mode, flat=True, keep=True, out=out, **kw))
                    ms = float(np.median(times))
                    print(json.dumps({"shape": shape, "groups": 1 if gb is None else gb.ngroups, "n": n, "dtype": dt, "mode": mname, "form": form,
                                      "ms": round(ms, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                                      "kernel_ms_last": round(d.last_kernel_ms(), 3), "avgs_ms": round(base_ms, 3), "ratio_to_avgs": round(ms / base_ms, 3),
                                      "frac_roofline": round(n * nbytes / (ms * 1e-3) / HBM, 3)}), flush=True)
        if gb is not None:
            gb.destroy()
    d.close()


if __name__ == "__main__":
    main()
