"""The prefix scans at size: ms per call of every shape that runs the reduce-then-scan pass of csrc/scan_prefix.hpp -- whole-column sums /
avgs / vars, a resumed shard, the wide windows that go through an accumulator-form prefix, the chained mins (whose writer is the pass's)
-- the same over the flat layout of a grouping at 100 and at 1e5 groups with the per-group reductions, and the moving averages of
tools/ema_probe.py.  One JSON line per shape; no pass / fail threshold (profiles/r14_prefix_skeleton.md compares two builds).

    python tools/prefix_probe.py [--n 1e9] [--families column,flat,ema] [--reps 21] [--tag NAME]

Columns from aqg_gen_column: the int32 column v1; the float32 column v3; the int64 column is v1 + 0 in 64 bits, the double column an ema of v1
(any doubles do), the 16-bit columns are the first 2 n bytes of v1;
the decay column is aqg_decay_from_times of the id column.  The grouped shapes time the call over columns taken as already in the flat
layout; the flatten is not part of it.  ms: HIP events around the whole C-ABI call (aqg_timer_start / aqg_timer_stop_ms): the median, the
least and the greatest of --reps timed calls after two warm-up calls."""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import EMA_ADJUSTED, EMA_RECURSIVE

GEN_ID1, GEN_ID3, GEN_V1, GEN_V3 = 0, 2, 6, 8
OP_ADD = 0
SCAN = {"sums": 0, "avgs": 1, "mins": 2, "maxs": 3, "sumw": 4, "vars": 12, "varw": 14}
RED = {"sum": 0, "avg": 4, "var": 5}


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
    ap.add_argument("--families", default="column,flat,ema")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    n, d, fams = int(a.n), A.Device(0), a.families.split(",")
    gen = lambda col, K: d.gen_column(col, 42, 0, n, n, K)
    xi = gen(GEN_V1, 100)
    ids = gen(GEN_ID3, max(1, n // 100_000))
    out = d.empty(2 * n, np.uint64)                                            # 16 bytes per row: every result fits

    def report(family, shape, dtype, times, **more):
        print(json.dumps({"tag": a.tag, "family": family, "shape": shape, "dtype": dtype, "n": n, **more, "ms": round(float(np.median(times)), 3),
                          "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}), flush=True)

    if "column" in fams:
        xl = d.ewise(OP_ADD, xi, np.int64(0), keep=True)
        xd = d.ema(xi, alpha=0.5, keep=True)
        assert xl.dtype == np.int64 and xd.dtype == np.float64
        for name, x, w in (("sums", xi, 0), ("avgs", xi, 0), ("vars", xi, 0), ("sums", xl, 0), ("sums", xd, 0), ("sumw", xi, 20_000), ("sumw", xl, 20_000), ("varw", xi, 5000),
                           ("mins", xi, 0)):
            report("column", name + (str(w) if w else ""), x.dtype.name, timed(d, a.reps, lambda: d.scan(SCAN[name], x, w, keep=True, out=out)))
        report("column", "scan_resume sums", "int32", timed(d, a.reps, lambda: d.scan_resume(SCAN["sums"], xi, 12345, 1000, keep=True, out=out)))
        xl.free()
        xd.free()
    if "flat" in fams:
        x16, xu16 = (A.DevBuf(d, xi.ptr, np.dtype(t), n, owned=False) for t in (np.int16, np.uint16))     # the first 2 n bytes of v1: any bits do
        for shape, keys in (("g100", gen(GEN_ID1, 100)), ("g1e5", ids)):
            gb = d.groupby_build([keys])
            for name, w in (("sums", 0), ("avgs", 0), ("mins", 0), ("maxs", 0), ("vars", 0), ("sumw", 20_000)):
                report("flat", name + (str(w) if w else ""), "int32", timed(d, a.reps, lambda: d.grouped_scan(gb, SCAN[name], xi, w, flat=True, keep=True, out=out)),
                       groups=gb.ngroups, layout=shape)
            for name, x in (("sum", xi), ("var", xi), ("sum", x16), ("avg", xu16)):
                report("flat", "reduce " + name, x.dtype.name, timed(d, a.reps, lambda: d.grouped_reduce_flat(gb, RED[name], x)), groups=gb.ngroups, layout=shape)
            gb.destroy()
    if "ema" in fams:
        dec = d.decay_from_times(ids, 1e4, keep=True)
        xd = d.ema(xi, alpha=0.5, keep=True)
        xf = gen(GEN_V3, 100)
        for shape in ("flat", "g1e5"):
            gb = d.groupby_build([ids]) if shape == "g1e5" else None
            for x in (xi, xd, xf):
                for mode, mname in ((EMA_RECURSIVE, "recursive"), (EMA_ADJUSTED, "adjusted")):
                    for form, kw in (("alpha", {"alpha": 0.1}), ("decay", {"decay": dec})):
                        if gb is None:
                            times = timed(d, a.reps, lambda: d.ema(x, mode=mode, keep=True, out=out, **kw))
                        else:
                            times = timed(d, a.reps, lambda: d.grouped_ema(gb, x, mode=mode, flat=True, keep=True, out=out, **kw))
                        report("ema", mname + " " + form, x.dtype.name, times, groups=1 if gb is None else gb.ngroups, layout=shape)
            if gb is not None:
                gb.destroy()
    d.close()


if __name__ == "__main__":
    main()
