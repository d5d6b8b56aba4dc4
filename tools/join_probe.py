"""The joins on composite and typed keys at size: ms per call of the shapes of DESIGN.md section 4.10, one JSON line per shape and call.

    python tools/join_probe.py [--n 1e9] [--shapes 1,2,3,4,5] [--reps 5]

Shapes (fact columns from aqg_gen_column, n rows; every fact row has a partner):
  1  one 4-byte key (id1), a 100-row dimension: aqg_join_keys_lookup beside aqg_join_lookup (the parent's entry), then
     aqg_join_keys_pairs INNER / LEFT / SEMI into preallocated outputs
  2  (id4, id5), two 4-byte columns, a 10^4-row dimension -- the PACKED form: aqg_join_keys_lookup beside the only composition the
     library offered before, aqg_groupby_build over the concatenation of both tables' key columns (dimension rows first; the group
     id of a fact row is its dimension row)
  3  (int64 id4, id5) on the same shape -- the WIDE form
  4  aqg_gather_fill beside aqg_gather on the full index of shape 1 (a 4-byte value column of the dimension)
  5  the one-key joins behind their probe: one 4-byte key, n / 1000 build rows of distinct keys, n / 10 probe rows that each match once
     (10^6 and 10^8 at the default n): aqg_join_count, aqg_join_pairs into preallocated outputs, aqg_join_keys_pairs INNER on the
     same columns into outputs of its own (`m` and the checksum of the build rows must agree)
ms: HIP events around the whole call (aqg_timer_start / aqg_timer_stop_ms), the median of --reps timed calls after one warm-up call;
`times_ms` carries every call, so the spread is on the line.  `kernel_ms` is the probe kernel alone (aqg_last_kernel_ms) where the call
records one.  `rows_per_s` and `roofline` (the share of 8 TB/s) count algorithmic bytes: the probe key bytes plus 4 per row.
`checksum` (the sum of the answers) must agree between the calls of a shape."""
import argparse
import ctypes as C
import json
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd import capi

GEN_ID1, GEN_ID4, GEN_ID5 = 0, 3, 4
ROOF = 8e12


def timed(d, reps, call):
    call()                                   # warm-up: code objects, workspace, pooled handle buffers
    times = []
    for _ in range(reps):
        d.sync()
        d.timer_start()
        call()
        times.append(d.timer_stop_ms())
    return times


def line(shape, call, n, key_bytes, times, **extra):
    ms = float(np.median(times))
    print(json.dumps({"shape": shape, "call": call, "n": n, "ms": round(ms, 4), "times_ms": [round(t, 4) for t in times], "rows_per_s": round(n / ms * 1e3, 0),
                      "roofline": round(n * (key_bytes + 4) / (ms * 1e-3) / ROOF, 3), **extra}), flush=True)


def prefix_sum(d, ptr, n):
    """the checksum: the sum of the first 2^24 answers (uint32 at `ptr`), on the host"""
    return int(capi.DevBuf(d, ptr, np.uint32, min(n, 1 << 24), owned=False).to_host().astype(np.uint64).sum())


def keys_lookup(d, bd, pd, out):
    _, dts, bp = d._keyargs(bd)
    _, _, pp = d._keyargs(pd)
    return lambda: d._chk(d.lib.aqg_join_keys_lookup(d.ctx, len(bd), dts, bp, bd[0].n, pp, pd[0].n, out.ptr), "aqg_join_keys_lookup")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--shapes", default="1,2,3,4,5")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, d = int(a.n), A.Device(0)
    shapes = [int(t) for t in a.shapes.split(",")]
    gen = lambda col, K: d.gen_column(col, 42, 0, n, n, K)
    out = d.empty(n, np.uint32)
    host_sum = lambda b: prefix_sum(d, b.ptr, n)
    if 1 in shapes or 4 in shapes:
        fk = gen(GEN_ID1, 100)
        dim = d.to_device(np.random.default_rng(1).permutation(np.arange(1, 101, dtype=np.int32)))
        call = keys_lookup(d, [dim], [fk], out)
        if 1 in shapes:
            old = lambda: d._chk(d.lib.aqg_join_lookup(d.ctx, dim.tag, C.c_void_p(dim.ptr), C.c_uint32(100), C.c_void_p(fk.ptr), C.c_uint32(n), C.c_void_p(out.ptr)), "aqg_join_lookup")
            for name, f in (("aqg_join_lookup", old), ("aqg_join_keys_lookup", call), ("aqg_join_lookup again", old)):
                t = timed(d, a.reps, f)
                line(1, name, n, 4, t, kernel_ms=round(d.last_kernel_ms(), 4), routes=d.join_last()[0] if "keys" in name else None, checksum=host_sum(out))
            pr, br = d.empty(n, np.uint32), d.empty(n, np.uint32)
            _, dts, bp = d._keyargs([dim])
            _, _, pp = d._keyargs([fk])
            m = C.c_uint64()
            for kind, name in ((capi.JOIN_INNER, "INNER"), (capi.JOIN_LEFT, "LEFT"), (capi.JOIN_SEMI, "SEMI")):
                f = lambda: d._chk(d.lib.aqg_join_keys_pairs(d.ctx, kind, 1, dts, bp, 100, pp, n, pr.ptr, br.ptr, n, C.byref(m)), "aqg_join_keys_pairs")
                t = timed(d, a.reps, f)
                line(1, "aqg_join_keys_pairs " + name, n, 4, t, m=m.value)
            pr.free(); br.free()
        if 4 in shapes:
            call()
            val = d.to_device(np.arange(100, dtype=np.int32) * 7 - 300)
            g = d.empty(n, np.int32)
            fill = np.array([-1], np.int32)
            for name, f in (("aqg_gather", lambda: d._chk(d.lib.aqg_gather(d.ctx, val.tag, C.c_void_p(val.ptr), C.c_void_p(out.ptr), C.c_uint32(n), C.c_void_p(g.ptr)), "aqg_gather")),
                            ("aqg_gather_fill", lambda: d._chk(d.lib.aqg_gather_fill(d.ctx, val.tag, val.ptr, out.ptr, n, fill.ctypes.data, g.ptr), "aqg_gather_fill"))):
                t = timed(d, a.reps, f)
                line(4, name, n, 4, t, checksum=prefix_sum(d, g.ptr, n))
            g.free()
        fk.free()
    for s in (2, 3):
        if s not in shapes:
            continue
        f4, f5 = gen(GEN_ID4, 100), gen(GEN_ID5, 100)
        combos = np.random.default_rng(2).permutation(10_000)
        d4, d5 = (combos // 100 + 1).astype(np.int32), (combos % 100 + 1).astype(np.int32)
        if s == 3:                                                  # the first column as int64: 12 bytes, the WIDE form
            wide = d.empty(n, np.int64)
            step = 1 << 26
            for o in range(0, n, step):                             # widened through the host in slices
                part = capi.DevBuf(d, f4.ptr + 4 * o, np.int32, min(step, n - o), owned=False).to_host().astype(np.int64)
                d._chk(d.lib.aqg_h2d(d.ctx, C.c_void_p(wide.ptr + 8 * o), part.ctypes.data_as(C.c_void_p), C.c_size_t(part.nbytes)), "aqg_h2d")
            f4.free()
            f4, d4 = wide, d4.astype(np.int64)
        bd = [d.to_device(d4), d.to_device(d5)]
        kb = f4.dtype.itemsize + 4
        t = timed(d, a.reps, keys_lookup(d, bd, [f4, f5], out))
        line(s, "aqg_join_keys_lookup", n, kb, t, kernel_ms=round(d.last_kernel_ms(), 4), routes=d.join_last()[0], checksum=host_sum(out))
        # the composition: one group-by build over dimension rows followed by fact rows (the concatenation is not timed)
        cat = []
        for b, f in zip(bd, (f4, f5)):
            c = d.empty(n + b.n, f.dtype)
            esz = f.dtype.itemsize
            d._chk(d.lib.aqg_d2d(d.ctx, C.c_void_p(c.ptr), C.c_void_p(b.ptr), C.c_size_t(b.n * esz)), "aqg_d2d")
            d._chk(d.lib.aqg_d2d(d.ctx, C.c_void_p(c.ptr + b.n * esz), C.c_void_p(f.ptr), C.c_size_t(n * esz)), "aqg_d2d")
            cat.append(c)
        f4.free(); f5.free()
        state = {"gb": None}

        def compose():
            if state["gb"] is not None:
                state["gb"].destroy()
            state["gb"] = d.groupby_build(cat)
        t = timed(d, a.reps, compose)
        rev = d.lib.aqg_groupby_reversemap(state["gb"].h) + 4 * 10_000              # the fact rows' group ids: their dimension rows
        line(s, "aqg_groupby_build over the concatenation", n, kb, t, groups=state["gb"].ngroups, checksum=prefix_sum(d, rev, n))
        state["gb"].destroy()
        for b in cat + bd:
            b.free()
    if 5 in shapes:
        nb5, np5 = max(n // 1000, 1), max(n // 10, 1)
        fk = d.gen_column(GEN_ID1, 42, 0, np5, np5, nb5)
        dim = d.to_device(np.random.default_rng(5).permutation(np.arange(1, nb5 + 1, dtype=np.int32)))
        outs = [(d.empty(np5, np.uint32), d.empty(np5, np.uint32)) for _ in range(2)]
        _, dts, bp = d._keyargs([dim])
        _, _, pp = d._keyargs([fk])
        m = C.c_uint64()
        one = (d.ctx, dim.tag, C.c_void_p(dim.ptr), C.c_uint32(nb5), C.c_void_p(fk.ptr), C.c_uint32(np5))
        (pr, br), (kpr, kbr) = outs
        calls = (("aqg_join_count", None, lambda: d._chk(d.lib.aqg_join_count(*one, C.byref(m)), "aqg_join_count")),
                 ("aqg_join_pairs", br, lambda: d._chk(d.lib.aqg_join_pairs(*one, C.c_void_p(pr.ptr), C.c_void_p(br.ptr), C.c_uint64(np5), C.byref(m)), "aqg_join_pairs")),
                 ("aqg_join_keys_pairs INNER", kbr, lambda: d._chk(d.lib.aqg_join_keys_pairs(d.ctx, capi.JOIN_INNER, 1, dts, bp, nb5, pp, np5, kpr.ptr, kbr.ptr, np5, C.byref(m)),
                                                                    "aqg_join_keys_pairs")))
        for name, rows, f in calls:
            t = timed(d, a.reps, f)
            line(5, name, np5, 4, t, build_rows=nb5, m=m.value, **({} if rows is None else {"checksum": prefix_sum(d, rows.ptr, np5)}))
        for b in (fk, dim, pr, br, kpr, kbr):
            b.free()
    d.close()


if __name__ == "__main__":
    main()
