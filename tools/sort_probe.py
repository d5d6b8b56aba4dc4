"""aqg_sort_rows at size: ms per call, digit passes run, and GB/s per pass for the six key shapes of DESIGN.md "Device sort".

    python tools/sort_probe.py [n ...]            (default: 1e8 1e9)

ms/call: HIP events around the whole call (histogram, its one host round trip, every pass).  chain ms: aqg_last_kernel_ms, the passes
alone.  GB/s per pass: 20 B/row (a carried one-plane pass: upsweep reads the 4-byte image, the scatter reads {image, id} and writes
{image, id}) times n, over chain ms / passes -- a common yardstick, not each pass's exact bytes (kernel-level times: rocprofv3)."""
import sys

import numpy as np

sys.path.insert(0, ".")
import aquery2_amd as A
from aquery2_amd.capi import DOUBLE, INT32, INT64, UINT32, UINT128, ORDER_ASC, ORDER_DESC


def shapes(rng, n):
    yield "random uint32", [(UINT32, rng.integers(0, 2**32, n, dtype=np.uint32))], [ORDER_ASC]
    yield "random int64", [(INT64, rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64))], [ORDER_ASC]
    yield "int64 ids 1..100", [(INT64, rng.integers(1, 101, n, dtype=np.int64))], [ORDER_ASC]
    yield "two int32 keys", [(INT32, rng.integers(-2**31, 2**31 - 1, n, dtype=np.int32)),
                             (INT32, rng.integers(-2**31, 2**31 - 1, n, dtype=np.int32))], [ORDER_ASC, ORDER_DESC]
    yield "double", [(DOUBLE, rng.random(n))], [ORDER_ASC]
    yield "16-byte key", [(UINT128, rng.integers(0, 2**64, 2 * n, dtype=np.uint64))], [ORDER_ASC]


def main():
    sizes = [int(float(a)) for a in sys.argv[1:]] or [100_000_000, 1_000_000_000]
    d = A.Device(0)
    rng = np.random.default_rng(5)
    for n in sizes:
        for name, cols, orders in shapes(rng, n):
            keys = []
            for tag, a in cols:
                b = d.to_device(a)
                b.n, b._tag = n, tag
                keys.append(b)
            del cols
            out = d.empty(n, np.uint32)
            d.sort_rows(keys, orders, out=out, keep=True)      # warm-up: code objects, workspace
            reps = 5 if n <= 100_000_000 else 3
            times, chains = [], []
            for _ in range(reps):
                d.sync()
                d.timer_start()
                d.sort_rows(keys, orders, out=out, keep=True)
                times.append(d.timer_stop_ms())
                chains.append(d.last_kernel_ms())
            passes = d.sort_last_passes()
            ms, chain = float(np.median(times)), float(np.median(chains))
            gbps = 20 * n / (chain / passes) / 1e6 if passes else 0.0
            print(f"n={n:.0e} {name:18s} {ms:9.3f} ms/call  chain {chain:9.3f} ms  passes {passes}  {gbps:7.0f} GB/s per pass", flush=True)
            for b in keys:
                b._raw = None
                b.free()
            out.free()
    d.close()


if __name__ == "__main__":
    main()
