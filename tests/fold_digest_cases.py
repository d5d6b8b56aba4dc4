"""The floating folds whose exact bits tests/golden/fold_digests.json pins (tools/gen_fold_digests.py writes it, tests/test_gpu_fold_digests.py
holds the device to it).  The other tests hold floating sums and averages to an error bound; a change of the BRACKETING -- which
operands the block tree of aquery2_amd/csrc/fold_tree.hpp combines in which order -- stays within that bound and shows only here.

Values: float32 and float64, normal(0, 100) with a stretch of 1e30 among them, seeded.  Stamps: int64 0, 1, 2, ...  Ops: SUM and AVG.
Every shape is chosen for the path through the tree it takes (the comments below); the cases of tests/wj_cases.py and
tests/timewin_cases.py that already have such a shape are used by name.  outputs(dev) runs them all through the public Python API."""
import numpy as np

import timewin_cases
import wj_cases
from golden_util import digest

SUM, AVG, CLOSED = 1, 2, 1                                 # AQG_RANGEW_SUM, AQG_RANGEW_AVG, AQG_RANGEW_CLOSED
STAGED, INPLACE = 16, 32                                   # AQG_WJ_FOLD_*
OPS = (("sum", SUM), ("avg", AVG))
DTYPES = (np.float32, np.float64)
N_TILES = 3 * 2048 + 130                                   # three tiles of the fold kernel and a part of one
N_LEVEL3 = 262144 + 130                                    # S[2] / P[2] are reached
INF = float("inf")


def column(n, dtype, seed, late=False):
    """the 1e30s absorb every sum they are part of: they stand early in the column, so that most windows of a finite span and most
    intervals do not hold them, or (late) near its end, so that the running sums in front of them do not"""
    x = np.random.default_rng(4200 + seed).normal(0, 100, n)
    at = n - 150 if late else n // 50
    x[at:at + 97] = 1e30
    return x.astype(dtype)


def intervals(n, m, seed):
    """m queries [lo, hi): seeded uniform ends, the first ones replaced by hand-placed ends on, one before and one after 64, 4096 and
    262144, both ends in one block, in adjacent blocks, lo > hi and hi > n"""
    rng = np.random.default_rng(4300 + seed)
    lo, hi = rng.integers(0, n + 1, m), rng.integers(0, n + 1, m)
    short = rng.random(m) < 0.5
    hi = np.where(short, np.minimum(lo + rng.integers(0, 300, m), n), hi)
    pts = sorted({0, 1, n - 1, n} | {min(k + d, n) for k in (64, 4096, 262144) if k - 1 <= n for d in (-1, 0, 1)})
    hand = [(a, b) for a in pts for b in pts]
    hand += [(5, 9), (70, 100), (63, 65), (64, 128), (100, 140), (128, 192), (70, 3), (n - 3, n + 1000), (0, 0xFFFFFFFF), (n, n + 5), (1, n - 1)]
    assert len(hand) <= m
    lo[:len(hand)] = [a for a, _ in hand]
    hi[:len(hand)] = [b for _, b in hand]
    return lo.astype(np.uint32), hi.astype(np.uint32)


def outputs(dev):
    """name -> (digest of the output's bits, AQG_WJ_FOLD_* route or None), in a fixed order"""
    out = {}
    for dt in DTYPES:
        tag = np.dtype(dt).name
        # aqg_rangew, flat, closed: a window inside one block / over two adjacent blocks / about 15 whole blocks, all staged (the direct
        # loop over the staged level 1) / windows that begin in front of the staged tiles (S[1] / P[1]) / the running scan
        t = np.arange(N_TILES, dtype=np.int64)
        xd, xl, td = dev.to_device(column(N_TILES, dt, 1)), dev.to_device(column(N_TILES, dt, 1, late=True)), dev.to_device(t)
        for span in (5, 100, 1000, 3000, INF):
            for on, op in OPS:
                got = dev.rangew(op, td, span, xl if span == INF else xd, frame=CLOSED)
                out["rangew/%s/n%d/span%g/%s" % (tag, N_TILES, span, on)] = (digest(got), None)
        # aqg_grouped_rangew: three groups of unequal size
        sizes = (1000, 3200, N_TILES - 4200)
        keys = np.repeat(np.arange(3, dtype=np.int32), sizes)[np.random.default_rng(4400).permutation(N_TILES)]
        gb = dev.groupby_build([keys])
        for span in (100, INF):
            for on, op in OPS:
                out["grouped_rangew/%s/n%d/span%g/%s" % (tag, N_TILES, span, on)] = (digest(dev.grouped_rangew(gb, op, td, span, xd, frame=CLOSED)), None)
        gb.destroy()
        xd.free(); xl.free(); td.free()
        # aqg_rangew over a tree of three levels above the rows
        t = np.arange(N_LEVEL3, dtype=np.int64)
        xd, xl, td = dev.to_device(column(N_LEVEL3, dt, 2)), dev.to_device(column(N_LEVEL3, dt, 2, late=True)), dev.to_device(t)
        for span in (200000, INF):
            for on, op in OPS:
                got = dev.rangew(op, td, span, xl if span == INF else xd, frame=CLOSED)
                out["rangew/%s/n%d/span%g/%s" % (tag, N_LEVEL3, span, on)] = (digest(got), None)
        # aqg_interval_fold: INPLACE over that column, STAGED over a short one
        for n, m, want in ((N_LEVEL3, 4096, INPLACE), (4097, 65536, STAGED)):
            xf = xd if n == N_LEVEL3 else dev.to_device(column(n, dt, 3))
            lo, hi = intervals(n, m, n % 7)
            ld, hd = dev.to_device(lo), dev.to_device(hi)
            for on, op in OPS:
                got = dev.interval_fold(op, xf, ld, hd, fill=-7.0)
                out["interval_fold/%s/n%d/m%d/%s" % (tag, n, m, on)] = (digest(got), want)
                assert dev.join_window_last()[0] == want, (n, m, dev.join_window_last())
            ld.free(); hd.free()
            if xf is not xd:
                xf.free()
        xd.free(); xl.free(); td.free()
    # the named cases of the other modules with floating values
    folds = wj_cases.folds()
    for name in ("edges_level2_f64", "staged_f64", "staged_1e30", "values_1e30", "f32"):
        f = folds[name]
        for on, op in OPS:
            out["wj_cases.folds/%s/%s" % (name, on)] = (digest(dev.interval_fold(op, f.x, f.lo, f.hi, fill=-7.0)), None)
    for c in timewin_cases.grouped_cases():
        if c.name in ("g-1e30-beside-ones", "g-tile-edges"):
            keys, t_row, x_row = c.rows()
            gb = dev.groupby_build([keys])
            for on, op in OPS:
                out["timewin_cases.grouped/%s/%s" % (c.name, on)] = (digest(dev.grouped_rangew(gb, op, t_row, c.span, x_row, frame=c.frame)), None)
            gb.destroy()
    return out
