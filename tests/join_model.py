"""The numpy model of the hash joins (include/aqg.h: aqg_join_lookup, aqg_join_count / aqg_join_pairs, aqg_join_groupby_sum).

The reference runs its joins in MonetDB, so the contract is the library's own and this model states it: an inner equi-join on
one integer key column, pairs ordered by probe row and then by ascending build row; the look-up form answers with the LOWEST
build row of a key.  Two keys are equal when their VALUES within the one key dtype are equal -- nothing here sign-extends or
reinterprets a key, which is what makes it a second opinion on the kernels' 64-bit key images.  Plain sorting and searching,
no C behind it; tests/test_join_model.py holds it to the oracle's restatement."""
import numpy as np

NONE = 0xFFFFFFFF


def _keys(build, probe):
    build, probe = np.asarray(build), np.asarray(probe)
    assert build.dtype == probe.dtype and build.dtype.kind in "iub", (build.dtype, probe.dtype)
    if build.dtype == np.bool_:
        build, probe = build.astype(np.uint8), probe.astype(np.uint8)
    return build, probe


def _runs(build, probe):
    """(stable order of the build rows, first and one-past-last position of every probe key's run in that order)"""
    order = np.argsort(build, kind="stable")
    sb = build[order]
    by_key = np.argsort(probe, kind="stable")       # searching in key order walks the build side once: several times faster at 1e6 rows
    sp = probe[by_key]
    lo, hi = np.empty(len(probe), dtype=np.int64), np.empty(len(probe), dtype=np.int64)
    lo[by_key], hi[by_key] = np.searchsorted(sb, sp, side="left"), np.searchsorted(sb, sp, side="right")
    return order, lo, hi


def lookup(build, probe):
    """uint32[np]: the lowest build row whose key equals probe[i], else 0xFFFFFFFF"""
    build, probe = _keys(build, probe)
    out = np.full(len(probe), NONE, dtype=np.uint32)
    if len(build) == 0 or len(probe) == 0:
        return out
    order, lo, hi = _runs(build, probe)
    hit = hi > lo
    out[hit] = order[lo[hit]]                       # stable order: the first row of a run is the lowest
    return out


def pairs(build, probe):
    """(probe_rows, build_rows), uint32: every matching pair, by probe row, then by ascending build row"""
    build, probe = _keys(build, probe)
    if len(build) == 0 or len(probe) == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    order, lo, hi = _runs(build, probe)
    cnt = hi - lo
    total = int(cnt.sum())
    probe_rows = np.repeat(np.arange(len(probe), dtype=np.int64), cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    build_rows = order[np.repeat(lo, cnt) + within]
    return probe_rows.astype(np.uint32), build_rows.astype(np.uint32)


def count(build, probe):
    """the number of matching pairs, a Python int"""
    build, probe = _keys(build, probe)
    if len(build) == 0 or len(probe) == 0:
        return 0
    _, lo, hi = _runs(build, probe)
    return sum((hi - lo).tolist())                  # Python ints: exact beyond 2^64


def star_sum(dim_key, dim_w, fk, gkey, val):
    """fact JOIN dim ON fk = dim_key, sum(val * w) BY gkey -> (keys, first_rows, sums): the groups in first-occurrence order
    among the joined rows, first_rows as row ids of the FACT table (uint32), sums as exact Python ints.  Of duplicate dimension
    keys the lowest row wins; fact rows without a partner are dropped."""
    dim_w, gkey, val = np.asarray(dim_w), np.asarray(gkey), np.asarray(val)
    row = lookup(dim_key, fk)
    rows = np.nonzero(row != NONE)[0]
    if len(rows) == 0:
        return gkey[:0].copy(), np.zeros(0, np.uint32), []
    g = gkey[rows]
    uniq, first_idx, inv = np.unique(g, return_index=True, return_inverse=True)
    perm = np.argsort(first_idx, kind="stable")                 # groups by their first joined row
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[perm] = np.arange(len(uniq))
    gid = rank[inv.reshape(-1)]
    # exact sums of products up to 2^64 in magnitude: 16-bit limbs keep every partial sum of <= 2^21 rows below 2^54 in int64
    v = val[rows].astype(np.int64)
    w = dim_w[row[rows]].astype(np.int64)
    assert len(rows) <= 1 << 21
    v_hi, v_lo, w_hi, w_lo = v >> 16, v & 0xFFFF, w >> 16, w & 0xFFFF
    by_group = np.argsort(gid, kind="stable")
    starts = np.searchsorted(gid[by_group], np.arange(len(uniq)))
    part = [np.add.reduceat((a * b)[by_group], starts).tolist() for a, b in ((v_hi, w_hi), (v_hi, w_lo), (v_lo, w_hi), (v_lo, w_lo))]
    sums = [(hh << 32) + ((hl + lh) << 16) + ll for hh, hl, lh, ll in zip(*part)]
    return uniq[perm], rows[first_idx[perm]].astype(np.uint32), sums
