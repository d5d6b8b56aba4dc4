"""The numpy model of aqg_median / aqg_grouped_median (include/aqg.h, median section).

No executable reference median exists (the reference declares the name, common/types.py:343, and leaves the body and the h2o query
out), so the model lives here: the rows of every group in ascending order of their key IMAGE -- the order of aqg_sort_rows under
AQG_ORDER_ASC -- and the element of rank (c-1)/2 (lower) or c/2 (upper) of the c rows."""
import numpy as np

SEL_LOWER, SEL_UPPER = 0, 1


def image(x):
    """the order-preserving unsigned image of a column, as tests/test_gpu_sort.py::images builds it for ORDER_ASC"""
    x = np.asarray(x)
    if x.dtype == np.bool_:
        x = x.astype(np.uint8)
    if x.dtype.kind == "f":
        u = np.uint32 if x.itemsize == 4 else np.uint64
        b = x.view(u).copy()
        sign = u(1) << u(8 * x.itemsize - 1)
        b[x == 0] = 0
        b[np.isnan(x)] = x.dtype.type(np.nan).view(u) & ~sign
        return np.where(b & sign, ~b, b | sign).astype(u)
    u = np.dtype(f"u{x.itemsize}")
    b = x.view(u).copy()
    if x.dtype.kind == "i":
        b ^= u.type(1 << (8 * x.itemsize - 1))
    return b


def grouped_both(x, gid, ngroups):
    """{which: (median of every group, flags)} for both medians from one sort: x[i] belongs to group gid[i] (dense ids below ngroups,
    every group non-empty).  flags[g]: the answer of group g is compared by value, not by bits -- the rank lands on a zero of a group
    that holds both zeros, or on a NaN (which zero / which NaN comes back is unspecified)."""
    x = np.asarray(x)
    gid = np.asarray(gid, dtype=np.int64)
    if ngroups == 0:
        return {w: (x[:0].copy(), np.zeros(0, dtype=bool)) for w in (SEL_LOWER, SEL_UPPER)}
    counts = np.bincount(gid, minlength=ngroups)
    assert counts.min() >= 1, "every group holds a row"
    order = np.lexsort((image(x), gid)) if ngroups > 1 else np.argsort(image(x), kind="stable")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    both = None
    if x.dtype.kind == "f":
        bits = x.view(np.uint32 if x.itemsize == 4 else np.uint64)
        neg_zero = (x == 0) & (bits != 0)
        pos_zero = (x == 0) & (bits == 0)
        both = (np.bincount(gid, weights=neg_zero, minlength=ngroups) > 0) & (np.bincount(gid, weights=pos_zero, minlength=ngroups) > 0)
    res = {}
    for which in (SEL_LOWER, SEL_UPPER):
        rank = counts // 2 if which == SEL_UPPER else (counts - 1) // 2
        out = x[order[starts + rank]]
        flags = np.zeros(ngroups, dtype=bool) if both is None else np.isnan(out) | ((out == 0) & both)
        res[which] = (out, flags)
    return res


def grouped(x, gid, ngroups, which=SEL_LOWER):
    """(median of every group, flags) for one of the two medians: see grouped_both"""
    assert which in (SEL_LOWER, SEL_UPPER)
    return grouped_both(x, gid, ngroups)[which]


def flat(x, which=SEL_LOWER):
    """(median of the whole column, flag); an empty column gives the type's zero (the header layer's `first` convention)"""
    x = np.asarray(x)
    if len(x) == 0:
        return np.zeros(1, dtype=x.dtype)[0], False
    out, flags = grouped(x, np.zeros(len(x), dtype=np.int64), 1, which)
    return out[0], bool(flags[0])


def flat_both(x):
    """{which: (median, flag)} of the whole column from one sort (a non-empty column)"""
    r = grouped_both(x, np.zeros(len(x), dtype=np.int64), 1)
    return {w: (r[w][0][0], bool(r[w][1][0])) for w in r}


def same(got, want, flags):
    """bit for bit, except where `flags` says by value (==, or both NaN)"""
    got, want, flags = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(flags)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bit_eq = got.view(u) == want.view(u)
    with np.errstate(invalid="ignore"):
        val_eq = (got == want) | ((got != got) & (want != want))
    return bool(np.all(np.where(flags, val_eq, bit_eq)))


def first_occurrence_ids(*keys):
    """(gid per row, ngroups): dense group ids numbered by first occurrence of the key tuple (aqg_groupby_build's contract)"""
    n = len(keys[0])
    if n == 0:
        return np.zeros(0, dtype=np.int64), 0
    order = np.lexsort(keys[::-1])
    change = np.zeros(n, dtype=bool)
    change[0] = True
    for k in keys:
        ks = np.asarray(k)[order]
        change[1:] |= ks[1:] != ks[:-1]
    sorted_gid = np.cumsum(change) - 1                       # ids in key order
    first_row = np.full(sorted_gid[-1] + 1, n, dtype=np.int64)
    np.minimum.at(first_row, sorted_gid, order)
    renum = np.empty(len(first_row), dtype=np.int64)
    renum[np.argsort(first_row, kind="stable")] = np.arange(len(first_row))
    gid = np.empty(n, dtype=np.int64)
    gid[order] = renum[sorted_gid]
    return gid, len(first_row)
