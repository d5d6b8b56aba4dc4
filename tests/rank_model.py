"""The contract of aqg_rank / aqg_grouped_rank(_flat) (include/aqg.h, ranking section), stated twice:

  five_sorted    a stable np.lexsort over (group, key image, position) and a walk over the tie runs of that order
  five_counting  the O(c^2) counting definition per slice: rows whose image is less, equal, equal and in front, and the distinct images
                 that are less

Both give a row's five integers (min, max, dense, first, c); `finish` turns them into a method's value.  The two must agree on every
case (tests/test_rank_model.py).  `bug` plants one of MISTAKES into the first statement: the cases must refuse every one of them."""
import numpy as np

MIN, MAX, DENSE, FIRST, AVERAGE, PERCENT, CUME_DIST, NTILE = range(8)
METHODS = (MIN, MAX, DENSE, FIRST, AVERAGE, PERCENT, CUME_DIST, NTILE)
METHOD_NAMES = ("min", "max", "dense", "first", "average", "percent", "cume_dist", "ntile")
ASC, DESC = 0, 1

MISTAKES = ("ties_by_descending_position", "nans_not_tied", "negative_zero_less", "desc_reverses_first", "max_off_at_group_end",
            "dense_not_restarted", "head_lost_at_tile_edge", "percent_divides_by_c", "ntile_remainder_last", "ranks_cross_groups")


def is_double(method):
    return method in (AVERAGE, PERCENT, CUME_DIST)


def out_dtype(method):
    return np.dtype(np.float64 if is_double(method) else np.uint32)


def image(x, bug=None):
    """the order-preserving unsigned image of key_image.hpp, widened to uint64: unsigned order of images == value order under ASC"""
    x = np.asarray(x)
    dt = x.dtype
    if dt == np.bool_:
        return x.astype(np.uint64)
    if dt.kind == "u":
        return x.astype(np.uint64)
    if dt.kind == "i":
        return x.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    bits = dt.itemsize * 8
    b = x.view(np.uint32 if bits == 32 else np.uint64).astype(np.uint64)
    sign, full = np.uint64(1 << (bits - 1)), np.uint64((1 << bits) - 1)
    expo = np.uint64(0x7f800000 if bits == 32 else 0x7ff0000000000000)
    qnan = np.uint64(0x7fc00000 if bits == 32 else 0x7ff8000000000000)
    mag = b & ~sign & full
    if bug != "negative_zero_less":
        b = np.where(mag == 0, np.uint64(0), b)
    if bug != "nans_not_tied":
        b = np.where(mag > expo, qnan, b)
    return np.where((b & sign) != 0, ~b & full, b | sign)


def group_ids(starts, n):
    gid = np.zeros(n, np.int64)
    gid[np.asarray(starts[1:], np.int64)] = 1
    return np.cumsum(gid)


def five_sorted(x, starts, order, bug=None, tile=None):
    """(min, max, dense, first, c) of every row: x in the layout scanned, slices [starts[g], starts[g+1])"""
    n = len(x)
    starts = np.asarray(starts, np.int64)
    gid = group_ids(starts, n)
    img = image(x, bug)
    pos = np.arange(n)
    if order == DESC and bug == "desc_reverses_first":
        srt = np.lexsort((pos, img, gid))
        ends = np.append(starts[1:], n)
        srt = np.concatenate([srt[s:e][::-1] for s, e in zip(starts, ends)]) if n else srt
    else:
        key = ~img if order == DESC else img
        srt = np.lexsort((-pos if bug == "ties_by_descending_position" else pos, key, gid))
    sg, si = gid[srt], img[srt]
    i = np.arange(n)
    gs = np.ones(n, bool)
    gs[1:] = sg[1:] != sg[:-1]
    head = gs.copy()
    head[1:] |= si[1:] != si[:-1]
    if bug == "ranks_cross_groups":
        gs[1:] = False
    if bug == "head_lost_at_tile_edge" and tile:
        head[tile::tile] &= gs[tile::tile]
    # the walk: the head of a row's run, the head of the next run, the start and the end of its group
    hd = np.maximum.accumulate(np.where(head, i, 0))
    nx = np.minimum.accumulate(np.where(head, i, n)[::-1])[::-1]
    nx = np.append(nx[1:], n)                                # the next head strictly behind the row
    g0 = np.maximum.accumulate(np.where(gs, i, 0))
    g1 = np.minimum.accumulate(np.where(gs, i, n)[::-1])[::-1]
    g1 = np.append(g1[1:], n)
    heads = np.cumsum(head)
    dense = heads - heads[g0] + 1
    if bug == "dense_not_restarted":
        dense = heads
    mn, mx, first, c = hd - g0 + 1, nx - g0, i - g0 + 1, g1 - g0
    if bug == "max_off_at_group_end":
        mx = np.where(nx == g1, mx - 1, mx)
    out = [np.empty(n, np.int64) for _ in range(5)]
    for o, v in zip(out, (mn, mx, dense, first, c)):
        o[srt] = v
    return tuple(out)


def five_counting(x, starts, order):
    """the counting definition, slice by slice: less = rows that sort strictly before, eq = rows that tie, eqb = ties in front"""
    n = len(x)
    img = image(x)
    if order == DESC:
        img = ~img
    out = [np.empty(n, np.int64) for _ in range(5)]
    ends = list(starts[1:]) + [n]
    for s, e in zip(starts, ends):
        im = img[s:e]
        c = e - s
        j = np.arange(c)
        first_occ = np.empty(c, bool)
        res = [np.empty(c, np.int64) for _ in range(4)]
        for b0 in range(0, c, 1024):                         # row blocks bound the c x c tables
            rows = slice(b0, min(c, b0 + 1024))
            eqm = im[None, :] == im[rows, None]
            ltm = im[None, :] < im[rows, None]
            res[0][rows] = ltm.sum(1)
            res[1][rows] = eqm.sum(1)
            res[2][rows] = (eqm & (j[None, :] < j[rows, None])).sum(1)
        first_occ[:] = res[2] == 0
        for b0 in range(0, c, 1024):
            rows = slice(b0, min(c, b0 + 1024))
            res[3][rows] = ((im[None, :] < im[rows, None]) & first_occ[None, :]).sum(1)
        less, eq, eqb, dless = res
        for o, v in zip(out, (less + 1, less + eq, dless + 1, less + eqb + 1, np.full(c, c))):
            o[s:e] = v
    return tuple(out)


def finish(method, k, five, bug=None):
    """a method's value from the five integers: uint32, or float64 computed with ONE IEEE division"""
    mn, mx, dense, first, c = five
    if method == MIN:
        return mn.astype(np.uint32)
    if method == MAX:
        return mx.astype(np.uint32)
    if method == DENSE:
        return dense.astype(np.uint32)
    if method == FIRST:
        return first.astype(np.uint32)
    if method == AVERAGE:
        return (mn + mx).astype(np.float64) * 0.5
    if method == PERCENT:
        den = c if bug == "percent_divides_by_c" else c - 1
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(c == 1, 0.0, (mn - 1).astype(np.float64) / den.astype(np.float64))
    if method == CUME_DIST:
        return mx.astype(np.float64) / c.astype(np.float64)
    assert method == NTILE and k >= 1
    q, r, o = c // k, c % k, first - 1
    if bug == "ntile_remainder_last":                        # the LAST r buckets take the extra row
        narrow = (k - r) * q
        return np.where(o < narrow, o // np.maximum(q, 1), (k - r) + (o - narrow) // (q + 1)).astype(np.uint32) + np.uint32(1)
    wide = r * (q + 1)
    return (np.where(o < wide, o // (q + 1), r + (o - wide) // np.maximum(q, 1)) + 1).astype(np.uint32)


def rank(x, starts, method, order=ASC, k=0, bug=None, tile=None):
    """the answer of aqg_rank (starts = [0]) / aqg_grouped_rank_flat (x in the flat layout) by the first statement"""
    return finish(method, k, five_sorted(x, starts, order, bug, tile), bug)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
