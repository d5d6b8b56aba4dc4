"""The model of the as-of join (include/aqg.h: aqg_join_asof).

The reference runs its joins in MonetDB and has no as-of join at all, so the contract is the library's own and this file states it
twice in plain Python / numpy.  A side is a list of 0..8 key columns in the (tag, data) format of tests/join_keys_model.py, whose
tuple equality is used as it stands (-0.0 == +0.0, a row holding a NaN key matches nothing), plus one numeric `on` column.

With B(i) = the build rows whose key tuple equals probe row i's and whose `on` is not NaN:
    BACKWARD   the row of B(i) with the largest `on` <= probe `on` (< under strict); among rows of that `on` the HIGHEST row id
    FORWARD    the row of B(i) with the smallest `on` >= probe `on` (> under strict); among rows of that `on` the LOWEST row id
    no such row, a probe row whose `on` is NaN: 0xFFFFFFFF
Order is numeric, -0.0 == +0.0.  Without key columns every row is in one group.

asof_rows         brute force: per probe row, a loop-free numpy restatement of the sentences above over the VALUES of its tuple's
                  build rows (numpy compares them numerically; every comparison with a NaN is false)
asof_rows_sorted  the way a device does it: order-preserving unsigned IMAGES of `on`, the build rows ordered by (group, image, row),
                  one binary search per probe row in its group's segment.  `mutant` plants one deliberate mistake
                  (tests/test_asof_model.py asserts that the named cases tell every mutant from the model).
tests/test_asof_model.py holds the two equal and pins them to recorded answers of pandas merge_asof (tests/golden/asof_merge_asof.json)."""
import numpy as np

import join_keys_model as jkm

NONE = 0xFFFFFFFF
BACKWARD, FORWARD = 0, 1
LDS, HBM, NOKEYS, PRESORTED = 1, 2, 4, 8             # aqg_join_asof_last

MUTANTS = ("ties_wrong_end", "strict_ignored", "bounds_swapped", "segment_end_plus_1", "segment_start_minus_1", "nan_build_accepted",
           "nan_probe_answered", "unsigned_as_signed", "negative_zero_below", "unmatched_to_group_0")


def _tuples(cols, n):
    return jkm.rows(cols) if cols else [()] * n


# ---- brute force -------------------------------------------------------------------------------------------------------------------
def asof_rows(build_cols, build_on, probe_cols, probe_on, direction, strict):
    assert direction in (BACKWARD, FORWARD)
    bon, pon = np.asarray(build_on), np.asarray(probe_on)
    assert bon.dtype == pon.dtype
    table = {}
    for r, t in enumerate(_tuples(build_cols, len(bon))):
        if t is not None:
            table.setdefault(t, []).append(r)
    table = {t: np.array(r, dtype=np.int64) for t, r in table.items()}
    out = np.full(len(pon), NONE, dtype=np.uint32)
    for i, t in enumerate(_tuples(probe_cols, len(pon))):
        rows = table.get(t) if t is not None else None
        if rows is None:
            continue
        x, p = bon[rows], pon[i]
        if direction == BACKWARD:
            ok = x < p if strict else x <= p
        else:
            ok = x > p if strict else x >= p
        if not ok.any():
            continue
        rows, x = rows[ok], x[ok]
        if direction == BACKWARD:
            out[i] = rows[x == x.max()].max()
        else:
            out[i] = rows[x == x.min()].min()
    return out


# ---- images, segments, binary search -------------------------------------------------------------------------------------------------
SIGN = np.uint64(1 << 63)
NAN_IMAGE = np.uint64(0xFFF8000000000000)


def image(a, mutant=None):
    """uint64 images whose unsigned order is the numeric order of `a`: both zeros one image, every NaN one image above +inf"""
    a = np.asarray(a)
    if a.dtype.kind == "u":
        if mutant == "unsigned_as_signed":
            return a.view(np.dtype("i%d" % a.dtype.itemsize)).astype(np.int64).view(np.uint64) ^ SIGN
        return a.astype(np.uint64)
    if a.dtype.kind == "i":
        return a.astype(np.int64).view(np.uint64) ^ SIGN
    assert a.dtype.kind == "f"
    b = a.astype(np.float64).view(np.uint64).copy()              # float32 -> float64 is exact and keeps the order
    if mutant != "negative_zero_below":
        b[(b & ~SIGN) == 0] = 0
    b[(b & ~SIGN) > np.uint64(0x7FF0000000000000)] = np.uint64(0x7FF8000000000000)
    return np.where(b & SIGN != 0, ~b, b | SIGN)


def group_ids(build_cols, nb, probe_cols, npr):
    """(gid of every build row, G, gid of every probe row or -1): dense ids by first occurrence, a NaN row a group of its own"""
    ids, gb = {}, np.empty(nb, np.int64)
    G = 0
    for r, t in enumerate(_tuples(build_cols, nb)):
        if t is None or t not in ids:
            if t is not None:
                ids[t] = G
            gb[r] = G
            G += 1
        else:
            gb[r] = ids[t]
    gp = np.array([ids.get(t, -1) if t is not None else -1 for t in _tuples(probe_cols, npr)], dtype=np.int64).reshape(npr)
    return gb, G, gp


def asof_rows_sorted(build_cols, build_on, probe_cols, probe_on, direction, strict, mutant=None):
    assert direction in (BACKWARD, FORWARD) and (mutant is None or mutant in MUTANTS)
    bon, pon = np.asarray(build_on), np.asarray(probe_on)
    nb, npr = len(bon), len(pon)
    out = np.full(npr, NONE, dtype=np.uint32)
    if nb == 0 or npr == 0:
        return out
    fp = bon.dtype.kind == "f"
    gb, G, gp = group_ids(build_cols, nb, probe_cols, npr)
    if mutant == "unmatched_to_group_0":
        gp[gp < 0] = 0
    bimg, key = image(bon, mutant), image(pon, mutant)
    rows = np.arange(nb)
    order = np.lexsort((-rows if mutant == "ties_wrong_end" else rows, bimg, gb))
    simg = bimg[order]
    off = np.searchsorted(gb[order], np.arange(G + 1))
    if mutant == "strict_ignored":
        strict = False
    upper = (direction == BACKWARD) != bool(strict)              # upper bound: the first image above the key; lower: not below it
    if mutant == "bounds_swapped":
        upper = not upper
    live = gp >= 0
    if fp and mutant != "nan_probe_answered":
        live &= key != NAN_IMAGE
    for g in np.unique(gp[live]):
        at = np.nonzero(live & (gp == g))[0]
        b, e = int(off[g]), int(off[g + 1])
        if mutant == "segment_end_plus_1":
            e = min(e + 1, nb)
        if mutant == "segment_start_minus_1":
            b = max(b - 1, 0)
        pos = b + np.searchsorted(simg[b:e], key[at], side="right" if upper else "left")
        if direction == BACKWARD:
            ok, p = pos > b, pos - 1
        else:
            ok, p = pos < e, pos
        p = np.where(ok, p, 0)
        if fp and direction == FORWARD and mutant != "nan_build_accepted":
            ok &= simg[p] != NAN_IMAGE                           # the NaN tail of a segment is nobody's partner
        out[at[ok]] = order[p[ok]]
    return out


def presorted(build_on):
    """the build side's `on` is non-decreasing in image order: NaNs, if any, only at the end"""
    im = image(build_on)
    return bool(np.all(im[:-1] <= im[1:]))


def sort_passes(build_cols, build_on):
    """the digit passes of the ordering step: the byte positions at which the sort keys vary -- the dense group ids (4 bytes, only
    with key columns) and, unless the side is presorted, the images of `on` in their own width"""
    bon = np.asarray(build_on)
    n = 0
    if build_cols:
        gb, _, _ = group_ids(build_cols, len(bon), [], 0)
        n += sum(len(np.unique((gb >> (8 * d)) & 255)) > 1 for d in range(4))
    if not presorted(bon):
        n += _image_passes(bon)
    return n


def _image_passes(bon):
    """varying byte positions of the column's images in the column's own width (the images aqg_sort_rows sorts on)"""
    w = bon.dtype.itemsize
    if bon.dtype.kind == "f" and w == 4:
        b = bon.view(np.uint32).astype(np.uint64)
        b[(b & np.uint64(0x7FFFFFFF)) == 0] = 0
        b[(b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)] = np.uint64(0x7FC00000)
        im = np.where(b & np.uint64(0x80000000) != 0, ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    elif bon.dtype.kind == "i":
        im = bon.view(np.dtype("u%d" % w)).astype(np.uint64) ^ np.uint64(1 << (8 * w - 1))
    else:
        im = image(bon)
    return sum(len(np.unique((im >> np.uint64(8 * d)) & np.uint64(255))) > 1 for d in range(w))
