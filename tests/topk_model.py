"""The numpy model of aqg_topk / aqg_grouped_topk (include/aqg.h, top-k section) and the checker of a device answer.

The rows of every group of the FLAT layout in the order of aqg_sort_rows -- a stable argsort of the key image of median_model.image,
complemented for ORDER_DESC, so that equal images keep ascending positions -- and the first k of them.  `check` holds a device answer
to the contract without fixing WHICH rows are taken when more rows tie on the k-th image than there are slots left."""
import numpy as np

from median_model import image

ORDER_ASC, ORDER_DESC = 0, 1
MISSING = np.uint32(0xFFFFFFFF)


def keys_of(x, order):
    """the unsigned key a row is ranked by: ascending key = the order asked for"""
    assert order in (ORDER_ASC, ORDER_DESC)
    im = image(x)
    return ~im if order == ORDER_DESC else im


def _as_col(x):
    x = np.asarray(x)
    return x.astype(np.uint8) if x.dtype == np.bool_ else x


def topk(x, offsets, k, order):
    """(vals (G, k), pos (G, k) uint32, flags (G, k)) of a column in the flat layout: group g is x[offsets[g]:offsets[g + 1]].
    Slots past min(k, count) hold zero bytes / 0xFFFFFFFF.  flags: the slot is compared by value, not by bits -- a NaN, or a zero of
    a group that holds both zeros (which of the equal-image rows comes back is then visible in the bits)."""
    x = _as_col(x)
    offsets = np.asarray(offsets, dtype=np.int64)
    G = len(offsets) - 1
    vals = np.zeros((G, k), x.dtype)
    pos = np.full((G, k), MISSING, np.uint32)
    flags = np.zeros((G, k), bool)
    if G == 0 or len(x) == 0:
        return vals, pos, flags
    counts = np.diff(offsets)
    gid = np.repeat(np.arange(G), counts)
    key = keys_of(x, order)
    srt = np.lexsort((key, gid)) if G > 1 else np.argsort(key, kind="stable")        # both stable: equal keys keep ascending positions
    slot = np.arange(k)[None, :]
    valid = slot < counts[:, None]
    at = np.minimum(offsets[:-1, None] + slot, len(x) - 1)
    p = srt[at]
    pos[valid] = p[valid].astype(np.uint32)
    vals[valid] = x[p][valid]
    if x.dtype.kind == "f":
        bits = x.view(np.uint32 if x.itemsize == 4 else np.uint64)
        zero = x == 0
        both = (np.bincount(gid, weights=zero & (bits != 0), minlength=G) > 0) & (np.bincount(gid, weights=zero & (bits == 0), minlength=G) > 0)
        flags = valid & (np.isnan(vals) | ((vals == 0) & both[:, None]))
    return vals, pos, flags


def same(got, want, flags):
    """bit for bit, except where `flags` says by value (==, or both NaN)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bit_eq = got.view(u) == want.view(u)
    with np.errstate(invalid="ignore"):
        val_eq = (got == want) | ((got != got) & (want != want))
    return bool(np.all(np.where(flags, val_eq, bit_eq)))


def check(got_vals, got_pos, x, offsets, k, order, model=None):
    """raises AssertionError unless (got_vals, got_pos) is a valid answer for the flat-layout column x.  got_pos None: a call without
    positions; the values are then held to the model's, bit for bit where no slot is flagged and by key image elsewhere.
    model: topk(x, offsets, k2, order) for some k2 >= k, computed once by a caller that checks several k (its first k slots are used)."""
    x = _as_col(x)
    offsets = np.asarray(offsets, dtype=np.int64)
    G = len(offsets) - 1
    got_vals = _as_col(got_vals)
    assert got_vals.dtype == x.dtype and got_vals.shape == (G, k), ("shape / dtype", got_vals.dtype, got_vals.shape)
    want_vals, want_pos, flags = (a[:, :k] for a in model) if model is not None else topk(x, offsets, k, order)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
    counts = np.diff(offsets)
    valid = np.arange(k)[None, :] < counts[:, None]
    assert not got_vals.view(u)[~valid].any(), "a padding slot of the values is not zero bytes"
    key = keys_of(x, order)
    if got_pos is None:
        assert np.array_equal(keys_of(got_vals, order)[valid], key[want_pos[valid]]), "a slot does not hold the image of its rank"
        assert same(got_vals[valid], want_vals[valid], flags[valid]), "a value differs from the model's"
        return
    got_pos = np.asarray(got_pos)
    assert got_pos.dtype == np.uint32 and got_pos.shape == (G, k), ("shape / dtype of the positions", got_pos.dtype, got_pos.shape)
    assert np.all(got_pos[~valid] == MISSING), "a padding slot of the positions is not 0xFFFFFFFF"
    if not valid.any():
        return
    p = got_pos.astype(np.int64)
    lo, hi = offsets[:-1, None], offsets[1:, None]
    assert np.all(((p >= lo) & (p < hi))[valid]), "a position lies outside its group"
    pc = np.where(valid, p, 0)
    assert np.array_equal(got_vals.view(u)[valid], x.view(u)[pc][valid]), "a value is not bitwise the element at its position"
    kk = key[pc]
    assert np.array_equal(kk[valid], key[want_pos[valid]]), "a slot does not hold the image of its rank (a wanted row was dropped)"
    # (image, position) strictly ascending along the slots of a group: ordered, ties by ascending position, no position twice
    nxt = valid[:, 1:]
    a, b, pa, pb = kk[:, :-1], kk[:, 1:], pc[:, :-1], pc[:, 1:]
    assert np.all(((a < b) | ((a == b) & (pa < pb)))[nxt]), "slots out of order: equal images with descending or repeated positions"
