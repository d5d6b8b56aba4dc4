"""The numpy model of aqg_window_quantiles / aqg_grouped_window_quantiles (include/aqg.h, moving quantiles section), built on
tests/median_model.py and tests/quantile_model.py: the window of row i is the last min(w, predecessors of i in its slice + 1) rows of
its slice, sorted by their key IMAGE (ties by position), and quantile j is the element of rank quantile_model.rank(num[j], den, len,
which) -- Python integers, which are exact.  A slice is the whole column, or a group of the flat layout (gid: one id per position,
equal ids adjacent).

Every knob a planted mistake turns (tests/test_winq_model.py) is a keyword of Windows / quantiles; the defaults are the contract."""
import numpy as np

from median_model import SEL_LOWER, SEL_UPPER, image, same  # noqa: F401  (re-exported for the tests)
from quantile_model import rank


def slice_starts(n, gid=None):
    """start[i] = first position of the slice of position i"""
    if gid is None:
        return np.zeros(n, np.int64)
    gid = np.asarray(gid)
    head = np.ones(n, dtype=bool)
    head[1:] = gid[1:] != gid[:-1]
    return np.maximum.accumulate(np.where(head, np.arange(n), 0)).astype(np.int64)


class Windows:
    """the sorted windows of one column under one w, asked for any number of quantile lists.
    lo[i], hi[i]: the window of row i is positions lo[i] .. hi[i] (inclusive); image_fn: the order"""

    def __init__(self, x, w, gid=None, image_fn=image, shift=0, clamp=True, tile=None):
        x = np.asarray(x)
        self.x = x.astype(np.uint8) if x.dtype == np.bool_ else x
        self.n, self.w = n, w = len(self.x), int(w)
        assert w >= 1
        i = np.arange(n, dtype=np.int64)
        start = slice_starts(n, gid) if clamp else np.zeros(n, np.int64)
        if tile is not None:                                   # (a planted mistake: every tile edge is a slice start)
            start = np.maximum(start, i // tile * tile)
        self.hi = i - shift                                    # (shift: a planted mistake; 0 is the contract)
        self.lo = np.maximum(self.hi - (w - 1), start)
        self.hi = np.maximum(self.hi, self.lo)
        self.len = self.hi - self.lo + 1
        # key[p] = rank of (image, position) in the whole column: its order within any window is the window's own
        self.order = np.argsort(image_fn(self.x), kind="stable")
        key = np.empty(n, np.int32)
        key[self.order] = i
        if n:
            pad = np.concatenate([np.full(w - 1, n, np.int32), key])
            win = np.lib.stride_tricks.sliding_window_view(pad, w)[self.hi]               # win[i, k] = key[hi[i] - (w - 1) + k]
            self.sorted = np.sort(np.where(np.arange(w)[None, :] >= (w - self.len)[:, None], win, n), axis=1)    # outside the window: last
        else:
            self.sorted = np.zeros((0, w), np.int64)
        self.both = None
        if self.x.dtype.kind == "f":
            bits = self.x.view(np.uint32 if self.x.itemsize == 4 else np.uint64)
            cn = np.concatenate([[0], np.cumsum((self.x == 0) & (bits != 0))])
            cp = np.concatenate([[0], np.cumsum((self.x == 0) & (bits == 0))])
            self.both = ((cn[self.hi + 1] - cn[self.lo]) > 0) & ((cp[self.hi + 1] - cp[self.lo]) > 0)

    def ranks(self, nums, den, which, rank_fn=rank, use_w=False):
        """[nq][n] ranks; rank_fn is asked once per distinct window length"""
        ln = np.full(self.n, self.w) if use_w else self.len
        ul, inv = np.unique(ln, return_inverse=True)
        table = np.array([[rank_fn(num, den, int(c), which) for c in ul] for num in nums], dtype=np.int64).reshape(len(nums), len(ul))
        return np.minimum(table[:, inv.reshape(-1)], self.len - 1)          # (only a planted mistake reaches the clip)

    def quantiles(self, nums, den, which=SEL_LOWER, rank_fn=rank, use_w=False):
        """(out[nq][n], flags[nq][n]); flags: the slot is compared by value, not by bits -- the rank lands on a zero of a window that holds
        both zeros, or on a NaN (the median's rule)"""
        nq = len(nums)
        if self.n == 0:
            return self.x[:0].reshape(nq, 0).copy(), np.zeros((nq, 0), dtype=bool)
        r = self.ranks(nums, den, which, rank_fn, use_w)
        out = self.x[self.order[np.take_along_axis(self.sorted, r.T, axis=1).T]]
        flags = np.zeros(out.shape, dtype=bool) if self.both is None else np.isnan(out) | ((out == 0) & self.both[None, :])
        return out, flags


def windows(x, w, nums, den, which=SEL_LOWER, gid=None):
    return Windows(x, w, gid).quantiles(nums, den, which)
