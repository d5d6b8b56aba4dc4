"""The numpy model of aqg_quantiles / aqg_grouped_quantiles (include/aqg.h, quantiles section), built on tests/median_model.py: the rows
of every group in ascending order of their key IMAGE, and for quantile j of a group of c rows the element of rank
floor(num[j] (c - 1) / den) (lower) or ceil(num[j] (c - 1) / den) (upper).  The ranks come from Python integers, which are exact."""
import numpy as np

from median_model import SEL_LOWER, SEL_UPPER, first_occurrence_ids, image, same  # noqa: F401  (re-exported for the tests)


def rank(num, den, c, which):
    """the rank of quantile num / den among c >= 1 rows, in Python integers"""
    assert c >= 1 and den >= 1 and 0 <= num <= den and which in (SEL_LOWER, SEL_UPPER)
    p = int(num) * (int(c) - 1)
    return p // int(den) if which == SEL_LOWER else -((-p) // int(den))


class Sorted:
    """one sort of a grouped column, asked for any number of quantile lists: x[i] belongs to group gid[i] (dense ids below ngroups, every
    group non-empty)"""

    def __init__(self, x, gid, ngroups):
        x = np.asarray(x)
        self.x = x.astype(np.uint8) if x.dtype == np.bool_ else x
        self.G = ngroups
        gid = np.asarray(gid, dtype=np.int64)
        self.counts = np.bincount(gid, minlength=ngroups) if ngroups else np.zeros(0, np.int64)
        assert ngroups == 0 or self.counts.min() >= 1, "every group holds a row"
        self.order = np.lexsort((image(self.x), gid)) if ngroups > 1 else np.argsort(image(self.x), kind="stable")
        self.starts = np.concatenate([[0], np.cumsum(self.counts)[:-1]]).astype(np.int64) if ngroups else np.zeros(0, np.int64)
        self.both = None
        if self.x.dtype.kind == "f" and ngroups:
            bits = self.x.view(np.uint32 if self.x.itemsize == 4 else np.uint64)
            neg_zero, pos_zero = (self.x == 0) & (bits != 0), (self.x == 0) & (bits == 0)
            self.both = (np.bincount(gid, weights=neg_zero, minlength=ngroups) > 0) & (np.bincount(gid, weights=pos_zero, minlength=ngroups) > 0)

    def ranks(self, nums, den, which, rank_fn=rank):
        """[G][nq] ranks; rank_fn is asked once per distinct group size"""
        uc, inv = np.unique(self.counts, return_inverse=True)
        table = np.array([[rank_fn(num, den, int(c), which) for num in nums] for c in uc], dtype=np.int64).reshape(len(uc), len(nums))
        return table[inv.reshape(-1)]

    def quantiles(self, nums, den, which=SEL_LOWER, rank_fn=rank):
        """(out[G][nq], flags[G][nq]); flags: the slot is compared by value, not by bits -- the rank lands on a zero of a group that holds
        both zeros, or on a NaN (the median's rule)"""
        nq = len(nums)
        if self.G == 0:
            return self.x[:0].reshape(0, nq).copy(), np.zeros((0, nq), dtype=bool)
        r = self.ranks(nums, den, which, rank_fn)
        out = self.x[self.order[self.starts[:, None] + r]]
        flags = np.zeros(out.shape, dtype=bool) if self.both is None else np.isnan(out) | ((out == 0) & self.both[:, None])
        return out, flags


def grouped(x, gid, ngroups, nums, den, which=SEL_LOWER):
    return Sorted(x, gid, ngroups).quantiles(nums, den, which)


def flat(x, nums, den, which=SEL_LOWER):
    """(out[nq], flags[nq]) of the whole column; an empty column gives zeros"""
    x = np.asarray(x)
    if len(x) == 0:
        return np.zeros(len(nums), dtype=np.uint8 if x.dtype == np.bool_ else x.dtype), np.zeros(len(nums), dtype=bool)
    out, flags = grouped(x, np.zeros(len(x), dtype=np.int64), 1, nums, den, which)
    return out[0], flags[0]
