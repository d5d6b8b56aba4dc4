"""The numpy model of aqg_count_distinct / aqg_grouped_count_distinct (include/aqg.h, count distinct section).

The distinct count of a slice is the size of the reference's std::unordered_set<T> over it (server/vector_type.hpp:153-174,
server/table.h:328-332): equality by C++ ==.  Integers and bool by value; floating values: -0.0 and +0.0 are one value, and a NaN
equals nothing, itself included, so every NaN ROW is a value of its own.  Hence: the distinct key images (median_model.image) of
the rows that are not NaN, plus the number of NaN rows.  tests/golden/ref_distinct.json holds what the reference's headers answer."""
import numpy as np

from median_model import first_occurrence_ids, image  # noqa: F401  (first_occurrence_ids: the group ids of aqg_groupby_build)


def grouped(x, gid, ngroups):
    """np.uint32 per group: x[i] belongs to group gid[i] (dense ids below ngroups)"""
    x = np.asarray(x)
    gid = np.asarray(gid, dtype=np.int64)
    out = np.zeros(ngroups, dtype=np.int64)
    if len(x) == 0:
        return out.astype(np.uint32)
    nan = np.isnan(x) if x.dtype.kind == "f" else np.zeros(len(x), dtype=bool)
    out += np.bincount(gid[nan], minlength=ngroups)
    im, g = image(x)[~nan], gid[~nan]
    if len(im):
        order = np.lexsort((im, g))
        im, g = im[order], g[order]
        new = np.ones(len(im), dtype=bool)
        new[1:] = (im[1:] != im[:-1]) | (g[1:] != g[:-1])
        out += np.bincount(g[new], minlength=ngroups)
    return out.astype(np.uint32)


def flat(x):
    """the distinct count of the whole column (0 for an empty one)"""
    x = np.asarray(x)
    return int(grouped(x, np.zeros(len(x), dtype=np.int64), 1)[0])
