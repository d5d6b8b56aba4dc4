"""The generated group loop with an element-wise operator whose scalar operand is a per-group aggregate (`price - min(price)` under
GROUP BY is emitted as `price[val] - min(price[val])`, engine/ast.py:749-784): tests/emitted/group_scalars.cpp, in the generator's shape, through
the header layer.  The header layer recognises the scalar among the aggregates the grouping already holds and answers the operator for ALL groups
with one aqg_grouped_ewise call; a scalar made on the host from several aggregates keeps the per-group path.

Expected columns come from a numpy model: groups in first-occurrence order, a group's rows in DESCENDING row order (the row lists of
ht_postproc: `first(col[vecs[g]])` is the group's last row, scans run from the last row to the first), avg = the exact integer sum as a
double divided by the count, max seeded with the smallest positive normal of floating types (the reference's defect D8, kept).
Everything is compared bit for bit except the covariance, whose outer avg sums DOUBLES with atomic adds in no fixed order: include/aqg.h
bounds such a sum by (n_g - 1) 2^-53 sum|x| around the exactly rounded one, and the division by the count adds half an ulp."""
import math
import subprocess

import numpy as np
import pytest

import median_model as mm
from test_gpu_emitted import EM, _trade, run

pytestmark = pytest.mark.gpu


def _synthetic():
    """host_main's `synthetic` dataset: the key column a and the value column c"""
    n = 200_000
    a, c = np.empty(n, np.int32), np.empty(n, np.int32)
    x, mask = 12345, (1 << 64) - 1
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & mask
        a[i] = (x >> 33) % 1000
        c[i] = (x >> 20) % 97
    return a, c


class Model:
    def __init__(self, key, price):
        self.key, self.price = key, price
        gid, self.G = mm.first_occurrence_ids(key)
        n = key.size
        first = np.full(self.G, n, np.int64)
        np.minimum.at(first, gid, np.arange(n))
        self.keys = key[first]
        order = np.lexsort((-np.arange(n), gid))                       # group after group, descending row id inside a group
        counts = np.bincount(gid, minlength=self.G)
        ends = np.cumsum(counts)
        self.groups = [price[order[e - c:e]] for c, e in zip(counts, ends)]     # int32 slices in row-list order

    def col(self, fn, dtype):
        return np.array([fn(p) for p in self.groups], dtype=dtype)


def avg(p):
    return np.float64(int(p.astype(np.int64).sum())) / np.float64(p.size)


def i128(values):
    out = np.zeros(len(values), dtype=np.dtype([("lo", "<u8"), ("hi", "<i8")]))
    for i, v in enumerate(values):
        out[i] = ((int(v) & ((1 << 64) - 1)), int(v) >> 64)
    return out


def idiv(p, d):
    """int32 division of the element-wise kernels for non-negative operands: x / 0 is defined as 0"""
    return np.zeros_like(p) if d == 0 else p // np.int32(d)


def avgw3_last(p):
    k = min(3, p.size)
    return np.float64(int(p[-k:].astype(np.int64).sum())) / np.float64(k)


DBL_MIN, FLT_MIN = np.finfo(np.float64).tiny, np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-C", EM, "build/group_scalars.so", "build/host_main"], stdout=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def models():
    return {"trade_small": Model(*_trade(50_000, 300)), "synthetic": Model(*_synthetic())}


def calls(tmp_path, out):
    ge, fb, gc, groups = (int(t) for t in (tmp_path / f"{out}.calls").read_text().split())
    return ge, fb, gc, groups


def column(tmp_path, out, k, dtype):
    return np.fromfile(tmp_path / f"{out}.out.{k}", dtype)


@pytest.mark.parametrize("dataset", ["trade_small", "synthetic"])
def test_recognised_scalars_cost_one_call_for_all_groups(tmp_path, built, models, dataset):
    m = models[dataset]
    run("group_scalars.so", dataset, "dll_gs_demean", "dll_gs_norm", "dll_gs_flat", "dll_gs_cov", cwd=str(tmp_path))
    for out in ("gs_demean", "gs_norm", "gs_flat", "gs_cov"):
        assert np.array_equal(column(tmp_path, out, 0, np.int32), m.keys), out

    # sum(price - min(price)) [int scalar, VEC_SCALAR], max(price - avg(price)) [double scalar]
    want = i128(m.col(lambda p: int((p - p.min()).astype(np.int64).sum()), object))
    assert column(tmp_path, "gs_demean", 1, want.dtype).tobytes() == want.tobytes()
    want = m.col(lambda p: max(DBL_MIN, (p.astype(np.float64) - avg(p)).max()), np.float64)
    assert column(tmp_path, "gs_demean", 2, np.float64).tobytes() == want.tobytes()

    # max(price / first(price)): int / int divides in int and converts to the generator's result type, float; min(max(price) - price)
    want = m.col(lambda p: max(FLT_MIN, idiv(p, p[0]).astype(np.float32).max()), np.float32)
    assert column(tmp_path, "gs_norm", 1, np.float32).tobytes() == want.tobytes()
    want = m.col(lambda p: (p.max() - p).min(), np.int32)
    assert column(tmp_path, "gs_norm", 2, np.int32).tobytes() == want.tobytes()

    # the column operand is a scan result (flat layout): max(maxs(price) - min(price)), last(avgs(3, price) - avg(price))
    want = m.col(lambda p: (np.maximum.accumulate(p) - p.min()).max(), np.int32)
    assert column(tmp_path, "gs_flat", 1, np.int32).tobytes() == want.tobytes()
    want = m.col(lambda p: avgw3_last(p) - avg(p), np.float64)
    assert column(tmp_path, "gs_flat", 2, np.float64).tobytes() == want.tobytes()

    # covariance(price, price) = avg((x - avg(x)) * (y - avg(y))): the scalars travel through the function's local variables
    got = column(tmp_path, "gs_cov", 1, np.float64)
    assert got.size == m.G
    for g, p in enumerate(m.groups):
        d = p.astype(np.float64) - avg(p)
        prod = d * d
        exact = math.fsum(prod.tolist())
        bound = (p.size - 1) * 2.0 ** -53 * exact / p.size + 2.0 ** -52 * exact / p.size
        assert abs(got[g] - exact / p.size) <= bound, (g, got[g], exact / p.size, bound)

    # one aqg_grouped_ewise call per distinct (operator, column, aggregate), whatever the group count; nothing fell back
    for out, exprs in (("gs_demean", 2), ("gs_norm", 2), ("gs_flat", 2), ("gs_cov", 1)):
        ge, fb, gc, groups = calls(tmp_path, out)
        assert groups == m.G
        assert fb == 0, (out, fb)
        assert ge == exprs, (out, ge)
        assert gc <= 8, (out, gc)                                      # the aggregates: a handful of grouped calls, not one per group


@pytest.mark.parametrize("dataset", ["trade_small", "synthetic"])
def test_a_scalar_derived_on_the_host_keeps_the_per_group_path(tmp_path, built, models, dataset):
    """sum(price - (max(price) - min(price))): the scalar has no provenance, so it is recognised only where its VALUE is that of a cached
    aggregate.  The first group's constant-scalar column serves the groups whose scalar equals the first group's; at the first group j
    whose scalar differs the runtime looks among the aggregates it holds (min and max of the column here) for one with the scalars of
    groups 0 and j.
      trade_small  max - min is neither: no grouped call, every group from j on falls back -- the unchanged per-group path.
      synthetic    c % 97 has min 0 in 865 of the 1000 groups, so max - min IS max there, in groups 0 and j too: max is taken for the source
                   (one grouped call), and exactly the groups whose min is not 0 are caught by the per-group comparison and fall back.
    Either way the results are exact, and the counters are predicted from the model."""
    m = models[dataset]
    run("group_scalars.so", dataset, "dll_gs_derived", cwd=str(tmp_path))
    assert np.array_equal(column(tmp_path, "gs_derived", 0, np.int32), m.keys)
    want = i128(m.col(lambda p: int((p - (p.max() - p.min())).astype(np.int64).sum()), object))
    assert column(tmp_path, "gs_derived", 1, want.dtype).tobytes() == want.tobytes()
    ge, fb, gc, groups = calls(tmp_path, "gs_derived")
    s = m.col(lambda p: p.max() - p.min(), np.int64)
    differs = np.nonzero(s != s[0])[0]
    assert differs.size, "the dataset's groups do not all share one scalar"
    j = int(differs[0])
    source = next((a for a in (m.col(np.min, np.int64), m.col(np.max, np.int64)) if a[0] == s[0] and a[j] == s[j]), None)
    assert (source is None) == (dataset == "trade_small")
    assert groups == m.G
    if source is None:
        assert ge == 0 and fb == m.G - j
    else:
        assert ge == 1 and fb == int((s[j:] != source[j:]).sum()) > 0
