"""The few-group row pass that streams its rows through LDS by DMA (groupby_few.hip): one 4-byte key column, one to four
accumulators over 4-byte value columns, a table that fits LDS.  Every output is compared with the oracle through groupby_agg, at
hint 128 (where the plan read back must be the fast LDS plan) and at hint 0.  Sizes cover the edges of a workgroup's span, of a
ring stage (512 rows) and the rows after the last whole stage; keys cover the LDS empty mark, negative keys, keys that are all
multiples of 1024, more keys than the LDS table holds, and a group first seen in the last rows."""
import numpy as np
import pytest

import aquery2_amd
import checker as ck
import golden_util as gu
from aquery2_amd import capi

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


@pytest.fixture(scope="module")
def gpu():
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def check(gpu, oracle, keys, ops, vals, hint, fast=True, handle=None):
    o = oracle.groupby([keys])
    gb = gpu.groupby_agg([keys], ops, vals, hint=hint, handle=handle)
    if fast:
        assert gb.plan & capi.PLAN_FAST_LDS, ("plan", hex(gb.plan))
    assert gb.ngroups == o["ngroups"], (gb.ngroups, o["ngroups"])
    assert np.array_equal(gb.first_rows(), o["first_rows"])
    assert np.array_equal(gb.keys(0, keys.dtype), keys[o["first_rows"]])
    for j, (op, v) in enumerate(zip(ops, vals)):
        got, want = gb.result(j, op, ck.tag_of(v)), oracle.grouped_reduce(op, v, o)
        if v.dtype.kind == "f" and op in (ck.RED_SUM, ck.RED_AVG):
            assert np.allclose(got, want, rtol=1e-12, atol=1e-9), j
        else:
            assert gu.same_bits(got, want), j
    return gb


def id1(rng, n, groups=100):
    return rng.integers(1, groups + 1, n).astype(np.int32)


@pytest.mark.parametrize("n", [(1 << 16) + d for d in range(8)] + [5_000_003, 30_000_000])
def test_sizes(gpu, oracle, n):
    rng = np.random.default_rng(n)
    k, v = id1(rng, n), rng.integers(1, 6, n).astype(np.int32)
    check(gpu, oracle, k, [ck.RED_SUM], [v], 128)
    check(gpu, oracle, k, [ck.RED_SUM], [v], 0, fast=False)


@pytest.mark.parametrize("kind", ["one", "empty_mark", "negative", "x1024", "3000", "10000", "late"])
def test_keys(gpu, oracle, kind):
    rng = np.random.default_rng(7)
    n = 1_000_003
    v = rng.integers(-100, 100, n).astype(np.int32)
    fast = True
    if kind == "one":
        k = np.full(n, 42, np.int32)
    elif kind == "empty_mark":            # INT32_MIN is the LDS table's empty mark: it has a slot of its own
        k = np.where(rng.random(n) < 0.3, INT32_MIN, id1(rng, n)).astype(np.int32)
    elif kind == "negative":
        k = -id1(rng, n)
    elif kind == "x1024":
        k = id1(rng, n) * 1024
    elif kind == "3000":                  # more keys than the LDS table at hint 128 holds: the overflow goes to the group table
        k, fast = id1(rng, n, 3000), False
    elif kind == "10000":                 # ... and past the table the hint sized: the call is planned again
        k, fast = id1(rng, n, 10_000), False
    else:                                 # a group first seen in the very last rows
        k = id1(rng, n, 50)
        k[-3:] = 77
    check(gpu, oracle, k, [ck.RED_SUM, ck.RED_COUNT], [v, v], 128, fast=fast)
    check(gpu, oracle, k, [ck.RED_SUM], [v], 0, fast=False)


def test_extreme_values(gpu, oracle):
    """INT32_MIN / INT32_MAX on every row: the sums need the 128-bit result slots"""
    n = (1 << 16) + 5
    rng = np.random.default_rng(3)
    k = id1(rng, n, 3)
    for x in (INT32_MIN, INT32_MAX):
        check(gpu, oracle, k, [ck.RED_SUM, ck.RED_MIN, ck.RED_MAX], [np.full(n, x, np.int32)] * 3, 128)
    u = np.full(n, 0xFFFFFFFF, np.uint32)
    check(gpu, oracle, k, [ck.RED_SUM, ck.RED_MAX], [u, u], 128)


def test_value_types_four_accumulators(gpu, oracle):
    rng = np.random.default_rng(11)
    n = 5_000_003
    k = id1(rng, n)
    vi = rng.integers(-1000, 1000, n).astype(np.int32)
    vu = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    vf = np.round(rng.uniform(-100, 100, n), 3).astype(np.float32)
    check(gpu, oracle, k, [ck.RED_SUM, ck.RED_SUM, ck.RED_SUM], [vi, vu, vf], 128)
    check(gpu, oracle, k, [ck.RED_COUNT, ck.RED_MIN, ck.RED_MAX, ck.RED_AVG], [vi, vu, vf, vi], 128)
    check(gpu, oracle, k, [ck.RED_MIN, ck.RED_MAX, ck.RED_AVG, ck.RED_SUM], [vf, vf, vf, vu], 128)
    check(gpu, oracle, k, [ck.RED_COUNT, ck.RED_MIN, ck.RED_MAX, ck.RED_AVG], [vi, vu, vf, vi], 0, fast=False)


def test_unaligned_column(gpu, oracle):
    """a value column that is not 16-byte aligned takes the generic plans"""
    rng = np.random.default_rng(5)
    n = 1_000_003
    k, v = id1(rng, n), rng.integers(1, 6, n).astype(np.int32)
    base = gpu.to_device(np.concatenate([np.zeros(1, np.int32), v]))
    vv = aquery2_amd.DevBuf(gpu, base.ptr + 4, np.int32, n, owned=False)
    vv._base = base
    o = oracle.groupby([k])
    gb = gpu.groupby_agg([k], [ck.RED_SUM], [vv], hint=128)
    assert gb.ngroups == o["ngroups"]
    assert np.array_equal(gb.first_rows(), o["first_rows"])
    assert gu.same_bits(gb.result(0, ck.RED_SUM, ck.INT32), oracle.grouped_reduce(ck.RED_SUM, v, o))


def test_handles_reused(gpu, oracle):
    """three calls on one handle, two handles interleaved, a call of another shape in between"""
    rng = np.random.default_rng(9)
    n1, n2 = 2_000_003, (1 << 16) + 3
    k1, v1 = id1(rng, n1), rng.integers(1, 6, n1).astype(np.int32)
    k2, v2 = id1(rng, n2, 7), rng.integers(-5, 6, n2).astype(np.int32)
    h1 = check(gpu, oracle, k1, [ck.RED_SUM], [v1], 128)
    h2 = check(gpu, oracle, k2, [ck.RED_SUM, ck.RED_MAX], [v2, v2], 128)
    for _ in range(2):
        check(gpu, oracle, k1, [ck.RED_SUM], [v1], 128, handle=h1)
        check(gpu, oracle, k2, [ck.RED_SUM, ck.RED_MAX], [v2, v2], 128, handle=h2)
        check(gpu, oracle, k1.astype(np.int64), [ck.RED_SUM], [v1], 128, fast=False)
