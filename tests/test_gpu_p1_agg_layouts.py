"""The three LDS layouts of the per-partition aggregation (partition1_agg.hip), each pinned by its own case: at default thresholds
every hashed partition plan below ~4000 partitions takes the slot layout, so p1_agg_kernel (dense ids) ran in no committed test.

  dense ids   AQG_P1_BINS=128 AQG_DISABLE_RANGED=1   (with AQG_P1_BINS set, aqg_partition_parts never picks the slot layout)
  slot        AQG_DISABLE_RANGED=1
  direct      no switch, over a dense key domain: range partitions

The hashed layouts: 1 200 007 rows (partition plans start at 2^20; not a multiple of the 4096-row step) in ~100 000 groups: ~780
groups and ~9400 rows per partition at 128 bins -- two full steps plus an edge step -- and partitions shorter than one step where the
slot layout takes ~570 bins (the eight-accumulator sets, by their hint).  The direct layout: 4 400 021 rows, because range partitions
are planned from 2^22 rows on (plan_pack); the low end of its key domain is thin (~8800 rows over the first 3000 keys), so that the
partitions there are short.  One hot key holds a partition's worth of rows; the hashed layouts also see the key that equals the tables'
empty mark (0x80000000, ~0), which has an entry of its own.  Accumulator sets: none (COUNT), one, eight 4-byte ones with squares through the generic arm, eight with 8-byte planes,
and the last two over an 8-byte key word.  Every case is a fresh process (the switches are read once per process) and compares plan
bits, groups, first rows, keys and every result with the oracle, as test_gpu_plans.py does."""
import pytest

from test_gpu_plans import run_forced

pytestmark = pytest.mark.gpu

DATA = r'''
HASHED = %s
n, G = 1_200_007 if HASHED else 4_400_021, 100_000     # (range partitions are planned from 2^22 rows on)
if HASHED:
    key = rng.integers(0, G, n).astype(np.int32)
else:                                                          # a dense domain whose low end is thin: ~8800 rows over the first 3000 keys
    key = np.where(rng.random(n) < 0.002, rng.integers(0, 3000, n), rng.integers(3000, G, n)).astype(np.int32)
key[rng.choice(n, 9_400, replace=False)] = 77                  # one partition-sized hot key
special = np.arange(3, n, 4001)
if HASHED: key[special] = np.int32(-2**31)                     # the 4-byte empty mark
key8 = (key.astype(np.int64) << 33) | 5
key8[special] = -1                                             # the 8-byte empty mark
v1, v2 = rng.integers(-9, 10, n).astype(np.int32), rng.integers(-3, 12, n).astype(np.int32)
ub, us = rng.integers(2**31 - 1000, 2**31 + 1000, n).astype(np.uint32), rng.integers(0, 1000, n).astype(np.uint32)
v3 = np.round(rng.uniform(0, 100, n), 3).astype(np.float32)
v4, v5 = rng.integers(-2**40, 2**40, n).astype(np.int64), np.round(rng.uniform(0, 1000, n), 6)
class Ranged:                                                  # one level, range partitions; narrow value columns may travel inside the key word
    def __eq__(self, plan): return plan & ~capi.PLAN_PACKED_VALUES == capi.PLAN_PART_ONE | capi.PLAN_RANGE_PARTITIONS
PLAN = capi.PLAN_PART_ONE if HASHED else Ranged()
# (an accumulator is shared between aggregates only over the same device column, and every value argument is uploaded on its own: count each aggregate's in full)
FOUR = ([ck.RED_SUM, ck.RED_MIN, ck.RED_MAX, ck.RED_AVG, ck.RED_VAR, ck.RED_VAR], [v2, ub, v3, v3, us, v1])                       # 8 accumulators, 4-byte planes: 1 + 1 + 1 + 1 + 2 + 2; add, min, max over int32 / uint32 / float32, two squares
EIGHT =([ck.RED_SUM, ck.RED_SUM, ck.RED_AVG, ck.RED_MIN, ck.RED_MAX, ck.RED_VAR], [v4, v5, v3, ub, v1, v2])                      # 8 accumulators, 8-byte planes: both halves of an int64 sum, a float64 sum, a square
'''

SETS = {
    "count": "check([key], [ck.RED_COUNT], [v1], 120_000, PLAN)",
    "one_sum": "check([key], [ck.RED_SUM], [v1], 120_000, PLAN)",
    "eight_of_4_bytes": "check([key], *FOUR, 600_000, PLAN)",
    "eight_with_8_byte_planes": "check([key], *EIGHT, 600_000, PLAN)",
    "key64_eight_of_4_bytes": "check([key8], *FOUR, 600_000, PLAN)",
    "key64_eight_with_8_byte_planes": "check([key8], *EIGHT, 600_000, PLAN)",
}
LAYOUTS = {
    "dense_ids": ({"AQG_P1_BINS": "128", "AQG_DISABLE_RANGED": "1"}, True),
    "slot": ({"AQG_DISABLE_RANGED": "1"}, True),
    "direct": ({}, False),
}
CASES = [(layout, name) for layout in LAYOUTS for name in SETS if not (layout == "direct" and name.startswith("key64"))]


@pytest.mark.parametrize("layout,accs", CASES)
def test_partition_aggregation_layout(layout, accs):
    env, hashed = LAYOUTS[layout]
    run_forced(env, DATA % hashed + SETS[accs] + "\n")
