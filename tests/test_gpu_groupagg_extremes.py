"""The group-by aggregates at the numeric extremes, plan by plan: aqg_groupby_agg through every plan of DESIGN.md section 4.1,
aqg_grouped_reduce on a build handle through its three routes, aqg_grouped_reduce_flat and aqg_grouped_corr -- full-range integers of
every type, 8-byte sums that carry and borrow in every group, `avg` on, below and above a rounding tie of the 128-bit sum, 4-byte
columns at the ends of their type (the packed value fields and their late-row escape), floating columns of every exponent with
+-Inf groups, all-Inf and all-negative groups (the seeds of min and max) and NaN groups.

One test per plan (the two slowest cut by value type); each makes several calls, every call reads the plan back, asserts it and prints it.  The inputs, the group
shapes (one group of a third of the rows, 60 one-row groups, random ones) and the `check` routine with its derived bounds are
tests/groupagg_cases.py; what the oracle is worth at these inputs is tests/test_groupagg_model.py.  Plans behind a switch run in a
child process (test_gpu_plans.run_forced: the switches are read once per process).

Left out by design, per plan (the tables of groupagg_cases.PLANS carry the reasons next to the shapes): more than four accumulators
for the fast, multi-pass LDS and wide-tuple shapes; the ops that need group sizes where 3000 groups leave the LDS
budget one accumulator; a group of a third of the rows for the wide-tuple plan (its partitions are sized by rows); NaN sets where
every row is its own group or a shape has fewer than 20 groups (one NaN group would be more than the 10 % the recipe allows)."""
import pytest

import groupagg_cases as gc
from test_gpu_plans import run_forced

pytestmark = pytest.mark.gpu

CHILD = "import groupagg_cases as gc\ngc.%s\nprint('OK', flush=True)\n"


@pytest.fixture(scope="module")
def gpu():
    import aquery2_amd
    d = aquery2_amd.Device(0)
    yield d
    d.close()


def forced(name):
    run_forced(gc.PLAN_ENV[name], CHILD % f"run_plan(gpu, oracle, {name!r})")


# ---- aqg_groupby_agg: 200 003 rows ---------------------------------------------------------------------------------------------------
def test_few_lds_plan(gpu, oracle):
    """the LDS-DMA row stream (groupby_few.hip): one aligned int32 key, one to four accumulators over int32 / uint32 / float32"""
    gc.run_plan(gpu, oracle, "few_lds")


def test_fast_lds_plan_wide_and_tiny_values(gpu, oracle):
    """agg32_kernel's VW = 8 instantiation: 1-, 2- and 8-byte value columns under one int32, two int32 and one int64 key"""
    gc.run_plan(gpu, oracle, "fast_v8")


def test_small_lds_plan_through_the_hashed_row_pass(gpu, oracle):
    gc.run_plan(gpu, oracle, "small_lds")


def test_hbm_table_plan(gpu, oracle):
    gc.run_plan(gpu, oracle, "hbm_table")


# ---- aqg_groupby_agg: just above 2^20 rows ---------------------------------------------------------------------------------------------
def test_dense_plan(gpu, oracle):
    gc.run_plan(gpu, oracle, "dense")


def test_big_lds_plan(gpu, oracle):
    gc.run_plan(gpu, oracle, "big_lds")


def test_one_level_partition_plan_hashed(gpu, oracle):
    """key * 5003 and an 8-byte key word: the default (cursor) scatter"""
    gc.run_plan(gpu, oracle, "part_one")


def test_one_level_partition_plan_hashed_chunk_histogram_scatter():
    forced("part_one_cursors_off")


def test_one_level_partition_plan_over_range_partitions(gpu, oracle):
    """a dense key domain at >= 2^22 rows (range partitions are planned from there on): the direct-indexed aggregation"""
    gc.run_plan(gpu, oracle, "part_one_ranged")


def test_one_level_partition_plan_over_range_partitions_chunk_histogram_scatter():
    forced("part_one_ranged_cursors_off")


def test_two_level_partition_plan():
    forced("part_two")


def test_round1_partition_pipeline():
    forced("part_round1")


def test_ordering_tail():
    forced("sorted_tail")


def test_row_emit_plan(gpu, oracle):
    gc.run_row_emit(gpu, oracle)


@pytest.mark.parametrize("values", ["int4", "int8", "fp"])
def test_wide_tuple_partition_plan(gpu, oracle, values):
    gc.run_plan(gpu, oracle, "part_wide_" + values)


# ---- aqg_groupby_agg: the packed value fields (>= 2^22 rows) ---------------------------------------------------------------------------
def test_packed_value_fields_at_the_ends_of_the_type_and_their_late_rows():
    run_forced(gc.PLAN_ENV["packed_values"], CHILD % "run_packed_values(gpu, oracle)")


# ---- aqg_grouped_reduce on a build handle, the flat form, corr -------------------------------------------------------------------------
@pytest.mark.parametrize("n,G", [(gc.N_SMALL, 1000), (gc.N_MID, 300_000)])
def test_grouped_reduce(gpu, oracle, n, G):
    gc.run_grouped_reduce(gpu, oracle, n, G)


@pytest.mark.parametrize("values", ["int", "fp"])
def test_grouped_reduce_partitioned_on_the_group_id(gpu, oracle, values):
    gc.run_gid_partition(gpu, oracle, values)


@pytest.mark.parametrize("n,G", [(4097, 5), (120_001, 1000)])
def test_grouped_reduce_flat(gpu, oracle, n, G):
    gc.run_reduce_flat(gpu, oracle, n, G)


@pytest.mark.parametrize("n,G", [(50, 4), (100_003, 100)])
def test_grouped_corr(gpu, oracle, n, G):
    gc.run_corr(gpu, oracle, n, G)
