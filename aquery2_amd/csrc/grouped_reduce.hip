// grouped_reduce.hip -- aqg_grouped_reduce / aqg_grouped_corr: accumulators indexed by the dense group ids of a build (grouping by
// the reversemap column through the group-by plans of groupby.hip).
#include "groupby_plan.hpp"

namespace {
// Grouping by a column of the dense group ids of `g` (0 .. G - 1): its key spec with the exact range, and g's scratch handle for the result
int dense_id_keys(aqg_ctx* ctx, aqg_groupby* g, const uint32_t* gid_col, KeySpec* ks, aqg_groupby** h) {
    const int kdt = AQG_UINT32;
    const void* kcol = gid_col;
    AQG_TRY(aqg_make_keyspec(ctx, 1, &kdt, &kcol, g->n, ks));
    ks->range_known = 1; ks->range_lo = 0; ks->range_hi = (long long)g->ngroups - 1;
    if (!g->scratch) g->scratch = new aqg_groupby();
    *h = g->scratch;
    (*h)->ctx = ctx; (*h)->n = g->n; (*h)->has_reversemap = false;
    return AQG_OK;
}
} // namespace

extern "C" {

namespace {
// corr(x, y) of every group from its five sums (server/aggregations.h:401-406): all of them __int128 in the reference (InnerType there is
// the Coercion STRUCT, so GetLongType<InnerType> is __int128 whatever the inputs are), len * s wraps in 128 bits, FPType = double
__global__ void __launch_bounds__(256) corr_final_kernel(const aqg_i128* __restrict__ sx, const aqg_i128* __restrict__ sx2, const aqg_i128* __restrict__ sy,
                                                        const aqg_i128* __restrict__ sy2, const aqg_i128* __restrict__ sxy, const uint32_t* __restrict__ counts,
                                                        uint32_t G, double* __restrict__ out) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
        const aqg_i128 len = i128_from_u64(counts[g]);
        const double a = i128_to_double(i128_mul(len, sxy[g])) - i128_to_double(i128_mul(sx[g], sy[g]));
        const double b = i128_to_double(i128_mul(len, sx2[g])) - i128_to_double(i128_mul(sx[g], sx[g]));
        const double c = i128_to_double(i128_mul(len, sy2[g])) - i128_to_double(i128_mul(sy[g], sy[g]));
        out[g] = a / sqrt(b * c);
    }
}
__global__ void __launch_bounds__(256) take_rows_kernel(const uint64_t* __restrict__ acc_rows, uint32_t G, uint32_t* __restrict__ rows) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) rows[g] = (uint32_t)acc_rows[g];
}
} // namespace

// the core of aqg_grouped_reduce: groups by a column of dense group ids (the build's reversemap, or the group index of every position
// of the flat layout -- segscan.hip) through the ordinary group-by plans; ids appear in first-occurrence order, so group g is result g
int aqg_grouped_reduce_keyed(aqg_ctx* ctx, aqg_groupby* g, const uint32_t* gid_col, int op, int t, const void* x, void* out_dev) {
    const uint32_t G = g->ngroups, n = g->n;
    // beyond the LDS tables: the build's ids are dense and its group sizes known -- partitioned on the id, direct-indexed (partition_wide.hip)
    constexpr uint32_t GID_MIN = 1u << 16;       // (measured again in round 3, with the value inside the id word: 6.5 against 7.5 ms at 1e5 groups, equal for values that do not pack)
    if (gid_col == g->reversemap && g->has_counts && G > GID_MIN && n >= (1u << 22)) {       // (up to ~3e6 groups the one-level hashed plan is as fast: 8.0-8.4 ms against 9.0 per 1e9 rows; 1e7 groups: 17 against 9)
        const uint32_t* off = aqg_groupby_offsets(g);
        if (off) {
            const int rc = aqg_gid_reduce(ctx, gid_col, off, g->counts, n, G, op, t, x, out_dev);
            if (rc != AQG_ERR_DTYPE) { if (rc == AQG_OK) g->plan_bits = AQG_PLAN_GID_PARTITION; return rc; }
        }
    }
    KeySpec ks;
    aqg_groupby* h = nullptr;
    AQG_TRY(dense_id_keys(ctx, g, gid_col, &ks, &h));
    Plan plan;
    AQG_TRY(aqg_make_plan(ctx, 1, &op, &t, &x, n, &plan));
    AQG_TRY(aqg_run_with_retry(ctx, ks, plan, n, G, false, h, nullptr, nullptr));
    if (h->ngroups != G) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_reduce: group ids are not dense");
    g->plan_bits = h->plan_bits;
    AQG_HIP(ctx, hipMemcpyAsync(out_dev, h->results[0], (size_t)G * aqg_dtype_size(aqg_reduce_out_dtype(op, t)), hipMemcpyDeviceToDevice, ctx->stream));
    return AQG_OK;
}

// out[g] = op(col[vecs[g]]) for every group in one pass (generated loop engine/ast.py:722-789).
// The group id column (reversemap) is itself a dense first-occurrence key, so grouping by it
// reproduces the group order; the value column is read once.  vecs[g] is in DESCENDING row order
// (hasher.h:192-196), hence first(col[vecs[g]]) is the LAST row of the group and last(...) its first row.
int aqg_grouped_reduce(aqg_ctx* ctx, const aqg_groupby* gc, int op, int t, const void* x, void* out_dev) {
    aqg_groupby* g = const_cast<aqg_groupby*>(gc);
    if (!ctx || !g || (!x && g->n) || !out_dev) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_reduce: bad argument");
    if (!g->has_reversemap) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_reduce: handle has no reversemap (use aqg_groupby_build)");
    if (!dt_is_num(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_grouped_reduce: value dtype");
    const uint32_t G = g->ngroups, n = g->n;
    if (G == 0) return AQG_OK;
    if (op == AQG_RED_LAST) return aqg_gather(ctx, t, x, g->first_rows, G, out_dev);
    KeySpec ks;
    aqg_groupby* h = nullptr;
    AQG_TRY(dense_id_keys(ctx, g, g->reversemap, &ks, &h));
    if (op == AQG_RED_FIRST) {
        Plan plan;
        memset(&plan, 0, sizeof plan);
        plan.nagg = 1;
        plan.agg[0].op = AQG_RED_MAX; plan.agg[0].dt = AQG_UINT64; plan.agg[0].acc1 = plan.agg[0].acc2 = plan.agg[0].acc3 = -1;
        plan.agg[0].acc0 = aqg_add_acc(&plan, ACC_MAX, AQG_NONE, nullptr, 0);
        AQG_TRY(aqg_run_with_retry(ctx, ks, plan, n, G, false, h, nullptr, nullptr));
        uint32_t* rows = nullptr;
        AQG_TRY(aqg_ws_reset(ctx));
        AQG_TRY(aqg_ws_get(ctx, G, &rows));
        hipLaunchKernelGGL(take_rows_kernel, dim3(aqg_grid(ctx, G, 256, 1, 8)), dim3(256), 0, ctx->stream, (const uint64_t*)h->results[0], G, rows);
        return aqg_gather(ctx, t, x, rows, G, out_dev);
    }
    return aqg_grouped_reduce_keyed(ctx, g, g->reversemap, op, t, x, out_dev);
}

// out[g] = corr(x[vecs[g]], y[vecs[g]]) for every group (h2o Q9 `pow(corr(v1, v2), 2) BY id2, id4`, benchmark/h2o/groupby.sql:20; the generated
// loop engine/ast.py:749-784 emits `corr(v1[val], v2[val])`): the product column x * y (evaluated in the C++ type of the operands like the
// reference's `x[i] * y[i]`, aggregations.h:397), then ONE grouped pass with five accumulators -- sum x, sum x*x, sum y, sum y*y, sum xy --
// and the reference's formula per group.  Integer columns of up to four bytes (every sum then fits a 64-bit accumulator exactly).
int aqg_grouped_corr(aqg_ctx* ctx, aqg_groupby* g, int tx, const void* x, int ty, const void* y, double* out_dev) {
    if (!ctx || !g || ((!x || !y) && g->n) || !out_dev) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_corr: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_corr: handle has no reversemap (use aqg_groupby_build)");
    auto small_int = [](int dt) { return dt == AQG_INT8 || dt == AQG_INT16 || dt == AQG_INT32 || dt == AQG_UINT8 || dt == AQG_UINT16 || dt == AQG_UINT32; };
    if (!small_int(tx) || !small_int(ty)) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_grouped_corr: integer columns of up to four bytes (others: aqg_corr per group)");
    const uint32_t G = g->ngroups, n = g->n;
    if (G == 0) return AQG_OK;
    const int pt = (tx == AQG_UINT32 || ty == AQG_UINT32) ? AQG_UINT32 : AQG_INT32;      // usual arithmetic conversions of the two operands
    size_t cap = 0;
    void* xy = aqg_pool_alloc(ctx, (size_t)n * 4 + 64, &cap);
    if (!xy) return aqg_fail(ctx, AQG_ERR_NOMEM, "aqg_grouped_corr: product column");
    int rc = aqg_ewise(ctx, AQG_OP_MUL, AQG_VEC_VEC, tx, x, ty, y, pt, xy, n);
    if (rc == AQG_OK) {
        KeySpec ks;
        aqg_groupby* h = nullptr;
        rc = dense_id_keys(ctx, g, g->reversemap, &ks, &h);
        // up to 3072 groups: two passes through the fast LDS plan (at most four accumulators each) -- {sum x, sum x*x, sum y, sum y*y} over
        // the two columns, then {sum xy} over the product column.  Beyond (h2o Q9: 1e4 groups): five single-accumulator passes -- four
        // accumulators per slot push a 1e4-slot table out of LDS (dense plan, three passes over the rows: 19.5 ms per 1e9 rows) while one
        // accumulator streams at 1.45 ms per pass
        size_t sums_cap = 0;
        void* sums = aqg_pool_alloc(ctx, (size_t)G * 80 + 64, &sums_cap);                      // [5][G] 128-bit sums, copied out of the scratch handle pass by pass
        if (!sums) rc = aqg_fail(ctx, AQG_ERR_NOMEM, "aqg_grouped_corr: sums");
        const int ops5[5] = {AQG_RED_SUM, AQG_RED_SUMSQ, AQG_RED_SUM, AQG_RED_SUMSQ, AQG_RED_SUM};
        const int dts5[5] = {tx, tx, ty, ty, pt};
        const void* vals5[5] = {x, x, y, y, xy};
        auto slot = [&](int j) { return static_cast<char*>(sums) + (size_t)j * G * 16; };
        auto pass = [&](int first, int count) -> int {
            Plan plan;
            AQG_TRY(aqg_make_plan(ctx, count, ops5 + first, dts5 + first, vals5 + first, n, &plan));
            AQG_TRY(aqg_run_with_retry(ctx, ks, plan, n, G, false, h, nullptr, nullptr));
            if (h->ngroups != G) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_corr: group ids are not dense");
            for (int j = 0; j < count; ++j) AQG_HIP(ctx, hipMemcpyAsync(slot(first + j), h->results[j], (size_t)G * 16, hipMemcpyDeviceToDevice, ctx->stream));
            return AQG_OK;
        };
        if (rc == AQG_OK) {
            if (G <= 3072) { rc = pass(0, 4); if (rc == AQG_OK) rc = pass(4, 1); }
            else for (int j = 0; j < 5 && rc == AQG_OK; ++j) rc = pass(j, 1);
        }
        if (rc == AQG_OK) {
            hipLaunchKernelGGL(corr_final_kernel, dim3(aqg_grid(ctx, G, 256, 1, 8)), dim3(256), 0, ctx->stream, (const aqg_i128*)slot(0), (const aqg_i128*)slot(1),
                               (const aqg_i128*)slot(2), (const aqg_i128*)slot(3), (const aqg_i128*)slot(4), g->counts, G, out_dev);
            rc = aqg_check_launch(ctx, "corr_final_kernel");
        }
        if (sums) aqg_pool_give(ctx, sums, sums_cap);
    }
    aqg_pool_give(ctx, xy, cap);           // (stream-ordered reuse: every later user of the buffer runs on this stream)
    return rc;
}

} // extern "C"
