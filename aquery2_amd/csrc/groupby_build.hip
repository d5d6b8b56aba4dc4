// groupby_build.hip -- aqg_groupby_build: the group table without aggregates (run_with_retry, groupby.hip), then the dense id of every
// row (reversemap) and the group sizes.  12 B/row of HBM traffic.
#include "groupby_plan.hpp"

namespace {

// ---- second pass of aqg_groupby_build: reversemap + counts ---------------------------------------
// LDS_COUNTS: group counts in an LDS histogram.  LDS_MAP: additionally a private copy of the {key -> dense id} map in LDS
// (small group counts: every lookup becomes an LDS probe instead of an L2 round trip).
template <bool LDS_COUNTS, bool LDS_MAP>
__global__ void __launch_bounds__(256) assign_kernel(KeySpec ks, GTable gt, const uint32_t* __restrict__ slot_gid, const uint32_t* __restrict__ occ, uint32_t n,
                                                     uint32_t G, uint32_t mcap, uint32_t* __restrict__ reversemap, uint32_t* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint32_t* lc = reinterpret_cast<uint32_t*>(smem_raw);                       // [G] counts
    uint64_t* mkey = reinterpret_cast<uint64_t*>(smem_raw + (((size_t)G * 4 + 15) & ~(size_t)15));   // [mcap] keys
    uint32_t* mgid = reinterpret_cast<uint32_t*>(mkey + mcap);                  // [mcap] dense ids
    __shared__ uint32_t sentinel_gid;
    if constexpr (LDS_COUNTS) for (uint32_t g = threadIdx.x; g < G; g += blockDim.x) lc[g] = 0;
    if constexpr (LDS_MAP) {
        for (uint32_t s = threadIdx.x; s < mcap; s += blockDim.x) mkey[s] = EMPTY64;
        if (threadIdx.x == 0) sentinel_gid = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < G; i += blockDim.x) {
            const uint32_t s0 = occ[i];
            const uint32_t gid = slot_gid[s0];
            if (s0 == gt.cap) { sentinel_gid = gid; continue; }
            const uint64_t key = *gt.key_p(s0);
            uint32_t s = hash64(key) & (mcap - 1);
            while (true) {                                                       // keys are distinct: plain claim by CAS
                unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&mkey[s]), EMPTY64, key);
                if (old == EMPTY64) { mgid[s] = gid; break; }
                s = (s + 1) & (mcap - 1);
            }
        }
    }
    if constexpr (LDS_COUNTS || LDS_MAP) __syncthreads();
    const uint32_t nchunk = n >> 2;
    const bool vec_ok = ks.nkeys == 1 && ks.total_bytes == 4;
    auto one = [&](uint64_t key) -> uint32_t {
        uint32_t g = 0;
        if constexpr (LDS_MAP) {
            if (key == EMPTY64) g = sentinel_gid;
            else {
                uint32_t s = hash64(key) & (mcap - 1);
                while (mkey[s] != key) s = (s + 1) & (mcap - 1);               // every key of the column is in the map
                g = mgid[s];
            }
        } else {
            uint32_t s = ks.wide ? gt_find_wide(gt, ks, (uint32_t)key) : gt_find(gt, key);
            g = s == FAIL ? 0u : slot_gid[s];
        }
        if constexpr (LDS_COUNTS) atomicAdd(&lc[g], 1u); else atomicAdd(&counts[g], 1u);
        return g;
    };
    uint32_t c_lo, c_hi;
    wg_span(nchunk, c_lo, c_hi);
    for (uint32_t c = c_lo + threadIdx.x; c < c_hi; c += blockDim.x) {
        const size_t base = (size_t)c * 4;
        uint64_t key[4];
        if (vec_ok) {
            pack<uint32_t, 4> kv = *reinterpret_cast<const pack<uint32_t, 4>*>(static_cast<const uint32_t*>(ks.col[0]) + base);
#pragma unroll
            for (int j = 0; j < 4; ++j) key[j] = kv.v[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) key[j] = ks.wide ? (uint64_t)(base + j) : pack_key(ks, base + j);
        }
        pack<uint32_t, 4> o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[j] = one(key[j]);
        *reinterpret_cast<pack<uint32_t, 4>*>(reversemap + base) = o;
    }
    if (blockIdx.x == 0) {
        uint32_t row = (nchunk << 2) + threadIdx.x;
        if (row < n) reversemap[row] = one(ks.wide ? (uint64_t)row : pack_key(ks, row));
    }
    if constexpr (LDS_COUNTS) {
        __syncthreads();
        for (uint32_t g = threadIdx.x; g < G; g += blockDim.x) { uint32_t c = lc[g]; if (c) atomicAdd(&counts[g], c); }
    }
}

// The BUILD over a dense 4-byte key domain of up to 2^21 values (8 MB: what the L2s hold of it, the Infinity Cache the rest): the id of every
// row comes from a look-up table key -> group id filled from the group table, read in ROW order -- instead of probing the partitioned rows
// and routing {row, id} pairs back by row (2.3 + 12 ms per 1e9 rows).  1e9 random 4-byte gathers cost 6.3 ms out of a 4 MB table and 17 ms
// out of a 40 MB one (request-rate bound), hence the limit.  The domain comes from a sample: a key outside it, or one the table does not
// know, sets the flag and the call repeats through the routed form.
__global__ void __launch_bounds__(256) lookup_fill_kernel(GTable gt, const uint32_t* __restrict__ slot_gid, uint32_t kmin, uint32_t D, uint32_t* __restrict__ table, uint32_t* __restrict__ flag) {
    const uint32_t G = gt.flags[1];
    for (uint32_t s = blockIdx.x * 256 + threadIdx.x; s < G; s += gridDim.x * 256) {
        const uint32_t x = (uint32_t)*gt.key_p(s) - kmin;
        if (x < D) table[x] = slot_gid[s]; else *flag = 1u;
    }
}
__global__ void __launch_bounds__(256) lookup_assign_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t kmin, uint32_t D, const uint32_t* __restrict__ table,
                                                            uint32_t* __restrict__ reversemap, uint32_t* __restrict__ flag) {
    const uint32_t nvec = n >> 2;
    uint32_t bad = 0;
    for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < nvec; c += gridDim.x * 256) {
        const uint4 k = reinterpret_cast<const uint4*>(keys)[c];
        const uint32_t x0 = k.x - kmin, x1 = k.y - kmin, x2 = k.z - kmin, x3 = k.w - kmin;
        bad |= (x0 >= D) | (x1 >= D) | (x2 >= D) | (x3 >= D);
        uint4 g;
        g.x = table[x0 < D ? x0 : 0]; g.y = table[x1 < D ? x1 : 0]; g.z = table[x2 < D ? x2 : 0]; g.w = table[x3 < D ? x3 : 0];
        bad |= (g.x == 0xFFFFFFFFu) | (g.y == 0xFFFFFFFFu) | (g.z == 0xFFFFFFFFu) | (g.w == 0xFFFFFFFFu);
        reinterpret_cast<uint4*>(reversemap)[c] = g;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const uint32_t i = (nvec << 2) + threadIdx.x, x = keys[i] - kmin;
        const uint32_t g = table[x < D ? x : 0];
        bad |= (x >= D) | (g == 0xFFFFFFFFu);
        reversemap[i] = g;
    }
    if (bad) *flag = 1u;
}

} // namespace

// aqg_groupby_build over a partition plan: the group id of every row, through a key -> id table in row order, or from the rows still
// lying partitioned in the workspace
int aqg_assign_build_ids(aqg_ctx* ctx, const AggPlan& p, aqg_groupby* h, const AggBufs& b, uint32_t G) {
    h->build_assigned = false;
    if (!(p.for_build && p.use_part && p.n && G && (p.lookup_build || b.prows.valid))) return AQG_OK;
    size_t c = h->reversemap ? h->cap_rows * 4 : 0;
    AQG_TRY(aqg_dev_realloc(ctx, &h->reversemap, &c, ((size_t)p.n + 4) * 4));
    h->cap_rows = c / 4;
    if (p.lookup_build) {
        uint32_t* table;
        AQG_TRY(aqg_ws_get(ctx, (size_t)p.lk_D + 64, &table));
        AQG_HIP(ctx, hipMemsetAsync(table, 0xFF, (size_t)p.lk_D * 4, ctx->stream));
        hipLaunchKernelGGL(lookup_fill_kernel, dim3(aqg_grid(ctx, G, 256, 1, 8)), dim3(256), 0, ctx->stream, b.gt, (const uint32_t*)b.slot_gid, p.lk_min, p.lk_D, table, b.gt.flags + 8);
        hipLaunchKernelGGL(lookup_assign_kernel, dim3(aqg_grid(ctx, p.n / 4 + 1, 256, 1, 8)), dim3(256), 0, ctx->stream, static_cast<const uint32_t*>(p.ks.col[0]), p.n, p.lk_min, p.lk_D,
                           (const uint32_t*)table, h->reversemap, b.gt.flags + 8);
        AQG_TRY(aqg_check_launch(ctx, "lookup_assign_kernel"));
        uint32_t miss = 0;
        AQG_HIP(ctx, hipMemcpyAsync(&miss, b.gt.flags + 8, 4, hipMemcpyDeviceToHost, ctx->stream));
        AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (miss) { h->no_lookup_build = true; return AQG_ERR_RANGE_MISS; }      // a key outside the sampled domain: once more, through the routed form
        h->plan_bits |= AQG_PLAN_BUILD_PARTITIONED | AQG_PLAN_BUILD_LOOKUP;
    } else {
        AQG_TRY(aqg_partition_assign(ctx, b.prows, b.gt, b.slot_gid, h->reversemap));
        h->plan_bits |= AQG_PLAN_BUILD_PARTITIONED;
    }
    h->build_assigned = true;
    return AQG_OK;
}

extern "C" {

int aqg_groupby_build(aqg_ctx* ctx, int nkeys, const int* key_dtypes, const void* const* keys, uint32_t n,
                      uint32_t max_groups_hint, aqg_groupby** out) {
    if (!ctx || !out || !key_dtypes || !keys) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_groupby_build: bad argument");
    AQG_CHECK_ROWS(ctx, n, "aqg_groupby_build");
    Plan plan;
    memset(&plan, 0, sizeof plan);
    aqg_handle_guard hg(out);
    aqg_groupby* h = hg.h;
    h->ctx = ctx; h->n = n; h->sharded = false;
    h->flat_valid = h->flat_gid_valid = false; h->flat_short_w = 0;
    GTable gt; uint32_t* slot_gid = nullptr; uint32_t* occ_dev = nullptr;
    DenseOut dn;
    dn.used = false;
    KeySpec ks;
    int nn = 0, ndt[MAXKEYS];
    const void* ncol[MAXKEYS];
    AQG_TRY(aqg_normalize_keys(ctx, h, nkeys, key_dtypes, keys, n, &nn, ndt, ncol));
    AQG_TRY(aqg_make_keyspec(ctx, nn, ndt, ncol, n, &ks));
    AQG_TRY(aqg_run_with_retry(ctx, ks, plan, n, max_groups_hint, true, h, &gt, &slot_gid, &occ_dev, &dn));
    size_t c = h->reversemap ? h->cap_rows * 4 : 0;
    AQG_TRY(aqg_dev_realloc(ctx, &h->reversemap, &c, ((size_t)n + 4) * 4));
    h->cap_rows = c / 4;
    uint32_t G = h->ngroups;
    if (n && !h->build_assigned) {
        hipMemsetAsync(h->counts, 0, (size_t)(G ? G : 1) * 4, ctx->stream);
        unsigned grid = aqg_grid(ctx, n / 4 + 1, 256, 2, 8);
        if (dn.used) {                      // direct-indexed table: the dense id of a row is slot_gid[idx(row)]
            AQG_TRY(aqg_dense_assign(ctx, ks, dn.spec, slot_gid, n, G, h->reversemap, h->counts));
        } else if (G <= 2048 && !ks.wide) {
            const uint32_t mcap = next_pow2((uint64_t)G * 2 + 2);
            size_t lds = (((size_t)G * 4 + 15) & ~(size_t)15) + (size_t)mcap * 12 + 16;
            hipLaunchKernelGGL((assign_kernel<true, true>), dim3(grid), dim3(256), lds, ctx->stream, ks, gt, slot_gid, occ_dev, n, G, mcap, h->reversemap, h->counts);
        } else if (G <= 36000) {            // group counts in an LDS histogram (up to 144 KB) instead of 1e9 global atomics
            size_t lds = (size_t)G * 4 + 16;
            hipFuncSetAttribute(reinterpret_cast<const void*>(&assign_kernel<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (lds > 20 * 1024) { const unsigned per_cu = (unsigned)((160 * 1024) / (lds + 1024)); grid = aqg_grid(ctx, n / 4 + 1, 256, 2, per_cu ? per_cu : 1); }
            hipLaunchKernelGGL((assign_kernel<true, false>), dim3(grid), dim3(256), lds, ctx->stream, ks, gt, slot_gid, occ_dev, n, G, 0u, h->reversemap, h->counts);
        } else {
            hipLaunchKernelGGL((assign_kernel<false, false>), dim3(grid), dim3(256), 0, ctx->stream, ks, gt, slot_gid, occ_dev, n, G, 0u, h->reversemap, h->counts);
        }
        AQG_TRY(aqg_check_launch(ctx, "assign_kernel"));
    }
    h->has_counts = true; h->has_reversemap = true;
    AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return hg.hand_over();
}

} // extern "C"
