// join_tail.hip -- the second half of every hash join of this library (join_tail.hpp): the grouped build side as one guard, and the
// phase behind the probe -- one algorithm over gid[np], whatever probe filled it:
//   count   output rows of every probe row by kind (c = build rows of its group): INNER c, LEFT max(c, 1), SEMI c > 0, ANTI c == 0
//   total   their sum in 64 bits, on the host BEFORE the 32-bit offsets are trusted (duplicate keys pass 2^32 at small inputs)
//   scan    aqg_exclusive_scan_u32 of the counts: the offset of every probe row's output
//   emit    pairs by probe row, then ascending build row (from the descending row lists); SEMI / ANTI the probe row at its offset
#include "join_tail.hpp"

#include "dev_common.hpp"

namespace {

// (cnt[np] = 0: the scan's total slot)
__global__ void __launch_bounds__(256) join_count_kernel(int kind, const uint32_t* __restrict__ gid, uint32_t np, const uint32_t* __restrict__ counts, uint32_t* __restrict__ cnt) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= np; i += gridDim.x * blockDim.x) {
        uint32_t c = 0;
        if (i < np) {
            const uint32_t g = gid[i];
            switch (kind) {
            case AQG_JOIN_INNER: c = g != NONE ? counts[g] : 0u; break;
            case AQG_JOIN_LEFT: c = g != NONE ? counts[g] : 1u; break;
            case AQG_JOIN_SEMI: c = g != NONE; break;
            default: c = g == NONE; break;
            }
        }
        cnt[i] = c;
    }
}
__global__ void __launch_bounds__(256) join_total_kernel(const uint32_t* __restrict__ cnt, uint32_t np, unsigned long long* __restrict__ total) {
    unsigned long long s = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) s += cnt[i];
    s = wave_reduce(s, OpAdd{});
    if (lane_id() == 0 && s) atomicAdd(total, s);
}
__global__ void __launch_bounds__(256) join_emit_kernel(int kind, const uint32_t* __restrict__ gid, uint32_t np, const uint32_t* __restrict__ out_off,
                                                        const uint32_t* __restrict__ grp_off, const uint32_t* __restrict__ rows_desc,
                                                        uint32_t* __restrict__ probe_rows, uint32_t* __restrict__ build_rows) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) {
        const uint32_t g = gid[i], o = out_off[i];
        if (kind == AQG_JOIN_SEMI) { if (g != NONE) probe_rows[o] = i; continue; }
        if (kind == AQG_JOIN_ANTI) { if (g == NONE) probe_rows[o] = i; continue; }
        if (g == NONE) {
            if (kind == AQG_JOIN_LEFT) { probe_rows[o] = i; build_rows[o] = NONE; }
            continue;
        }
        const uint32_t b = grp_off[g], e = grp_off[g + 1];
        for (uint32_t t = 0; t < e - b; ++t) { probe_rows[o + t] = i; build_rows[o + t] = rows_desc[e - 1 - t]; }   // ascending build rows
    }
}

} // namespace

JoinBuild::~JoinBuild() {
    aqg_free(ctx, grp_off);
    aqg_free(ctx, rows_desc);
    aqg_free(ctx, dkeys);
    if (gb) aqg_groupby_destroy(gb);
}

int JoinBuild::setup(int nkeys, const int* dts, const void* const* cols, uint32_t nb, bool emit_build_rows) {
    AQG_TRY(aqg_groupby_build(ctx, nkeys, dts, cols, nb, 0, &gb));
    G = aqg_groupby_ngroups(gb);
    if (!emit_build_rows) return AQG_OK;
    AQG_TRY(aqg_malloc(ctx, ((size_t)G + 1) * 4, (void**)&grp_off));
    AQG_TRY(aqg_malloc(ctx, (size_t)nb * 4, (void**)&rows_desc));
    return aqg_groupby_postproc(gb, grp_off, rows_desc);
}

int JoinBuild::keys0() {
    AQG_TRY(aqg_malloc(ctx, (size_t)G * 8, &dkeys));
    return aqg_groupby_keys(gb, 0, dkeys);
}

// total, cnt[np + 1], the scan's block sums; 256 bytes of alignment each
size_t aqg_join_tail_ws_bytes(uint32_t np) { return 8 + ((size_t)np + 1) * 4 + (((size_t)np + 1) / 2048 + 2) * 4 + 3 * 256; }

int aqg_join_tail(aqg_ctx* ctx, int kind, const uint32_t* gid, uint32_t np, const JoinBuild& build, uint32_t* probe_rows, uint32_t* build_rows,
                  uint64_t capacity, uint64_t* m_host, const char* who) {
    unsigned long long* total = nullptr;
    uint32_t *cnt = nullptr, *bsum = nullptr;
    AQG_TRY(aqg_ws_get(ctx, 1, &total));
    AQG_TRY(aqg_ws_get(ctx, (size_t)np + 1, &cnt));
    AQG_TRY(aqg_ws_get(ctx, ((size_t)np + 1) / 2048 + 2, &bsum));
    const unsigned pg = aqg_grid(ctx, np, 256, 4, 8);
    hipLaunchKernelGGL(join_count_kernel, dim3(pg), dim3(256), 0, ctx->stream, kind, gid, np, build.counts(), cnt);
    AQG_HIP(ctx, hipMemsetAsync(total, 0, 8, ctx->stream));
    hipLaunchKernelGGL(join_total_kernel, dim3(pg), dim3(256), 0, ctx->stream, (const uint32_t*)cnt, np, total);
    AQG_TRY(aqg_check_launch(ctx, "join_total_kernel"));
    unsigned long long m64 = 0;
    AQG_TRY(aqg_d2h(ctx, &m64, total, 8));
    *m_host = m64;
    if (!probe_rows || !m64) return AQG_OK;
    // output rows are addressed by uint32 offsets like every row index of this library
    if (m64 > (unsigned long long)AQG_MAX_ROWS) return aqg_fail(ctx, AQG_ERR_OVERFLOW, (std::string(who) + ": more than AQG_MAX_ROWS output rows (*m_host holds the count)").c_str());
    if (capacity < m64) return aqg_fail(ctx, AQG_ERR_OVERFLOW, (std::string(who) + ": output capacity too small (*m_host holds the count)").c_str());
    AQG_TRY(aqg_exclusive_scan_u32(ctx, cnt, (uint64_t)np + 1, bsum));
    hipLaunchKernelGGL(join_emit_kernel, dim3(pg), dim3(256), 0, ctx->stream, kind, gid, np, (const uint32_t*)cnt, (const uint32_t*)build.grp_off,
                       (const uint32_t*)build.rows_desc, probe_rows, build_rows);
    AQG_TRY(aqg_check_launch(ctx, "join_emit_kernel"));
    return aqg_sync(ctx);
}
