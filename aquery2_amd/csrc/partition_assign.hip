// partition_assign.hip -- the build's id pass over the rows a partition plan left (aqg_partition_assign*), and the routing of the ids back
// into row order through the tile scatter of tile_scatter.hip
#include "partition1_int.hpp"
#include "tile_scatter.hpp"

// ==== the BUILD through the partition plans: group id of every row ============================================================================
// aqg_groupby_build needs, beyond the group table, the dense id of every row (AQHashTable's reversemap, server/hasher.h:167-179).  Up to
// here a build above the LDS tables inserted every row into an HBM table and looked every row up again (1e9 rows, 1e7 groups: 37 + 47 ms
// of scattered HBM accesses).  Now the group table comes from the partition plan (no accumulators, counts only), and the rows -- still
// lying partitioned in the workspace, {key, row id} -- are walked ONCE more per partition: the partition's records (p1_agg notes which
// range of the record table it wrote) go into an LDS table {key -> dense id of the record}, every row probes it and writes
// reversemap[row id].  8 B/row read + a scattered 4-byte write per row.
namespace {
template <bool K64>
__global__ void __launch_bounds__(1024) p_assign_kernel(PartRows pr, GTable gt, const uint32_t* __restrict__ slot_gid, uint32_t* __restrict__ gid_part /* [ntotal]: the id of the row at every partitioned position */) {
    using K = key_t_<K64>;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    K* ktab = reinterpret_cast<K*>(smem_raw);                        // [cap]
    uint32_t* gtab = reinterpret_cast<uint32_t*>(ktab + pr.cap);     // [cap]
    __shared__ uint32_t special_gid;
    const K EMPTYK = empty_key<K64>();
    const uint32_t cap = pr.cap, NB = pr.nparts;
    for (uint32_t part = blockIdx.x; part < NB; part += gridDim.x) {
        const uint32_t b = pr.pstart[(size_t)part * pr.pstride];
        const uint32_t e = part + 1 < NB ? pr.pstart[(size_t)(part + 1) * pr.pstride] : pr.ntotal;
        if (b == e) continue;
        const uint32_t base = pr.part_base[2 * (size_t)part], used = pr.part_base[2 * (size_t)part + 1];
        for (uint32_t s = threadIdx.x; s < cap; s += 1024) ktab[s] = EMPTYK;
        if (threadIdx.x == 0) special_gid = 0;
        __syncthreads();
        for (uint32_t r = threadIdx.x; r < used; r += 1024) {         // this partition's records -> {key -> dense id}
            const uint32_t rec = base + r;
            const K k = (K)*gt.key_p(rec);
            const uint32_t gid = slot_gid[rec];
            if (k == EMPTYK) { special_gid = gid; continue; }
            uint32_t slot = __umulhi(key_hash<K64>(k) * NB, cap);
            for (uint32_t step = 0; step < cap; ++step) {
                K c;
                if constexpr (K64) c = atomicCAS(reinterpret_cast<unsigned long long*>(&ktab[slot]), (unsigned long long)EMPTYK, (unsigned long long)k);
                else c = atomicCAS(&ktab[slot], EMPTYK, k);
                if (c == EMPTYK || c == k) { gtab[slot] = gid; break; }
                slot = slot + 1 == cap ? 0 : slot + 1;
            }
        }
        __syncthreads();
        {   // a lane takes AR consecutive rows of a step by 16-byte loads and stores (4-byte aligned: a partition starts anywhere), the next step's
            // keys in flight while this step's are looked up (four rows per lane by dword loads, one step at a time: 2.3 ms per 1e9 rows)
            constexpr int AR = K64 ? 4 : 8;
            constexpr uint32_t STEP = 1024 * AR;
            struct Batch { K key[AR]; };
            auto load_full = [&](uint32_t i0, Batch& t) { __builtin_memcpy(t.key, static_cast<const K*>(pr.keys) + i0 + threadIdx.x * AR, sizeof t.key); };
            const uint32_t nfull = (e - b) / STEP, nsteps = nfull + ((e - b) % STEP ? 1u : 0u);
            const uint32_t safe_last = nfull ? b + (nfull - 1) * STEP : (b + STEP <= pr.ntotal ? b : pr.ntotal - STEP);    // (the partitioned build runs from 2^20 rows)
            Batch cur;
            load_full(nfull ? b : safe_last, cur);
            uint32_t i0 = b;
            for (uint32_t st = 0; st < nsteps; ++st, i0 += STEP) {
                const bool edge = st >= nfull;
                const uint32_t o = i0 + threadIdx.x * AR;
                if (edge) {
#pragma unroll
                    for (int q = 0; q < AR; ++q) cur.key[q] = static_cast<const K*>(pr.keys)[o + q < e ? o + q : e - 1];
                }
                Batch nxt;
                load_full(st + 1 < nfull ? i0 + STEP : safe_last, nxt);
                __builtin_amdgcn_sched_barrier(0);
                uint32_t slot[AR], gid[AR]; K w[AR];
#pragma unroll
                for (int q = 0; q < AR; ++q) { slot[q] = __umulhi(key_hash<K64>(cur.key[q]) * NB, cap); w[q] = ktab[slot[q]]; }
#pragma unroll
                for (int q = 0; q < AR; ++q) {
                    if (cur.key[q] == EMPTYK) gid[q] = special_gid;
                    else {
                        uint32_t sl = slot[q];
                        K c = w[q];
                        for (uint32_t step = 0; c != cur.key[q] && step < cap; ++step) { sl = sl + 1 == cap ? 0 : sl + 1; c = ktab[sl]; }
                        gid[q] = gtab[sl];
                    }
                }
                if (!edge) __builtin_memcpy(gid_part + o, gid, sizeof gid);
                else {
#pragma unroll
                    for (int q = 0; q < AR; ++q) if (o + q < e) gid_part[o + q] = gid[q];
                }
                cur = nxt;
            }
        }
        __syncthreads();
    }
}
// out[idx[i]] = val[i] for a PERMUTATION idx of 0 .. n-1 (every row id once): a scattered 4-byte store per row runs at the rate of the
// memory side (~3e10/s: 43 ms per 1e9 rows as the build's last step), so the pairs {idx, val} are first partitioned on idx -- order-
// preserving bins, the tile scatter again, no histogram: a partition's size IS its index interval -- until an interval spans 64 K
// rows; the stores of a workgroup then land inside a 256 KB window that its L2 turns into whole lines.
// the last step: partition p holds exactly the pairs whose index lies in [pstart[p], pstart[p + 1]) -- as many pairs as indices.  One
// workgroup per partition places the values in LDS by index (a window of 32 K indices at a time: a partition of 64 K rows takes two sweeps
// over its pairs) and streams the window out: every store instruction writes whole lines.  (Plain stores through the index, every
// workgroup inside its own 256 KB window: 14 ms per 1e9 rows -- 2048 such windows do not fit the L2s.)
constexpr uint32_t ROUTE_W = 32768;
__global__ void __launch_bounds__(1024) route_final_kernel(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ val, const uint32_t* __restrict__ pstart, uint32_t nparts,
                                                           uint32_t n, uint32_t* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint32_t* win = reinterpret_cast<uint32_t*>(smem_raw);
    for (uint32_t p = blockIdx.x; p < nparts; p += gridDim.x) {
        const uint32_t b = pstart ? pstart[p] : 0u, e = pstart ? pstart[p + 1] : n;
        for (uint32_t w0 = b; w0 < e; w0 += ROUTE_W) {
            const uint32_t w1 = e - w0 < ROUTE_W ? e : w0 + ROUTE_W;
            // (consecutive pairs per lane by 16-byte loads with the next step in flight -- what took gid_agg from 2 to 5.6 TB/s -- changed nothing here:
            // 3.32 against 3.36 ms; a partition of up to 65536 rows is read once per 32768-row window and the window's random LDS stores are what it waits for)
            for (uint32_t i0 = b + threadIdx.x; i0 < e; i0 += 4 * 1024) {
                uint32_t r[4], v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) { const uint32_t i = i0 + q * 1024, ic = i < e ? i : e - 1; r[q] = idx[ic]; v[q] = val[ic]; }
#pragma unroll
                for (int q = 0; q < 4; ++q) if (i0 + q * 1024 < e && r[q] >= w0 && r[q] < w1) win[r[q] - w0] = v[q];
            }
            __syncthreads();
            for (uint32_t j = threadIdx.x; j < w1 - w0; j += 1024) out[w0 + j] = win[j];
            __syncthreads();
        }
    }
}
size_t aqg_route_ws_bytes(uint32_t n) { return ((size_t)n + 64) * 16 + ((size_t)1 << 20); }
int aqg_route_by_row(aqg_ctx* ctx, const uint32_t* idx, const uint32_t* val, uint32_t n, uint32_t* out) {
    uint32_t bits = 0;
    while (bits < 21 && ((uint64_t)n >> bits) > 65536) ++bits;
    const uint32_t* isrc = idx;
    const uint32_t* vsrc = val;
    const uint32_t* final_pstart = nullptr;
    if (bits) {
        const uint32_t levels = (bits + 6) / 7, PP = 1u << bits;
        const uint32_t M = (uint32_t)((((uint64_t)1 << bits) << 32) / n);
        uint32_t *iA, *iB, *vA, *vB, *pstart, *pfirst, *seg, *tp, *cur;
        AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &iA)); AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &iB));
        AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &vA)); AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &vB));
        AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &pstart)); AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &pfirst));
        AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &seg)); AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &tp)); AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &cur));
        aqg_gid_setup(ctx, nullptr, n, M, PP, pstart, pfirst);                  // (no offsets: a partition's size is its index interval)
        final_pstart = pstart;
        const LevelBufs lb{seg, tp, nullptr, cur, nullptr};
        uint32_t nseg = 1;
        for (uint32_t l = 0; l < levels; ++l) {
            uint32_t shift;
            const uint32_t nb = 1u << aqg_level_bits(bits, levels, l, &shift);
            uint32_t* idst = (l & 1) ? iB : iA;
            uint32_t* vdst = (l & 1) ? vB : vA;
            Planes pl;
            memset(&pl, 0, sizeof pl);
            pl.add_column(isrc, idst, 4); pl.add_column(vsrc, vdst, 4);
            AQG_TRY(aqg_scatter_level_offsets(ctx, lb, pstart, false, 0u, isrc, pl, n, nseg, M, shift, nb, "route by row: level"));
            nseg *= nb;
            isrc = idst; vsrc = vdst;
        }
    }
    AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(&route_final_kernel), (size_t)ROUTE_W * 4));
    hipLaunchKernelGGL(route_final_kernel, dim3(bits ? (1u << bits) : 1u), dim3(1024), (size_t)ROUTE_W * 4, ctx->stream, isrc, vsrc, final_pstart, bits ? (1u << bits) : 1u, n, out);
    return aqg_check_launch(ctx, "route_final_kernel");
}
} // namespace
size_t aqg_partition_assign_ws_bytes(uint32_t n) { return ((size_t)n + 64) * 4 + aqg_route_ws_bytes(n) + 65536; }
int aqg_partition_assign(aqg_ctx* ctx, const PartRows& pr, GTable gt, const uint32_t* slot_gid, uint32_t* reversemap) {
    if (!pr.valid) return aqg_fail(ctx, AQG_ERR_ARG, "partitioned build: no partitioned rows");
    uint32_t* gid_part;
    AQG_TRY(aqg_ws_get(ctx, (size_t)pr.ntotal + 64, &gid_part));
    const size_t lds = (size_t)pr.cap * (pr.ksz + 4) + 64;
    const unsigned grid = pr.nparts < 2u * (unsigned)ctx->num_cu ? pr.nparts : 2u * (unsigned)ctx->num_cu;
    if (pr.ksz == 4) {
        AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(&p_assign_kernel<false>), lds));
        hipLaunchKernelGGL((p_assign_kernel<false>), dim3(grid), dim3(1024), lds, ctx->stream, pr, gt, slot_gid, gid_part);
    } else {
        AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(&p_assign_kernel<true>), lds));
        hipLaunchKernelGGL((p_assign_kernel<true>), dim3(grid), dim3(1024), lds, ctx->stream, pr, gt, slot_gid, gid_part);
    }
    AQG_TRY(aqg_check_launch(ctx, "p_assign_kernel"));
    return aqg_route_by_row(ctx, pr.rows, gid_part, pr.ntotal, reversemap);      // the ids back into row order
}
