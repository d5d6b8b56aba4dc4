// groupby_few.hip -- the row pass of the fast LDS group-by for its most common shape: one 4-byte key column, one to four
// accumulators over 4-byte value columns (int32 / uint32 / float), a table that fits LDS_SMALL (h2o Q1).  Every other fast
// shape keeps agg32_kernel (groupby_fast.hip); the table layout, the merge into the group table and everything downstream are
// the same (groupby.hip, groupby_tail.hip).
//
// agg32_kernel reads its rows with plain 16-byte loads and tops out at ~5.7-5.8 TB/s however they are issued.  Here every wave
// streams its share of the workgroup's span through a ring of its own in LDS by global_load_lds_dwordx4 with the nt policy,
// one stage ahead, and reads back only what it loaded itself: no barrier and no ordinary global load in the row loop.  On
// MI355X the same stream with Q1's per-row LDS work ran at 6.9 TB/s against 6.1 TB/s with plain loads
// (profiles/r4_stream_ceiling.md).
#include "groupby_fast.hpp"

namespace {

constexpr int FEW_WAVES = 4;                          // 256-thread workgroups
constexpr int FEW_STAGES = 2;                         // ring stages per wave: one stage in flight while one is consumed
constexpr int FEW_SUB = 2;                            // 1 KB DMAs per column per stage: 8 rows per lane, as in agg32_kernel
constexpr uint32_t FEW_ROWS = 256 * FEW_SUB;          // rows of one stage
constexpr size_t FEW_COL_BYTES = 1024 * FEW_SUB;      // one column of one stage
constexpr size_t FEW_LDS_PER_CU = 160 * 1024, FEW_LDS_MAX = 150 * 1024;   // (150 KB: the largest workgroup the planner already launches)

constexpr size_t few_ring_bytes(int nv) { return (size_t)FEW_WAVES * FEW_STAGES * (1 + nv) * FEW_COL_BYTES; }

// 16 bytes per lane from `src` into LDS at the wave-uniform byte address `lds` + lane * 16, streaming (nt).  Issued by inline asm
// so that hipcc does not see it: it counts a __builtin_amdgcn_global_load_lds as a pending LDS write of unknown address and
// waits vmcnt(0) before every ds_read, which drains the ring.  Retired by the caller's counted s_waitcnt vmcnt.  M0 holds the
// LDS destination and is restored inside the statement.
__device__ inline void glds16_nt(const void* src, uint32_t lds) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds) : "memory");
}

template <int NV, bool COUNT>
__global__ void __launch_bounds__(256) few32_kernel(const uint32_t* __restrict__ keys, FastVals fv, GTable gt, uint32_t n, uint32_t lcap) {
    constexpr size_t STAGE = (1 + NV) * FEW_COL_BYTES;             // key column, then the value columns
    constexpr int DMAS = (1 + NV) * FEW_SUB;                        // DMA instructions per stage
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t LT = lcap + 1;
    uint64_t* lacc = reinterpret_cast<uint64_t*>(smem_raw + few_ring_bytes(NV));   // [NV][LT]
    uint32_t* lkey = reinterpret_cast<uint32_t*>(lacc + (size_t)NV * LT);          // [LT], slot lcap = the key equal to the empty mark
    uint32_t* lcount = lkey + LT;                                                   // [LT] if COUNT
    uint32_t* ltouch = lcount + (COUNT ? LT : 0);                                   // [1]  sentinel slot used?
    uint32_t* lused = ltouch + 1;                                                   // [1]
    const uint32_t lmask = lcap - 1, llimit = lcap - (lcap >> 2), lbits = 31 - __clz(lcap);
    for (uint32_t s = threadIdx.x; s < LT; s += blockDim.x) {
        lkey[s] = EMPTY32;
        _Pragma("unroll") for (int a = 0; a < NV; ++a) lacc[(size_t)a * LT + s] = acc_init(fv.kind[a]);
        if constexpr (COUNT) lcount[s] = 0;
    }
    if (threadIdx.x == 0) { *lused = 0; *ltouch = 0; }
    __syncthreads();

    auto slow_slot = [&](uint32_t k) -> uint32_t {     // insert path (first sight of a key in this workgroup)
        if (k == EMPTY32) { *ltouch = 1; return lcap; }
        uint32_t s = fib_slot(k, lbits);
        for (uint32_t p = 0; p <= lmask; ++p) {
            const uint32_t cur = lkey[s];
            if (cur == k) return s;
            if (cur == EMPTY32) {
                if (*lused >= llimit) return FAIL;
                const uint32_t old = atomicCAS(&lkey[s], EMPTY32, k);
                if (old == EMPTY32) { atomicAdd(lused, 1u); return s; }
                if (old == k) return s;
            }
            s = (s + 1) & lmask;
        }
        return FAIL;
    };
    auto operand = [&](int a, uint32_t bits) -> uint64_t {
        switch (fv.vkind[a]) {
        case 0: return val_operand_t((int32_t)bits, fv.kind[a], fv.square[a]);
        case 1: return val_operand_t(bits, fv.kind[a], fv.square[a]);
        default: return val_operand_t(__uint_as_float(bits), fv.kind[a], fv.square[a]);
        }
    };
    auto to_table = [&](uint32_t k, const uint32_t* vbits) {   // rare: LDS table at its load limit
        const uint32_t g = gt_find_or_insert(gt, (uint64_t)k);
        if (g == FAIL) return;
        atomicMin(gt.first_p(g), OCCUPIED);
        if constexpr (COUNT) atomicAdd(gt.count_p(g), 1u);
        _Pragma("unroll") for (int a = 0; a < NV; ++a) acc_apply(gt.acc_p(a, g), fv.kind[a], operand(a, vbits[a]));
    };
    // M rows: all probes issued before the first compare, then the accumulators (agg32_kernel's row, VW = 4)
    auto rows = [&](auto m_tag, const auto& k, const auto& v) {
        constexpr int M = decltype(m_tag)::value;
        uint32_t slot[M], cur[M];
#pragma unroll
        for (int j = 0; j < M; ++j) { slot[j] = fib_slot(k[j], lbits); cur[j] = lkey[slot[j]]; }
#pragma unroll
        for (int j = 0; j < M; ++j) if (cur[j] != k[j] || k[j] == EMPTY32) slot[j] = slow_slot(k[j]);
        if constexpr (COUNT) {
#pragma unroll
            for (int j = 0; j < M; ++j) if (slot[j] != FAIL) atomicAdd(&lcount[slot[j]], 1u);
        }
        _Pragma("unroll") for (int a = 0; a < NV; ++a) {
            uint64_t* la = lacc + (size_t)a * LT;
            // wave-uniform branches, one per accumulator per M rows; plain sums keep their own straight-line form
            if (fv.kind[a] == ACC_ADD_F && !fv.square[a]) {
#pragma unroll
                for (int j = 0; j < M; ++j) if (slot[j] != FAIL) atomicAdd(reinterpret_cast<double*>(&la[slot[j]]), (double)__uint_as_float(v[a][j]));
            } else if (fv.kind[a] == ACC_ADD_I && !fv.square[a] && fv.vkind[a] == 0) {
#pragma unroll
                for (int j = 0; j < M; ++j) if (slot[j] != FAIL) atomicAdd(reinterpret_cast<unsigned long long*>(&la[slot[j]]), (unsigned long long)(int64_t)(int32_t)v[a][j]);
            } else if (fv.kind[a] == ACC_ADD_I && !fv.square[a]) {
#pragma unroll
                for (int j = 0; j < M; ++j) if (slot[j] != FAIL) atomicAdd(reinterpret_cast<unsigned long long*>(&la[slot[j]]), (unsigned long long)v[a][j]);
            } else {
#pragma unroll
                for (int j = 0; j < M; ++j) if (slot[j] != FAIL) acc_apply(&la[slot[j]], fv.kind[a], operand(a, v[a][j]));
            }
        }
#pragma unroll
        for (int j = 0; j < M; ++j) {
            if (slot[j] == FAIL) {
                uint32_t vb[NV];
                _Pragma("unroll") for (int a = 0; a < NV; ++a) vb[a] = v[a][j];
                to_table(k[j], vb);
            }
        }
    };

    // the workgroup's span of whole stages; wave w takes stages w, w + FEW_WAVES, ... of it
    const uint32_t nstage = n / FEW_ROWS;
    uint32_t c_lo, c_hi;
    wg_span(nstage, c_lo, c_hi);
    const uint32_t first = c_lo + w;
    const uint32_t m = first < c_hi ? (c_hi - first + FEW_WAVES - 1) / FEW_WAVES : 0;
    unsigned char* ring = smem_raw + (size_t)w * FEW_STAGES * STAGE;
    const uint32_t ring_lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)ring);
    auto issue = [&](uint32_t i) {
        const size_t row = (size_t)(first + i * FEW_WAVES) * FEW_ROWS + lane * 4;
        const uint32_t st = ring_lds + (uint32_t)((i % FEW_STAGES) * STAGE);
#pragma unroll
        for (int r = 0; r < FEW_SUB; ++r) {
            glds16_nt(keys + row + r * 256, __builtin_amdgcn_readfirstlane(st + r * 1024));
            _Pragma("unroll") for (int a = 0; a < NV; ++a)
                glds16_nt(static_cast<const uint32_t*>(fv.col[a]) + row + r * 256, __builtin_amdgcn_readfirstlane(st + (uint32_t)((1 + a) * FEW_COL_BYTES) + r * 1024));
        }
    };
    static_assert(FEW_STAGES == 2, "the wait below leaves exactly one stage in flight");
    if (m) issue(0);
    for (uint32_t i = 0; i < m; ++i) {
        // the stage refilled now was read by the previous step: its ds_reads (and every LDS atomic) are done first
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (i + 1 < m) {
            issue(i + 1);
            asm volatile("s_waitcnt vmcnt(%0)" :: "i"(DMAS) : "memory");     // stage i has landed, stage i + 1 is in flight
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const unsigned char* st = ring + (size_t)(i % FEW_STAGES) * STAGE;
        uint32_t k[8], v[NV][8];
#pragma unroll
        for (int r = 0; r < FEW_SUB; ++r) {
            const pack<uint32_t, 4> kq = *reinterpret_cast<const pack<uint32_t, 4>*>(st + r * 1024 + lane * 16);
            _Pragma("unroll") for (int j = 0; j < 4; ++j) k[4 * r + j] = kq.v[j];
            _Pragma("unroll") for (int a = 0; a < NV; ++a) {
                const pack<uint32_t, 4> vq = *reinterpret_cast<const pack<uint32_t, 4>*>(st + (1 + a) * FEW_COL_BYTES + r * 1024 + lane * 16);
                _Pragma("unroll") for (int j = 0; j < 4; ++j) v[a][4 * r + j] = vq.v[j];
            }
        }
        rows(std::integral_constant<int, 8>{}, k, v);
    }
    if (blockIdx.x == gridDim.x - 1) {                 // rows after the last whole stage (< FEW_ROWS): plain loads, same table
        for (uint32_t row = nstage * FEW_ROWS + threadIdx.x; row < n; row += blockDim.x) {
            const uint32_t k[1] = {keys[row]};
            uint32_t v[NV][1];
            _Pragma("unroll") for (int a = 0; a < NV; ++a) v[a][0] = static_cast<const uint32_t*>(fv.col[a])[row];
            rows(std::integral_constant<int, 1>{}, k, v);
        }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < LT; s += blockDim.x) {
        const uint32_t key = lkey[s];
        if (s < lcap ? key == EMPTY32 : *ltouch == 0) continue;
        const uint32_t g = gt_find_or_insert(gt, s < lcap ? (uint64_t)key : (uint64_t)EMPTY32);
        if (g == FAIL) continue;
        atomicMin(gt.first_p(g), OCCUPIED);
        if constexpr (COUNT) atomicAdd(gt.count_p(g), lcount[s]);
        _Pragma("unroll") for (int a = 0; a < NV; ++a) acc_apply(gt.acc_p(a, g), fv.kind[a], lacc[(size_t)a * LT + s]);
    }
}

size_t few_lds_bytes(int nacc, bool need_count, uint32_t lcap) {
    return few_ring_bytes(nacc) + (size_t)(lcap + 1) * (4 + 8 * (size_t)nacc + (need_count ? 4 : 0)) + 16;
}

} // namespace

bool aqg_few_fits(int nacc, bool need_count, uint32_t lcap) {
    return nacc >= 1 && nacc <= 4 && few_lds_bytes(nacc, need_count, lcap) <= FEW_LDS_MAX;
}

int aqg_few_aggregate(aqg_ctx* ctx, const uint32_t* keys, int nacc, bool need_count, const FastVals& fv, GTable gt, uint32_t n, uint32_t lcap) {
    const size_t lds = few_lds_bytes(nacc, need_count, lcap);
    // two workgroups (8 waves) per CU kept the stream fullest; more waves, with the ring's LDS split finer, ran slower
    const size_t per_cu = FEW_LDS_PER_CU / lds;
    const unsigned grid = (unsigned)ctx->num_cu * (per_cu >= 2 ? 2u : 1u);
    auto launch = [&](auto kern) -> int {
        AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
        aqg_kernel_timer_begin(ctx);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * FEW_WAVES), lds, ctx->stream, keys, fv, gt, n, lcap);
        aqg_kernel_timer_end(ctx);
        return aqg_check_launch(ctx, "few32_kernel");
    };
    auto by_nv = [&](auto count_tag) -> int {
        constexpr bool C = decltype(count_tag)::value;
        switch (nacc) {
        case 1: return launch(&few32_kernel<1, C>);
        case 2: return launch(&few32_kernel<2, C>);
        case 3: return launch(&few32_kernel<3, C>);
        default: return launch(&few32_kernel<4, C>);
        }
    };
    return need_count ? by_nv(std::true_type{}) : by_nv(std::false_type{});
}
