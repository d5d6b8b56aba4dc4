// groupby_hashed.hip -- the hashed row pass of the group-by: agg_kernel over LDS tables (one or MAX_PASSES hash classes) or the HBM table.
// Any dtypes / MIN / MAX / VAR, packed or wide tuples; the plan that takes it is made in groupby.hip (RowPass::HASHED).
#include "groupby_plan.hpp"

namespace {

// ---- the single-pass aggregation kernel -------------------------------------------------------
// K32: one 4-byte key column (h2o Q1/Q3/Q4/Q5).  LDS slot = {key32, first_row32} in one 8-byte
// word, so a hit costs one ds_read_b64 + one LDS atomic per accumulator.
// Tables that do not fit one 64 KB LDS table (up to ~25,000 groups: h2o Q2) use BLOCK = 1024, one workgroup per CU with a table
// of up to 150 KB (gfx950: 160 KB of LDS per workgroup), and `npass` passes over the rows: pass p aggregates only the keys
// whose pass hash equals p, so every pass's groups fit the table.  npass x (key + value bytes) of streaming reads beat the
// ~3e10/s scattered HBM atomics of the global table by an order of magnitude (Q2, 1e9 rows: 54 ms -> see DESIGN.md).
constexpr uint32_t SKIP = 0xFFFFFFFEu;          // row belongs to another pass
template <bool USE_LDS, bool K32, int NACC, int BLOCK = 256>
__global__ void __launch_bounds__(BLOCK) agg_kernel(KeySpec ks, AccSpec as, GTable gt, uint32_t n, uint32_t lcap, int need_count, uint32_t lrep, uint32_t npass) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // LDS layout (USE_LDS): lkey u64[lcap+1] | lacc[a] u64[lcap+1] ... | lfirst u32[lcap+1] (wide keys) | lcount u32[lcap+1] | lused u32
    // `lrep` replicas of the table (lane l uses replica l % lrep) cut same-address / same-bank conflicts
    // of the LDS atomics when there are fewer groups than lanes
    const uint32_t LT = USE_LDS ? lrep * (lcap + 1) : 0;   // total LDS slots
    uint64_t* lkey = reinterpret_cast<uint64_t*>(smem_raw);
    uint64_t* lacc = lkey + LT;
    uint32_t* lfirst = reinterpret_cast<uint32_t*>(lacc + (size_t)NACC * LT);
    uint32_t* lcount = lfirst + (K32 ? 0 : LT);
    uint32_t* lused = lcount + (need_count ? LT : 0);
    const uint32_t rbase = USE_LDS ? (threadIdx.x & (lrep - 1)) * (lcap + 1) : 0;
    const uint32_t llimit = lcap - (lcap >> 2);   // stop inserting at 75 % load; further new keys go to HBM
    // slot of a hash: multiply-shift, so the capacity need not be a power of two (it is sized to the LDS budget)
    // h1 is a Fibonacci hash: its top bits pick the pass, the remaining bits (h1 * npass drops exactly the pass bits) pick the
    // slot.  Consecutive integer keys -- dictionary ids, the usual group-by key -- land almost evenly spaced (three-distance
    // theorem), so they hardly ever collide; a second, random-looking mix here cost the build path 2.7x on h2o Q1 (100 dense keys).
    auto home = [&](uint32_t h1) -> uint32_t { return __umulhi(h1 * npass, lcap); };

  for (uint32_t pass = 0; pass < npass; ++pass) {
    if constexpr (USE_LDS) {
        if (pass) __syncthreads();
        for (uint32_t s = threadIdx.x; s < LT; s += blockDim.x) {
            if constexpr (K32) lkey[s] = ((uint64_t)NOROW << 32) | EMPTY32; else { lkey[s] = EMPTY64; lfirst[s] = NOROW; }
            _Pragma("unroll") for (int a = 0; a < NACC; ++a) lacc[(size_t)a * LT + s] = acc_init(as.kind[a]);
            if (need_count) lcount[s] = 0;
        }
        if (threadIdx.x < lrep) lused[threadIdx.x] = 0;
        __syncthreads();
    }

    // returns the LDS slot of `key` (inserting it), or FAIL when the table is at its load limit
    auto lds_slot = [&](uint64_t key, uint32_t s) -> uint32_t {   // s: home slot
        if constexpr (K32) {
            uint32_t k = (uint32_t)key;
            if (k == EMPTY32) return rbase + lcap;
            uint32_t* kw = reinterpret_cast<uint32_t*>(lkey + rbase);
            uint32_t* used = lused + (threadIdx.x & (lrep - 1));
            for (uint32_t p = 0; p < lcap; ++p) {
                uint32_t cur = kw[2 * s];
                if (cur == k) return rbase + s;
                if (cur == EMPTY32) {
                    if (*used >= llimit) return FAIL;
                    uint32_t old = atomicCAS(&kw[2 * s], EMPTY32, k);
                    if (old == EMPTY32) { atomicAdd(used, 1u); return rbase + s; }
                    if (old == k) return rbase + s;
                }
                s = s + 1 == lcap ? 0 : s + 1;
            }
            return FAIL;
        } else {
            if (key == EMPTY64) return rbase + lcap;
            uint64_t* kw = lkey + rbase;
            uint32_t* used = lused + (threadIdx.x & (lrep - 1));
            for (uint32_t p = 0; p < lcap; ++p) {
                uint64_t cur = kw[s];
                if (cur == key) return rbase + s;
                if (cur == EMPTY64) {
                    if (*used >= llimit) return FAIL;
                    unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&kw[s]), EMPTY64, key);
                    if (old == EMPTY64) { atomicAdd(used, 1u); return rbase + s; }
                    if (old == key) return rbase + s;
                }
                s = s + 1 == lcap ? 0 : s + 1;
            }
            return FAIL;
        }
    };
    auto lds_touch_first = [&](uint32_t s, uint32_t row) {
        uint32_t* f = K32 ? reinterpret_cast<uint32_t*>(lkey) + 2 * s + 1 : lfirst + s;
        if (row < *f) atomicMin(f, row);
    };

    // one row whose slot is known
    auto to_global = [&](uint64_t key, uint32_t row, const uint64_t* vals) {
        uint32_t g = ks.wide ? gt_find_or_insert_wide(gt, ks, row) : gt_find_or_insert(gt, key);
        if (g == FAIL) return;
        gt_touch_first(gt, g, row);
        if (need_count) atomicAdd(gt.count_p(g), 1u);
        _Pragma("unroll") for (int a = 0; a < NACC; ++a) acc_apply(gt.acc_p(a, g), as.kind[a], vals[a]);
    };

    const uint32_t nchunk = n >> 2;   // 4 consecutive rows per lane per step
    const bool vec_ok = K32 && ks.nkeys == 1;
    uint32_t c_lo, c_hi;
    wg_span(nchunk, c_lo, c_hi);
    for (uint32_t c = c_lo + threadIdx.x; c < c_hi; c += blockDim.x) {
        const size_t base = (size_t)c * 4;
        uint64_t key[4];
        if (vec_ok) {
            pack<uint32_t, 4> kv = *reinterpret_cast<const pack<uint32_t, 4>*>(static_cast<const uint32_t*>(ks.col[0]) + base);
#pragma unroll
            for (int j = 0; j < 4; ++j) key[j] = kv.v[j];
        } else if (!ks.wide) {
            pack_key4(ks, base, key);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) key[j] = base + j;
        }
        uint64_t vals[NACC ? NACC : 1][4];
        _Pragma("unroll") for (int a = 0; a < NACC; ++a) val_operand4(as.dt[a], as.col[a], base, as.kind[a], as.square[a], as.part[a], vals[a]);
        uint32_t slot[4];
        if constexpr (USE_LDS) {
            // speculative first probe of all four rows at once: one LDS round trip in the common (hit) case
            uint64_t w[4];
            uint32_t hs[4];                     // home slot (without the replica base)
#pragma unroll
            for (int j = 0; j < 4; ++j) {     // all four probes are issued unconditionally (a branch in front of an LDS read serialises them)
                const uint32_t h1 = lds_h1<K32>(key[j]);
                hs[j] = home(h1);
                w[j] = lkey[rbase + hs[j]];
                slot[j] = npass > 1 && __umulhi(h1, npass) != pass ? SKIP : rbase + hs[j];
            }
            if constexpr (K32) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint32_t row = (uint32_t)base + j;
                    if (slot[j] == SKIP) continue;
                    if ((uint32_t)w[j] == (uint32_t)key[j] && (uint32_t)key[j] != EMPTY32) {
                        if (row < (uint32_t)(w[j] >> 32)) atomicMin(reinterpret_cast<uint32_t*>(lkey) + 2 * slot[j] + 1, row);
                    } else {
                        slot[j] = lds_slot(key[j], hs[j]);
                        if (slot[j] != FAIL) lds_touch_first(slot[j], row);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (slot[j] == SKIP) continue;
                    if (!(w[j] == key[j] && key[j] != EMPTY64)) slot[j] = lds_slot(key[j], hs[j]);
                    if (slot[j] != FAIL) lds_touch_first(slot[j], (uint32_t)base + j);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) slot[j] = FAIL;
        }
        if (need_count) {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (slot[j] < SKIP) atomicAdd(&lcount[slot[j]], 1u);
        }
        _Pragma("unroll") for (int a = 0; a < NACC; ++a) {
            uint64_t* la = lacc + (size_t)a * LT;
            switch (as.kind[a]) {   // wave-uniform: one branch per accumulator per four rows
            case ACC_ADD_I:
#pragma unroll
                for (int j = 0; j < 4; ++j) if (slot[j] < SKIP) atomicAdd(reinterpret_cast<unsigned long long*>(&la[slot[j]]), (unsigned long long)vals[a][j]);
                break;
            case ACC_ADD_F:
#pragma unroll
                for (int j = 0; j < 4; ++j) if (slot[j] < SKIP) atomicAdd(reinterpret_cast<double*>(&la[slot[j]]), __builtin_bit_cast(double, vals[a][j]));
                break;
            case ACC_MIN:
#pragma unroll
                for (int j = 0; j < 4; ++j) if (slot[j] < SKIP) atomicMin(reinterpret_cast<unsigned long long*>(&la[slot[j]]), (unsigned long long)vals[a][j]);
                break;
            default:
#pragma unroll
                for (int j = 0; j < 4; ++j) if (slot[j] < SKIP) atomicMax(reinterpret_cast<unsigned long long*>(&la[slot[j]]), (unsigned long long)vals[a][j]);
                break;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (slot[j] == FAIL) {   // LDS table full (or HBM mode): straight to the global table
                uint64_t v1[NACC ? NACC : 1];
                _Pragma("unroll") for (int a = 0; a < NACC; ++a) v1[a] = vals[a][j];
                to_global(key[j], (uint32_t)base + j, v1);
            }
        }
    }
    // tail rows (< 4) by the first lanes of block 0
    if (blockIdx.x == 0 && pass == 0) {
        uint32_t row = (nchunk << 2) + threadIdx.x;
        if (row < n) {
            uint64_t k = ks.wide ? (uint64_t)row : pack_key(ks, row);
            uint64_t v1[NACC ? NACC : 1];
            _Pragma("unroll") for (int a = 0; a < NACC; ++a) v1[a] = val_operand(as.dt[a], as.col[a], row, as.kind[a], as.square[a], as.part[a]);
            to_global(k, row, v1);
        }
    }

    if constexpr (USE_LDS) {
        __syncthreads();
        // merge this workgroup's table into the global one
        for (uint32_t s = threadIdx.x; s < LT; s += blockDim.x) {
            uint64_t key; uint32_t first;
            if constexpr (K32) {
                uint64_t w = lkey[s];
                first = (uint32_t)(w >> 32);
                key = (uint32_t)w;
            } else { key = lkey[s]; first = lfirst[s]; }
            if (first == NOROW) continue;          // never touched (covers the sentinel slot too)
            uint32_t g = gt_find_or_insert(gt, key);
            if (g == FAIL) continue;
            atomicMin(gt.first_p(g), first);
            if (need_count) atomicAdd(gt.count_p(g), lcount[s]);
            _Pragma("unroll") for (int a = 0; a < NACC; ++a) acc_apply(gt.acc_p(a, g), as.kind[a], lacc[(size_t)a * LT + s]);
        }
    }
  }   // passes
}

} // namespace

// the hashed table: LDS (one or MAX_PASSES hash classes) or HBM
int aqg_pass_hashed(aqg_ctx* ctx, const AggPlan& p, const GTable& gt) {
    const AccSpec& as = p.plan.as;
    // (one table per workgroup: replicas were measured slower on MI355X, h2o Q1, 100 groups: 1 replica 1.98 ms, 4 replicas 2.12 ms per 1e9 rows)
    const size_t lds = p.use_lds ? (size_t)(p.lcap + 1) * p.lds_slot_bytes + 4 * 64 : 0;
    const unsigned bpc = !p.use_lds ? 8 : lds <= 20 * 1024 ? 8 : lds <= 40 * 1024 ? 4 : lds <= 80 * 1024 ? 2 : 1;
    const unsigned block = p.big_lds ? (as.nacc <= 2 ? 1024 : 512) : 256;
    const unsigned grid = p.big_lds ? (unsigned)ctx->num_cu : aqg_grid(ctx, p.n / 4 + 1, 256, 2, bpc);
    auto launch = [&](auto kern) -> int {
        if (lds) AQG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, ctx->stream, p.ks, as, gt, p.n, p.lcap, p.plan.need_count, 1u, p.npass);
        return AQG_OK;
    };
    auto by_nacc = [&](auto lds_tag, auto k32_tag, auto block_tag) -> int {
        constexpr bool L = decltype(lds_tag)::value, K = decltype(k32_tag)::value;
        constexpr int B = decltype(block_tag)::value;
        // big tables: 1024 threads per workgroup up to 2 accumulators (<= 128 VGPRs without spills), 512 beyond
#define AQG_AGG_CASE(N) case N: if constexpr ((B == 1024 && N > 2) || (B == 512 && N <= 2)) return AQG_ERR_ARG; else return launch(&agg_kernel<L, K, N, B>);
        switch (as.nacc) {
        AQG_AGG_CASE(0) AQG_AGG_CASE(1) AQG_AGG_CASE(2) AQG_AGG_CASE(3) AQG_AGG_CASE(4) AQG_AGG_CASE(5) AQG_AGG_CASE(6) AQG_AGG_CASE(7)
        default: if constexpr (B == 1024) return AQG_ERR_ARG; else return launch(&agg_kernel<L, K, 8, B>);
        }
#undef AQG_AGG_CASE
    };
    auto by_k32 = [&](auto lds_tag, auto block_tag) -> int { return p.k32 ? by_nacc(lds_tag, std::true_type{}, block_tag) : by_nacc(lds_tag, std::false_type{}, block_tag); };
    aqg_kernel_timer_begin(ctx);
    if (p.big_lds && block == 1024) AQG_TRY(by_k32(std::true_type{}, std::integral_constant<int, 1024>{}));
    else if (p.big_lds) AQG_TRY(by_k32(std::true_type{}, std::integral_constant<int, 512>{}));
    else if (p.use_lds) AQG_TRY(by_k32(std::true_type{}, std::integral_constant<int, 256>{}));
    else AQG_TRY(by_k32(std::false_type{}, std::integral_constant<int, 256>{}));
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "agg_kernel");
}
