// groupby_starjoin.hip -- the row pass of aqg_join_groupby_sum (RowPass::STARJOIN; the call itself: groupby.hip).
#include "groupby_plan.hpp"

namespace {

// ---- fused star join + group-by sum (BASELINE config 4: fact JOIN small(key, w) ON fk, sum(val * w) BY gkey) -----------------
// 12 B/row of HBM traffic (fk, gkey, val) instead of the 44 B/row of the composed lookup -> gather -> multiply -> group-by:
// the dimension side {key -> w} is an LDS open-addressing table built by every workgroup from the (small) dimension columns,
// the group table is the K32 LDS table of agg_kernel ({key, first_row} in one 8-byte word), and the exact 64-bit product is
// accumulated as two 64-bit sums of its 32-bit halves (no overflow for n < 2^32).  Fact rows without a partner are dropped
// (inner join); of duplicate dimension keys the lowest row wins (aqg_join_lookup's contract).
__global__ void __launch_bounds__(256) starjoin_kernel(const uint32_t* __restrict__ gkeys, StarJoin sj, GTable gt, uint32_t n, uint32_t lcap) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const uint32_t LT = lcap + 1;
    uint64_t* lkey = reinterpret_cast<uint64_t*>(smem_raw);          // [LT] {first_row << 32 | key}
    uint64_t* lacc = lkey + LT;                                      // [2][LT] sums of the low / high halves of the products
    uint32_t* dkey = reinterpret_cast<uint32_t*>(lacc + 2 * (size_t)LT);   // [dcap]
    uint32_t* dval = dkey + sj.dcap;                                 // [dcap] row while building, then w
    __shared__ uint32_t lused, dsent;                                // dsent: row / w of the dimension key equal to EMPTY32
    const uint32_t lmask = lcap - 1, llimit = lcap - (lcap >> 2), dmask = sj.dcap - 1, lbits = 31 - __clz(lcap), dbits = 31 - __clz(sj.dcap);
    for (uint32_t s = threadIdx.x; s < LT; s += blockDim.x) { lkey[s] = ((uint64_t)NOROW << 32) | EMPTY32; lacc[s] = 0; lacc[LT + s] = 0; }
    for (uint32_t s = threadIdx.x; s < sj.dcap; s += blockDim.x) { dkey[s] = EMPTY32; dval[s] = NOROW; }
    if (threadIdx.x == 0) { lused = 0; dsent = NOROW; }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < sj.nb; r += blockDim.x) {     // dimension table: key -> lowest row
        const uint32_t k = sj.dim_keys[r];
        if (k == EMPTY32) { atomicMin(&dsent, r); continue; }
        uint32_t s = fib_slot(k, dbits);
        while (true) {
            uint32_t cur = dkey[s];
            if (cur == EMPTY32) { uint32_t old = atomicCAS(&dkey[s], EMPTY32, k); cur = old == EMPTY32 ? k : old; }
            if (cur == k) { atomicMin(&dval[s], r); break; }
            s = (s + 1) & dmask;
        }
    }
    __syncthreads();
    __shared__ uint32_t wmax;                                        // largest |w| of the dimension side
    if (threadIdx.x == 0) wmax = 0;
    __syncthreads();
    {
        uint32_t m = 0;
        for (uint32_t r = threadIdx.x; r < sj.nb; r += blockDim.x) {
            const uint32_t wb = sj.dim_vals[r];
            const uint32_t a = sj.dim_signed ? (uint32_t)((int32_t)wb < 0 ? 0u - wb : wb) : wb;
            m = a > m ? a : m;
        }
        m = wave_reduce(m, OpMax{});
        if (lane_id() == 0) atomicMax(&wmax, m);
    }
    for (uint32_t s = threadIdx.x; s < sj.dcap; s += blockDim.x) if (dval[s] != NOROW) dval[s] = sj.dim_vals[dval[s]];
    const bool has_sent = dsent != NOROW;
    const uint32_t sent_w = has_sent ? sj.dim_vals[dsent] : 0;
    __syncthreads();

    auto group_slot = [&](uint32_t k) -> uint32_t {                  // insert path of the group table
        if (k == EMPTY32) return lcap;
        uint32_t* kw = reinterpret_cast<uint32_t*>(lkey);
        uint32_t s = fib_slot(k, lbits);
        for (uint32_t p = 0; p <= lmask; ++p) {
            uint32_t cur = kw[2 * s];
            if (cur == k) return s;
            if (cur == EMPTY32) {
                if (lused >= llimit) return FAIL;
                uint32_t old = atomicCAS(&kw[2 * s], EMPTY32, k);
                if (old == EMPTY32) { atomicAdd(&lused, 1u); return s; }
                if (old == k) return s;
            }
            s = (s + 1) & lmask;
        }
        return FAIL;
    };
    const bool any_signed = sj.val_signed || sj.dim_signed;
    auto product = [&](uint32_t vbits, uint32_t wbits) -> uint64_t {   // exact 64-bit product (bits)
        const int64_t v = sj.val_signed ? (int64_t)(int32_t)vbits : (int64_t)vbits;
        const int64_t w = sj.dim_signed ? (int64_t)(int32_t)wbits : (int64_t)wbits;
        return (uint64_t)v * (uint64_t)w;
    };
    auto lo_half = [&](uint64_t p) -> unsigned long long { return p & 0xFFFFFFFFull; };
    auto hi_half = [&](uint64_t p) -> unsigned long long { return any_signed ? (unsigned long long)((int64_t)p >> 32) : p >> 32; };
    auto to_global = [&](uint32_t k, uint32_t row, uint64_t p) {     // LDS table at its load limit, or tail rows
        uint32_t g = gt_find_or_insert(gt, (uint64_t)k);
        if (g == FAIL) return;
        gt_touch_first(gt, g, row);
        atomicAdd(reinterpret_cast<unsigned long long*>(gt.acc_p(0, g)), lo_half(p));
        atomicAdd(reinterpret_cast<unsigned long long*>(gt.acc_p(1, g)), hi_half(p));
    };
    auto dim_lookup = [&](uint32_t k, uint32_t first_probe, uint32_t s, uint32_t& w) -> bool {   // first_probe = dkey[s]
        if (k == EMPTY32) { w = sent_w; return has_sent; }
        uint32_t cur = first_probe;
        for (uint32_t p = 0; p <= dmask; ++p) {
            if (cur == k) { w = dval[s]; return true; }
            if (cur == EMPTY32) return false;
            s = (s + 1) & dmask;
            cur = dkey[s];
        }
        return false;
    };

    constexpr int R = 8;                                             // rows per lane per step: two 16-byte loads per column
    const uint32_t nchunk = n / R;
    uint32_t c_lo, c_hi;
    wg_span(nchunk, c_lo, c_hi);
    // |product| < 2^32 * wmax; when this workgroup's rows cannot overflow 63 bits of that, ONE 64-bit LDS atomic per row carries
    // the whole product (split into its halves at the merge); otherwise the halves are summed separately
    const bool one_acc = (uint64_t)wmax * ((uint64_t)(c_hi - c_lo) * R + R) < (1ull << 31);
    // the 16-byte loads need 16-byte aligned columns; a column view that starts at an odd element takes 4-byte loads
    const bool aligned = ((reinterpret_cast<uintptr_t>(sj.fk) | reinterpret_cast<uintptr_t>(gkeys) | reinterpret_cast<uintptr_t>(sj.vals)) & 15) == 0;
    for (uint32_t c = c_lo + threadIdx.x; c < c_hi; c += blockDim.x) {
        const size_t base = (size_t)c * R;
        uint32_t f[R], g[R], v[R];
        if (aligned) {
#pragma unroll
            for (int h = 0; h < R / 4; ++h) {
                const pack<uint32_t, 4> f4 = *reinterpret_cast<const pack<uint32_t, 4>*>(sj.fk + base + 4 * h);
                const pack<uint32_t, 4> g4 = *reinterpret_cast<const pack<uint32_t, 4>*>(gkeys + base + 4 * h);
                const pack<uint32_t, 4> v4 = *reinterpret_cast<const pack<uint32_t, 4>*>(sj.vals + base + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) { f[4 * h + j] = f4.v[j]; g[4 * h + j] = g4.v[j]; v[4 * h + j] = v4.v[j]; }
            }
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j) { f[j] = sj.fk[base + j]; g[j] = gkeys[base + j]; v[j] = sj.vals[base + j]; }
        }
        uint32_t ds[R], dk[R], gs[R];
        uint64_t gw[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {                                // 2 R LDS probes in flight
            ds[j] = fib_slot(f[j], dbits); dk[j] = dkey[ds[j]];
            gs[j] = fib_slot(g[j], lbits); gw[j] = lkey[gs[j]];
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            uint32_t w;
            if (!dim_lookup(f[j], dk[j], ds[j], w)) continue;        // no partner: the row is not in the join
            const uint64_t p = product(v[j], w);
            const uint32_t row = (uint32_t)base + j, k = g[j];
            uint32_t s = gs[j];
            if ((uint32_t)gw[j] == k && k != EMPTY32) {
                if (row < (uint32_t)(gw[j] >> 32)) atomicMin(reinterpret_cast<uint32_t*>(lkey) + 2 * s + 1, row);
            } else {
                s = group_slot(k);
                if (s == FAIL) { to_global(k, row, p); continue; }
                uint32_t* fr = reinterpret_cast<uint32_t*>(lkey) + 2 * s + 1;
                if (row < *fr) atomicMin(fr, row);
            }
            if (one_acc) atomicAdd(reinterpret_cast<unsigned long long*>(&lacc[s]), (unsigned long long)p);
            else {
                atomicAdd(reinterpret_cast<unsigned long long*>(&lacc[s]), lo_half(p));
                atomicAdd(reinterpret_cast<unsigned long long*>(&lacc[LT + s]), hi_half(p));
            }
        }
    }
    if (blockIdx.x == 0) {                                           // tail rows (< R)
        const uint32_t row = nchunk * R + threadIdx.x;
        if (row < n) {
            const uint32_t k = sj.fk[row], s0 = fib_slot(k, dbits);
            uint32_t w;
            if (dim_lookup(k, dkey[s0], s0, w)) to_global(gkeys[row], row, product(sj.vals[row], w));
        }
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < LT; s += blockDim.x) {        // merge into the global table
        const uint64_t wd = lkey[s];
        const uint32_t first = (uint32_t)(wd >> 32);
        if (first == NOROW) continue;
        uint32_t g = gt_find_or_insert(gt, (uint64_t)(uint32_t)wd);
        if (g == FAIL) continue;
        atomicMin(gt.first_p(g), first);
        if (one_acc) {                                              // lacc[s] is the exact (signed or unsigned) 64-bit sum of this workgroup
            atomicAdd(reinterpret_cast<unsigned long long*>(gt.acc_p(0, g)), lo_half(lacc[s]));
            atomicAdd(reinterpret_cast<unsigned long long*>(gt.acc_p(1, g)), hi_half(lacc[s]));
        } else {
            atomicAdd(reinterpret_cast<unsigned long long*>(gt.acc_p(0, g)), (unsigned long long)lacc[s]);
            atomicAdd(reinterpret_cast<unsigned long long*>(gt.acc_p(1, g)), (unsigned long long)lacc[LT + s]);
        }
    }
}

} // namespace

int aqg_pass_starjoin(aqg_ctx* ctx, const AggPlan& p, const GTable& gt) {
    const size_t lds = (size_t)(p.lcap + 1) * 24 + (size_t)p.plan.sj->dcap * 8 + 64;
    const unsigned bpc = lds <= 20 * 1024 ? 8 : lds <= 40 * 1024 ? 4 : lds <= 80 * 1024 ? 2 : 1;
    AQG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&starjoin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    aqg_kernel_timer_begin(ctx);
    hipLaunchKernelGGL(starjoin_kernel, dim3(aqg_grid(ctx, p.n / 8 + 1, 256, 2, bpc)), dim3(256), lds, ctx->stream, static_cast<const uint32_t*>(p.ks.col[0]), *p.plan.sj, gt, p.n, p.lcap);
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "starjoin_kernel");
}
