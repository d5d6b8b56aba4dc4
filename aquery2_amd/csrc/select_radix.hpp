// select_radix.hpp -- the pieces of the MSD radix selection that select.hip (median) and topk.hip (top-k) both run: the constants of the three
// routes, images, the state of a selection between digits, the histogram pass, the bin choice, the SPLIT route's chunk plan and histogram
// kernel, and the host-side sizes and switches.  (select.hip's own header comment describes the algorithm.)
#pragma once
#include "select_dev.hpp"

namespace selradix {
using namespace seldev;

constexpr int SB = 256;                       // lanes per workgroup
constexpr int NWV = SB / 64;
constexpr uint32_t TILE = 2048;               // SMALL: flat positions per workgroup
constexpr uint32_t SMALL_CAP = 512;           // largest AQG_SELECT_SMALL_MAX (rows staged behind a tile)
constexpr uint32_t SPLIT_CHUNK = 8192;        // SPLIT: rows per chunk
constexpr int UNR = 4;                        // 16-byte loads in flight per lane
enum { KIND_UNSIGNED = 0, KIND_SIGNED = 1, KIND_FP = 2, KIND_DESC = 4 /* or-ed in by topk.hip: the complemented image, descending value */ };
enum { ROUTE_SMALL = 1, ROUTE_GROUP = 2, ROUTE_SPLIT = 4 };
// control words of a call (device, owned by the context): read back by aqg_select_last_routes
enum { CTL_ROUTES = 0, CTL_PASSES = 1, CTL_NGROUP = 2, CTL_NSPLIT = 3, CTL_NCHUNK = 4, CTL_RESULT = 8 /* 16 bytes */, CTL_OFF = 12 /* offsets {0, n} of the flat call */, CTL_WORDS = 16 };

template <class U, int KIND> __device__ inline U image_of(U r) {
    if constexpr ((KIND & KIND_DESC) != 0) return (U)~image_of<U, KIND & ~KIND_DESC>(r);
    else if constexpr (KIND == KIND_FP) return img_fp<U>(r);
    else return img_int<U, KIND == KIND_SIGNED>(r);
}
template <class U, int KIND> __device__ inline U value_of(U i) {
    if constexpr (KIND == KIND_FP) return unimg_fp<U>(i);
    else return unimg_int<U, KIND == KIND_SIGNED>(i);
}
// images that several bit patterns share (both zeros, every NaN): the element is looked up in the slice instead of rebuilt
template <class U, int KIND> __device__ inline bool image_is_shared(U i) {
    if constexpr (KIND == KIND_FP) return i == img_fp_zero<U>() || i == img_fp_nan<U>();
    else return false;
}

// the selection of one slice between digits
struct SelState {
    uint64_t prefix, kmask;       // image bits chosen so far / which bits those are
    uint64_t vand, vor;           // AND / OR of the images of the last pass's candidates
    uint32_t lo, hi, k, gidx;     // slice, rank among the candidates, group
    uint32_t shift, done;         // low bit of the next digit; 1: the image is known, 2: known and shared (the element is looked up)
    uint32_t cbase, passes;       // SPLIT: first chunk of the group; histogram passes so far
};
static_assert(sizeof(SelState) == 64, "SelState");

// after a pass: the bin `bin` (rows below it: excl, rows in it: cnt, candidates: total) holds the rank.  true: st.prefix is the whole image.
__device__ inline bool sel_advance(SelState& st, uint32_t bin, uint32_t excl, uint32_t cnt, uint32_t total) {
    st.k -= excl;
    st.prefix |= (uint64_t)bin << st.shift;
    st.kmask |= 0xFFull << st.shift;
    if (st.shift == 0) return true;
    const uint64_t below = (1ull << st.shift) - 1;
    if (cnt == total) {                                 // no candidate left the race: skip the bits they all share
        const uint64_t diff = (st.vand ^ st.vor) & below;
        if (!diff) { st.prefix |= st.vand & below; return true; }
        const int hb = 63 - __clzll((long long)diff);
        const uint32_t ns = hb >= 7 ? (uint32_t)hb - 7 : 0u;
        const uint64_t mid = below & ~((1ull << (ns + 8)) - 1);
        st.prefix |= st.vand & mid;
        st.kmask |= mid;
        st.shift = ns;
    } else {
        st.shift = st.shift >= 8 ? st.shift - 8 : 0u;
    }
    return false;
}

// histograms a pass fills.  2-byte columns count BOTH digits in their first pass: when every value shares the upper byte (small
// counters, flags) the lower byte's counts are already there and the column is read once
template <class U> constexpr uint32_t NHIST = sizeof(U) == 2 ? 2u : 1u;
// the first pass of a 2-byte column found every row in one bin of the upper digit: the lower digit's histogram decides
template <class U> __device__ inline bool both_digits_known(const SelState& st, uint32_t cnt, uint32_t total) {
    return sizeof(U) == 2 && st.passes == 1 && cnt == total && ((st.vand ^ st.vor) >> 8) == 0;
}

struct OpAnd { template <class T> __device__ T operator()(T a, T b) const { return (T)(a & b); } };
struct OpOr { template <class T> __device__ T operator()(T a, T b) const { return (T)(a | b); } };

// One histogram pass of a workgroup over rows [lo, hi) (lo < hi) of x: rows whose image matches `prefix` on `kmask` add their digit at
// `shift` to h (LDS; NHIST * 256 bins) and fold into vand / vor.  16-byte loads over the aligned middle of the slice, UNR of them in flight per lane; the
// up to 2 (V - 1) elements in front of and behind it take one lane each.
template <class U, int KIND>
__device__ inline void hist_rows(const U* __restrict__ x, uint32_t lo, uint32_t hi, U prefix, U kmask, uint32_t shift, uint32_t* h, U& vand, U& vor) {
    constexpr uint32_t V = 16 / sizeof(U);
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(x + lo) & 15);
    uint32_t hl = mis ? (16 - mis) / (uint32_t)sizeof(U) : 0u;
    if (hl > hi - lo) hl = hi - lo;
    const uint32_t a0 = lo + hl, nvec = (hi - a0) / V, ts = a0 + nvec * V, tl = hi - ts;
    auto row = [&](U raw, bool live) {
        const U im = image_of<U, KIND>(raw);
        const bool m = live && ((U)(im ^ prefix) & kmask) == 0;
        hist_add(h, (uint32_t)(im >> shift) & 255u, m);
        if constexpr (NHIST<U> == 2) { if (kmask == 0) hist_add(h + 256, (uint32_t)im & 255u, m); }
        vand &= m ? im : (U)~U(0);
        vor |= m ? im : U(0);
    };
    {
        const bool live = threadIdx.x < hl + tl;
        const uint32_t e = threadIdx.x < hl ? lo + threadIdx.x : ts + (threadIdx.x - hl);
        row(x[live ? e : lo], live);
    }
    const vec16<U>* xv = reinterpret_cast<const vec16<U>*>(x + a0);
    for (uint32_t vb = 0; vb < nvec; vb += SB * UNR) {
        vec16<U> r[UNR];
        bool live[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const uint32_t vi = vb + u * SB + threadIdx.x;
            live[u] = vi < nvec;
            r[u] = xv[live[u] ? vi : nvec - 1];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (uint32_t e = 0; e < V; ++e) row(r[u].v[e], live[u]);
    }
}
// vand / vor of the lanes -> the workgroup's (LDS)
template <class U> __device__ inline void fold_and_or(U vand, U vor, unsigned long long* s_and, unsigned long long* s_or) {
    vand = wave_reduce(vand, OpAnd{});
    vor = wave_reduce(vor, OpOr{});
    if (lane_id() == 0) { atomicAnd(s_and, (unsigned long long)vand); atomicOr(s_or, (unsigned long long)vor); }
}
// any element of rows [lo, hi) whose image is `im` -> *out (the writers race with equal-ranking elements: whichever lands is one of them)
template <class U, int KIND> __device__ inline void find_rows(const U* __restrict__ x, uint32_t lo, uint32_t hi, U im, U* out) {
    for (uint32_t i = lo + threadIdx.x; i < hi; i += SB) {
        const U raw = x[i];
        if (image_of<U, KIND>(raw) == im) { *out = raw; break; }
    }
}

struct BinSel { uint32_t bin, excl, cnt, total; };
// the bin that holds rank k, from this lane's bin count c (lane = bin)
__device__ inline void choose_bin(uint32_t c, uint32_t k, uint32_t* wsum, BinSel* sel) {
    const uint32_t incl = block_scan_incl(c, wsum);
    if (c && incl - c <= k && k < incl) { sel->bin = threadIdx.x; sel->excl = incl - c; sel->cnt = c; }
    if (threadIdx.x == SB - 1) sel->total = incl;
    __syncthreads();
}

// ---- SPLIT ----------------------------------------------------------------------------------------------------------------------------------
// chunk numbering: group s of the split list owns chunks [cbase, cbase + ceil(rows / SPLIT_CHUNK))
static __global__ void __launch_bounds__(SB) select_split_plan_kernel(SelState* __restrict__ sst, uint32_t* __restrict__ ctl) {
    __shared__ uint32_t wsum[NWV];
    const uint32_t ns = ctl[CTL_NSPLIT];
    uint32_t carry = 0;
    for (uint32_t b = 0; b < ns; b += SB) {
        const uint32_t s = b + threadIdx.x;
        const uint32_t nc = s < ns ? (sst[s].hi - sst[s].lo + SPLIT_CHUNK - 1) / SPLIT_CHUNK : 0u;
        const uint32_t incl = block_scan_incl(nc, wsum);
        if (s < ns) sst[s].cbase = carry + incl - nc;
        __shared__ uint32_t tot;
        if (threadIdx.x == SB - 1) tot = incl;
        __syncthreads();
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) ctl[CTL_NCHUNK] = carry;
}
// this workgroup's span of chunks and the split group its first chunk belongs to
__device__ inline bool split_span(const SelState* sst, const uint32_t* ctl, uint32_t& q0, uint32_t& q1, uint32_t& s, uint32_t& ns) {
    const uint32_t nchunk = ctl[CTL_NCHUNK];
    ns = ctl[CTL_NSPLIT];
    const uint32_t per = (nchunk + gridDim.x - 1) / gridDim.x;
    const uint64_t b = (uint64_t)blockIdx.x * per;
    if (b >= nchunk) return false;
    q0 = (uint32_t)b;
    q1 = b + per < nchunk ? (uint32_t)(b + per) : nchunk;
    uint32_t l = 0, r = ns;                                 // the last s with cbase <= q0
    while (r - l > 1) { const uint32_t m = (l + r) / 2; if (sst[m].cbase <= q0) l = m; else r = m; }
    s = l;
    return true;
}
template <class U, int KIND>
__global__ void __launch_bounds__(SB) select_split_hist_kernel(const U* __restrict__ x, SelState* sst, const uint32_t* __restrict__ ctl, uint32_t* __restrict__ ghist) {
    __shared__ uint32_t h[256 * NHIST<U>];
    __shared__ unsigned long long s_and, s_or;
    uint32_t q0, q1, s, ns;
    if (!split_span(sst, ctl, q0, q1, s, ns)) return;
    for (uint32_t j = 0; j < NHIST<U>; ++j) h[j * 256 + threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_and = ~0ull; s_or = 0ull; }
    __syncthreads();
    U vand = (U)~U(0), vor = 0;
    bool touched = false;
    auto flush = [&]() {                                    // this workgroup's share of group s -> HBM
        if (touched) {
            fold_and_or(vand, vor, &s_and, &s_or);
            __syncthreads();
            for (uint32_t j = 0; j < NHIST<U>; ++j)
                if (h[j * 256 + threadIdx.x]) atomicAdd(&ghist[((size_t)s * NHIST<U> + j) * 256 + threadIdx.x], h[j * 256 + threadIdx.x]);
            if (threadIdx.x == 0) { atomicAnd((unsigned long long*)&sst[s].vand, s_and); atomicOr((unsigned long long*)&sst[s].vor, s_or); }
            __syncthreads();
            for (uint32_t j = 0; j < NHIST<U>; ++j) h[j * 256 + threadIdx.x] = 0;
            if (threadIdx.x == 0) { s_and = ~0ull; s_or = 0ull; }
            __syncthreads();
        }
        vand = (U)~U(0); vor = 0; touched = false;
    };
    for (uint32_t q = q0; q < q1; ++q) {
        while (s + 1 < ns && sst[s + 1].cbase <= q) { flush(); ++s; }
        if (sst[s].done) continue;
        const uint32_t lo = sst[s].lo + (q - sst[s].cbase) * SPLIT_CHUNK, ghi = sst[s].hi;
        const uint32_t hi = ghi - lo < SPLIT_CHUNK ? ghi : lo + SPLIT_CHUNK;
        hist_rows<U, KIND>(x, lo, hi, (U)sst[s].prefix, (U)sst[s].kmask, sst[s].shift, h, vand, vor);
        touched = true;
    }
    flush();
}
// ---- host ----
struct SelSwitches { uint32_t small_max, split_min; };

inline uint32_t split_cap(uint32_t n, uint32_t G, uint32_t split_min) {       // most groups the SPLIT route can meet
    const uint32_t by_rows = n / (split_min ? split_min : 1u);
    return (by_rows < G ? by_rows : G) + 1;
}
inline size_t select_ws_bytes(uint32_t n, uint32_t G, SelSwitches sw) {
    auto rup = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const uint32_t glcap = (n / (sw.small_max + 1) < G ? n / (sw.small_max + 1) : G) + 1;
    return rup(((size_t)aqg_ceil_div(n, TILE) + 1) * 4) + rup((size_t)glcap * 4) + rup((size_t)split_cap(n, G, sw.split_min) * (sizeof(SelState) + 2048)) + 4096;
}
inline int ensure_ctl(aqg_ctx* ctx) {
    if (!ctx->select_ctl) AQG_HIP(ctx, hipMalloc(&ctx->select_ctl, 256));
    AQG_HIP(ctx, hipMemsetAsync(ctx->select_ctl, 0, CTL_WORDS * 4, ctx->stream));
    return AQG_OK;
}
inline SelSwitches select_switches() {
    const aqg_switch_set& s = aqg_switches();
    return SelSwitches{s.select_small_max < SMALL_CAP ? s.select_small_max : SMALL_CAP, s.select_split_min};
}

} // namespace selradix
