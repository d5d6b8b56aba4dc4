// select_radix.hpp -- the device side of the MSD radix selection that select.hip (median), topk.hip (top-k) and quantile.hip (quantiles)
// run; window_quantile.hip takes the images and the quantile ranks.  Here: the constants of the three routes, images, the state of a
// selection between digits, the load shape of a slice (sweep_rows), the histogram pass, the step after it (digit_step), the routing of the
// groups (classify_groups), the SMALL route (small_tile), and the SPLIT route's chunk plan and histogram kernel.  The host side is
// select_host.hpp.  (select.hip's own header comment describes the algorithm.)
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
constexpr uint32_t QMAX = AQG_QUANTILES_MAX;  // ranks of one quantile call
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

// the ranks of a quantile call: num[j] / den, j < nq, rounded down (which = AQG_SEL_LOWER) or up
struct QArgs { uint32_t nq, den, which, num[QMAX]; };
// rank of quantile num / den among c >= 1 rows: floor resp. ceil of num (c - 1) / den
__device__ inline uint32_t quantile_rank(const QArgs& a, uint32_t j, uint32_t c) {
    const uint64_t p = (uint64_t)a.num[j] * (c - 1);
    return (uint32_t)(p / a.den + (a.which && p % a.den != 0 ? 1u : 0u));
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
// the state of a SPLIT group before its first digit: rank k among the rows [lo, hi) of group g
__device__ inline SelState split_state(uint32_t lo, uint32_t hi, uint32_t k, uint32_t g, uint32_t bits) {
    SelState st{};
    st.vand = ~0ull;
    st.lo = lo; st.hi = hi; st.k = k; st.gidx = g;
    st.shift = bits - 8;
    return st;
}

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

// rows [lo, hi) (lo < hi) of x through f(raw, position, live), every lane of the workgroup calling f the same number of times: 16-byte loads
// over the aligned middle of the slice, UNR of them in flight per lane; the up to 2 (V - 1) elements in front of and behind it take one
// lane each.  (A dead call gets a row of the slice that is there, and live = false.)  f is taken by value: behind a reference, what a
// [&] lambda points to stays in memory across the LDS atomics of its body (profiles/r13_selection_skeleton.md).
template <class U, class F>
__device__ inline void sweep_rows(const U* __restrict__ x, uint32_t lo, uint32_t hi, F f) {
    constexpr uint32_t V = 16 / sizeof(U);
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(x + lo) & 15);
    uint32_t hl = mis ? (16 - mis) / (uint32_t)sizeof(U) : 0u;
    if (hl > hi - lo) hl = hi - lo;
    const uint32_t a0 = lo + hl, nvec = (hi - a0) / V, ts = a0 + nvec * V, tl = hi - ts;
    {
        const bool live = threadIdx.x < hl + tl;
        const uint32_t e = threadIdx.x < hl ? lo + threadIdx.x : ts + (threadIdx.x - hl);
        const uint32_t p = live ? e : lo;
        f(x[p], p, live);
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
            for (uint32_t e = 0; e < V; ++e) f(r[u].v[e], a0 + (vb + u * SB + threadIdx.x) * V + e, live[u]);
    }
}
// One histogram pass of a workgroup over rows [lo, hi) (lo < hi) of x: rows whose image matches `prefix` on `kmask` add their digit at
// `shift` to h (LDS; NHIST * 256 bins) and fold into vand / vor.
template <class U, int KIND>
__device__ inline void hist_rows(const U* __restrict__ x, uint32_t lo, uint32_t hi, U prefix, U kmask, uint32_t shift, uint32_t* h, U& vand, U& vor) {
    sweep_rows<U>(x, lo, hi, [&](U raw, uint32_t, bool live) {
        const U im = image_of<U, KIND>(raw);
        const bool m = live && ((U)(im ^ prefix) & kmask) == 0;
        hist_add(h, (uint32_t)(im >> shift) & 255u, m);
        if constexpr (NHIST<U> == 2) { if (kmask == 0) hist_add(h + 256, (uint32_t)im & 255u, m); }
        vand &= m ? im : (U)~U(0);
        vor |= m ? im : U(0);
    });
}
// vand / vor of the lanes -> the workgroup's (LDS)
template <class U> __device__ inline void fold_and_or(U vand, U vor, unsigned long long* s_and, unsigned long long* s_or) {
    vand = wave_reduce(vand, OpAnd{});
    vor = wave_reduce(vor, OpOr{});
    if (lane_id() == 0) { atomicAnd(s_and, (unsigned long long)vand); atomicOr(s_or, (unsigned long long)vor); }
}
// One digit pass of the workgroup that owns rows [lo, hi): the histograms of st's candidates -> h (LDS), their AND / OR -> st.vand / vor
template <class U, int KIND>
__device__ inline void group_pass(const U* __restrict__ x, uint32_t lo, uint32_t hi, SelState& st, uint32_t* h, unsigned long long* s_and, unsigned long long* s_or) {
    __syncthreads();
    for (uint32_t j = 0; j < NHIST<U>; ++j) h[j * 256 + threadIdx.x] = 0;
    if (threadIdx.x == 0) { *s_and = ~0ull; *s_or = 0ull; }
    __syncthreads();
    U vand = (U)~U(0), vor = 0;
    hist_rows<U, KIND>(x, lo, hi, (U)st.prefix, (U)st.kmask, st.shift, h, vand, vor);
    fold_and_or(vand, vor, s_and, s_or);
    __syncthreads();
    ++st.passes;
    st.vand = *s_and; st.vor = *s_or;
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

// The step after a histogram pass, from this lane's bin counts of the pass's histograms (c: the digit at st.shift; c2: the lower digit of
// a 2-byte column's first pass, else c again) and st.vand / vor of its candidates.  Every lane of the workgroup calls it with the same
// st.  true: the selection is over, st.prefix is the image and st.k the rank among the rows equal to it.
template <class U> __device__ inline bool digit_step(SelState& st, uint32_t c, uint32_t c2, uint32_t* wsum, BinSel* sel) {
    if (st.vand == st.vor) { st.prefix = st.vand; return true; }               // one candidate, or all of them equal
    choose_bin(c, st.k, wsum, sel);
    if (both_digits_known<U>(st, sel->cnt, sel->total)) {
        __syncthreads();
        choose_bin(c2, st.k, wsum, sel);
        st.prefix = (st.vand & ~0xFFull) | sel->bin;
        st.k -= sel->excl;
        return true;
    }
    return sel_advance(st, sel->bin, sel->excl, sel->cnt, sel->total);
}

// ---- routing: one lane per group ------------------------------------------------------------------------------------------------------------
// SMALL group g (rows from lo) -> tile_first of the tile it starts in, when it can be the first SMALL group that starts there: only a
// group whose predecessor starts in another tile, or is not SMALL, can be it
__device__ inline void small_tile_mark(const uint32_t* __restrict__ off, uint32_t g, uint32_t lo, uint32_t small_max, uint32_t* __restrict__ tile_first) {
    bool first = g == 0;
    if (!first) { const uint32_t plo = off[g - 1], pc = lo - plo; first = plo / TILE != lo / TILE || pc > small_max || pc == 0; }
    if (first) atomicMin(&tile_first[lo / TILE], g);
}
// The body of a family's classify kernel: SMALL groups mark the first of them that starts in each tile (tile_first), GROUP groups go to
// glist, and a SPLIT group takes the next number s of the split list and init_split(g, lo, hi, c, s) writes its state(s).
template <class F>
__device__ inline void classify_groups(const uint32_t* __restrict__ off, uint32_t G, uint32_t small_max, uint32_t split_min, uint32_t* __restrict__ tile_first,
                                       uint32_t* __restrict__ glist, uint32_t* __restrict__ ctl, F&& init_split) {
    uint32_t mask = 0;
    for (uint32_t g = blockIdx.x * SB + threadIdx.x; g < G; g += gridDim.x * SB) {
        const uint32_t lo = off[g], hi = off[g + 1], c = hi - lo;
        if (c == 0) continue;
        if (c <= small_max) {
            mask |= ROUTE_SMALL;
            small_tile_mark(off, g, lo, small_max, tile_first);
        } else if (c < split_min) {
            mask |= ROUTE_GROUP;
            glist[atomicAdd(&ctl[CTL_NGROUP], 1u)] = g;
        } else {
            mask |= ROUTE_SPLIT;
            init_split(g, lo, hi, c, atomicAdd(&ctl[CTL_NSPLIT], 1u));
        }
    }
    mask = wave_reduce(mask, OpOr{});
    if (lane_id() == 0 && mask) {
        atomicOr(&ctl[CTL_ROUTES], mask);
        if (mask & ROUTE_SMALL) atomicMax(&ctl[CTL_PASSES], 1u);       // ranking by comparison: one pass over the group
    }
}

// ---- SMALL ----------------------------------------------------------------------------------------------------------------------------------
// The body of a family's SMALL kernel, for the workgroup of one tile of flat positions.  What a family writes:
//   pair(g, lo, c, a_first)        group g has c = 1 or 2 rows (a lane each, from the column itself); a_first: x[lo] is its first row in order
//   ranks(c) -> r                  once per group of 3 .. small_max rows: what its rows' ranks are compared with
//   ranked(g, lo, r, ii, less)     row lo + ii of such a group has rank `less` (rows that sort before it, ties by position)
//   whole(g, lo, c, im)            (optional; rank.hip) takes the place of ranks / ranked: a wavefront gets the c staged images im[0 .. c) of such
//                                  a group and does its own counting (ties, distinct values)
template <class U, int KIND, class P, class K, class R, class W = std::nullptr_t>
__device__ inline void small_tile(const U* __restrict__ x, uint32_t n, const uint32_t* __restrict__ off, uint32_t G, const uint32_t* __restrict__ tile_first, uint32_t small_max,
                                  P&& pair, K&& ranks, R&& ranked, W&& whole = nullptr) {
    constexpr uint32_t V = 16 / sizeof(U), ROWS = TILE + SMALL_CAP, PER = (ROWS / V + SB - 1) / SB;
    __shared__ U img[ROWS];
    __shared__ uint32_t goff[TILE + 2];
    __shared__ uint32_t s_ng;
    const uint32_t g0 = tile_first[blockIdx.x];
    if (g0 == 0xFFFFFFFFu) return;
    const uint32_t tbeg = blockIdx.x * TILE, tend = n - tbeg < TILE ? n : tbeg + TILE;
    if (threadIdx.x == 0) s_ng = 0xFFFFFFFFu;
    __syncthreads();
    // offsets of the groups that start in this tile, and the end of the last one
    for (uint32_t base = 0;; base += SB) {
        const uint32_t i = base + threadIdx.x, gi = g0 + i < G ? g0 + i : G;
        const uint32_t o = off[gi];
        if (i < TILE + 2) goff[i] = o;
        const bool beyond = o >= tend || gi == G;
        if (beyond) atomicMin(&s_ng, i);
        if (__syncthreads_or(beyond)) break;
    }
    const uint32_t ng = s_ng;
    bool any = false;
    for (uint32_t gi = threadIdx.x; gi < ng; gi += SB) {
        const uint32_t lo = goff[gi], c = goff[gi + 1] - lo;
        if (c > small_max || c == 0) continue;
        if (c <= 2) pair(g0 + gi, lo, c, c == 1 || !(image_of<U, KIND>(x[lo + 1]) < image_of<U, KIND>(x[lo])));
        else any = true;
    }
    if (!__syncthreads_or(any)) return;
    // images of rows [tbeg, tbeg + ROWS) -> LDS
    const uint32_t L = n - tbeg < ROWS ? n - tbeg : ROWS;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0 && L >= V) {
        const uint32_t nvec = L / V;
        const vec16<U>* xv = reinterpret_cast<const vec16<U>*>(x + tbeg);
        vec16<U> r[PER];
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u) { const uint32_t vi = u * SB + threadIdx.x; r[u] = xv[vi < nvec ? vi : nvec - 1]; }
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u) {
            const uint32_t vi = u * SB + threadIdx.x;
            if (vi < nvec) {
#pragma unroll
                for (uint32_t e = 0; e < V; ++e) img[vi * V + e] = image_of<U, KIND>(r[u].v[e]);
            }
        }
        for (uint32_t i = nvec * V + threadIdx.x; i < L; i += SB) img[i] = image_of<U, KIND>(x[tbeg + i]);
    } else {
#pragma unroll 4
        for (uint32_t i = threadIdx.x; i < L; i += SB) img[i] = image_of<U, KIND>(x[tbeg + i]);
    }
    __syncthreads();
    // a wavefront per group: rank of every row = rows that sort before it (ties by position)
    const uint32_t lane = lane_id();
    for (uint32_t gi = wave_id(); gi < ng; gi += NWV) {
        const uint32_t lo = goff[gi], c = goff[gi + 1] - lo;
        if (c < 3 || c > small_max) continue;
        const uint32_t base = lo - tbeg;
        if constexpr (!std::is_same_v<std::decay_t<W>, std::nullptr_t>) { whole(g0 + gi, lo, c, &img[base]); continue; }
        const auto r = ranks(c);
        for (uint32_t eb = 0; eb < c; eb += 64) {
            const bool live = eb + lane < c;
            const uint32_t ii = live ? eb + lane : c - 1;
            const U mine = img[base + ii];
            uint32_t less = 0;
#pragma unroll 4
            for (uint32_t j = 0; j < c; ++j) {
                const U v = img[base + j];
                less += (v < mine) | ((v == mine) & (j < ii));
            }
            if (live) ranked(g0 + gi, lo, r, ii, less);
        }
    }
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
} // namespace selradix
