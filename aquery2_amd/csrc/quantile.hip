// quantile.hip -- aqg_quantiles / aqg_grouped_quantiles(_flat): up to AQG_QUANTILES_MAX ranks of a column and of every group's slice of
// the flat layout, in ONE radix selection (select.hip's header comment describes the selection of one rank; include/aqg.h, quantiles
// section, the contract).
//
// What the ranks of a group share is the expensive part of a digit: the read of the group's rows.  The selection of a group is nq
// states (SelState), one per rank.  Two states have either chosen the same bins so far -- then they count the same candidates and only
// their ranks differ -- or different ones, and then no row is a candidate of both.  So between digits the live states of a group fall
// into at most nq LEADERS (QLive: distinct (prefix, kmask, shift)), a row matches at most one leader, and one pass over the slice fills
// one histogram per leader in LDS with one LDS atomic per row.  After the pass every live state takes its bin from its leader's
// histogram with its own rank (choose_bin) and advances (sel_advance) with every shortcut of the single selection: all candidates equal,
// bit skipping, both digits of a 2-byte column in the first pass.  The first digit has one leader whatever nq is.
// Routes, thresholds and the classify step are the median's:
//   SMALL  comparison counting in LDS: the lane whose row's count equals rank j writes out[g * nq + j]; one pass whatever nq is
//   GROUP  one workgroup per group, nq x NHIST x 256 bins in LDS, states and leaders in LDS
//   SPLIT  chunked: states (plane q of the state array: sst[q * scap + s]) and leaders in HBM; per digit one histogram launch for the
//          groups with one leader, one for the groups with several (none in the first digit) and one choose launch; the chunk plan and
//          split_span read plane 0
#include "groupby_handle.hpp"
#include "select_radix.hpp"

namespace {
using namespace selradix;

constexpr uint32_t QMAX = AQG_QUANTILES_MAX;
enum { QCTL_RESULT = 16 /* QMAX * 8 bytes behind the control words of select_radix.hpp */ };
template <class U> constexpr uint32_t HSTRIDE = 256 * NHIST<U>;           // bins of one leader

struct QArgs { uint32_t nq, den, which, num[QMAX]; };
// rank of quantile num / den among c >= 1 rows: floor resp. ceil of num (c - 1) / den
__device__ inline uint32_t quantile_rank(const QArgs& a, uint32_t j, uint32_t c) {
    const uint64_t p = (uint64_t)a.num[j] * (c - 1);
    return (uint32_t)(p / a.den + (a.which && p % a.den != 0 ? 1u : 0u));
}
// the distinct candidate sets of a group's live states between digits
struct QLive {
    uint64_t prefix[QMAX], kmask[QMAX];
    uint64_t vand[QMAX], vor[QMAX];       // AND / OR of the images of the leader's candidates in the last pass
    uint32_t shift[QMAX];
    uint32_t lead[QMAX];                  // the leader state j counts with
    uint32_t nl, pad[3];                  // leaders; 0: every state of the group is done
};
__device__ inline void live_init(QLive* lv, uint32_t bits) {
    for (uint32_t q = 0; q < QMAX; ++q) { lv->prefix[q] = lv->kmask[q] = 0; lv->vand[q] = ~0ull; lv->vor[q] = 0; lv->shift[q] = bits - 8; lv->lead[q] = 0; }
    lv->nl = 1;
}
__device__ inline uint64_t uniform64(uint64_t v) {
    return (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)v) | (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32;
}

// ---- routing: one lane per group (select.hip's classify, with nq states per SPLIT group) -------------------------------------------------
__global__ void __launch_bounds__(SB) quant_classify_kernel(const uint32_t* __restrict__ off, uint32_t G, uint32_t small_max, uint32_t split_min, QArgs qa, int bits, uint32_t scap,
                                                             uint32_t* __restrict__ tile_first, uint32_t* __restrict__ glist, SelState* __restrict__ sst, QLive* __restrict__ slive,
                                                             uint32_t* __restrict__ ctl) {
    uint32_t mask = 0;
    for (uint32_t g = blockIdx.x * SB + threadIdx.x; g < G; g += gridDim.x * SB) {
        const uint32_t lo = off[g], hi = off[g + 1], c = hi - lo;
        if (c == 0) continue;
        if (c <= small_max) {
            mask |= ROUTE_SMALL;
            bool first = g == 0;
            if (!first) { const uint32_t plo = off[g - 1], pc = lo - plo; first = plo / TILE != lo / TILE || pc > small_max || pc == 0; }
            if (first) atomicMin(&tile_first[lo / TILE], g);
        } else if (c < split_min) {
            mask |= ROUTE_GROUP;
            glist[atomicAdd(&ctl[CTL_NGROUP], 1u)] = g;
        } else {
            mask |= ROUTE_SPLIT;
            const uint32_t s = atomicAdd(&ctl[CTL_NSPLIT], 1u);
            for (uint32_t q = 0; q < qa.nq; ++q) {
                SelState st{};
                st.vand = ~0ull;
                st.lo = lo; st.hi = hi; st.k = quantile_rank(qa, q, c); st.gidx = g;
                st.shift = (uint32_t)bits - 8;
                sst[(size_t)q * scap + s] = st;
            }
            live_init(&slive[s], (uint32_t)bits);
        }
    }
    mask = wave_reduce(mask, OpOr{});
    if (lane_id() == 0 && mask) {
        atomicOr(&ctl[CTL_ROUTES], mask);
        if (mask & ROUTE_SMALL) atomicMax(&ctl[CTL_PASSES], 1u);
    }
}

// ---- SMALL ----------------------------------------------------------------------------------------------------------------------------------
template <class U, int KIND>
__global__ void __launch_bounds__(SB) quant_small_kernel(const U* __restrict__ x, uint32_t n, const uint32_t* __restrict__ off, uint32_t G,
                                                          const uint32_t* __restrict__ tile_first, uint32_t small_max, QArgs qa, U* __restrict__ out) {
    constexpr uint32_t V = 16 / sizeof(U), ROWS = TILE + SMALL_CAP, PER = (ROWS / V + SB - 1) / SB;
    __shared__ U img[ROWS];
    __shared__ uint32_t goff[TILE + 2];
    __shared__ uint32_t s_ng;
    const uint32_t g0 = tile_first[blockIdx.x];
    if (g0 == 0xFFFFFFFFu) return;
    const uint32_t tbeg = blockIdx.x * TILE, tend = n - tbeg < TILE ? n : tbeg + TILE;
    const uint32_t nq = qa.nq;
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
    // one or two rows: a lane each, from the column itself
    bool any = false;
    for (uint32_t gi = threadIdx.x; gi < ng; gi += SB) {
        const uint32_t lo = goff[gi], c = goff[gi + 1] - lo;
        if (c > small_max || c == 0) continue;
        U* o = out + (size_t)(g0 + gi) * nq;
        if (c == 1) { const U a = x[lo]; for (uint32_t j = 0; j < nq; ++j) o[j] = a; }
        else if (c == 2) {
            U a = x[lo], b = x[lo + 1];
            if (image_of<U, KIND>(b) < image_of<U, KIND>(a)) { const U t = a; a = b; b = t; }
            for (uint32_t j = 0; j < nq; ++j) o[j] = quantile_rank(qa, j, 2) ? b : a;
        } else any = true;
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
    // a wavefront per group: rank of every row = rows that sort before it (ties by position); the row whose rank is quantile j's answers it
    const uint32_t lane = lane_id();
    for (uint32_t gi = wave_id(); gi < ng; gi += NWV) {
        const uint32_t lo = goff[gi], c = goff[gi + 1] - lo;
        if (c < 3 || c > small_max) continue;
        const uint32_t base = lo - tbeg;
        uint32_t k[QMAX];
#pragma unroll
        for (uint32_t j = 0; j < QMAX; ++j) k[j] = j < nq ? quantile_rank(qa, j, c) : 0xFFFFFFFFu;
        U* o = out + (size_t)(g0 + gi) * nq;
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
            if (live) {
                const U raw = x[lo + ii];
#pragma unroll
                for (uint32_t j = 0; j < QMAX; ++j)
                    if (less == k[j]) o[j] = raw;
            }
        }
    }
}

// ---- the multi-prefix pass --------------------------------------------------------------------------------------------------------------------
// hist_rows (select_radix.hpp) for the nl leaders of lv: a row whose image matches leader q adds its digit at shift[q] to h + q * HSTRIDE
// (LDS) and folds into vand[q] / vor[q].  The same load shape: 16-byte loads over the aligned middle, UNR in flight per lane, the up to
// 2 (V - 1) elements in front of and behind it one lane each.
// NLT: the compile-time bound of nl (1, 2, 4 or QMAX), so that one leader costs what hist_rows costs.
template <class U, int KIND, uint32_t NLT, uint32_t NA>
__device__ __forceinline__ void hist_rows_nl(const U* __restrict__ x, uint32_t lo, uint32_t hi, const QLive* lv, uint32_t nl, uint32_t* h, U (&vand)[NA], U (&vor)[NA]) {
    static_assert(NLT <= NA, "one vand / vor per leader");
    constexpr uint32_t V = 16 / sizeof(U);
    U P[NLT], M[NLT];
    uint32_t S[NLT];
#pragma unroll
    for (uint32_t q = 0; q < NLT; ++q) {
        const uint32_t qq = q < nl ? q : 0u;
        P[q] = (U)uniform64(lv->prefix[qq]); M[q] = (U)uniform64(lv->kmask[qq]); S[q] = __builtin_amdgcn_readfirstlane(lv->shift[qq]);
    }
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(x + lo) & 15);
    uint32_t hl = mis ? (16 - mis) / (uint32_t)sizeof(U) : 0u;
    if (hl > hi - lo) hl = hi - lo;
    const uint32_t a0 = lo + hl, nvec = (hi - a0) / V, ts = a0 + nvec * V, tl = hi - ts;
    auto row = [&](U raw, bool live) {
        const U im = image_of<U, KIND>(raw);
        uint32_t slot = 0;
        bool m = false;
#pragma unroll
        for (uint32_t q = 0; q < NLT; ++q) {
            if (NLT == 1 || q < nl) {                       // (uniform)
                const bool mq = live && ((U)(im ^ P[q]) & M[q]) == 0;
                slot = mq ? q * HSTRIDE<U> + ((uint32_t)(im >> S[q]) & 255u) : slot;
                m |= mq;
                vand[q] &= mq ? im : (U)~U(0);
                vor[q] |= mq ? im : U(0);
            }
        }
        hist_add(h, slot, m);
        if constexpr (NHIST<U> == 2) { if (M[0] == 0) hist_add(h + 256, (uint32_t)im & 255u, m); }     // (the first pass: one leader)
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
// NA == 1: the caller has one leader (the first digit of every group; nq == 1); NA == QMAX: any number
template <class U, int KIND, uint32_t NA>
__device__ __forceinline__ void hist_rows_multi(const U* __restrict__ x, uint32_t lo, uint32_t hi, const QLive* lv, uint32_t nl, uint32_t* h, U (&vand)[NA], U (&vor)[NA]) {
    if constexpr (NA == 1) hist_rows_nl<U, KIND, 1>(x, lo, hi, lv, nl, h, vand, vor);
    else if (nl == 1) hist_rows_nl<U, KIND, 1>(x, lo, hi, lv, nl, h, vand, vor);
    else if (nl == 2) hist_rows_nl<U, KIND, 2>(x, lo, hi, lv, nl, h, vand, vor);
    else if (nl <= 4) hist_rows_nl<U, KIND, 4>(x, lo, hi, lv, nl, h, vand, vor);
    else hist_rows_nl<U, KIND, QMAX>(x, lo, hi, lv, nl, h, vand, vor);
}
// after a pass: every live state of a group (sts[j * stride], j < nq) takes its bin from its leader's histogram (hist + lead * HSTRIDE)
// and advances; finished ones write out[j] unless their image is shared (done = 2: looked up by the caller).  Then the leaders of the
// states still live are rebuilt in lv.  Every lane of the workgroup calls it; the histograms and lv->vand / vor are complete on entry.
// Returns the number of leaders left.
template <class U, int KIND>
__device__ inline uint32_t quant_advance(SelState* sts, size_t stride, uint32_t nq, QLive* lv, const uint32_t* hist, uint32_t* wsum, BinSel* sel, U* out, uint32_t* passes) {
    for (uint32_t j = 0; j < nq; ++j) {
        SelState st = sts[j * stride];
        if (st.done) continue;                              // (uniform)
        const uint32_t l = lv->lead[j];
        const uint32_t* hl = hist + l * HSTRIDE<U>;
        ++st.passes;
        st.vand = lv->vand[l]; st.vor = lv->vor[l];
        bool done;
        if (st.vand == st.vor) { st.prefix = st.vand; done = true; }       // one candidate, or all of them equal
        else {
            choose_bin(hl[threadIdx.x], st.k, wsum, sel);
            if (both_digits_known<U>(st, sel->cnt, sel->total)) {
                __syncthreads();
                choose_bin(hl[256 * (NHIST<U> - 1) + threadIdx.x], st.k, wsum, sel);
                st.prefix = (st.vand & ~0xFFull) | sel->bin;
                done = true;
            } else done = sel_advance(st, sel->bin, sel->excl, sel->cnt, sel->total);
        }
        __syncthreads();                                    // (every lane has read the state and sel)
        if (threadIdx.x == 0) {
            if (done) {
                const U result = (U)st.prefix;
                st.done = image_is_shared<U, KIND>(result) ? 2u : 1u;
                if (st.done == 1) out[j] = value_of<U, KIND>(result);
                *passes = st.passes > *passes ? st.passes : *passes;
            }
            sts[j * stride] = st;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t nl = 0;
        for (uint32_t j = 0; j < nq; ++j) {
            const SelState& st = sts[j * stride];
            if (st.done) continue;
            uint32_t l = 0;
            while (l < nl && !(lv->prefix[l] == st.prefix && lv->kmask[l] == st.kmask && lv->shift[l] == st.shift)) ++l;
            if (l == nl) { lv->prefix[l] = st.prefix; lv->kmask[l] = st.kmask; lv->shift[l] = st.shift; ++nl; }
            lv->lead[j] = l;
        }
        for (uint32_t l = 0; l < QMAX; ++l) { lv->vand[l] = ~0ull; lv->vor[l] = 0ull; }
        lv->nl = nl;
    }
    __syncthreads();
    return lv->nl;
}

// ---- GROUP ----------------------------------------------------------------------------------------------------------------------------------
template <class U, int KIND>
__global__ void __launch_bounds__(SB) quant_group_kernel(const U* __restrict__ x, const uint32_t* __restrict__ off, const uint32_t* __restrict__ glist,
                                                          uint32_t* __restrict__ ctl, QArgs qa, U* __restrict__ out) {
    __shared__ uint32_t h[QMAX * HSTRIDE<U>];
    __shared__ uint32_t wsum[NWV];
    __shared__ SelState sts[QMAX];
    __shared__ QLive lv;
    __shared__ BinSel sel;
    __shared__ uint32_t s_passes;
    const uint32_t ngl = ctl[CTL_NGROUP], nq = qa.nq;
    if (threadIdx.x == 0) s_passes = 0;
    for (uint32_t li = blockIdx.x; li < ngl; li += gridDim.x) {
        const uint32_t g = glist[li], lo = off[g], hi = off[g + 1], c = hi - lo;
        __syncthreads();
        if (threadIdx.x < nq) {
            SelState st{};
            st.k = quantile_rank(qa, threadIdx.x, c);
            st.shift = sizeof(U) * 8 - 8;
            sts[threadIdx.x] = st;
        }
        if (threadIdx.x == 0) live_init(&lv, sizeof(U) * 8);
        __syncthreads();
        uint32_t nl = 1;
        while (nl) {
            for (uint32_t i = threadIdx.x; i < nl * HSTRIDE<U>; i += SB) h[i] = 0;
            __syncthreads();
            U vand[QMAX], vor[QMAX];
#pragma unroll
            for (uint32_t q = 0; q < QMAX; ++q) { vand[q] = (U)~U(0); vor[q] = 0; }
            hist_rows_multi<U, KIND, QMAX>(x, lo, hi, &lv, nl, h, vand, vor);
#pragma unroll
            for (uint32_t q = 0; q < QMAX; ++q)
                if (q < nl) fold_and_or(vand[q], vor[q], (unsigned long long*)&lv.vand[q], (unsigned long long*)&lv.vor[q]);
            __syncthreads();
            nl = quant_advance<U, KIND>(sts, 1, nq, &lv, h, wsum, &sel, out + (size_t)g * nq, &s_passes);
        }
        if constexpr (KIND == KIND_FP) {
            for (uint32_t j = 0; j < nq; ++j)
                if (sts[j].done == 2) find_rows<U, KIND>(x, lo, hi, (U)sts[j].prefix, out + (size_t)g * nq + j);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_passes) atomicMax(&ctl[CTL_PASSES], s_passes);
}

// ---- SPLIT ----------------------------------------------------------------------------------------------------------------------------------
// select_split_hist_kernel for the leaders of every split group: the histograms of this workgroup's span of chunks in LDS, merged into
// ghist[(s * nq + l) * HSTRIDE ...] and slive[s].vand / vor once per group.  Two instantiations share a digit: NA == 1 takes the groups
// with one leader (every group in the first digit, and whenever the ranks still agree) at the cost of select_split_hist_kernel, NA ==
// QMAX takes the groups with several; each skips the other's groups without a look at their rows.
template <class U, int KIND, uint32_t NA>
__global__ void __launch_bounds__(SB) quant_split_hist_kernel(const U* __restrict__ x, const SelState* __restrict__ sst, QLive* slive, const uint32_t* __restrict__ ctl,
                                                               uint32_t nq, uint32_t* __restrict__ ghist) {
    __shared__ uint32_t h[NA * HSTRIDE<U>];
    __shared__ unsigned long long s_and[NA], s_or[NA];
    uint32_t q0, q1, s, ns;
    if (!split_span(sst, ctl, q0, q1, s, ns)) return;
    for (uint32_t i = threadIdx.x; i < NA * HSTRIDE<U>; i += SB) h[i] = 0;
    if (threadIdx.x < NA) { s_and[threadIdx.x] = ~0ull; s_or[threadIdx.x] = 0ull; }
    __syncthreads();
    U vand[NA], vor[NA];
#pragma unroll
    for (uint32_t q = 0; q < NA; ++q) { vand[q] = (U)~U(0); vor[q] = 0; }
    uint32_t nl = 0;                                        // leaders of group s, once one of its chunks has been counted
    auto flush = [&]() {                                    // this workgroup's share of group s -> HBM
        if (nl) {
#pragma unroll
            for (uint32_t q = 0; q < NA; ++q)
                if (q < nl) fold_and_or(vand[q], vor[q], &s_and[q], &s_or[q]);
            __syncthreads();
            uint32_t* gh = ghist + (size_t)s * nq * HSTRIDE<U>;
            for (uint32_t i = threadIdx.x; i < nl * HSTRIDE<U>; i += SB)
                if (h[i]) atomicAdd(&gh[i], h[i]);
            if (threadIdx.x < nl) { atomicAnd((unsigned long long*)&slive[s].vand[threadIdx.x], s_and[threadIdx.x]); atomicOr((unsigned long long*)&slive[s].vor[threadIdx.x], s_or[threadIdx.x]); }
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < nl * HSTRIDE<U>; i += SB) h[i] = 0;
            if (threadIdx.x < NA) { s_and[threadIdx.x] = ~0ull; s_or[threadIdx.x] = 0ull; }
            __syncthreads();
        }
#pragma unroll
        for (uint32_t q = 0; q < NA; ++q) { vand[q] = (U)~U(0); vor[q] = 0; }
        nl = 0;
    };
    // of group s: its leaders if they are this instantiation's (else 0), its rows, and the first chunk of the next group
    uint32_t gl, glo, ghi, gcb, next;
    auto enter = [&]() {
        gl = slive[s].nl;
        if ((NA == 1) != (gl == 1)) gl = 0;
        glo = sst[s].lo; ghi = sst[s].hi; gcb = sst[s].cbase;
        next = s + 1 < ns ? sst[s + 1].cbase : 0xFFFFFFFFu;
    };
    enter();
    for (uint32_t q = q0; q < q1; ++q) {
        while (next <= q) { flush(); ++s; enter(); }
        if (gl == 0) continue;
        const uint32_t lo = glo + (q - gcb) * SPLIT_CHUNK;
        const uint32_t hi = ghi - lo < SPLIT_CHUNK ? ghi : lo + SPLIT_CHUNK;
        hist_rows_multi<U, KIND, NA>(x, lo, hi, &slive[s], gl, h, vand, vor);
        nl = gl;
    }
    flush();
}
template <class U, int KIND>
__global__ void __launch_bounds__(SB) quant_split_choose_kernel(SelState* __restrict__ sst, QLive* __restrict__ slive, uint32_t* __restrict__ ctl, uint32_t nq, uint32_t scap,
                                                                 uint32_t* __restrict__ ghist, U* __restrict__ out) {
    __shared__ uint32_t wsum[NWV];
    __shared__ BinSel sel;
    __shared__ uint32_t s_passes;
    const uint32_t ns = ctl[CTL_NSPLIT];
    if (threadIdx.x == 0) s_passes = 0;
    __syncthreads();
    for (uint32_t s = blockIdx.x; s < ns; s += gridDim.x) {
        const uint32_t nl = slive[s].nl;
        __syncthreads();                                    // (every lane has read nl before lane 0 rewrites it)
        if (nl == 0) continue;
        uint32_t* gh = ghist + (size_t)s * nq * HSTRIDE<U>;
        quant_advance<U, KIND>(sst + s, scap, nq, &slive[s], gh, wsum, &sel, out + (size_t)sst[s].gidx * nq, &s_passes);
        for (uint32_t i = threadIdx.x; i < nl * HSTRIDE<U>; i += SB) gh[i] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_passes) atomicMax(&ctl[CTL_PASSES], s_passes);
}
// finished states whose image is shared by several bit patterns: any element of the slice with that image
template <class U, int KIND>
__global__ void __launch_bounds__(SB) quant_split_find_kernel(const U* __restrict__ x, const SelState* __restrict__ sst, const uint32_t* __restrict__ ctl, uint32_t nq, uint32_t scap,
                                                               U* __restrict__ out) {
    uint32_t q0, q1, s, ns;
    if (!split_span(sst, ctl, q0, q1, s, ns)) return;
    uint32_t shared, glo, ghi, gcb, gidx, next;            // of group s: a bit per state to look up, its rows, the next group's first chunk
    auto enter = [&]() {
        shared = 0;
        for (uint32_t j = 0; j < nq; ++j) shared |= (sst[(size_t)j * scap + s].done == 2 ? 1u : 0u) << j;
        glo = sst[s].lo; ghi = sst[s].hi; gcb = sst[s].cbase; gidx = sst[s].gidx;
        next = s + 1 < ns ? sst[s + 1].cbase : 0xFFFFFFFFu;
    };
    enter();
    for (uint32_t q = q0; q < q1; ++q) {
        while (next <= q) { ++s; enter(); }
        if (!shared) continue;
        const uint32_t lo = glo + (q - gcb) * SPLIT_CHUNK;
        const uint32_t hi = ghi - lo < SPLIT_CHUNK ? ghi : lo + SPLIT_CHUNK;
        for (uint32_t j = 0; j < nq; ++j)
            if (shared >> j & 1) find_rows<U, KIND>(x, lo, hi, (U)sst[(size_t)j * scap + s].prefix, out + (size_t)gidx * nq + j);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
// select_ws_bytes for nq states and histograms per split group, and its leaders
size_t quant_ws_bytes(uint32_t n, uint32_t G, uint32_t nq, SelSwitches sw) {
    return select_ws_bytes(n, G, sw) + (size_t)split_cap(n, G, sw.split_min) * ((size_t)nq * (sizeof(SelState) + 2048) + sizeof(QLive)) + 1024;
}
template <class U, int KIND>
int run_quant(aqg_ctx* ctx, const QArgs& qa, const void* xv, uint32_t n, const uint32_t* off, uint32_t G, SelSwitches sw, void* outv) {
    const U* x = static_cast<const U*>(xv);
    U* out = static_cast<U*>(outv);
    uint32_t* ctl = ctx->select_ctl;
    const uint32_t nq = qa.nq, ntiles = aqg_ceil_div(n, TILE), scap = split_cap(n, G, sw.split_min);
    const uint32_t glcap = (n / (sw.small_max + 1) < G ? n / (sw.small_max + 1) : G) + 1;
    // routes no group of this call can take are not launched (as run_select)
    const bool do_small = sw.small_max >= 1, do_group = n > sw.small_max && sw.split_min > sw.small_max + 1, do_split = n >= sw.split_min && n > sw.small_max;
    uint32_t *tile_first, *glist, *ghist;
    SelState* sst;
    QLive* slive;
    AQG_TRY(aqg_ws_get(ctx, (size_t)ntiles + 1, &tile_first));
    AQG_TRY(aqg_ws_get(ctx, glcap, &glist));
    AQG_TRY(aqg_ws_get(ctx, (size_t)scap * nq, &sst));
    AQG_TRY(aqg_ws_get(ctx, scap, &slive));
    AQG_TRY(aqg_ws_get(ctx, (size_t)scap * nq * HSTRIDE<U>, &ghist));
    if (do_small) AQG_HIP(ctx, hipMemsetAsync(tile_first, 0xFF, (size_t)ntiles * 4, ctx->stream));
    if (do_split) AQG_HIP(ctx, hipMemsetAsync(ghist, 0, (size_t)scap * nq * HSTRIDE<U> * 4, ctx->stream));
    const unsigned ggrid = aqg_grid(ctx, G, SB, 1, 8);
    hipLaunchKernelGGL(quant_classify_kernel, dim3(ggrid), dim3(SB), 0, ctx->stream, off, G, sw.small_max, sw.split_min, qa, (int)sizeof(U) * 8, scap, tile_first, glist, sst, slive, ctl);
    aqg_kernel_timer_begin(ctx);
    if (do_small) hipLaunchKernelGGL((quant_small_kernel<U, KIND>), dim3(ntiles), dim3(SB), 0, ctx->stream, x, n, off, G, tile_first, sw.small_max, qa, out);
    if (do_group) {
        const uint32_t cap = (uint32_t)ctx->num_cu * 8;
        hipLaunchKernelGGL((quant_group_kernel<U, KIND>), dim3(glcap < cap ? glcap : cap), dim3(SB), 0, ctx->stream, x, off, glist, ctl, qa, out);
    }
    if (do_split) {
        const uint64_t chunks = (uint64_t)aqg_ceil_div(n, SPLIT_CHUNK) + scap;
        const unsigned hgrid = (unsigned)(chunks < (uint64_t)ctx->num_cu * 8 ? chunks : (uint64_t)ctx->num_cu * 8);
        const unsigned cgrid = scap < 1024u ? scap : 1024u;
        hipLaunchKernelGGL(select_split_plan_kernel, dim3(1), dim3(SB), 0, ctx->stream, sst, ctl);
        for (size_t p = 0; p < sizeof(U); ++p) {
            hipLaunchKernelGGL((quant_split_hist_kernel<U, KIND, 1>), dim3(hgrid), dim3(SB), 0, ctx->stream, x, sst, slive, ctl, nq, ghist);
            if (p) hipLaunchKernelGGL((quant_split_hist_kernel<U, KIND, QMAX>), dim3(hgrid), dim3(SB), 0, ctx->stream, x, sst, slive, ctl, nq, ghist);
            hipLaunchKernelGGL((quant_split_choose_kernel<U, KIND>), dim3(cgrid), dim3(SB), 0, ctx->stream, sst, slive, ctl, nq, scap, ghist, out);
        }
        if constexpr (KIND == KIND_FP) hipLaunchKernelGGL((quant_split_find_kernel<U, KIND>), dim3(hgrid), dim3(SB), 0, ctx->stream, x, sst, ctl, nq, scap, out);
    }
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "quantile selection");
}
int dispatch_quant(aqg_ctx* ctx, const QArgs& qa, int t, const void* x, uint32_t n, const uint32_t* off, uint32_t G, SelSwitches sw, void* out) {
    switch (t) {
    case AQG_UINT8: case AQG_BOOL: return run_quant<uint8_t, KIND_UNSIGNED>(ctx, qa, x, n, off, G, sw, out);
    case AQG_UINT16: return run_quant<uint16_t, KIND_UNSIGNED>(ctx, qa, x, n, off, G, sw, out);
    case AQG_UINT32: return run_quant<uint32_t, KIND_UNSIGNED>(ctx, qa, x, n, off, G, sw, out);
    case AQG_UINT64: return run_quant<uint64_t, KIND_UNSIGNED>(ctx, qa, x, n, off, G, sw, out);
    case AQG_INT8: return run_quant<uint8_t, KIND_SIGNED>(ctx, qa, x, n, off, G, sw, out);
    case AQG_INT16: return run_quant<uint16_t, KIND_SIGNED>(ctx, qa, x, n, off, G, sw, out);
    case AQG_INT32: return run_quant<uint32_t, KIND_SIGNED>(ctx, qa, x, n, off, G, sw, out);
    case AQG_INT64: return run_quant<uint64_t, KIND_SIGNED>(ctx, qa, x, n, off, G, sw, out);
    case AQG_FLOAT: return run_quant<uint32_t, KIND_FP>(ctx, qa, x, n, off, G, sw, out);
    case AQG_DOUBLE: return run_quant<uint64_t, KIND_FP>(ctx, qa, x, n, off, G, sw, out);
    }
    return AQG_ERR_DTYPE;
}
// the checks every entry shares; fills qa
int check_quant(aqg_ctx* ctx, int which, uint32_t nq, const uint32_t* num, uint32_t den, int t, QArgs* qa) {
    if (which != AQG_SEL_LOWER && which != AQG_SEL_UPPER) return aqg_fail(ctx, AQG_ERR_ARG, "quantiles: which must be AQG_SEL_LOWER or AQG_SEL_UPPER");
    if (nq < 1 || nq > QMAX || !num || den < 1) return aqg_fail(ctx, AQG_ERR_ARG, "quantiles: 1 <= nq <= AQG_QUANTILES_MAX ranks num[j] / den with den >= 1");
    *qa = QArgs{};
    qa->nq = nq; qa->den = den; qa->which = (uint32_t)which;
    for (uint32_t j = 0; j < nq; ++j) {
        if (num[j] > den) return aqg_fail(ctx, AQG_ERR_ARG, "quantiles: num[j] > den");
        qa->num[j] = num[j];
    }
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "quantiles: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    return AQG_OK;
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g, int which, uint32_t nq, const uint32_t* num, uint32_t den, int t, const void* x, const void* out, QArgs* qa) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped quantiles: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped quantiles: the handle was not made by aqg_groupby_build");
    AQG_TRY(check_quant(ctx, which, nq, num, den, t, qa));
    if ((!x || !out) && g->n) return aqg_fail(ctx, AQG_ERR_ARG, "grouped quantiles: null column");
    return AQG_OK;
}

} // namespace

extern "C" {

int aqg_quantiles(aqg_ctx* ctx, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, uint32_t n, void* out_host) {
    if (!ctx || !out_host) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_quantiles: bad argument");
    QArgs qa;
    AQG_TRY(check_quant(ctx, which, nq, num_host, den, t, &qa));
    if (!x && n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_quantiles: null column");
    AQG_CHECK_ROWS(ctx, n, "aqg_quantiles");
    AQG_TRY(ensure_ctl(ctx));
    const size_t bytes = (size_t)nq * esz_of(t);
    memset(out_host, 0, bytes);
    if (n == 0) return AQG_OK;
    const SelSwitches sw = select_switches();
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, quant_ws_bytes(n, 1, nq, sw)));
    uint32_t* ctl = ctx->select_ctl;
    hipLaunchKernelGGL(flat_offsets_kernel, dim3(1), dim3(1), 0, ctx->stream, ctl + CTL_OFF, n);
    AQG_TRY(dispatch_quant(ctx, qa, t, x, n, ctl + CTL_OFF, 1, sw, ctl + QCTL_RESULT));
    return aqg_d2h(ctx, out_host, ctl + QCTL_RESULT, bytes);
}

int aqg_grouped_quantiles_flat(aqg_ctx* ctx, aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* xflat, void* out_dev) {
    QArgs qa;
    AQG_TRY(check_grouped(ctx, g, which, nq, num_host, den, t, xflat, out_dev, &qa));
    AQG_TRY(ensure_ctl(ctx));
    const uint32_t n = g->n, G = g->ngroups;
    if (n == 0 || G == 0) return AQG_OK;
    const uint32_t* off = aqg_groupby_offsets(g);
    if (!off) return AQG_ERR_HIP;
    const SelSwitches sw = select_switches();
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, quant_ws_bytes(n, G, nq, sw)));
    return dispatch_quant(ctx, qa, t, xflat, n, off, G, sw, out_dev);
}

int aqg_grouped_quantiles(aqg_ctx* ctx, aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, void* out_dev) {
    QArgs qa;
    AQG_TRY(check_grouped(ctx, g, which, nq, num_host, den, t, x, out_dev, &qa));
    AQG_TRY(ensure_ctl(ctx));
    const uint32_t n = g->n, G = g->ngroups;
    if (n == 0 || G == 0) return AQG_OK;
    const uint32_t* off = aqg_groupby_offsets(g);
    if (!off) return AQG_ERR_HIP;
    const SelSwitches sw = select_switches();
    const int esz = esz_of(t);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * esz + 4096 + aqg_postproc_ws_bytes(n, G, esz) + quant_ws_bytes(n, G, nq, sw)));
    unsigned char* xs;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n * esz + 64, &xs));
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x, esz, xs, /*ws_managed=*/true));
    return dispatch_quant(ctx, qa, t, xs, n, off, G, sw, out_dev);
}

} // extern "C"
