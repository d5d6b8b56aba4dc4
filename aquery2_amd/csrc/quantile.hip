// quantile.hip -- aqg_quantiles / aqg_grouped_quantiles(_flat): up to AQG_QUANTILES_MAX ranks of a column and of every group's slice of
// the flat layout, in ONE radix selection (select.hip's header comment describes the selection of one rank; include/aqg.h, quantiles
// section, the contract).
//
// What the ranks of a group share is the expensive part of a digit: the read of the group's rows.  The selection of a group is nq
// states (SelState), one per rank.  Two states have either chosen the same bins so far -- then they count the same candidates and only
// their ranks differ -- or different ones, and then no row is a candidate of both.  So between digits the live states of a group fall
// into at most nq LEADERS (QLive: distinct (prefix, kmask, shift)), a row matches at most one leader, and one pass over the slice fills
// one histogram per leader in LDS with one LDS atomic per row.  After the pass every live state takes its bin from its leader's
// histogram with its own rank and advances (digit_step) with every shortcut of the single selection: all candidates equal,
// bit skipping, both digits of a 2-byte column in the first pass.  The first digit has one leader whatever nq is.
// Routes, thresholds and the classify step are the median's:
//   SMALL  comparison counting in LDS: the lane whose row's count equals rank j writes out[g * nq + j]; one pass whatever nq is
//   GROUP  one workgroup per group, nq x NHIST x 256 bins in LDS, states and leaders in LDS
//   SPLIT  chunked: states (plane q of the state array: sst[q * scap + s]) and leaders in HBM; per digit one histogram launch for the
//          groups with one leader, one for the groups with several (none in the first digit) and one choose launch; the chunk plan and
//          split_span read plane 0
#include "select_host.hpp"

namespace {
using namespace selradix;

enum { QCTL_RESULT = 16 /* QMAX * 8 bytes behind the control words of select_radix.hpp */ };
template <class U> constexpr uint32_t HSTRIDE = 256 * NHIST<U>;           // bins of one leader

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

// ---- routing: one lane per group (nq states per SPLIT group) ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB) quant_classify_kernel(const uint32_t* __restrict__ off, uint32_t G, uint32_t small_max, uint32_t split_min, QArgs qa, int bits, uint32_t scap,
                                                             uint32_t* __restrict__ tile_first, uint32_t* __restrict__ glist, SelState* __restrict__ sst, QLive* __restrict__ slive,
                                                             uint32_t* __restrict__ ctl) {
    classify_groups(off, G, small_max, split_min, tile_first, glist, ctl, [&](uint32_t g, uint32_t lo, uint32_t hi, uint32_t c, uint32_t s) {
        for (uint32_t q = 0; q < qa.nq; ++q) sst[(size_t)q * scap + s] = split_state(lo, hi, quantile_rank(qa, q, c), g, (uint32_t)bits);
        live_init(&slive[s], (uint32_t)bits);
    });
}

// ---- SMALL ----------------------------------------------------------------------------------------------------------------------------------
template <class U, int KIND>
__global__ void __launch_bounds__(SB) quant_small_kernel(const U* __restrict__ x, uint32_t n, const uint32_t* __restrict__ off, uint32_t G,
                                                          const uint32_t* __restrict__ tile_first, uint32_t small_max, QArgs qa, U* __restrict__ out) {
    struct Ranks { uint32_t k[QMAX]; };
    const uint32_t nq = qa.nq;
    small_tile<U, KIND>(
        x, n, off, G, tile_first, small_max,
        [&](uint32_t g, uint32_t lo, uint32_t c, bool a_first) {
            const U a = x[a_first ? lo : lo + 1], b = x[a_first ? lo + c - 1 : lo];
            for (uint32_t j = 0; j < nq; ++j) out[(size_t)g * nq + j] = quantile_rank(qa, j, c) ? b : a;
        },
        [&](uint32_t c) {
            Ranks r;
#pragma unroll
            for (uint32_t j = 0; j < QMAX; ++j) r.k[j] = j < nq ? quantile_rank(qa, j, c) : 0xFFFFFFFFu;
            return r;
        },
        [&](uint32_t g, uint32_t lo, const Ranks& r, uint32_t ii, uint32_t less) {                  // the row whose rank is quantile j's answers it
            const U raw = x[lo + ii];
#pragma unroll
            for (uint32_t j = 0; j < QMAX; ++j)
                if (less == r.k[j]) out[(size_t)g * nq + j] = raw;
        });
}

// ---- the multi-prefix pass --------------------------------------------------------------------------------------------------------------------
// hist_rows (select_radix.hpp) for the nl leaders of lv: a row whose image matches leader q adds its digit at shift[q] to h + q * HSTRIDE
// (LDS) and folds into vand[q] / vor[q].
// NLT: the compile-time bound of nl (1, 2, 4 or QMAX), so that one leader costs what hist_rows costs.
template <class U, int KIND, uint32_t NLT, uint32_t NA>
__device__ __forceinline__ void hist_rows_nl(const U* __restrict__ x, uint32_t lo, uint32_t hi, const QLive* lv, uint32_t nl, uint32_t* h, U (&vand)[NA], U (&vor)[NA]) {
    static_assert(NLT <= NA, "one vand / vor per leader");
    U P[NLT], M[NLT];
    uint32_t S[NLT];
#pragma unroll
    for (uint32_t q = 0; q < NLT; ++q) {
        const uint32_t qq = q < nl ? q : 0u;
        P[q] = (U)uniform64(lv->prefix[qq]); M[q] = (U)uniform64(lv->kmask[qq]); S[q] = __builtin_amdgcn_readfirstlane(lv->shift[qq]);
    }
    sweep_rows<U>(x, lo, hi, [&](U raw, uint32_t, bool live) {
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
    });
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
        const bool done = digit_step<U>(st, hl[threadIdx.x], hl[256 * (NHIST<U> - 1) + threadIdx.x], wsum, sel);
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
int run_quant(aqg_ctx* ctx, const QArgs& qa, const SelInput& in, SelSwitches sw, void* outv) {
    const U* x = static_cast<const U*>(in.x);
    U* out = static_cast<U*>(outv);
    uint32_t* ctl = ctx->select_ctl;
    const uint32_t nq = qa.nq;
    SelPlan p;
    AQG_TRY(p.init(ctx, in.n, in.G, sw, nq * NHIST<U>, nq));
    QLive* slive;
    AQG_TRY(aqg_ws_get(ctx, p.scap, &slive));
    hipLaunchKernelGGL(quant_classify_kernel, dim3(p.ggrid), dim3(SB), 0, ctx->stream, in.off, in.G, sw.small_max, sw.split_min, qa, (int)sizeof(U) * 8, p.scap, p.tile_first, p.glist, p.sst, slive, ctl);
    aqg_kernel_timer_begin(ctx);
    if (p.do_small) hipLaunchKernelGGL((quant_small_kernel<U, KIND>), dim3(p.ntiles), dim3(SB), 0, ctx->stream, x, in.n, in.off, in.G, p.tile_first, sw.small_max, qa, out);
    if (p.do_group) hipLaunchKernelGGL((quant_group_kernel<U, KIND>), dim3(p.wgrid), dim3(SB), 0, ctx->stream, x, in.off, p.glist, ctl, qa, out);
    if (p.do_split) {
        hipLaunchKernelGGL(select_split_plan_kernel, dim3(1), dim3(SB), 0, ctx->stream, p.sst, ctl);
        for (size_t d = 0; d < sizeof(U); ++d) {
            hipLaunchKernelGGL((quant_split_hist_kernel<U, KIND, 1>), dim3(p.hgrid), dim3(SB), 0, ctx->stream, x, p.sst, slive, ctl, nq, p.ghist);
            if (d) hipLaunchKernelGGL((quant_split_hist_kernel<U, KIND, QMAX>), dim3(p.hgrid), dim3(SB), 0, ctx->stream, x, p.sst, slive, ctl, nq, p.ghist);
            hipLaunchKernelGGL((quant_split_choose_kernel<U, KIND>), dim3(p.cgrid), dim3(SB), 0, ctx->stream, p.sst, slive, ctl, nq, p.scap, p.ghist, out);
        }
        if constexpr (KIND == KIND_FP) hipLaunchKernelGGL((quant_split_find_kernel<U, KIND>), dim3(p.hgrid), dim3(SB), 0, ctx->stream, x, p.sst, ctl, nq, p.scap, out);
    }
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "quantile selection");
}
int dispatch_quant(aqg_ctx* ctx, const QArgs& qa, int t, const SelInput& in, SelSwitches sw, void* out) {
    return dispatch_kind(t, [&]<class U, int KIND>() { return run_quant<U, KIND>(ctx, qa, in, sw, out); });
}
// the checks every entry shares; fills qa
int check_args(aqg_ctx* ctx, int which, uint32_t nq, const uint32_t* num, uint32_t den, int t, QArgs* qa) {
    AQG_TRY(check_quant(ctx, "quantiles", which, nq, num, den, qa));
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "quantiles: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    return AQG_OK;
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g, int which, uint32_t nq, const uint32_t* num, uint32_t den, int t, const void* x, const void* out, QArgs* qa) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped quantiles: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped quantiles: the handle was not made by aqg_groupby_build");
    AQG_TRY(check_args(ctx, which, nq, num, den, t, qa));
    if ((!x || !out) && g->n) return aqg_fail(ctx, AQG_ERR_ARG, "grouped quantiles: null column");
    return AQG_OK;
}

int grouped_quantiles(aqg_ctx* ctx, aqg_groupby* g, int which, uint32_t nq, const uint32_t* num, uint32_t den, int t, const void* x, bool row_layout, void* out_dev) {
    QArgs qa;
    AQG_TRY(check_grouped(ctx, g, which, nq, num, den, t, x, out_dev, &qa));
    const SelSwitches sw = select_switches();
    SelInput in;
    AQG_TRY(select_prologue(ctx, g, x, g->n, esz_of(t), quant_ws_bytes(g->n, g->ngroups, nq, sw), row_layout, &in));
    if (!in.G) return AQG_OK;
    return dispatch_quant(ctx, qa, t, in, sw, out_dev);
}

} // namespace

extern "C" {

int aqg_quantiles(aqg_ctx* ctx, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, uint32_t n, void* out_host) {
    if (!ctx || !out_host) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_quantiles: bad argument");
    QArgs qa;
    AQG_TRY(check_args(ctx, which, nq, num_host, den, t, &qa));
    if (!x && n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_quantiles: null column");
    AQG_CHECK_ROWS(ctx, n, "aqg_quantiles");
    const SelSwitches sw = select_switches();
    SelInput in;
    AQG_TRY(select_prologue(ctx, nullptr, x, n, esz_of(t), quant_ws_bytes(n, 1, nq, sw), false, &in));
    const size_t bytes = (size_t)nq * esz_of(t);
    memset(out_host, 0, bytes);
    if (!in.G) return AQG_OK;
    uint32_t* result = ctx->select_ctl + QCTL_RESULT;
    AQG_TRY(dispatch_quant(ctx, qa, t, in, sw, result));
    return aqg_d2h(ctx, out_host, result, bytes);
}

int aqg_grouped_quantiles_flat(aqg_ctx* ctx, aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* xflat, void* out_dev) {
    return grouped_quantiles(ctx, g, which, nq, num_host, den, t, xflat, /*row_layout=*/false, out_dev);
}

int aqg_grouped_quantiles(aqg_ctx* ctx, aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, void* out_dev) {
    return grouped_quantiles(ctx, g, which, nq, num_host, den, t, x, /*row_layout=*/true, out_dev);
}

} // extern "C"
