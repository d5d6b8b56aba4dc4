// select.hip -- aqg_median / aqg_grouped_median(_flat): the lower / upper median of a column and of every group's slice of the flat layout
// (`median`, reference common/types.py:343; benchmark/h2o/groupby.sql:11-12, the one h2o query the reference leaves commented out).
//
// A selection, not a sort: rows are never moved.  Values are compared through their order-preserving images (key_image.hpp), and the
// rank-k image of a slice is found by MSD radix selection: histogram one 8-bit digit of the rows that still match the bits chosen so far,
// take the bin that holds the rank, subtract the rows below it, descend.  Every histogram pass also folds the AND and the OR of the
// candidates' images: when they agree every candidate is the same value and the selection is over (one candidate is the plain case), and
// when the chosen bin holds every candidate the next digit starts at their highest differing bit.
// Group sizes of one call range from one row to the whole column, so there are three routes, chosen per group on the device:
//   SMALL  up to AQG_SELECT_SMALL_MAX rows: a workgroup stages the images of a tile of flat positions (plus one group's worth behind it) in
//          LDS and its wavefronts rank every group that STARTS in the tile by comparison counting, many groups per workgroup, one launch;
//          groups of one or two rows take a lane each
//   GROUP  one workgroup owns one group: an LDS histogram per digit, the slice re-read per digit (from L2 / Infinity Cache at h2o sizes)
//   SPLIT  from AQG_SELECT_SPLIT_MIN rows: the group is cut into chunks, workgroups histogram a contiguous span of chunks in LDS and merge
//          into the group's histogram in HBM; a small kernel chooses the bin between digits.  Digits are separated by launches: no
//          workgroup ever waits for another.
// A classify kernel over the offsets routes the groups (two compact lists, a per-tile first group); nothing comes back to the host, and
// the number of launches depends on the dtype's width only.
#include "select_host.hpp"

namespace {
using namespace selradix;

__device__ inline uint32_t median_rank(int which, uint32_t c) { return which ? c / 2 : (c - 1) / 2; }

// ---- routing: one lane per group ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB) select_classify_kernel(const uint32_t* __restrict__ off, uint32_t G, uint32_t small_max, uint32_t split_min, int which, int bits,
                                                              uint32_t* __restrict__ tile_first, uint32_t* __restrict__ glist, SelState* __restrict__ sst, uint32_t* __restrict__ ctl) {
    classify_groups(off, G, small_max, split_min, tile_first, glist, ctl,
                    [&](uint32_t g, uint32_t lo, uint32_t hi, uint32_t c, uint32_t s) { sst[s] = split_state(lo, hi, median_rank(which, c), g, (uint32_t)bits); });
}
// ---- SMALL ----------------------------------------------------------------------------------------------------------------------------------
template <class U, int KIND>
__global__ void __launch_bounds__(SB) select_small_kernel(const U* __restrict__ x, uint32_t n, const uint32_t* __restrict__ off, uint32_t G,
                                                           const uint32_t* __restrict__ tile_first, uint32_t small_max, int which, U* __restrict__ out) {
    small_tile<U, KIND>(
        x, n, off, G, tile_first, small_max,
        [&](uint32_t g, uint32_t lo, uint32_t c, bool a_first) { const U a = x[lo], b = x[lo + c - 1]; out[g] = a_first == (which != 0) ? b : a; },
        [&](uint32_t c) { return median_rank(which, c); },
        [&](uint32_t g, uint32_t lo, uint32_t k, uint32_t ii, uint32_t less) { if (less == k) out[g] = x[lo + ii]; });        // the row of rank k is the answer
}

// ---- GROUP ----------------------------------------------------------------------------------------------------------------------------------
template <class U, int KIND>
__global__ void __launch_bounds__(SB) select_group_kernel(const U* __restrict__ x, const uint32_t* __restrict__ off, const uint32_t* __restrict__ glist,
                                                           uint32_t* __restrict__ ctl, int which, U* __restrict__ out) {
    __shared__ uint32_t h[256 * NHIST<U>];
    __shared__ uint32_t wsum[NWV];
    __shared__ unsigned long long s_and, s_or;
    __shared__ BinSel sel;
    const uint32_t ngl = ctl[CTL_NGROUP];
    uint32_t maxp = 0;
    for (uint32_t li = blockIdx.x; li < ngl; li += gridDim.x) {
        const uint32_t g = glist[li], lo = off[g], hi = off[g + 1], c = hi - lo;
        SelState st{};
        st.k = median_rank(which, c);
        st.shift = sizeof(U) * 8 - 8;
        do {
            group_pass<U, KIND>(x, lo, hi, st, h, &s_and, &s_or);
        } while (!digit_step<U>(st, h[threadIdx.x], h[256 * (NHIST<U> - 1) + threadIdx.x], wsum, &sel));
        maxp = st.passes > maxp ? st.passes : maxp;
        const U result = (U)st.prefix;
        if (image_is_shared<U, KIND>(result)) find_rows<U, KIND>(x, lo, hi, result, out + g);
        else if (threadIdx.x == 0) out[g] = value_of<U, KIND>(result);
    }
    if (threadIdx.x == 0 && maxp) atomicMax(&ctl[CTL_PASSES], maxp);
}

// ---- SPLIT ----------------------------------------------------------------------------------------------------------------------------------
// (the chunk plan and the histogram pass: select_radix.hpp)
template <class U, int KIND>
__global__ void __launch_bounds__(SB) select_split_choose_kernel(SelState* __restrict__ sst, uint32_t* __restrict__ ctl, uint32_t* __restrict__ ghist, U* __restrict__ out) {
    __shared__ uint32_t wsum[NWV];
    __shared__ BinSel sel;
    const uint32_t ns = ctl[CTL_NSPLIT];
    for (uint32_t s = blockIdx.x; s < ns; s += gridDim.x) {
        SelState st = sst[s];
        __syncthreads();                                    // (every lane has read the state before lane 0 rewrites it)
        if (st.done) continue;
        uint32_t* gh = ghist + (size_t)s * NHIST<U> * 256;
        const uint32_t c = gh[threadIdx.x], c2 = gh[256 * (NHIST<U> - 1) + threadIdx.x];
        for (uint32_t j = 0; j < NHIST<U>; ++j) gh[j * 256 + threadIdx.x] = 0;
        ++st.passes;
        const bool done = digit_step<U>(st, c, c2, wsum, &sel);
        if (threadIdx.x == 0) {
            if (done) {
                const U result = (U)st.prefix;
                st.done = image_is_shared<U, KIND>(result) ? 2u : 1u;
                if (st.done == 1) out[st.gidx] = value_of<U, KIND>(result);
                atomicMax(&ctl[CTL_PASSES], st.passes);
            }
            st.vand = ~0ull; st.vor = 0ull;
            sst[s] = st;
        }
    }
}
// groups whose image is shared by several bit patterns: any element of the slice with that image
template <class U, int KIND>
__global__ void __launch_bounds__(SB) select_split_find_kernel(const U* __restrict__ x, const SelState* __restrict__ sst, const uint32_t* __restrict__ ctl, U* __restrict__ out) {
    uint32_t q0, q1, s, ns;
    if (!split_span(sst, ctl, q0, q1, s, ns)) return;
    for (uint32_t q = q0; q < q1; ++q) {
        while (s + 1 < ns && sst[s + 1].cbase <= q) ++s;
        if (sst[s].done != 2) continue;
        const uint32_t lo = sst[s].lo + (q - sst[s].cbase) * SPLIT_CHUNK, ghi = sst[s].hi;
        find_rows<U, KIND>(x, lo, ghi - lo < SPLIT_CHUNK ? ghi : lo + SPLIT_CHUNK, (U)sst[s].prefix, out + sst[s].gidx);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
// the three routes over a column in the flat layout (workspace sized by select_ws_bytes and not reset in here; the control words are zero)
template <class U, int KIND>
int run_select(aqg_ctx* ctx, int which, const SelInput& in, SelSwitches sw, void* outv) {
    const U* x = static_cast<const U*>(in.x);
    U* out = static_cast<U*>(outv);
    uint32_t* ctl = ctx->select_ctl;
    SelPlan p;
    AQG_TRY(p.init(ctx, in.n, in.G, sw, NHIST<U>));
    hipLaunchKernelGGL(select_classify_kernel, dim3(p.ggrid), dim3(SB), 0, ctx->stream, in.off, in.G, sw.small_max, sw.split_min, which, (int)sizeof(U) * 8, p.tile_first, p.glist, p.sst, ctl);
    aqg_kernel_timer_begin(ctx);
    if (p.do_small) hipLaunchKernelGGL((select_small_kernel<U, KIND>), dim3(p.ntiles), dim3(SB), 0, ctx->stream, x, in.n, in.off, in.G, p.tile_first, sw.small_max, which, out);
    if (p.do_group) hipLaunchKernelGGL((select_group_kernel<U, KIND>), dim3(p.wgrid), dim3(SB), 0, ctx->stream, x, in.off, p.glist, ctl, which, out);
    if (p.do_split) {
        hipLaunchKernelGGL(select_split_plan_kernel, dim3(1), dim3(SB), 0, ctx->stream, p.sst, ctl);
        for (size_t d = 0; d < sizeof(U); ++d) {
            hipLaunchKernelGGL((select_split_hist_kernel<U, KIND>), dim3(p.hgrid), dim3(SB), 0, ctx->stream, x, p.sst, ctl, p.ghist);
            hipLaunchKernelGGL((select_split_choose_kernel<U, KIND>), dim3(p.cgrid), dim3(SB), 0, ctx->stream, p.sst, ctl, p.ghist, out);
        }
        if constexpr (KIND == KIND_FP) hipLaunchKernelGGL((select_split_find_kernel<U, KIND>), dim3(p.hgrid), dim3(SB), 0, ctx->stream, x, p.sst, ctl, out);
    }
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "median selection");
}
int dispatch_select(aqg_ctx* ctx, int which, int t, const SelInput& in, SelSwitches sw, void* out) {
    return dispatch_kind(t, [&]<class U, int KIND>() { return run_select<U, KIND>(ctx, which, in, sw, out); });
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g, int which, int t, const void* x, const void* out) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped median: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped median: the handle was not made by aqg_groupby_build");
    if (which != AQG_SEL_LOWER && which != AQG_SEL_UPPER) return aqg_fail(ctx, AQG_ERR_ARG, "grouped median: which must be AQG_SEL_LOWER or AQG_SEL_UPPER");
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "grouped median: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    if ((!x || !out) && g->n) return aqg_fail(ctx, AQG_ERR_ARG, "grouped median: null column");
    return AQG_OK;
}
int grouped_median(aqg_ctx* ctx, aqg_groupby* g, int which, int t, const void* x, bool row_layout, void* out_dev) {
    AQG_TRY(check_grouped(ctx, g, which, t, x, out_dev));
    const SelSwitches sw = select_switches();
    SelInput in;
    AQG_TRY(select_prologue(ctx, g, x, g->n, esz_of(t), select_ws_bytes(g->n, g->ngroups, sw), row_layout, &in));
    if (!in.G) return AQG_OK;
    return dispatch_select(ctx, which, t, in, sw, out_dev);
}

} // namespace

extern "C" {

int aqg_median(aqg_ctx* ctx, int which, int t, const void* x, uint32_t n, void* out_host16) {
    if (!ctx || !out_host16) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_median: bad argument");
    if (which != AQG_SEL_LOWER && which != AQG_SEL_UPPER) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_median: which must be AQG_SEL_LOWER or AQG_SEL_UPPER");
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_median: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    if (!x && n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_median: null column");
    AQG_CHECK_ROWS(ctx, n, "aqg_median");
    const SelSwitches sw = select_switches();
    SelInput in;
    AQG_TRY(select_prologue(ctx, nullptr, x, n, esz_of(t), select_ws_bytes(n, 1, sw), false, &in));
    memset(out_host16, 0, 16);
    if (!in.G) return AQG_OK;
    uint32_t* result = ctx->select_ctl + CTL_RESULT;
    AQG_TRY(dispatch_select(ctx, which, t, in, sw, result));
    return aqg_d2h(ctx, out_host16, result, 16);
}

int aqg_grouped_median_flat(aqg_ctx* ctx, aqg_groupby* g, int which, int t, const void* xflat, void* out_dev) {
    return grouped_median(ctx, g, which, t, xflat, /*row_layout=*/false, out_dev);
}

int aqg_grouped_median(aqg_ctx* ctx, aqg_groupby* g, int which, int t, const void* x, void* out_dev) {
    return grouped_median(ctx, g, which, t, x, /*row_layout=*/true, out_dev);
}

int aqg_select_last_routes(aqg_ctx* ctx, uint32_t* routes_host, uint32_t* passes_host) {
    if (!ctx || !routes_host || !passes_host) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_select_last_routes: bad argument");
    uint32_t w[2] = {0, 0};
    if (ctx->select_ctl) AQG_TRY(aqg_d2h(ctx, w, ctx->select_ctl, 8));
    *routes_host = w[0];
    *passes_host = w[1];
    return AQG_OK;
}

} // extern "C"
