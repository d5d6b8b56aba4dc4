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
#include "groupby_handle.hpp"
#include "select_radix.hpp"

namespace {
using namespace selradix;

// ---- routing: one lane per group ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB) select_classify_kernel(const uint32_t* __restrict__ off, uint32_t G, uint32_t small_max, uint32_t split_min, int which, int bits,
                                                              uint32_t* __restrict__ tile_first, uint32_t* __restrict__ glist, SelState* __restrict__ sst, uint32_t* __restrict__ ctl) {
    uint32_t mask = 0;
    for (uint32_t g = blockIdx.x * SB + threadIdx.x; g < G; g += gridDim.x * SB) {
        const uint32_t lo = off[g], hi = off[g + 1], c = hi - lo;
        if (c == 0) continue;
        if (c <= small_max) {
            mask |= ROUTE_SMALL;
            // the first SMALL group that starts in its tile: only a group whose predecessor starts in another tile, or is not SMALL, can be it
            bool first = g == 0;
            if (!first) { const uint32_t plo = off[g - 1], pc = lo - plo; first = plo / TILE != lo / TILE || pc > small_max || pc == 0; }
            if (first) atomicMin(&tile_first[lo / TILE], g);
        } else if (c < split_min) {
            mask |= ROUTE_GROUP;
            glist[atomicAdd(&ctl[CTL_NGROUP], 1u)] = g;
        } else {
            mask |= ROUTE_SPLIT;
            SelState st{};
            st.vand = ~0ull;
            st.lo = lo; st.hi = hi; st.k = which ? c / 2 : (c - 1) / 2; st.gidx = g;
            st.shift = (uint32_t)bits - 8;
            sst[atomicAdd(&ctl[CTL_NSPLIT], 1u)] = st;
        }
    }
    mask = wave_reduce(mask, OpOr{});
    if (lane_id() == 0 && mask) {
        atomicOr(&ctl[CTL_ROUTES], mask);
        if (mask & ROUTE_SMALL) atomicMax(&ctl[CTL_PASSES], 1u);       // ranking by comparison: one pass over the group
    }
}
// ---- SMALL ----------------------------------------------------------------------------------------------------------------------------------
template <class U, int KIND>
__global__ void __launch_bounds__(SB) select_small_kernel(const U* __restrict__ x, uint32_t n, const uint32_t* __restrict__ off, uint32_t G,
                                                           const uint32_t* __restrict__ tile_first, uint32_t small_max, int which, U* __restrict__ out) {
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
    // one or two rows: a lane each, from the column itself
    bool any = false;
    for (uint32_t gi = threadIdx.x; gi < ng; gi += SB) {
        const uint32_t lo = goff[gi], c = goff[gi + 1] - lo;
        if (c > small_max || c == 0) continue;
        if (c == 1) out[g0 + gi] = x[lo];
        else if (c == 2) {
            const U a = x[lo], b = x[lo + 1];
            const bool swap = image_of<U, KIND>(b) < image_of<U, KIND>(a);
            out[g0 + gi] = (swap != (which != 0)) ? b : a;
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
    // a wavefront per group: rank of every row = rows that sort before it (ties by position); the row of rank k is the answer
    const uint32_t lane = lane_id();
    for (uint32_t gi = wave_id(); gi < ng; gi += NWV) {
        const uint32_t lo = goff[gi], c = goff[gi + 1] - lo;
        if (c < 3 || c > small_max) continue;
        const uint32_t base = lo - tbeg, k = which ? c / 2 : (c - 1) / 2;
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
            if (live && less == k) out[g0 + gi] = x[lo + ii];
        }
    }
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
        st.k = which ? c / 2 : (c - 1) / 2;
        st.shift = sizeof(U) * 8 - 8;
        U result;
        for (;;) {
            __syncthreads();
            for (uint32_t j = 0; j < NHIST<U>; ++j) h[j * 256 + threadIdx.x] = 0;
            if (threadIdx.x == 0) { s_and = ~0ull; s_or = 0ull; }
            __syncthreads();
            U vand = (U)~U(0), vor = 0;
            hist_rows<U, KIND>(x, lo, hi, (U)st.prefix, (U)st.kmask, st.shift, h, vand, vor);
            fold_and_or(vand, vor, &s_and, &s_or);
            __syncthreads();
            ++st.passes;
            st.vand = s_and; st.vor = s_or;
            if (st.vand == st.vor) { result = (U)st.vand; break; }          // one candidate, or all of them equal
            choose_bin(h[threadIdx.x], st.k, wsum, &sel);
            if (both_digits_known<U>(st, sel.cnt, sel.total)) {
                __syncthreads();
                choose_bin(h[256 * (NHIST<U> - 1) + threadIdx.x], st.k, wsum, &sel);
                result = (U)((st.vand & ~0xFFull) | sel.bin);
                break;
            }
            if (sel_advance(st, sel.bin, sel.excl, sel.cnt, sel.total)) { result = (U)st.prefix; break; }
        }
        maxp = st.passes > maxp ? st.passes : maxp;
        if (image_is_shared<U, KIND>(result)) find_rows<U, KIND>(x, lo, hi, result, out + g);
        else if (threadIdx.x == 0) out[g] = value_of<U, KIND>(result);
    }
    if (threadIdx.x == 0 && maxp) atomicMax(&ctl[CTL_PASSES], maxp);
}

// ---- SPLIT ----------------------------------------------------------------------------------------------------------------------------------
// (the chunk plan and the histogram pass: select_dev.hpp)
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
        bool done;
        if (st.vand == st.vor) { st.prefix = st.vand; done = true; }
        else {
            choose_bin(c, st.k, wsum, &sel);
            if (both_digits_known<U>(st, sel.cnt, sel.total)) {
                __syncthreads();
                choose_bin(c2, st.k, wsum, &sel);
                st.prefix = (st.vand & ~0xFFull) | sel.bin;
                done = true;
            } else done = sel_advance(st, sel.bin, sel.excl, sel.cnt, sel.total);
        }
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
int run_select(aqg_ctx* ctx, int which, const void* xv, uint32_t n, const uint32_t* off, uint32_t G, SelSwitches sw, void* outv) {
    const U* x = static_cast<const U*>(xv);
    U* out = static_cast<U*>(outv);
    uint32_t* ctl = ctx->select_ctl;
    const uint32_t ntiles = aqg_ceil_div(n, TILE), scap = split_cap(n, G, sw.split_min);
    const uint32_t glcap = (n / (sw.small_max + 1) < G ? n / (sw.small_max + 1) : G) + 1;
    // routes no group of this call can take are not launched (what the host knows without a look at the groups: n bounds every group)
    const bool do_small = sw.small_max >= 1, do_group = n > sw.small_max && sw.split_min > sw.small_max + 1, do_split = n >= sw.split_min && n > sw.small_max;
    uint32_t *tile_first, *glist, *ghist;
    SelState* sst;
    AQG_TRY(aqg_ws_get(ctx, (size_t)ntiles + 1, &tile_first));
    AQG_TRY(aqg_ws_get(ctx, glcap, &glist));
    AQG_TRY(aqg_ws_get(ctx, scap, &sst));
    AQG_TRY(aqg_ws_get(ctx, (size_t)scap * 256 * NHIST<U>, &ghist));
    if (do_small) AQG_HIP(ctx, hipMemsetAsync(tile_first, 0xFF, (size_t)ntiles * 4, ctx->stream));
    if (do_split) AQG_HIP(ctx, hipMemsetAsync(ghist, 0, (size_t)scap * 1024 * NHIST<U>, ctx->stream));
    const unsigned ggrid = aqg_grid(ctx, G, SB, 1, 8);
    hipLaunchKernelGGL(select_classify_kernel, dim3(ggrid), dim3(SB), 0, ctx->stream, off, G, sw.small_max, sw.split_min, which, (int)sizeof(U) * 8, tile_first, glist, sst, ctl);
    aqg_kernel_timer_begin(ctx);
    if (do_small) {
        hipLaunchKernelGGL((select_small_kernel<U, KIND>), dim3(ntiles), dim3(SB), 0, ctx->stream, x, n, off, G, tile_first, sw.small_max, which, out);
    }
    if (do_group) {
        const uint32_t cap = (uint32_t)ctx->num_cu * 8;
        hipLaunchKernelGGL((select_group_kernel<U, KIND>), dim3(glcap < cap ? glcap : cap), dim3(SB), 0, ctx->stream, x, off, glist, ctl, which, out);
    }
    if (do_split) {
        const uint64_t chunks = (uint64_t)aqg_ceil_div(n, SPLIT_CHUNK) + scap;
        const unsigned hgrid = (unsigned)(chunks < (uint64_t)ctx->num_cu * 8 ? chunks : (uint64_t)ctx->num_cu * 8);
        const unsigned cgrid = scap < 1024u ? scap : 1024u;
        hipLaunchKernelGGL(select_split_plan_kernel, dim3(1), dim3(SB), 0, ctx->stream, sst, ctl);
        for (size_t p = 0; p < sizeof(U); ++p) {
            hipLaunchKernelGGL((select_split_hist_kernel<U, KIND>), dim3(hgrid), dim3(SB), 0, ctx->stream, x, sst, ctl, ghist);
            hipLaunchKernelGGL((select_split_choose_kernel<U, KIND>), dim3(cgrid), dim3(SB), 0, ctx->stream, sst, ctl, ghist, out);
        }
        if constexpr (KIND == KIND_FP) hipLaunchKernelGGL((select_split_find_kernel<U, KIND>), dim3(hgrid), dim3(SB), 0, ctx->stream, x, sst, ctl, out);
    }
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "median selection");
}
int dispatch_select(aqg_ctx* ctx, int which, int t, const void* x, uint32_t n, const uint32_t* off, uint32_t G, SelSwitches sw, void* out) {
    switch (t) {
    case AQG_UINT8: case AQG_BOOL: return run_select<uint8_t, KIND_UNSIGNED>(ctx, which, x, n, off, G, sw, out);
    case AQG_UINT16: return run_select<uint16_t, KIND_UNSIGNED>(ctx, which, x, n, off, G, sw, out);
    case AQG_UINT32: return run_select<uint32_t, KIND_UNSIGNED>(ctx, which, x, n, off, G, sw, out);
    case AQG_UINT64: return run_select<uint64_t, KIND_UNSIGNED>(ctx, which, x, n, off, G, sw, out);
    case AQG_INT8: return run_select<uint8_t, KIND_SIGNED>(ctx, which, x, n, off, G, sw, out);
    case AQG_INT16: return run_select<uint16_t, KIND_SIGNED>(ctx, which, x, n, off, G, sw, out);
    case AQG_INT32: return run_select<uint32_t, KIND_SIGNED>(ctx, which, x, n, off, G, sw, out);
    case AQG_INT64: return run_select<uint64_t, KIND_SIGNED>(ctx, which, x, n, off, G, sw, out);
    case AQG_FLOAT: return run_select<uint32_t, KIND_FP>(ctx, which, x, n, off, G, sw, out);
    case AQG_DOUBLE: return run_select<uint64_t, KIND_FP>(ctx, which, x, n, off, G, sw, out);
    }
    return AQG_ERR_DTYPE;
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g, int which, int t, const void* x, const void* out) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped median: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped median: the handle was not made by aqg_groupby_build");
    if (which != AQG_SEL_LOWER && which != AQG_SEL_UPPER) return aqg_fail(ctx, AQG_ERR_ARG, "grouped median: which must be AQG_SEL_LOWER or AQG_SEL_UPPER");
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "grouped median: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    if ((!x || !out) && g->n) return aqg_fail(ctx, AQG_ERR_ARG, "grouped median: null column");
    return AQG_OK;
}

} // namespace

extern "C" {

int aqg_median(aqg_ctx* ctx, int which, int t, const void* x, uint32_t n, void* out_host16) {
    if (!ctx || !out_host16) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_median: bad argument");
    if (which != AQG_SEL_LOWER && which != AQG_SEL_UPPER) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_median: which must be AQG_SEL_LOWER or AQG_SEL_UPPER");
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_median: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    if (!x && n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_median: null column");
    AQG_CHECK_ROWS(ctx, n, "aqg_median");
    AQG_TRY(ensure_ctl(ctx));
    memset(out_host16, 0, 16);
    if (n == 0) return AQG_OK;
    const SelSwitches sw = select_switches();
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, select_ws_bytes(n, 1, sw)));
    uint32_t* ctl = ctx->select_ctl;
    hipLaunchKernelGGL(flat_offsets_kernel, dim3(1), dim3(1), 0, ctx->stream, ctl + CTL_OFF, n);
    AQG_TRY(dispatch_select(ctx, which, t, x, n, ctl + CTL_OFF, 1, sw, ctl + CTL_RESULT));
    return aqg_d2h(ctx, out_host16, ctl + CTL_RESULT, 16);
}

int aqg_grouped_median_flat(aqg_ctx* ctx, aqg_groupby* g, int which, int t, const void* xflat, void* out_dev) {
    AQG_TRY(check_grouped(ctx, g, which, t, xflat, out_dev));
    AQG_TRY(ensure_ctl(ctx));
    const uint32_t n = g->n, G = g->ngroups;
    if (n == 0 || G == 0) return AQG_OK;
    const uint32_t* off = aqg_groupby_offsets(g);
    if (!off) return AQG_ERR_HIP;
    const SelSwitches sw = select_switches();
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, select_ws_bytes(n, G, sw)));
    return dispatch_select(ctx, which, t, xflat, n, off, G, sw, out_dev);
}

int aqg_grouped_median(aqg_ctx* ctx, aqg_groupby* g, int which, int t, const void* x, void* out_dev) {
    AQG_TRY(check_grouped(ctx, g, which, t, x, out_dev));
    AQG_TRY(ensure_ctl(ctx));
    const uint32_t n = g->n, G = g->ngroups;
    if (n == 0 || G == 0) return AQG_OK;
    const uint32_t* off = aqg_groupby_offsets(g);
    if (!off) return AQG_ERR_HIP;
    const SelSwitches sw = select_switches();
    const int esz = esz_of(t);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * esz + 4096 + aqg_postproc_ws_bytes(n, G, esz) + select_ws_bytes(n, G, sw)));
    unsigned char* xs;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n * esz + 64, &xs));
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x, esz, xs, /*ws_managed=*/true));
    return dispatch_select(ctx, which, t, xs, n, off, G, sw, out_dev);
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
