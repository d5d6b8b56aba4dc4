// select_host.hpp -- the host side that select.hip (median), topk.hip (top-k) and quantile.hip (quantiles) share: the switches, the
// workspace sizes, the plan of a call (SelPlan: capacities, routes to launch, grids, the common buffers), the dtype dispatch, the
// prologue of an entry point and the validation of a quantile list (window_quantile.hip takes the last two).
#pragma once
#include <string>
#include "groupby_handle.hpp"
#include "select_radix.hpp"

namespace selradix {

struct SelSwitches { uint32_t small_max, split_min; };

inline SelSwitches select_switches() {
    const aqg_switch_set& s = aqg_switches();
    return SelSwitches{s.select_small_max < SMALL_CAP ? s.select_small_max : SMALL_CAP, s.select_split_min};
}
// most groups a route can meet whose groups hold at least `rows` of the n rows (and one slot to spare)
inline uint32_t route_cap(uint32_t n, uint32_t G, uint32_t rows) { return (n / rows < G ? n / rows : G) + 1; }
inline uint32_t split_cap(uint32_t n, uint32_t G, uint32_t split_min) { return route_cap(n, G, split_min ? split_min : 1u); }
inline uint32_t group_cap(uint32_t n, uint32_t G, uint32_t small_max) { return route_cap(n, G, small_max + 1); }
inline size_t select_ws_bytes(uint32_t n, uint32_t G, SelSwitches sw) {
    auto rup = [](size_t b) { return (b + 255) & ~(size_t)255; };
    return rup(((size_t)aqg_ceil_div(n, TILE) + 1) * 4) + rup((size_t)group_cap(n, G, sw.small_max) * 4) + rup((size_t)split_cap(n, G, sw.split_min) * (sizeof(SelState) + 2048)) + 4096;
}
inline int ensure_ctl(aqg_ctx* ctx) {
    if (!ctx->select_ctl) AQG_HIP(ctx, aqg_scratch_malloc(ctx, &ctx->select_ctl, 256));
    AQG_HIP(ctx, hipMemsetAsync(ctx->select_ctl, 0, CTL_WORDS * 4, ctx->stream));
    return AQG_OK;
}

// What the three routes of a call over n rows in G groups share: the capacities of the lists, the routes to launch (a route no group of
// this call can take is not launched: what the host knows without a look at the groups, n bounds every group), the grids, and the common
// buffers, carved from the workspace (sized by the family's *_ws_bytes and not reset in here) with their memsets issued.
struct SelPlan {
    uint32_t ntiles, scap, glcap;
    bool do_small, do_group, do_split;
    unsigned ggrid, wgrid, hgrid, cgrid;        // classify (a lane per group) / GROUP / SPLIT over the chunks / SPLIT over the groups
    uint32_t *tile_first, *glist, *ghist;
    SelState* sst;
    // nhist: 256-bin histograms per split group; planes: states per split group (sst[q * scap + s])
    int init(aqg_ctx* ctx, uint32_t n, uint32_t G, SelSwitches sw, uint32_t nhist, uint32_t planes = 1) {
        ntiles = aqg_ceil_div(n, TILE); scap = split_cap(n, G, sw.split_min); glcap = group_cap(n, G, sw.small_max);
        do_small = sw.small_max >= 1;
        do_group = n > sw.small_max && sw.split_min > sw.small_max + 1;
        do_split = n >= sw.split_min && n > sw.small_max;
        const uint64_t cap = (uint64_t)ctx->num_cu * 8, chunks = (uint64_t)aqg_ceil_div(n, SPLIT_CHUNK) + scap;
        ggrid = aqg_grid(ctx, G, SB, 1, 8);
        wgrid = (unsigned)(glcap < cap ? glcap : cap);
        hgrid = (unsigned)(chunks < cap ? chunks : cap);
        cgrid = scap < 1024u ? scap : 1024u;
        AQG_TRY(aqg_ws_get(ctx, (size_t)ntiles + 1, &tile_first));
        AQG_TRY(aqg_ws_get(ctx, glcap, &glist));
        AQG_TRY(aqg_ws_get(ctx, (size_t)scap * planes, &sst));
        AQG_TRY(aqg_ws_get(ctx, (size_t)scap * nhist * 256, &ghist));
        if (do_small) AQG_HIP(ctx, hipMemsetAsync(tile_first, 0xFF, (size_t)ntiles * 4, ctx->stream));
        if (do_split) AQG_HIP(ctx, hipMemsetAsync(ghist, 0, (size_t)scap * nhist * 1024, ctx->stream));
        return AQG_OK;
    }
};

// f.template operator()<U, KIND>() for the image type and kind of dtype t
template <class F> int dispatch_kind(int t, F&& f) {
    switch (t) {
    case AQG_UINT8: case AQG_BOOL: return f.template operator()<uint8_t, KIND_UNSIGNED>();
    case AQG_UINT16: return f.template operator()<uint16_t, KIND_UNSIGNED>();
    case AQG_UINT32: return f.template operator()<uint32_t, KIND_UNSIGNED>();
    case AQG_UINT64: return f.template operator()<uint64_t, KIND_UNSIGNED>();
    case AQG_INT8: return f.template operator()<uint8_t, KIND_SIGNED>();
    case AQG_INT16: return f.template operator()<uint16_t, KIND_SIGNED>();
    case AQG_INT32: return f.template operator()<uint32_t, KIND_SIGNED>();
    case AQG_INT64: return f.template operator()<uint64_t, KIND_SIGNED>();
    case AQG_FLOAT: return f.template operator()<uint32_t, KIND_FP>();
    case AQG_DOUBLE: return f.template operator()<uint64_t, KIND_FP>();
    }
    return AQG_ERR_DTYPE;
}

// the column of a call in the flat layout; G == 0: there is nothing to select
struct SelInput { const void* x; const uint32_t* off; uint32_t n, G; };
// What every entry point does between its checks and its dispatch.  g == nullptr: the n rows of x are the one group of a flat call.
// Else the groups of g, and x is in the flat layout already or, with row_layout, is brought into it (workspace).  ws_bytes: the family's
// *_ws_bytes of the call.  The control words are zeroed in any case.
inline int select_prologue(aqg_ctx* ctx, aqg_groupby* g, const void* x, uint32_t n, int esz, size_t ws_bytes, bool row_layout, SelInput* in) {
    AQG_TRY(ensure_ctl(ctx));
    *in = SelInput{x, nullptr, n, 0};
    const uint32_t G = g ? g->ngroups : 1u;
    if (n == 0 || G == 0) return AQG_OK;
    if (g && !(in->off = aqg_groupby_offsets(g))) return AQG_ERR_HIP;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (row_layout ? (size_t)n * esz + 4096 + aqg_postproc_ws_bytes(n, G, esz) : 0) + ws_bytes));
    if (!g) {
        uint32_t* off = ctx->select_ctl + CTL_OFF;
        hipLaunchKernelGGL(flat_offsets_kernel, dim3(1), dim3(1), 0, ctx->stream, off, n);
        in->off = off;
    } else if (row_layout) {
        unsigned char* xs;
        AQG_TRY(aqg_ws_get(ctx, (size_t)n * esz + 64, &xs));
        AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x, esz, xs, /*ws_managed=*/true));
        in->x = xs;
    }
    in->G = G;
    return AQG_OK;
}

// the checks of a quantile list that every entry taking one shares (`what` heads the messages); fills qa
inline int check_quant(aqg_ctx* ctx, const char* what, int which, uint32_t nq, const uint32_t* num, uint32_t den, QArgs* qa) {
    auto fail = [&](const char* msg) { return aqg_fail(ctx, AQG_ERR_ARG, (std::string(what) + msg).c_str()); };
    if (which != AQG_SEL_LOWER && which != AQG_SEL_UPPER) return fail(": which must be AQG_SEL_LOWER or AQG_SEL_UPPER");
    if (nq < 1 || nq > QMAX || !num || den < 1) return fail(": 1 <= nq <= AQG_QUANTILES_MAX ranks num[j] / den with den >= 1");
    *qa = QArgs{};
    qa->nq = nq; qa->den = den; qa->which = (uint32_t)which;
    for (uint32_t j = 0; j < nq; ++j) {
        if (num[j] > den) return fail(": num[j] > den");
        qa->num[j] = num[j];
    }
    return AQG_OK;
}

} // namespace selradix
