// topk.hip -- aqg_topk / aqg_grouped_topk(_flat): the k largest or k smallest elements of a column and of every group's slice of the flat
// layout, in order, with their positions (h2o Q8 `largest two v3 by id6`, benchmark/h2o/groupby.sql:16-17; ORDER BY x DESC LIMIT k).
//
// A selection, not a sort: rows are never moved.  Every row is compared through its KEY: the order-preserving image of key_image.hpp under
// AQG_ORDER_ASC, its complement under AQG_ORDER_DESC, so that both orders are "the m = min(k, c) smallest keys of the c rows, ties by
// ascending position".  The three routes and their thresholds are those of select.hip (select_radix.hpp), chosen per group on the device:
//   SMALL  a workgroup stages the keys of a tile of flat positions in LDS and its wavefronts rank every group that starts in the tile by
//          comparison counting (ties by position); a row of rank r < m stores itself at slot r.  One launch, no threshold search.
//   GROUP  one workgroup owns one group: the MSD radix selection of select.hip finds the key T of rank m - 1 and, on the way, how many of
//          the rows equal to T are wanted (`need`: the rank left among the candidates, plus one); one more pass over the slice collects the
//          positions of every row below T and of `need` rows equal to T into LDS, the workgroup ranks them there and writes them out.
//          A group of at most k rows skips the search and collects everything.
//   SPLIT  the per-chunk histograms of select.hip with a choose kernel between digits, a collect pass over the chunks with two cursors per
//          group in HBM (rows below T; a ticket bounded by `need` for the rows equal to T), and one workgroup per group that ranks and emits.
//          No workgroup waits for another.
// Elements are written as read back through their position, so every value is an element of the input bit for bit whatever its image.
// Which of the rows equal to T are taken when there are more than `need` depends on the order the wavefronts arrive in.
#include "select_host.hpp"

namespace {
using namespace selradix;

constexpr uint32_t KMAX = AQG_TOPK_MAX;
static_assert(KMAX % SB == 0 && SMALL_CAP <= KMAX, "the candidates of a group are ranked SB at a time; a SMALL group fits its own slots");
constexpr uint32_t DONE_KEY = 1, DONE_ALL = 3;          // SelState::done of a SPLIT group: T is st.prefix / every row is taken

__device__ inline uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// the lanes of a wavefront with `p` set take consecutive numbers from *counter (one atomic per wavefront; others: 0xFFFFFFFF).
// *end: one past the last number this wavefront took (the same in every lane; 0 when no lane asked)
__device__ inline uint32_t wave_take(uint32_t* counter, bool p, uint32_t* end) {
    const uint64_t mask = __ballot(p);
    *end = 0;
    if (!mask) return 0xFFFFFFFFu;
    const int leader = __ffsll((long long)mask) - 1, lane = lane_id();
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, leader, 64);
    *end = base + (uint32_t)__popcll(mask);
    return p ? base + (uint32_t)__popcll(mask & ((1ull << lane) - 1)) : 0xFFFFFFFFu;
}

// What one group keeps: every row whose key is below T, and `need` of the rows whose key is T (all: every row).  Their positions go to
// cand[0, m): the rows below T from slot 0 up by cnt[0], the rows equal to T from slot m - need up by the ticket cnt[1].  `full` (the same
// in every lane of a wavefront) stops the tickets once they are out, so that a slice of equal rows does not queue up on one counter.
template <class U, int KIND>
struct Keep {
    U T;
    uint32_t m, need;
    bool all;
    uint32_t* cnt;
    uint32_t* cand;
    bool full;
    __device__ inline void row(U raw, uint32_t pos, bool live) {
        const U key = image_of<U, KIND>(raw);
        const bool lt = live && (all || key < T);
        uint32_t end;
        const uint32_t s = wave_take(&cnt[0], lt, &end);
        if (lt && s < m) cand[s] = pos;
        if (all || full) return;
        const bool eq = live && key == T;
        const uint32_t t = wave_take(&cnt[1], eq, &end);
        if (eq && t < need) cand[m - need + t] = pos;
        full = end >= need;
    }
};

// cand[0, m): the positions a group keeps (LDS).  Their keys -> keys[], then every candidate counts the candidates that sort before it
// (key, then position) and writes its element, re-read through the position, to that slot of the group's k.
template <class U, int KIND>
__device__ inline void rank_emit(const U* __restrict__ x, const uint32_t* cand, U* keys, uint32_t m, size_t slot0, U* __restrict__ vals, uint32_t* __restrict__ pos_out) {
    for (uint32_t i = threadIdx.x; i < m; i += SB) keys[i] = image_of<U, KIND>(x[cand[i]]);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m; i += SB) {
        const U mine = keys[i];
        const uint32_t mp = cand[i];
        uint32_t r = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < m; ++j) {
            const U v = keys[j];
            r += (v < mine) | ((v == mine) & (cand[j] < mp));
        }
        vals[slot0 + r] = x[mp];
        if (pos_out) pos_out[slot0 + r] = mp;
    }
}

// ---- routing: one lane per group (the rank wanted is the last of the m kept rows) ------------------------------------------------------------
__global__ void __launch_bounds__(SB) topk_classify_kernel(const uint32_t* __restrict__ off, uint32_t G, uint32_t small_max, uint32_t split_min, uint32_t k, int bits,
                                                            uint32_t* __restrict__ tile_first, uint32_t* __restrict__ glist, SelState* __restrict__ sst, uint32_t* __restrict__ ctl) {
    classify_groups(off, G, small_max, split_min, tile_first, glist, ctl, [&](uint32_t g, uint32_t lo, uint32_t hi, uint32_t c, uint32_t s) {
        SelState st = split_state(lo, hi, min_u32(k, c) - 1, g, (uint32_t)bits);
        st.done = c <= k ? DONE_ALL : 0u;
        sst[s] = st;
    });
}

// ---- SMALL ----------------------------------------------------------------------------------------------------------------------------------
template <class U, int KIND>
__global__ void __launch_bounds__(SB) topk_small_kernel(const U* __restrict__ x, uint32_t n, const uint32_t* __restrict__ off, uint32_t G,
                                                         const uint32_t* __restrict__ tile_first, uint32_t small_max, uint32_t k, U* __restrict__ vals, uint32_t* __restrict__ pos_out) {
    auto put = [&](uint32_t g, uint32_t slot, uint32_t p) {
        const size_t o = (size_t)g * k + slot;
        vals[o] = x[p];
        if (pos_out) pos_out[o] = p;
    };
    small_tile<U, KIND>(
        x, n, off, G, tile_first, small_max,
        [&](uint32_t g, uint32_t lo, uint32_t c, bool a_first) {                                     // (equal keys: positions ascend)
            put(g, 0, a_first ? lo : lo + 1);
            if (c == 2 && k > 1) put(g, 1, a_first ? lo + 1 : lo);
        },
        [&](uint32_t c) { return min_u32(k, c); },
        [&](uint32_t g, uint32_t lo, uint32_t m, uint32_t ii, uint32_t less) { if (less < m) put(g, less, lo + ii); });      // the rows of rank below m are the answer
}

// ---- GROUP ----------------------------------------------------------------------------------------------------------------------------------
template <class U, int KIND>
__global__ void __launch_bounds__(SB) topk_group_kernel(const U* __restrict__ x, const uint32_t* __restrict__ off, const uint32_t* __restrict__ glist,
                                                         uint32_t* __restrict__ ctl, uint32_t k, U* __restrict__ vals, uint32_t* __restrict__ pos_out) {
    __shared__ uint32_t h[256 * NHIST<U>];
    __shared__ uint32_t wsum[NWV];
    __shared__ unsigned long long s_and, s_or;
    __shared__ BinSel sel;
    __shared__ uint32_t s_cnt[2];
    __shared__ uint32_t cand[KMAX];
    __shared__ U keys[KMAX];
    const uint32_t ngl = ctl[CTL_NGROUP];
    uint32_t maxp = 0;
    for (uint32_t li = blockIdx.x; li < ngl; li += gridDim.x) {
        const uint32_t g = glist[li], lo = off[g], hi = off[g + 1], c = hi - lo, m = min_u32(k, c);
        SelState st{};
        st.k = m - 1;
        st.shift = sizeof(U) * 8 - 8;
        while (c > k) {                                                         // the key of rank m - 1; st.k ends as that rank among the rows equal to it
            group_pass<U, KIND>(x, lo, hi, st, h, &s_and, &s_or);
            if (digit_step<U>(st, h[threadIdx.x], h[256 * (NHIST<U> - 1) + threadIdx.x], wsum, &sel)) break;
        }
        const U T = (U)st.prefix;
        __syncthreads();
        if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
        for (uint32_t i = threadIdx.x; i < m; i += SB) cand[i] = lo;
        __syncthreads();
        Keep<U, KIND> keep{T, m, c > k ? st.k + 1 : 0u, c <= k, s_cnt, cand, false};
        sweep_rows<U>(x, lo, hi, [&](U raw, uint32_t p, bool live) { keep.row(raw, p, live); });
        __syncthreads();
        rank_emit<U, KIND>(x, cand, keys, m, (size_t)g * k, vals, pos_out);
        maxp = st.passes + 1 > maxp ? st.passes + 1 : maxp;                      // the digit passes and the collecting one
    }
    if (threadIdx.x == 0 && maxp) atomicMax(&ctl[CTL_PASSES], maxp);
}

// ---- SPLIT ----------------------------------------------------------------------------------------------------------------------------------
// between digits (as select_split_choose_kernel): the finished state keeps T in prefix and the rank among the rows equal to T in k
template <class U>
__global__ void __launch_bounds__(SB) topk_split_choose_kernel(SelState* __restrict__ sst, uint32_t* __restrict__ ctl, uint32_t* __restrict__ ghist) {
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
            if (done) st.done = DONE_KEY;
            st.vand = ~0ull; st.vor = 0ull;
            sst[s] = st;
        }
    }
}
// the collect pass over the chunks: positions -> cand[s * k ...) (HBM), counted by the group's two cursors cur[2 s], cur[2 s + 1]
template <class U, int KIND>
__global__ void __launch_bounds__(SB) topk_split_collect_kernel(const U* __restrict__ x, const SelState* __restrict__ sst, const uint32_t* __restrict__ ctl, uint32_t k,
                                                                 uint32_t* __restrict__ cur, uint32_t* __restrict__ cand) {
    uint32_t q0, q1, s, ns;
    if (!split_span(sst, ctl, q0, q1, s, ns)) return;
    for (uint32_t q = q0; q < q1; ++q) {
        while (s + 1 < ns && sst[s + 1].cbase <= q) ++s;
        const uint32_t glo = sst[s].lo, ghi = sst[s].hi, done = sst[s].done;
        if (!done) continue;                                // (cannot happen: sizeof(U) digit rounds finish every selection)
        const uint32_t lo = glo + (q - sst[s].cbase) * SPLIT_CHUNK, hi = ghi - lo < SPLIT_CHUNK ? ghi : lo + SPLIT_CHUNK;
        const bool all = done == DONE_ALL;
        const uint32_t m = min_u32(k, ghi - glo), need = all ? 0u : min_u32(sst[s].k + 1, m);
        Keep<U, KIND> keep{(U)sst[s].prefix, m, need, all, cur + 2 * (size_t)s, cand + (size_t)s * k, false};
        keep.full = !all && __shfl(__hip_atomic_load(&cur[2 * (size_t)s + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0, 64) >= need;
        sweep_rows<U>(x, lo, hi, [&](U raw, uint32_t p, bool live) { keep.row(raw, p, live); });
    }
}
// one workgroup per SPLIT group ranks its candidates and writes them out
template <class U, int KIND>
__global__ void __launch_bounds__(SB) topk_split_emit_kernel(const U* __restrict__ x, const SelState* __restrict__ sst, uint32_t* __restrict__ ctl, uint32_t k,
                                                              const uint32_t* __restrict__ candg, U* __restrict__ vals, uint32_t* __restrict__ pos_out) {
    __shared__ uint32_t cand[KMAX];
    __shared__ U keys[KMAX];
    const uint32_t ns = ctl[CTL_NSPLIT];
    for (uint32_t s = blockIdx.x; s < ns; s += gridDim.x) {
        const uint32_t m = min_u32(k, sst[s].hi - sst[s].lo);
        if (!sst[s].done) continue;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < m; i += SB) cand[i] = candg[(size_t)s * k + i];
        __syncthreads();
        rank_emit<U, KIND>(x, cand, keys, m, (size_t)sst[s].gidx * k, vals, pos_out);
        if (threadIdx.x == 0) atomicMax(&ctl[CTL_PASSES], sst[s].passes + 1);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
size_t topk_ws_bytes(uint32_t n, uint32_t G, uint32_t k, SelSwitches sw) {
    return select_ws_bytes(n, G, sw) + (size_t)split_cap(n, G, sw.split_min) * ((size_t)k * 4 + 8) + 1024;
}
// the three routes over a column in the flat layout (workspace sized by topk_ws_bytes and not reset in here; the control words are zero)
template <class U, int KIND>
int run_topk(aqg_ctx* ctx, const SelInput& in, uint32_t k, SelSwitches sw, void* valsv, uint32_t* pos_out) {
    const U* x = static_cast<const U*>(in.x);
    U* vals = static_cast<U*>(valsv);
    uint32_t* ctl = ctx->select_ctl;
    SelPlan p;
    AQG_TRY(p.init(ctx, in.n, in.G, sw, NHIST<U>));
    uint32_t *cur, *cand;
    AQG_TRY(aqg_ws_get(ctx, (size_t)p.scap * 2, &cur));
    AQG_TRY(aqg_ws_get(ctx, (size_t)p.scap * k, &cand));
    // the slots no row fills: zero bytes and the missing-row marker
    AQG_HIP(ctx, hipMemsetAsync(vals, 0, (size_t)in.G * k * sizeof(U), ctx->stream));
    if (pos_out) AQG_HIP(ctx, hipMemsetAsync(pos_out, 0xFF, (size_t)in.G * k * 4, ctx->stream));
    if (p.do_split) {
        AQG_HIP(ctx, hipMemsetAsync(cur, 0, (size_t)p.scap * 8, ctx->stream));
        AQG_HIP(ctx, hipMemsetAsync(cand, 0, (size_t)p.scap * k * 4, ctx->stream));        // (a slot no row took would still be a position of the column)
    }
    hipLaunchKernelGGL(topk_classify_kernel, dim3(p.ggrid), dim3(SB), 0, ctx->stream, in.off, in.G, sw.small_max, sw.split_min, k, (int)sizeof(U) * 8, p.tile_first, p.glist, p.sst, ctl);
    aqg_kernel_timer_begin(ctx);
    if (p.do_small) hipLaunchKernelGGL((topk_small_kernel<U, KIND>), dim3(p.ntiles), dim3(SB), 0, ctx->stream, x, in.n, in.off, in.G, p.tile_first, sw.small_max, k, vals, pos_out);
    if (p.do_group) hipLaunchKernelGGL((topk_group_kernel<U, KIND>), dim3(p.wgrid), dim3(SB), 0, ctx->stream, x, in.off, p.glist, ctl, k, vals, pos_out);
    if (p.do_split) {
        hipLaunchKernelGGL(select_split_plan_kernel, dim3(1), dim3(SB), 0, ctx->stream, p.sst, ctl);
        for (size_t d = 0; d < sizeof(U); ++d) {
            hipLaunchKernelGGL((select_split_hist_kernel<U, KIND>), dim3(p.hgrid), dim3(SB), 0, ctx->stream, x, p.sst, ctl, p.ghist);
            hipLaunchKernelGGL((topk_split_choose_kernel<U>), dim3(p.cgrid), dim3(SB), 0, ctx->stream, p.sst, ctl, p.ghist);
        }
        hipLaunchKernelGGL((topk_split_collect_kernel<U, KIND>), dim3(p.hgrid), dim3(SB), 0, ctx->stream, x, p.sst, ctl, k, cur, cand);
        hipLaunchKernelGGL((topk_split_emit_kernel<U, KIND>), dim3(p.cgrid), dim3(SB), 0, ctx->stream, x, p.sst, ctl, k, cand, vals, pos_out);
    }
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "top-k selection");
}
template <class U, int KIND>
int run_topk_order(aqg_ctx* ctx, int order, const SelInput& in, uint32_t k, SelSwitches sw, void* vals, uint32_t* pos_out) {
    if (order == AQG_ORDER_DESC) return run_topk<U, KIND | KIND_DESC>(ctx, in, k, sw, vals, pos_out);
    return run_topk<U, KIND>(ctx, in, k, sw, vals, pos_out);
}
int dispatch_topk(aqg_ctx* ctx, int order, int t, const SelInput& in, uint32_t k, SelSwitches sw, void* vals, uint32_t* pos_out) {
    return dispatch_kind(t, [&]<class U, int KIND>() { return run_topk_order<U, KIND>(ctx, order, in, k, sw, vals, pos_out); });
}
int check_args(aqg_ctx* ctx, int order, int t, uint32_t k) {
    if (order != AQG_ORDER_ASC && order != AQG_ORDER_DESC) return aqg_fail(ctx, AQG_ERR_ARG, "top-k: order must be AQG_ORDER_ASC or AQG_ORDER_DESC");
    if (k < 1 || k > KMAX) return aqg_fail(ctx, AQG_ERR_ARG, "top-k: 1 <= k <= AQG_TOPK_MAX");
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "top-k: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    return AQG_OK;
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g, int order, int t, const void* x, uint32_t k, const void* vals) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped top-k: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped top-k: the handle was not made by aqg_groupby_build");
    AQG_TRY(check_args(ctx, order, t, k));
    if ((!x || !vals) && g->n) return aqg_fail(ctx, AQG_ERR_ARG, "grouped top-k: null column");
    return AQG_OK;
}

int grouped_topk(aqg_ctx* ctx, aqg_groupby* g, int order, int t, const void* x, bool row_layout, uint32_t k, void* vals, uint32_t* pos_out) {
    AQG_TRY(check_grouped(ctx, g, order, t, x, k, vals));
    const SelSwitches sw = select_switches();
    SelInput in;
    AQG_TRY(select_prologue(ctx, g, x, g->n, esz_of(t), topk_ws_bytes(g->n, g->ngroups, k, sw), row_layout, &in));
    if (!in.G) return AQG_OK;
    return dispatch_topk(ctx, order, t, in, k, sw, vals, pos_out);
}

} // namespace

extern "C" {

int aqg_topk(aqg_ctx* ctx, int order, int t, const void* x, uint32_t n, uint32_t k, void* vals_out_dev, uint32_t* rows_out_dev) {
    if (!ctx || !vals_out_dev) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_topk: bad argument");
    AQG_TRY(check_args(ctx, order, t, k));
    if (!x && n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_topk: null column");
    AQG_CHECK_ROWS(ctx, n, "aqg_topk");
    const SelSwitches sw = select_switches();
    SelInput in;
    AQG_TRY(select_prologue(ctx, nullptr, x, n, esz_of(t), topk_ws_bytes(n, 1, k, sw), false, &in));
    if (!in.G) {                                            // no row: k empty slots
        AQG_HIP(ctx, hipMemsetAsync(vals_out_dev, 0, (size_t)k * esz_of(t), ctx->stream));
        if (rows_out_dev) AQG_HIP(ctx, hipMemsetAsync(rows_out_dev, 0xFF, (size_t)k * 4, ctx->stream));
        return AQG_OK;
    }
    return dispatch_topk(ctx, order, t, in, k, sw, vals_out_dev, rows_out_dev);
}

int aqg_grouped_topk_flat(aqg_ctx* ctx, aqg_groupby* g, int order, int t, const void* xflat, uint32_t k, void* vals_out_dev, uint32_t* pos_out_dev) {
    return grouped_topk(ctx, g, order, t, xflat, /*row_layout=*/false, k, vals_out_dev, pos_out_dev);
}

int aqg_grouped_topk(aqg_ctx* ctx, aqg_groupby* g, int order, int t, const void* x, uint32_t k, void* vals_out_dev, uint32_t* pos_out_dev) {
    return grouped_topk(ctx, g, order, t, x, /*row_layout=*/true, k, vals_out_dev, pos_out_dev);
}

} // extern "C"
