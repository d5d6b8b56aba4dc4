// distinct.hip -- aqg_count_distinct / aqg_grouped_count_distinct(_flat): count(distinct x) of a column and of every group's slice of the
// flat layout (`(x).distinct_size()`, reference common/types.py:271-277; under GROUP BY `(x[val]).distinct_size()` inside the generated
// loop, engine/ast.py:749-784; the reference builds a std::unordered_set per call, server/vector_type.hpp:153-174, server/table.h:328-332).
//
// Equality is the reference's ==: integers and BOOL by value; floating columns through img_fp (key_image.hpp), so -0.0 and +0.0 are one
// value, and every NaN ROW counts as a value of its own (NaN != NaN: the set keeps them all).
// One algorithm, two phases, no per-group routes; the launches do not depend on the group count.
//   phase 1  a workgroup owns a tile of TILE consecutive flat positions: images and group ordinals (the group's index within the tile)
//            staged in LDS, (ordinal, image) pairs deduplicated in an LDS open-addressing table whose slots hold ROW POSITIONS -- a lane
//            that meets a claimed slot compares with the claimant through the staged arrays.  A claiming row and a NaN row add 1 to their
//            ordinal's counter.  A group wholly inside the tile gets its count by a plain store; a group that crosses a tile edge (at most
//            the first and the last of a tile) adds its NaN rows to out[g] and appends its claiming rows as (group, image) pairs to a list
//   phase 2  (only when pairs were written: one host round trip reads their number) the pairs go through the group-by planner as a
//            count-only group-by; every resulting pair group adds 1 to out[group]
// `out` is zeroed first and every update is a store to a group no other tile writes or an integer add: the result does not depend on
// the order the pairs land in.
#include "groupby_handle.hpp"
#include "select_dev.hpp"

namespace {
using namespace seldev;

constexpr int SB = 256;                        // lanes per workgroup
constexpr int NWV = SB / 64;
constexpr uint32_t TILE = 2048;                // flat positions per workgroup (8-byte columns: 44 KiB of LDS, three workgroups per CU)
constexpr uint32_t PER = TILE / SB;            // rows per lane
constexpr uint32_t SLOTS = 2 * TILE;           // the table's load never passes 0.5: a tile cannot overflow it
constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t HW = TILE / 32;             // words of the tile's bitmap of group starts
static_assert(HW == 64, "one wavefront scans the bitmap of group starts");
// control words of a call (device, owned by the context): read back by aqg_distinct_last
enum { CTL_PAIRS = 0, CTL_CROSS = 1, CTL_OFF = 2 /* offsets {0, n} of the flat call */, CTL_RESULT = 4, CTL_WORDS = 8 };

__device__ inline uint32_t slot_hash(uint64_t im, uint32_t o) {
    return (uint32_t)(((im + (uint64_t)o * 0x9E3779B97F4A7C15ull) * 0xBF58476D1CE4E5B9ull) >> 40) & (SLOTS - 1);
}

// tile_first[t] = the group that holds flat position t * TILE (the last g with off[g] <= t * TILE): one lane per tile
__global__ void __launch_bounds__(SB) distinct_tile_first_kernel(const uint32_t* __restrict__ off, uint32_t G, uint32_t ntiles, uint32_t* __restrict__ tile_first) {
    for (uint32_t t = blockIdx.x * SB + threadIdx.x; t < ntiles; t += gridDim.x * SB) {
        const uint32_t tbeg = t * TILE;
        uint32_t l = 0, r = G;
        while (r - l > 1) { const uint32_t m = l + (r - l) / 2; if (off[m] <= tbeg) l = m; else r = m; }
        tile_first[t] = l;
    }
}

template <class U, bool FP>
__global__ void __launch_bounds__(SB) distinct_tile_kernel(const U* __restrict__ x, uint32_t n, const uint32_t* __restrict__ off, uint32_t G,
                                                            const uint32_t* __restrict__ tile_first, uint32_t* __restrict__ out,
                                                            uint32_t* __restrict__ pair_gid, U* __restrict__ pair_img, uint32_t* __restrict__ ctl) {
    constexpr uint32_t V = 16 / sizeof(U), NV = (TILE / V + SB - 1) / SB;
    __shared__ U img[TILE];
    __shared__ uint16_t ord[TILE];
    __shared__ uint32_t slot[SLOTS];
    __shared__ uint32_t cnt[TILE + 2];           // claims + NaN rows per ordinal; [TILE], [TILE + 1]: NaN rows of the first / last group when it crosses the tile's edge
    __shared__ uint32_t hb[HW], hpre[HW];        // bit i: a group starts at tile position i (i > 0) / set bits in the words before
    __shared__ uint32_t wsum[NWV];
    __shared__ uint32_t s_ng, s_base, s_end;
    const uint32_t tbeg = blockIdx.x * TILE, L = n - tbeg < TILE ? n - tbeg : TILE, tend = tbeg + L;
    const uint32_t g0 = tile_first[blockIdx.x];
    // the tile's rows are asked for first, so that their way from HBM overlaps the walk over the offsets: 16-byte loads over the aligned
    // middle, the up to 2 (V - 1) elements around it a lane each
    const U* xt = x + tbeg;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(xt) & 15);
    const uint32_t lead = mis ? (16 - mis) / (uint32_t)sizeof(U) : 0u, hl = lead < L ? lead : L;
    const uint32_t nvec = (L - hl) / V, ts = hl + nvec * V, tl = L - ts;
    const bool edge = threadIdx.x < hl + tl;
    const uint32_t ei = !edge ? 0u : threadIdx.x < hl ? threadIdx.x : ts + (threadIdx.x - hl);
    const U eraw = xt[ei];
    vec16<U> r[NV];
    if (nvec) {
        const vec16<U>* xv = reinterpret_cast<const vec16<U>*>(xt + hl);
#pragma unroll
        for (uint32_t u = 0; u < NV; ++u) { const uint32_t vi = u * SB + threadIdx.x; r[u] = xv[vi < nvec ? vi : nvec - 1]; }
    }
    const uint32_t first_off = off[g0];
    for (uint32_t i = threadIdx.x; i < SLOTS; i += SB) slot[i] = EMPTY;
    for (uint32_t i = threadIdx.x; i < TILE + 2; i += SB) cnt[i] = 0;
    if (threadIdx.x < HW) hb[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_end = 0xFFFFFFFFu;
    __syncthreads();
    // the groups that start inside the tile, behind its first position; the first offset at or beyond the tile's end is where its last group ends
    for (uint32_t base = 0;; base += SB) {
        const uint32_t gi = g0 + 1 + base + threadIdx.x;
        const uint32_t o = gi < G ? off[gi] : n;
        const bool beyond = gi >= G || o >= tend;
        if (!beyond) atomicOr(&hb[(o - tbeg) >> 5], 1u << ((o - tbeg) & 31));
        const uint64_t bm = __ballot(beyond);
        if (bm && lane_id() == __ffsll((long long)bm) - 1) atomicMin(&s_end, o);
        if (__syncthreads_or(beyond)) break;
    }
    if (threadIdx.x < HW) {
        const uint32_t c = __popc(hb[threadIdx.x]);
        const uint32_t incl = wave_scan_incl(c, OpAdd{}, (int)threadIdx.x);
        hpre[threadIdx.x] = incl - c;
        if (threadIdx.x == HW - 1) s_ng = incl + 1;
    }
    __syncthreads();
    const uint32_t ng = s_ng, glast = g0 + ng - 1;
    const bool cross_first = first_off < tbeg, cross_last = s_end > tend;
    // images and ordinals of rows [tbeg, tend) -> LDS
    auto put = [&](uint32_t i, U raw) {
        if constexpr (FP) img[i] = img_fp<U>(raw);
        else img[i] = raw;
        ord[i] = (uint16_t)(hpre[i >> 5] + __popc(hb[i >> 5] & (0xFFFFFFFFu >> (31 - (i & 31)))));
    };
    if (edge) put(ei, eraw);
    if (nvec) {
#pragma unroll
        for (uint32_t u = 0; u < NV; ++u) {
            const uint32_t vi = u * SB + threadIdx.x;
            if (vi < nvec) {
#pragma unroll
                for (uint32_t e = 0; e < V; ++e) put(hl + vi * V + e, r[u].v[e]);
            }
        }
    }
    __syncthreads();        // staging is complete: a claimed position is readable from here on
    uint32_t claimed = 0;   // bit k: row k * SB + lane of a crossing group claimed its slot (it becomes a pair)
#pragma unroll 1
    for (uint32_t k = 0; k < PER; ++k) {
        const uint32_t i = k * SB + threadIdx.x;
        const bool live = i < L;
        const U im = img[live ? i : 0];
        const uint32_t o = ord[live ? i : 0];
        bool nan = false, mine = false;
        if constexpr (FP) nan = im == img_fp_nan<U>();
        if (live && !nan) {
            uint32_t h = slot_hash((uint64_t)im, o);
            for (;;) {
                uint32_t cur = reinterpret_cast<volatile uint32_t*>(slot)[h];
                if (cur == EMPTY) cur = atomicCAS(&slot[h], EMPTY, i);
                if (cur == EMPTY) { mine = true; break; }
                if (ord[cur] == o && img[cur] == im) break;
                h = (h + 1) & (SLOTS - 1);
            }
        }
        const bool at_first = o == 0 && cross_first, cross = at_first || (o == ng - 1 && cross_last);
        hist_add(cnt, nan && cross ? TILE + (at_first ? 0u : 1u) : o, live && (mine || nan));
        if (mine && cross) claimed |= 1u << k;
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < ng; j += SB) {
        const bool cross = (j == 0 && cross_first) || (j == ng - 1 && cross_last);
        if (!cross) out[g0 + j] = cnt[j];
    }
    if (!cross_first && !cross_last) return;
    const uint32_t mine_n = __popc(claimed);
    const uint32_t incl = block_scan_incl(mine_n, wsum);
    if (threadIdx.x == SB - 1) s_base = incl ? atomicAdd(&ctl[CTL_PAIRS], incl) : 0u;
    __syncthreads();
    uint32_t p = s_base + incl - mine_n;
    for (uint32_t k = 0; k < PER; ++k) {
        if (claimed >> k & 1) {
            const uint32_t i = k * SB + threadIdx.x;
            pair_gid[p] = g0 + ord[i];
            pair_img[p] = img[i];
            ++p;
        }
    }
    if (threadIdx.x == 0) {
        if (cnt[TILE]) atomicAdd(&out[g0], cnt[TILE]);
        if (cnt[TILE + 1]) atomicAdd(&out[glast], cnt[TILE + 1]);
        if (cross_last && !(ng == 1 && cross_first)) atomicAdd(&ctl[CTL_CROSS], 1u);      // a crossing group is counted by the tile it starts in
    }
}

// phase 2: every distinct (group, image) pair of the crossing groups is one more value of its group.  The pair groups come out clustered
// by group (first occurrence in a list that tiles wrote in turn), so a wavefront walks one contiguous span and adds once per RUN of equal
// groups -- a run that reaches the end of a step is carried into the next -- instead of once per pair onto a handful of addresses
__global__ void __launch_bounds__(SB) distinct_add_pairs_kernel(const uint32_t* __restrict__ gid, uint32_t m, uint32_t* __restrict__ out) {
    const uint32_t nw = gridDim.x * NWV, w = blockIdx.x * NWV + wave_id(), lane = lane_id();
    const uint32_t per = ((m + nw - 1) / nw + 63) & ~63u;
    const uint64_t lo64 = (uint64_t)w * per;
    if (lo64 >= m) return;
    const uint32_t lo = (uint32_t)lo64, hi = lo64 + per < m ? lo + per : m;
    uint32_t cg = 0xFFFFFFFFu, cc = 0;                  // the carried run (the same in every lane)
    for (uint32_t b = lo; b < hi; b += 64) {
        const uint32_t nlive = hi - b < 64 ? hi - b : 64;
        const bool live = lane < nlive;
        const uint32_t g = gid[live ? b + lane : hi - 1];
        const uint32_t prev = __shfl_up(g, 1, 64);
        const bool head = live && g != (lane == 0 ? cg : prev);
        const uint64_t mask = __ballot(head);
        if (mask == 0) { cc += nlive; continue; }
        const uint32_t f = (uint32_t)__ffsll((long long)mask) - 1, last = 63 - (uint32_t)__clzll((long long)mask);
        if (lane == 0 && cc + f) atomicAdd(&out[cg], cc + f);
        if (head && lane != last) {
            const uint64_t higher = mask & ~((2ull << lane) - 1);
            atomicAdd(&out[g], (uint32_t)__ffsll((long long)higher) - 1 - lane);
        }
        cg = __shfl(g, (int)last, 64);
        cc = nlive - last;
    }
    if (lane == 0 && cc) atomicAdd(&out[cg], cc);
}
__global__ void distinct_add_kernel(uint32_t* out, uint32_t v) { *out += v; }

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
size_t distinct_ws_bytes(uint32_t n) { return ((size_t)aqg_ceil_div(n, TILE) + 1) * 4 + 4096; }
int ensure_ctl(aqg_ctx* ctx) {
    if (!ctx->distinct_ctl) AQG_HIP(ctx, aqg_scratch_malloc(ctx, &ctx->distinct_ctl, 256));
    AQG_HIP(ctx, hipMemsetAsync(ctx->distinct_ctl, 0, CTL_WORDS * 4, ctx->stream));
    return AQG_OK;
}
// the pair list of a call, worst case one pair per row: it outlives the context's workspace, which belongs to the planner in phase 2.
// Grow-only, owned by the context: no allocation in steady state
int ensure_pairs(aqg_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->distinct_pairs_cap) return AQG_OK;
    AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->distinct_pairs) { (void)hipFree(ctx->distinct_pairs); ctx->distinct_pairs = nullptr; ctx->distinct_pairs_cap = 0; }
    void* p = nullptr;
    const hipError_t e = aqg_scratch_malloc(ctx, &p, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); ctx->err = std::string("count distinct: pair list: ") + hipGetErrorString(e); return AQG_ERR_NOMEM; }
    ctx->distinct_pairs = p;
    ctx->distinct_pairs_cap = bytes;
    return AQG_OK;
}

// both phases over a column in the flat layout (the workspace holds distinct_ws_bytes(n) and is not reset in here; the control words are zero).
// head: the control words as the host read them behind phase 1
template <class U, bool FP>
int run_distinct(aqg_ctx* ctx, const void* xv, uint32_t n, const uint32_t* off, uint32_t G, aqg_groupby** scratch, uint32_t* out, uint32_t* head) {
    const U* x = static_cast<const U*>(xv);
    uint32_t* ctl = ctx->distinct_ctl;
    const uint32_t ntiles = aqg_ceil_div(n, TILE);
    const size_t img_at = ((size_t)n * 4 + 255) & ~(size_t)255;
    AQG_TRY(ensure_pairs(ctx, img_at + (size_t)n * sizeof(U) + 256));
    uint32_t* pair_gid = static_cast<uint32_t*>(ctx->distinct_pairs);
    U* pair_img = reinterpret_cast<U*>(static_cast<char*>(ctx->distinct_pairs) + img_at);
    uint32_t* tile_first;
    AQG_TRY(aqg_ws_get(ctx, (size_t)ntiles + 1, &tile_first));
    AQG_HIP(ctx, hipMemsetAsync(out, 0, (size_t)G * 4, ctx->stream));
    hipLaunchKernelGGL(distinct_tile_first_kernel, dim3(aqg_grid(ctx, ntiles, SB, 1, 8)), dim3(SB), 0, ctx->stream, off, G, ntiles, tile_first);
    aqg_kernel_timer_begin(ctx);
    hipLaunchKernelGGL((distinct_tile_kernel<U, FP>), dim3(ntiles), dim3(SB), 0, ctx->stream, x, n, off, G, tile_first, out, pair_gid, pair_img, ctl);
    aqg_kernel_timer_end(ctx);
    AQG_TRY(aqg_check_launch(ctx, "count distinct: tile pass"));
    AQG_TRY(aqg_d2h(ctx, head, ctl, CTL_WORDS * 4));    // the call's one host round trip (the flat call's result rides along: final when no pairs were left)
    const uint32_t m = head[CTL_PAIRS];
    if (m == 0) return AQG_OK;
    // the crossing groups' pairs through the planner, count only.  One group (the flat call): the images alone
    constexpr int img_dt = sizeof(U) == 1 ? AQG_UINT8 : sizeof(U) == 2 ? AQG_UINT16 : sizeof(U) == 4 ? AQG_UINT32 : AQG_UINT64;
    const int dts[2] = {AQG_UINT32, img_dt};
    const void* cols[2] = {pair_gid, pair_img};
    const bool frozen = ctx->evk_frozen;
    ctx->evk_frozen = true;                              // the tile pass stays the timed kernel of the call
    const int rc = G == 1 ? aqg_groupby_agg(ctx, 1, dts + 1, cols + 1, 0, nullptr, nullptr, nullptr, m, 0, scratch)
                          : aqg_groupby_agg(ctx, 2, dts, cols, 0, nullptr, nullptr, nullptr, m, 0, scratch);
    ctx->evk_frozen = frozen;
    AQG_TRY(rc);
    const uint32_t pg = (*scratch)->ngroups;
    if (G == 1) hipLaunchKernelGGL(distinct_add_kernel, dim3(1), dim3(1), 0, ctx->stream, out, pg);
    else hipLaunchKernelGGL(distinct_add_pairs_kernel, dim3(aqg_grid(ctx, pg, SB, 16, 8)), dim3(SB), 0, ctx->stream, static_cast<const uint32_t*>((*scratch)->keys_out[0]), pg, out);
    return aqg_check_launch(ctx, "count distinct: pair groups");
}
// integers and BOOL compare by their bits: one instantiation per width
int dispatch_distinct(aqg_ctx* ctx, int t, const void* x, uint32_t n, const uint32_t* off, uint32_t G, aqg_groupby** scratch, uint32_t* out, uint32_t* head) {
    switch (t) {
    case AQG_FLOAT: return run_distinct<uint32_t, true>(ctx, x, n, off, G, scratch, out, head);
    case AQG_DOUBLE: return run_distinct<uint64_t, true>(ctx, x, n, off, G, scratch, out, head);
    }
    switch (esz_of(t)) {
    case 1: return run_distinct<uint8_t, false>(ctx, x, n, off, G, scratch, out, head);
    case 2: return run_distinct<uint16_t, false>(ctx, x, n, off, G, scratch, out, head);
    case 4: return run_distinct<uint32_t, false>(ctx, x, n, off, G, scratch, out, head);
    case 8: return run_distinct<uint64_t, false>(ctx, x, n, off, G, scratch, out, head);
    }
    return AQG_ERR_DTYPE;
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g, int t, const void* x, const void* out) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped count distinct: bad argument");
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "grouped count distinct: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped count distinct: the handle was not made by aqg_groupby_build");
    if ((!x || !out) && g->n) return aqg_fail(ctx, AQG_ERR_ARG, "grouped count distinct: null column");
    return AQG_OK;
}

} // namespace

extern "C" {

int aqg_count_distinct(aqg_ctx* ctx, int t, const void* x, uint32_t n, uint32_t* out_host) {
    if (!ctx || !out_host) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_count_distinct: bad argument");
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_count_distinct: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    if (!x && n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_count_distinct: null column");
    AQG_CHECK_ROWS(ctx, n, "aqg_count_distinct");
    AQG_TRY(ensure_ctl(ctx));
    if (n == 0) { *out_host = 0; return AQG_OK; }
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, distinct_ws_bytes(n)));
    uint32_t* ctl = ctx->distinct_ctl;
    hipLaunchKernelGGL(flat_offsets_kernel, dim3(1), dim3(1), 0, ctx->stream, ctl + CTL_OFF, n);
    uint32_t head[CTL_WORDS];
    uint32_t count = 0;
    AQG_TRY(dispatch_distinct(ctx, t, x, n, ctl + CTL_OFF, 1, &ctx->distinct_scratch, ctl + CTL_RESULT, head));
    if (head[CTL_PAIRS] == 0) count = head[CTL_RESULT];
    else AQG_TRY(aqg_d2h(ctx, &count, ctl + CTL_RESULT, 4));
    *out_host = count;
    return AQG_OK;
}

int aqg_grouped_count_distinct_flat(aqg_ctx* ctx, aqg_groupby* g, int t, const void* xflat, uint32_t* out_dev) {
    AQG_TRY(check_grouped(ctx, g, t, xflat, out_dev));
    AQG_TRY(ensure_ctl(ctx));
    const uint32_t n = g->n, G = g->ngroups;
    if (n == 0 || G == 0) return AQG_OK;
    const uint32_t* off = aqg_groupby_offsets(g);
    if (!off) return AQG_ERR_HIP;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, distinct_ws_bytes(n)));
    uint32_t head[CTL_WORDS];
    return dispatch_distinct(ctx, t, xflat, n, off, G, &g->scratch3, out_dev, head);
}

int aqg_grouped_count_distinct(aqg_ctx* ctx, aqg_groupby* g, int t, const void* x, uint32_t* out_dev) {
    AQG_TRY(check_grouped(ctx, g, t, x, out_dev));
    AQG_TRY(ensure_ctl(ctx));
    const uint32_t n = g->n, G = g->ngroups;
    if (n == 0 || G == 0) return AQG_OK;
    const uint32_t* off = aqg_groupby_offsets(g);
    if (!off) return AQG_ERR_HIP;
    const int esz = esz_of(t);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * esz + 4096 + aqg_postproc_ws_bytes(n, G, esz) + distinct_ws_bytes(n)));
    unsigned char* xs;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n * esz + 64, &xs));
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x, esz, xs, /*ws_managed=*/true));
    uint32_t head[CTL_WORDS];
    return dispatch_distinct(ctx, t, xs, n, off, G, &g->scratch3, out_dev, head);
}

int aqg_distinct_last(aqg_ctx* ctx, uint32_t* tile_rows, uint32_t* crossing_groups, uint64_t* pairs) {
    if (!ctx || !tile_rows || !crossing_groups || !pairs) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_distinct_last: bad argument");
    uint32_t w[2] = {0, 0};
    if (ctx->distinct_ctl) AQG_TRY(aqg_d2h(ctx, w, ctx->distinct_ctl, 8));
    *tile_rows = TILE;
    *crossing_groups = w[CTL_CROSS];
    *pairs = w[CTL_PAIRS];
    return AQG_OK;
}

} // extern "C"
