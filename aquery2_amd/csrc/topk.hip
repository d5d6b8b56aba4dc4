// topk.hip -- aqg_topk / aqg_grouped_topk(_flat): the k largest or k smallest elements of a column and of every group's slice of the flat
// layout, in order, with their positions (h2o Q8 `largest two v3 by id6`, benchmark/h2o/groupby.sql:16-17; ORDER BY x DESC LIMIT k).
//
// A selection, not a sort: rows are never moved.  Every row is compared through its KEY: the order-preserving image of key_image.hpp under
// AQG_ORDER_ASC, its complement under AQG_ORDER_DESC, so that both orders are "the m = min(k, c) smallest keys of the c rows, ties by
// ascending position".  The three routes and their thresholds are those of select.hip (select_dev.hpp), chosen per group on the device:
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
#include "groupby_handle.hpp"
#include "select_radix.hpp"

namespace {
using namespace selradix;

constexpr uint32_t KMAX = AQG_TOPK_MAX;
static_assert(KMAX % SB == 0 && SMALL_CAP <= KMAX, "the candidates of a group are ranked SB at a time; a SMALL group fits its own slots");
constexpr uint32_t DONE_KEY = 1, DONE_ALL = 3;          // SelState::done of a SPLIT group: T is st.prefix / every row is taken

__device__ inline uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// rows [lo, hi) (lo < hi) of x through f(raw, position, live), every lane of the workgroup calling f the same number of times: 16-byte loads
// over the aligned middle of the slice, UNR of them in flight per lane, the elements in front of and behind it one lane each (as hist_rows)
template <class U, class F>
__device__ inline void sweep_rows(const U* __restrict__ x, uint32_t lo, uint32_t hi, F&& f) {
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

// ---- routing: one lane per group (as select_classify_kernel; the rank wanted is the last of the m kept rows) -------------------------------
__global__ void __launch_bounds__(SB) topk_classify_kernel(const uint32_t* __restrict__ off, uint32_t G, uint32_t small_max, uint32_t split_min, uint32_t k, int bits,
                                                            uint32_t* __restrict__ tile_first, uint32_t* __restrict__ glist, SelState* __restrict__ sst, uint32_t* __restrict__ ctl) {
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
            SelState st{};
            st.vand = ~0ull;
            st.lo = lo; st.hi = hi; st.k = min_u32(k, c) - 1; st.gidx = g;
            st.shift = (uint32_t)bits - 8;
            st.done = c <= k ? DONE_ALL : 0u;
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
__global__ void __launch_bounds__(SB) topk_small_kernel(const U* __restrict__ x, uint32_t n, const uint32_t* __restrict__ off, uint32_t G,
                                                         const uint32_t* __restrict__ tile_first, uint32_t small_max, uint32_t k, U* __restrict__ vals, uint32_t* __restrict__ pos_out) {
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
    auto put = [&](uint32_t gi, uint32_t slot, uint32_t p) {
        const size_t o = (size_t)(g0 + gi) * k + slot;
        vals[o] = x[p];
        if (pos_out) pos_out[o] = p;
    };
    // one or two rows: a lane each, from the column itself
    bool any = false;
    for (uint32_t gi = threadIdx.x; gi < ng; gi += SB) {
        const uint32_t lo = goff[gi], c = goff[gi + 1] - lo;
        if (c > small_max || c == 0) continue;
        if (c == 1) put(gi, 0, lo);
        else if (c == 2) {
            const uint32_t second = image_of<U, KIND>(x[lo + 1]) < image_of<U, KIND>(x[lo]) ? 0u : 1u;     // (equal keys: positions ascend)
            put(gi, 0, lo + 1 - second);
            if (k > 1) put(gi, 1, lo + second);
        } else any = true;
    }
    if (!__syncthreads_or(any)) return;
    // keys of rows [tbeg, tbeg + ROWS) -> LDS
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
    // a wavefront per group: rank of every row = rows that sort before it (ties by position); the rows of rank below m are the answer
    const uint32_t lane = lane_id();
    for (uint32_t gi = wave_id(); gi < ng; gi += NWV) {
        const uint32_t lo = goff[gi], c = goff[gi + 1] - lo;
        if (c < 3 || c > small_max) continue;
        const uint32_t base = lo - tbeg, m = min_u32(k, c);
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
            if (live && less < m) put(gi, less, lo + ii);
        }
    }
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
        U T = 0;
        while (c > k) {                                                         // the key of rank m - 1; st.k ends as that rank among the rows equal to it
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
            if (st.vand == st.vor) { T = (U)st.vand; break; }                   // one candidate, or all of them equal
            choose_bin(h[threadIdx.x], st.k, wsum, &sel);
            if (both_digits_known<U>(st, sel.cnt, sel.total)) {
                __syncthreads();
                choose_bin(h[256 * (NHIST<U> - 1) + threadIdx.x], st.k, wsum, &sel);
                T = (U)((st.vand & ~0xFFull) | sel.bin);
                st.k -= sel.excl;
                break;
            }
            if (sel_advance(st, sel.bin, sel.excl, sel.cnt, sel.total)) { T = (U)st.prefix; break; }
        }
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
        bool done;
        if (st.vand == st.vor) { st.prefix = st.vand; done = true; }
        else {
            choose_bin(c, st.k, wsum, &sel);
            if (both_digits_known<U>(st, sel.cnt, sel.total)) {
                __syncthreads();
                choose_bin(c2, st.k, wsum, &sel);
                st.prefix = (st.vand & ~0xFFull) | sel.bin;
                st.k -= sel.excl;
                done = true;
            } else done = sel_advance(st, sel.bin, sel.excl, sel.cnt, sel.total);
        }
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
int run_topk(aqg_ctx* ctx, const void* xv, uint32_t n, const uint32_t* off, uint32_t G, uint32_t k, SelSwitches sw, void* valsv, uint32_t* pos_out) {
    const U* x = static_cast<const U*>(xv);
    U* vals = static_cast<U*>(valsv);
    uint32_t* ctl = ctx->select_ctl;
    const uint32_t ntiles = aqg_ceil_div(n, TILE), scap = split_cap(n, G, sw.split_min);
    const uint32_t glcap = (n / (sw.small_max + 1) < G ? n / (sw.small_max + 1) : G) + 1;
    const bool do_small = sw.small_max >= 1, do_group = n > sw.small_max && sw.split_min > sw.small_max + 1, do_split = n >= sw.split_min && n > sw.small_max;
    uint32_t *tile_first, *glist, *ghist, *cur, *cand;
    SelState* sst;
    AQG_TRY(aqg_ws_get(ctx, (size_t)ntiles + 1, &tile_first));
    AQG_TRY(aqg_ws_get(ctx, glcap, &glist));
    AQG_TRY(aqg_ws_get(ctx, scap, &sst));
    AQG_TRY(aqg_ws_get(ctx, (size_t)scap * 256 * NHIST<U>, &ghist));
    AQG_TRY(aqg_ws_get(ctx, (size_t)scap * 2, &cur));
    AQG_TRY(aqg_ws_get(ctx, (size_t)scap * k, &cand));
    // the slots no row fills: zero bytes and the missing-row marker
    AQG_HIP(ctx, hipMemsetAsync(vals, 0, (size_t)G * k * sizeof(U), ctx->stream));
    if (pos_out) AQG_HIP(ctx, hipMemsetAsync(pos_out, 0xFF, (size_t)G * k * 4, ctx->stream));
    if (do_small) AQG_HIP(ctx, hipMemsetAsync(tile_first, 0xFF, (size_t)ntiles * 4, ctx->stream));
    if (do_split) {
        AQG_HIP(ctx, hipMemsetAsync(ghist, 0, (size_t)scap * 1024 * NHIST<U>, ctx->stream));
        AQG_HIP(ctx, hipMemsetAsync(cur, 0, (size_t)scap * 8, ctx->stream));
        AQG_HIP(ctx, hipMemsetAsync(cand, 0, (size_t)scap * k * 4, ctx->stream));        // (a slot no row took would still be a position of the column)
    }
    const unsigned ggrid = aqg_grid(ctx, G, SB, 1, 8);
    hipLaunchKernelGGL(topk_classify_kernel, dim3(ggrid), dim3(SB), 0, ctx->stream, off, G, sw.small_max, sw.split_min, k, (int)sizeof(U) * 8, tile_first, glist, sst, ctl);
    aqg_kernel_timer_begin(ctx);
    if (do_small) {
        hipLaunchKernelGGL((topk_small_kernel<U, KIND>), dim3(ntiles), dim3(SB), 0, ctx->stream, x, n, off, G, tile_first, sw.small_max, k, vals, pos_out);
    }
    if (do_group) {
        const uint32_t cap = (uint32_t)ctx->num_cu * 8;
        hipLaunchKernelGGL((topk_group_kernel<U, KIND>), dim3(glcap < cap ? glcap : cap), dim3(SB), 0, ctx->stream, x, off, glist, ctl, k, vals, pos_out);
    }
    if (do_split) {
        const uint64_t chunks = (uint64_t)aqg_ceil_div(n, SPLIT_CHUNK) + scap;
        const unsigned hgrid = (unsigned)(chunks < (uint64_t)ctx->num_cu * 8 ? chunks : (uint64_t)ctx->num_cu * 8);
        const unsigned cgrid = scap < 1024u ? scap : 1024u;
        hipLaunchKernelGGL(select_split_plan_kernel, dim3(1), dim3(SB), 0, ctx->stream, sst, ctl);
        for (size_t p = 0; p < sizeof(U); ++p) {
            hipLaunchKernelGGL((select_split_hist_kernel<U, KIND>), dim3(hgrid), dim3(SB), 0, ctx->stream, x, sst, ctl, ghist);
            hipLaunchKernelGGL((topk_split_choose_kernel<U>), dim3(cgrid), dim3(SB), 0, ctx->stream, sst, ctl, ghist);
        }
        hipLaunchKernelGGL((topk_split_collect_kernel<U, KIND>), dim3(hgrid), dim3(SB), 0, ctx->stream, x, sst, ctl, k, cur, cand);
        hipLaunchKernelGGL((topk_split_emit_kernel<U, KIND>), dim3(cgrid), dim3(SB), 0, ctx->stream, x, sst, ctl, k, cand, vals, pos_out);
    }
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "top-k selection");
}
template <class U, int KIND>
int run_topk_order(aqg_ctx* ctx, int order, const void* x, uint32_t n, const uint32_t* off, uint32_t G, uint32_t k, SelSwitches sw, void* vals, uint32_t* pos_out) {
    if (order == AQG_ORDER_DESC) return run_topk<U, KIND | KIND_DESC>(ctx, x, n, off, G, k, sw, vals, pos_out);
    return run_topk<U, KIND>(ctx, x, n, off, G, k, sw, vals, pos_out);
}
int dispatch_topk(aqg_ctx* ctx, int order, int t, const void* x, uint32_t n, const uint32_t* off, uint32_t G, uint32_t k, SelSwitches sw, void* vals, uint32_t* pos_out) {
    switch (t) {
    case AQG_UINT8: case AQG_BOOL: return run_topk_order<uint8_t, KIND_UNSIGNED>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    case AQG_UINT16: return run_topk_order<uint16_t, KIND_UNSIGNED>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    case AQG_UINT32: return run_topk_order<uint32_t, KIND_UNSIGNED>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    case AQG_UINT64: return run_topk_order<uint64_t, KIND_UNSIGNED>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    case AQG_INT8: return run_topk_order<uint8_t, KIND_SIGNED>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    case AQG_INT16: return run_topk_order<uint16_t, KIND_SIGNED>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    case AQG_INT32: return run_topk_order<uint32_t, KIND_SIGNED>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    case AQG_INT64: return run_topk_order<uint64_t, KIND_SIGNED>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    case AQG_FLOAT: return run_topk_order<uint32_t, KIND_FP>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    case AQG_DOUBLE: return run_topk_order<uint64_t, KIND_FP>(ctx, order, x, n, off, G, k, sw, vals, pos_out);
    }
    return AQG_ERR_DTYPE;
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

} // namespace

extern "C" {

int aqg_topk(aqg_ctx* ctx, int order, int t, const void* x, uint32_t n, uint32_t k, void* vals_out_dev, uint32_t* rows_out_dev) {
    if (!ctx || !vals_out_dev) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_topk: bad argument");
    AQG_TRY(check_args(ctx, order, t, k));
    if (!x && n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_topk: null column");
    AQG_CHECK_ROWS(ctx, n, "aqg_topk");
    AQG_TRY(ensure_ctl(ctx));
    if (n == 0) {                                           // no row: k empty slots
        AQG_HIP(ctx, hipMemsetAsync(vals_out_dev, 0, (size_t)k * esz_of(t), ctx->stream));
        if (rows_out_dev) AQG_HIP(ctx, hipMemsetAsync(rows_out_dev, 0xFF, (size_t)k * 4, ctx->stream));
        return AQG_OK;
    }
    const SelSwitches sw = select_switches();
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, topk_ws_bytes(n, 1, k, sw)));
    uint32_t* ctl = ctx->select_ctl;
    hipLaunchKernelGGL(flat_offsets_kernel, dim3(1), dim3(1), 0, ctx->stream, ctl + CTL_OFF, n);
    return dispatch_topk(ctx, order, t, x, n, ctl + CTL_OFF, 1, k, sw, vals_out_dev, rows_out_dev);
}

int aqg_grouped_topk_flat(aqg_ctx* ctx, aqg_groupby* g, int order, int t, const void* xflat, uint32_t k, void* vals_out_dev, uint32_t* pos_out_dev) {
    AQG_TRY(check_grouped(ctx, g, order, t, xflat, k, vals_out_dev));
    AQG_TRY(ensure_ctl(ctx));
    const uint32_t n = g->n, G = g->ngroups;
    if (n == 0 || G == 0) return AQG_OK;
    const uint32_t* off = aqg_groupby_offsets(g);
    if (!off) return AQG_ERR_HIP;
    const SelSwitches sw = select_switches();
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, topk_ws_bytes(n, G, k, sw)));
    return dispatch_topk(ctx, order, t, xflat, n, off, G, k, sw, vals_out_dev, pos_out_dev);
}

int aqg_grouped_topk(aqg_ctx* ctx, aqg_groupby* g, int order, int t, const void* x, uint32_t k, void* vals_out_dev, uint32_t* pos_out_dev) {
    AQG_TRY(check_grouped(ctx, g, order, t, x, k, vals_out_dev));
    AQG_TRY(ensure_ctl(ctx));
    const uint32_t n = g->n, G = g->ngroups;
    if (n == 0 || G == 0) return AQG_OK;
    const uint32_t* off = aqg_groupby_offsets(g);
    if (!off) return AQG_ERR_HIP;
    const SelSwitches sw = select_switches();
    const int esz = esz_of(t);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * esz + 4096 + aqg_postproc_ws_bytes(n, G, esz) + topk_ws_bytes(n, G, k, sw)));
    unsigned char* xs;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n * esz + 64, &xs));
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x, esz, xs, /*ws_managed=*/true));
    return dispatch_topk(ctx, order, t, xs, n, off, G, k, sw, vals_out_dev, pos_out_dev);
}

} // extern "C"
