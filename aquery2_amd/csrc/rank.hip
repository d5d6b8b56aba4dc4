// rank.hip -- aqg_rank / aqg_grouped_rank(_flat): where every row stands in its slice -- RANK, DENSE_RANK, ROW_NUMBER, PERCENT_RANK,
// CUME_DIST and NTILE(k) OVER (PARTITION BY group ORDER BY x), pandas' groupby().rank(method=...), kdb's rank / xrank.
// The reference has no such function; the contract is include/aqg.h's (ranking section) and the exact model tests/rank_model.py.
//
// Every method is a function of five integers of a row: min (1 + rows of its slice that sort strictly before it), max (rows that sort
// before it or tie), dense (1 + distinct values before it), first (min + ties in front of it in the layout) and c (rows of the slice).
// Values are compared through their order-preserving images (key_image.hpp), complemented for AQG_ORDER_DESC.  Two routes, chosen per
// group by its size, both taken by one call whose groups ask for both:
//   SMALL   up to AQG_SELECT_SMALL_MAX rows: the tile staging of the selections' SMALL route (small_tile, select_radix.hpp) with this
//           file's own counting -- a wavefront per group counts, for every row, the images below it, equal to it and equal in front of
//           it; DENSE marks first occurrences in LDS and counts the marked images below the row.  Groups of one or two rows take a lane.
//   SORTED  every other group: their flat positions (one compaction launch; none when every group is big) are ordered by (group, image)
//           with aqg_sort_rows, stable, so ties stay in layout order.  Over that order
//             rank_mark_kernel   a lane per group: the entries of a group are contiguous in the order and start where the groups before
//                                it end, so its start is marked without a look at the rows
//             rank_flag_kernel   gathers the image of every entry, marks the tie-run heads beside the group starts (a byte per entry)
//                                and folds a summary per tile: last / first head, last / first group start, heads since the last group start
//             rank_carry_kernel  one workgroup scans the tile summaries forwards (run head, group start, heads since it) and backwards
//                                (next head, next group start): tie runs and groups may span any number of tiles, nobody spins
//             rank_emit_kernel   reads order and marks (16- and 8-byte loads), finishes both scans inside the tile, derives the five
//                                integers and scatters the method's value to out[position]: one writer per element, no atomics
// The sort reads its digit histogram back (as aqg_sort_rows always does); beyond that the host needs one number, the rows in groups
// above the SMALL threshold, which it reads once per handle and layout (aqg_groupby::rank_big_rows).
#include "select_host.hpp"

namespace {
using namespace selradix;

constexpr int EB = 256;                     // lanes per workgroup of the SORTED kernels
constexpr int ENW = EB / 64;
constexpr int EPT = 8;                      // consecutive sorted entries per lane: two 16-byte loads of the order, one 8-byte load of the marks
constexpr uint32_t ET = EB * EPT;           // entries per workgroup: the emit tile
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t SEGBIT = 1ull << 63;     // a head count that was restarted by a group start
constexpr uint8_t F_HEAD = 1, F_GS = 2;     // marks of an entry: first of its tie run / first of its group

__host__ __device__ inline bool rank_is_double(int method) { return method >= AQG_RANK_AVERAGE && method <= AQG_RANK_CUME_DIST; }

// the value of a method from a row's five integers (O: uint32_t or double, as aqg_rank_out_dtype says)
template <class O> __device__ inline O rank_value(int method, uint32_t k, uint32_t mn, uint32_t mx, uint32_t dense, uint32_t first, uint32_t c) {
    if constexpr (std::is_same_v<O, double>) {
        if (method == AQG_RANK_AVERAGE) return (double)((uint64_t)mn + mx) * 0.5;
        if (method == AQG_RANK_PERCENT) return c == 1 ? 0.0 : (double)(mn - 1) / (double)(c - 1);
        return (double)mx / (double)c;
    } else {
        if (method == AQG_RANK_MIN) return mn;
        if (method == AQG_RANK_MAX) return mx;
        if (method == AQG_RANK_DENSE) return dense;
        if (method == AQG_RANK_FIRST) return first;
        const uint32_t q = c / k, r = c % k, o = first - 1, wide = r * (q + 1);       // NTILE: the first r buckets hold q + 1 rows
        return o < wide ? o / (q + 1) + 1 : r + (o - wide) / q + 1;                   // (o >= wide implies q >= 1)
    }
}

// heads counted since the last group start: a + b, unless b starts a group itself
struct OpSegAdd { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return (b & SEGBIT) ? b : a + b; } };

// exclusive scan of one value per lane over the workgroup in lane order (id: op's identity; wtot: ENW words of LDS); total = all lanes
template <class T, class Op> __device__ inline T block_scan_excl(T v, Op op, T id, T* wtot, T& total) {
    const int lane = lane_id(), wid = wave_id();
    const T incl = wave_scan_incl(v, op, lane);
    if (lane == 63) wtot[wid] = incl;
    T ex = shfl_up_t(incl, 1);
    if (lane == 0) ex = id;
    __syncthreads();
    T base = id;
    total = id;
    for (int w = 0; w < ENW; ++w) { if (w == wid) base = total; total = op(total, wtot[w]); }
    __syncthreads();
    return op(base, ex);
}

// ---- routing: one lane per group ------------------------------------------------------------------------------------------------------------
// bigc[g] = rows of group g when the SORTED route ranks it, else 0 (bigc[G] = 0: the exclusive scan leaves the route's row count there);
// SMALL groups mark the first of them that starts in each tile
__global__ void __launch_bounds__(SB) rank_classify_kernel(const uint32_t* __restrict__ off, uint32_t G, uint32_t small_max, uint32_t* __restrict__ tile_first, uint32_t* __restrict__ bigc) {
    for (uint64_t gg = (uint64_t)blockIdx.x * SB + threadIdx.x; gg <= G; gg += (uint64_t)gridDim.x * SB) {
        const uint32_t g = (uint32_t)gg;
        uint32_t big = 0;
        if (g < G) {
            const uint32_t lo = off[g], c = off[g + 1] - lo;
            if (c > small_max) big = c;
            else if (c) small_tile_mark(off, g, lo, small_max, tile_first);
        }
        bigc[g] = big;
    }
}
// pos[bigbase[g] + i] = the flat position of row i of SORTED group g: the positions of the route's rows, ascending
__global__ void __launch_bounds__(256) rank_compact_kernel(const uint32_t* __restrict__ gid, const uint32_t* __restrict__ off, const uint32_t* __restrict__ bigbase,
                                                            uint32_t n, uint32_t small_max, uint32_t* __restrict__ pos) {
    uint32_t lo, hi;
    wg_span(n, lo, hi, 256);
    for (uint32_t p = lo + threadIdx.x; p < hi; p += blockDim.x) {
        const uint32_t g = gid[p], glo = off[g];
        if (off[g + 1] - glo > small_max) pos[bigbase[g] + (p - glo)] = p;
    }
}

// marks[bigbase[g]] = first entry of its group (and of a tie run), for every SORTED group: where its entries begin in the sorted order
__global__ void __launch_bounds__(256) rank_mark_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ bigbase, uint32_t G, uint32_t small_max, uint8_t* __restrict__ marks) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x)
        if (off[g + 1] - off[g] > small_max) marks[bigbase[g]] = F_HEAD | F_GS;
}

// ---- SMALL ----------------------------------------------------------------------------------------------------------------------------------
template <class U, int KIND, class O>
__global__ void __launch_bounds__(SB) rank_small_kernel(const U* __restrict__ x, uint32_t n, const uint32_t* __restrict__ off, uint32_t G, const uint32_t* __restrict__ tile_first,
                                                         uint32_t small_max, int method, uint32_t k, O* __restrict__ out) {
    __shared__ uint8_t firstf[TILE + SMALL_CAP];            // DENSE: is the staged row the first of its value in its group?
    const uint32_t tbeg = blockIdx.x * TILE;
    small_tile<U, KIND>(
        x, n, off, G, tile_first, small_max,
        [&](uint32_t, uint32_t lo, uint32_t c, bool) {
            if (c == 1) { out[lo] = rank_value<O>(method, k, 1, 1, 1, 1, 1); return; }
            const U a = image_of<U, KIND>(x[lo]), b = image_of<U, KIND>(x[lo + 1]);
            const uint32_t eq = a == b, lt0 = b < a, lt1 = a < b;
            out[lo] = rank_value<O>(method, k, lt0 + 1, lt0 + 1 + eq, lt0 + 1, lt0 + 1, 2);
            out[lo + 1] = rank_value<O>(method, k, lt1 + 1, lt1 + 1 + eq, lt1 + 1, lt1 + eq + 1, 2);
        },
        [](uint32_t) { return 0u; }, [](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {},
        [&](uint32_t, uint32_t lo, uint32_t c, const U* im) {
            const uint32_t lane = lane_id();
            uint8_t* ff = firstf + (lo - tbeg);
            if (method == AQG_RANK_DENSE) {                 // (the wavefront's own LDS writes, read back by itself below)
                for (uint32_t eb = 0; eb < c; eb += 64) {
                    const bool live = eb + lane < c;
                    const uint32_t ii = live ? eb + lane : c - 1;
                    const U mine = im[ii];
                    uint32_t eqb = 0;
#pragma unroll 4
                    for (uint32_t j = 0; j < c; ++j) eqb += (im[j] == mine) & (j < ii);
                    if (live) ff[ii] = eqb == 0;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            for (uint32_t eb = 0; eb < c; eb += 64) {
                const bool live = eb + lane < c;
                const uint32_t ii = live ? eb + lane : c - 1;
                const U mine = im[ii];
                uint32_t lt = 0, eq = 0, eqb = 0, dl = 0;
                if (method == AQG_RANK_DENSE) {
#pragma unroll 4
                    for (uint32_t j = 0; j < c; ++j) dl += (im[j] < mine) & ff[j];
                } else {
#pragma unroll 4
                    for (uint32_t j = 0; j < c; ++j) {
                        const U v = im[j];
                        const uint32_t e = v == mine;
                        lt += v < mine; eq += e; eqb += e & (j < ii);
                    }
                }
                if (live) out[lo + ii] = rank_value<O>(method, k, lt + 1, lt + eq, dl + 1, lt + eqb + 1, c);
            }
        });
}

// ---- SORTED ---------------------------------------------------------------------------------------------------------------------------------
struct TileSum { uint32_t last_head1, last_gs1, first_head, first_gs; uint64_t cnt; };      // (last_*1: index + 1, 0 = none; first_*: NONE = none)
struct TileCarry { uint32_t head1, gs1, next_head, next_gs; uint64_t cnt; };                // what a tile needs from the tiles before and behind it

// the live entries of a lane
__device__ inline uint32_t lane_entries(uint32_t i0, uint32_t m) { return i0 >= m ? 0u : (m - i0 < (uint32_t)EPT ? m - i0 : (uint32_t)EPT); }
// ord[i0 .. i0 + EPT) (i0 a multiple of EPT, the order 16-byte aligned); 0 for an entry that is not there
__device__ inline void load_order(const uint32_t* __restrict__ ord, uint32_t i0, uint32_t nl, uint32_t (&p)[EPT]) {
    if (nl == (uint32_t)EPT) {
        const vec16<uint32_t> a = load16(ord + i0), b = load16(ord + i0 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { p[j] = a.v[j]; p[4 + j] = b.v[j]; }
    } else {
#pragma unroll
        for (int j = 0; j < EPT; ++j) p[j] = (uint32_t)j < nl ? ord[i0 + j] : 0u;
    }
}
// a lane's summary of its EPT marks f (byte j: entry i0 + j), in the shape of a tile's
__device__ inline TileSum lane_summary(uint64_t f, uint32_t i0) {
    TileSum s{0, 0, NONE, NONE, 0};
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const uint32_t fl = (uint32_t)(f >> (8 * j)) & 255u, i = i0 + j;
        if (fl & F_HEAD) { s.last_head1 = i + 1; if (s.first_head == NONE) s.first_head = i; s.cnt += 1; }
        if (fl & F_GS) { s.last_gs1 = i + 1; if (s.first_gs == NONE) s.first_gs = i; s.cnt = SEGBIT | 1ull; }
    }
    return s;
}

template <class U, int KIND>
__global__ void __launch_bounds__(EB) rank_flag_kernel(const U* __restrict__ x, const uint32_t* __restrict__ ord, uint32_t m, uint64_t* __restrict__ flags8, TileSum* __restrict__ ts) {
    __shared__ U s_im[EB];
    __shared__ uint64_t w64[ENW];
    __shared__ uint32_t red[ENW][4];
    const uint32_t i0 = blockIdx.x * ET + threadIdx.x * EPT, nl = lane_entries(i0, m);
    uint32_t p[EPT];
    U im[EPT];
    load_order(ord, i0, nl, p);
#pragma unroll
    for (int j = 0; j < EPT; ++j) im[j] = (uint32_t)j < nl ? image_of<U, KIND>(x[p[j]]) : U(0);
    U lim = im[0];
#pragma unroll
    for (int j = 1; j < EPT; ++j) if ((uint32_t)j < nl) lim = im[j];
    s_im[threadIdx.x] = lim;
    __syncthreads();
    uint64_t f = 0;
    if (nl) {
        f = flags8[i0 / EPT];                                           // the group starts (rank_mark_kernel; zero for a whole column)
        if (i0 == 0) f |= F_HEAD | F_GS;
        U pim = 0;
        if (threadIdx.x) pim = s_im[threadIdx.x - 1];                   // (the lane in front is full when this one has entries)
        else if (i0) pim = image_of<U, KIND>(x[ord[i0 - 1]]);
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            if ((uint32_t)j < nl) {
                if (im[j] != pim) f |= (uint64_t)F_HEAD << (8 * j);
                pim = im[j];
            }
        }
        flags8[i0 / EPT] = f;
    }
    const TileSum s = lane_summary(f, i0);
    uint64_t cnt;
    block_scan_excl(s.cnt, OpSegAdd{}, (uint64_t)0, w64, cnt);
    const uint32_t lh = wave_reduce(s.last_head1, OpMax{}), lgs = wave_reduce(s.last_gs1, OpMax{});
    const uint32_t fh = wave_reduce(s.first_head, OpMin{}), fg = wave_reduce(s.first_gs, OpMin{});
    if (lane_id() == 0) { red[wave_id()][0] = lh; red[wave_id()][1] = lgs; red[wave_id()][2] = fh; red[wave_id()][3] = fg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        TileSum t{0, 0, NONE, NONE, cnt};
        for (int w = 0; w < ENW; ++w) {
            t.last_head1 = OpMax{}(t.last_head1, red[w][0]); t.last_gs1 = OpMax{}(t.last_gs1, red[w][1]);
            t.first_head = OpMin{}(t.first_head, red[w][2]); t.first_gs = OpMin{}(t.first_gs, red[w][3]);
        }
        ts[blockIdx.x] = t;
    }
}

// one workgroup: tc[j] = the fold of the summaries of the tiles in front of tile j (run head, group start, heads since it) and behind it
// (the next head, the next group start; m when there is none)
__global__ void __launch_bounds__(EB) rank_carry_kernel(const TileSum* __restrict__ ts, uint32_t ntiles, uint32_t m, TileCarry* __restrict__ tc) {
    __shared__ uint64_t w64[ENW];
    __shared__ uint32_t w32[ENW];
    uint32_t ch = 0, cg = 0;
    uint64_t cc = 0;
    for (uint32_t base = 0; base < ntiles; base += EB) {
        const uint32_t j = base + threadIdx.x;
        const bool live = j < ntiles;
        const TileSum s = live ? ts[j] : TileSum{0, 0, NONE, NONE, 0};
        uint32_t th, tg;
        uint64_t tcnt;
        const uint32_t eh = block_scan_excl(s.last_head1, OpMax{}, 0u, w32, th);
        const uint32_t eg = block_scan_excl(s.last_gs1, OpMax{}, 0u, w32, tg);
        const uint64_t ec = block_scan_excl(s.cnt, OpSegAdd{}, (uint64_t)0, w64, tcnt);
        if (live) { tc[j].head1 = OpMax{}(ch, eh); tc[j].gs1 = OpMax{}(cg, eg); tc[j].cnt = OpSegAdd{}(cc, ec); }
        ch = OpMax{}(ch, th); cg = OpMax{}(cg, tg); cc = OpSegAdd{}(cc, tcnt);
    }
    uint32_t nh = m, ng = m;
    for (uint32_t base = 0; base < ntiles; base += EB) {                // from the last tile backwards
        const uint32_t r = base + threadIdx.x;
        const bool live = r < ntiles;
        const uint32_t j = live ? ntiles - 1 - r : 0u;
        const uint32_t fh = live ? ts[j].first_head : NONE, fg = live ? ts[j].first_gs : NONE;
        uint32_t th, tg;
        const uint32_t eh = block_scan_excl(fh, OpMin{}, NONE, w32, th);
        const uint32_t eg = block_scan_excl(fg, OpMin{}, NONE, w32, tg);
        if (live) { tc[j].next_head = OpMin{}(nh, eh); tc[j].next_gs = OpMin{}(ng, eg); }
        nh = OpMin{}(nh, th); ng = OpMin{}(ng, tg);
    }
}

template <class O>
__global__ void __launch_bounds__(EB) rank_emit_kernel(const uint32_t* __restrict__ ord, const uint64_t* __restrict__ flags8, const TileCarry* __restrict__ tc, uint32_t m,
                                                        int method, uint32_t k, O* __restrict__ out) {
    __shared__ uint64_t w64[ENW];
    __shared__ uint32_t w32[ENW];
    __shared__ uint32_t rev[2][EB];
    const uint32_t i0 = blockIdx.x * ET + threadIdx.x * EPT, nl = lane_entries(i0, m);
    uint32_t p[EPT];
    load_order(ord, i0, nl, p);
    const uint64_t f = nl ? flags8[i0 / EPT] : 0ull;
    const TileCarry c = tc[blockIdx.x];
    const TileSum s = lane_summary(f, i0);
    // forwards: the head of the run and the start of the group an entry is in, the heads since that start
    uint32_t t32;
    uint64_t t64;
    uint32_t hd1 = OpMax{}(c.head1, block_scan_excl(s.last_head1, OpMax{}, 0u, w32, t32));
    uint32_t gs1 = OpMax{}(c.gs1, block_scan_excl(s.last_gs1, OpMax{}, 0u, w32, t32));
    uint32_t cnt = (uint32_t)OpSegAdd{}(c.cnt, block_scan_excl(s.cnt, OpSegAdd{}, (uint64_t)0, w64, t64));
    // backwards: the next head and the next group start behind the lane (the same scan over the lanes in reverse)
    const uint32_t rt = EB - 1 - threadIdx.x;
    rev[0][rt] = s.first_head; rev[1][rt] = s.first_gs;
    __syncthreads();
    const uint32_t eh = block_scan_excl(rev[0][threadIdx.x], OpMin{}, NONE, w32, t32);
    const uint32_t eg = block_scan_excl(rev[1][threadIdx.x], OpMin{}, NONE, w32, t32);
    rev[0][rt] = eh; rev[1][rt] = eg;                                   // (block_scan_excl ended on a barrier: every lane has read its slot)
    __syncthreads();
    uint32_t nh = OpMin{}(c.next_head, rev[0][threadIdx.x]), ng = OpMin{}(c.next_gs, rev[1][threadIdx.x]);
    uint32_t nhe[EPT], nge[EPT];
#pragma unroll
    for (int j = EPT - 1; j >= 0; --j) {
        const uint32_t fl = (uint32_t)(f >> (8 * j)) & 255u;
        nhe[j] = nh; nge[j] = ng;
        if (fl & F_HEAD) nh = i0 + j;
        if (fl & F_GS) ng = i0 + j;
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        if ((uint32_t)j < nl) {
            const uint32_t fl = (uint32_t)(f >> (8 * j)) & 255u, i = i0 + j;
            if (fl & F_GS) { gs1 = i + 1; cnt = 0; }
            if (fl & F_HEAD) { hd1 = i + 1; ++cnt; }
            const uint32_t gs = gs1 - 1, hd = hd1 - 1;                  // (entry 0 is a head and a group start: both are set from there on)
            out[p[j]] = rank_value<O>(method, k, hd - gs + 1, nhe[j] - gs, cnt, i - gs + 1, nge[j] - gs);
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
struct RankCall { int method, order; uint32_t k; int t; };

size_t rank_sorted_ws_bytes(uint32_t m) {
    const size_t ntiles = aqg_ceil_div(m, ET);
    return ntiles * (sizeof(TileSum) + sizeof(TileCarry)) + 4096;
}

// the SORTED route over the order `ord` of its m entries (x in the flat layout; flags8: the marks, group starts set)
template <class O> int run_sorted(aqg_ctx* ctx, const RankCall& rc, const void* x, const uint32_t* ord, uint32_t m, uint64_t* flags8, void* out) {
    const uint32_t ntiles = aqg_ceil_div(m, ET);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, rank_sorted_ws_bytes(m)));
    TileSum* ts;
    TileCarry* tc;
    AQG_TRY(aqg_ws_get(ctx, ntiles, &ts));
    AQG_TRY(aqg_ws_get(ctx, ntiles, &tc));
    AQG_TRY(dispatch_kind(rc.t, [&]<class U, int KIND>() {
        hipLaunchKernelGGL((rank_flag_kernel<U, KIND>), dim3(ntiles), dim3(EB), 0, ctx->stream, static_cast<const U*>(x), ord, m, flags8, ts);
        return AQG_OK;
    }));
    hipLaunchKernelGGL(rank_carry_kernel, dim3(1), dim3(EB), 0, ctx->stream, ts, ntiles, m, tc);
    aqg_kernel_timer_begin(ctx);
    hipLaunchKernelGGL((rank_emit_kernel<O>), dim3(ntiles), dim3(EB), 0, ctx->stream, ord, flags8, tc, m, rc.method, rc.k, static_cast<O*>(out));
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "rank emit");
}

// g == nullptr: the n rows of x are one group.  Else the groups of g, x in the flat layout or (row_layout) brought into it.
template <class O> int run_rank(aqg_ctx* ctx, aqg_groupby* g, const RankCall& rc, const void* x, uint32_t n, bool row_layout, void* out) {
    const uint32_t small_max = select_switches().small_max, G = g ? g->ngroups : 1u;
    const int esz = esz_of(rc.t);
    const uint32_t *off = nullptr, *gid = nullptr;
    if (g) {                                                            // (both are made on first use and reset the workspace then)
        if (!(off = aqg_groupby_offsets(g))) return AQG_ERR_HIP;
        AQG_TRY(aqg_flat_gid(ctx, g, &gid));
    }
    const uint32_t ntiles = aqg_ceil_div(n, TILE);
    const size_t scan_words = ((size_t)G + 1 + 2047) / 2048 + 16;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (row_layout ? aqg_postproc_ws_bytes(n, G, esz) : 0) + ((size_t)ntiles + 1 + G + 2 + scan_words) * 4 + 4096));
    uint32_t *tile_first, *bigc, *bsum;
    AQG_TRY(aqg_ws_get(ctx, (size_t)ntiles + 1, &tile_first));
    AQG_TRY(aqg_ws_get(ctx, (size_t)G + 2, &bigc));
    AQG_TRY(aqg_ws_get(ctx, scan_words, &bsum));
    if (!g) {
        hipLaunchKernelGGL(flat_offsets_kernel, dim3(1), dim3(1), 0, ctx->stream, bsum, n);      // (no scan without groups: its scratch holds {0, n})
        off = bsum;
    }
    AQG_HIP(ctx, hipMemsetAsync(tile_first, 0xFF, (size_t)ntiles * 4, ctx->stream));
    hipLaunchKernelGGL(rank_classify_kernel, dim3(aqg_grid(ctx, (uint64_t)G + 1, SB, 1, 8)), dim3(SB), 0, ctx->stream, off, G, small_max, tile_first, bigc);
    AQG_TRY(aqg_check_launch(ctx, "rank_classify_kernel"));
    uint32_t m = n > small_max ? n : 0u;                                // rows of the SORTED route
    if (g) {
        AQG_TRY(aqg_exclusive_scan_u32(ctx, bigc, (uint64_t)G + 1, bsum));
        if (!g->rank_big_valid || g->rank_big_max != small_max) {
            AQG_TRY(aqg_d2h(ctx, &g->rank_big_rows, bigc + G, 4));
            g->rank_big_max = small_max;
            g->rank_big_valid = true;
        }
        m = g->rank_big_rows;
    }
    ctx->rank_routes = (m < n ? AQG_RANK_ROUTE_SMALL : 0) | (m ? AQG_RANK_ROUTE_SORTED : 0);
    ctx->rank_tile = ET;
    // what has to outlive the sort's workspace, in ONE pool buffer (the pool keeps one large buffer between calls): the flat column of a
    // row-layout call, the positions of the SORTED groups' rows when there are SMALL groups beside them, the order, the marks
    auto rup = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t xs_b = row_layout ? rup((size_t)n * esz + 64) : 0, pos_b = m && m < n ? rup((size_t)m * 4) : 0, ord_b = rup((size_t)m * 4);
    const size_t mark_b = (size_t)aqg_ceil_div(m, ET) * EB * 8;
    PoolBuf keep(ctx);
    if (xs_b + (m ? pos_b + ord_b + mark_b : 0)) AQG_TRY(keep.get(xs_b + (m ? pos_b + ord_b + mark_b : 0)));
    char* kp = static_cast<char*>(keep.p);
    if (row_layout) {
        AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x, esz, kp, /*ws_managed=*/true));
        x = kp;
    }
    if (m < n) {
        AQG_TRY(dispatch_kind(rc.t, [&]<class U, int KIND>() {
            auto go = [&]<int KD>() {
                hipLaunchKernelGGL((rank_small_kernel<U, KD, O>), dim3(ntiles), dim3(SB), 0, ctx->stream, static_cast<const U*>(x), n, off, G, tile_first, small_max, rc.method, rc.k,
                                   static_cast<O*>(out));
                return aqg_check_launch(ctx, "rank_small_kernel");
            };
            return rc.order == AQG_ORDER_DESC ? go.template operator()<KIND | KIND_DESC>() : go.template operator()<KIND>();
        }));
    }
    if (!m) return AQG_OK;
    uint32_t *pos = reinterpret_cast<uint32_t*>(kp + xs_b), *ord = reinterpret_cast<uint32_t*>(kp + xs_b + pos_b);
    uint64_t* marks = reinterpret_cast<uint64_t*>(kp + xs_b + pos_b + ord_b);
    if (m < n) {
        hipLaunchKernelGGL(rank_compact_kernel, dim3(aqg_grid(ctx, n, 256, 4, 8)), dim3(256), 0, ctx->stream, gid, off, bigc, n, small_max, pos);
        AQG_TRY(aqg_check_launch(ctx, "rank_compact_kernel"));
    }
    // a group's entries start where those of the SORTED groups before it end
    AQG_HIP(ctx, hipMemsetAsync(marks, 0, mark_b, ctx->stream));
    if (g) hipLaunchKernelGGL(rank_mark_kernel, dim3(aqg_grid(ctx, G, 256, 1, 8)), dim3(256), 0, ctx->stream, off, bigc, G, small_max, reinterpret_cast<uint8_t*>(marks));
    const int sdt[2] = {AQG_UINT32, rc.t}, sord[2] = {AQG_ORDER_ASC, rc.order};
    const void* scol[2] = {gid, x};
    const int first = g ? 0 : 1;
    AQG_TRY(aqg_sort_rows(ctx, 2 - first, sdt + first, scol + first, sord + first, n, m < n ? pos : nullptr, m, ord));
    return run_sorted<O>(ctx, rc, x, ord, m, marks, out);
}

// the checks every entry shares (n rows of dtype t at x, ranks at out)
int check_rank(aqg_ctx* ctx, int method, int order, uint32_t k, int t, const void* x, uint32_t n, const void* out) {
    if (method < AQG_RANK_MIN || method > AQG_RANK_NTILE) return aqg_fail(ctx, AQG_ERR_ARG, "rank: unknown method");
    if (order != AQG_ORDER_ASC && order != AQG_ORDER_DESC) return aqg_fail(ctx, AQG_ERR_ARG, "rank: order must be AQG_ORDER_ASC or AQG_ORDER_DESC");
    if (method == AQG_RANK_NTILE && k < 1) return aqg_fail(ctx, AQG_ERR_ARG, "rank: NTILE needs k >= 1");
    if (!esz_of(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "rank: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    if ((!x || !out) && n) return aqg_fail(ctx, AQG_ERR_ARG, "rank: null column");
    AQG_CHECK_ROWS(ctx, n, "rank");
    if (overlaps(out, (uint64_t)n * (rank_is_double(method) ? 8 : 4), x, (uint64_t)n * esz_of(t))) return aqg_fail(ctx, AQG_ERR_ARG, "rank: out overlaps x");
    return AQG_OK;
}
int rank_entry(aqg_ctx* ctx, aqg_groupby* g, int method, int order, uint32_t k, int t, const void* x, uint32_t n, bool row_layout, void* out) {
    AQG_TRY(check_rank(ctx, method, order, k, t, x, n, out));
    if (n == 0 || (g && g->ngroups == 0)) return AQG_OK;
    const RankCall rc{method, order, k, t};
    return rank_is_double(method) ? run_rank<double>(ctx, g, rc, x, n, row_layout, out) : run_rank<uint32_t>(ctx, g, rc, x, n, row_layout, out);
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped rank: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped rank: the handle was not made by aqg_groupby_build");
    return AQG_OK;
}

} // namespace

extern "C" {

int aqg_rank_out_dtype(int method) {
    if (method < AQG_RANK_MIN || method > AQG_RANK_NTILE) return -1;
    return rank_is_double(method) ? AQG_DOUBLE : AQG_UINT32;
}

int aqg_rank(aqg_ctx* ctx, int method, int order, uint32_t k, int t, const void* x, uint32_t n, void* out_dev) {
    if (!ctx) return AQG_ERR_ARG;
    return rank_entry(ctx, nullptr, method, order, k, t, x, n, false, out_dev);
}

int aqg_grouped_rank(aqg_ctx* ctx, aqg_groupby* g, int method, int order, uint32_t k, int t, const void* x, void* out_flat_dev) {
    AQG_TRY(check_grouped(ctx, g));
    return rank_entry(ctx, g, method, order, k, t, x, g->n, /*row_layout=*/true, out_flat_dev);
}

int aqg_grouped_rank_flat(aqg_ctx* ctx, aqg_groupby* g, int method, int order, uint32_t k, int t, const void* xflat, void* out_flat_dev) {
    AQG_TRY(check_grouped(ctx, g));
    return rank_entry(ctx, g, method, order, k, t, xflat, g->n, /*row_layout=*/false, out_flat_dev);
}

int aqg_rank_last(aqg_ctx* ctx, uint32_t* routes_host, uint32_t* tile_rows_host) {
    if (!ctx || !routes_host || !tile_rows_host) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_rank_last: bad argument");
    *routes_host = ctx->rank_routes;
    *tile_rows_host = ctx->rank_tile;
    return AQG_OK;
}

} // extern "C"
