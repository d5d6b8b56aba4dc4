// range_window.hip -- windows measured in TIME, not in rows: out[i] = op over the rows [lo_i, i] of row i's slice that lie within `span`
// of its stamp (kdb's wj window, pandas rolling("5s"), SQL RANGE BETWEEN span PRECEDING AND CURRENT ROW).  The reference has no such
// function; the contract is include/aqg.h's and the exact model tests/timewin_model.py.
//
// Two passes that know nothing of each other:
//   bounds   lo[i] by a binary search per row over [slice start, i] on the monotone predicate "d(i, j) within span".  The tile's stamps
//            and the tile before it are staged in LDS as order-preserving images; a search reads HBM only for the part of its range in
//            front of that.  The rising / falling steps inside slices are counted in the same launch (one atomic add per workgroup).
//   fold     a block tree of radix 64 over the layout (fold_tree.hpp, shared with the window join: the tree, its build, the result
//            store, the op-by-dtype dispatch and the fold's argument checks): level k + 1 holds the fold of every aligned block of 64
//            elements of level k, and levels >= 1 also hold the prefix and suffix folds inside their blocks.  A query [lo, i] is the
//            suffix of lo's block, the whole blocks between (the same question one level up) and the prefix of i's block.  Whole
//            blocks that all lie in the staged level 1 are folded directly, in one loop: the window join's fold never does that, so
//            the two bracket a floating sum differently, on purpose.  COMBINING ONLY: nothing is ever subtracted back out, so a NaN,
//            an Inf or a 1e30 acts on exactly the windows that hold it.  The tree knows nothing of groups: lo >= the slice start, so
//            a block that straddles a group start is only ever entered through the part inside the window.
// Level 0 keeps no prefix / suffix folds: they would cost 2 sizeof(A) bytes per row written and read back (32 for 64-bit sums) against
// at most 63 LDS reads at either end of a window; the levels above cost 3 sizeof(A) / 63 bytes per row all together.
// No atomics and no look-back in the fold: the bracketing of a floating sum depends on n, lo and i alone.
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "scan_dev.hpp"
#include "stamps_dev.hpp"
#include "groupby_handle.hpp"
#include "fold_tree.hpp"

namespace {
using namespace aqgscan;

constexpr int RX = 64;                  // radix of the block tree (fold_tree.hpp), as the fold kernel below sees it; tests/timewin_cases.py reads it
constexpr int RSH = 6;
static_assert(RX == TREE_RX && RSH == TREE_RSH, "the fold kernel walks the tree of fold_tree.hpp");

// ---- bounds --------------------------------------------------------------------------------------------------------------------------
// order-preserving image of a stamp: uint64 for integer / DATE / TIME columns (d = larger - smaller, exact), the double itself otherwise
template <class T> struct stamp_img {
    static constexpr bool FP = std::is_floating_point_v<T>;
    using I = std::conditional_t<FP, double, uint64_t>;
    __device__ static I of(T v) {
        if constexpr (FP) return (double)v;
        else if constexpr (std::is_same_v<T, ema_date> || std::is_same_v<T, ema_time>) return (uint64_t)stamp_of(v) ^ 0x8000000000000000ull;
        else if constexpr (std::is_unsigned_v<T>) return (uint64_t)v;
        else return (uint64_t)(int64_t)v ^ 0x8000000000000000ull;
    }
};
template <class I> __device__ inline bool within(I a, I b, const span_lim& s) {
    if constexpr (std::is_same_v<I, double>) { const double d = fabs(a - b); return s.closed ? d <= s.span : d < s.span; }
    else return (a > b ? a - b : b - a) <= s.dmax;
}

// one workgroup per tile of TS rows; lane t takes rows t, t + SB, ... of the tile (coalesced stores)
template <class T, bool SEG> __global__ void __launch_bounds__(SB)
rangew_bounds_kernel(const T* __restrict__ t, uint32_t n, span_lim lim, const uint32_t* __restrict__ gid, const uint32_t* __restrict__ off,
                     uint32_t* __restrict__ lo_out, unsigned long long* __restrict__ steps) {
    using IM = stamp_img<T>;
    using I = typename IM::I;
    __shared__ I L[2 * TS];
    __shared__ uint32_t cnt[2];
    const uint32_t tile = (uint32_t)blockIdx.x * TS, win0 = tile >= (uint32_t)TS ? tile - TS : 0u;
    const uint32_t wend = n - tile > (uint32_t)TS ? tile + TS : n;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    for (uint32_t q = win0 + threadIdx.x; q < wend; q += SB) L[q - win0] = IM::of(t[q]);
    __syncthreads();
    uint32_t up = 0, down = 0;
    for (uint32_t p = tile + threadIdx.x; p < wend; p += SB) {
        const uint32_t start = SEG ? off[gid[p]] : 0u;
        const I ti = L[p - win0];
        uint32_t lo = start, hi = p;
        if (start < win0) {                                   // the slice begins in front of the staged rows
            if (within(ti, L[0], lim)) hi = win0; else lo = win0 + 1;
        }
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const I tm = mid >= win0 ? L[mid - win0] : IM::of(t[mid]);
            if (within(ti, tm, lim)) hi = mid; else lo = mid + 1;
        }
        lo_out[p] = lo;
        if (p > start) {                                      // p - 1 >= win0: p > start >= 0 and p >= tile
            const I tp = L[p - 1 - win0];
            up += tp < ti;
            down += tp > ti;
        }
    }
    up = wave_reduce(up, OpAdd{});
    down = wave_reduce(down, OpAdd{});
    if (lane_id() == 0) { if (up) atomicAdd(&cnt[0], up); if (down) atomicAdd(&cnt[1], down); }
    __syncthreads();
    if (threadIdx.x == 0 && (cnt[0] | cnt[1])) atomicAdd(steps, (unsigned long long)cnt[0] | ((unsigned long long)cnt[1] << 32));
}

// ---- the fold over the block tree of fold_tree.hpp ---------------------------------------------------------------------------------
// out[p] = fold of x[min(lo[p], p) .. p].  One workgroup per tile of TS rows; the tile and the tile before it are staged in LDS with
// their 64 elements of level 1, so a window that begins inside them reads nothing else.
template <class T, class ALG, int WR> __global__ void __launch_bounds__(SB)
rangew_fold_kernel(const T* __restrict__ x, uint32_t n, const uint32_t* __restrict__ lo, tree_levels<typename ALG::A> lv, void* __restrict__ outv) {
    using A = typename ALG::A;
    using O = typename rangew_out<T, WR>::type;
    __shared__ T L[2 * TS];
    __shared__ A L1[2 * TS / RX];
    O* __restrict__ out = static_cast<O*>(outv);
    const uint32_t tile = (uint32_t)blockIdx.x * TS, win0 = tile >= (uint32_t)TS ? tile - TS : 0u;
    const uint32_t wend = n - tile > (uint32_t)TS ? tile + TS : n;
    const uint32_t b0 = win0 >> RSH, b1 = (wend + RX - 1) >> RSH;          // the staged elements of level 1: [b0, b1)
    for (uint32_t q = win0 + threadIdx.x; q < wend; q += SB) L[q - win0] = x[q];
    if (b0 + threadIdx.x < b1) L1[threadIdx.x] = lv.T[1][b0 + threadIdx.x];
    __syncthreads();
    auto get0 = [&](uint32_t q) -> A { return ALG::lift(q >= win0 ? L[q - win0] : x[q]); };
    for (uint32_t p = tile + threadIdx.x; p < wend; p += SB) {
        const uint32_t l0 = lo[p];
        uint32_t a = l0 < p ? l0 : p, b = p;
        const uint32_t len = b - a + 1;
        A left = ALG::identity(), mid = ALG::identity(), right = ALG::identity();
        if ((a >> RSH) == (b >> RSH)) {
            for (uint32_t q = a; q <= b; ++q) mid = ALG::op(mid, get0(q));
        } else {
            for (uint32_t q = a; q <= (a | (RX - 1)); ++q) left = ALG::op(left, get0(q));
            for (uint32_t q = b & ~(uint32_t)(RX - 1); q <= b; ++q) right = ALG::op(right, get0(q));
            a = (a >> RSH) + 1; b = (b >> RSH) - 1;                        // whole blocks between: elements [a, b] of level 1
            if (a <= b && a >= b0) {                                       // all of them staged (b < b1: row p is)
                for (uint32_t q = a; q <= b; ++q) mid = ALG::op(mid, L1[q - b0]);
            } else if (a <= b) {
                for (int k = 1; k <= NLV; ++k) {
                    if ((a >> RSH) == (b >> RSH)) {
                        for (uint32_t q = a; q <= b; ++q) mid = ALG::op(mid, lv.T[k][q]);
                        break;
                    }
                    left = ALG::op(left, lv.S[k][a]);
                    right = ALG::op(lv.P[k][b], right);
                    a = (a >> RSH) + 1; b = (b >> RSH) - 1;
                    if (a > b) break;
                }
            }
        }
        const A acc = ALG::op(ALG::op(left, mid), right);
        fold_store<T, WR>(out, p, acc, len);
    }
}
__global__ void __launch_bounds__(SB) rangew_count_kernel(uint32_t n, const uint32_t* __restrict__ lo, uint32_t* __restrict__ out) {
    const uint64_t p = (uint64_t)blockIdx.x * SB + threadIdx.x;
    if (p < n) { const uint32_t l = lo[p]; out[p] = (uint32_t)p - (l < p ? l : (uint32_t)p) + 1; }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
bool stamp_dtype(int t) { return dt_is_num(t) || t == AQG_DATE || t == AQG_TIME; }
int check_times(aqg_ctx* ctx, int tt, const void* times, uint32_t n, const void* lo_out, uint64_t out_bytes) {
    if ((!times || !lo_out) && n) return aqg_fail(ctx, AQG_ERR_ARG, "rangew: null column");
    AQG_CHECK_ROWS(ctx, n, "rangew");
    if (!stamp_dtype(tt)) return aqg_fail(ctx, AQG_ERR_DTYPE, "rangew: numeric, DATE and TIME stamps");
    if (overlaps(lo_out, out_bytes, times, (uint64_t)n * dt_size(tt))) return aqg_fail(ctx, AQG_ERR_ARG, "rangew: out overlaps the stamps");
    return AQG_OK;
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped rangew: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped rangew: the handle was not made by aqg_groupby_build");
    return AQG_OK;
}

// g == nullptr: the whole column.  The workspace is the caller's (aqg_flat_gid may reset it: call before any sub-allocation).
int run_bounds(aqg_ctx* ctx, aqg_groupby* g, int tt, const void* times, uint32_t n, const span_lim& lim, uint32_t* lo_out) {
    const uint32_t *gid = nullptr, *off = nullptr;
    if (g) { AQG_TRY(aqg_flat_gid(ctx, g, &gid)); off = g->flat_off; }
    if (!ctx->rangew_steps) AQG_HIP(ctx, aqg_scratch_malloc(ctx, &ctx->rangew_steps, 256));
    AQG_HIP(ctx, hipMemsetAsync(ctx->rangew_steps, 0, 8, ctx->stream));
    const unsigned grid = aqg_ceil_div(n, TS);
    auto go = [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        const T* t = static_cast<const T*>(times);
        if (g) hipLaunchKernelGGL((rangew_bounds_kernel<T, true>), dim3(grid), dim3(SB), 0, ctx->stream, t, n, lim, gid, off, lo_out, ctx->rangew_steps);
        else hipLaunchKernelGGL((rangew_bounds_kernel<T, false>), dim3(grid), dim3(SB), 0, ctx->stream, t, n, lim, gid, off, lo_out, ctx->rangew_steps);
        return aqg_check_launch(ctx, "rangew_bounds_kernel");
    };
    if (tt == AQG_DATE) return go(aqg_tag<ema_date>{});
    if (tt == AQG_TIME) return go(aqg_tag<ema_time>{});
    return aqg_dispatch_num(tt, go);
}

template <class T, class ALG, int WR> int run_tree(aqg_ctx* ctx, const T* x, uint32_t n, const uint32_t* lo, void* out) {
    tree_levels<typename ALG::A> lv{};
    AQG_TRY((build_tree<T, ALG>(ctx, x, n, lv)));
    aqg_kernel_timer_begin(ctx);
    hipLaunchKernelGGL((rangew_fold_kernel<T, ALG, WR>), dim3(aqg_ceil_div(n, TS)), dim3(SB), 0, ctx->stream, x, n, lo, lv, out);
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "rangew_fold_kernel");
}
// (workspace sized by fold_ws_bytes and not reset in here)
int run_fold(aqg_ctx* ctx, int op, int t, const void* xv, uint32_t n, const uint32_t* lo, void* out) {
    ctx->rangew_fold_n = n;
    if (op == AQG_RANGEW_COUNT) {
        hipLaunchKernelGGL(rangew_count_kernel, dim3(aqg_ceil_div(n, SB)), dim3(SB), 0, ctx->stream, n, lo, static_cast<uint32_t*>(out));
        return aqg_check_launch(ctx, "rangew_count_kernel");
    }
    return fold_dispatch(op, t, [&]<class T, class ALG, int WR>() -> int { return run_tree<T, ALG, WR>(ctx, static_cast<const T*>(xv), n, lo, out); });
}
uint64_t out_bytes(int op, int t, uint32_t n) { return (uint64_t)n * dt_size(out_dtype(op, t)); }

// bounds into workspace, then the fold: the stamps and the values are in one layout (g: the flat layout of that build)
int bounds_then_fold(aqg_ctx* ctx, aqg_groupby* g, int op, int tt, const void* times, const span_lim& lim, int t, const void* x, uint32_t n, void* out) {
    uint32_t* lo;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &lo));
    AQG_TRY(run_bounds(ctx, g, tt, times, n, lim, lo));
    return run_fold(ctx, op, t, x, n, lo, out);
}

} // namespace

extern "C" {

int aqg_rangew_out_dtype(int op, int t) { return out_dtype(op, t); }

int aqg_rangew_bounds(aqg_ctx* ctx, int tt, const void* times, uint32_t n, double span, int frame, uint32_t* lo_out) {
    if (!ctx) return AQG_ERR_ARG;
    span_lim lim;
    AQG_TRY(make_lim(ctx, span, frame, &lim));
    AQG_TRY(check_times(ctx, tt, times, n, lo_out, (uint64_t)n * 4));
    if (n == 0) return AQG_OK;
    return run_bounds(ctx, nullptr, tt, times, n, lim, lo_out);
}

int aqg_grouped_rangew_bounds_flat(aqg_ctx* ctx, aqg_groupby* g, int tt, const void* times_flat, double span, int frame, uint32_t* lo_flat_out) {
    AQG_TRY(check_grouped(ctx, g));
    span_lim lim;
    AQG_TRY(make_lim(ctx, span, frame, &lim));
    AQG_TRY(check_times(ctx, tt, times_flat, g->n, lo_flat_out, (uint64_t)g->n * 4));
    if (g->n == 0 || g->ngroups == 0) return AQG_OK;
    return run_bounds(ctx, g, tt, times_flat, g->n, lim, lo_flat_out);
}

int aqg_rangew_fold(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, const uint32_t* lo, void* out) {
    if (!ctx) return AQG_ERR_ARG;
    AQG_TRY(check_fold(ctx, "rangew", op, t, x, n, true, out));
    if (!lo && n) return aqg_fail(ctx, AQG_ERR_ARG, "rangew: null bounds");
    if (overlaps(out, out_bytes(op, t, n), lo, (uint64_t)n * 4)) return aqg_fail(ctx, AQG_ERR_ARG, "rangew: out overlaps the bounds");
    if (n == 0) return AQG_OK;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, fold_ws_bytes(n)));
    return run_fold(ctx, op, t, x, n, lo, out);
}

int aqg_rangew(aqg_ctx* ctx, int op, int tt, const void* times, double span, int frame, int t, const void* x, uint32_t n, void* out) {
    if (!ctx) return AQG_ERR_ARG;
    span_lim lim;
    AQG_TRY(check_fold(ctx, "rangew", op, t, x, n, true, out));
    AQG_TRY(make_lim(ctx, span, frame, &lim));
    AQG_TRY(check_times(ctx, tt, times, n, out, out_bytes(op, t, n)));
    if (n == 0) return AQG_OK;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * 4 + 1024 + fold_ws_bytes(n)));
    return bounds_then_fold(ctx, nullptr, op, tt, times, lim, t, x, n, out);
}

int aqg_grouped_rangew_flat(aqg_ctx* ctx, aqg_groupby* g, int op, int tt, const void* times_flat, double span, int frame, int t, const void* xflat, void* out_flat) {
    AQG_TRY(check_grouped(ctx, g));
    span_lim lim;
    const uint32_t n = g->n;
    AQG_TRY(check_fold(ctx, "rangew", op, t, xflat, n, true, out_flat));
    AQG_TRY(make_lim(ctx, span, frame, &lim));
    AQG_TRY(check_times(ctx, tt, times_flat, n, out_flat, out_bytes(op, t, n)));
    if (n == 0 || g->ngroups == 0) return AQG_OK;
    const uint32_t* gid;
    AQG_TRY(aqg_flat_gid(ctx, g, &gid));                                  // (made here: it resets the workspace on first use)
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * 4 + 1024 + fold_ws_bytes(n)));
    return bounds_then_fold(ctx, g, op, tt, times_flat, lim, t, xflat, n, out_flat);
}

int aqg_grouped_rangew(aqg_ctx* ctx, aqg_groupby* g, int op, int tt, const void* times_row, double span, int frame, int t, const void* x_row, void* out_flat) {
    AQG_TRY(check_grouped(ctx, g));
    span_lim lim;
    const uint32_t n = g->n;
    AQG_TRY(check_fold(ctx, "rangew", op, t, x_row, n, true, out_flat));
    AQG_TRY(make_lim(ctx, span, frame, &lim));
    AQG_TRY(check_times(ctx, tt, times_row, n, out_flat, out_bytes(op, t, n)));
    if (n == 0 || g->ngroups == 0) return AQG_OK;
    const uint32_t* gid;
    AQG_TRY(aqg_flat_gid(ctx, g, &gid));
    const int tsz = (int)dt_size(tt), xsz = op == AQG_RANGEW_COUNT ? 0 : (int)dt_size(t);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * (tsz + xsz + 4) + 8192 + aqg_postproc_ws_bytes(n, g->ngroups, tsz) + aqg_postproc_ws_bytes(n, g->ngroups, xsz ? xsz : 1) + fold_ws_bytes(n)));
    unsigned char *ts, *xs = nullptr;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n * tsz + 64, &ts));
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, times_row, tsz, ts, /*ws_managed=*/true));
    if (xsz) {
        AQG_TRY(aqg_ws_get(ctx, (size_t)n * xsz + 64, &xs));
        AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x_row, xsz, xs, /*ws_managed=*/true));
    }
    return bounds_then_fold(ctx, g, op, tt, ts, lim, t, xs, n, out_flat);
}

int aqg_rangew_last(aqg_ctx* ctx, uint32_t* nlevels, uint32_t* block_rows, uint32_t* steps_up, uint32_t* steps_down) {
    if (!ctx) return AQG_ERR_ARG;
    AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long st = 0;
    if (ctx->rangew_steps) AQG_HIP(ctx, hipMemcpy(&st, ctx->rangew_steps, 8, hipMemcpyDeviceToHost));
    if (steps_up) *steps_up = (uint32_t)st;
    if (steps_down) *steps_down = (uint32_t)(st >> 32);
    // levels 0 .. L-1: level k holds ceil(n / 64^k) elements in blocks of 64 of them, 64^(k+1) rows; the top level is one block
    uint32_t L = 1;
    while (level_count(ctx->rangew_fold_n, (int)L - 1) > (uint32_t)RX) ++L;
    if (nlevels) *nlevels = L;
    if (block_rows)
        for (uint32_t k = 0; k < 8; ++k) {
            const uint64_t r = k < L ? 1ull << (RSH * (k + 1)) : 0ull;
            block_rows[k] = r > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)r;
        }
    return AQG_OK;
}

} // extern "C"
