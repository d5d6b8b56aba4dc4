// fold_tree.hpp -- the combining-only block tree of radix 64 that the time-range windows (range_window.hip) and the interval fold of
// the window join (join_window.hip) share: the span limits and the result types of the AQG_RANGEW_* aggregates, the checks and the
// op-by-dtype dispatch of a fold (fold_dispatch), the build of the levels and the result store (fold_store).  The walk over the levels
// stays spelled out in each of the two fold kernels: shared as a device function it cost the time-range fold 1 - 3 %.
//
// Level k + 1 holds the fold of every aligned block of 64 elements of level k, and levels >= 1 also hold the prefix and suffix folds
// inside their blocks.  A range [a, b] is the suffix of a's block, the whole blocks between (the same question one level up) and the
// prefix of b's block.  COMBINING ONLY: nothing is ever subtracted back out.  Level 0 keeps no prefix / suffix folds: they would cost
// 2 sizeof(A) bytes per row written and read back (32 for 64-bit sums) against at most 63 reads at either end of a range; the levels
// above cost 3 sizeof(A) / 63 bytes per row all together.  No atomics and no look-back: the bracketing of a floating sum depends on n
// and the two ends alone (and on the kernel: range_window.hip folds staged whole blocks directly, join_window.hip always walks up;
// tests/golden/fold_digests.json pins the bits of both).
#pragma once
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "scan_dev.hpp"

namespace {
using namespace aqgscan;

constexpr int TREE_RX = 64;             // radix of the block tree: one wave folds one block
constexpr int TREE_RSH = 6;
constexpr int NLV = 5;                  // levels above the rows: 64^5 rows per element of level 5, at most 4 of them

// ---- span -> the limits of both distance predicates ---------------------------------------------------------------------------------
// integer stamps: "within <=> d <= dmax" (CLOSED dmax = floor(span), OPEN dmax = ceil(span) - 1, saturated at 2^64 - 1); floating
// stamps compare the rounded distance with the span itself
struct span_lim { uint64_t dmax; double span; int closed; };
// AQG_ERR_ARG for a bad frame or span
int make_lim(aqg_ctx* ctx, double span, int frame, span_lim* lim, const char* who = "rangew") {
    if (frame != AQG_RANGEW_OPEN && frame != AQG_RANGEW_CLOSED) return aqg_fail(ctx, AQG_ERR_ARG, (std::string(who) + ": bad frame").c_str());
    if (!(frame == AQG_RANGEW_CLOSED ? span >= 0.0 : span > 0.0))
        return aqg_fail(ctx, AQG_ERR_ARG, (std::string(who) + ": span >= 0 (closed) or > 0 (open), not NaN").c_str());
    const double c = frame == AQG_RANGEW_CLOSED ? __builtin_floor(span) : __builtin_ceil(span);
    uint64_t d = c >= 18446744073709551616.0 ? ~0ull : (uint64_t)c;
    if (frame == AQG_RANGEW_OPEN && c < 18446744073709551616.0) d -= 1;                 // (c >= 1 here)
    lim->dmax = d; lim->span = span; lim->closed = frame == AQG_RANGEW_CLOSED;
    return AQG_OK;
}

// ---- the aggregates -------------------------------------------------------------------------------------------------------------------
bool good_op(int op) { return op >= AQG_RANGEW_COUNT && op <= AQG_RANGEW_MAX; }
int out_dtype(int op, int t) {
    if (!good_op(op)) return AQG_ERROR;
    if (op == AQG_RANGEW_COUNT) return AQG_UINT32;
    if (!dt_is_num(t)) return AQG_ERROR;
    if (op == AQG_RANGEW_SUM) return aqg_long_type(t);
    return op == AQG_RANGEW_AVG ? AQG_DOUBLE : t;
}
enum : int { RW_SUM = 0, RW_AVG, RW_MINMAX };
template <class T, int WR> struct rangew_out { using type = std::conditional_t<WR == RW_AVG, double, std::conditional_t<WR == RW_MINMAX, T, std::conditional_t<std::is_floating_point_v<T>, double, aqg_i128>>>; };

// The checks of a fold's op, dtype and value column x[0 .. n).  `rangew`: the entries of range_window.hip, whose output has n elements
// as well and is checked here too; each family refuses in the order it always has (errors of several kinds at once are tested).
int check_fold(aqg_ctx* ctx, const char* who, int op, int t, const void* x, uint32_t n, bool rangew = false, const void* out = nullptr) {
    const std::string w(who);
    const bool val = op != AQG_RANGEW_COUNT;
    if (!good_op(op)) return aqg_fail(ctx, AQG_ERR_ARG, (w + ": bad op").c_str());
    if (rangew) {
        if ((!out || (!x && val)) && n) return aqg_fail(ctx, AQG_ERR_ARG, (w + ": null column").c_str());
        if ((uint64_t)n > (uint64_t)AQG_MAX_ROWS) return aqg_fail(ctx, AQG_ERR_ARG, (w + ": more than AQG_MAX_ROWS rows").c_str());
    }
    if (val && !dt_is_num(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, (w + (rangew ? ": the column dtype is not numeric" : ": the value column's dtype is not numeric")).c_str());
    if (!rangew && val && !x && n) return aqg_fail(ctx, AQG_ERR_ARG, (w + ": null column").c_str());
    if (rangew && val && overlaps(out, (size_t)n * dt_size(out_dtype(op, t)), x, (size_t)n * dt_size(t)))
        return aqg_fail(ctx, AQG_ERR_ARG, (w + ": out overlaps an input").c_str());
    return AQG_OK;
}

// the one switch over the aggregates that fold (not COUNT) by numeric dtype: fn.template operator()<T, ALG, WR>()
template <class F> int fold_dispatch(int op, int t, F&& fn) {
    return aqg_dispatch_num(t, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        switch (op) {
        case AQG_RANGEW_SUM: return fn.template operator()<T, sum_alg<T>, RW_SUM>();
        case AQG_RANGEW_AVG: return fn.template operator()<T, sum_alg<T>, RW_AVG>();
        case AQG_RANGEW_MIN: return fn.template operator()<T, min_alg<T>, RW_MINMAX>();
        case AQG_RANGEW_MAX: return fn.template operator()<T, max_alg<T>, RW_MINMAX>();
        }
        return AQG_ERR_ARG;
    });
}

// ---- the block tree ------------------------------------------------------------------------------------------------------------------
template <class A> struct tree_levels { A* T[NLV + 1]; A* P[NLV + 1]; A* S[NLV + 1]; };      // [1 .. NLV]; level 0 is the column itself

// ---- the result store ---------------------------------------------------------------------------------------------------------------
// out[i] = the result of `op` from the accumulator of a range of `len` rows
template <class T, int WR, class A> __device__ inline void fold_store(typename rangew_out<T, WR>::type* __restrict__ out, uint64_t i, const A& acc, uint32_t len) {
    if constexpr (WR == RW_MINMAX) out[i] = acc;
    else if constexpr (WR == RW_AVG) out[i] = sum_alg<T>::to_double(acc) / (double)len;
    else if constexpr (std::is_floating_point_v<T>) out[i] = acc;
    else out[i] = sum_alg<T>::to_i128(acc);                               // (one 16-byte store)
}

// ---- the build -------------------------------------------------------------------------------------------------------------------------
template <class ALG, class A> __device__ inline A wave_prefix(A v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const A y = shfl_up_any(v, o); if (lane >= o) v = ALG::op(y, v); }
    return v;
}
template <class ALG, class A> __device__ inline A wave_suffix(A v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const A y = shfl_idx_any(v, lane + o < 64 ? lane + o : 63); if (lane + o < 64) v = ALG::op(v, y); }
    return v;
}
// One workgroup per 4096 elements of level k (`in`, m of them; RAW: the column, lifted): writes level k + 1 -- the block totals with
// their prefix and suffix folds -- and its own element of level k + 2.  PS_IN: the prefix / suffix folds of level k as well.
template <class ALG, class In, bool RAW, bool PS_IN> __global__ void __launch_bounds__(SB)
rangew_level_kernel(const In* __restrict__ in, uint32_t m, typename ALG::A* __restrict__ Pin, typename ALG::A* __restrict__ Sin,
                    typename ALG::A* __restrict__ T1, typename ALG::A* __restrict__ P1, typename ALG::A* __restrict__ S1, uint32_t m1,
                    typename ALG::A* __restrict__ T2) {
    using A = typename ALG::A;
    __shared__ A tot[TREE_RX];
    const int lane = lane_id(), wave = wave_id();
    const uint64_t wg0 = (uint64_t)blockIdx.x * (TREE_RX * TREE_RX);
    for (int b = wave; b < TREE_RX; b += SB / 64) {
        const uint64_t idx = wg0 + (uint64_t)b * TREE_RX + lane;
        A v = ALG::identity();
        if (idx < m) { if constexpr (RAW) v = ALG::lift(in[idx]); else v = in[idx]; }
        const A pre = wave_prefix<ALG>(v, lane);
        if constexpr (PS_IN) {
            const A suf = wave_suffix<ALG>(v, lane);
            if (idx < m) { Pin[idx] = pre; Sin[idx] = suf; }
        }
        if (lane == 63) tot[b] = pre;
    }
    __syncthreads();
    if (wave == 0) {
        const uint64_t idx = (uint64_t)blockIdx.x * TREE_RX + lane;
        const A v = tot[lane];
        const A pre = wave_prefix<ALG>(v, lane), suf = wave_suffix<ALG>(v, lane);
        if (idx < m1) { T1[idx] = v; P1[idx] = pre; S1[idx] = suf; }
        if (lane == 63) T2[blockIdx.x] = pre;
    }
}

// elements of level k of a column of n rows
uint32_t level_count(uint32_t n, int k) { uint64_t m = n; for (int j = 0; j < k; ++j) m = (m + TREE_RX - 1) / TREE_RX; return (uint32_t)m; }
// workspace of one tree over n rows (build_tree does not reset it)
size_t fold_ws_bytes(uint32_t n) {
    size_t b = 0;
    for (int k = 1; k <= NLV; ++k) b += 3 * ((size_t)level_count(n, k) * 16 + 256);
    return b + 4096;
}

// lv = the levels 1 .. NLV over the column x[0 .. n), from the caller's workspace (sized with fold_ws_bytes): three launches build
// levels 1-2, 3-4 and 5 whatever n is (the last one's element of level 6 goes to a spare slot nobody reads)
template <class T, class ALG> int build_tree(aqg_ctx* ctx, const T* x, uint32_t n, tree_levels<typename ALG::A>& lv) {
    using A = typename ALG::A;
    static_assert(sizeof(A) <= 16, "fold_ws_bytes");
    uint32_t cnt[NLV + 2];
    for (int k = 0; k <= NLV + 1; ++k) cnt[k] = level_count(n, k);
    for (int k = 1; k <= NLV; ++k) {
        AQG_TRY(aqg_ws_get(ctx, (size_t)cnt[k], &lv.T[k]));
        AQG_TRY(aqg_ws_get(ctx, (size_t)cnt[k], &lv.P[k]));
        AQG_TRY(aqg_ws_get(ctx, (size_t)cnt[k], &lv.S[k]));
    }
    A* spare;
    AQG_TRY(aqg_ws_get(ctx, (size_t)1, &spare));
    hipLaunchKernelGGL((rangew_level_kernel<ALG, T, true, false>), dim3(cnt[2]), dim3(SB), 0, ctx->stream, x, n, (A*)nullptr, (A*)nullptr, lv.T[1], lv.P[1], lv.S[1], cnt[1], lv.T[2]);
    AQG_TRY(aqg_check_launch(ctx, "rangew_level_kernel"));
    hipLaunchKernelGGL((rangew_level_kernel<ALG, A, false, true>), dim3(cnt[4]), dim3(SB), 0, ctx->stream, (const A*)lv.T[2], cnt[2], lv.P[2], lv.S[2], lv.T[3], lv.P[3], lv.S[3], cnt[3], lv.T[4]);
    AQG_TRY(aqg_check_launch(ctx, "rangew_level_kernel"));
    hipLaunchKernelGGL((rangew_level_kernel<ALG, A, false, true>), dim3(cnt[6]), dim3(SB), 0, ctx->stream, (const A*)lv.T[4], cnt[4], lv.P[4], lv.S[4], lv.T[5], lv.P[5], lv.S[5], cnt[5], spare);
    return aqg_check_launch(ctx, "rangew_level_kernel");
}

} // namespace
