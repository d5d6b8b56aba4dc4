// ema.hip -- exponential moving averages of a column and of every group of a build: the first-order linear recurrence
//     y[i] = a_i y[i-1] + b_i x[i]                                  (AQG_EMA_RECURSIVE: kdb's ema, pandas ewm(adjust=False).mean())
//     y[i] = N[i] / D[i], N[i] = a_i N[i-1] + x[i], D[i] = a_i D[i-1] + 1      (AQG_EMA_ADJUSTED: pandas ewm(adjust=True).mean())
// with a constant decay a_i = 1 - alpha or a decay COLUMN a_i = decay[i] (time-decayed averages: aqg_decay_from_times).
// The reference has no such function; the contract is include/aqg.h's and the exact model tests/ema_model.py.
//
// A row is an affine map (ema_alg, scan_dev.hpp) and the scan composes maps IN ROW ORDER: the reduce-then-scan pass of scan_prefix.hpp
// (prefix_reduce_kernel -> launch_agg_scan -> prefix_scan_kernel with the W_EMA writer), which goes through the ordered parts only: the
// lane's serial loop over its 8 rows, block_scan_excl, the aggregate scan, seg_alg for the grouped form.  Affine maps do not commute,
// so neither block_fold nor the chained single-pass route of scan.hip may carry them.  No atomics, no look-back: the bracketing depends
// on n, the group starts and the tile geometry alone, and results are bit-reproducible.
// What is EMA's own is ema_rows below: two input columns (the decay form), and a lift that takes the row's position in its slice (a
// first row discards what precedes it) besides its value.
// HBM-bound: sizeof(T) + 8 bytes per row (constant alpha) or sizeof(T) + 16 (decay column), read twice and written once.
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "scan_prefix.hpp"
#include "stamps_dev.hpp"
#include "groupby_handle.hpp"

namespace {
using namespace aqgscan;

// one lane's 8 consecutive rows for the kernels of scan_prefix.hpp: values, decays (DEC), the start bits of the 8 positions (flat
// column: row 0 alone starts a slice -- its lift discards what precedes it, so the fold needs no restart there)
template <class T, bool ADJ, bool DEC, bool SEG_> struct ema_rows : lane_block<SEG_> {
    using In = T;
    using ALG = ema_alg<ADJ>;
    static constexpr bool SEG = SEG_;
    struct args { const T* x; const double* decay; const uint8_t* heads8; double d, alpha; };
    T v[IT];
    double dc[IT];
    bool row0;
    double d, alpha;
    __device__ void load(const args& a, uint32_t n) {
        this->place(n);
        d = a.d; alpha = a.alpha;
        row0 = !SEG && this->base == 0;
        this->fetch(a.x, n, v);
        if constexpr (DEC) this->fetch(a.decay, n, dc);
        this->starts(a.heads8);
    }
    __device__ typename ALG::A lift(int j) const {
        const double xd = (double)v[j];
        if (SEG ? this->head(j) : (row0 && j == 0)) return ALG::lift_first(xd);     // (its decay is not read into the result)
        if constexpr (DEC) return ALG::lift(dc[j], 1.0 - dc[j], xd); else return ALG::lift(d, alpha, xd);
    }
};

// ---- decay[i] = 2^(-|t[i] - t[i-1]| / halflife), decay[0] = 1 --------------------------------------------------------------------------
// (the stamps of DATE / TIME columns: stamps_dev.hpp)
// |a - b| as an unevaluated sum hi + lo of two doubles, EXACT: integers subtract in integer arithmetic first (a difference of 64-bit stamps
// has up to 64 bits), floating columns take the rounding error of their subtraction along
struct dd { double hi, lo; };
template <class T> __device__ inline dd abs_diff(T a, T b) {
    if constexpr (std::is_same_v<T, ema_date> || std::is_same_v<T, ema_time>) return abs_diff(stamp_of(a), stamp_of(b));
    else if constexpr (std::is_floating_point_v<T>) {
        const double x = (double)a, y = (double)b, s = x - y, bb = s - x, e = (x - (s - bb)) + (-y - bb);       // two-sum
        return s < 0 ? dd{-s, -e} : dd{s, e};
    } else {
        const uint64_t hi = (uint64_t)(a > b ? a : b), lo = (uint64_t)(a > b ? b : a), d = hi - lo;
        const double h = (double)d;                                                                         // (rounds beyond 2^53)
        const double l = h >= 18446744073709551616.0 ? -(double)(0ull - d) : (double)(int64_t)(d - (uint64_t)h);
        return {h, l};
    }
}
// 2^(-dt / halflife).  The quotient q is rounded, and exp2 turns its error into q ln2 ulps of the result -- 10 ulp at a decay of 1e-8 --
// so the part of the quotient the rounding lost (the exact remainder of the division and the low word of dt, over halflife) is put
// back to first order: 2^-(q + ql) = 2^-q (1 - ql ln2), |ql ln2| < 2^-53 q.  One fma: exp2's own error and half an ulp are all that is left.
__device__ inline double decay_of(dd dt, double halflife) {
    const double q = dt.hi / halflife;
    double ql = (fma(-q, halflife, dt.hi) + dt.lo) / halflife;
    if (!(fabs(ql) < 1.0)) ql = 0.0;                                     // (q overflowed or is NaN: exp2 alone says what comes back)
    const double e = exp2(-q);
    return fma(e, -ql * 0.6931471805599453, e);
}
// heads: the start bitmap of a flat layout (every group's first decay is 1), or null: row 0 alone is a first row
template <class T> __global__ void __launch_bounds__(SB) decay_kernel(const T* __restrict__ t, uint32_t n, double halflife, const uint32_t* __restrict__ heads, double* __restrict__ out) {
    uint32_t lo, hi;
    wg_span(n, lo, hi, 256);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const bool first = heads ? (heads[i >> 5] >> (i & 31)) & 1u : i == 0;
        out[i] = first ? 1.0 : decay_of(abs_diff(t[i], t[i - 1]), halflife);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct EmaArgs { int mode; double d, alpha; const double* decay; };

size_t ema_ws_bytes(uint32_t n) {
    const size_t ntiles = aqg_ceil_div(n, TS);
    return (ntiles + ntiles / CH + 2) * sizeof(SegCarry<ema_adj>) + 8192;
}
// heads8 == nullptr: the whole column
int dispatch_ema(aqg_ctx* ctx, const EmaArgs& ea, int t, const void* xv, const uint8_t* heads8, uint32_t n, double* out) {
    return aqg_dispatch_num(t, [&](auto tt) -> int {
        using T = typename decltype(tt)::type;
        const T* x = static_cast<const T*>(xv);
        auto by = [&](auto adj, auto dec) -> int {
            constexpr bool ADJ = decltype(adj)::value, DEC = decltype(dec)::value;
            return heads8 ? prefix_pass<ema_rows<T, ADJ, DEC, true>, W_EMA>(ctx, {x, ea.decay, heads8, ea.d, ea.alpha}, n, {}, out, "ema scan")
                          : prefix_pass<ema_rows<T, ADJ, DEC, false>, W_EMA>(ctx, {x, ea.decay, nullptr, ea.d, ea.alpha}, n, {}, out, "ema scan");
        };
        if (ea.mode == AQG_EMA_ADJUSTED) return ea.decay ? by(std::true_type{}, std::true_type{}) : by(std::true_type{}, std::false_type{});
        return ea.decay ? by(std::false_type{}, std::true_type{}) : by(std::false_type{}, std::false_type{});
    });
}

// the checks every entry shares; fills *ea
int check_ema(aqg_ctx* ctx, int mode, int t, const void* x, uint32_t n, double alpha, const double* decay, const double* out, EmaArgs* ea) {
    if (mode != AQG_EMA_RECURSIVE && mode != AQG_EMA_ADJUSTED) return aqg_fail(ctx, AQG_ERR_ARG, "ema: bad mode");
    if (!decay && !(alpha > 0.0 && alpha <= 1.0)) return aqg_fail(ctx, AQG_ERR_ARG, "ema: 0 < alpha <= 1");
    if ((!x || !out) && n) return aqg_fail(ctx, AQG_ERR_ARG, "ema: null column");
    AQG_CHECK_ROWS(ctx, n, "ema");
    if (!dt_is_num(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "ema: the column dtype is not numeric");
    if (overlaps(out, (uint64_t)n * 8, x, (uint64_t)n * dt_size(t)) || overlaps(out, (uint64_t)n * 8, decay, (uint64_t)n * 8))
        return aqg_fail(ctx, AQG_ERR_ARG, "ema: out overlaps an input");
    ea->mode = mode;
    ea->decay = decay;
    ea->alpha = decay ? 0.0 : alpha;
    ea->d = decay ? 0.0 : 1.0 - alpha;
    return AQG_OK;
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped ema: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped ema: the handle was not made by aqg_groupby_build");
    return AQG_OK;
}

} // namespace

extern "C" {

int aqg_scan_ema(aqg_ctx* ctx, int mode, int t, const void* x, uint32_t n, double alpha, const double* decay_dev, double* out) {
    if (!ctx) return AQG_ERR_ARG;
    EmaArgs ea;
    AQG_TRY(check_ema(ctx, mode, t, x, n, alpha, decay_dev, out, &ea));
    if (n == 0) return AQG_OK;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, ema_ws_bytes(n)));
    return dispatch_ema(ctx, ea, t, x, nullptr, n, out);
}

int aqg_grouped_ema_flat(aqg_ctx* ctx, aqg_groupby* g, int mode, int t, const void* xflat, double alpha, const double* decay_flat, double* out_flat) {
    AQG_TRY(check_grouped(ctx, g));
    EmaArgs ea;
    AQG_TRY(check_ema(ctx, mode, t, xflat, g->n, alpha, decay_flat, out_flat, &ea));
    if (g->n == 0 || g->ngroups == 0) return AQG_OK;
    if (!aqg_groupby_offsets(g)) return AQG_ERR_HIP;                      // makes the start bitmap of the flat layout on first use
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, ema_ws_bytes(g->n)));
    return dispatch_ema(ctx, ea, t, xflat, reinterpret_cast<const uint8_t*>(g->flat_heads), g->n, out_flat);
}

int aqg_grouped_ema(aqg_ctx* ctx, aqg_groupby* g, int mode, int t, const void* x, double alpha, const double* decay_row, double* out_flat) {
    AQG_TRY(check_grouped(ctx, g));
    EmaArgs ea;
    AQG_TRY(check_ema(ctx, mode, t, x, g->n, alpha, decay_row, out_flat, &ea));
    const uint32_t n = g->n;
    if (n == 0 || g->ngroups == 0) return AQG_OK;
    if (!aqg_groupby_offsets(g)) return AQG_ERR_HIP;
    const int esz = (int)dt_size(t);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * (esz + (decay_row ? 8 : 0)) + 8192 + aqg_postproc_ws_bytes(n, g->ngroups, esz) + aqg_postproc_ws_bytes(n, g->ngroups, 8) + ema_ws_bytes(n)));
    unsigned char *xs, *ds = nullptr;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n * esz + 64, &xs));
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x, esz, xs, /*ws_managed=*/true));
    if (decay_row) {
        AQG_TRY(aqg_ws_get(ctx, (size_t)n * 8 + 64, &ds));
        AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, decay_row, 8, ds, /*ws_managed=*/true));
        ea.decay = reinterpret_cast<const double*>(ds);
    }
    return dispatch_ema(ctx, ea, t, xs, reinterpret_cast<const uint8_t*>(g->flat_heads), n, out_flat);
}

static int decay_from_times(aqg_ctx* ctx, int t, const void* times, uint32_t n, double halflife, const uint32_t* heads, double* decay_out) {
    if (!(halflife > 0.0) || halflife > 1.7976931348623157e308) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_decay_from_times: halflife > 0 and finite");
    if ((!times || !decay_out) && n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_decay_from_times: null column");
    AQG_CHECK_ROWS(ctx, n, "aqg_decay_from_times");
    if (!dt_is_num(t) && t != AQG_DATE && t != AQG_TIME) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_decay_from_times: numeric, DATE and TIME columns");
    if (overlaps(decay_out, (uint64_t)n * 8, times, (uint64_t)n * dt_size(t))) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_decay_from_times: out overlaps the times");
    if (n == 0) return AQG_OK;
    const unsigned grid = aqg_grid(ctx, n, SB, 4, 16);
    auto go = [&](auto tt) -> int {
        using T = typename decltype(tt)::type;
        hipLaunchKernelGGL((decay_kernel<T>), dim3(grid), dim3(SB), 0, ctx->stream, static_cast<const T*>(times), n, halflife, heads, decay_out);
        return aqg_check_launch(ctx, "decay_kernel");
    };
    if (t == AQG_DATE) return go(aqg_tag<ema_date>{});
    if (t == AQG_TIME) return go(aqg_tag<ema_time>{});
    return aqg_dispatch_num(t, go);
}

int aqg_decay_from_times(aqg_ctx* ctx, int t, const void* times, uint32_t n, double halflife, double* decay_out) {
    if (!ctx) return AQG_ERR_ARG;
    return decay_from_times(ctx, t, times, n, halflife, nullptr, decay_out);
}

int aqg_grouped_decay_from_times_flat(aqg_ctx* ctx, aqg_groupby* g, int t, const void* times_flat, double halflife, double* decay_flat) {
    AQG_TRY(check_grouped(ctx, g));
    if (g->n && g->ngroups && !aqg_groupby_offsets(g)) return AQG_ERR_HIP;
    return decay_from_times(ctx, t, times_flat, g->n, halflife, g->flat_heads, decay_flat);
}

} // extern "C"
