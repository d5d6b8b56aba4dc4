// pair_window.hip -- moving and running statistics of TWO columns: covw / corrw / betaw over the last min(w, rows so far) rows and the
// running covs / corrs / betas, for a whole column and for every group of a grouping's flat layout (include/aqg_pair.h).
//
// The rule is that of the variance scans (scan_dev.hpp): no cancellation against anything wider than it must be.
//   ROUTE_REG / ROUTE_LDS (w <= 8 / w <= 64)   var_short_tile for two columns: one tile of 2048 rows per workgroup, both columns and
//       their w - 1 row halo staged in LDS, two passes over the window -- the means of the differences from an anchor INSIDE the window,
//       then the co-deviations.  Direct sums, no subtraction of anything outside the window: a non-finite row acts on the windows that
//       hold it and on no other.
//   ROUTE_PREFIX (longer windows, the running ops)   the co-moment algebra of scan_dev.hpp (comom_alg: anchors = the group's first row)
//       through the reduce-then-scan pass of scan_prefix.hpp; a running op is the prefix itself, a window the difference of two prefixes
//       (three to five doubles a row in workspace).
// The columns have any two of the ten numeric dtypes: a row is staged once into an 8-byte slot (scan_dev.hpp: slot_load) by a
// wave-uniform switch, so there is one kernel per (route, op family, layout) and none per (TX, TY).
// The grouped forms take the layouts of scan_window.hpp (whole_column / by_group): group starts, clamping and the distance column are
// the shared ones.
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "scan_dev.hpp"
#include "scan_window.hpp"
#include "scan_prefix.hpp"
#include "groupby_handle.hpp"
#include "pair_route.hpp"

namespace {
using namespace aqgscan;

static_assert(aqgpair::TILE_ROWS == (uint32_t)TS && aqgpair::REG_MAX_W == (uint32_t)VAR_REG_W && aqgpair::LDS_MAX_W == VAR_DIRECT_MAX_W && aqgpair::CHUNK == CH,
              "pair_route.hpp restates the scan geometry");
static_assert((int)AQG_SCAN2_COVS == (int)aqgpair::OP_COVS && (int)AQG_SCAN2_COVW == (int)aqgpair::OP_COVW && (int)AQG_SCAN2_BETAW == (int)aqgpair::OP_BETAW &&
              (uint32_t)AQG_SCAN2_ROUTE_REG == (uint32_t)aqgpair::ROUTE_REG && (uint32_t)AQG_SCAN2_ROUTE_LDS == (uint32_t)aqgpair::ROUTE_LDS &&
              (uint32_t)AQG_SCAN2_ROUTE_PREFIX == (uint32_t)aqgpair::ROUTE_PREFIX, "pair_route.hpp restates aqg_scan2op");
static_assert(sizeof(comom) == 64 && sizeof(SegCarry<comom>) == 72, "the aggregates pair_ws sizes");

struct pair_cols { const void* x; const void* y; int tx, ty; };

// ---- the short routes ---------------------------------------------------------------------------------------------------------------
// FAM 0 cov / 1 corr / 2 beta: only the sums the statistic needs (three / five / four).  RW > 0: the window's differences (w <= RW) are
// kept in registers, anchored at the position's own row; RW == 0: both passes read LDS, anchored at the window's first row.  Lane t
// takes positions t, t + SB, ...: consecutive lanes read consecutive 8-byte slots (no bank conflict) and store consecutive doubles.
template <int FAM, int RW, class M>
__global__ void __launch_bounds__(SB) pair_short_kernel(pair_cols c, uint32_t n, uint32_t w, M seg, double* __restrict__ out) {
    __shared__ uint64_t LX[TS + VAR_DIRECT_MAX_W], LY[TS + VAR_DIRECT_MAX_W];
    const uint32_t H = w - 1, tile_start = blockIdx.x * TS;
    for (uint32_t q = threadIdx.x; q < H + TS; q += SB) {
        const int64_t g = (int64_t)tile_start - (int64_t)H + q;
        const bool in = g >= 0 && g < (int64_t)n;
        LX[q] = in ? slot_load(c.x, c.tx, (uint64_t)g) : 0ull;
        LY[q] = in ? slot_load(c.y, c.ty, (uint64_t)g) : 0ull;
    }
    __syncthreads();
    // (wave-uniform: columns without an 8-byte integer take the loop whose differences are plain double subtractions -- with the
    // run-time choice inside the window loops w = 64 over doubles ran at 8.6 ms per 1e8 rows)
    const bool wx = slot_wide(c.tx), wy = slot_wide(c.ty);
    auto rows = [&]<bool WIDE>() {
        auto difx = [&](uint64_t v, uint64_t k) { return slot_diff(v, k, WIDE && wx); };
        auto dify = [&](uint64_t v, uint64_t k) { return slot_diff(v, k, WIDE && wy); };
        for (uint32_t j = threadIdx.x; j < TS; j += SB) {
            const uint32_t p = tile_start + j;
            if (p >= n) break;
            const uint32_t len = seg.len(p, w), idx = H + j;           // L[idx] holds row p; len <= w, so idx + 1 - len >= 0
            const double dn = (double)len;
            double cxy = 0, cxx = 0, cyy = 0;
            if constexpr (RW > 0) {
                const uint64_t kx = LX[idx], ky = LY[idx];
                double dx[RW], dy[RW], sx = 0, sy = 0;
#pragma unroll
                for (int e = 0; e < RW; ++e) {
                    const bool live = (uint32_t)e < len;
                    dx[e] = live ? difx(LX[idx - e], kx) : 0.0;
                    dy[e] = live ? dify(LY[idx - e], ky) : 0.0;
                    sx += dx[e];
                    sy += dy[e];
                }
                const double mx = sx / dn, my = sy / dn;
#pragma unroll
                for (int e = 0; e < RW; ++e) if ((uint32_t)e < len) {
                    const double a = dx[e] - mx, b = dy[e] - my;
                    cxy += a * b;
                    if constexpr (FAM != 0) cxx += a * a;
                    if constexpr (FAM == 1) cyy += b * b;
                }
            } else {
                const uint32_t lo = idx + 1 - len;
                const uint64_t kx = LX[lo], ky = LY[lo];
                double sx = 0, sy = 0;
                for (uint32_t e = lo + 1; e <= idx; ++e) { sx += difx(LX[e], kx); sy += dify(LY[e], ky); }
                const double mx = sx / dn, my = sy / dn;
                for (uint32_t e = lo; e <= idx; ++e) {
                    const double a = difx(LX[e], kx) - mx, b = dify(LY[e], ky) - my;
                    cxy += a * b;
                    if constexpr (FAM != 0) cxx += a * a;
                    if constexpr (FAM == 1) cyy += b * b;
                }
            }
            out[p] = pair_finish<FAM>(cxy, cxx, cyy, dn);
        }
    };
    if (wx || wy) rows.template operator()<true>(); else rows.template operator()<false>();
}

// ---- the prefix route ---------------------------------------------------------------------------------------------------------------
// the rows of the pass: the lane's eight slots of either column
template <class T> __device__ inline void slots_of(const void* __restrict__ col, uint32_t n, uint32_t base, uint64_t (&dst)[IT]) {
    T t[IT];
    uint32_t cnt;
    load_tile_items(static_cast<const T*>(col), n, base, t, cnt);
#pragma unroll
    for (int j = 0; j < IT; ++j) {
        if constexpr (sizeof(T) == 8 && std::is_integral_v<T>) dst[j] = (uint32_t)j < cnt ? (uint64_t)t[j] : 0ull;
        else dst[j] = (uint32_t)j < cnt ? slot_of((double)t[j]) : 0ull;
    }
}
__device__ inline void fetch_slots(const void* __restrict__ col, int t, uint32_t n, uint32_t base, uint64_t (&dst)[IT]) {
    switch (t) {
    case AQG_INT8: slots_of<int8_t>(col, n, base, dst); break;
    case AQG_INT16: slots_of<int16_t>(col, n, base, dst); break;
    case AQG_INT32: slots_of<int32_t>(col, n, base, dst); break;
    case AQG_UINT8: slots_of<uint8_t>(col, n, base, dst); break;
    case AQG_UINT16: slots_of<uint16_t>(col, n, base, dst); break;
    case AQG_UINT32: slots_of<uint32_t>(col, n, base, dst); break;
    case AQG_FLOAT: slots_of<float>(col, n, base, dst); break;
    case AQG_DOUBLE: slots_of<double>(col, n, base, dst); break;
    default: slots_of<uint64_t>(col, n, base, dst); break;        // INT64 / UINT64: the bits
    }
}
template <bool SEG_> struct pair_rows : lane_block<SEG_> {
    using In = double;
    using ALG = comom_alg;
    static constexpr bool SEG = SEG_;
    struct args { pair_cols c; const uint8_t* heads8; /* SEG */ };
    uint64_t vx[IT], vy[IT];
    uint32_t fl;
    __device__ void load(const args& a, uint32_t n) {
        this->place(n);
        fl = (slot_wide(a.c.tx) ? 1u : 0u) | (slot_wide(a.c.ty) ? 2u : 0u);
        fetch_slots(a.c.x, a.c.tx, n, this->base, vx);
        fetch_slots(a.c.y, a.c.ty, n, this->base, vy);
        this->starts(a.heads8);
    }
    __device__ comom lift(int j) const { return comom_alg::lift(vx[j], vy[j], fl); }
};

// windows of any length: P[i] = the anchored sums of i's group up to i (one pair of anchors per group); the window is the difference
// of two of them
template <int FAM, class M>
__global__ void __launch_bounds__(SB) pair_prefix_diff_kernel(const dsums<pair_sums(FAM)>* __restrict__ P, M seg, uint32_t n, uint32_t w, double* __restrict__ out) {
    constexpr int NS = pair_sums(FAM);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t d = seg.dist(i), len = d + 1 < w ? d + 1 : w;
        dsums<NS> a = P[i];
        if (len <= d) {
            const dsums<NS> b = P[i - len];
#pragma unroll
            for (int k = 0; k < NS; ++k) a.v[k] -= b.v[k];
        }
        out[i] = pair_value<FAM>(a.v[0], a.v[1], a.v[2], a.v[NS > 3 ? 3 : 0], a.v[NS > 4 ? 4 : 0], (double)len);   // (sums a family lacks are not read)
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// The aggregates' scan stays in one workgroup (CHUNKED = false): the chunk kernels would be three more instantiations over a 72-byte
// aggregate for 0.1 ms at 1e8 rows.
template <bool SEG, int WR>
int pair_pass(aqg_ctx* ctx, const pair_cols& c, const uint8_t* heads8, uint32_t n, void* out) {
    using ROWS = pair_rows<SEG>;
    using O = typename prefix_out<double, WR>::type;
    AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(&prefix_scan_kernel<ROWS, WR>), (size_t)TS * sizeof(O)));   // (five doubles a row: 80 KB)
    return prefix_pass<ROWS, WR, false>(ctx, {c, heads8}, n, {}, out, "pair prefix scan", /*timed=*/false);
}

// g == nullptr: the n rows are one group.  Else the groups of g, both columns in the flat layout.  Resets and sizes the workspace.
template <bool SEG>
int run_pair(aqg_ctx* ctx, aqg_groupby* g, int op, const pair_cols& c, uint32_t n, uint32_t w, double* out) {
    using M = std::conditional_t<SEG, by_group, whole_column>;
    using C = typename carry_alg<comom_alg, SEG>::A;
    using DC = typename carry_alg<none_alg, true>::A;
    const int fam = aqgpair::op_family(op);
    const uint32_t route = aqgpair::route_of(op, n, w), ww = aqgpair::clamp_window(w, n);
    const uint8_t* heads8 = nullptr;
    M seg{};
    if constexpr (SEG) {
        if (!aqg_groupby_offsets(g)) return AQG_ERR_HIP;             // (makes the start bitmap on first use and resets the workspace then)
        seg = by_group{g->flat_heads, nullptr};
        heads8 = reinterpret_cast<const uint8_t*>(g->flat_heads);
    }
    ctx->scan2_route = route;
    ctx->scan2_tile = TS;
    AQG_TRY(aqg_ws_reset(ctx));
    if (route != aqgpair::ROUTE_PREFIX) {
        const uint32_t ntiles = aqg_ceil_div(n, TS);
        auto go = [&](auto kern) { return launch_window(ctx, kern, ntiles, SB, 0, "pair_short_kernel", c, n, ww, seg, out); };
        const bool reg = route == aqgpair::ROUTE_REG;
        switch (fam) {
        case 0: return reg ? go(&pair_short_kernel<0, VAR_REG_W, M>) : go(&pair_short_kernel<0, 0, M>);
        case 1: return reg ? go(&pair_short_kernel<1, VAR_REG_W, M>) : go(&pair_short_kernel<1, 0, M>);
        default: return reg ? go(&pair_short_kernel<2, VAR_REG_W, M>) : go(&pair_short_kernel<2, 0, M>);
        }
    }
    AQG_TRY(aqg_ws_ensure(ctx, aqgpair::ws_bytes(op, n, w, SEG, sizeof(C), sizeof(DC))));
    aqg_kernel_timer_begin(ctx);                                      // the timer spans every pass of the route
    int rc;
    if (aqgpair::op_running(op)) {
        rc = fam == 0 ? pair_pass<SEG, W_COVS>(ctx, c, heads8, n, out) : fam == 1 ? pair_pass<SEG, W_CORRS>(ctx, c, heads8, n, out) : pair_pass<SEG, W_BETAS>(ctx, c, heads8, n, out);
        aqg_kernel_timer_end(ctx);
        return rc;
    }
    const unsigned grid = aqg_grid(ctx, n, SB, 4, 16);
    auto windows = [&]<int FAM, int WR>() -> int {
        // (the prefix first in the arena, then the aggregates of its pass, then -- per group -- the distances and their pass)
        dsums<pair_sums(FAM)>* P;
        AQG_TRY(aqg_ws_get(ctx, n, &P));
        AQG_TRY((pair_pass<SEG, WR>(ctx, c, heads8, n, P)));
        if constexpr (SEG) {
            // (what group_windows::distances() of segscan.hip does: that struct takes ONE typed column and is local to its file; the
            // layout type by_group, its clamping and the W_DIST pass are the shared ones -- keep the two in step)
            uint32_t* D;
            AQG_TRY(aqg_ws_get(ctx, n, &D));
            seg.D = D;
            AQG_TRY((prefix_pass<position_rows, W_DIST>(ctx, {heads8}, n, {}, D, "segmented prefix scan", /*timed=*/false)));
        }
        hipLaunchKernelGGL((pair_prefix_diff_kernel<FAM, M>), dim3(grid), dim3(SB), 0, ctx->stream, P, seg, n, ww, out);
        return aqg_check_launch(ctx, "pair_prefix_diff_kernel");
    };
    rc = fam == 0 ? windows.template operator()<0, W_CO3>() : fam == 1 ? windows.template operator()<1, W_CO5>() : windows.template operator()<2, W_CO4>();
    aqg_kernel_timer_end(ctx);
    return rc;
}

// the checks every entry shares (n rows of dtypes tx, ty at x, y; n doubles at out)
int check_pair(aqg_ctx* ctx, int op, int tx, const void* x, int ty, const void* y, uint32_t n, uint32_t w, const void* out) {
    if (!aqgpair::op_known(op)) return aqg_fail(ctx, AQG_ERR_ARG, "scan2: unknown op");
    if (!aqgpair::op_running(op) && w == 0) return aqg_fail(ctx, AQG_ERR_ARG, "scan2: window 0 is undefined for covw / corrw / betaw");
    if (!dt_is_num(tx) || !dt_is_num(ty)) return aqg_fail(ctx, AQG_ERR_DTYPE, "scan2: the column dtypes are not numeric (128-bit results are not inputs)");
    if ((!x || !y || !out) && n) return aqg_fail(ctx, AQG_ERR_ARG, "scan2: null column");
    AQG_CHECK_ROWS(ctx, n, "scan2");
    return AQG_OK;
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped scan2: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped scan2: the handle was not made by aqg_groupby_build");
    return AQG_OK;
}
int esz_of(int t) { return (int)aqg_dtype_size(t); }

} // namespace

extern "C" {

int aqg_scan2(aqg_ctx* ctx, int op, int tx, const void* x, int ty, const void* y, uint32_t n, uint32_t w, double* out) {
    if (!ctx) return AQG_ERR_ARG;
    AQG_TRY(check_pair(ctx, op, tx, x, ty, y, n, w, out));
    if (n == 0) return AQG_OK;
    return run_pair<false>(ctx, nullptr, op, pair_cols{x, y, tx, ty}, n, w, out);
}

int aqg_grouped_scan2_flat(aqg_ctx* ctx, aqg_groupby* g, int op, int tx, const void* xflat, int ty, const void* yflat, uint32_t w, double* out_flat) {
    AQG_TRY(check_grouped(ctx, g));
    AQG_TRY(check_pair(ctx, op, tx, xflat, ty, yflat, g->n, w, out_flat));
    if (g->n == 0 || g->ngroups == 0) return AQG_OK;
    return run_pair<true>(ctx, g, op, pair_cols{xflat, yflat, tx, ty}, g->n, w, out_flat);
}

int aqg_grouped_scan2(aqg_ctx* ctx, aqg_groupby* g, int op, int tx, const void* x_row, int ty, const void* y_row, uint32_t w, double* out_flat) {
    AQG_TRY(check_grouped(ctx, g));
    AQG_TRY(check_pair(ctx, op, tx, x_row, ty, y_row, g->n, w, out_flat));
    const uint32_t n = g->n;
    if (n == 0 || g->ngroups == 0) return AQG_OK;
    // flatten + the flat form: the two flat columns outlive the workspace of the radix passes in one pool buffer
    const size_t xb = ((size_t)n * esz_of(tx) + 64 + 255) & ~(size_t)255, yb = (size_t)n * esz_of(ty) + 64;
    PoolBuf keep(ctx);
    AQG_TRY(keep.get(xb + yb));
    char* kp = static_cast<char*>(keep.p);
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x_row, esz_of(tx), kp, /*ws_managed=*/false));
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, y_row, esz_of(ty), kp + xb, /*ws_managed=*/false));
    return run_pair<true>(ctx, g, op, pair_cols{kp, kp + xb, tx, ty}, n, w, out_flat);
}

int aqg_scan2_last(aqg_ctx* ctx, uint32_t* route, uint32_t* tile_rows) {
    if (!ctx || !route || !tile_rows) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_scan2_last: bad argument");
    *route = ctx->scan2_route;
    *tile_rows = ctx->scan2_tile;
    return AQG_OK;
}

} // extern "C"
