// segscan.hip -- per-group scans, windows and shifts in ONE launch set for all groups: the device form of the generated loop
//     for g: out[g] = scan(w, col[vecs[g]])          (engine/ast.py:696-790; frozen sample mem_opt.cpp:53-63: avgw(10, sales[vecs[i]], col[i]))
// whose results the generated code lays out in one flat buffer sliced by the group offsets (`buf + g.offsets[i]`).
//
// The FLAT LAYOUT of a grouping: position offsets[g] + i holds element i of group g's row list vecs[g] (ht_postproc order,
// server/hasher.h:181-198: descending row id inside a group).  aqg_grouped_flatten brings a column into that layout with the
// value-carrying radix passes of postproc.hip (no row ids, no gather); a bitmap of group starts (`heads`) then makes every scan of
// scan.hip segmented:
//   prefix scans (sums / avgs / mins / maxs / vars / stddevs, the per-group reductions, distance and group index of a position): the
//       pass of scan_prefix.hpp in its SEG = true layout -- reduce-then-scan over 2048-position tiles with the carry
//       {value, last group start, groups so far}; a group start resets the value;
//   windows (sumw / avgw, minw / maxw): the kernels of scan_window.hpp in their by_group form -- tile + halo in LDS, every window
//       clamped at its group's start (no carry between tiles: a window never reaches back further than the halo); varw / stddevw:
//       two passes over windows of up to 64 positions, longer ones from a segmented prefix of moments about the group's first element (any w);
//   shifts (deltas / prev / aggnext / ratiow): neighbour loads guarded by the start bits.
// Integer results are exact; floating sums follow the tile order (tolerance as for the whole-column scans).
// HBM-bound: sizeof(T) + sizeof(out) bytes per row for the scan proper, 12 (one radix pass, <= 256 groups) to 20 x passes for flatten.
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "scan_dev.hpp"
#include "scan_window.hpp"
#include "scan_prefix.hpp"
#include "groupby_handle.hpp"

namespace {
using namespace aqgscan;

struct ipair { int64_t s, q; };
// sum and sum of squares of a group for var / stddev (aggregations.h:332-348): exact for integer columns of up to four bytes -- x * x in the
// C++ type of the operands, like the reference's `arr[i] * arr[i]` -- and in double for floating columns (the square in the column's type)
template <class T> struct varred_alg {
    using A = std::conditional_t<std::is_floating_point_v<T>, dpair, ipair>;
    __device__ static A identity() { A r; r.s = 0; r.q = 0; return r; }
    __device__ static A lift(T v) {
        A r;
        if constexpr (std::is_floating_point_v<T>) { r.s = (double)v; r.q = (double)(T)(v * v); }
        else {
            using P = decltype(v * v);
            using UP = std::make_unsigned_t<P>;
            const P sq = (P)((UP)(P)v * (UP)(P)v);
            r.s = (int64_t)v;
            r.q = (int64_t)sq;
        }
        return r;
    }
    __device__ static A op(A a, A b) { A r; r.s = a.s + b.s; r.q = a.q + b.q; return r; }
};
// ---- group starts ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) heads_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ counts, uint32_t G,
                                                    uint32_t* __restrict__ heads, uint32_t* __restrict__ shorts, uint32_t short_w) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g <= G; g += gridDim.x * blockDim.x) {
        const uint32_t p = off[g];                                       // g == G: the end of the table, a start nobody owns
        if (heads) atomicOr(&heads[p >> 5], 1u << (p & 31));
        if (shorts && g < G && counts[g] <= short_w) atomicOr(&shorts[p >> 5], 1u << (p & 31));
    }
}
// ---- shifts / ratios --------------------------------------------------------------------------------------------------------------
template <class T, int OP>
__global__ void __launch_bounds__(SB) seg_shift_kernel(const T* __restrict__ x, uint32_t n, uint32_t w, const uint32_t* __restrict__ heads,
                                                       const uint32_t* __restrict__ shorts, void* __restrict__ out) {
    using FP = std::conditional_t<sizeof(T) == 4, float, double>;           // GetFPType
    using O = std::conditional_t<OP == AQG_SCAN_RATIOW, FP, T>;
    uint32_t lo, hi;
    wg_span(n, lo, hi, 256);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const T cur = x[i];
        O r;
        if constexpr (OP == AQG_SCAN_DELTAS) r = head_bit(heads, i) ? (T)0 : (T)(cur - x[i - 1]);          // ret[0] = 0 (aggregations.h:441)
        else if constexpr (OP == AQG_SCAN_PREV) r = head_bit(heads, i) ? cur : x[i - 1];                     // ret[0] = arr[0] (:457)
        else if constexpr (OP == AQG_SCAN_NEXT) r = head_bit(heads, i + 1) ? cur : x[i + 1];                 // the last row repeats (:476)
        else {
            // ratiow (:169-183): a group of at most w rows degrades to w = min(w, 1); the first w rows divide by the group's first row
            const uint32_t d = dist_to_head(heads, i, w);
            uint32_t we = w;
            if (shorts && d < w && head_bit(shorts, i - d)) we = w ? 1u : 0u;
            const T prv = d < we ? x[i - d] : x[i - we];
            r = (FP)(cur / (FP)prv);
        }
        static_cast<O*>(out)[i] = r;
    }
}

// four consecutive positions per lane (vector load / store, the start bits of the four as one nibble); ratios = ratiow(1) included.
// Needs 16-byte aligned columns (sub-views of columns take the scalar kernel above).  1e9 rows: deltas 2.7 -> see DESIGN.md
template <class T, int OP>
__global__ void __launch_bounds__(SB) seg_shift4_kernel(const T* __restrict__ x, uint32_t n, const uint32_t* __restrict__ heads, void* __restrict__ out) {
    using FP = std::conditional_t<sizeof(T) == 4, float, double>;
    using O = std::conditional_t<OP == AQG_SCAN_RATIOW, FP, T>;
    constexpr int V = 4;
    const uint32_t nv = n / V;
    const uint32_t q = blockIdx.x * SB + threadIdx.x;
    if (q < nv) {
        const uint32_t p = q * V;
        const pack<T, V> c = *reinterpret_cast<const pack<T, V>*>(x + p);
        const uint32_t hw = heads[p >> 5] >> (p & 31);                 // bits of p .. p+3 (p is a multiple of 4: they share a word)
        pack<O, V> o;
        if constexpr (OP == AQG_SCAN_NEXT) {
            const T right = head_bit(heads, p + V) ? c.v[V - 1] : x[p + V];   // (bit n is set: no read beyond the column)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool last = j + 1 < V ? ((hw >> (j + 1)) & 1u) : head_bit(heads, p + V);
                o.v[j] = last ? c.v[j] : (j + 1 < V ? c.v[j + 1] : right);
            }
        } else {
            const T left = (hw & 1u) ? c.v[0] : x[p - 1];               // (position 0 starts a group: no read in front of the column)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool h = (hw >> j) & 1u;
                const T prv = j ? c.v[j - 1] : left;
                if constexpr (OP == AQG_SCAN_DELTAS) o.v[j] = h ? (T)0 : (T)(c.v[j] - prv);
                else if constexpr (OP == AQG_SCAN_PREV) o.v[j] = h ? c.v[j] : prv;
                else o.v[j] = (FP)(c.v[j] / (FP)(h ? c.v[j] : prv));
            }
        }
        *reinterpret_cast<pack<O, V>*>(static_cast<O*>(out) + p) = o;
    }
    if (q == 0) {                                                       // the last n % 4 positions
        for (uint32_t i = nv * V; i < n; ++i) {
            const T cur = x[i];
            const bool h = head_bit(heads, i);
            O r;
            if constexpr (OP == AQG_SCAN_DELTAS) r = h ? (T)0 : (T)(cur - x[i - 1]);
            else if constexpr (OP == AQG_SCAN_PREV) r = h ? cur : x[i - 1];
            else if constexpr (OP == AQG_SCAN_NEXT) r = head_bit(heads, i + 1) ? cur : x[i + 1];
            else r = (FP)(cur / (FP)(h ? cur : x[i - 1]));
            static_cast<O*>(out)[i] = r;
        }
    }
}

__global__ void __launch_bounds__(256) ends_kernel(const uint32_t* __restrict__ off, uint32_t G, uint32_t* __restrict__ last_pos) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) last_pos[g] = off[g + 1] - 1;
}
__global__ void __launch_bounds__(256) counts64_kernel(const uint32_t* __restrict__ counts, uint32_t G, uint64_t* __restrict__ out) {
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) out[g] = counts[g];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
size_t heads_bytes(uint32_t n) { return (((size_t)n + 32) / 32 + 8) * 4; }      // bit n included, two words of padding (the byte behind a block is read)

// offsets + start bitmap of the flat layout, made once per build (uses the workspace: call before any sub-allocation of a call)
int ensure_flat(aqg_ctx* ctx, aqg_groupby* g) {
    if (g->flat_valid) return AQG_OK;
    const uint32_t n = g->n, G = g->ngroups;
    AQG_TRY(aqg_dev_realloc(ctx, &g->flat_off, &g->cap_flat_off, ((size_t)G + 2) * 4));
    AQG_TRY(aqg_dev_realloc(ctx, &g->flat_heads, &g->cap_flat_heads, heads_bytes(n)));
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, ((size_t)(G + 2048) / 2048 + 16) * 4 + 4096));
    uint32_t* bsum;
    AQG_TRY(aqg_ws_get(ctx, (G + 2048) / 2048 + 16, &bsum));
    AQG_TRY(aqg_group_offsets(ctx, g, g->flat_off, bsum));
    AQG_HIP(ctx, hipMemsetAsync(g->flat_heads, 0, heads_bytes(n), ctx->stream));
    hipLaunchKernelGGL(heads_kernel, dim3(aqg_grid(ctx, (uint64_t)G + 1, 256, 1, 8)), dim3(256), 0, ctx->stream, g->flat_off, g->counts, G, g->flat_heads, (uint32_t*)nullptr, 0u);
    AQG_TRY(aqg_check_launch(ctx, "heads_kernel"));
    g->flat_valid = true;
    g->flat_gid_valid = false;
    g->flat_short_w = 0;
    g->rank_big_valid = false;
    return AQG_OK;
}
int ensure_short(aqg_ctx* ctx, aqg_groupby* g, uint32_t w) {
    if (g->flat_short_w == w && g->flat_short) return AQG_OK;
    AQG_TRY(aqg_dev_realloc(ctx, &g->flat_short, &g->cap_flat_short, heads_bytes(g->n)));
    AQG_HIP(ctx, hipMemsetAsync(g->flat_short, 0, heads_bytes(g->n), ctx->stream));
    hipLaunchKernelGGL(heads_kernel, dim3(aqg_grid(ctx, (uint64_t)g->ngroups + 1, 256, 1, 8)), dim3(256), 0, ctx->stream, g->flat_off, g->counts, g->ngroups,
                       (uint32_t*)nullptr, g->flat_short, w);
    AQG_TRY(aqg_check_launch(ctx, "heads_kernel"));
    g->flat_short_w = w;
    return AQG_OK;
}

size_t carry_ws_bytes(uint32_t n) {
    const size_t ntiles = aqg_ceil_div(n, TS);
    return ntiles * 48 + (ntiles / CH + 2) * 48 + 4096;
}
const uint8_t* heads8_of(const aqg_groupby* g) { return reinterpret_cast<const uint8_t*>(g->flat_heads); }
// one segmented prefix pass (workspace already sized)
template <class T, class ALG, int WR>
int seg_pass(aqg_ctx* ctx, aqg_groupby* g, const T* x, uint32_t n, void* out) {
    static_assert(sizeof(SegCarry<typename ALG::A>) <= 48, "carry_ws_bytes");
    return prefix_pass<value_rows<T, ALG, true>, WR>(ctx, {x, heads8_of(g)}, n, {}, out, "segmented prefix scan");
}
int dist_column(aqg_ctx* ctx, aqg_groupby* g, uint32_t n, uint32_t* D) { return prefix_pass<position_rows, W_DIST>(ctx, {heads8_of(g)}, n, {}, D, "segmented prefix scan"); }

// what window_scan (scan_window.hpp) asks of a layout, for the flat layout of a grouping
template <class T> struct group_windows {
    using seg_t = by_group;
    aqg_ctx* ctx; aqg_groupby* g; const T* x; uint32_t n; unsigned row_grid;
    by_group seg() const { return {g->flat_heads, nullptr}; }
    int reserve(size_t) { return AQG_OK; }                           // the caller sized the workspace (scan_ws_bytes) and it is not reset in here
    int raw_prefix(typename sum_alg<T>::A* S) { return seg_pass<T, sum_alg<T>, W_RAW>(ctx, g, x, n, S); }
    int moments(dpair* P) { return seg_pass<T, mom_alg<T>, W_MOM>(ctx, g, x, n, P); }
    int distances(by_group& s) {
        uint32_t* D;
        AQG_TRY(aqg_ws_get(ctx, n, &D));
        s.D = D;
        return dist_column(ctx, g, n, D);
    }
};

size_t scan_ws_bytes(int op, int t, uint32_t n, uint32_t w) {
    size_t need = carry_ws_bytes(n) * 2 + 65536;
    const size_t esz = aqg_dtype_size(t);
    switch (op) {
    case AQG_SCAN_SUMW: case AQG_SCAN_AVGW: need += (size_t)n * (4 + 16) + 8192; break;          // (only the wide-window path uses them)
    case AQG_SCAN_MINW: case AQG_SCAN_MAXW: need += (size_t)n * (4 + 2 * esz) + 8192; break;
    case AQG_SCAN_VARW: case AQG_SCAN_STDDEVW: need += (size_t)n * (4 + sizeof(dpair)) + 8192; break;   // (windows longer than VAR_DIRECT_MAX_W)
    default: break;
    }
    (void)w;
    return need;
}

// the scan of a column already in the flat layout (workspace sized by scan_ws_bytes and not reset in here)
int scan_flat(aqg_ctx* ctx, aqg_groupby* g, int op, int t, const void* xv, uint32_t w, void* out) {
    const uint32_t n = g->n;
    const uint32_t* heads = g->flat_heads;
    if (op == AQG_SCAN_RATIOW && w >= 2) AQG_TRY(ensure_short(ctx, g, w));
    const uint32_t* shorts = (op == AQG_SCAN_RATIOW && w >= 2) ? g->flat_short : nullptr;
    return aqg_dispatch_num(t, [&](auto tt) -> int {
        using T = typename decltype(tt)::type;
        const T* x = static_cast<const T*>(xv);
        const unsigned egrid = aqg_grid(ctx, n, SB, 4, 16);
        auto shift = [&](auto kern, const char* what) -> int {
            aqg_kernel_timer_begin(ctx);
            hipLaunchKernelGGL(kern, dim3(egrid), dim3(SB), 0, ctx->stream, x, n, w, heads, shorts, out);
            aqg_kernel_timer_end(ctx);
            return aqg_check_launch(ctx, what);
        };
        group_windows<T> grp{ctx, g, x, n, egrid};
        const bool al16 = ((reinterpret_cast<uintptr_t>(xv) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 && n >= 4;
        auto shift4 = [&](auto kern, const char* what) -> int {
            aqg_kernel_timer_begin(ctx);
            hipLaunchKernelGGL(kern, dim3(aqg_ceil_div(n / 4, SB)), dim3(SB), 0, ctx->stream, x, n, heads, out);
            aqg_kernel_timer_end(ctx);
            return aqg_check_launch(ctx, what);
        };
        switch (op) {
        case AQG_SCAN_SUMS: return seg_pass<T, sum_alg<T>, W_SUMS>(ctx, g, x, n, out);
        case AQG_SCAN_AVGS: return seg_pass<T, sum_alg<T>, W_AVGS>(ctx, g, x, n, out);
        case AQG_SCAN_MINS: return seg_pass<T, min_alg<T>, W_MINS>(ctx, g, x, n, out);
        case AQG_SCAN_MAXS: return seg_pass<T, max_alg<T>, W_MAXS>(ctx, g, x, n, out);
        case AQG_SCAN_VARS: return seg_pass<T, mom_alg<T>, W_VARS>(ctx, g, x, n, out);
        case AQG_SCAN_STDDEVS: return seg_pass<T, mom_alg<T>, W_STDDEVS>(ctx, g, x, n, out);
        case AQG_SCAN_VARW: case AQG_SCAN_STDDEVW: case AQG_SCAN_SUMW: case AQG_SCAN_AVGW:
            return window_scan(ctx, grp, op, x, n, w > n ? n : w, out);                 // (a window is clamped by its group anyway)
        case AQG_SCAN_DELTAS: return al16 ? shift4(&seg_shift4_kernel<T, AQG_SCAN_DELTAS>, "deltas (grouped)") : shift(&seg_shift_kernel<T, AQG_SCAN_DELTAS>, "deltas (grouped)");
        case AQG_SCAN_PREV: return al16 ? shift4(&seg_shift4_kernel<T, AQG_SCAN_PREV>, "prev (grouped)") : shift(&seg_shift_kernel<T, AQG_SCAN_PREV>, "prev (grouped)");
        case AQG_SCAN_NEXT: return al16 ? shift4(&seg_shift4_kernel<T, AQG_SCAN_NEXT>, "aggnext (grouped)") : shift(&seg_shift_kernel<T, AQG_SCAN_NEXT>, "aggnext (grouped)");
        case AQG_SCAN_RATIOW: return (al16 && w == 1) ? shift4(&seg_shift4_kernel<T, AQG_SCAN_RATIOW>, "ratios (grouped)") : shift(&seg_shift_kernel<T, AQG_SCAN_RATIOW>, "ratiow (grouped)");
        case AQG_SCAN_MINW: case AQG_SCAN_MAXW: {
            const bool is_max = op == AQG_SCAN_MAXW;
            // the deque never expires anything when w == 0 or w >= n: the running min / max of the group (no seed)
            if (w == 0 || w >= n) return is_max ? seg_pass<T, max_alg<T>, W_MAXP>(ctx, g, x, n, out) : seg_pass<T, min_alg<T>, W_MINP>(ctx, g, x, n, out);
            return window_scan(ctx, grp, op, x, n, w, out);
        }
        }
        return AQG_ERR_ARG;
    });
}

int check_build(aqg_ctx* ctx, const aqg_groupby* g, const char* what) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, what);
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped scan: the handle was not made by aqg_groupby_build");
    return AQG_OK;
}
int flat_esz(int t) {
    switch (t) {
    case AQG_INT8: case AQG_UINT8: case AQG_BOOL: case AQG_CHAR: return 1;
    case AQG_INT16: case AQG_UINT16: return 2;
    case AQG_INT32: case AQG_UINT32: case AQG_FLOAT: case AQG_DATE: return 4;
    case AQG_INT64: case AQG_UINT64: case AQG_DOUBLE: case AQG_TIME: return 8;
    }
    return 0;
}

} // namespace

// the group index of every flat position, cached in the handle (one segmented pass over the start bitmap on first use; resets the workspace then)
int aqg_flat_gid(aqg_ctx* ctx, aqg_groupby* g, const uint32_t** gid) {
    AQG_TRY(ensure_flat(ctx, g));
    if (!g->flat_gid_valid) {
        const uint32_t n = g->n;
        AQG_TRY(aqg_ws_reset(ctx));
        AQG_TRY(aqg_ws_ensure(ctx, carry_ws_bytes(n) * 2 + 65536));
        AQG_TRY(aqg_dev_realloc(ctx, &g->flat_gid, &g->cap_flat_gid, ((size_t)n + 4) * 4));
        AQG_TRY((prefix_pass<position_rows, W_GID>(ctx, {heads8_of(g)}, n, {}, g->flat_gid, "segmented prefix scan")));
        g->flat_gid_valid = true;
    }
    *gid = g->flat_gid;
    return AQG_OK;
}

extern "C" {

const uint32_t* aqg_groupby_offsets(aqg_groupby* g) {
    if (!g || !g->has_counts) return nullptr;
    return ensure_flat(g->ctx, g) == AQG_OK ? g->flat_off : nullptr;
}

int aqg_grouped_flatten(aqg_ctx* ctx, aqg_groupby* g, int t, const void* x, void* out_flat) {
    AQG_TRY(check_build(ctx, g, "aqg_grouped_flatten: bad argument"));
    if ((!x || !out_flat) && g->n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_flatten: bad argument");
    const int esz = flat_esz(t);
    if (!esz) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_grouped_flatten: 1-, 2-, 4- and 8-byte elements");
    if (g->n == 0) return AQG_OK;
    return aqg_radix_by_group(ctx, g, nullptr, x, esz, out_flat, /*ws_managed=*/false);
}

int aqg_grouped_scan_flat(aqg_ctx* ctx, aqg_groupby* g, int op, int t, const void* xflat, uint32_t w, void* out_flat) {
    AQG_TRY(check_build(ctx, g, "aqg_grouped_scan_flat: bad argument"));
    if ((!xflat || !out_flat) && g->n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_scan_flat: bad argument");
    if (op < 0 || op > AQG_SCAN_STDDEVW) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_scan_flat: bad op");
    if (w == 0 && (op == AQG_SCAN_SUMW || op == AQG_SCAN_AVGW || op == AQG_SCAN_VARW || op == AQG_SCAN_STDDEVW))
        return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_scan: window 0 is undefined for sumw/avgw/varw");
    if (!dt_is_num(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "grouped scan: the column dtype is not numeric");
    if (g->n == 0) return AQG_OK;
    AQG_TRY(ensure_flat(ctx, g));
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, scan_ws_bytes(op, t, g->n, w)));
    return scan_flat(ctx, g, op, t, xflat, w, out_flat);
}

int aqg_grouped_scan(aqg_ctx* ctx, aqg_groupby* g, int op, int t, const void* x, uint32_t w, void* out_flat) {
    AQG_TRY(check_build(ctx, g, "aqg_grouped_scan: bad argument"));
    if ((!x || !out_flat) && g->n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_scan: bad argument");
    if (op < 0 || op > AQG_SCAN_STDDEVW) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_scan: bad op");
    if (w == 0 && (op == AQG_SCAN_SUMW || op == AQG_SCAN_AVGW || op == AQG_SCAN_VARW || op == AQG_SCAN_STDDEVW))
        return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_scan: window 0 is undefined for sumw/avgw/varw");
    if (!dt_is_num(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "grouped scan: the column dtype is not numeric");
    const uint32_t n = g->n;
    if (n == 0) return AQG_OK;
    AQG_TRY(ensure_flat(ctx, g));
    const int esz = flat_esz(t);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * esz + 4096 + aqg_postproc_ws_bytes(n, g->ngroups, esz) + scan_ws_bytes(op, t, n, w)));
    unsigned char* xs;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n * esz + 64, &xs));
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x, esz, xs, /*ws_managed=*/true));
    return scan_flat(ctx, g, op, t, xs, w, out_flat);
}

// out[g] = op(flat[offsets[g] .. offsets[g+1])): reductions of per-group scan results (`max(ratios(x[vecs[g]]))`, tests/q4.a:23)
int aqg_grouped_reduce_flat(aqg_ctx* ctx, aqg_groupby* g, int op, int t, const void* xflat, void* out_dev) {
    AQG_TRY(check_build(ctx, g, "aqg_grouped_reduce_flat: bad argument"));
    if ((!xflat && g->n) || !out_dev) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_grouped_reduce_flat: bad argument");
    if (!dt_is_num(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_grouped_reduce_flat: value dtype");
    const uint32_t n = g->n, G = g->ngroups;
    if (G == 0) return AQG_OK;
    AQG_TRY(ensure_flat(ctx, g));
    if (op == AQG_RED_COUNT) {
        hipLaunchKernelGGL(counts64_kernel, dim3(aqg_grid(ctx, G, 256, 1, 8)), dim3(256), 0, ctx->stream, g->counts, G, static_cast<uint64_t*>(out_dev));
        return aqg_check_launch(ctx, "counts64_kernel");
    }
    if (op == AQG_RED_FIRST) return aqg_gather(ctx, t, xflat, g->flat_off, G, out_dev);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, carry_ws_bytes(n) * 2 + (size_t)G * 4 + 65536));
    if (op == AQG_RED_LAST) {
        uint32_t* lastp;
        AQG_TRY(aqg_ws_get(ctx, G, &lastp));
        hipLaunchKernelGGL(ends_kernel, dim3(aqg_grid(ctx, G, 256, 1, 8)), dim3(256), 0, ctx->stream, g->flat_off, G, lastp);
        return aqg_gather(ctx, t, xflat, lastp, G, out_dev);
    }
    if (op == AQG_RED_SUM || op == AQG_RED_AVG || op == AQG_RED_MIN || op == AQG_RED_MAX) {
        return aqg_dispatch_num(t, [&](auto tt) -> int {
            using T = typename decltype(tt)::type;
            const T* x = static_cast<const T*>(xflat);
            switch (op) {
            case AQG_RED_SUM: return seg_pass<T, sum_alg<T>, W_RED_SUM>(ctx, g, x, n, out_dev);
            case AQG_RED_AVG: return seg_pass<T, sum_alg<T>, W_RED_AVG>(ctx, g, x, n, out_dev);
            case AQG_RED_MIN: return seg_pass<T, min_alg<T>, W_RED_MIN>(ctx, g, x, n, out_dev);
            default: return seg_pass<T, max_alg<T>, W_RED_MAX>(ctx, g, x, n, out_dev);
            }
        });
    }
    if ((op == AQG_RED_VAR || op == AQG_RED_STDDEV) && (aqg_dtype_size(t) <= 4 || dt_is_fp(t))) {
        return aqg_dispatch_num(t, [&](auto tt) -> int {
            using T = typename decltype(tt)::type;
            if constexpr (sizeof(T) <= 4 || std::is_floating_point_v<T>) {
                const T* x = static_cast<const T*>(xflat);
                return op == AQG_RED_VAR ? seg_pass<T, varred_alg<T>, W_RED_VAR>(ctx, g, x, n, out_dev) : seg_pass<T, varred_alg<T>, W_RED_STDDEV>(ctx, g, x, n, out_dev);
            } else return AQG_ERR_DTYPE;
        });
    }
    // VAR / STDDEV: through the group-by plans, keyed by the group index of every flat position
    const uint32_t* gid;
    AQG_TRY(aqg_flat_gid(ctx, g, &gid));
    return aqg_grouped_reduce_keyed(ctx, g, gid, op, t, xflat, out_dev);
}

} // extern "C"
