// join_window.hip -- the window join (kdb's wj / wj1, an interval join followed by an aggregate): for every probe row an aggregate of
// the build rows that share its key tuple and whose `on` lies within `before` in front of / `after` behind the probe row's own
// (include/aqg.h: aqg_join_window; the contract restated executably: tests/wj_model.py).
//
//   group, order   asof_order.hpp, shared with the as-of join: gid[np], the build rows by (group, on, row), their images.
//   bounds   wj_bounds_kernel: four consecutive probe rows per lane and TWO binary searches per probe row over img[off[g] .. off[g+1]):
//            lo = the first row that is not in front of the window, hi = the first row that is behind it or NaN.  All eight searches
//            of a lane advance in lock step; the trip count is the wavefront's longest segment, every step predicated per lane, the
//            loads of a step issued before its compares.  Integer images are affine in the value: the difference of two images IS
//            the distance.  Floating images are not: the values come back out of the images (unimg_fp) and are subtracted in double,
//            once, which is monotone in the build value -- the searches are exact against a model that subtracts the same way.
//            LDS: the images and the offsets copied into LDS first (small build sides under large probe sides); HBM: read in place.
//   fold     interval_fold_kernel over the block tree of fold_tree.hpp (shared with the time-range windows): one query [lo, hi) per
//            lane anywhere in a column -- the suffix walk in lo's block, S[k] / P[k] up the levels, a direct loop where both ends
//            meet in one block, the prefix walk in (hi - 1)'s block.  STAGED: the column and its level 1 copied into LDS first;
//            INPLACE: read from HBM / L2.  Both routes combine the same operands in the same order: their results agree bit for bit.
#include "asof_order.hpp"
#include "fold_tree.hpp"

namespace {

// ---- bounds --------------------------------------------------------------------------------------------------------------------------
struct WjArgs {
    const uint32_t* gid;           // [np] group of the probe row or NONE; nullptr: no key columns, every row in group 0
    const void* probe_on;
    uint32_t np;
    const void* img;               // [nb] images in (group, on, row) order
    const uint32_t* off;           // [G + 1] segment offsets; nullptr: one segment [0, nb)
    uint32_t nb, G;
    int kind, fp, prevailing, aligned;
    span_lim before, after;        // (dmax clamped to the image's width)
    uint32_t *lo, *hi;
};

// the value a floating image stands for (both zeros: +0.0; the NaN image: a NaN)
template <class U> __device__ inline double wj_value(U i) {
    if constexpr (sizeof(U) == 4) return (double)__uint_as_float(unimg_fp<uint32_t>(i));
    else return __longlong_as_double((long long)unimg_fp<uint64_t>(i));
}
// is the distance of two images, big > small, within the span?
template <class U> __device__ inline bool wj_within(int fp, U big, U small, const span_lim& s) {
    if (fp) { const double d = wj_value(big) - wj_value(small); return s.closed ? d <= s.span : d < s.span; }
    return (uint64_t)(U)(big - small) <= s.dmax;
}

// The windows of R probe rows per lane.  EVERY lane of the wavefront calls this (rows that do not exist come with live == false): the
// trip count is the wavefront's longest segment, and a lane whose searches are over keeps stepping with n == 0, reading element 0.
// Each step issues the 2 R loads of the 2 R searches before any of them is compared.
template <class U, int R>
__device__ inline void wj_search(const WjArgs& a, const U* img, const uint32_t* off, const uint32_t (&g)[R], const U (&key)[R], bool live,
                                 uint32_t (&rlo)[R], uint32_t (&rhi)[R]) {
    const U nan_img = img_fp_nan<U>();
    uint32_t pl[R], nl[R], ph[R], nh[R], sb[R];
    uint32_t maxn = 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const bool go = live && g[q] != NONE && !(a.fp && key[q] == nan_img);
        const uint32_t gg = go ? g[q] : 0u;
        uint32_t b = 0, e = a.nb;
        if (off) { b = off[gg]; e = off[gg + 1]; }
        sb[q] = go ? b : 0u;
        pl[q] = ph[q] = sb[q];
        nl[q] = nh[q] = go ? e - b : 0u;
        maxn = nl[q] > maxn ? nl[q] : maxn;
    }
    maxn = wave_reduce(maxn, OpMax{});
    const int trips = 32 - __clz(maxn);                // a segment of L rows is decided in floor(log2 L) + 1 halvings
    for (int t = 0; t < trips; ++t) {
        U vl[R], vh[R];
        uint32_t ml[R], mh[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            ml[q] = nl[q] ? pl[q] + (nl[q] >> 1) : 0u; vl[q] = img[ml[q]];
            mh[q] = nh[q] ? ph[q] + (nh[q] >> 1) : 0u; vh[q] = img[mh[q]];
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            // lower bound: mid is in front of the window -- earlier than the probe row and beyond `before`
            const uint32_t hl = nl[q] >> 1;
            const bool front = nl[q] && vl[q] < key[q] && !wj_within<U>(a.fp, key[q], vl[q], a.before);
            pl[q] = front ? ml[q] + 1 : pl[q];
            nl[q] = front ? nl[q] - hl - 1 : hl;
            // upper bound: mid is not behind the window -- not NaN, and not later than the probe row by more than `after`
            const uint32_t hh = nh[q] >> 1;
            const bool behind = (a.fp && vh[q] == nan_img) || (vh[q] > key[q] && !wj_within<U>(a.fp, vh[q], key[q], a.after));
            const bool inside = nh[q] && !behind;
            ph[q] = inside ? mh[q] + 1 : ph[q];
            nh[q] = inside ? nh[q] - hh - 1 : hh;
        }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {                      // (no window: sb == pl == ph == 0)
        rlo[q] = a.prevailing && pl[q] > sb[q] ? pl[q] - 1 : pl[q];        // the row in front of the window: rows before lo are never NaN
        rhi[q] = ph[q];
    }
}

template <class U, bool LDS>
__global__ void __launch_bounds__(256) wj_bounds_kernel(WjArgs a) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const U* img = static_cast<const U*>(a.img);
    const uint32_t* off = a.off;
    if constexpr (LDS) {                               // [nb] images, [G + 1] offsets
        U* li = reinterpret_cast<U*>(smem_raw);
        uint32_t* lf = reinterpret_cast<uint32_t*>(li + a.nb);
        for (uint32_t j = threadIdx.x; j < a.nb; j += blockDim.x) li[j] = img[j];
        for (uint32_t j = threadIdx.x; j <= a.G; j += blockDim.x) lf[j] = off ? off[j] : (j ? a.nb : 0u);
        __syncthreads();
        img = li; off = lf;
    }
    const uint32_t nchunk = a.aligned ? a.np / AR : 0u;
    uint32_t c_lo, c_hi;
    wg_span(nchunk, c_lo, c_hi);
    for (uint32_t base = c_lo; base < c_hi; base += blockDim.x) {          // (uniform over the workgroup: every lane reaches the search)
        const uint32_t ch = base + threadIdx.x;
        const bool live = ch < c_hi;
        uint32_t g[AR] = {0u, 0u, 0u, 0u}, rlo[AR], rhi[AR];
        uint64_t raw[AR] = {0ull, 0ull, 0ull, 0ull};
        U key[AR];
        if (live) {
            if (a.gid) {
                const pack<uint32_t, 4> gv = *reinterpret_cast<const pack<uint32_t, 4>*>(a.gid + (size_t)ch * AR);
#pragma unroll
                for (int q = 0; q < AR; ++q) g[q] = gv.v[q];
            }
            on_load4(a.kind, a.probe_on, ch, raw);
        }
#pragma unroll
        for (int q = 0; q < AR; ++q) key[q] = on_img<U>(a.kind, raw[q]);
        wj_search<U, AR>(a, img, off, g, key, live, rlo, rhi);
        if (live) {
            pack<uint32_t, 4> ol, oh;
#pragma unroll
            for (int q = 0; q < AR; ++q) { ol.v[q] = rlo[q]; oh.v[q] = rhi[q]; }
            *reinterpret_cast<pack<uint32_t, 4>*>(a.lo + (size_t)ch * AR) = ol;
            *reinterpret_cast<pack<uint32_t, 4>*>(a.hi + (size_t)ch * AR) = oh;
        }
    }
    // the tail, and every row of columns or outputs off the vector width
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)nchunk * AR + (uint64_t)blockIdx.x * blockDim.x; base < a.np; base += stride) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < a.np;
        uint32_t g[1] = {0u}, rlo[1], rhi[1];
        U key[1] = {U(0)};
        if (live) {
            if (a.gid) g[0] = a.gid[i];
            key[0] = on_img<U>(a.kind, on_raw(a.kind, a.probe_on, (size_t)i));
        }
        wj_search<U, 1>(a, img, off, g, key, live, rlo, rhi);
        if (live) { a.lo[i] = rlo[0]; a.hi[i] = rhi[0]; }
    }
}

__global__ void __launch_bounds__(256) wj_iota_kernel(uint32_t n, uint32_t* __restrict__ out) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) out[j] = j;
}

// ---- the fold --------------------------------------------------------------------------------------------------------------------------
struct wj_fill16 { uint64_t w[2]; };                   // the bytes of *fill_host, zero-extended
template <class O> __device__ inline O wj_fill_as(const wj_fill16& f) { O o; __builtin_memcpy(&o, &f, sizeof(O)); return o; }

// out[i] = fold of x[lo[i] .. min(hi[i], n)), one query per lane; an empty interval writes `empty` (sums: zero; AVG / MIN / MAX: the fill).
// STAGED: level 1 and the column are in LDS (dynamic: cnt1 accumulators, then n elements).
template <class T, class ALG, int WR, bool STAGED> __global__ void __launch_bounds__(256)
interval_fold_kernel(const T* __restrict__ x, uint32_t n, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, uint32_t m,
                     tree_levels<typename ALG::A> lv, uint32_t cnt1, wj_fill16 fill, void* __restrict__ outv) {
    using A = typename ALG::A;
    using O = typename rangew_out<T, WR>::type;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    O* __restrict__ out = static_cast<O*>(outv);
    const T* x0 = x;
    const A* t1 = lv.T[1];
    if constexpr (STAGED) {
        A* l1 = reinterpret_cast<A*>(smem_raw);
        T* lx = reinterpret_cast<T*>(l1 + cnt1);
        for (uint32_t j = threadIdx.x; j < cnt1; j += blockDim.x) l1[j] = lv.T[1][j];
        for (uint32_t j = threadIdx.x; j < n; j += blockDim.x) lx[j] = x[j];
        __syncthreads();
        x0 = lx; t1 = l1;
    }
    const O empty = WR == RW_SUM ? O{} : wj_fill_as<O>(fill);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        uint32_t a = lo[i], e = hi[i];
        e = e < n ? e : n;
        if (a >= e) { out[i] = empty; continue; }
        uint32_t b = e - 1;
        const uint32_t len = e - a;
        A left = ALG::identity(), mid = ALG::identity(), right = ALG::identity();
        if ((a >> TREE_RSH) == (b >> TREE_RSH)) {
            for (uint32_t q = a; q <= b; ++q) mid = ALG::op(mid, ALG::lift(x0[q]));
        } else {
            for (uint32_t q = a; q <= (a | (TREE_RX - 1)); ++q) left = ALG::op(left, ALG::lift(x0[q]));
            for (uint32_t q = b & ~(uint32_t)(TREE_RX - 1); q <= b; ++q) right = ALG::op(right, ALG::lift(x0[q]));
            a = (a >> TREE_RSH) + 1; b = (b >> TREE_RSH) - 1;                        // whole blocks between: elements [a, b] of level 1
            if (a <= b) {
                for (int k = 1; k <= NLV; ++k) {
                    if ((a >> TREE_RSH) == (b >> TREE_RSH)) {
                        const A* tk = k == 1 ? t1 : lv.T[k];
                        for (uint32_t q = a; q <= b; ++q) mid = ALG::op(mid, tk[q]);
                        break;
                    }
                    left = ALG::op(left, lv.S[k][a]);
                    right = ALG::op(lv.P[k][b], right);
                    a = (a >> TREE_RSH) + 1; b = (b >> TREE_RSH) - 1;
                    if (a > b) break;
                }
            }
        }
        const A acc = ALG::op(ALG::op(left, mid), right);
        fold_store<T, WR>(out, i, acc, len);
    }
}
__global__ void __launch_bounds__(256) interval_count_kernel(uint32_t n, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, uint32_t m,
                                                             uint32_t* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t a = lo[i], e = hi[i] < n ? hi[i] : n;
        out[i] = a < e ? e - a : 0u;
    }
}
// every interval is empty (a column of no rows): out[i] = the empty value, elements of 4, 8 or 16 bytes
template <class O> __global__ void __launch_bounds__(256) wj_empty_kernel(uint32_t m, wj_fill16 v, O* __restrict__ out) {
    const O e = wj_fill_as<O>(v);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) out[i] = e;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
constexpr int WJ_FLAGS = AQG_WJ_OPEN_LO | AQG_WJ_OPEN_HI | AQG_WJ_PREVAILING;

void wj_clear(aqg_ctx* ctx) { ctx->wj_routes = ctx->wj_groups = ctx->wj_passes = 0; }

// the bytes an empty window writes: zero for COUNT and SUM, *fill_host (NULL: zero) for AVG / MIN / MAX
wj_fill16 empty_value(int op, int odt, const void* fill_host) {
    wj_fill16 f{{0, 0}};
    if (fill_host && op != AQG_RANGEW_COUNT && op != AQG_RANGEW_SUM) memcpy(&f, fill_host, dt_size(odt));
    return f;
}
int write_empty(aqg_ctx* ctx, int odt, const wj_fill16& f, uint32_t m, void* out) {
    const unsigned grid = aqg_grid(ctx, m, 256, 4, 8);
    switch (dt_size(odt)) {
    case 1: hipLaunchKernelGGL((wj_empty_kernel<uint8_t>), dim3(grid), dim3(256), 0, ctx->stream, m, f, static_cast<uint8_t*>(out)); break;
    case 2: hipLaunchKernelGGL((wj_empty_kernel<uint16_t>), dim3(grid), dim3(256), 0, ctx->stream, m, f, static_cast<uint16_t*>(out)); break;
    case 4: hipLaunchKernelGGL((wj_empty_kernel<uint32_t>), dim3(grid), dim3(256), 0, ctx->stream, m, f, static_cast<uint32_t*>(out)); break;
    case 8: hipLaunchKernelGGL((wj_empty_kernel<uint64_t>), dim3(grid), dim3(256), 0, ctx->stream, m, f, static_cast<uint64_t*>(out)); break;
    default: hipLaunchKernelGGL((wj_empty_kernel<aqg_i128>), dim3(grid), dim3(256), 0, ctx->stream, m, f, static_cast<aqg_i128*>(out)); break;
    }
    return aqg_check_launch(ctx, "wj_empty_kernel");
}

template <class T, class ALG, int WR>
int fold_tree_run(aqg_ctx* ctx, const T* x, uint32_t n, const uint32_t* lo, const uint32_t* hi, uint32_t m, const wj_fill16& fill, void* out, uint32_t* route) {
    using A = typename ALG::A;
    tree_levels<A> lv{};
    AQG_TRY((build_tree<T, ALG>(ctx, x, n, lv)));
    const uint32_t cnt1 = level_count(n, 1);
    const size_t lds = (size_t)n * sizeof(T) + (size_t)cnt1 * sizeof(A);
    const bool staged = join_lds_route(lds, m);
    *route = staged ? AQG_WJ_FOLD_STAGED : AQG_WJ_FOLD_INPLACE;
    const unsigned grid = aqg_grid(ctx, m, 256, 1, staged ? (lds <= 20 * 1024 ? 8 : 3) : 16);
    aqg_kernel_timer_begin(ctx);
    if (staged) hipLaunchKernelGGL((interval_fold_kernel<T, ALG, WR, true>), dim3(grid), dim3(256), lds, ctx->stream, x, n, lo, hi, m, lv, cnt1, fill, out);
    else hipLaunchKernelGGL((interval_fold_kernel<T, ALG, WR, false>), dim3(grid), dim3(256), 0, ctx->stream, x, n, lo, hi, m, lv, cnt1, fill, out);
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "interval_fold_kernel");
}

// the fold of m > 0 queries over a column of n rows (workspace: reset here, sized with fold_ws_bytes); *route: the AQG_WJ_FOLD_* bit
int fold_run(aqg_ctx* ctx, int op, int t, const void* xv, uint32_t n, const uint32_t* lo, const uint32_t* hi, uint32_t m, const void* fill_host,
             void* out, uint32_t* route) {
    *route = 0;
    const int odt = out_dtype(op, t);
    const wj_fill16 fill = empty_value(op, odt, fill_host);
    if (n == 0) return write_empty(ctx, odt, fill, m, out);
    if (op == AQG_RANGEW_COUNT) {
        hipLaunchKernelGGL(interval_count_kernel, dim3(aqg_grid(ctx, m, 256, 4, 8)), dim3(256), 0, ctx->stream, n, lo, hi, m, static_cast<uint32_t*>(out));
        return aqg_check_launch(ctx, "interval_count_kernel");
    }
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, fold_ws_bytes(n)));
    return fold_dispatch(op, t, [&]<class T, class ALG, int WR>() -> int {
        return fold_tree_run<T, ALG, WR>(ctx, static_cast<const T*>(xv), n, lo, hi, m, fill, out, route);
    });
}

struct WjSides : JoinSides { span_lim before, after; };

// the checks the three join entries share (asof_order.hpp's of the two sides, then the spans)
int check_wj_sides(aqg_ctx* ctx, int flags, int nkeys, const int* dts, const void* const* bk, const void* build_on, uint32_t nb, const void* const* pk,
                   const void* probe_on, uint32_t np, int on_dtype, double before, double after, WjSides* s) {
    AQG_TRY(check_sides(ctx, "aqg_join_window", flags, WJ_FLAGS, nkeys, dts, bk, build_on, nb, pk, probe_on, np, on_dtype, s));
    AQG_TRY(make_lim(ctx, before, (flags & AQG_WJ_OPEN_LO) ? AQG_RANGEW_OPEN : AQG_RANGEW_CLOSED, &s->before, "aqg_join_window (before)"));
    return make_lim(ctx, after, (flags & AQG_WJ_OPEN_HI) ? AQG_RANGEW_OPEN : AQG_RANGEW_CLOSED, &s->after, "aqg_join_window (after)");
}

// order (into order_out), then lo / hi of every probe row; nb, np > 0.  Queued on the stream: the caller keeps `ord` until it drained.
template <class U>
int bounds_run(aqg_ctx* ctx, AsofOrder<U>& ord, const WjSides& s, uint32_t* order_out, uint32_t* lo, uint32_t* hi, uint32_t* routes) {
    AQG_TRY(ord.run(ctx, "aqg_join_window", s.nkeys, s.dts, s.bk, s.build_on, s.nb, s.pk, s.np, s.kind, s.on_dtype, order_out));
    if (!ord.srt) {                                    // in order as it stands
        hipLaunchKernelGGL(wj_iota_kernel, dim3(aqg_grid(ctx, s.nb, 256, 4, 8)), dim3(256), 0, ctx->stream, s.nb, order_out);
        AQG_TRY(aqg_check_launch(ctx, "wj_iota_kernel"));
    }
    WjArgs a{};
    a.gid = ord.gid; a.probe_on = s.probe_on; a.np = s.np;
    a.img = ord.img; a.off = ord.off; a.nb = s.nb; a.G = ord.G;
    a.kind = s.kind; a.fp = s.kind == ON_F32 || s.kind == ON_F64; a.prevailing = (s.flags & AQG_WJ_PREVAILING) != 0;
    a.before = s.before; a.after = s.after;
    if (sizeof(U) == 4) {                              // distances of 32-bit images are below 2^32
        if (a.before.dmax > 0xFFFFFFFFull) a.before.dmax = 0xFFFFFFFFull;
        if (a.after.dmax > 0xFFFFFFFFull) a.after.dmax = 0xFFFFFFFFull;
    }
    a.aligned = ((reinterpret_cast<uintptr_t>(lo) | reinterpret_cast<uintptr_t>(hi) | reinterpret_cast<uintptr_t>(s.probe_on) | reinterpret_cast<uintptr_t>(ord.gid)) & 15) == 0;
    a.lo = lo; a.hi = hi;
    const size_t table = ord.table_bytes(s.nb);        // the as-of join's table bytes decide the route; the rows are not staged here
    const bool use_lds = join_lds_route(table, s.np);
    const size_t lds = (size_t)s.nb * sizeof(U) + ((size_t)ord.G + 1) * 4;
    const unsigned grid = join_probe_grid(ctx, s.np, AR, use_lds, lds);
    aqg_kernel_timer_begin(ctx);
    if (use_lds) hipLaunchKernelGGL((wj_bounds_kernel<U, true>), dim3(grid), dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL((wj_bounds_kernel<U, false>), dim3(grid), dim3(256), 0, ctx->stream, a);
    aqg_kernel_timer_end(ctx);
    AQG_TRY(aqg_check_launch(ctx, "wj_bounds_kernel"));
    *routes = ord.routes | (use_lds ? AQG_ASOF_ROUTE_LDS : AQG_ASOF_ROUTE_HBM);
    return AQG_OK;
}

template <class U>
int bounds_call(aqg_ctx* ctx, const WjSides& s, uint32_t* order_out, uint32_t* lo, uint32_t* hi) {
    AsofOrder<U> ord(ctx);
    uint32_t routes = 0;
    AQG_TRY(bounds_run<U>(ctx, ord, s, order_out, lo, hi, &routes));
    AQG_TRY(aqg_sync(ctx));                            // the kernels read the handle's and the pool's buffers
    ctx->wj_routes = routes; ctx->wj_groups = ord.G; ctx->wj_passes = ord.passes;
    return AQG_OK;
}

template <class U>
int window_call(aqg_ctx* ctx, const WjSides& s, int op, int t, const void* build_x, const void* fill_host, void* out) {
    AsofOrder<U> ord(ctx);
    PoolBuf order(ctx), lo(ctx), hi(ctx), xs(ctx);
    AQG_TRY(order.get((size_t)s.nb * 4));
    AQG_TRY(lo.get((size_t)s.np * 4));
    AQG_TRY(hi.get((size_t)s.np * 4));
    uint32_t routes = 0, fold_route = 0;
    AQG_TRY(bounds_run<U>(ctx, ord, s, static_cast<uint32_t*>(order.p), static_cast<uint32_t*>(lo.p), static_cast<uint32_t*>(hi.p), &routes));
    const void* x = build_x;
    if (op != AQG_RANGEW_COUNT && ord.srt) {           // (a build side in order as it stands is its own gather)
        AQG_TRY(xs.get((size_t)s.nb * dt_size(t)));
        AQG_TRY(aqg_gather(ctx, t, build_x, static_cast<const uint32_t*>(order.p), s.nb, xs.p));
        x = xs.p;
    }
    AQG_TRY(fold_run(ctx, op, t, x, s.nb, static_cast<const uint32_t*>(lo.p), static_cast<const uint32_t*>(hi.p), s.np, fill_host, out, &fold_route));
    AQG_TRY(aqg_sync(ctx));                            // the kernels read the handle's and the pool's buffers
    ctx->wj_routes = routes | fold_route; ctx->wj_groups = ord.G; ctx->wj_passes = ord.passes;
    return AQG_OK;
}

} // namespace

extern "C" {

int aqg_join_window_bounds(aqg_ctx* ctx, int flags, int nkeys, const int* key_dtypes, const void* const* build_keys, const void* build_on, uint32_t nb,
                           const void* const* probe_keys, const void* probe_on, uint32_t np, int on_dtype, double before, double after,
                           uint32_t* order_out, uint32_t* lo_out, uint32_t* hi_out) {
    if (!ctx) return AQG_ERR_ARG;
    wj_clear(ctx);
    WjSides s;
    AQG_TRY(check_wj_sides(ctx, flags, nkeys, key_dtypes, build_keys, build_on, nb, probe_keys, probe_on, np, on_dtype, before, after, &s));
    if ((!order_out && nb) || ((!lo_out || !hi_out) && np)) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_window_bounds: null output");
    const size_t ob = (size_t)nb * 4, pb = (size_t)np * 4;
    if (over_sides(s, order_out, ob) || over_sides(s, lo_out, pb) || over_sides(s, hi_out, pb) || overlaps(order_out, ob, lo_out, pb) ||
        overlaps(order_out, ob, hi_out, pb) || overlaps(lo_out, pb, hi_out, pb))
        return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_window_bounds: an output overlaps an input column or another output");
    if (np == 0) return AQG_OK;
    if (nb == 0) {
        AQG_HIP(ctx, hipMemsetAsync(lo_out, 0, pb, ctx->stream));
        AQG_HIP(ctx, hipMemsetAsync(hi_out, 0, pb, ctx->stream));
        return aqg_sync(ctx);
    }
    if (on_width(s.kind) == 8) return bounds_call<uint64_t>(ctx, s, order_out, lo_out, hi_out);
    return bounds_call<uint32_t>(ctx, s, order_out, lo_out, hi_out);
}

int aqg_interval_fold(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, const uint32_t* lo, const uint32_t* hi, uint32_t m,
                      const void* fill_host, void* out) {
    if (!ctx) return AQG_ERR_ARG;
    wj_clear(ctx);
    AQG_TRY(check_fold(ctx, "aqg_interval_fold", op, t, x, n));
    AQG_CHECK_ROWS(ctx, n, "aqg_interval_fold");
    AQG_CHECK_ROWS(ctx, m, "aqg_interval_fold");
    if ((!lo || !hi || !out) && m) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_interval_fold: null column");
    const size_t ob = (size_t)m * dt_size(out_dtype(op, t)), qb = (size_t)m * 4;
    if ((op != AQG_RANGEW_COUNT && overlaps(out, ob, x, (size_t)n * dt_size(t))) || overlaps(out, ob, lo, qb) || overlaps(out, ob, hi, qb))
        return aqg_fail(ctx, AQG_ERR_ARG, "aqg_interval_fold: out overlaps an input");
    if (m == 0) return AQG_OK;
    uint32_t route = 0;
    AQG_TRY(fold_run(ctx, op, t, x, n, lo, hi, m, fill_host, out, &route));
    ctx->wj_routes = route;
    return AQG_OK;
}

int aqg_join_window(aqg_ctx* ctx, int op, int flags, int nkeys, const int* key_dtypes, const void* const* build_keys, const void* build_on, uint32_t nb,
                    const void* const* probe_keys, const void* probe_on, uint32_t np, int on_dtype, double before, double after, int t,
                    const void* build_x, const void* fill_host, void* out) {
    if (!ctx) return AQG_ERR_ARG;
    wj_clear(ctx);
    WjSides s;
    AQG_TRY(check_fold(ctx, "aqg_join_window", op, t, build_x, nb));
    AQG_TRY(check_wj_sides(ctx, flags, nkeys, key_dtypes, build_keys, build_on, nb, probe_keys, probe_on, np, on_dtype, before, after, &s));
    if (!out && np) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_window: null output");
    const int odt = out_dtype(op, t);
    const size_t ob = (size_t)np * dt_size(odt);
    if (over_sides(s, out, ob) || (op != AQG_RANGEW_COUNT && overlaps(out, ob, build_x, (size_t)nb * dt_size(t))))
        return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_window: the output overlaps an input column");
    if (np == 0) return AQG_OK;
    if (nb == 0) {
        AQG_TRY(write_empty(ctx, odt, empty_value(op, odt, fill_host), np, out));
        return aqg_sync(ctx);
    }
    if (on_width(s.kind) == 8) return window_call<uint64_t>(ctx, s, op, t, build_x, fill_host, out);
    return window_call<uint32_t>(ctx, s, op, t, build_x, fill_host, out);
}

int aqg_join_window_last(aqg_ctx* ctx, uint32_t* routes, uint32_t* build_groups, uint32_t* sort_passes) {
    if (!ctx || !routes || !build_groups || !sort_passes) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_window_last: bad argument");
    *routes = ctx->wj_routes;
    *build_groups = ctx->wj_groups;
    *sort_passes = ctx->wj_passes;
    return AQG_OK;
}

} // extern "C"
