// asof.hip -- the as-of join: for every probe row the nearest earlier (BACKWARD) or later (FORWARD) build row of the same key tuple,
// "nearest" by one ordered column `on` (include/aqg.h: aqg_join_asof; the contract restated executably: tests/asof_model.py).
//
//   group, order   asof_order.hpp (shared with the window join, join_window.hip): gid[np] = {group id | NONE}, srt[nb] = the build
//            rows by (group id, on, row), img[nb] = the order-preserving unsigned images of `on` in that order.
//   search   asof_probe_kernel: four consecutive probe rows per lane, one binary search each over img[off[g] .. off[g+1]), the four
//            advancing in lock step; the trip count is the wavefront's longest segment, every step predicated per lane.
//            LDS: img, srt and the offsets copied into LDS first (small build sides under large probe sides); HBM: read in place.
#include "asof_order.hpp"

namespace {

struct AsofArgs {
    const uint32_t* gid;           // [np] group of the probe row or NONE; nullptr: no key columns, every row in group 0
    const void* probe_on;
    uint32_t np;
    const void* img;               // [nb] images in (group, on, row) order
    const uint32_t* srt;           // [nb] build rows in that order; nullptr: the identity
    const uint32_t* off;           // [G + 1] segment offsets; nullptr: one segment [0, nb)
    uint32_t nb, G;
    int kind, fp, forward, upper, aligned;
    uint32_t* out;
};

// The partners of R probe rows per lane.  EVERY lane of the wavefront calls this (rows that do not exist come with live == false): the
// trip count is the wavefront's longest segment, and a lane whose search is over keeps stepping with n == 0, reading element 0.
// Each step issues the R loads of the R searches before any of them is compared.
template <class U, int R>
__device__ inline void asof_search(const AsofArgs& a, const U* img, const uint32_t* srt, const uint32_t* off, const uint32_t (&g)[R], const U (&key)[R],
                                   bool live, uint32_t (&res)[R]) {
    const U nan_img = img_fp_nan<U>();
    uint32_t pos[R], n[R], lo[R], hi[R];
    uint32_t maxn = 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const bool go = live && g[q] != NONE && !(a.fp && key[q] == nan_img);
        const uint32_t gg = go ? g[q] : 0u;
        uint32_t b = 0, e = a.nb;
        if (off) { b = off[gg]; e = off[gg + 1]; }
        lo[q] = go ? b : 0u;
        hi[q] = go ? e : 0u;
        pos[q] = lo[q];
        n[q] = hi[q] - lo[q];
        maxn = n[q] > maxn ? n[q] : maxn;
    }
    maxn = wave_reduce(maxn, OpMax{});
    const int trips = 32 - __clz(maxn);                // a segment of L rows is decided in floor(log2 L) + 1 halvings
    for (int t = 0; t < trips; ++t) {
        U v[R];
        uint32_t mid[R];
#pragma unroll
        for (int q = 0; q < R; ++q) { mid[q] = n[q] ? pos[q] + (n[q] >> 1) : 0u; v[q] = img[mid[q]]; }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const uint32_t half = n[q] >> 1;
            const bool right = n[q] && (a.upper ? v[q] <= key[q] : v[q] < key[q]);      // the bound lies behind mid
            pos[q] = right ? mid[q] + 1 : pos[q];
            n[q] = right ? n[q] - half - 1 : half;
        }
    }
    // pos: the first row of the segment whose image is above (upper) / not below (lower) the key
#pragma unroll
    for (int q = 0; q < R; ++q) {
        bool ok = a.forward ? pos[q] < hi[q] : pos[q] > lo[q];
        const uint32_t p = ok ? (a.forward ? pos[q] : pos[q] - 1) : 0u;
        if (a.fp && a.forward) ok = ok && img[p] != nan_img;       // the NaN tail of a segment is nobody's partner
        res[q] = ok ? (srt ? srt[p] : p) : NONE;
    }
}

template <class U, bool LDS>
__global__ void __launch_bounds__(256) asof_probe_kernel(AsofArgs a) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const U* img = static_cast<const U*>(a.img);
    const uint32_t* srt = a.srt;
    const uint32_t* off = a.off;
    if constexpr (LDS) {                               // [nb] images, [nb] rows, [G + 1] offsets
        U* li = reinterpret_cast<U*>(smem_raw);
        uint32_t* ls = reinterpret_cast<uint32_t*>(li + a.nb);
        uint32_t* lf = ls + a.nb;
        for (uint32_t j = threadIdx.x; j < a.nb; j += blockDim.x) { li[j] = img[j]; ls[j] = srt ? srt[j] : j; }
        for (uint32_t j = threadIdx.x; j <= a.G; j += blockDim.x) lf[j] = off ? off[j] : (j ? a.nb : 0u);
        __syncthreads();
        img = li; srt = ls; off = lf;
    }
    const uint32_t nchunk = a.aligned ? a.np / AR : 0u;
    uint32_t c_lo, c_hi;
    wg_span(nchunk, c_lo, c_hi);
    for (uint32_t base = c_lo; base < c_hi; base += blockDim.x) {          // (uniform over the workgroup: every lane reaches the search)
        const uint32_t ch = base + threadIdx.x;
        const bool live = ch < c_hi;
        uint32_t g[AR] = {0u, 0u, 0u, 0u}, res[AR];
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
        asof_search<U, AR>(a, img, srt, off, g, key, live, res);
        if (live) {
            pack<uint32_t, 4> o;
#pragma unroll
            for (int q = 0; q < AR; ++q) o.v[q] = res[q];
            *reinterpret_cast<pack<uint32_t, 4>*>(a.out + (size_t)ch * AR) = o;
        }
    }
    // the tail, and every row of columns or outputs off the vector width
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)nchunk * AR + (uint64_t)blockIdx.x * blockDim.x; base < a.np; base += stride) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < a.np;
        uint32_t g[1] = {0u}, res[1];
        U key[1] = {U(0)};
        if (live) {
            if (a.gid) g[0] = a.gid[i];
            key[0] = on_img<U>(a.kind, on_raw(a.kind, a.probe_on, (size_t)i));
        }
        asof_search<U, 1>(a, img, srt, off, g, key, live, res);
        if (live) a.out[i] = res[0];
    }
}

template <class U>
int asof_run(aqg_ctx* ctx, const JoinSides& s, int forward, int strict, uint32_t* out) {
    // 1-4. the ordered build side and the groups of the probe rows
    AsofOrder<U> ord(ctx);
    AQG_TRY(ord.run(ctx, "aqg_join_asof", s.nkeys, s.dts, s.bk, s.build_on, s.nb, s.pk, s.np, s.kind, s.on_dtype));
    uint32_t routes = ord.routes;
    // 5. the search
    AsofArgs a{};
    a.gid = ord.gid; a.probe_on = s.probe_on; a.np = s.np;
    a.img = ord.img; a.srt = ord.srt; a.off = ord.off; a.nb = s.nb; a.G = ord.G;
    a.kind = s.kind; a.fp = s.kind == ON_F32 || s.kind == ON_F64; a.forward = forward; a.upper = forward ? strict : !strict;
    a.aligned = ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(s.probe_on) | reinterpret_cast<uintptr_t>(ord.gid)) & 15) == 0;
    a.out = out;
    const size_t lds = ord.table_bytes(s.nb);
    const bool use_lds = join_lds_route(lds, s.np);
    routes |= use_lds ? AQG_ASOF_ROUTE_LDS : AQG_ASOF_ROUTE_HBM;
    const unsigned grid = join_probe_grid(ctx, s.np, AR, use_lds, lds);
    aqg_kernel_timer_begin(ctx);
    if (use_lds) hipLaunchKernelGGL((asof_probe_kernel<U, true>), dim3(grid), dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL((asof_probe_kernel<U, false>), dim3(grid), dim3(256), 0, ctx->stream, a);
    aqg_kernel_timer_end(ctx);
    AQG_TRY(aqg_check_launch(ctx, "asof_probe_kernel"));
    ctx->asof_routes = routes;
    ctx->asof_groups = ord.G;
    ctx->asof_passes = ord.passes;
    return aqg_sync(ctx);                              // the kernels read the handle's and the pool's buffers
}

} // namespace

extern "C" {

int aqg_join_asof(aqg_ctx* ctx, int direction, int flags, int nkeys, const int* key_dtypes, const void* const* build_keys, const void* build_on,
                  uint32_t nb, const void* const* probe_keys, const void* probe_on, uint32_t np, int on_dtype, uint32_t* out) {
    if (!ctx) return AQG_ERR_ARG;
    ctx->asof_routes = ctx->asof_groups = ctx->asof_passes = 0;
    JoinSides s;
    AQG_TRY(check_sides(ctx, "aqg_join_asof", flags, AQG_ASOF_STRICT, nkeys, key_dtypes, build_keys, build_on, nb, probe_keys, probe_on, np, on_dtype, &s));
    if (direction != AQG_ASOF_BACKWARD && direction != AQG_ASOF_FORWARD) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_asof: bad direction");
    if (!out && np) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_asof: null column");
    const size_t ob = (size_t)np * 4;
    if (over_sides(s, out, ob)) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_asof: the output overlaps an input column");
    if (np == 0) return AQG_OK;
    if (nb == 0) { AQG_HIP(ctx, hipMemsetAsync(out, 0xFF, ob, ctx->stream)); return aqg_sync(ctx); }
    const int forward = direction == AQG_ASOF_FORWARD, strict = (flags & AQG_ASOF_STRICT) != 0;
    if (on_width(s.kind) == 8) return asof_run<uint64_t>(ctx, s, forward, strict, out);
    return asof_run<uint32_t>(ctx, s, forward, strict, out);
}

int aqg_join_asof_last(aqg_ctx* ctx, uint32_t* routes, uint32_t* build_groups, uint32_t* sort_passes) {
    if (!ctx || !routes || !build_groups || !sort_passes) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_asof_last: bad argument");
    *routes = ctx->asof_routes;
    *build_groups = ctx->asof_groups;
    *sort_passes = ctx->asof_passes;
    return AQG_OK;
}

} // extern "C"
