// asof.hip -- the as-of join: for every probe row the nearest earlier (BACKWARD) or later (FORWARD) build row of the same key tuple,
// "nearest" by one ordered column `on` (include/aqg.h: aqg_join_asof; the contract restated executably: tests/asof_model.py).
//
//   group    the build side is grouped on its key tuples (JoinBuild::setup) and the probe side is sent through the tuple probe of
//            join_keys.hip into gid[np] = {group id | NONE}.  No key columns: one group, no probe.
//   order    srt[nb] = the build rows by (group id, on, row): aqg_sort_rows over {reversemap, on}, stable.  A build side whose `on`
//            is already non-decreasing (asof_sorted_kernel: the normal state of a tick table) sorts by the group id alone, and not
//            at all without key columns.  img[nb] = the order-preserving unsigned image of `on` in that order (key_image.hpp: both
//            zeros one image, NaN above +inf, so a group's NaN rows are the tail of its segment).
//   search   asof_probe_kernel: four consecutive probe rows per lane, one binary search each over img[off[g] .. off[g+1]), the four
//            advancing in lock step; the trip count is the wavefront's longest segment, every step predicated per lane.
//            LDS: img, srt and the offsets copied into LDS first (small build sides under large probe sides); HBM: read in place.
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "join_tail.hpp"
#include "key_image.hpp"

namespace {

constexpr int AR = 4;                                  // consecutive probe rows per lane

enum OnKind : int { ON_U8, ON_I8, ON_U16, ON_I16, ON_U32, ON_I32, ON_F32, ON_U64, ON_I64, ON_F64 };
int on_kind(int dt) {
    switch (dt) {
    case AQG_UINT8: return ON_U8;   case AQG_INT8: return ON_I8;   case AQG_UINT16: return ON_U16; case AQG_INT16: return ON_I16;
    case AQG_UINT32: return ON_U32; case AQG_INT32: return ON_I32; case AQG_FLOAT: return ON_F32;
    case AQG_UINT64: return ON_U64; case AQG_INT64: return ON_I64; case AQG_DOUBLE: return ON_F64;
    }
    return -1;
}
__host__ __device__ inline int on_width(int kind) { return kind <= ON_I8 ? 1 : kind <= ON_I16 ? 2 : kind <= ON_F32 ? 4 : 8; }

// element i of the column, its bytes zero-extended
__device__ inline uint64_t on_raw(int kind, const void* col, size_t i) {
    switch (on_width(kind)) {
    case 1: return static_cast<const uint8_t*>(col)[i];
    case 2: return static_cast<const uint16_t*>(col)[i];
    case 4: return static_cast<const uint32_t*>(col)[i];
    default: return static_cast<const uint64_t*>(col)[i];
    }
}
// the image of an element: U = uint32_t for elements of up to 4 bytes (narrow integers widened first), uint64_t for 8-byte ones
template <class U> __device__ inline U on_img(int kind, uint64_t raw) {
    if constexpr (sizeof(U) == 4) {
        switch (kind) {
        case ON_I8: return img_int<uint32_t, true>((uint32_t)(int32_t)(int8_t)raw);
        case ON_I16: return img_int<uint32_t, true>((uint32_t)(int32_t)(int16_t)raw);
        case ON_I32: return img_int<uint32_t, true>((uint32_t)raw);
        case ON_F32: return img_fp<uint32_t>((uint32_t)raw);
        default: return (uint32_t)raw;
        }
    } else {
        switch (kind) {
        case ON_I64: return img_int<uint64_t, true>(raw);
        case ON_F64: return img_fp<uint64_t>(raw);
        default: return raw;
        }
    }
}
// four consecutive elements (rows 4*chunk ..) of a 16-byte aligned column: vector loads
__device__ inline void on_load4(int kind, const void* col, uint32_t chunk, uint64_t (&v)[AR]) {
    const size_t r0 = (size_t)chunk * AR;
    switch (on_width(kind)) {
    case 1: { const pack<uint8_t, 4> a = *reinterpret_cast<const pack<uint8_t, 4>*>(static_cast<const uint8_t*>(col) + r0);
#pragma unroll
        for (int q = 0; q < AR; ++q) v[q] = a.v[q]; } break;
    case 2: { const pack<uint16_t, 4> a = *reinterpret_cast<const pack<uint16_t, 4>*>(static_cast<const uint16_t*>(col) + r0);
#pragma unroll
        for (int q = 0; q < AR; ++q) v[q] = a.v[q]; } break;
    case 4: { const pack<uint32_t, 4> a = *reinterpret_cast<const pack<uint32_t, 4>*>(static_cast<const uint32_t*>(col) + r0);
#pragma unroll
        for (int q = 0; q < AR; ++q) v[q] = a.v[q]; } break;
    default: {
        const pack<uint64_t, 2> a = *reinterpret_cast<const pack<uint64_t, 2>*>(static_cast<const uint64_t*>(col) + r0);
        const pack<uint64_t, 2> b = *reinterpret_cast<const pack<uint64_t, 2>*>(static_cast<const uint64_t*>(col) + r0 + 2);
        v[0] = a.v[0]; v[1] = a.v[1]; v[2] = b.v[0]; v[3] = b.v[1]; } break;
    }
}

// *unsorted = 1 unless the column is non-decreasing in image order (NaN is the largest image: NaNs, if any, only at the end)
template <class U>
__global__ void __launch_bounds__(256) asof_sorted_kernel(int kind, const void* __restrict__ on, uint32_t nb, uint32_t* __restrict__ unsorted) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i + 1 < nb; i += gridDim.x * blockDim.x)
        bad |= on_img<U>(kind, on_raw(kind, on, i)) > on_img<U>(kind, on_raw(kind, on, (size_t)i + 1));
    if (bad) *unsorted = 1u;
}

// img[j] = the image of on[srt[j]] (srt == nullptr: the column is in order as it stands)
template <class U>
__global__ void __launch_bounds__(256) asof_image_kernel(int kind, const void* __restrict__ on, const uint32_t* __restrict__ srt, uint32_t nb, U* __restrict__ img) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nb; j += gridDim.x * blockDim.x)
        img[j] = on_img<U>(kind, on_raw(kind, on, srt ? srt[j] : j));
}

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

// a device buffer from the context's pool, given back when the call ends (the workspace is reset by the steps in between)
struct PoolBuf {
    aqg_ctx* ctx;
    void* p = nullptr;
    size_t cap = 0;
    explicit PoolBuf(aqg_ctx* c) : ctx(c) {}
    PoolBuf(const PoolBuf&) = delete;
    PoolBuf& operator=(const PoolBuf&) = delete;
    ~PoolBuf() { aqg_pool_give(ctx, p, cap); }
    int get(size_t bytes) {
        hipError_t e = hipSuccess;
        p = aqg_pool_alloc(ctx, bytes < 256 ? 256 : bytes, &cap, &e);
        if (!p) { ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e); return AQG_ERR_NOMEM; }
        return AQG_OK;
    }
};

bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes) {
    if (!a || !b || !abytes || !bbytes) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}

template <class U>
int asof_run(aqg_ctx* ctx, int forward, int strict, int nkeys, const int* dts, const void* const* bk, const void* build_on, uint32_t nb,
             const void* const* pk, const void* probe_on, uint32_t np, int kind, int on_dtype, uint32_t* out) {
    uint32_t routes = nkeys ? 0u : (uint32_t)AQG_ASOF_ROUTE_NOKEYS;
    // 1. is the build side in time order already?
    uint32_t* flag = nullptr;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_get(ctx, 1, &flag));
    AQG_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
    hipLaunchKernelGGL((asof_sorted_kernel<U>), dim3(aqg_grid(ctx, nb, 256, 4, 8)), dim3(256), 0, ctx->stream, kind, build_on, nb, flag);
    AQG_TRY(aqg_check_launch(ctx, "asof_sorted_kernel"));
    uint32_t unsorted = 0;
    AQG_TRY(aqg_d2h(ctx, &unsorted, flag, 4));
    if (!unsorted) routes |= AQG_ASOF_ROUTE_PRESORTED;
    // 2. group the build side
    JoinBuild build(ctx);
    const uint32_t *off = nullptr, *rmap = nullptr;
    uint32_t G = 1;
    if (nkeys) {
        AQG_TRY(build.setup(nkeys, dts, bk, nb, false));
        G = build.G;
        rmap = aqg_groupby_reversemap(build.gb);
        off = aqg_groupby_offsets(build.gb);
        if (!rmap || !off) return aqg_fail(ctx, AQG_ERR_HIP, "aqg_join_asof: the build side's group offsets");
    }
    // 3. the build rows by (group, on, row), and the images of `on` in that order
    PoolBuf srt(ctx), img(ctx);
    AQG_TRY(img.get((size_t)nb * sizeof(U)));
    uint32_t passes = 0;
    if (nkeys || unsorted) {
        AQG_TRY(srt.get((size_t)nb * 4));
        const int sdt[2] = {AQG_UINT32, on_dtype}, sord[2] = {AQG_ORDER_ASC, AQG_ORDER_ASC};
        const void* scol[2] = {rmap, build_on};
        const int first = nkeys ? 0 : 1, count = (nkeys ? 1 : 0) + (unsorted ? 1 : 0);
        AQG_TRY(aqg_sort_rows(ctx, count, sdt + first, scol + first, sord + first, nb, nullptr, nb, static_cast<uint32_t*>(srt.p)));
        AQG_TRY(aqg_sort_last_passes(ctx, &passes));
    }
    hipLaunchKernelGGL((asof_image_kernel<U>), dim3(aqg_grid(ctx, nb, 256, 4, 8)), dim3(256), 0, ctx->stream, kind, build_on,
                       static_cast<const uint32_t*>(srt.p), nb, static_cast<U*>(img.p));
    AQG_TRY(aqg_check_launch(ctx, "asof_image_kernel"));
    // 4. the groups of the probe rows
    uint32_t* gid = nullptr;
    AQG_TRY(aqg_ws_reset(ctx));
    if (nkeys) {
        AQG_TRY(aqg_ws_ensure(ctx, aqg_jk_table_bytes(nkeys, dts, G) + (size_t)np * 4 + 512));
        AQG_TRY(aqg_ws_get(ctx, (size_t)np, &gid));
        AQG_TRY(aqg_jk_probe_gid(ctx, nkeys, dts, bk, pk, np, build.gb, gid));
    }
    // 5. the search
    AsofArgs a{};
    a.gid = gid; a.probe_on = probe_on; a.np = np;
    a.img = img.p; a.srt = static_cast<const uint32_t*>(srt.p); a.off = off; a.nb = nb; a.G = G;
    a.kind = kind; a.fp = kind == ON_F32 || kind == ON_F64; a.forward = forward; a.upper = forward ? strict : !strict;
    a.aligned = ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(probe_on) | reinterpret_cast<uintptr_t>(gid)) & 15) == 0;
    a.out = out;
    const size_t lds = (size_t)nb * sizeof(U) + (size_t)nb * 4 + ((size_t)G + 1) * 4;
    const bool use_lds = join_lds_route(lds, np);
    routes |= use_lds ? AQG_ASOF_ROUTE_LDS : AQG_ASOF_ROUTE_HBM;
    const unsigned grid = aqg_grid(ctx, np / AR + 1, 256, 2, use_lds ? (lds <= 20 * 1024 ? 8 : 3) : 8);
    aqg_kernel_timer_begin(ctx);
    if (use_lds) hipLaunchKernelGGL((asof_probe_kernel<U, true>), dim3(grid), dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL((asof_probe_kernel<U, false>), dim3(grid), dim3(256), 0, ctx->stream, a);
    aqg_kernel_timer_end(ctx);
    AQG_TRY(aqg_check_launch(ctx, "asof_probe_kernel"));
    ctx->asof_routes = routes;
    ctx->asof_groups = G;
    ctx->asof_passes = passes;
    return aqg_sync(ctx);                              // the kernels read the handle's and the pool's buffers
}

} // namespace

extern "C" {

int aqg_join_asof(aqg_ctx* ctx, int direction, int flags, int nkeys, const int* key_dtypes, const void* const* build_keys, const void* build_on,
                  uint32_t nb, const void* const* probe_keys, const void* probe_on, uint32_t np, int on_dtype, uint32_t* out) {
    if (!ctx) return AQG_ERR_ARG;
    ctx->asof_routes = ctx->asof_groups = ctx->asof_passes = 0;
    if (nkeys < 0 || nkeys > 8) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_asof: bad argument (0..8 key columns)");
    if (nkeys) AQG_TRY(aqg_jk_check(ctx, nkeys, key_dtypes, build_keys, nb, probe_keys, np));
    const int kind = on_kind(on_dtype);
    if (kind < 0) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_join_asof: the `on` column is INT8/16/32/64, UINT8/16/32/64, FLOAT or DOUBLE");
    AQG_CHECK_ROWS(ctx, nb, "aqg_join_asof");
    AQG_CHECK_ROWS(ctx, np, "aqg_join_asof");
    if ((direction != AQG_ASOF_BACKWARD && direction != AQG_ASOF_FORWARD) || (flags & ~AQG_ASOF_STRICT))
        return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_asof: bad direction or flags");
    if ((!build_on && nb) || (!probe_on && np) || (!out && np)) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_asof: null column");
    const size_t ob = (size_t)np * 4, w = (size_t)on_width(kind);
    bool ov = overlaps(out, ob, build_on, nb * w) || overlaps(out, ob, probe_on, np * w);
    for (int k = 0; k < nkeys; ++k) {
        const size_t kw = aqg_dtype_size(key_dtypes[k]);
        ov = ov || overlaps(out, ob, build_keys[k], nb * kw) || overlaps(out, ob, probe_keys[k], np * kw);
    }
    if (ov) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_asof: the output overlaps an input column");
    if (np == 0) return AQG_OK;
    if (nb == 0) { AQG_HIP(ctx, hipMemsetAsync(out, 0xFF, ob, ctx->stream)); return aqg_sync(ctx); }
    const int forward = direction == AQG_ASOF_FORWARD, strict = (flags & AQG_ASOF_STRICT) != 0;
    if (w == 8) return asof_run<uint64_t>(ctx, forward, strict, nkeys, key_dtypes, build_keys, build_on, nb, probe_keys, probe_on, np, kind, on_dtype, out);
    return asof_run<uint32_t>(ctx, forward, strict, nkeys, key_dtypes, build_keys, build_on, nb, probe_keys, probe_on, np, kind, on_dtype, out);
}

int aqg_join_asof_last(aqg_ctx* ctx, uint32_t* routes, uint32_t* build_groups, uint32_t* sort_passes) {
    if (!ctx || !routes || !build_groups || !sort_passes) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_asof_last: bad argument");
    *routes = ctx->asof_routes;
    *build_groups = ctx->asof_groups;
    *sort_passes = ctx->asof_passes;
    return AQG_OK;
}

} // extern "C"
