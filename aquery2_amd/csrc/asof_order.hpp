// asof_order.hpp -- what the as-of join (asof.hip) and the window join (join_window.hip) share: the ordering step (the `on` column's
// order-preserving images, the build side by (group, on, row), the groups of the probe rows) and the entry checks of the two sides.
//
//   group    the build side is grouped on its key tuples (JoinBuild::setup) and the probe side is sent through the tuple probe of
//            join_keys.hip into gid[np] = {group id | NONE}.  No key columns: one group, no probe.
//   order    srt[nb] = the build rows by (group id, on, row): aqg_sort_rows over {reversemap, on}, stable.  A build side whose `on`
//            is already non-decreasing (asof_sorted_kernel: the normal state of a tick table) sorts by the group id alone, and not
//            at all without key columns.  img[nb] = the order-preserving unsigned image of `on` in that order (key_image.hpp: both
//            zeros one image, NaN above +inf, so a group's NaN rows are the tail of its segment).
// Everything here sits in an unnamed namespace: each of the two files compiles its own copy of the two small kernels.
#pragma once
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

// ---- the entry checks of both joins -----------------------------------------------------------------------------------------------------
struct JoinSides {
    int nkeys; const int* dts; const void* const* bk; const void* build_on; uint32_t nb;
    const void* const* pk; const void* probe_on; uint32_t np; int kind, on_dtype, flags;
};
// The checks of the two sides that the as-of and the window joins share, in the order both have always refused in; `who`: the public
// entry, `mask`: the flag bits it knows.  s->kind: the OnKind of the `on` column.  (What follows in the callers -- the direction, the
// spans, the outputs -- refuses with AQG_ERR_ARG like the last two checks here.)
int check_sides(aqg_ctx* ctx, const char* who, int flags, int mask, int nkeys, const int* dts, const void* const* bk, const void* build_on, uint32_t nb,
                const void* const* pk, const void* probe_on, uint32_t np, int on_dtype, JoinSides* s) {
    const std::string w(who);
    if (nkeys < 0 || nkeys > 8) return aqg_fail(ctx, AQG_ERR_ARG, (w + ": bad argument (0..8 key columns)").c_str());
    if (nkeys) AQG_TRY(aqg_jk_check(ctx, nkeys, dts, bk, nb, pk, np));
    const int kind = on_kind(on_dtype);
    if (kind < 0) return aqg_fail(ctx, AQG_ERR_DTYPE, (w + ": the `on` column is INT8/16/32/64, UINT8/16/32/64, FLOAT or DOUBLE").c_str());
    if ((uint64_t)nb > (uint64_t)AQG_MAX_ROWS || (uint64_t)np > (uint64_t)AQG_MAX_ROWS) return aqg_fail(ctx, AQG_ERR_ARG, (w + ": more than AQG_MAX_ROWS rows").c_str());
    if (flags & ~mask) return aqg_fail(ctx, AQG_ERR_ARG, (w + ": unknown flag bits").c_str());
    if ((!build_on && nb) || (!probe_on && np)) return aqg_fail(ctx, AQG_ERR_ARG, (w + ": null column").c_str());
    *s = JoinSides{nkeys, dts, bk, build_on, nb, pk, probe_on, np, kind, on_dtype, flags};
    return AQG_OK;
}
// does the output [out, out + bytes) lie over a column of either side?
bool over_sides(const JoinSides& s, const void* out, size_t bytes) {
    const size_t w = (size_t)on_width(s.kind);
    bool ov = overlaps(out, bytes, s.build_on, s.nb * w) || overlaps(out, bytes, s.probe_on, s.np * w);
    for (int k = 0; k < s.nkeys; ++k) {
        const size_t kw = aqg_dtype_size(s.dts[k]);
        ov = ov || overlaps(out, bytes, s.bk[k], s.nb * kw) || overlaps(out, bytes, s.pk[k], s.np * kw);
    }
    return ov;
}

// The ordered build side of one call and the groups of its probe rows.  The object owns the build handle and the pool buffers: it
// lives until the stream has drained behind the kernels that read them.  After run():
//   img   [nb] images in (group, on, row) order          srt   [nb] build rows in that order; nullptr: the identity
//   off   [G + 1] segment offsets; nullptr: one segment  gid   [np] groups of the probe rows (workspace); nullptr: no key columns
// The workspace is left reset and holding only the probe's table and gid, sized for them plus `ws_extra` bytes of the caller's.
template <class U> struct AsofOrder {
    JoinBuild build;
    PoolBuf srt_buf, img_buf;
    const U* img = nullptr;
    const uint32_t *srt = nullptr, *off = nullptr;
    uint32_t* gid = nullptr;
    uint32_t G = 1, routes = 0, passes = 0;
    explicit AsofOrder(aqg_ctx* c) : build(c), srt_buf(c), img_buf(c) {}

    // srt_out: where the order goes when a sort runs (nullptr: a pool buffer of this object)
    int run(aqg_ctx* ctx, const char* who, int nkeys, const int* dts, const void* const* bk, const void* build_on, uint32_t nb,
            const void* const* pk, uint32_t np, int kind, int on_dtype, uint32_t* srt_out = nullptr, size_t ws_extra = 0) {
        routes = nkeys ? 0u : (uint32_t)AQG_ASOF_ROUTE_NOKEYS;
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
        const uint32_t* rmap = nullptr;
        if (nkeys) {
            AQG_TRY(build.setup(nkeys, dts, bk, nb, false));
            G = build.G;
            rmap = aqg_groupby_reversemap(build.gb);
            off = aqg_groupby_offsets(build.gb);
            if (!rmap || !off) { ctx->err = std::string(who) + ": the build side's group offsets"; return AQG_ERR_HIP; }
        }
        // 3. the build rows by (group, on, row), and the images of `on` in that order
        AQG_TRY(img_buf.get((size_t)nb * sizeof(U)));
        if (nkeys || unsorted) {
            uint32_t* dst = srt_out;
            if (!dst) { AQG_TRY(srt_buf.get((size_t)nb * 4)); dst = static_cast<uint32_t*>(srt_buf.p); }
            const int sdt[2] = {AQG_UINT32, on_dtype}, sord[2] = {AQG_ORDER_ASC, AQG_ORDER_ASC};
            const void* scol[2] = {rmap, build_on};
            const int first = nkeys ? 0 : 1, count = (nkeys ? 1 : 0) + (unsorted ? 1 : 0);
            AQG_TRY(aqg_sort_rows(ctx, count, sdt + first, scol + first, sord + first, nb, nullptr, nb, dst));
            AQG_TRY(aqg_sort_last_passes(ctx, &passes));
            srt = dst;
        }
        hipLaunchKernelGGL((asof_image_kernel<U>), dim3(aqg_grid(ctx, nb, 256, 4, 8)), dim3(256), 0, ctx->stream, kind, build_on, srt, nb,
                           static_cast<U*>(img_buf.p));
        AQG_TRY(aqg_check_launch(ctx, "asof_image_kernel"));
        img = static_cast<const U*>(img_buf.p);
        // 4. the groups of the probe rows
        AQG_TRY(aqg_ws_reset(ctx));
        if (nkeys) {
            AQG_TRY(aqg_ws_ensure(ctx, aqg_jk_table_bytes(nkeys, dts, G) + (size_t)np * 4 + 512 + ws_extra));
            AQG_TRY(aqg_ws_get(ctx, (size_t)np, &gid));
            AQG_TRY(aqg_jk_probe_gid(ctx, nkeys, dts, bk, pk, np, build.gb, gid));
        } else if (ws_extra) {
            AQG_TRY(aqg_ws_ensure(ctx, ws_extra));
        }
        return AQG_OK;
    }
    // bytes of the ordered build side as the as-of search stages it in LDS: images, rows and offsets
    size_t table_bytes(uint32_t nb) const { return (size_t)nb * sizeof(U) + (size_t)nb * 4 + ((size_t)G + 1) * 4; }
};

} // namespace
