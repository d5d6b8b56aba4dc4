// key_image.hpp -- order-preserving unsigned key images and the LDS digit histogram, shared by sort.hip and select.hip.
//
// A value's IMAGE is an unsigned integer of its own width whose unsigned order is the value order of aqg_sort_rows under
// AQG_ORDER_ASC: sign flip for signed integers; for floating values -0.0 -> +0.0 and every NaN -> one quiet NaN first, then the
// sign-dependent flip, so that -inf < ... < 0 < ... < +inf < NaN.
#pragma once
#include "../../include/aqg.h"
#include "dev_common.hpp"

// ---- images of values already in registers (U: the unsigned type of the value's width) ------------------------------------------
template <class U, bool SIGNED> __device__ inline U img_int(U r) {
    if constexpr (SIGNED) r = (U)(r ^ (U(1) << (sizeof(U) * 8 - 1)));
    return r;
}
template <class B> __device__ inline B img_fp(B b) {
    constexpr B sign = B(1) << (sizeof(B) * 8 - 1), expo = sizeof(B) == 4 ? (B)0x7f800000u : (B)0x7ff0000000000000ull;
    constexpr B qnan = sizeof(B) == 4 ? (B)0x7fc00000u : (B)0x7ff8000000000000ull;
    if ((b & ~sign) == 0) b = 0;                       // -0.0 == +0.0
    else if ((b & ~sign) > expo) b = qnan;             // every NaN is one key, after +inf
    return (b & sign) ? (B)~b : (B)(b | sign);
}
// the two images that more than one bit pattern maps to: a value with such an image cannot be rebuilt from it
template <class B> __device__ constexpr B img_fp_zero() { return B(1) << (sizeof(B) * 8 - 1); }
template <class B> __device__ constexpr B img_fp_nan() { return (B)((sizeof(B) == 4 ? (B)0x7fc00000u : (B)0x7ff8000000000000ull) | (B(1) << (sizeof(B) * 8 - 1))); }
// the value of an image (floating: any image but the two above)
template <class U, bool SIGNED> __device__ inline U unimg_int(U r) { return img_int<U, SIGNED>(r); }
template <class B> __device__ inline B unimg_fp(B i) {
    constexpr B sign = B(1) << (sizeof(B) * 8 - 1);
    return (i & sign) ? (B)(i & ~sign) : (B)~i;
}

// ---- images of column elements under a sort order (AQG_ORDER_ASC / DESC / NEG) ----------------------------------------------------
template <class U, bool SIGNED> __device__ inline uint64_t enc_int(const void* p, uint32_t row, int ord) {
    U r = static_cast<const U*>(p)[row];
    if (ord == AQG_ORDER_NEG) r = (U)(U(0) - r);
    r = img_int<U, SIGNED>(r);
    if (ord == AQG_ORDER_DESC) r = (U)~r;
    return (uint64_t)r;
}
template <class U, class B> __device__ inline uint64_t enc_fp(const void* p, uint32_t row, int ord) {
    B b = img_fp<B>(static_cast<const B*>(p)[row]);
    if (ord == AQG_ORDER_DESC) b = (B)~b;
    return (uint64_t)b;
}

// LDS histogram add of one digit per lane: a wavefront whose live lanes share the digit adds once (constant and near-constant
// digit positions would otherwise serialise 64 lanes on one bank)
__device__ inline void hist_add(uint32_t* h, uint32_t d, bool live) {
    const uint64_t act = __ballot(live);
    const uint32_t first = __shfl(d, act ? __ffsll((long long)act) - 1 : 0, 64);
    const uint64_t same = __ballot(live && d == first);
    if (same == act) {
        if (act && lane_id() == __ffsll((long long)act) - 1) atomicAdd(&h[first], (uint32_t)__popcll(act));
    } else if (live) {
        atomicAdd(&h[d], 1u);
    }
}
