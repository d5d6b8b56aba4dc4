// join_keys.hpp -- the ONE encoding of a join key tuple, shared by the kernels of join_keys.hip and the host (aqg_join_tuple_slots).
// A tuple of typed key columns becomes up to eight 64-bit words, one per NORMALISED column; equality of the words is the group-by's
// equality of the tuples (groupby_keys.hip) with one difference: a NaN equals nothing, so it is reported beside the word instead of
// being made a value.  Unlike aqg_normalize_keys nothing here looks at a column's contents: both sides of a join encode alike.
//   integers, BOOL, DATE    the element's bytes, zero-extended (one dtype list serves both sides: no sign extension is needed)
//   FLOAT / DOUBLE          the bit pattern with -0.0 -> +0.0 ALWAYS; any NaN sets `nan`
//   TIME                    the 7 field bytes (the padding byte masked off)
//   TIMESTAMP               two words: date (4 bytes), time (7 bytes)
//   INT128 / UINT128        two words: low, high
// PACKED: the widths of the words sum to at most 8 bytes -- they are shifted into one word, and that word is the tuple.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/aqg.h"

constexpr int JK_MAXW = 8;
enum JKind : int { JK_U8, JK_U16, JK_U32, JK_U64, JK_F32, JK_F64, JK_TIME, JK_TS_DATE, JK_TS_TIME, JK_128_LO, JK_128_HI };

struct JKCols {
    int nw;                        // normalised columns (words of a WIDE tuple)
    int packed;                    // the words fit one 64-bit word
    int kind[JK_MAXW];
    int shift[JK_MAXW];            // PACKED: bit position of word c
    const void* col[JK_MAXW];      // the caller's column the word is read from
};

__host__ __device__ inline int jk_width(int kind) {
    switch (kind) { case JK_U8: return 1; case JK_U16: return 2; case JK_U32: case JK_F32: case JK_TS_DATE: return 4; default: return 8; }
}

// host: the normalised columns of a dtype list.  AQG_ERR_DTYPE before AQG_ERR_ARG: a string key is a dtype error whatever else is wrong.
inline int jk_plan(int nkeys, const int* dts, const void* const* cols, JKCols* out) {
    memset(out, 0, sizeof *out);
    int total = 0;
    for (int k = 0; k < nkeys; ++k) {
        switch (dts[k]) {
        case AQG_INT8: case AQG_UINT8: case AQG_BOOL: case AQG_INT16: case AQG_UINT16: case AQG_INT32: case AQG_UINT32: case AQG_DATE: case AQG_FLOAT:
        case AQG_INT64: case AQG_UINT64: case AQG_DOUBLE: case AQG_TIME: total += 1; break;
        case AQG_TIMESTAMP: case AQG_INT128: case AQG_UINT128: total += 2; break;
        default: return AQG_ERR_DTYPE;
        }
    }
    if (total > JK_MAXW) return AQG_ERR_ARG;
    int m = 0;
    auto push = [&](int kind, const void* c) { out->kind[m] = kind; out->col[m] = c; ++m; };
    for (int k = 0; k < nkeys; ++k) {
        const void* c = cols ? cols[k] : nullptr;
        switch (dts[k]) {
        case AQG_INT8: case AQG_UINT8: case AQG_BOOL: push(JK_U8, c); break;
        case AQG_INT16: case AQG_UINT16: push(JK_U16, c); break;
        case AQG_INT32: case AQG_UINT32: case AQG_DATE: push(JK_U32, c); break;
        case AQG_INT64: case AQG_UINT64: push(JK_U64, c); break;
        case AQG_FLOAT: push(JK_F32, c); break;
        case AQG_DOUBLE: push(JK_F64, c); break;
        case AQG_TIME: push(JK_TIME, c); break;
        case AQG_TIMESTAMP: push(JK_TS_DATE, c); push(JK_TS_TIME, c); break;
        default: push(JK_128_LO, c); push(JK_128_HI, c); break;
        }
    }
    out->nw = m;
    int bytes = 0;
    for (int c = 0; c < m; ++c) { out->shift[c] = (bytes & 7) * 8; bytes += jk_width(out->kind[c]); }
    out->packed = bytes <= 8;
    return AQG_OK;
}

constexpr uint64_t JK_TIME_MASK = 0x00FFFFFFFFFFFFFFull;

// element i of a column of T: host columns (numpy views of byte arrays) need not be aligned
template <class T> __host__ __device__ inline T jk_ld(const void* col, size_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<const T*>(col)[i];
#else
    T v;
    memcpy(&v, static_cast<const char*>(col) + i * sizeof(T), sizeof(T));
    return v;
#endif
}
__host__ __device__ inline uint64_t jk_f32(uint32_t b, bool& nan) { nan |= (b & 0x7FFFFFFFu) > 0x7F800000u; return b == 0x80000000u ? 0u : b; }
__host__ __device__ inline uint64_t jk_f64(uint64_t b, bool& nan) { nan |= (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; return b == 0x8000000000000000ull ? 0ull : b; }

// word `kind` of row i; nan |= the word is a NaN
__host__ __device__ inline uint64_t jk_word(int kind, const void* col, size_t i, bool& nan) {
    switch (kind) {
    case JK_U8: return jk_ld<uint8_t>(col, i);
    case JK_U16: return jk_ld<uint16_t>(col, i);
    case JK_U32: return jk_ld<uint32_t>(col, i);
    case JK_U64: return jk_ld<uint64_t>(col, i);
    case JK_F32: return jk_f32(jk_ld<uint32_t>(col, i), nan);
    case JK_F64: return jk_f64(jk_ld<uint64_t>(col, i), nan);
    case JK_TIME: return jk_ld<uint64_t>(col, i) & JK_TIME_MASK;
    case JK_TS_DATE: return jk_ld<uint32_t>(col, 3 * i);
    case JK_TS_TIME: return ((uint64_t)jk_ld<uint32_t>(col, 3 * i + 1) | ((uint64_t)jk_ld<uint32_t>(col, 3 * i + 2) << 32)) & JK_TIME_MASK;
    case JK_128_LO: return jk_ld<uint64_t>(col, 2 * i);
    default: return jk_ld<uint64_t>(col, 2 * i + 1);
    }
}

// The hash of a tuple: 32-bit multiplies only (the probe loop is bound by VALU issue).  All 32 bits are the slot's tag; the slot of a
// table of 2^bits slots is the TOP bits (the well-mixed ones of a product).
__host__ __device__ inline uint32_t jk_hash_step(uint32_t h, uint64_t w) {
    h = (h ^ (uint32_t)w) * 0x9E3779B1u;
    return (h ^ (uint32_t)(w >> 32)) * 0x85EBCA6Bu;
}
__host__ __device__ inline uint32_t jk_hash_end(uint32_t h) { return (h ^ (h >> 15)) * 0xC2B2AE35u; }
constexpr uint32_t JK_HASH_SEED = 0x27D4EB2Fu;
__host__ __device__ inline uint32_t jk_slot(uint32_t h, uint32_t bits) { return h >> (32 - bits); }

// the words of row i (w[0] alone when packed) and its hash; returns false for a row holding a NaN
__host__ __device__ inline bool jk_row(const JKCols& kc, size_t i, uint64_t (&w)[JK_MAXW], uint32_t* hash) {
    bool nan = false;
    uint64_t pk = 0;
    uint32_t h = JK_HASH_SEED;
#pragma unroll
    for (int c = 0; c < JK_MAXW; ++c) {
        if (c < kc.nw) {
            const uint64_t v = jk_word(kc.kind[c], kc.col[c], i, nan);
            if (kc.packed) pk |= v << kc.shift[c]; else { w[c] = v; h = jk_hash_step(h, v); }
        }
    }
    if (kc.packed) { w[0] = pk; h = jk_hash_step(h, pk); }
    *hash = jk_hash_end(h);
    return !nan;
}
