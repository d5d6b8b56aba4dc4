// scan_dev.hpp -- tile vocabulary shared by the scan kernels (scan_prefix.hpp: the prefix pass of scan.hip, segscan.hip and ema.hip;
// scan_window.hpp: the sliding windows of both layouts; scan.hip: the chained kernel): accumulator algebras and the carry of a segmented
// scan, the workgroup exclusive scan, blocked tile loads, the LDS-transposed tile store, the variance
// vocabulary and the scan of the tile aggregates (K2 of the prefix pass).
#pragma once
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "chain_dev.hpp"

// ---- the carry of a segmented scan -------------------------------------------------------------------------------------------
// (in an unnamed namespace, like the kernels of the .hip files that use it: the type names go into the names of the kernels' LDS
// variables, by which the compiler lays them out -- with them inside aqgscan the carry scans of segscan.hip compiled to other code)
namespace {
// v: fold of the values behind the last group start of the range (of the whole range when it has none); s: position + 1 of that
// start (0: none); c: group starts in the range
template <class A> struct SegCarry { A v; uint32_t s; uint32_t c; };
template <class ALG> struct seg_alg {
    using A = SegCarry<typename ALG::A>;
    __device__ static A identity() { A r; r.v = ALG::identity(); r.s = 0; r.c = 0; return r; }
    __device__ static A op(A a, A b) { A r; r.s = b.s ? b.s : a.s; r.c = a.c + b.c; r.v = b.s ? b.v : ALG::op(a.v, b.v); return r; }
};
} // namespace

namespace aqgscan {

constexpr int SB = 256;        // lanes per workgroup
constexpr int IT = 8;          // consecutive elements per lane
constexpr int TS = SB * IT;    // tile
constexpr uint32_t HALO_MAX_BYTES = 96 * 1024;

// ---- accumulator algebra ----------------------------------------------------------------------
// any trivially copyable struct of whole dwords travels word by word
template <class A> __device__ inline A shfl_up_words(A x, int off) {
    static_assert(sizeof(A) % 4 == 0, "carry structs are whole dwords");
    uint32_t w[sizeof(A) / 4];
    __builtin_memcpy(w, &x, sizeof(A));
#pragma unroll
    for (size_t k = 0; k < sizeof(A) / 4; ++k) w[k] = (uint32_t)__shfl_up((int)w[k], off, 64);
    __builtin_memcpy(&x, w, sizeof(A));
    return x;
}
template <class A> __device__ inline A shfl_up_any(A x, int off) {
    if constexpr (std::is_class_v<A> && !std::is_same_v<A, aqg_i128>) return shfl_up_words(x, off);
    else if constexpr (std::is_same_v<A, aqg_i128>) {
        aqg_i128 r;
        r.lo = __shfl_up((unsigned long long)x.lo, off, 64);
        r.hi = __shfl_up((unsigned long long)x.hi, off, 64);
        return r;
    } else return shfl_up_t(x, off);
}
using aqgchain::shfl_xor_any;
template <class A> __device__ inline A shfl_idx_any(A x, int src) {
    if constexpr (std::is_same_v<A, aqg_i128>) {
        aqg_i128 r;
        r.lo = __shfl((unsigned long long)x.lo, src, 64);
        r.hi = __shfl((unsigned long long)x.hi, src, 64);
        return r;
    } else return shfl_idx_t(x, src);
}

// sum accumulator of T: exact integers (64 bits for <=4-byte inputs, 128 for 8-byte), double for fp
template <class T> struct sum_alg {
    using A = std::conditional_t<std::is_floating_point_v<T>, double,
              std::conditional_t<sizeof(T) == 8, aqg_i128, std::conditional_t<std::is_unsigned_v<T>, uint64_t, int64_t>>>;
    __device__ static A identity() { if constexpr (std::is_same_v<A, aqg_i128>) return {0, 0}; else return (A)0; }
    __device__ static A lift(T v) {
        if constexpr (std::is_same_v<A, aqg_i128>) { if constexpr (std::is_unsigned_v<T>) return i128_from_u64(v); else return i128_from_i64(v); }
        else return (A)v;
    }
    __device__ static A op(A a, A b) { if constexpr (std::is_same_v<A, aqg_i128>) return i128_add(a, b); else return a + b; }
    __device__ static A sub(A a, A b) {
        if constexpr (std::is_same_v<A, aqg_i128>) { aqg_i128 nb = {~b.lo + 1, ~b.hi + (b.lo == 0 ? 1ull : 0ull)}; return i128_add(a, nb); }
        else return a - b;
    }
    __device__ static aqg_i128 to_i128(A a) {
        if constexpr (std::is_same_v<A, aqg_i128>) return a;
        else if constexpr (std::is_unsigned_v<A>) return i128_from_u64(a);
        else return i128_from_i64((int64_t)a);
    }
    __device__ static double to_double(A a) {
        if constexpr (std::is_same_v<A, aqg_i128>) {
            if constexpr (std::is_unsigned_v<T>) return u128_to_double(a.hi, a.lo); else return i128_to_double(a);
        } else return (double)a;
    }
};
// Identities are the true ends of the ordering -- +-Inf for floating types, not +-max(): a fold that starts from max() turns a +Inf
// row into max().  The reference's seeds (mins: max(), maxs / max: numeric_limits<T>::min()) are applied where a result is written.
template <class T> struct min_alg {
    using A = T;
    __host__ __device__ static A identity() { if constexpr (std::is_floating_point_v<T>) return (T)INFINITY; else return dlimits<T>::max(); }
    __device__ static A lift(T v) { return v; }
    __device__ static A op(A a, A b) { return b < a ? b : a; }
};
template <class T> struct max_alg {
    using A = T;
    __host__ __device__ static A identity() { if constexpr (std::is_floating_point_v<T>) return -(T)INFINITY; else return dlimits<T>::min(); }
    __device__ static A lift(T v) { return v; }
    __device__ static A op(A a, A b) { return b > a ? b : a; }
};
template <class T, bool IS_MAX> using minmax_alg = std::conditional_t<IS_MAX, max_alg<T>, min_alg<T>>;
// affine maps y -> a y + b of the exponential moving averages (ema.hip): a row lifts to {decay, weight * x} (recursive form) or to
// {decay, x, 1} (adjusted form: numerator and denominator ride the same decay), and op(l, r) is "l, then r".  THE MAPS DO NOT COMMUTE:
// only the ordered parts of the skeleton may fold them -- the lane's serial loop, block_scan_excl, launch_agg_scan, seg_alg -- never
// block_fold or the chained look-back of scan.hip.  A slice's first row lifts to a map with a = 0, which discards what precedes it.
// fma: one rounding per component and combine (the build contracts nothing by itself).
struct ema_rec { double a, b; };
struct ema_adj { double a, num, den; };
template <bool ADJ> struct ema_alg {
    using A = std::conditional_t<ADJ, ema_adj, ema_rec>;
    __device__ static A identity() { if constexpr (ADJ) return {1.0, 0.0, 0.0}; else return {1.0, 0.0}; }
    // decay outside [0, 1] (NaN included) poisons the slice like a NaN row: a NaN factor makes every later combine NaN
    __device__ static A lift(double decay, double weight, double x) {
        if (!(decay >= 0.0 && decay <= 1.0)) decay = weight = __builtin_nan("");
        if constexpr (ADJ) return {decay, decay != decay ? decay : x, 1.0}; else return {decay, weight * x};
    }
    __device__ static A lift_first(double x) { if constexpr (ADJ) return {0.0, x, 1.0}; else return {0.0, x}; }
    __device__ static A op(A l, A r) {
        if constexpr (ADJ) return {l.a * r.a, fma(r.a, l.num, r.num), fma(r.a, l.den, r.den)};
        else return {l.a * r.a, fma(r.a, l.b, r.b)};
    }
    __device__ static double value(A m) { if constexpr (ADJ) return m.num / m.den; else return m.b; }
};

// exclusive scan of one value per lane across the workgroup; `total` = fold of all lanes
template <class ALG, class A> __device__ inline A block_scan_excl(A v, A* lds_w /* >= 5 */, A& total) {
    const int lane = lane_id(), wid = wave_id();
    A incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        A y = shfl_up_any(incl, off);
        if (lane >= off) incl = ALG::op(y, incl);
    }
    if (lane == 63) lds_w[wid] = incl;
    __syncthreads();
    A base = ALG::identity();
    for (int w = 0; w < wid; ++w) base = ALG::op(base, lds_w[w]);
    A tot = ALG::identity();
    for (int w = 0; w < SB / 64; ++w) tot = ALG::op(tot, lds_w[w]);
    total = tot;
    A prev = shfl_up_any(incl, 1);
    if (lane == 0) prev = ALG::identity();
    __syncthreads();
    return ALG::op(base, prev);
}

template <class T> __device__ inline void load_tile_items(const T* __restrict__ x, uint32_t n, uint32_t base, T (&v)[IT], uint32_t& cnt) {
    cnt = base >= n ? 0 : (n - base < (uint32_t)IT ? n - base : IT);
    if (cnt == IT && (((uintptr_t)(x + base)) & (sizeof(T) * IT > 16 ? 15 : sizeof(T) * IT - 1)) == 0) {
        pack<T, IT> p = *reinterpret_cast<const pack<T, IT>*>(x + base);
#pragma unroll
        for (int j = 0; j < IT; ++j) v[j] = p.v[j];
    } else {
#pragma unroll
        for (int j = 0; j < IT; ++j) if ((uint32_t)j < cnt) v[j] = x[base + j];
    }
}

// Blocked results (IT consecutive elements per lane) are written through LDS so that consecutive lanes store consecutive
// elements: a lane-blocked store of 16-byte results touches 64 different 128-B lines per instruction (sums: 2.4 TB/s),
// the transposed one writes whole lines.
template <class O> __device__ inline void store_tile_striped(O* __restrict__ out, uint32_t tile_base, const O (&v)[IT], uint32_t n, O* lds /* TS elements */) {
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < IT; ++j) lds[t * IT + j] = v[j];
    __syncthreads();
    const uint32_t live = tile_base + TS <= n ? TS : n - tile_base;
#pragma unroll
    for (int j = 0; j < IT; ++j) { uint32_t e = j * SB + t; if (e < live) out[tile_base + e] = lds[e]; }
}
// avgs (aggregations.h:219-228) starts its sum with `s = ret[0] = arr[0]`: the first element ROUNDED to double.  An 8-byte integer
// beyond 2^53 does not survive that, and every later row divides the sum that carries the difference.  This is the difference
// (LongType)(double)v - v as a 128-bit value (|difference| <= 2^10), to be added to the exact running sum.
template <class T> __device__ inline aqg_i128 first_row_rounding(T v) {
    static_assert(sizeof(T) == 8 && std::is_integral_v<T>, "narrower integers are exact in a double");
    const double d = (double)v;
    if constexpr (std::is_unsigned_v<T>) {
        if (d >= 18446744073709551616.0) return i128_from_u64(0ull - (uint64_t)v);             // rounded up to 2^64
        return i128_from_i64((int64_t)((uint64_t)d - (uint64_t)v));
    } else {
        if (d >= 9223372036854775808.0) return i128_from_u64(0x8000000000000000ull - (uint64_t)v);   // rounded up to 2^63
        return i128_from_i64((int64_t)((uint64_t)(int64_t)d - (uint64_t)v));
    }
}
struct dpair { double s, q; };

// ---- variance scans (vars / stddevs / varw / stddevw) --------------------------------------------------------------------------
// Variance does not change when a constant is added to the data, but E[x^2] - E[x]^2 from raw sums loses everything to
// cancellation once mean^2 dwarfs the spread (int32 near 2^31: relative errors ~1e-1).  Every variance path here works on
// differences x - K from an anchor K that is itself an element of the data, so the terms are bounded by the range of the values.
// x - K, computed in the column's own arithmetic: exact for integers (two's complement, |x - K| < 2^63) and representable as a
// double while |x - K| < 2^53; for floating columns one rounding at most (none when x and K are within a factor of two)
template <class T> __device__ inline double anchored(T x, T k) {
    if constexpr (std::is_floating_point_v<T>) return (double)x - (double)k;
    else return (double)(int64_t)((uint64_t)x - (uint64_t)k);
}
// moments about an anchor: k = the first element of the range, s = sum (x - k), q = sum (x - k)^2, n = elements.  The combine
// moves b onto a's anchor: sum (x - ka) = s_b + n_b d, sum (x - ka)^2 = q_b + 2 d s_b + n_b d^2 with d = kb - ka (exact for
// integers), whose terms are bounded by n_b (range)^2 as well.  Identity: n = 0.
template <class T> struct mom_alg {
    struct A { T k; uint32_t n; double s, q; };
    __device__ static A identity() { A r; r.k = (T)0; r.n = 0; r.s = 0; r.q = 0; return r; }
    __device__ static A lift(T v) { A r; r.k = v; r.n = 1; r.s = 0; r.q = 0; return r; }
    __device__ static A op(A a, A b) {
        if (!b.n) return a;
        if (!a.n) return b;
        const double d = anchored(b.k, a.k), nb = (double)b.n;
        A r;
        r.k = a.k;
        r.n = a.n + b.n;
        r.s = a.s + (b.s + nb * d);
        r.q = a.q + (b.q + (2.0 * d * b.s + nb * d * d));
        return r;
    }
};
// population variance of n elements from their anchored sums (0 when every difference is 0)
__device__ inline double var_from(double s, double q, double n) {
    const double v = (q - s * s / n) / n;
    return v > 0 ? v : 0.0;
}
constexpr uint32_t VAR_DIRECT_MAX_W = 64;         // longer windows take the anchored prefix difference below
constexpr int VAR_REG_W = 8;                      // windows up to this long keep their differences in registers
// varw / stddevw over one tile of TS positions, windows of up to VAR_DIRECT_MAX_W (len_of(p) = the window's length at p, 1..w):
// the tile and its w - 1 row halo are staged in LDS with coalesced loads, lane t takes positions t, t + SB, ... (conflict-free LDS
// reads, coalesced stores).  Two passes over the window: the mean of the differences from an anchor inside the window, then the
// squared deviations from it -- no cancellation against anything wider than the window.  RW > 0: the window's differences
// (w <= RW) are kept in registers, RW == 0: both passes read LDS.
template <class T, bool SD, int RW, class LEN>
__device__ inline void var_short_tile(const T* __restrict__ x, uint32_t n, uint32_t w, LEN len_of, T* L /* TS + VAR_DIRECT_MAX_W */, double* __restrict__ out) {
    const uint32_t H = w - 1, tile_start = blockIdx.x * TS;
    for (uint32_t q = threadIdx.x; q < H + TS; q += SB) {
        const int64_t g = (int64_t)tile_start - (int64_t)H + q;
        L[q] = (g >= 0 && g < (int64_t)n) ? x[g] : (T)0;
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < TS; j += SB) {
        const uint32_t p = tile_start + j;
        if (p >= n) break;
        const uint32_t len = len_of(p), idx = H + j;            // L[idx] holds row p; len <= w, so idx + 1 - len >= 0
        double var;
        if constexpr (RW > 0) {
            const T k = L[idx];                                   // anchor: the position's own element
            double d[RW], s = 0;
#pragma unroll
            for (int e = 0; e < RW; ++e) { d[e] = (uint32_t)e < len ? anchored(L[idx - e], k) : 0.0; s += d[e]; }
            const double m = s / (double)len;
            double q = 0;
#pragma unroll
            for (int e = 0; e < RW; ++e) if ((uint32_t)e < len) { const double t = d[e] - m; q += t * t; }
            var = q / (double)len;
        } else {
            const uint32_t lo = idx + 1 - len;
            const T k = L[lo];                                    // anchor: the window's first element
            double s = 0;
            for (uint32_t e = lo + 1; e <= idx; ++e) s += anchored(L[e], k);
            const double m = s / (double)len;
            double q = 0;
            for (uint32_t e = lo; e <= idx; ++e) { const double t = anchored(L[e], k) - m; q += t * t; }
            var = q / (double)len;
        }
        out[p] = SD ? sqrt(var) : var;
    }
}

// ---- pair statistics (covw / corrw / betaw and their running forms: pair_window.hip) ------------------------------------------------
// The two columns of a pair call have any two of the ten numeric dtypes, and the kernels are not instantiated per (TX, TY): a row is
// staged once into an 8-byte SLOT by a wave-uniform switch on the dtype tag, and everything behind the staging load is dtype-blind.
// Every dtype of up to four bytes and both floating ones convert to double exactly, so their slot is the double and x - k in double IS
// anchored<T>(x, k); an 8-byte integer keeps its bits and the difference is taken in two's complement, as anchored<T> takes it (`wide`).
__device__ inline uint64_t slot_of(double v) { return (uint64_t)__double_as_longlong(v); }
__device__ inline double slot_diff(uint64_t x, uint64_t k, bool wide) {
    return wide ? (double)(int64_t)(x - k) : __longlong_as_double((long long)x) - __longlong_as_double((long long)k);
}
__host__ __device__ inline bool slot_wide(int t) { return t == AQG_INT64 || t == AQG_UINT64; }
// element i of a column of dtype t as a slot (t is one of the ten numeric tags: the entries check it)
__device__ inline uint64_t slot_load(const void* __restrict__ p, int t, uint64_t i) {
    switch (t) {
    case AQG_INT8: return slot_of((double)static_cast<const int8_t*>(p)[i]);
    case AQG_INT16: return slot_of((double)static_cast<const int16_t*>(p)[i]);
    case AQG_INT32: return slot_of((double)static_cast<const int32_t*>(p)[i]);
    case AQG_UINT8: return slot_of((double)static_cast<const uint8_t*>(p)[i]);
    case AQG_UINT16: return slot_of((double)static_cast<const uint16_t*>(p)[i]);
    case AQG_UINT32: return slot_of((double)static_cast<const uint32_t*>(p)[i]);
    case AQG_FLOAT: return slot_of((double)static_cast<const float*>(p)[i]);
    default: return static_cast<const uint64_t*>(p)[i];                      // INT64 / UINT64 / DOUBLE: the bits
    }
}
// the statistic of n rows from their sums about ANY pair of constants: FAM 0 cov, 1 corr, 2 beta (population moments).  The co-deviation
// sums come first, so that the short routes, which hold them directly (sx = sy = 0), and the prefix route share one finish.
// corr: NaN where either computed variance is not positive, clamped to [-1, 1]; beta: NaN where that of x is not positive.
template <int FAM> __device__ inline double pair_finish(double cxy, double cxx, double cyy, double n) {
    if constexpr (FAM == 0) return cxy / n;
    else if constexpr (FAM == 1) {
        if (!(cxx > 0 && cyy > 0)) return __builtin_nan("");
        const double r = cxy / (sqrt(cxx) * sqrt(cyy));
        return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    } else return cxx > 0 ? cxy / cxx : __builtin_nan("");
}
template <int FAM> __device__ inline double pair_value(double sx, double sy, double sxy, double sxx, double syy, double n) {
    const double cxy = sxy - sx * sy / n;
    double cxx = 0, cyy = 0;
    if constexpr (FAM != 0) cxx = sxx - sx * sx / n;
    if constexpr (FAM == 1) cyy = syy - sy * sy / n;
    return pair_finish<FAM>(cxy, cxx, cyy, n);
}
constexpr int pair_sums(int fam) { return fam == 0 ? 3 : (fam == 1 ? 5 : 4); }     // cov: sx sy sxy; beta: + sxx; corr: + syy
template <int NS> struct dsums { double v[NS]; };                                  // {sx, sy, sxy, sxx, syy}, the first NS of them
// co-moments about a pair of anchors, beside mom_alg: kx, ky = the slots of the range's first row, n = rows, fl = bit 0 / 1: x / y is
// `wide` (rides in the aggregate so that the combine needs no dtype), and the five sums of (x - kx), (y - ky), their squares and their
// product.  The combine moves b onto a's anchors with dx = kxb - kxa, dy = kyb - kya:
//   sum (x - kxa)(y - kya) = sxy_b + dx sy_b + dy sx_b + n_b dx dy,   the squares as in mom_alg;
// every term is bounded by n_b range_x range_y.  Identity: n = 0.
struct comom { uint64_t kx, ky; uint32_t n, fl; double sx, sy, sxx, syy, sxy; };
struct comom_alg {
    using A = comom;
    __device__ static A identity() { A r; r.kx = r.ky = 0; r.n = r.fl = 0; r.sx = r.sy = r.sxx = r.syy = r.sxy = 0; return r; }
    __device__ static A lift(uint64_t x, uint64_t y, uint32_t fl) { A r = identity(); r.kx = x; r.ky = y; r.n = 1; r.fl = fl; return r; }
    __device__ static A op(A a, A b) {
        if (!b.n) return a;
        if (!a.n) return b;
        const double dx = slot_diff(b.kx, a.kx, b.fl & 1u), dy = slot_diff(b.ky, a.ky, b.fl & 2u), nb = (double)b.n;
        A r;
        r.kx = a.kx; r.ky = a.ky; r.fl = a.fl;
        r.n = a.n + b.n;
        r.sx = a.sx + (b.sx + nb * dx);
        r.sy = a.sy + (b.sy + nb * dy);
        r.sxx = a.sxx + (b.sxx + (2.0 * dx * b.sx + nb * dx * dx));
        r.syy = a.syy + (b.syy + (2.0 * dy * b.sy + nb * dy * dy));
        r.sxy = a.sxy + (b.sxy + ((dx * b.sy + dy * b.sx) + nb * dx * dy));
        return r;
    }
};

// K2: exclusive scan of the tile aggregates by one workgroup
template <class ALG> __global__ void __launch_bounds__(SB) agg_scan_kernel(typename ALG::A* __restrict__ tile_agg, uint32_t ntiles) {
    using A = typename ALG::A;
    __shared__ A lds_w[8];
    __shared__ A carry_s;
    if (threadIdx.x == 0) carry_s = ALG::identity();
    __syncthreads();
    for (uint32_t base = 0; base < ntiles; base += SB * IT) {
        uint32_t b = base + threadIdx.x * IT;
        A v[IT];
        A a = ALG::identity();
#pragma unroll
        for (int j = 0; j < IT; ++j) { v[j] = (b + j < ntiles) ? tile_agg[b + j] : ALG::identity(); a = ALG::op(a, v[j]); }
        A total;
        A excl = block_scan_excl<ALG>(a, lds_w, total);
        A run = ALG::op(carry_s, excl);
#pragma unroll
        for (int j = 0; j < IT; ++j) { if (b + j < ntiles) tile_agg[b + j] = run; run = ALG::op(run, v[j]); }
        __syncthreads();
        if (threadIdx.x == 0) carry_s = ALG::op(carry_s, total);
        __syncthreads();
    }
}

// K2 for many tiles: chunks of CH aggregates are reduced by one workgroup each, the few chunk totals are scanned by one
// workgroup, then every chunk is scanned with its carry-in (one workgroup over 488k aggregates took 0.57 ms at 1e9 rows)
constexpr uint32_t CH = SB * IT;
template <class ALG> __global__ void __launch_bounds__(SB) agg_chunk_sum_kernel(const typename ALG::A* __restrict__ tile_agg, uint32_t ntiles, typename ALG::A* __restrict__ chunk_tot) {
    using A = typename ALG::A;
    __shared__ A lds_w[8];
    const uint32_t b = blockIdx.x * CH + threadIdx.x * IT;
    A a = ALG::identity();
#pragma unroll
    for (int j = 0; j < IT; ++j) if (b + j < ntiles) a = ALG::op(a, tile_agg[b + j]);
    A total;
    block_scan_excl<ALG>(a, lds_w, total);
    if (threadIdx.x == 0) chunk_tot[blockIdx.x] = total;
}
template <class ALG> __global__ void __launch_bounds__(SB) agg_chunk_scan_kernel(typename ALG::A* __restrict__ tile_agg, uint32_t ntiles, const typename ALG::A* __restrict__ chunk_excl) {
    using A = typename ALG::A;
    __shared__ A lds_w[8];
    const uint32_t b = blockIdx.x * CH + threadIdx.x * IT;
    A v[IT];
    A a = ALG::identity();
#pragma unroll
    for (int j = 0; j < IT; ++j) { v[j] = (b + j < ntiles) ? tile_agg[b + j] : ALG::identity(); a = ALG::op(a, v[j]); }
    A total;
    A run = ALG::op(chunk_excl[blockIdx.x], block_scan_excl<ALG>(a, lds_w, total));
#pragma unroll
    for (int j = 0; j < IT; ++j) { if (b + j < ntiles) tile_agg[b + j] = run; run = ALG::op(run, v[j]); }
}
// exclusive scan of the tile aggregates in place; `chunk_tot` holds ceil(ntiles / CH) + 1 values of workspace
template <class ALG> void launch_agg_scan(aqg_ctx* ctx, typename ALG::A* tile_agg, uint32_t ntiles, typename ALG::A* chunk_tot) {
    if (ntiles <= 4 * CH || !chunk_tot) { hipLaunchKernelGGL((agg_scan_kernel<ALG>), dim3(1), dim3(SB), 0, ctx->stream, tile_agg, ntiles); return; }
    const uint32_t nch = aqg_ceil_div(ntiles, CH);
    hipLaunchKernelGGL((agg_chunk_sum_kernel<ALG>), dim3(nch), dim3(SB), 0, ctx->stream, tile_agg, ntiles, chunk_tot);
    hipLaunchKernelGGL((agg_scan_kernel<ALG>), dim3(1), dim3(SB), 0, ctx->stream, chunk_tot, nch);
    hipLaunchKernelGGL((agg_chunk_scan_kernel<ALG>), dim3(nch), dim3(SB), 0, ctx->stream, tile_agg, ntiles, chunk_tot);
}


} // namespace aqgscan
