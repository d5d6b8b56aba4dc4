// scan_window.hpp -- the sliding windows (sumw / avgw, minw / maxw, varw / stddevw), written once for both layouts: a whole column
// (scan.hip) is the flat row-list layout (segscan.hip) of one group.  Every kernel takes its layout as a type: `whole_column`
// carries nothing, and its instantiations hold no load, branch or LDS for group starts; `by_group` carries the bitmap of group starts
// and, for the row-at-a-time kernels of the wide windows, the distance D of every position to its group's start.  window_scan() is
// the one host dispatch; the callers keep what only one layout has (the running form of a window as long as the column, van Herk).
#pragma once
#include "scan_dev.hpp"

namespace aqgscan {

constexpr uint32_t DIRECT_MAX_W = 64;             // floating sumw / avgw up to this long add their rows one by one

// ---- group starts ----------------------------------------------------------------------------------------------------------------
__device__ inline bool head_bit(const uint32_t* __restrict__ heads, uint32_t p) { return (heads[p >> 5] >> (p & 31)) & 1u; }
// number of predecessors of position p inside its group, capped at maxd (walks the bitmap backwards; position 0 always starts a group)
__device__ inline uint32_t dist_to_head(const uint32_t* __restrict__ heads, uint32_t p, uint32_t maxd) {
    uint32_t wi = p >> 5;
    const uint32_t b = p & 31;
    uint32_t m = heads[wi] & (0xFFFFFFFFu >> (31 - b));
    if (m) { const uint32_t d = b - (31 - __clz((int)m)); return d < maxd ? d : maxd; }
    uint32_t d = b + 1;
    while (d <= maxd && wi > 0) {
        m = heads[--wi];
        if (m) { d += __clz((int)m); return d < maxd ? d : maxd; }
        d += 32;
    }
    return maxd;
}

// ---- the two layouts: dist(i) = predecessors of row i in its group, len(i, w) = rows of the window of length w that ends at i ----
struct whole_column {
    static constexpr bool SEG = false;
    __device__ uint32_t dist(uint32_t i) const { return i; }
    __device__ uint32_t len(uint32_t i, uint32_t w) const { return i + 1 < w ? i + 1 : w; }            // growing prefix for i < w
};
struct by_group {
    static constexpr bool SEG = true;
    const uint32_t* heads;      // bit p: position p starts a group (bit n is set; padded: the byte behind a block may be read)
    const uint32_t* D;          // distance column (the wide-window kernels only; null elsewhere)
    __device__ uint32_t dist(uint32_t i) const { return D[i]; }
    __device__ uint32_t len(uint32_t i, uint32_t w) const { return dist_to_head(heads, i, w - 1) + 1; }
    __device__ const uint8_t* heads8() const { return reinterpret_cast<const uint8_t*>(heads); }
};

// position + 1 of the last group start in or before each block of IT positions of the extended tile (0: none in this tile): one
// round of the blocked loops below.  `lh` = that of the lane's own block alone; returns what lies BEFORE the block.
__device__ inline uint32_t starts_before(uint32_t lh, uint32_t& carry_m, uint32_t* lds_m) {
    using MX = max_alg<uint32_t>;
    uint32_t totm;
    const uint32_t before = MX::op(carry_m, block_scan_excl<MX>(lh, lds_m, totm));
    carry_m = MX::op(carry_m, totm);
    return before;
}

// ---- sliding sums: tile + halo in LDS, prefix difference -------------------------------------------
// MODE 0 sumw (LongType out) / 1 avgw (double).  by_group: every window is clamped at its group's start.
template <class T, int MODE, class M>
__global__ void __launch_bounds__(SB) window_sum_kernel(const T* __restrict__ x, uint32_t n, uint32_t w, M seg, void* __restrict__ out) {
    using ALG = sum_alg<T>;
    using A = typename ALG::A;
    // Integer sums wrap, so one prefix over the whole extended tile serves every group.  A floating prefix does not: the difference of
    // two prefixes carries the rounding of everything in front of the window, other groups' rows included (a group of ones behind a
    // group of 1e30s came out as noise).  Floating columns restart the prefix at every group start (seg_alg).
    constexpr bool SEG = M::SEG, RESTART = SEG && std::is_floating_point_v<T>;
    using SA = seg_alg<ALG>;
    using C = typename SA::A;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    __shared__ A lds_w[8];
    C* lds_c = nullptr;
    uint32_t* lds_m = nullptr;
    if constexpr (RESTART) { __shared__ C c[8]; lds_c = c; }
    if constexpr (SEG) { __shared__ uint32_t m[8]; lds_m = m; }
    const uint32_t tile_start = blockIdx.x * TS, tile_end = tile_start + TS < n ? tile_start + TS : n;
    // LDS position p <-> row tile_start - H + p, with the halo H = w - 1 rounded up to whole blocks of IT rows; rows before
    // row 0 count as zeros, so the growing prefix of the first w rows needs no special case below
    const uint32_t H = (w - 1 + IT - 1) / IT * IT;
    const uint32_t L = H + TS, nblk = L / IT;
    A* S = reinterpret_cast<A*>(smem_raw);                       // inclusive prefix of x over the extended tile
    uint32_t* LH = reinterpret_cast<uint32_t*>(S + L);            // SEG, per block of IT positions: {position + 1 of the last group start BEFORE the block (0: none in this tile), the block's start bits : 8}
    // a lane takes blocks of IT consecutive rows straight from HBM (vector load), scans them in registers and writes the
    // prefixes to LDS once; blocks beyond the first SB (the halo's worth) take further rounds with a running carry
    A carry = ALG::identity();
    C carry_c = SA::identity();
    uint32_t carry_m = 0;
    for (uint32_t blk0 = 0; blk0 < nblk; blk0 += SB) {
        const uint32_t blk = blk0 + threadIdx.x;
        const int64_t g0 = (int64_t)tile_start - (int64_t)H + (int64_t)blk * IT;
        T v[IT];
        if (blk < nblk && g0 >= 0 && g0 + IT <= (int64_t)n && (((uintptr_t)(x + g0)) & (sizeof(T) * IT > 16 ? 15 : sizeof(T) * IT - 1)) == 0) {
            pack<T, IT> pk = *reinterpret_cast<const pack<T, IT>*>(x + g0);
#pragma unroll
            for (int j = 0; j < IT; ++j) v[j] = pk.v[j];
        } else {
#pragma unroll
            for (int j = 0; j < IT; ++j) { const int64_t g = g0 + j; v[j] = (blk < nblk && g >= 0 && g < (int64_t)n) ? x[g] : (T)0; }
        }
        uint32_t hb = 0, lh = 0;
        if constexpr (SEG) {
            hb = (blk < nblk && g0 >= 0 && g0 < (int64_t)n) ? seg.heads8()[g0 >> 3] : 0u;
            lh = hb ? blk * IT + (31 - __clz((int)hb)) + 1 : 0u;
        }
        A loc[IT];
        A a = ALG::identity();
        A excl;
        if constexpr (RESTART) {
            C ac = SA::identity();
#pragma unroll
            for (int j = 0; j < IT; ++j) {
                if ((hb >> j) & 1u) { ac.v = ALG::identity(); ac.s = 1; ++ac.c; }
                ac.v = ALG::op(ac.v, ALG::lift(v[j]));
                loc[j] = ac.v;
            }
            C totc;
            const C ec = SA::op(carry_c, block_scan_excl<SA>(ac, lds_c, totc));
            excl = ec.v;                                            // what the group that reaches into this block has summed before it
            carry_c = SA::op(carry_c, totc);
        } else {
#pragma unroll
            for (int j = 0; j < IT; ++j) { a = ALG::op(a, ALG::lift(v[j])); loc[j] = a; }
            A tot;
            excl = ALG::op(carry, block_scan_excl<ALG>(a, lds_w, tot));
            carry = ALG::op(carry, tot);
        }
        uint32_t before = 0;
        if constexpr (SEG) before = starts_before(lh, carry_m, lds_m);
        if (blk < nblk) {
#pragma unroll
            for (int j = 0; j < IT; ++j) S[blk * IT + j] = (RESTART && (hb & ((2u << j) - 1u))) ? loc[j] : ALG::op(excl, loc[j]);   // behind a start inside the block: no carry-in
            if constexpr (SEG) LH[blk] = (before << 8) | hb;
        }
    }
    __syncthreads();
    for (uint32_t i = tile_start + threadIdx.x; i < tile_end; i += SB) {
        const uint32_t idx = i - tile_start + H;
        uint32_t len, lower, st = 0;                              // the window is LDS positions lower .. idx
        if constexpr (SEG) {
            const uint32_t blk = idx >> 3, j = idx & 7;
            const uint32_t lhb = LH[blk], m = lhb & ((2u << j) - 1u);
            st = m ? blk * IT + (31 - __clz((int)m)) + 1 : (lhb >> 8);  // position + 1 of the group's start (0: further back than the halo)
            lower = idx + 1 - w;                                  // idx >= H >= w - 1
            if (st && st - 1 > lower) lower = st - 1;
            len = idx - lower + 1;
        } else {
            len = seg.len(i, w);
            lower = idx + 1 - len;
        }
        A s = lower ? ALG::sub(S[idx], S[lower - 1]) : S[idx];
        if constexpr (RESTART) { if (st && st - 1 == lower) s = S[idx]; }    // the window starts where the group does: the restarted prefix is the sum
        if constexpr (MODE == 0) {
            if constexpr (std::is_floating_point_v<T>) static_cast<double*>(out)[i] = s;
            else static_cast<aqg_i128*>(out)[i] = ALG::to_i128(s);
        } else {
            static_cast<double*>(out)[i] = ALG::to_double(s) / (double)len;
        }
    }
}

// floating inputs, short windows: add the window's elements directly (oldest first) -- no prefix cancellation.  Each layout keeps
// the loop it was measured with: grid-stride for a whole column, one span of rows per workgroup for groups.
template <class T, int MODE, class M>
__global__ void __launch_bounds__(SB) window_direct_kernel(const T* __restrict__ x, uint32_t n, uint32_t w, M seg, double* __restrict__ out) {
    auto row = [&](uint32_t i) {
        const uint32_t len = seg.len(i, w);
        double s = 0;
        for (uint32_t j = i + 1 - len; j <= i; ++j) s += (double)x[j];
        out[i] = MODE == 0 ? s : s / (double)len;
    };
    if constexpr (M::SEG) {
        uint32_t lo, hi;
        wg_span(n, lo, hi, 256);
        for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) row(i);
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) row(i);
    }
}
// large-window fallback for sums: out[i] = S[i] - S[i-len] over an inclusive prefix S in accumulator form that restarts with every group
template <class T, int MODE, class M>
__global__ void __launch_bounds__(SB) prefix_diff_kernel(const typename sum_alg<T>::A* __restrict__ S, M seg, uint32_t n, uint32_t w, void* __restrict__ out) {
    using ALG = sum_alg<T>;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t d = seg.dist(i), len = d + 1 < w ? d + 1 : w;
        auto s = d >= len ? ALG::sub(S[i], S[i - len]) : S[i];
        if constexpr (MODE == 0) {
            if constexpr (std::is_floating_point_v<T>) static_cast<double*>(out)[i] = s; else static_cast<aqg_i128*>(out)[i] = ALG::to_i128(s);
        } else static_cast<double*>(out)[i] = ALG::to_double(s) / (double)len;
    }
}

// ---- sliding min / max: tile + halo in LDS, doubling, eight elements per lane ---------------------------------------------
// M_k[p] = best of the 2^k elements ending at p; M_{k+1}[p] = better(M_k[p], M_k[p - 2^k]); the window of length w is
// better(M_K[p], M_K[p - (w - 2^K)]) with 2^K <= w < 2^(K+1).  A lane works on blocks of eight consecutive positions: the levels
// with 2^k < 8 happen in registers in one step (block + predecessor block), every later level reads its neighbour block with
// 16-byte LDS loads (positions are laid out so that blocks are 16-byte aligned).  Positions before row 0 hold the identity, so
// the growing prefix of the first w rows needs no special case.  (Element-at-a-time doubling: minw(100) ran at 34 % of the
// HBM roofline, bounded by LDS instructions.)
// by_group: a level is taken only where the position 2^k back still belongs to the group: DS[p] = predecessors of p inside its
// group (16 bits, capped; a start further back than the halo: "far").
template <class T, bool IS_MAX, class M>
__global__ void __launch_bounds__(SB) window_minmax_kernel(const T* __restrict__ x, uint32_t n, uint32_t w, M seg, T* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    using ALG = minmax_alg<T, IS_MAX>;
    constexpr bool SEG = M::SEG;
    constexpr int E = 8;
    struct alignas(E * sizeof(T) > 16 ? 16 : E * sizeof(T)) blk_t { T v[E]; };
    struct alignas(16) dblk_t { uint16_t d[E]; };
    const uint32_t tile_start = blockIdx.x * TS;
    const uint32_t H = (w - 1 + E - 1) / E * E;                   // halo, rounded up to whole blocks
    const uint32_t L = H + TS, nblk = L / E;                      // LDS position p <-> row tile_start - H + p
    T* M0 = reinterpret_cast<T*>(smem_raw);
    T* M1 = M0 + L;
    uint16_t* DS = reinterpret_cast<uint16_t*>(M1 + L);           // SEG only
    const T ident = ALG::identity();
    for (uint32_t p = threadIdx.x; p < H; p += SB) {
        const int64_t g = (int64_t)tile_start - (int64_t)H + p;
        M0[p] = g >= 0 ? x[g] : ident;                            // g < tile_start <= n - 1
    }
    {
        const uint32_t g0 = tile_start + threadIdx.x * E;         // TS == SB * E: one block of the tile per lane
        blk_t b;
        if (g0 + E <= n && (reinterpret_cast<uintptr_t>(x + g0) & (alignof(blk_t) - 1)) == 0) b = *reinterpret_cast<const blk_t*>(x + g0);
        else {
#pragma unroll
            for (int q = 0; q < E; ++q) b.v[q] = g0 + q < n ? x[g0 + q] : ident;
        }
        *reinterpret_cast<blk_t*>(M0 + H + threadIdx.x * E) = b;
    }
    if constexpr (SEG) {                                           // distances to the group starts
        __shared__ uint32_t lds_m[8];
        uint32_t carry_m = 0;
        for (uint32_t blk0 = 0; blk0 < nblk; blk0 += SB) {
            const uint32_t blk = blk0 + threadIdx.x;
            const int64_t g0 = (int64_t)tile_start - (int64_t)H + (int64_t)blk * E;
            const uint32_t hb = (blk < nblk && g0 >= 0 && g0 < (int64_t)n) ? seg.heads8()[g0 >> 3] : 0u;
            const uint32_t lh = hb ? blk * E + (31 - __clz((int)hb)) + 1 : 0u;
            uint32_t cur = starts_before(lh, carry_m, lds_m);
            if (blk < nblk) {
                dblk_t dd;
#pragma unroll
                for (int q = 0; q < E; ++q) {
                    if ((hb >> q) & 1) cur = blk * E + q + 1;
                    const uint32_t dist = cur ? blk * E + q - (cur - 1) : 0xFFFFu;
                    dd.d[q] = (uint16_t)(dist < 0xFFFFu ? dist : 0xFFFFu);
                }
                *reinterpret_cast<dblk_t*>(DS + blk * E) = dd;
            }
        }
    }
    __syncthreads();
    uint32_t K = 0;
    while ((2u << K) <= w) ++K;                                    // 2^K <= w < 2^(K+1)
    const uint32_t KA = K < 3 ? K : 3;
    T* cur = M0; T* nxt = M1;
    if (KA) {                                                      // levels 0 .. KA-1 in registers
        for (uint32_t blk = threadIdx.x; blk < nblk; blk += SB) {
            T a[2 * E];
            uint32_t dist[SEG ? 2 * E : 1];
            const blk_t own = *reinterpret_cast<const blk_t*>(cur + blk * E);
            blk_t prev;
            if (blk) prev = *reinterpret_cast<const blk_t*>(cur + (blk - 1) * E);
#pragma unroll
            for (int q = 0; q < E; ++q) { a[q] = blk ? prev.v[q] : ident; a[E + q] = own.v[q]; }
            if constexpr (SEG) {
                const dblk_t downd = *reinterpret_cast<const dblk_t*>(DS + blk * E);
                dblk_t dprev;
                if (blk) dprev = *reinterpret_cast<const dblk_t*>(DS + (blk - 1) * E);
#pragma unroll
                for (int q = 0; q < E; ++q) { dist[q] = blk ? dprev.d[q] : 0u; dist[E + q] = downd.d[q]; }
            }
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k) {
                if (k < KA) {
                    const int d = 1 << k;
#pragma unroll
                    for (int j = 2 * E - 1; j >= d; --j) {
                        if constexpr (SEG) { if (dist[j] < (uint32_t)d) continue; }
                        a[j] = ALG::op(a[j], a[j - d]);
                    }
                }
            }
            blk_t o;
#pragma unroll
            for (int q = 0; q < E; ++q) o.v[q] = a[E + q];
            *reinterpret_cast<blk_t*>(nxt + blk * E) = o;
        }
        __syncthreads();
        T* t = cur; cur = nxt; nxt = t;
    }
    for (uint32_t k = KA; k < K; ++k) {                            // 2^k is a multiple of the block: aligned neighbour blocks
        const uint32_t db = (1u << k) / E, dk = 1u << k;
        for (uint32_t blk = threadIdx.x; blk < nblk; blk += SB) {
            blk_t a = *reinterpret_cast<const blk_t*>(cur + blk * E);
            if (blk >= db) {
                const blk_t b = *reinterpret_cast<const blk_t*>(cur + (blk - db) * E);
                dblk_t dd;
                if constexpr (SEG) dd = *reinterpret_cast<const dblk_t*>(DS + blk * E);
#pragma unroll
                for (int q = 0; q < E; ++q) {
                    if constexpr (SEG) { if (dd.d[q] < dk) continue; }
                    a.v[q] = ALG::op(a.v[q], b.v[q]);
                }
            }
            *reinterpret_cast<blk_t*>(nxt + blk * E) = a;
        }
        __syncthreads();
        T* t = cur; cur = nxt; nxt = t;
    }
    const uint32_t off = w - (1u << K);                            // second span ends off positions earlier (0 <= off < 2^K, off <= H)
    const uint32_t p0 = H + threadIdx.x * E, g0 = tile_start + threadIdx.x * E;
    if (g0 < n) {
        blk_t a = *reinterpret_cast<const blk_t*>(cur + p0);
        if (off) {
            dblk_t dd;
            if constexpr (SEG) dd = *reinterpret_cast<const dblk_t*>(DS + p0);
#pragma unroll
            for (int q = 0; q < E; ++q) {
                if constexpr (SEG) { if (dd.d[q] < off) continue; }
                a.v[q] = ALG::op(a.v[q], cur[p0 + q - off]);
            }
        }
        if (g0 + E <= n && (reinterpret_cast<uintptr_t>(out + g0) & (alignof(blk_t) - 1)) == 0) *reinterpret_cast<blk_t*>(out + g0) = a;
        else {
#pragma unroll
            for (int q = 0; q < E; ++q) if (g0 + q < n) out[g0 + q] = a.v[q];
        }
    }
}

// large-window fallback for min/max: doubling passes through HBM (ping-pong), then the two-span combine
template <class T, bool IS_MAX, class M>
__global__ void __launch_bounds__(SB) doubling_pass_kernel(const T* __restrict__ src, T* __restrict__ dst, M seg, uint32_t n, uint32_t d) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        T a = src[i];
        if (seg.dist(i) >= d) a = minmax_alg<T, IS_MAX>::op(a, src[i - d]);
        dst[i] = a;
    }
}
template <class T, bool IS_MAX, class M>
__global__ void __launch_bounds__(SB) doubling_final_kernel(const T* __restrict__ m, T* __restrict__ out, M seg, uint32_t n, uint32_t w, uint32_t span) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t d = seg.dist(i), len = d + 1 < w ? d + 1 : w;
        T a = m[i];
        if (len > span) a = minmax_alg<T, IS_MAX>::op(a, m[i - (len - span)]);
        out[i] = a;
    }
}

// ---- sliding variances ------------------------------------------------------------------------------------------------------------
// varw / stddevw, windows of up to VAR_DIRECT_MAX_W: one tile per workgroup (var_short_tile)
template <class T, bool SD, int RW, class M>
__global__ void __launch_bounds__(SB) var_short_kernel(const T* __restrict__ x, uint32_t n, uint32_t w, M seg, double* __restrict__ out) {
    __shared__ T L[TS + VAR_DIRECT_MAX_W];
    var_short_tile<T, SD, RW>(x, n, w, [&](uint32_t p) { return seg.len(p, w); }, L, out);
}
// windows of any length: P[i] = anchored sums of x over [first of the group .. i], one anchor per group; the window is the
// difference of two of them
template <bool SD, class M>
__global__ void __launch_bounds__(SB) var_prefix_diff_kernel(const dpair* __restrict__ P, M seg, uint32_t n, uint32_t w, double* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t d = seg.dist(i), len = d + 1 < w ? d + 1 : w;
        dpair a = P[i];
        if (len <= d) { const dpair b = P[i - len]; a.s -= b.s; a.q -= b.q; }
        const double v = var_from(a.s, a.q, (double)len);
        out[i] = SD ? sqrt(v) : v;
    }
}

// ---- host: the one window dispatch ---------------------------------------------------------------------------------------------------
// allow the dynamic LDS, time, launch, check
template <class K, class... Args>
int launch_window(aqg_ctx* ctx, K kern, unsigned grid, unsigned block, size_t lds, const char* what, Args... args) {
    if (lds) AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
    aqg_kernel_timer_begin(ctx);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, ctx->stream, args...);
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, what);
}

// sumw / avgw / minw / maxw / varw / stddevw of n rows with the window ww (1 <= ww <= n; for minw / maxw ww < n: the caller takes the
// running form).  LAYOUT (column_windows of scan.hip, group_windows of segscan.hip) gives
//   seg_t, seg()            the kernels' layout argument (without distances)
//   row_grid                the grid of the row-at-a-time kernels
//   reserve(bytes)          workspace for `bytes` of the buffers taken here, on top of what its own producers take
//   raw_prefix(S)           S[i] = sum of the rows of i's group up to i, in accumulator form
//   moments(P)              P[i] = anchored moments of the same rows
//   distances(seg)          fills in what seg.dist() reads
template <class T, class LAYOUT>
int window_scan(aqg_ctx* ctx, LAYOUT& lay, int op, const T* x, uint32_t n, uint32_t ww, void* out) {
    using M = typename LAYOUT::seg_t;
    const uint32_t ntiles = aqg_ceil_div(n, TS);
    auto tiles = [&](auto kern, size_t lds, const char* what, auto* o) { return launch_window(ctx, kern, ntiles, SB, lds, what, x, n, ww, lay.seg(), o); };
    auto rows = [&](auto kern, auto... args) { hipLaunchKernelGGL(kern, dim3(lay.row_grid), dim3(SB), 0, ctx->stream, args...); };
    switch (op) {
    case AQG_SCAN_VARW: case AQG_SCAN_STDDEVW: {
        // the intended population variance of the last min(w, rows of the group so far) rows (D9)
        const bool sd = op == AQG_SCAN_STDDEVW;
        double* o = static_cast<double*>(out);
        if (ww <= (uint32_t)VAR_REG_W) return sd ? tiles(&var_short_kernel<T, true, VAR_REG_W, M>, 0, "var_short_kernel", o) : tiles(&var_short_kernel<T, false, VAR_REG_W, M>, 0, "var_short_kernel", o);
        if (ww <= VAR_DIRECT_MAX_W) return sd ? tiles(&var_short_kernel<T, true, 0, M>, 0, "var_short_kernel", o) : tiles(&var_short_kernel<T, false, 0, M>, 0, "var_short_kernel", o);
        AQG_TRY(lay.reserve((size_t)n * sizeof(dpair)));
        dpair* P;
        AQG_TRY(aqg_ws_get(ctx, n, &P));
        if constexpr (!M::SEG) aqg_kernel_timer_begin(ctx);                 // a whole column: the timer spans every pass (per group: the last producer's scan, as before)
        AQG_TRY(lay.moments(P));
        M seg = lay.seg();
        AQG_TRY(lay.distances(seg));
        if (sd) rows(&var_prefix_diff_kernel<true, M>, P, seg, n, ww, o); else rows(&var_prefix_diff_kernel<false, M>, P, seg, n, ww, o);
        if constexpr (!M::SEG) aqg_kernel_timer_end(ctx);
        return aqg_check_launch(ctx, "wide window variance");
    }
    case AQG_SCAN_SUMW: case AQG_SCAN_AVGW: {
        using A = typename sum_alg<T>::A;
        const bool avg = op == AQG_SCAN_AVGW;
        if constexpr (std::is_floating_point_v<T>) {
            if (ww <= DIRECT_MAX_W) {
                double* o = static_cast<double*>(out);
                return avg ? launch_window(ctx, &window_direct_kernel<T, 1, M>, lay.row_grid, SB, 0, "window_direct_kernel", x, n, ww, lay.seg(), o)
                           : launch_window(ctx, &window_direct_kernel<T, 0, M>, lay.row_grid, SB, 0, "window_direct_kernel", x, n, ww, lay.seg(), o);
            }
        }
        const size_t ext = (size_t)TS + (ww - 1 + IT - 1) / IT * IT;            // tile + halo rounded up to whole blocks
        const size_t lds = ext * sizeof(A) + (M::SEG ? ext / IT * 4 + 16 : 0);  // by_group: one {last start, start bits} word per block
        if (lds <= HALO_MAX_BYTES) return avg ? tiles(&window_sum_kernel<T, 1, M>, lds, "window_sum_kernel", out) : tiles(&window_sum_kernel<T, 0, M>, lds, "window_sum_kernel", out);
        // wide window: inclusive prefix through HBM, then the difference
        AQG_TRY(lay.reserve((size_t)n * sizeof(A)));
        A* S;
        AQG_TRY(aqg_ws_get(ctx, n, &S));
        AQG_TRY(lay.raw_prefix(S));
        M seg = lay.seg();
        AQG_TRY(lay.distances(seg));
        if (avg) rows(&prefix_diff_kernel<T, 1, M>, S, seg, n, ww, out); else rows(&prefix_diff_kernel<T, 0, M>, S, seg, n, ww, out);
        return aqg_check_launch(ctx, "wide window sum");
    }
    case AQG_SCAN_MINW: case AQG_SCAN_MAXW: {
        const bool is_max = op == AQG_SCAN_MAXW;
        T* o = static_cast<T*>(out);
        const size_t ext = (size_t)TS + (ww - 1 + 7) / 8 * 8;
        const size_t lds = ext * sizeof(T) * 2 + (M::SEG ? ext * 2 + 16 : 0);   // by_group: 16-bit distances
        if (lds <= HALO_MAX_BYTES) return is_max ? tiles(&window_minmax_kernel<T, true, M>, lds, "window_minmax_kernel", o) : tiles(&window_minmax_kernel<T, false, M>, lds, "window_minmax_kernel", o);
        // wide window: doubling passes through HBM
        AQG_TRY(lay.reserve((size_t)n * sizeof(T) * 2));
        T *b0, *b1;
        AQG_TRY(aqg_ws_get(ctx, n, &b0));
        AQG_TRY(aqg_ws_get(ctx, n, &b1));
        M seg = lay.seg();
        AQG_TRY(lay.distances(seg));
        uint32_t K = 0;
        while ((2u << K) <= ww && K < 31) ++K;
        const T* src = x;
        T* dst = b0;
        for (uint32_t k = 0; k < K; ++k) {
            if (is_max) rows(&doubling_pass_kernel<T, true, M>, src, dst, seg, n, 1u << k); else rows(&doubling_pass_kernel<T, false, M>, src, dst, seg, n, 1u << k);
            src = dst;
            dst = dst == b0 ? b1 : b0;
        }
        if (is_max) rows(&doubling_final_kernel<T, true, M>, src, o, seg, n, ww, 1u << K); else rows(&doubling_final_kernel<T, false, M>, src, o, seg, n, ww, 1u << K);
        return aqg_check_launch(ctx, "wide window min/max");
    }
    }
    return AQG_ERR_ARG;
}

} // namespace aqgscan
