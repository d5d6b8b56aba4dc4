// tile_scatter.hip -- the tile scatter of the partition plans: its kernels (the only translation unit that instantiates them) and one host
// function per launch sequence the plans repeat (tile_scatter.hpp)
#include "partition1_int.hpp"
#include "tile_scatter.hpp"

namespace {

// ==== two levels (more partitions than one level writes well) ==================================================================
// The run a tile writes per bin and plane is (LDS staging bytes / bins) long: 3000 bins leave 44-byte runs, and partial lines are
// what the memory system charges for (measured at 1e9 rows, 5 planes: the one-level scatter takes 8.0 ms at 64 bins, 10.6 at 256,
// 17 at 1024, 31 at 2900 -- the bytes at the L2 / fabric interface only grow from 41 to 53 GB).  Beyond ~1000 partitions the rows
// therefore move TWICE, through <= 64 coarse and then 64 fine bins per coarse one, in runs of a kilobyte:
//   p2_hist      sizes of the P fine partitions (P = 64 B1; LDS counters per workgroup, merged with global atomics)
//   p2_setup     exclusive scan -> partition starts; the write cursors of both levels
//   p2_scatter   level 1: user columns -> buffer set A by coarse bin; level 2: set A -> set B by fine bin inside each coarse
//                partition.  A tile is independent: it ranks its rows inside their bins (LDS atomics), RESERVES its run of every
//                bin with one global atomicAdd on that bin's cursor, stages each plane bin-major and streams it out.  No per-tile
//                histogram, no scan between the levels; rows inside a partition end up in arrival order (the aggregation does not
//                care: first rows come from the carried row ids).
//   p1_agg       as for one level, over the P fine partitions

// ---- 1- / 2-byte values -> dwords ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) p1_widen_kernel(const void* __restrict__ col, int esz, uint32_t n, uint32_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = esz == 1 ? (uint32_t)static_cast<const uint8_t*>(col)[i] : (uint32_t)static_cast<const uint16_t*>(col)[i];
}

template <int TB> __device__ inline uint32_t trow(int r) { return (uint32_t)(r >> 2) * (TB * 4) + threadIdx.x * 4 + (r & 3); }
template <int TB, bool FULL, class T, int R> __device__ inline void load_rows_t(const T* __restrict__ p, size_t tile_first, uint32_t nrows, int r0, T (&t)[R]) {
    const T* tp = p + tile_first;
    if constexpr (FULL) {
#pragma unroll
        for (int c = 0; c < R / 4; ++c) __builtin_memcpy(&t[4 * c], tp + trow<TB>(r0 + 4 * c), 4 * sizeof(T));
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) { const uint32_t o = trow<TB>(r0 + r); t[r] = tp[o < nrows ? o : nrows - 1]; }
    }
}

constexpr int HB = 16;    // rows per thread and step of the fine histogram
template <bool K64, bool RANGED = false>
__global__ void __launch_bounds__(1024) p2_hist_kernel(const key_t_<K64>* __restrict__ keys, uint32_t n, uint32_t P, uint32_t* __restrict__ ftot, uint32_t kmin = 0, uint32_t xmax = 0) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint32_t* cnt = reinterpret_cast<uint32_t*>(smem_raw);
    for (uint32_t b = threadIdx.x; b < (RANGED ? __umulhi(xmax, P) + 1 : P); b += 1024) cnt[b] = 0;
    __syncthreads();
    const uint64_t step = (uint64_t)1024 * HB;
    auto count = [&](const key_t_<K64> (&key)[HB], uint32_t nrows) {
#pragma unroll
        for (int r = 0; r < HB; ++r) {
            if (!(trow<1024>(r) < nrows)) continue;
            uint32_t h;
            if constexpr (RANGED) { h = (uint32_t)key[r] - kmin; h = h < xmax ? h : xmax; }       // (a key outside the sampled range: the scatter flags it)
            else h = key_hash<K64>(key[r]);
            atomicAdd(&cnt[__umulhi(h, P)], 1u);
        }
    };
    // whole steps, the next one's keys in flight while this one's are counted (one code path for the loads: a loader that may take the
    // clamped form is waited for right behind its loads); the partial step at the end of the column by itself
    const uint64_t nfull = (uint64_t)n / step, stride = gridDim.x;
    uint64_t t = blockIdx.x;
    key_t_<K64> cur[HB];
    if (t < nfull) load_rows_t<1024, true>(keys, t * step, (uint32_t)step, 0, cur);
    while (t < nfull) {
        const uint64_t tn = t + stride;
        key_t_<K64> nxt[HB];
        load_rows_t<1024, true>(keys, (tn < nfull ? tn : t) * step, (uint32_t)step, 0, nxt);
        __builtin_amdgcn_sched_barrier(0);
        count(cur, (uint32_t)step);
#pragma unroll
        for (int r = 0; r < HB; ++r) cur[r] = nxt[r];
        t = tn;
    }
    if (blockIdx.x == 0 && nfull * step < n) {
        key_t_<K64> last[HB];
        const uint32_t nrows = (uint32_t)(n - nfull * step);
        load_rows_t<1024, false>(keys, nfull * step, nrows, 0, last);
        count(last, nrows);
    }
    __syncthreads();
    const uint32_t nb = RANGED ? __umulhi(xmax, P) + 1 : P;                                        // (RANGED: P is the multiplier, not the bin count)
    for (uint32_t b = threadIdx.x; b < nb; b += 1024) { const uint32_t c = cnt[b]; if (c) atomicAdd(&ftot[b], c); }
}

// one workgroup: fstart = exclusive scan of the P partition sizes (P <= 4096); segments, tile counts and cursors of both levels
__global__ void __launch_bounds__(1024) p2_setup_kernel(const uint32_t* __restrict__ ftot, uint32_t P, uint32_t n, uint32_t tile_rows,
                                                        uint32_t* __restrict__ fstart /* [P + 1] */, uint32_t* __restrict__ cur2 /* [P] */,
                                                        uint32_t* __restrict__ seg1 /* [2] */, uint32_t* __restrict__ tp1 /* [2] */, uint32_t* __restrict__ cur1 /* [P / 64] */,
                                                        uint32_t* __restrict__ seg2 /* [P / 64 + 1] */, uint32_t* __restrict__ tp2 /* [P / 64 + 1] */,
                                                        uint32_t* __restrict__ xtp /* [8 * XTP_STRIDE + 1] or null */, uint32_t grid_per_xcd) {
    __shared__ uint32_t wsum[16], fs[4097], tcount[65], stile[64], xmax[8];
    uint32_t c[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint32_t b = threadIdx.x * 4 + k; c[k] = b < P ? ftot[b] : 0; s += c[k]; }
    const uint32_t incl = wave_scan_incl(s, OpAdd{}, lane_id());
    if (lane_id() == 63) wsum[wave_id()] = incl;
    __syncthreads();
    uint32_t base = incl - s;
    for (int w = 0; w < wave_id(); ++w) base += wsum[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = threadIdx.x * 4 + k;
        if (b < P) { fstart[b] = base; cur2[b] = base; fs[b] = base; }
        base += c[k];
    }
    if (threadIdx.x == 0) { fstart[P] = n; fs[P] = n; seg1[0] = 0; seg1[1] = n; tp1[0] = 0; tp1[1] = (uint32_t)(((uint64_t)n + tile_rows - 1) / tile_rows); }
    __syncthreads();
    const uint32_t B1 = P >> 6;
    if (threadIdx.x <= B1) { seg2[threadIdx.x] = fs[threadIdx.x << 6]; if (threadIdx.x < B1) cur1[threadIdx.x] = fs[threadIdx.x << 6]; }
    if (threadIdx.x < 64) {
        const uint32_t len = threadIdx.x < B1 ? fs[(threadIdx.x + 1) << 6] - fs[threadIdx.x << 6] : 0;
        const uint32_t t = (uint32_t)(((uint64_t)len + tile_rows - 1) / tile_rows);
        const uint32_t ti = wave_scan_incl(t, OpAdd{}, lane_id());
        tp2[threadIdx.x] = ti - t;
        if (threadIdx.x == 63) tcount[0] = ti;
        if (threadIdx.x + 1 == B1) tp2[B1] = ti;
        stile[threadIdx.x] = t;
    }
    if (xtp) {                                                   // level 2 by XCD: segments x, x + 8, ... and their tile prefixes
        __syncthreads();
        if (threadIdx.x < 8) {
            uint32_t run = 0, j = 0;
            for (uint32_t sgm = threadIdx.x; sgm < B1; sgm += 8, ++j) { xtp[threadIdx.x * XTP_STRIDE + j] = run; run += stile[sgm]; }
            xtp[threadIdx.x * XTP_STRIDE + j] = run;
            xmax[threadIdx.x] = run;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t m = 0;
            for (int x = 0; x < 8; ++x) m = xmax[x] > m ? xmax[x] : m;
            xtp[8 * XTP_STRIDE] = B1 <= 8 * (XTP_STRIDE - 1) && m <= grid_per_xcd ? 1u : 0u;     // (a skewed table: the plain walk)
            for (int x = 0; x < 8; ++x) xtp[8 * XTP_STRIDE + 32 + x * 32] = 0u;                   // the queue heads
        }
    }
}

// FULL: grid over all tiles of all segments, whole tiles only.  !FULL: one workgroup per segment takes its last, partial tile.
// NBMAX: bins per level, 128 (the levels of the two-level and wide plans) or 256 (the one-level range plan: FUSE0 keeps a bin in a byte)
template <int TB, int TR, bool K64, bool FULL, int MODE = BIN_HASHED, bool PACK = false, int NBMAX = 128>
__global__ void __launch_bounds__(TB, (FULL && TB * TR * 4 <= 65536) ? 8 : 1) p2_scatter_kernel(const key_t_<K64>* __restrict__ keys, Planes pl, P2Level lv) {
    constexpr int TPT = TB * TR;
    constexpr int HH = TR < 16 ? TR : 16;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint32_t* stage = reinterpret_cast<uint32_t*>(smem_raw);      // [TPT]
    static_assert(NBMAX == 128 || NBMAX == 256, "bins per level");
    __shared__ uint32_t lb[NBMAX + 1], gd[NBMAX], wtot, wbin[NBMAX / 64];
    __shared__ uint8_t tb[(TPT + 127) / 128];                   // FUSE0: the bin at every 128th staged position
    uint32_t seg, rb, nrows;
    if constexpr (FULL) {
        uint64_t b;
        if (lv.xtp && lv.xtp[8 * XTP_STRIDE]) {                  // XCD x walks its own segments
            // Which XCD this workgroup runs on is read from the hardware (the dispatcher's round-robin holds on some boxes and runs and not on
            // others: with blockIdx & 7 as the XCD, the same binary took 14.9 or 16.9 ms for h2o Q5).  The workgroup pulls the next tile
            // of ITS XCD's list from that list's queue head (one device-scope atomic); a list that has run dry sends it to the next one,
            // so every tile is taken whatever the placement of the workgroups: placement changes the speed only.
            if (threadIdx.x == 0) {
                const uint32_t me = __builtin_amdgcn_s_getreg((20) | (0 << 6) | ((4 - 1) << 11)) & 7u;       // HW_REG_XCC_ID
                uint32_t got = 0xFFFFFFFFu, gx = 0;
                for (uint32_t a = 0; a < 8 && got == 0xFFFFFFFFu; ++a) {
                    const uint32_t xx = (me + a) & 7u;
                    if (xx >= lv.nseg) continue;
                    const uint32_t total = lv.xtp[xx * XTP_STRIDE + ((lv.nseg - xx + 7) >> 3)];
                    uint32_t* head = lv.xq + xx * 32;
                    if (__hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= total) continue;
                    const uint32_t k = atomicAdd(head, 1u);
                    if (k < total) { got = k; gx = xx; }
                }
                wtot = got; lb[0] = gx;
            }
            __syncthreads();
            const uint32_t k = wtot, x = lb[0];
            __syncthreads();
            if (k == 0xFFFFFFFFu) return;
            const uint32_t* tp = lv.xtp + x * XTP_STRIDE;
            const uint32_t cnt = (lv.nseg - x + 7) >> 3;
            uint32_t lo = 0, hi = cnt;                           // largest j with tp[j] <= k
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (tp[mid] <= k) lo = mid; else hi = mid; }
            seg = x + 8 * lo;
            b = (uint64_t)lv.seg_start[seg] + (uint64_t)(k - tp[lo]) * TPT;
        } else {
        const uint32_t t = blockIdx.x;
        if (t >= lv.tile_prefix[lv.nseg]) return;
        uint32_t lo = 0, hi = lv.nseg;                           // largest segment with tile_prefix[seg] <= t
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (lv.tile_prefix[mid] <= t) lo = mid; else hi = mid; }
        seg = lo;
        b = (uint64_t)lv.seg_start[seg] + (uint64_t)(t - lv.tile_prefix[seg]) * TPT;
        }
        if (b + TPT > lv.seg_start[seg + 1]) return;             // the partial tile of the segment: the tail launch
        rb = (uint32_t)b; nrows = TPT;
    } else {
        seg = blockIdx.x;
        const uint32_t len = lv.seg_start[seg + 1] - lv.seg_start[seg];
        nrows = len % TPT;
        if (!nrows) return;
        rb = lv.seg_start[seg + 1] - nrows;
    }
    const uint32_t NB = lv.nbins;
    if (threadIdx.x <= NBMAX) lb[threadIdx.x] = 0;
    __syncthreads();
    // FUSE0 (4-byte key words; every caller's plane 0 IS the key column): the keys stay in registers from the ranking to the staging of
    // plane 0 -- COUNT the bins (non-returning LDS atomics), scan, then take every row's staged position from its bin's running cursor
    // and store the key word there.  The other form ranks rows while counting and re-reads the keys for their plane: 4 bytes per row
    // and level (h2o Q5 at 1e9 rows: 4 of a level's 28 GB).
    constexpr bool FUSE0 = !K64 && TR <= 16;
    uint32_t pos[TR];                                         // !FUSE0: (bin << 15) | rank; then the staged position
    uint32_t kw[FUSE0 ? TR : 1], dpk[FUSE0 ? (TR + 3) / 4 : 1];   // FUSE0: the key words and their bins (a byte each)
    uint32_t outside = 0;
    if constexpr (FUSE0) {
        load_rows_t<TB, FULL>(reinterpret_cast<const uint32_t*>(keys), rb, nrows, 0, kw);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < (TR + 3) / 4; ++q) dpk[q] = 0;
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            uint32_t hw;
            if constexpr (MODE == BIN_HASHED) hw = key_hash<false>(kw[r] & ~lv.kclear);
            else if constexpr (MODE == BIN_RANGED) { hw = (kw[r] & ~lv.kclear) - lv.kmin; outside |= hw > lv.xmax ? 1u : 0u; hw = hw < lv.xmax ? hw : lv.xmax; }
            else hw = kw[r] & ~lv.kclear;
            const uint32_t d = (__umulhi(hw, lv.P) >> lv.shift) & lv.mask;
            dpk[r >> 2] |= d << (8 * (r & 3));
            if (FULL || trow<TB>(r) < nrows) atomicAdd(&lb[d], 1u);
        }
        if constexpr (PACK) {     // plane 0 = the key word with the narrow value columns in its spare bits, every row verified.  Here, while the
            uint32_t bad = 0;     // positions are not live yet: behind the scan the sixteen field values spilled (0.3 extra bytes moved per byte)
#pragma unroll
            for (int r = 0; r < TR; ++r) bad |= kw[r] > pl.pk.kmax ? 1u : 0u;
            for (int f = 0; f < pl.pk.n; ++f) {
                uint32_t x[TR];
                load_rows_t<TB, FULL>(pl.pk.src[f], rb, nrows, 0, x);
#pragma unroll
                for (int r = 0; r < TR; ++r) { const uint32_t y = x[r] - pl.pk.min[f]; bad |= y > pl.pk.fmask[f] ? 1u : 0u; kw[r] |= (y & pl.pk.fmask[f]) << pl.pk.shift[f]; }
            }
            if (bad) *pl.pk.flag = 1u;                        // (rows beyond a partial tile repeat its last row: no false alarm)
        }
    } else {
#pragma unroll
        for (int h = 0; h < TR; h += HH) {
            key_t_<K64> key[HH];
            load_rows_t<TB, FULL>(keys, rb, nrows, h, key);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < HH; ++r) {
                uint32_t hw;
                if constexpr (MODE == BIN_HASHED) hw = key_hash<K64>(K64 ? key[r] : (key_t_<K64>)((uint32_t)key[r] & ~lv.kclear));
                else if constexpr (MODE == BIN_RANGED) { hw = ((uint32_t)key[r] & ~lv.kclear) - lv.kmin; outside |= hw > lv.xmax ? 1u : 0u; hw = hw < lv.xmax ? hw : lv.xmax; }
                else hw = (uint32_t)key[r];
                const uint32_t d = (__umulhi(hw, lv.P) >> lv.shift) & lv.mask;
                pos[h + r] = FULL || trow<TB>(h + r) < nrows ? (d << 15) | atomicAdd(&lb[d], 1u) : 0xFFFFFFFFu;
            }
        }
    }
    if constexpr (MODE == BIN_RANGED) { if (outside) *lv.flag = 1u; }     // (rows beyond a partial tile repeat its last row: no false alarm)
    __syncthreads();
    {   // first wavefronts: exclusive scan of the bin counts; reserve this tile's run of every bin with one atomic per bin
        uint32_t c = 0, incl = 0;
        if (threadIdx.x < NBMAX) {
            c = threadIdx.x < NB ? lb[threadIdx.x] : 0;
            incl = wave_scan_incl(c, OpAdd{}, lane_id());
            if (lane_id() == 63) wbin[wave_id()] = incl;
        }
        __syncthreads();
        if (threadIdx.x < NBMAX) {
            uint32_t excl = incl - c;
            for (int w = 0; w < wave_id(); ++w) excl += wbin[w];
            const uint32_t base = c ? atomicAdd(&lv.cursor[(size_t)seg * lv.cursor_per_seg + threadIdx.x], c) : 0;
            lb[threadIdx.x] = excl;
            gd[threadIdx.x] = base - excl;
        }
    }
    __syncthreads();
    uint32_t dlt[TR];                                         // destination row minus staged position, per output position
    if constexpr (FUSE0) {
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            if (FULL || trow<TB>(r) < nrows) {
                const uint32_t p = atomicAdd(&lb[(dpk[r >> 2] >> (8 * (r & 3))) & 0xFFu], 1u);     // the bin's cursor: exclusive start -> end
                pos[r] = p;
                stage[p] = kw[r];
            } else pos[r] = 0xFFFFFFFFu;
        }
        __syncthreads();
        // lb[d] is now the END of bin d in the staged order: the bin of an output position = the first bin that ends behind it, found
        // from the bin at the start of the position's block of 128 (tb, written by the bins themselves) in a step or two
        if (threadIdx.x < NB) {
            const uint32_t s0 = threadIdx.x ? lb[threadIdx.x - 1] : 0, e0 = lb[threadIdx.x];
            for (uint32_t blk = (s0 + 127) >> 7; (blk << 7) < e0; ++blk) tb[blk] = (uint8_t)threadIdx.x;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TR; ++i) {
            const uint32_t j = i * TB + threadIdx.x;
            uint32_t b = 0;
            if (FULL || j < nrows) { b = tb[j >> 7]; while (lb[b] <= j) ++b; }
            dlt[i] = FULL || j < nrows ? gd[b] : 0;
        }
        if (pl.p[0].dst) {                                     // (null: the key plane only ranks the rows -- nobody reads it behind this level)
            const Plane& Q = pl.p[0];
            uint32_t* dst = Q.dst + Q.dst_off_dw;
            const uint32_t dstride = (uint32_t)Q.dst_stride_dw;
#pragma unroll
            for (int i = 0; i < TR; ++i) {
                const uint32_t j = i * TB + threadIdx.x;
                if (FULL || j < nrows) dst[(size_t)(j + dlt[i]) * dstride] = stage[j];
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            if (FULL || pos[r] != 0xFFFFFFFFu) {
                const uint32_t d = pos[r] >> 15, p = lb[d] + (pos[r] & 0x7FFFu);
                pos[r] = p;
                stage[p] = d;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TR; ++i) { const uint32_t j = i * TB + threadIdx.x; dlt[i] = FULL || j < nrows ? gd[stage[j]] : 0; }
    }
#pragma nounroll
    for (int ci = FUSE0 ? 1 : 0; ci < pl.n; ++ci) {
        const Plane& Q = pl.p[ci];
        __syncthreads();                       // the previous plane (or the bin ids) has left `stage`
#pragma unroll
        for (int h = 0; h < TR; h += HH) {
            uint32_t v[HH];
            if (Q.kind == PL_ROWIDX) {
#pragma unroll
                for (int r = 0; r < HH; ++r) v[r] = rb + trow<TB>(h + r);
            } else if (Q.src_stride_dw == 1) {
                load_rows_t<TB, FULL>(Q.src, rb, nrows, h, v);
            } else {                                   // one dword of every element of a wider record (halves of 8-byte columns, fields of AoS records)
                const uint32_t* tp = Q.src + (size_t)Q.src_stride_dw * rb + Q.src_off_dw;
#pragma unroll
                for (int r = 0; r < HH; ++r) { const uint32_t o = trow<TB>(h + r); v[r] = tp[(size_t)Q.src_stride_dw * (FULL || o < nrows ? o : nrows - 1)]; }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < HH; ++r) if (FULL || pos[h + r] != 0xFFFFFFFFu) stage[pos[h + r]] = v[r];
        }
        __syncthreads();
        uint32_t* dst = Q.dst + Q.dst_off_dw;
        const uint32_t dstride = (uint32_t)Q.dst_stride_dw;
#pragma unroll
        for (int i = 0; i < TR; ++i) {
            const uint32_t j = i * TB + threadIdx.x;
            if (FULL || j < nrows) dst[(size_t)(j + dlt[i]) * dstride] = stage[j];
        }
    }
}

__global__ void __launch_bounds__(256) pn_gather_strided_kernel(const uint32_t* __restrict__ src, uint32_t stride, uint32_t count, uint32_t* __restrict__ dst) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < count; i += gridDim.x * 256) dst[i] = src[(size_t)i * stride];
}
// tile_prefix[s] = number of tiles of the segments before s; segment s = rows [seg_start[s], seg_start[s + 1])
__global__ void __launch_bounds__(1024) pn_tiles_kernel(const uint32_t* __restrict__ seg_start, uint32_t nseg, uint32_t tile_rows, uint32_t* __restrict__ tile_prefix) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base <= nseg; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nseg ? (uint32_t)(((uint64_t)(seg_start[i + 1] - seg_start[i]) + tile_rows - 1) / tile_rows) : 0;
        const uint32_t incl = wave_scan_incl(v, OpAdd{}, lane_id());
        if (lane_id() == 63) wsum[wave_id()] = incl;
        __syncthreads();
        uint32_t wbase = carry;
        for (int w = 0; w < wave_id(); ++w) wbase += wsum[w];
        if (i <= nseg) tile_prefix[i] = wbase + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = wbase + incl;
        __syncthreads();
    }
}
// bin counts of one level: a tile lies inside ONE segment, so its counts go to cnt[seg * nbins + bin] (LDS histogram, one atomic per bin)
// HASHED = false: the key is a row id and the bin ORDER-PRESERVING, f = umulhi(row, lv.P) with lv.P = floor(partitions * 2^32 / rows)
template <int TB, int TR, bool HASHED>
__global__ void __launch_bounds__(TB) pn_level_hist_kernel(const uint32_t* __restrict__ keys, P2Level lv, uint32_t* __restrict__ cnt) {
    constexpr uint32_t TPT = TB * TR;
    __shared__ uint32_t h[128];
    const uint32_t t = blockIdx.x;
    if (t >= lv.tile_prefix[lv.nseg]) return;
    uint32_t lo = 0, hi = lv.nseg;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (lv.tile_prefix[mid] <= t) lo = mid; else hi = mid; }
    const uint32_t seg = lo;
    const uint64_t b = (uint64_t)lv.seg_start[seg] + (uint64_t)(t - lv.tile_prefix[seg]) * TPT;
    const uint32_t e = lv.seg_start[seg + 1];
    const uint32_t nrows = b + TPT > e ? (uint32_t)(e - b) : TPT;
    if (threadIdx.x < 128) h[threadIdx.x] = 0;
    __syncthreads();
    {   // the tile's TR rows of a lane loaded together (a row at a time: TR memory latencies per tile)
        static_assert(TR % 4 == 0, "whole groups of four rows");
        uint32_t key[TR];
        if (nrows == TPT) load_rows_t<TB, true>(keys, (size_t)b, nrows, 0, key); else load_rows_t<TB, false>(keys, (size_t)b, nrows, 0, key);
#pragma unroll
        for (int r = 0; r < TR; ++r)
            if (trow<TB>(r) < nrows) atomicAdd(&h[(__umulhi(HASHED ? key_hash<false>(key[r]) : key[r], lv.P) >> lv.shift) & lv.mask], 1u);
    }
    __syncthreads();
    if (threadIdx.x < lv.nbins && h[threadIdx.x]) atomicAdd(&cnt[(size_t)seg * lv.nbins + threadIdx.x], h[threadIdx.x]);
}

// the two kernels of one combination {key word, bin mode, packing, bins}
template <bool K64, int MODE, bool PACK, int NBMAX>
int scatter_pair(aqg_ctx* ctx, const void* keys, const Planes& pl, const P2Level& lv, unsigned tiles, unsigned tails) {
    const size_t lds = (size_t)P2_PT * 4;
    const key_t_<K64>* k = static_cast<const key_t_<K64>*>(keys);
    AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(&p2_scatter_kernel<P2_TB, P2_TR, K64, true, MODE, PACK, NBMAX>), lds));
    AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(&p2_scatter_kernel<P2_TB, P2_TR, K64, false, MODE, PACK, NBMAX>), lds));
    hipLaunchKernelGGL((p2_scatter_kernel<P2_TB, P2_TR, K64, true, MODE, PACK, NBMAX>), dim3(tiles), dim3(P2_TB), lds, ctx->stream, k, pl, lv);
    hipLaunchKernelGGL((p2_scatter_kernel<P2_TB, P2_TR, K64, false, MODE, PACK, NBMAX>), dim3(tails), dim3(P2_TB), lds, ctx->stream, k, pl, lv);
    return AQG_OK;
}

} // namespace

void aqg_widen_column(aqg_ctx* ctx, const void* col, int esz, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(p1_widen_kernel, dim3(aqg_grid(ctx, n, 256, 4, 16)), dim3(256), 0, ctx->stream, col, esz, n, out);
}

// every combination that exists: 8-byte key words are hashed and never packed; 256 bins are the one-level range plan's
int aqg_scatter_pair(aqg_ctx* ctx, int kbytes, int mode, bool pack, int nbmax, const void* keys, const Planes& pl, const P2Level& lv, unsigned tiles, unsigned tails) {
    const int combo = kbytes << 16 | nbmax << 4 | mode << 1 | (pack ? 1 : 0);
    auto is = [](int kb, int nb, int m, bool pk) { return kb << 16 | nb << 4 | m << 1 | (pk ? 1 : 0); };
    if (combo == is(8, 128, BIN_HASHED, false)) return scatter_pair<true, BIN_HASHED, false, 128>(ctx, keys, pl, lv, tiles, tails);
    if (combo == is(4, 128, BIN_RAW, false)) return scatter_pair<false, BIN_RAW, false, 128>(ctx, keys, pl, lv, tiles, tails);
    if (combo == is(4, 128, BIN_RAW, true)) return scatter_pair<false, BIN_RAW, true, 128>(ctx, keys, pl, lv, tiles, tails);
    if (combo == is(4, 128, BIN_HASHED, false)) return scatter_pair<false, BIN_HASHED, false, 128>(ctx, keys, pl, lv, tiles, tails);
    if (combo == is(4, 128, BIN_HASHED, true)) return scatter_pair<false, BIN_HASHED, true, 128>(ctx, keys, pl, lv, tiles, tails);
    if (combo == is(4, 128, BIN_RANGED, false)) return scatter_pair<false, BIN_RANGED, false, 128>(ctx, keys, pl, lv, tiles, tails);
    if (combo == is(4, 128, BIN_RANGED, true)) return scatter_pair<false, BIN_RANGED, true, 128>(ctx, keys, pl, lv, tiles, tails);
    if (combo == is(4, 256, BIN_RANGED, false)) return scatter_pair<false, BIN_RANGED, false, 256>(ctx, keys, pl, lv, tiles, tails);
    if (combo == is(4, 256, BIN_RANGED, true)) return scatter_pair<false, BIN_RANGED, true, 256>(ctx, keys, pl, lv, tiles, tails);
    return AQG_ERR_ARG;
}

int aqg_scatter_level_counted(aqg_ctx* ctx, const LevelBufs& b, int mode, bool counted, const uint32_t* keys, const Planes& pl, uint32_t n, uint32_t nseg,
                              uint32_t P, uint32_t shift, uint32_t mask, uint32_t nb, const char* what) {
    const unsigned tiles = (unsigned)((uint64_t)n / P2_PT) + nseg + 1;
    hipLaunchKernelGGL(pn_tiles_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)b.seg, nseg, (uint32_t)P2_PT, b.tp);
    P2Level lv{b.seg, b.tp, b.cur, nseg, P, shift, mask, nb, nb};
    if (!counted) {
        AQG_HIP(ctx, hipMemsetAsync(b.cnt, 0, ((size_t)nseg * nb + 1) * 4, ctx->stream));
        if (mode == BIN_HASHED) hipLaunchKernelGGL((pn_level_hist_kernel<P2_TB, P2_TR, true>), dim3(tiles), dim3(P2_TB), 0, ctx->stream, keys, lv, b.cnt);
        else hipLaunchKernelGGL((pn_level_hist_kernel<P2_TB, P2_TR, false>), dim3(tiles), dim3(P2_TB), 0, ctx->stream, keys, lv, b.cnt);
    }
    AQG_TRY(aqg_exclusive_scan_u32(ctx, b.cnt, (uint64_t)nseg * nb + 1, b.bsum));        // cnt[i] = start of (segment, bin) i; the last word = n
    AQG_HIP(ctx, hipMemcpyAsync(b.cur, b.cnt, (size_t)nseg * nb * 4, hipMemcpyDeviceToDevice, ctx->stream));
    AQG_TRY(aqg_scatter_pair(ctx, 4, mode, false, 128, keys, pl, lv, tiles, nseg));
    AQG_TRY(aqg_check_launch(ctx, what));
    // the bins of this level are the segments of the next (and, after the last level, the partitions)
    AQG_HIP(ctx, hipMemcpyAsync(b.seg, b.cnt, ((size_t)nseg * nb + 1) * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return AQG_OK;
}

int aqg_scatter_level_offsets(aqg_ctx* ctx, const LevelBufs& b, const uint32_t* pstart, bool pack, uint32_t kclear, const uint32_t* keys, const Planes& pl,
                              uint32_t n, uint32_t nseg, uint32_t P, uint32_t shift, uint32_t nb, const char* what) {
    hipLaunchKernelGGL(pn_gather_strided_kernel, dim3(aqg_grid(ctx, (uint64_t)nseg + 1, 256, 1, 4)), dim3(256), 0, ctx->stream, pstart, nb << shift, nseg + 1, b.seg);
    hipLaunchKernelGGL(pn_gather_strided_kernel, dim3(aqg_grid(ctx, (uint64_t)nseg * nb, 256, 1, 4)), dim3(256), 0, ctx->stream, pstart, 1u << shift, nseg * nb, b.cur);
    hipLaunchKernelGGL(pn_tiles_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)b.seg, nseg, (uint32_t)P2_PT, b.tp);
    P2Level lv{b.seg, b.tp, b.cur, nseg, P, shift, nb - 1, nb, nb, kclear};
    const unsigned tiles = (unsigned)((uint64_t)n / P2_PT) + nseg + 1;
    AQG_TRY(aqg_scatter_pair(ctx, 4, BIN_RAW, pack, 128, keys, pl, lv, tiles, nseg));
    return aqg_check_launch(ctx, what);
}

int aqg_scatter_column_bins(aqg_ctx* ctx, int kbytes, bool ranged, const void* keys, uint32_t n, uint32_t P, uint32_t scale, uint32_t kmin, uint32_t xmax,
                            unsigned xgrid, ColumnBins* c) {
    AQG_TRY(aqg_ws_get(ctx, (size_t)P, &c->ftot));
    AQG_TRY(aqg_ws_get(ctx, (size_t)P + 1, &c->fstart));
    AQG_TRY(aqg_ws_get(ctx, (size_t)P, &c->cur2));
    AQG_TRY(aqg_ws_get(ctx, 2, &c->seg1));
    AQG_TRY(aqg_ws_get(ctx, 2, &c->tp1));
    AQG_TRY(aqg_ws_get(ctx, 64, &c->cur1));
    AQG_TRY(aqg_ws_get(ctx, 65, &c->seg2));
    AQG_TRY(aqg_ws_get(ctx, 65, &c->tp2));
    c->xtp = nullptr;
    if (xgrid) AQG_TRY(aqg_ws_get(ctx, 8 * XTP_STRIDE + 32 + 8 * 32, &c->xtp));     // tile prefixes per XCD | flag | eight queue heads on lines of their own
    AQG_HIP(ctx, hipMemsetAsync(c->ftot, 0, (size_t)P * 4, ctx->stream));
    const unsigned hgrid = aqg_grid(ctx, n, 1024, HB, 4);
    if (ranged && kbytes != 4) return AQG_ERR_ARG;                                   // (8-byte key words are hashed)
    if (ranged) hipLaunchKernelGGL((p2_hist_kernel<false, true>), dim3(hgrid), dim3(1024), (size_t)P * 4, ctx->stream, static_cast<const uint32_t*>(keys), n, scale, c->ftot, kmin, xmax);
    else if (kbytes == 4) hipLaunchKernelGGL((p2_hist_kernel<false>), dim3(hgrid), dim3(1024), (size_t)P * 4, ctx->stream, static_cast<const uint32_t*>(keys), n, P, c->ftot);
    else hipLaunchKernelGGL((p2_hist_kernel<true>), dim3(hgrid), dim3(1024), (size_t)P * 4, ctx->stream, static_cast<const uint64_t*>(keys), n, P, c->ftot);
    hipLaunchKernelGGL(p2_setup_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const uint32_t*)c->ftot, P, n, (uint32_t)P2_PT, c->fstart, c->cur2, c->seg1, c->tp1, c->cur1, c->seg2, c->tp2, c->xtp, (uint32_t)xgrid);
    return AQG_OK;
}
