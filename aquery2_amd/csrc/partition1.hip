// partition1.hip -- high-cardinality group-by in ONE partition level (h2o Q3 / Q5 / Q7 at 1e7 groups): replaces AQHashTable's
// robin-hood build (reference server/hasher.h:146-199, server/unordered_dense.h:1117-1147) and the generated per-group loop
// (engine/ast.py:722-789) where the groups do not fit one workgroup's LDS.
//
// Round 1 partitioned {key, row id, values} in two MSD levels of <= 8 bits: every level reads and writes all planes, ~100 B
// moved per row for 16 algorithmic (h2o Q5).  This plan moves them ONCE:
//   p1_hist     one workgroup per CHUNK of rows (a multiple of the 32768-row tile): bin counts of the chunk, [bin][chunk]
//   scan        exclusive scan of that matrix = start of every (bin, chunk) run
//   p1_scatter  one workgroup per chunk walks its tiles carrying the running bin cursors in LDS: rows are ranked inside their
//               bins with returning LDS atomics, each dword plane is staged bin-major in LDS (128 KB) and streamed out, so a
//               tile writes one run per bin and plane and consecutive tiles of a chunk continue each other's runs
//   p1_agg      one 1024-thread workgroup per partition: open-addressing KEY table {key, dense id} at a low load factor and
//               DENSE accumulator arrays indexed by the id -- the accumulators (28 B per group for Q5) are not multiplied by the
//               table's slack, which is what lets a partition hold ~3700 groups in 150 KB and 1e7 groups fit ~2900 bins
// Up to MAXBINS bins (LDS of the scatter: 128 KB of staging + 8 B per bin).  More groups than that: partition.hip (two levels).
// The range plan of <= 256 bins and the two-level plan (aqg_partition2_aggregate) move the rows with the tile scatter of tile_scatter.hip.
#include "partition1_int.hpp"
#include "dense.hpp"
#include "tile_scatter.hpp"

namespace {

constexpr int SR = 32;            // rows per thread and tile
constexpr int PT = SB * SR;       // rows per tile: 32768 (one staged dword plane = 128 KB)


// A lane owns SR / 4 groups of FOUR consecutive rows of a tile (one 16-byte load per 4-byte column and group).
__device__ inline uint32_t tile_row(int r) { return (uint32_t)(r >> 2) * (SB * 4) + threadIdx.x * 4 + (r & 3); }
// Loader of one BATCH of R rows of a lane: rows r0 .. r0 + R - 1 of the lane's SR rows of the tile.
// FULL: the tile has all its rows (every tile but the last one of the input): vector loads, no bounds.  Otherwise row by row
// with a clamped index (every load is issued, none sits behind a branch; the caller masks rows >= nrows).
template <bool FULL, class T, int R> __device__ inline void load_rows(const T* __restrict__ p, size_t tile_first, uint32_t nrows, int r0, T (&t)[R]) {
    const T* tp = p + tile_first;
    if constexpr (FULL) {
#pragma unroll
        for (int c = 0; c < R / 4; ++c) __builtin_memcpy(&t[4 * c], tp + tile_row(r0 + 4 * c), 4 * sizeof(T));
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) { const uint32_t o = tile_row(r0 + r); t[r] = tp[o < nrows ? o : nrows - 1]; }
    }
}

// Chunks of whole tiles cover rows [0, nfull); the rows behind the last whole tile, if any, are one more chunk (the TAIL chunk,
// index nchunks - 1), scattered by its own small kernel so that the main kernel never sees a partial tile.
struct Chunks {
    uint32_t n, nfull, chunk_rows, nchunks, nbins, has_tail;
    // range partitions (the one-level form of BIN_RANGED below): bin = umulhi(min(key - kmin, xmax), rmul); rflag is set by a key outside the sampled domain
    uint32_t ranged, kmin, xmax, rmul; uint32_t* rflag;
};
template <bool K64> __device__ inline uint32_t key_hash(key_t_<K64> k);
template <bool K64, bool RANGED> __device__ inline uint32_t p1_bin(const Chunks& ch, key_t_<K64> key, uint32_t& outside) {
    if constexpr (RANGED && !K64) {
        uint32_t x = (uint32_t)key - ch.kmin;
        outside |= x > ch.xmax ? 1u : 0u;
        x = x < ch.xmax ? x : ch.xmax;
        return __umulhi(x, ch.rmul);
    } else return __umulhi(key_hash<K64>(key), ch.nbins);
}
__device__ inline void chunk_range(const Chunks& ch, uint32_t c, uint64_t& b, uint64_t& e) {
    if (ch.has_tail && c + 1 == ch.nchunks) { b = ch.nfull; e = ch.n; return; }
    b = (uint64_t)c * ch.chunk_rows;
    e = b + ch.chunk_rows < ch.nfull ? b + ch.chunk_rows : ch.nfull;
    if (b > e) b = e;
}

// ---- key tuples of several columns -> one column of key words ---------------------------------------------------------------------
template <bool K64>
__global__ void __launch_bounds__(256) p1_pack_keys_kernel(KeySpec ks, uint32_t n, key_t_<K64>* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (key_t_<K64>)pack_key(ks, i);
}

// ---- bin counts of every chunk -----------------------------------------------------------------------------------------------
constexpr int HR = 16;   // rows per thread and step of the histogram pass
template <bool K64, bool RANGED = false>
__global__ void __launch_bounds__(SB) p1_hist_kernel(const key_t_<K64>* __restrict__ keys, Chunks ch, uint32_t* __restrict__ hist /* [bin][chunk] */) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint32_t* cnt = reinterpret_cast<uint32_t*>(smem_raw);
    for (uint32_t b = threadIdx.x; b < ch.nbins; b += SB) cnt[b] = 0;
    __syncthreads();
    uint64_t cb, ce;
    chunk_range(ch, blockIdx.x, cb, ce);
    constexpr uint64_t STEP = (uint64_t)SB * HR;
    if (!(ch.has_tail && blockIdx.x + 1 == ch.nchunks)) {     // whole tiles, so whole steps: the next step's keys in flight while this one's are counted
        key_t_<K64> cur[HR];
        if (cb < ce) load_rows<true>(keys, cb, (uint32_t)STEP, 0, cur);
        for (uint64_t rb = cb; rb < ce; rb += STEP) {
            key_t_<K64> nxt[HR];
            load_rows<true>(keys, rb + STEP < ce ? rb + STEP : rb, (uint32_t)STEP, 0, nxt);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < HR; ++r) { uint32_t o_ = 0; atomicAdd(&cnt[p1_bin<K64, RANGED>(ch, cur[r], o_)], 1u); }      // (a key outside the sampled domain: the scatter flags it)
#pragma unroll
            for (int r = 0; r < HR; ++r) cur[r] = nxt[r];
        }
    } else for (uint64_t rb = cb; rb < ce; rb += STEP) {      // the tail chunk (less than one tile)
        const uint32_t nrows = ce - rb < STEP ? (uint32_t)(ce - rb) : (uint32_t)STEP;
        key_t_<K64> key[HR];
        load_rows<false>(keys, rb, nrows, 0, key);
#pragma unroll
        for (int r = 0; r < HR; ++r)
            if (tile_row(r) < nrows) { uint32_t o_ = 0; atomicAdd(&cnt[p1_bin<K64, RANGED>(ch, key[r], o_)], 1u); }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < ch.nbins; b += SB) hist[(size_t)b * ch.nchunks + blockIdx.x] = cnt[b];
}

// ---- scatter -------------------------------------------------------------------------------------------------------------------
// One tile: rank the rows inside their bins, then stage and stream out plane after plane.  A lane's SR rows are handled in
// batches of H (all loads of a batch are issued before the first use: memory-level parallelism is what bounds these kernels,
// and 32 rows at once did not fit 128 registers); the keys are not kept: the key planes load them again (from L2).
constexpr int H = 16;
template <bool K64, bool FULL, bool RANGED = false>
__device__ inline void scatter_tile(const key_t_<K64>* __restrict__ keys, const Planes& pl, const Chunks& ch, uint64_t rb, uint32_t nrows, uint32_t* stage, uint32_t* lb, uint32_t* gd, uint32_t* wsum) {
    const uint32_t NB = ch.nbins;
    uint32_t outside = 0;
    for (uint32_t b = threadIdx.x; b <= NB; b += SB) lb[b] = 0;
    __syncthreads();
    uint32_t pos[SR];                                         // (bin << 15) | rank, later the staged position
#pragma unroll
    for (int h = 0; h < SR; h += H) {
        key_t_<K64> key[H];
        load_rows<FULL>(keys, rb, nrows, h, key);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < H; ++r) {
            const uint32_t d = p1_bin<K64, RANGED>(ch, key[r], outside);
            pos[h + r] = FULL || tile_row(h + r) < nrows ? (d << 15) | atomicAdd(&lb[d], 1u) : 0xFFFFFFFFu;
        }
    }
    if constexpr (RANGED) { if (outside) *ch.rflag = 1u; }      // (rows beyond a partial tile repeat its last row: no false alarm)
    __syncthreads();
    {   // exclusive scan of the bin counts: a thread owns bins 4 tid .. 4 tid + 3 (NB <= 4096)
        uint32_t c[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const uint32_t b = threadIdx.x * 4 + k; c[k] = b < NB ? lb[b] : 0; s += c[k]; }
        const uint32_t incl = wave_scan_incl(s, OpAdd{}, lane_id());
        if (lane_id() == 63) wsum[wave_id()] = incl;
        __syncthreads();
        uint32_t base = incl - s;
        for (int w = 0; w < wave_id(); ++w) base += wsum[w];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t b = threadIdx.x * 4 + k;
            if (b < NB) { lb[b] = base; gd[b] -= base; }
            base += c[k];
        }
        if (threadIdx.x == SB - 1) lb[NB] = base;             // == nrows
    }
    __syncthreads();
    // staged position of every row (two 15-bit positions per register); the bin of every staged position goes through the
    // stage buffer to the lane that will stream that position out (two 12-bit bin ids per register): the destination of
    // staged position j is j + gd[bin(j)]
    uint32_t ppos[SR / 2];
#pragma unroll
    for (int r = 0; r < SR; ++r) {
        uint32_t p = 0;
        if (FULL || pos[r] != 0xFFFFFFFFu) {
            const uint32_t d = pos[r] >> 15;
            p = lb[d] + (pos[r] & 0x7FFFu);
            stage[p] = d;
        }
        if (r & 1) ppos[r >> 1] |= p << 16; else ppos[r >> 1] = p;
    }
    __syncthreads();
    uint32_t pbin[SR / 2];
#pragma unroll
    for (int i = 0; i < SR; ++i) {
        const uint32_t j = i * SB + threadIdx.x;
        const uint32_t d = FULL || j < nrows ? stage[j] : 0;
        if (i & 1) pbin[i >> 1] |= d << 16; else pbin[i >> 1] = d;
    }
#pragma nounroll
    for (int ci = 0; ci < pl.n; ++ci) {
        const Plane& P = pl.p[ci];
        __syncthreads();                       // the previous plane (or the bin ids) has left `stage`
#pragma unroll
        for (int h = 0; h < SR; h += H) {
            uint32_t v[H];
            if (P.kind == PL_ROWIDX) {
#pragma unroll
                for (int r = 0; r < H; ++r) v[r] = (uint32_t)rb + tile_row(h + r);
            } else if (P.kind == PL_PACK) {            // the key word with the narrow value columns in its spare bits, every row verified (PackSpec)
                load_rows<FULL>(P.src, rb, nrows, h, v);
                uint32_t bad = 0;
#pragma unroll
                for (int r = 0; r < H; ++r) bad |= v[r] > pl.pk.kmax ? 1u : 0u;
                for (int f = 0; f < pl.pk.n; ++f) {
                    uint32_t x[H];
                    load_rows<FULL>(pl.pk.src[f], rb, nrows, h, x);
#pragma unroll
                    for (int r = 0; r < H; ++r) { const uint32_t y = x[r] - pl.pk.min[f]; bad |= y > pl.pk.fmask[f] ? 1u : 0u; v[r] |= (y & pl.pk.fmask[f]) << pl.pk.shift[f]; }
                }
                if (bad) *pl.pk.flag = 1u;             // (rows beyond a partial tile repeat its last row: no false alarm)
            } else if (P.src_stride_dw == 1) {
                load_rows<FULL>(P.src, rb, nrows, h, v);
            } else {                                   // one half of every element of an 8-byte column
                const uint32_t* tp = P.src + 2 * rb + P.src_off_dw;
#pragma unroll
                for (int r = 0; r < H; ++r) { const uint32_t o = tile_row(h + r); v[r] = tp[2 * (size_t)(FULL || o < nrows ? o : nrows - 1)]; }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < H; ++r) if (FULL || tile_row(h + r) < nrows) stage[(ppos[(h + r) >> 1] >> (((h + r) & 1) * 16)) & 0xFFFFu] = v[r];
        }
        __syncthreads();
        uint32_t* dst = P.dst + P.dst_off_dw;
        const uint32_t dstride = (uint32_t)P.dst_stride_dw;
#pragma unroll
        for (int i = 0; i < SR; ++i) {
            const uint32_t j = i * SB + threadIdx.x;
            if (FULL || j < nrows) dst[(size_t)(j + gd[(pbin[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu]) * dstride] = stage[j];
        }
    }
    __syncthreads();
    // cursors for the next tile: cursor + count = (cursor - lb[b]) + lb[b + 1]
    for (uint32_t b = threadIdx.x; b < NB; b += SB) gd[b] += lb[b + 1];
    __syncthreads();
}

template <bool K64, bool RANGED = false>
__global__ void __launch_bounds__(SB) p1_scatter_kernel(const key_t_<K64>* __restrict__ keys, Planes pl, Chunks ch, const uint32_t* __restrict__ hist_scanned) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint32_t* stage = reinterpret_cast<uint32_t*>(smem_raw);      // [PT] one plane of the tile, bin-major
    uint32_t* lb = stage + PT;                                    // [nbins + 1] counts, then first staged position of every bin
    uint32_t* gd = lb + (ch.nbins + 1);                           // [nbins] between tiles: global cursor; inside: cursor - lb
    __shared__ uint32_t wsum[SB / 64];
    const uint32_t NB = ch.nbins;
    uint64_t cb, ce;
    chunk_range(ch, blockIdx.x, cb, ce);
    for (uint32_t b = threadIdx.x; b < NB; b += SB) gd[b] = hist_scanned[(size_t)b * ch.nchunks + blockIdx.x];
    for (uint64_t rb = cb; rb + PT <= ce; rb += PT) scatter_tile<K64, true, RANGED>(keys, pl, ch, rb, PT, stage, lb, gd, wsum);
}
// the tail chunk: fewer rows than a tile (one workgroup, once per call)
template <bool K64, bool RANGED = false>
__global__ void __launch_bounds__(SB) p1_scatter_tail_kernel(const key_t_<K64>* __restrict__ keys, Planes pl, Chunks ch, const uint32_t* __restrict__ hist_scanned) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint32_t* stage = reinterpret_cast<uint32_t*>(smem_raw);
    uint32_t* lb = stage + PT;
    uint32_t* gd = lb + (ch.nbins + 1);
    __shared__ uint32_t wsum[SB / 64];
    const uint32_t NB = ch.nbins, c = ch.nchunks - 1;
    for (uint32_t b = threadIdx.x; b < NB; b += SB) gd[b] = hist_scanned[(size_t)b * ch.nchunks + c];
    scatter_tile<K64, false, RANGED>(keys, pl, ch, ch.nfull, ch.n - ch.nfull, stage, lb, gd, wsum);
}

} // namespace

static void p1_geometry(const aqg_ctx* ctx, uint32_t n, Chunks* ch) {
    const uint64_t tiles = (uint64_t)n / PT;                                 // whole tiles
    const uint64_t target = (uint64_t)ctx->num_cu * 4;                       // chunks: four rounds of one workgroup per CU
    uint64_t tiles_per_chunk = (tiles + target - 1) / target;
    if (tiles_per_chunk < 1) tiles_per_chunk = 1;
    ch->n = n;
    ch->nfull = (uint32_t)(tiles * PT);
    ch->has_tail = ch->nfull != n;
    ch->chunk_rows = (uint32_t)(tiles_per_chunk * PT);
    ch->nchunks = (uint32_t)((tiles + tiles_per_chunk - 1) / tiles_per_chunk) + ch->has_tail;
    ch->nbins = 0;
}

static bool p1_key_is_column(const KeySpec& ks, int ksz) { return ks.nkeys == 1 && (int)aqg_dtype_size(ks.dt[0]) == ksz; }

// which value columns travel inside the key word (PackSpec): one 4-byte integer key column whose sampled maximum leaves spare bits, 4-byte
// integer value columns whose sampled range fits them (at most two), every accumulator over such a column a plain sum / min / max / square
static int plan_pack(aqg_ctx* ctx, const KeySpec& ks, const AccSpec& as, uint32_t n, const ValCols& vc, PackPlan* pp) {
    memset(pp, 0, sizeof *pp);
    if (n < (1u << 22) || !p1_key_is_column(ks, 4) || !(ks.dt[0] == AQG_INT32 || ks.dt[0] == AQG_UINT32)) return AQG_OK;
    KeySpec probe;
    memset(&probe, 0, sizeof probe);
    probe.nkeys = 1; probe.dt[0] = ks.dt[0]; probe.col[0] = ks.col[0];
    int cand[MAXACC], nc = 0;
    for (int u = 0; u < vc.n && probe.nkeys < MAXKEYS; ++u) {
        if (!(vc.dt[u] == AQG_INT32 || vc.dt[u] == AQG_UINT32)) continue;
        bool ok = true;
        for (int a = 0; a < as.nacc; ++a) if (as.col[a] == vc.col[u] && as.dt[a] != AQG_NONE) ok = ok && as.part[a] == 0 && (as.kind[a] == ACC_ADD_I || as.kind[a] == ACC_MIN || as.kind[a] == ACC_MAX);
        if (!ok) continue;
        probe.dt[probe.nkeys] = vc.dt[u]; probe.col[probe.nkeys] = vc.col[u]; ++probe.nkeys;
        cand[nc++] = u;
    }
    long long mins[MAXKEYS], maxs[MAXKEYS];
    bool ok = false;
    AQG_TRY(aqg_key_ranges(ctx, probe, 1u << 20, mins, maxs, &ok, n));       // (a sample spread over the column: every row is verified while it is packed / binned)
    if (!ok) return AQG_OK;
    if (ks.range_known) { mins[0] = ks.range_lo; maxs[0] = ks.range_hi; }     // (the key's range as the caller knows it; the value columns' from the sample)
    pp->have_range = true; pp->key_lo = mins[0]; pp->key_hi = maxs[0]; pp->exact = ks.range_known != 0;
    if (!nc || mins[0] < 0 || maxs[0] >= (1ll << 31)) return AQG_OK;
    auto bits_of = [](unsigned long long v) { int b = 0; while (b < 33 && (1ull << b) <= v) ++b; return b; };
    int used = bits_of((unsigned long long)maxs[0]);
    if (used < 1) used = 1;
    pp->kmax = (uint32_t)((1ull << used) - 1);
    for (int i = 0; i < nc && pp->n < 2; ++i) {
        const unsigned long long range = (unsigned long long)(maxs[1 + i] - mins[1 + i]);
        const int fb = bits_of(range) < 1 ? 1 : bits_of(range);
        if (used + fb > 32) continue;
        const int f = pp->n++;
        pp->col[f] = vc.col[cand[i]]; pp->min[f] = (uint32_t)(long long)mins[1 + i]; pp->shift[f] = (uint32_t)used; pp->fmask[f] = (uint32_t)((1ull << fb) - 1);
        pp->kclear |= pp->fmask[f] << used;
        used += fb;
    }
    return AQG_OK;
}
// Range partitions over a dense key domain (p1_agg_direct_kernel): the sampled domain [key_lo, key_hi] cut into P pieces of at most W key
// values, P a multiple of 64 within the two-level plan's limits.  The slack on both ends (a sample of the first 2^20 rows rarely sees the
// extremes of the column) costs nothing: empty pieces of the domain are empty partitions.

// the direct-indexed aggregation over range partitions (p1_agg_direct_kernel)
static void plan_range(const PackPlan& pp, const AccSpec& as, int need_count, uint32_t parts_hashed, RangePlan* rp) {
    memset(rp, 0, sizeof *rp);
    if (aqg_switches().disable_ranged || !pp.have_range || pp.key_hi < pp.key_lo) return;
    const long long span = pp.key_hi - pp.key_lo + 1, slack = pp.exact ? 0 : span / 64 + 1024;
    // (the key column is int32 or uint32: its values as 64-bit integers; the bins work on the 32-bit difference to kmin, which wraps correctly)
    const long long lo = pp.key_lo - slack, hi = pp.key_hi + slack;
    const unsigned long long D = (unsigned long long)(hi - lo + 1);
    if (D >= (1ull << 32)) return;
    const uint32_t W = p1_direct_capacity(as, need_count);
    if (W < 64) return;
    uint64_t P = (D + (W - 4) - 1) / (W - 4);
    if (P < 256) P = 256;                                                     // every CU gets a partition
    P = (P + 63) & ~63ull;
    for (; P <= AQG_P2_MAXPARTS; P += 64) {
        if (D <= 8 * P) return;                                               // (a domain this small is not this plan's business)
        const uint64_t M = (P << 32) / D;                                     // umulhi(x, M) < P for every x < D
        if (M < 1 || M >= (1ull << 32)) return;
        if ((1ull << 32) / M + 2 <= W) { rp->on = true; rp->kmin = (uint32_t)lo; rp->D = (uint32_t)D; rp->P = (uint32_t)P; rp->M = (uint32_t)M; rp->W = W; return; }
    }
    (void)parts_hashed;
}

// The key as ONE column of 4- or 8-byte words (the user's column, or the packed tuple), the value columns as dword sources (1- / 2-byte ones
// widened), and `nsets` sets of partitioned buffers {keys, rows, values}: one for the one-level plan, A and B for the two levels
struct PartBufs { const void* keycol; const void* vsrc[MAXACC]; void *keys[2], *rows[2], *vals[2][MAXACC]; };
static int p1_buffers(aqg_ctx* ctx, const KeySpec& ks, int ksz, uint32_t n, const ValCols& vc, const PackPlan& pp, int nsets, PartBufs* b) {
    b->keycol = ks.col[0];
    if (!p1_key_is_column(ks, ksz)) {
        void* packed;
        AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * ksz, &packed));
        const unsigned g = aqg_grid(ctx, n, 256, 4, 16);
        if (ksz == 4) hipLaunchKernelGGL(p1_pack_keys_kernel<false>, dim3(g), dim3(256), 0, ctx->stream, ks, n, static_cast<uint32_t*>(packed));
        else hipLaunchKernelGGL(p1_pack_keys_kernel<true>, dim3(g), dim3(256), 0, ctx->stream, ks, n, static_cast<uint64_t*>(packed));
        b->keycol = packed;
    }
    for (int s = 0; s < nsets; ++s) {
        AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * ksz, &b->keys[s]));
        AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * 4, &b->rows[s]));
    }
    for (int u = 0; u < vc.n; ++u) {
        b->vals[0][u] = b->vals[1][u] = nullptr; b->vsrc[u] = nullptr;
        if (pack_field_of(pp, vc.col[u]) >= 0) continue;                     // travels in the key word
        for (int s = 0; s < nsets; ++s) AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * part_val_bytes(vc.dt[u]), &b->vals[s][u]));
        b->vsrc[u] = vc.col[u];
        const int esz = (int)aqg_dtype_size(vc.dt[u]);
        if (esz < 4) {                                                       // 1- / 2-byte values travel as dwords
            void* wide;
            AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * 4, &wide));
            aqg_widen_column(ctx, vc.col[u], esz, n, static_cast<uint32_t*>(wide));
            b->vsrc[u] = wide;
        }
    }
    return AQG_OK;
}
// the planes of one pass: the first takes the user's columns to set 0 (the key word with the packed fields, the row ids made from the row index),
// the second set 0 to set 1
static Planes p1_planes(const PartBufs& b, int ksz, const ValCols& vc, const PackPlan& pp, uint32_t* flag, bool level1) {
    Planes pl;
    memset(&pl, 0, sizeof pl);
    const void* ksrc = level1 ? b.keycol : b.keys[0];
    void* kdst = level1 ? b.keys[0] : b.keys[1];
    if (ksz == 4 && pp.n && level1) {
        pl.add(PL_PACK, ksrc, 1, 0, kdst, 1, 0);
        pl.pk.n = pp.n; pl.pk.kmax = pp.kmax; pl.pk.flag = flag;
        for (int f = 0; f < pp.n; ++f) { pl.pk.src[f] = static_cast<const uint32_t*>(pp.col[f]); pl.pk.min[f] = pp.min[f]; pl.pk.shift[f] = pp.shift[f]; pl.pk.fmask[f] = pp.fmask[f]; }
    }
    else pl.add_column(ksrc, kdst, ksz);
    if (level1) pl.add(PL_ROWIDX, nullptr, 0, 0, b.rows[0], 1, 0); else pl.add(PL_LOAD, b.rows[0], 1, 0, b.rows[1], 1, 0);
    for (int u = 0; u < vc.n; ++u) {
        if (!b.vals[0][u]) continue;                                         // (packed)
        pl.add_column(level1 ? b.vsrc[u] : b.vals[0][u], level1 ? b.vals[0][u] : b.vals[1][u], (int)part_val_bytes(vc.dt[u]));
    }
    return pl;
}
size_t aqg_partition1_ws_bytes(const aqg_ctx* ctx, const KeySpec& ks, uint32_t n, const AccSpec& as, uint32_t nbins) {
    const int ksz = ks.total_bytes <= 4 ? 4 : 8;
    ValCols vc;
    p1_val_cols(as, &vc);
    size_t per_row = (size_t)ksz + 4;
    if (!p1_key_is_column(ks, ksz)) per_row += ksz;                          // the packed key column
    for (int u = 0; u < vc.n; ++u) per_row += part_val_bytes(vc.dt[u]) + (aqg_dtype_size(vc.dt[u]) < 4 ? 4 : 0);   // + the widened copy
    Chunks ch;
    p1_geometry(ctx, n, &ch);
    const size_t hcount = (size_t)nbins * ch.nchunks;
    return ((size_t)n + 64) * per_row + 256 * (4 + 2 * MAXACC) + hcount * 4 + (hcount / 2048 + 64) * 4 + 65536;
}

// Partitioned aggregation of (ks, as) over n rows into the compact record table `out` (AoS records, `out_cap` slots,
// flags[1] = number of groups written, flags[0] = overflow).  Needs packed (<= 8 byte) keys and nbins from aqg_partition1_bins.
int aqg_partition1_aggregate(aqg_ctx* ctx, const KeySpec& ks, const AccSpec& as, uint32_t n, uint32_t nbins, int need_count, GTable out, uint32_t out_cap, PartRows* pr, int layout, int* ranged) {
    if (nbins < 1 || nbins > AQG_P1_MAXBINS) return aqg_fail(ctx, AQG_ERR_OVERFLOW, "one-level partitioned group-by: 1..3584 bins");
    const int ksz = ks.total_bytes <= 4 ? 4 : 8;
    ValCols vc;
    p1_val_cols(as, &vc);
    // a dense 4-byte key domain: range partitions and the direct-indexed aggregation, as in the two-level plan (no more bins than the
    // hashed plan was given: the workspace is sized by them)
    RangePlan rp;
    PackPlan pp;
    memset(&rp, 0, sizeof rp);
    memset(&pp, 0, sizeof pp);
    if (ranged && *ranged && !pr) {
        AQG_TRY(plan_pack(ctx, ks, as, n, vc, &pp));          // narrow value columns inside the key word, and the sample of the key range
        plan_range(pp, as, need_count, nbins, &rp);
        if (rp.on && rp.P > nbins) rp.on = false;
    }
    if (ranged) *ranged = (rp.on ? 2 : 0) | (pp.n ? 1 : 0);
    if (rp.on) nbins = rp.P;
    Chunks ch;
    p1_geometry(ctx, n, &ch);
    ch.nbins = nbins;
    ch.ranged = rp.on ? 1u : 0u; ch.kmin = rp.kmin; ch.xmax = rp.on ? rp.D - 1 : 0u; ch.rmul = rp.M; ch.rflag = out.flags + 6;

    PartBufs b;
    AQG_TRY(p1_buffers(ctx, ks, ksz, n, vc, pp, 1, &b));
    const Planes pl = p1_planes(b, ksz, vc, pp, out.flags + 6, true);
    // Range partitions of <= 256 bins go through the tile scatter of the two-level plan, as its only level: whole-column bin counts, write
    // cursors instead of per-chunk histograms, 16384-row tiles with the keys kept in registers, two workgroups per CU so that one tile's
    // loads run under the other's stores (h2o Q5 / Q7 at 1e9 rows, 1e6 groups: this kernel's own 32768-row tiles, one workgroup per CU,
    // moved 3.9 / 2.8 TB/s)
    if (rp.on && ksz == 4 && nbins <= 256 && !aqg_switches().disable_p1_cursors) {
        const uint32_t P = nbins;
        ColumnBins cb;
        AQG_TRY(aqg_scatter_column_bins(ctx, 4, true, b.keycol, n, P, rp.M, rp.kmin, rp.D - 1, 0u, &cb));
        P2Level lv{cb.seg1, cb.tp1, cb.cur2, 1u, rp.M, 0u, 0xFFFFFFFFu, P, 0u, 0u, rp.kmin, rp.D - 1, out.flags + 6, nullptr, nullptr};
        const unsigned tiles = (unsigned)(((uint64_t)n + P2_PT - 1) / P2_PT);
        AQG_TRY(aqg_scatter_pair(ctx, 4, BIN_RANGED, pp.n != 0, 256, b.keycol, pl, lv, tiles, 1u));
        AQG_TRY(aqg_check_launch(ctx, "one-level partition scatter (cursors)"));
        return p1_launch_agg_direct(ctx, as, vc, b.keys[0], b.rows[0], b.vals[0], cb.fstart, 1u, n, need_count, out, out_cap, pp.n ? &pp : nullptr, rp);
    }
    const size_t hcount = (size_t)nbins * ch.nchunks;
    uint32_t *hist, *bsum;
    AQG_TRY(aqg_ws_get(ctx, hcount, &hist));
    AQG_TRY(aqg_ws_get(ctx, hcount / 2048 + 64, &bsum));
    const size_t hist_lds = (size_t)nbins * 4;
    const size_t scat_lds = (size_t)PT * 4 + ((size_t)nbins * 2 + 1) * 4;
    const unsigned nmain = ch.nchunks - ch.has_tail;
    auto run = [&](auto k64, auto rng) -> int {
        constexpr bool K = decltype(k64)::value, R = decltype(rng)::value;
        const key_t_<K>* kc = static_cast<const key_t_<K>*>(b.keycol);
        hipLaunchKernelGGL((p1_hist_kernel<K, R>), dim3(ch.nchunks), dim3(SB), hist_lds, ctx->stream, kc, ch, hist);
        AQG_TRY(aqg_exclusive_scan_u32(ctx, hist, hcount, bsum));
        if (nmain) {
            AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(&p1_scatter_kernel<K, R>), scat_lds));
            hipLaunchKernelGGL((p1_scatter_kernel<K, R>), dim3(nmain), dim3(SB), scat_lds, ctx->stream, kc, pl, ch, (const uint32_t*)hist);
        }
        if (ch.has_tail) {
            AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(&p1_scatter_tail_kernel<K, R>), scat_lds));
            hipLaunchKernelGGL((p1_scatter_tail_kernel<K, R>), dim3(1), dim3(SB), scat_lds, ctx->stream, kc, pl, ch, (const uint32_t*)hist);
        }
        return aqg_check_launch(ctx, "one-level partition scatter");
    };
    if (rp.on) AQG_TRY(run(std::false_type{}, std::true_type{}));
    else if (ksz == 4) AQG_TRY(run(std::false_type{}, std::false_type{}));
    else AQG_TRY(run(std::true_type{}, std::false_type{}));

    if (rp.on) return p1_launch_agg_direct(ctx, as, vc, b.keys[0], b.rows[0], b.vals[0], hist, ch.nchunks, n, need_count, out, out_cap, pp.n ? &pp : nullptr, rp);
    return p1_launch_agg(ctx, ksz, as, vc, b.keys[0], b.rows[0], b.vals[0], hist, ch.nchunks, nbins, n, need_count, out, out_cap, pr, pp.n ? &pp : nullptr, layout);
}


// ---- two levels: host ---------------------------------------------------------------------------------------------------------------
// (why two levels, and what p2_hist / p2_setup / p2_scatter do: tile_scatter.hip)
static uint32_t p2_round_parts(uint32_t parts) { return (parts + 63) & ~63u; }

size_t aqg_partition2_ws_bytes(const aqg_ctx* ctx, const KeySpec& ks, uint32_t n, const AccSpec& as, uint32_t parts) {
    const int ksz = ks.total_bytes <= 4 ? 4 : 8;
    ValCols vc;
    p1_val_cols(as, &vc);
    size_t per_row = 2 * ((size_t)ksz + 4);
    if (!p1_key_is_column(ks, ksz)) per_row += ksz;
    for (int u = 0; u < vc.n; ++u) per_row += 2 * part_val_bytes(vc.dt[u]) + (aqg_dtype_size(vc.dt[u]) < 4 ? 4 : 0);
    return ((size_t)n + 64) * per_row + 256 * (8 + 4 * MAXACC) + (size_t)p2_round_parts(parts) * 16 + 65536;
}

int aqg_partition2_aggregate(aqg_ctx* ctx, const KeySpec& ks, const AccSpec& as, uint32_t n, uint32_t parts, int need_count, GTable out, uint32_t out_cap, PartRows* pr, int* pack, int layout) {
    const int ksz = ks.total_bytes <= 4 ? 4 : 8;
    ValCols vc;
    p1_val_cols(as, &vc);
    PackPlan pp;
    RangePlan rp;
    memset(&pp, 0, sizeof pp);
    memset(&rp, 0, sizeof rp);
    if (pack && *pack && !pr) {
        AQG_TRY(plan_pack(ctx, ks, as, n, vc, &pp));                         // narrow value columns inside the key word (fewer planes per level)
        plan_range(pp, as, need_count, parts, &rp);                          // a dense key domain: range partitions, direct-indexed aggregation
    }
    if (pack) *pack = (pp.n ? 1 : 0) | (rp.on ? 2 : 0);
    const uint32_t P = rp.on ? rp.P : p2_round_parts(parts), B1 = P >> 6;
    if (P < 64 || P > AQG_P2_MAXPARTS) return aqg_fail(ctx, AQG_ERR_OVERFLOW, "two-level partitioned group-by: 64..4096 partitions");
    PartBufs b;
    AQG_TRY(p1_buffers(ctx, ks, ksz, n, vc, pp, 2, &b));
    const unsigned tiles1 = (unsigned)(((uint64_t)n + P2_PT - 1) / P2_PT), tiles2 = (unsigned)((uint64_t)n / P2_PT) + B1 + 1;
    const unsigned xgrid = (tiles2 + 7) / 8 * 5 / 4 + 8;                       // workgroups per XCD of the level-2 launch (a quarter of slack)
    // the bin of a key word at both levels: the hash or (range partitions) the offset in the domain, scaled to P fine partitions;
    // level 1 takes the coarse partition (fine >> 6), level 2 the fine one inside it (fine & 63)
    const uint32_t scale = rp.on ? rp.M : P, xmax = rp.on ? rp.D - 1 : 0u;
    ColumnBins cb;
    AQG_TRY(aqg_scatter_column_bins(ctx, ksz, rp.on, b.keycol, n, P, scale, rp.kmin, xmax, xgrid, &cb));
    P2Level l1{cb.seg1, cb.tp1, cb.cur1, 1u, scale, 6u, 0xFFFFFFFFu, B1, 0u, 0u, rp.kmin, xmax, out.flags + 6};
    P2Level l2{cb.seg2, cb.tp2, cb.cur2, B1, scale, 0u, 63u, 64u, 64u, pp.kclear, rp.kmin, xmax, out.flags + 6, cb.xtp, cb.xtp + 8 * XTP_STRIDE + 32};
    const unsigned grid2 = 8 * xgrid < tiles2 ? tiles2 : 8 * xgrid;                  // (covers the plain walk too, should the setup decline the map)
    const int mode = rp.on ? BIN_RANGED : BIN_HASHED;
    AQG_TRY(aqg_scatter_pair(ctx, ksz, mode, pp.n != 0, 128, b.keycol, p1_planes(b, ksz, vc, pp, out.flags + 6, true), l1, tiles1, 1u));
    AQG_TRY(aqg_scatter_pair(ctx, ksz, mode, false, 128, b.keys[0], p1_planes(b, ksz, vc, pp, out.flags + 6, false), l2, grid2, B1));
    AQG_TRY(aqg_check_launch(ctx, "two-level partition scatter"));
    if (rp.on) return p1_launch_agg_direct(ctx, as, vc, b.keys[1], b.rows[1], b.vals[1], cb.fstart, 1u, n, need_count, out, out_cap, pp.n ? &pp : nullptr, rp);
    return p1_launch_agg(ctx, ksz, as, vc, b.keys[1], b.rows[1], b.vals[1], cb.fstart, 1u, P, n, need_count, out, out_cap, pr, pp.n ? &pp : nullptr, layout);
}
