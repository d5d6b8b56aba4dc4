// sort.hip -- aqg_sort_rows: a stable multi-column sort of row ids (TableInfo::order_by, reference server/table.h:447-465).
//
// Keys are mapped to order-preserving unsigned images (key_image.hpp: sign flip for signed types, the sign-dependent flip for floats after
// canonicalising -0.0 and NaN, complement for DESC, two's-complement negation for NEG) and packed, least significant key at the
// bottom, into segments of at most 64 bits; a 16-byte key is two segments.  The segments are sorted one after the other, least
// significant first, by an LSD radix sort over 8-bit digits:
//   - one histogram kernel per segment counts every digit position in a single read; a position where all rows share one
//     digit is skipped (the counts come to the host in one round trip for all segments),
//   - the first pass of a segment encodes its image from the raw columns and carries {image, id} from then on: one dword plane
//     of image when the segment's active digits span at most four bytes, two otherwise.  Read in row order (no rows_in, first
//     segment), the columns are encoded by the upsweep and again by the scatter; gathered through ids (rows_in, or the previous
//     segment's order), they are encoded once, by the upsweep, which writes the carried image.  The last pass of a segment
//     writes only ids,
//   - every pass is reduce-then-scan: per-chunk digit counts, one exclusive scan of the [digit][chunk] matrix, then a stable
//     scatter in which each workgroup walks its chunk (CHUNK rows) tile by tile: wavefront match-any by ballots ranks a row among
//     equal digits, a (round, wavefront, digit) count matrix in LDS orders the cells, and the tile is staged digit-major in LDS
//     and streamed out in runs (the pattern of postproc.hip).  No hand-off between workgroups inside a kernel.
// Up to SMALL rows are sorted by one workgroup in registers and LDS, every segment and pass in one launch.
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "key_image.hpp"

namespace {

constexpr int RB = 1024;                 // lanes per workgroup of the tile kernels
constexpr int ROUNDS = 4;                // rows per lane and tile
constexpr int RT = RB * ROUNDS;          // rows per tile
constexpr int NW = RB / 64;
constexpr int CELLS = ROUNDS * NW;
constexpr uint32_t CHUNK = 32u * RT;     // rows per workgroup of a pass (131072): 7630 chunks at 1e9 rows
constexpr uint32_t SMALL = RT;           // up to this many rows: one workgroup, one launch
constexpr int MAX_SEGS = 16;
constexpr int HB = 512;                  // lanes per workgroup of the histogram kernel

struct SortField { const void* ptr; uint8_t dt, ord, part, shift; };   // part: 1 = high half of a 16-byte key
struct SortSeg { SortField f[8]; int nf; int bits; };
struct SortSegs { SortSeg s[MAX_SEGS]; int nseg; };

__device__ inline uint64_t enc_128(const void* p, uint32_t row, int ord, bool sgn, int part) {
    const uint64_t* q = static_cast<const uint64_t*>(p) + 2 * (size_t)row;
    uint64_t lo = q[0], hi = q[1];
    if (ord == AQG_ORDER_NEG) { lo = ~lo + 1; hi = ~hi + (lo == 0); }
    if (sgn) hi ^= 1ull << 63;
    if (ord == AQG_ORDER_DESC) { lo = ~lo; hi = ~hi; }
    return part ? hi : lo;
}
__device__ inline uint64_t enc_field(const SortField& f, uint32_t row) {
    uint64_t u = 0;
    switch (f.dt) {
    case AQG_INT8: u = enc_int<uint8_t, true>(f.ptr, row, f.ord); break;
    case AQG_INT16: u = enc_int<uint16_t, true>(f.ptr, row, f.ord); break;
    case AQG_INT32: u = enc_int<uint32_t, true>(f.ptr, row, f.ord); break;
    case AQG_INT64: u = enc_int<uint64_t, true>(f.ptr, row, f.ord); break;
    case AQG_UINT8: case AQG_BOOL: u = enc_int<uint8_t, false>(f.ptr, row, f.ord); break;
    case AQG_UINT16: u = enc_int<uint16_t, false>(f.ptr, row, f.ord); break;
    case AQG_UINT32: u = enc_int<uint32_t, false>(f.ptr, row, f.ord); break;
    case AQG_UINT64: u = enc_int<uint64_t, false>(f.ptr, row, f.ord); break;
    case AQG_FLOAT: u = enc_fp<float, uint32_t>(f.ptr, row, f.ord); break;
    case AQG_DOUBLE: u = enc_fp<double, uint64_t>(f.ptr, row, f.ord); break;
    case AQG_INT128: u = enc_128(f.ptr, row, f.ord, true, f.part); break;
    case AQG_UINT128: u = enc_128(f.ptr, row, f.ord, false, f.part); break;
    }
    return u << f.shift;
}
__device__ inline uint64_t encode(const SortSeg& s, uint32_t row) {
    uint64_t img = 0;
    for (int i = 0; i < s.nf; ++i) img |= enc_field(s.f[i], row);
    return img;
}

// Tile-local stable positions of ROUNDS x RB rows by digit: pos = (rows of smaller digits) + (rows of the same digit in earlier
// (round, wavefront) cells) + (rank inside the wavefront by match-any).  tcnt[d] = rows of digit d in the tile.  The caller has
// synchronised after its last use of L; L.lbase / L.tcnt are valid on return.
struct TileLds { uint16_t cell[CELLS][256]; uint32_t lbase[256], tcnt[256], wsum[4]; };
__device__ inline void tile_rank(TileLds& L, const uint32_t d[ROUNDS], const bool live[ROUNDS], int nbits, uint32_t pos[ROUNDS]) {
    const int lane = lane_id(), wid = wave_id();
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    for (uint32_t i = threadIdx.x; i < CELLS * 256 / 2; i += RB) reinterpret_cast<uint32_t*>(&L.cell[0][0])[i] = 0;
    __syncthreads();
    uint32_t rank[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        uint64_t peers = __ballot(live[r]);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            if (bit >= nbits) break;                    // (uniform: the digit's higher bits are zero in every row)
            const uint64_t bal = __ballot((d[r] >> bit) & 1);
            peers &= ((d[r] >> bit) & 1) ? bal : ~bal;
        }
        rank[r] = __popcll(peers & lt_mask);
        if (live[r] && rank[r] == 0) L.cell[r * NW + wid][d[r]] = (uint16_t)__popcll(peers);
    }
    __syncthreads();
    uint32_t total = 0, incl = 0;
    if (threadIdx.x < 256) {                            // one lane per digit: exclusive prefix over the cells
        for (int c0 = 0; c0 < CELLS; c0 += 16) {
            uint32_t t[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) t[c] = L.cell[c0 + c][threadIdx.x];
#pragma unroll
            for (int c = 0; c < 16; ++c) { L.cell[c0 + c][threadIdx.x] = (uint16_t)total; total += t[c]; }
        }
        L.tcnt[threadIdx.x] = total;
        incl = wave_scan_incl(total, OpAdd{}, lane);
        if (lane == 63) L.wsum[wid] = incl;
    }
    __syncthreads();
    if (threadIdx.x < 256) {
        uint32_t base = 0;
        for (int w = 0; w < wid; ++w) base += L.wsum[w];
        L.lbase[threadIdx.x] = base + incl - total;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) pos[r] = live[r] ? L.lbase[d[r]] + L.cell[r * NW + wid][d[r]] + rank[r] : 0u;
}

// rows move to their positions: v[r] of every live row goes to tile slot pos[r], then lane slots are read back in order
__device__ inline void exchange(uint32_t* stage, uint32_t (&v)[ROUNDS], const uint32_t pos[ROUNDS], const bool live[ROUNDS]) {
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) if (live[r]) stage[pos[r]] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) if (live[r]) v[r] = stage[r * RB + threadIdx.x];
    __syncthreads();
}

// ---- small inputs: one workgroup sorts up to SMALL rows through every segment and digit position -------------------------
__global__ void __launch_bounds__(RB) sort_small_kernel(SortSegs segs, const uint32_t* rows_in, uint32_t m,
                                                        uint32_t* rows_out, uint32_t* __restrict__ passes_out) {
    __shared__ TileLds L;
    __shared__ uint32_t stage[RT];
    uint32_t id[ROUNDS], lo[ROUNDS], hi[ROUNDS], d[ROUNDS], pos[ROUNDS];
    bool live[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const uint32_t p = r * RB + threadIdx.x;
        live[r] = p < m;
        id[r] = live[r] ? (rows_in ? rows_in[p] : p) : 0u;
    }
    uint32_t passes = 0;
    for (int s = 0; s < segs.nseg; ++s) {
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const uint64_t img = live[r] ? encode(segs.s[s], id[r]) : 0ull;
            lo[r] = (uint32_t)img; hi[r] = (uint32_t)(img >> 32);
        }
        for (int dp = 0; dp * 8 < segs.s[s].bits; ++dp) {
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) d[r] = ((dp < 4 ? lo[r] : hi[r]) >> ((dp & 3) * 8)) & 255u;
            __syncthreads();                            // the previous exchange is done with stage / L
            tile_rank(L, d, live, 8, pos);
            bool varies = false;
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) varies |= live[r] && L.tcnt[d[r]] != m;
            if (!__syncthreads_or(varies)) continue;    // every row has this digit: the pass would not move a row
            ++passes;
            exchange(stage, id, pos, live);
            exchange(stage, lo, pos, live);
            exchange(stage, hi, pos, live);
        }
    }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) if (live[r]) rows_out[r * RB + threadIdx.x] = id[r];
    if (threadIdx.x == 0) *passes_out = passes;
}

// ---- up-front histogram: counts of every digit position of one segment, per workgroup -> part[block][pos][256] -------------
__global__ void __launch_bounds__(HB) sort_hist_kernel(SortSeg seg, const uint32_t* __restrict__ ids, uint32_t m, int npos, uint32_t* __restrict__ part) {
    __shared__ uint32_t h[8 * 256];
    for (uint32_t i = threadIdx.x; i < 8 * 256; i += HB) h[i] = 0;
    __syncthreads();
    const uint32_t step = gridDim.x * HB * 4;
    for (uint32_t base = blockIdx.x * HB * 4; base < m; base += step) {
        uint64_t img[4];
        bool live[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t p = base + k * HB + threadIdx.x, q = p < m ? p : m - 1;
            live[k] = p < m;
            img[k] = encode(seg, ids ? ids[q] : q);
        }
        for (int dp = 0; dp < npos; ++dp)
#pragma unroll
            for (int k = 0; k < 4; ++k) hist_add(h + dp * 256, (uint32_t)(img[k] >> (8 * dp)) & 255u, live[k]);
        if (base + step < base) break;                  // (32-bit wrap near AQG_MAX_ROWS)
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)npos * 256; i += HB) part[(size_t)blockIdx.x * 2048 + i] = h[i];
}
// tot[pos][d] += sum of part[b][pos][d] over this workgroup's slice of blocks (tot zeroed beforehand)
__global__ void __launch_bounds__(256) sort_hist_reduce_kernel(const uint32_t* __restrict__ part, uint32_t nblocks, uint32_t per, uint32_t* __restrict__ tot) {
    const uint32_t dp = blockIdx.x, b0 = blockIdx.y * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    uint32_t s = 0;
    for (uint32_t b = b0; b < b1; ++b) s += part[(size_t)b * 2048 + dp * 256 + threadIdx.x];
    if (s) atomicAdd(&tot[dp * 256 + threadIdx.x], s);
}

// ---- one pass: per-chunk counts (upsweep) and the stable scatter ----------------------------------------------------------
struct PassArgs {
    SortSeg seg;
    const uint32_t* ids_in;                 // ENC: the rows to encode (nullptr: identity); else the carried ids
    const uint32_t* lo_in; const uint32_t* hi_in;
    uint32_t m, nch;
    uint32_t imshift;                       // ENC: low bits of the segment image below its lowest active digit (dropped)
    uint32_t dshift;                        // digit shift inside the carried 64-bit image
    int nbits;                              // significant bits of this pass's digit
    uint32_t* counts;                       // [256][nch]: counts (upsweep output), exclusive-scanned (scatter input)
    uint32_t* ids_out; uint32_t* lo_out; uint32_t* hi_out;
    uint32_t* st_lo; uint32_t* st_hi;       // upsweep of an encoding pass through ids: the carried image of every row, in row order
};

template <bool ENC, bool WIMG, int NPL>
__device__ inline void load_row(const PassArgs& a, uint32_t q, uint32_t& id, uint32_t& lo, uint32_t& hi) {
    if constexpr (ENC) {
        id = a.ids_in ? a.ids_in[q] : q;
        const uint64_t img = encode(a.seg, id) >> a.imshift;
        lo = (uint32_t)img; hi = NPL == 2 ? (uint32_t)(img >> 32) : 0u;
    } else {
        id = a.ids_in[q];
        lo = 0; hi = 0;
        if (WIMG || a.dshift < 32) lo = a.lo_in[q];
        if constexpr (NPL == 2) { if (WIMG || a.dshift >= 32) hi = a.hi_in[q]; }
    }
}
__device__ inline uint32_t digit_of(uint32_t lo, uint32_t hi, uint32_t dshift) { return ((dshift < 32 ? lo : hi) >> (dshift & 31)) & 255u; }

// STORE (encoding passes that gather through ids): the upsweep also writes the carried image to st_lo / st_hi, so the columns are
// gathered once and the scatter reads the planes
template <bool ENC, int NPL, bool STORE>
__global__ void __launch_bounds__(256) sort_count_kernel(PassArgs a) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t c0 = blockIdx.x * CHUNK, c1 = a.m - c0 < CHUNK ? a.m : c0 + CHUNK;
    for (uint32_t base = c0; base < c1; base += 256 * 8) {
        uint32_t d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t p = base + k * 256 + threadIdx.x, q = p < c1 ? p : c1 - 1;
            uint32_t id, lo, hi;
            load_row<ENC, false, NPL>(a, q, id, lo, hi);
            d[k] = digit_of(lo, hi, a.dshift);
            if constexpr (STORE) {
                if (p < c1) { a.st_lo[p] = lo; if constexpr (NPL == 2) a.st_hi[p] = hi; }
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) hist_add(h, d[k], base + k * 256 + threadIdx.x < c1);
    }
    __syncthreads();
    a.counts[(size_t)threadIdx.x * a.nch + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter of one chunk, tile after tile; gbase[d] = where the chunk's next row of digit d goes.  The next tile's rows are
// loaded while the current one is written out.
template <bool ENC, bool WIMG, int NPL>
__global__ void __launch_bounds__(RB) sort_scatter_kernel(PassArgs a) {
    __shared__ TileLds L;
    __shared__ uint32_t gbase[256], stage[RT], delta[RT];
    const uint32_t c0 = blockIdx.x * CHUNK, c1 = a.m - c0 < CHUNK ? a.m : c0 + CHUNK;
    if (threadIdx.x < 256) gbase[threadIdx.x] = a.counts[(size_t)threadIdx.x * a.nch + blockIdx.x];
    uint32_t id[ROUNDS], lo[ROUNDS], hi[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const uint32_t p = c0 + r * RB + threadIdx.x;
        load_row<ENC, WIMG, NPL>(a, p < c1 ? p : c1 - 1, id[r], lo[r], hi[r]);
    }
    for (uint32_t tbase = c0; tbase < c1; tbase += RT) {
        const uint32_t nrows = c1 - tbase < (uint32_t)RT ? c1 - tbase : (uint32_t)RT;
        uint32_t d[ROUNDS], pos[ROUNDS];
        bool live[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) { live[r] = r * RB + threadIdx.x < nrows; d[r] = digit_of(lo[r], hi[r], a.dshift); }
        __syncthreads();                                // the previous tile is done with L / stage / delta; gbase is advanced
        tile_rank(L, d, live, a.nbits, pos);
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            if (live[r]) { delta[pos[r]] = gbase[d[r]] - L.lbase[d[r]]; stage[pos[r]] = id[r]; }
        }
        __syncthreads();
        uint32_t nlo[ROUNDS] = {}, nhi[ROUNDS] = {};    // the next tile's rows, in flight during the writes below
        const uint32_t nb = tbase + RT;
        if (nb < c1) {
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) {
                const uint32_t p = nb + r * RB + threadIdx.x;
                load_row<ENC, WIMG, NPL>(a, p < c1 ? p : c1 - 1, id[r], nlo[r], nhi[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const uint32_t j = r * RB + threadIdx.x;
            if (j < nrows) a.ids_out[j + delta[j]] = stage[j];
        }
        if constexpr (WIMG) {
#pragma unroll
            for (int h = 0; h < NPL; ++h) {
                __syncthreads();
#pragma unroll
                for (int r = 0; r < ROUNDS; ++r) if (live[r]) stage[pos[r]] = h ? hi[r] : lo[r];
                __syncthreads();
                uint32_t* out = h ? a.hi_out : a.lo_out;
#pragma unroll
                for (int r = 0; r < ROUNDS; ++r) {
                    const uint32_t j = r * RB + threadIdx.x;
                    if (j < nrows) out[j + delta[j]] = stage[j];
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < 256) gbase[threadIdx.x] += L.tcnt[threadIdx.x];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) { lo[r] = nlo[r]; hi[r] = nhi[r]; }
    }
}

__global__ void __launch_bounds__(256) iota_kernel(uint32_t* __restrict__ out, uint32_t m) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) out[i] = i;
}

int key_width(int dt) {
    switch (dt) {
    case AQG_INT8: case AQG_UINT8: case AQG_BOOL: return 1;
    case AQG_INT16: case AQG_UINT16: return 2;
    case AQG_INT32: case AQG_UINT32: case AQG_FLOAT: return 4;
    case AQG_INT64: case AQG_UINT64: case AQG_DOUBLE: return 8;
    case AQG_INT128: case AQG_UINT128: return 16;
    }
    return 0;
}

template <bool ENC, bool WIMG, int NPL> void launch_scatter(aqg_ctx* ctx, const PassArgs& a) {
    hipLaunchKernelGGL((sort_scatter_kernel<ENC, WIMG, NPL>), dim3(a.nch), dim3(RB), 0, ctx->stream, a);
}
template <bool ENC, int NPL, bool STORE> void launch_count(aqg_ctx* ctx, const PassArgs& a) {
    hipLaunchKernelGGL((sort_count_kernel<ENC, NPL, STORE>), dim3(a.nch), dim3(256), 0, ctx->stream, a);
}
void launch_pass(aqg_ctx* ctx, const PassArgs& a, bool enc, int npl, bool store) {
    if (store) { if (npl == 2) launch_count<true, 2, true>(ctx, a); else launch_count<true, 1, true>(ctx, a); }
    else if (enc) { if (npl == 2) launch_count<true, 2, false>(ctx, a); else launch_count<true, 1, false>(ctx, a); }
    else { if (npl == 2) launch_count<false, 2, false>(ctx, a); else launch_count<false, 1, false>(ctx, a); }
}
void launch_scatter_any(aqg_ctx* ctx, const PassArgs& a, bool enc, bool wimg, int npl) {
    if (enc) {
        if (wimg) { if (npl == 2) launch_scatter<true, true, 2>(ctx, a); else launch_scatter<true, true, 1>(ctx, a); }
        else launch_scatter<true, false, 1>(ctx, a);
    } else {
        if (wimg) { if (npl == 2) launch_scatter<false, true, 2>(ctx, a); else launch_scatter<false, true, 1>(ctx, a); }
        else { if (npl == 2) launch_scatter<false, false, 2>(ctx, a); else launch_scatter<false, false, 1>(ctx, a); }
    }
}

} // namespace

extern "C" {

int aqg_sort_rows(aqg_ctx* ctx, int nkeys, const int* key_dtypes, const void* const* keys, const int* orders,
                  uint32_t n, const uint32_t* rows_in, uint32_t m, uint32_t* rows_out) {
    if (!ctx) return AQG_ERR_ARG;
    if (nkeys < 1 || nkeys > 8 || !key_dtypes || !keys || !orders) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_sort_rows: nkeys must be 1..8");
    for (int j = 0; j < nkeys; ++j)
        if (!key_width(key_dtypes[j])) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_sort_rows: key dtype not supported");
    for (int j = 0; j < nkeys; ++j) {
        if (orders[j] < AQG_ORDER_ASC || orders[j] > AQG_ORDER_NEG) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_sort_rows: bad order");
        if (orders[j] == AQG_ORDER_NEG && dt_is_fp(key_dtypes[j])) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_sort_rows: NEG on a floating key");
        if (!keys[j] && n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_sort_rows: null key column");
    }
    AQG_CHECK_ROWS(ctx, n, "aqg_sort_rows");
    AQG_CHECK_ROWS(ctx, m, "aqg_sort_rows");
    if (!rows_in && m != n) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_sort_rows: rows_in == nullptr needs m == n");
    if (m && !rows_out) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_sort_rows: null rows_out");
    ctx->sort_passes = 0;
    ctx->sort_passes_on_dev = false;
    if (m == 0) return AQG_OK;

    // segments: key images of at most 64 bits each, packed from the least significant end (the last key)
    SortSegs segs{};
    {
        int used = 64;
        for (int j = nkeys - 1; j >= 0; --j) {
            const int w = key_width(key_dtypes[j]);
            for (int part = 0; part < (w == 16 ? 2 : 1); ++part) {
                const int bits = w == 16 ? 64 : 8 * w;
                if (used + bits > 64) { if (segs.nseg == MAX_SEGS) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_sort_rows: keys too wide"); ++segs.nseg; used = 0; }
                SortSeg& s = segs.s[segs.nseg - 1];
                s.f[s.nf++] = SortField{keys[j], (uint8_t)key_dtypes[j], (uint8_t)orders[j], (uint8_t)part, (uint8_t)used};
                used += bits;
                s.bits = used;
            }
        }
    }
    if (m <= SMALL) {
        if (!ctx->sort_passes_dev) AQG_HIP(ctx, aqg_scratch_malloc(ctx, &ctx->sort_passes_dev, 256));
        aqg_kernel_timer_begin(ctx);
        hipLaunchKernelGGL(sort_small_kernel, dim3(1), dim3(RB), 0, ctx->stream, segs, rows_in, m, rows_out, ctx->sort_passes_dev);
        aqg_kernel_timer_end(ctx);
        AQG_TRY(aqg_check_launch(ctx, "sort_small_kernel"));
        ctx->sort_passes_on_dev = true;
        return AQG_OK;
    }

    // workspace (sized once: a grow inside the call would move earlier sub-allocations)
    const uint32_t nch = aqg_ceil_div(m, CHUNK);
    const uint32_t hblocks = aqg_grid(ctx, m, HB, 4, 4);
    const bool overlap = rows_in && rows_in < rows_out + m && rows_out < rows_in + m;
    auto rup = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t hcount = (size_t)256 * nch;
    size_t need = rup((size_t)hblocks * 2048 * 4) + rup((size_t)segs.nseg * 2048 * 4) + rup(hcount * 4) + rup((hcount + 2047) / 2048 * 4 + 64)
                + 6 * rup((size_t)m * 4) + (overlap ? rup((size_t)m * 4) : 0) + 4096;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, need));
    uint32_t *part, *tot, *counts, *bsum, *rin = const_cast<uint32_t*>(rows_in);
    AQG_TRY(aqg_ws_get(ctx, (size_t)hblocks * 2048, &part));
    AQG_TRY(aqg_ws_get(ctx, (size_t)segs.nseg * 2048, &tot));
    AQG_TRY(aqg_ws_get(ctx, hcount, &counts));
    AQG_TRY(aqg_ws_get(ctx, (hcount + 2047) / 2048 + 16, &bsum));
    if (overlap) {
        AQG_TRY(aqg_ws_get(ctx, m, &rin));
        AQG_HIP(ctx, hipMemcpyAsync(rin, rows_in, (size_t)m * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }

    // every digit position of every segment, one read per segment, one round trip
    AQG_HIP(ctx, hipMemsetAsync(tot, 0, (size_t)segs.nseg * 2048 * 4, ctx->stream));
    const uint32_t per = aqg_ceil_div(hblocks, 32), slices = aqg_ceil_div(hblocks, per);
    for (int s = 0; s < segs.nseg; ++s) {
        const int npos = (segs.s[s].bits + 7) / 8;
        hipLaunchKernelGGL(sort_hist_kernel, dim3(hblocks), dim3(HB), 0, ctx->stream, segs.s[s], rin, m, npos, part);
        hipLaunchKernelGGL(sort_hist_reduce_kernel, dim3(npos, slices), dim3(256), 0, ctx->stream, part, hblocks, per, tot + (size_t)s * 2048);
    }
    AQG_TRY(aqg_check_launch(ctx, "sort histogram"));
    std::vector<uint32_t> th((size_t)segs.nseg * 2048);
    AQG_TRY(aqg_d2h(ctx, th.data(), tot, th.size() * 4));

    struct Pass { int seg, pos, npl; bool enc, wimg; uint32_t imshift, dshift; int nbits; };
    std::vector<Pass> passes;
    bool two_planes = false;
    for (int s = 0; s < segs.nseg; ++s) {
        std::vector<int> act;
        std::vector<int> nb;
        for (int dp = 0; dp * 8 < segs.s[s].bits; ++dp) {
            const uint32_t* t = &th[(size_t)s * 2048 + dp * 256];
            bool constant = false;
            int maxd = 0;
            for (int d = 0; d < 256; ++d) { if (t[d] == m) constant = true; if (t[d]) maxd = d; }
            if (constant) continue;
            int bits = 1;
            while ((1 << bits) <= maxd) ++bits;
            act.push_back(dp); nb.push_back(bits);
        }
        if (act.empty()) continue;
        const int npl = act.back() - act.front() < 4 ? 1 : 2;
        two_planes |= npl == 2;
        for (size_t i = 0; i < act.size(); ++i)
            passes.push_back(Pass{s, act[i], npl, i == 0, i + 1 < act.size(), (uint32_t)(8 * act.front()), (uint32_t)(8 * (act[i] - act.front())), nb[i]});
    }
    ctx->sort_passes = (uint32_t)passes.size();
    if (passes.empty()) {                               // every row has the same key: the input order stands
        if (!rows_in) hipLaunchKernelGGL(iota_kernel, dim3(aqg_grid(ctx, m, 256, 4, 8)), dim3(256), 0, ctx->stream, rows_out, m);
        else if (rows_in != rows_out) AQG_HIP(ctx, hipMemcpyAsync(rows_out, rin, (size_t)m * 4, hipMemcpyDeviceToDevice, ctx->stream));   // rin: a copy when the two overlap
        return aqg_check_launch(ctx, "iota_kernel");
    }
    uint32_t *ids[2], *lo[2] = {nullptr, nullptr}, *hi[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k) {
        AQG_TRY(aqg_ws_get(ctx, m, &ids[k]));
        AQG_TRY(aqg_ws_get(ctx, m, &lo[k]));
        if (two_planes) AQG_TRY(aqg_ws_get(ctx, m, &hi[k]));
    }
    aqg_kernel_timer_begin(ctx);
    const uint32_t *ids_cur = rin, *lo_cur = nullptr, *hi_cur = nullptr;
    for (size_t k = 0; k < passes.size(); ++k) {
        const Pass& p = passes[k];
        const bool last = k + 1 == passes.size();
        PassArgs a{};
        a.seg = segs.s[p.seg];
        a.ids_in = ids_cur; a.lo_in = lo_cur; a.hi_in = hi_cur;
        a.m = m; a.nch = nch; a.imshift = p.imshift; a.nbits = p.nbits;
        a.counts = counts;
        a.ids_out = last ? rows_out : ids[k & 1];
        a.lo_out = p.wimg ? lo[k & 1] : nullptr;
        a.hi_out = p.wimg && p.npl == 2 ? hi[k & 1] : nullptr;
        a.dshift = p.dshift;
        // a segment's first pass that gathers through ids (rows_in, or the previous segment's order): the upsweep encodes each row once
        // and leaves the carried image in the plane buffers of the other parity (the previous pass, a segment's last, wrote none), and
        // the scatter reads it as a carried pass.  Without ids the columns are read in order, and reading them twice is cheaper.
        const bool stage = p.enc && ids_cur != nullptr;
        if (stage) { a.st_lo = lo[(k + 1) & 1]; a.st_hi = p.npl == 2 ? hi[(k + 1) & 1] : nullptr; }
        launch_pass(ctx, a, p.enc, p.npl, stage);
        AQG_TRY(aqg_exclusive_scan_u32(ctx, counts, hcount, bsum));
        if (stage) { a.lo_in = a.st_lo; a.hi_in = a.st_hi; }
        launch_scatter_any(ctx, a, p.enc && !stage, p.wimg, p.npl);
        AQG_TRY(aqg_check_launch(ctx, "sort pass"));
        ids_cur = a.ids_out; lo_cur = a.lo_out; hi_cur = a.hi_out;
    }
    aqg_kernel_timer_end(ctx);
    return AQG_OK;
}

int aqg_sort_last_passes(aqg_ctx* ctx, uint32_t* passes_host) {
    if (!ctx || !passes_host) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_sort_last_passes: bad argument");
    if (ctx->sort_passes_on_dev) return aqg_d2h(ctx, passes_host, ctx->sort_passes_dev, 4);
    *passes_host = ctx->sort_passes;
    return AQG_OK;
}

} // extern "C"
