// groupby_tail.hip -- the tail of a group-by attempt: collect / rank / emit.  Occupied slots of the group table -> dense ids ordered by
// first row -> the handle's output columns.  The phases are called by run_agg (groupby.hip).
#include "groupby_plan.hpp"

namespace {

// first row of every group, after the fact: tiles are scanned in order by a small grid; once every group has a candidate,
// a workgroup stops as soon as its next tile starts beyond the largest candidate (no later row can lower any of them).
__global__ void __launch_bounds__(256) first_rows_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ keys_hi, int key8, uint32_t t0 /* first tile */, uint32_t n /* rows end */, GTable gt, const uint32_t* __restrict__ occ) {
    __shared__ uint32_t red[4];
    __shared__ uint32_t stop, all_seen;
    const uint32_t G = gt.flags[1];
    constexpr int FR = 4;                      // rows per lane and tile: the first round covers gridDim x 1024 rows (16 rows: 28 us on h2o Q1)
    constexpr uint32_t TILE = 256 * FR;
    for (uint32_t t = t0 + blockIdx.x; (uint64_t)t * TILE < n; t += gridDim.x) {
        const uint32_t tbase = t * TILE;
        // ONE lane samples the counter other workgroups keep incrementing: the branch below holds barriers, so every wavefront of
        // the workgroup must take the same side of it (a per-lane load could split them: divergent barrier, stale `red` / `stop`)
        if (threadIdx.x == 0) { stop = 0; all_seen = __hip_atomic_load(&gt.flags[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= G; }
        if (threadIdx.x < 4) red[threadIdx.x] = 0;
        __syncthreads();
        if (all_seen) {
            uint32_t m = 0;
            for (uint32_t i = threadIdx.x; i < G; i += blockDim.x) {
                uint32_t f = __hip_atomic_load(gt.first_p(occ[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                m = f > m ? f : m;
            }
            m = wave_reduce(m, OpMax{});
            if (lane_id() == 0) red[wave_id()] = m;
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t bound = red[0] > red[1] ? red[0] : red[1];
                bound = bound > red[2] ? bound : red[2];
                bound = bound > red[3] ? bound : red[3];
                stop = tbase > bound;
            }
            __syncthreads();
        }
        if (stop) break;
        for (int r = 0; r < FR; ++r) {
            uint32_t row = tbase + r * 256 + threadIdx.x;
            if (row < n) {
                uint32_t s = gt_find(gt, key8 ? reinterpret_cast<const uint64_t*>(keys)[row] : keys_hi ? ((uint64_t)keys[row] | ((uint64_t)keys_hi[row] << 32)) : (uint64_t)keys[row]);
                if (s != FAIL && row < *gt.first_p(s)) {
                    uint32_t old = atomicMin(gt.first_p(s), row);
                    if (old >= OCCUPIED) atomicAdd(&gt.flags[2], 1u);
                }
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) occ_iota_kernel(uint32_t* __restrict__ occ, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) occ[i] = i;
}
__global__ void __launch_bounds__(256) gt_init_kernel(GTable gt, AccSpec as) {
    if (blockIdx.x == 0 && threadIdx.x < 64) gt.flags[threadIdx.x] = 0;          // the 64 flag words, too (one launch instead of a fill behind it)
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s <= gt.cap; s += gridDim.x * blockDim.x) {
        *gt.key_p(s) = EMPTY64;
        *gt.first_p(s) = NOROW;
        *gt.count_p(s) = 0;
        for (int a = 0; a < as.nacc; ++a) *gt.acc_p(a, s) = acc_init(as.kind[a]);
    }
}

// ---- dense ids in first-occurrence order --------------------------------------------------------
// occupied slots -> occ[] (any order).  One returning atomic per workgroup and step, not per wavefront: with 1e8 occupied slots the
// single counter word was the whole cost (47 ms; the word saturates near 9e7 atomics per second).
__global__ void __launch_bounds__(256) collect_kernel(GTable gt, uint32_t* __restrict__ occ) {
    __shared__ uint32_t wcount[4];
    __shared__ uint32_t base;
    const uint64_t total = (uint64_t)gt.cap + 1;
    for (uint64_t s0 = (uint64_t)blockIdx.x * blockDim.x; s0 < total; s0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = s0 + threadIdx.x;
        const bool used = s < total && (*gt.first_p((uint32_t)s)) != NOROW;
        const uint64_t bal = __ballot(used);
        if (lane_id() == 0) wcount[wave_id()] = (uint32_t)__popcll(bal);
        __syncthreads();
        if (threadIdx.x == 0) { const uint32_t c = wcount[0] + wcount[1] + wcount[2] + wcount[3]; base = c ? atomicAdd(&gt.flags[1], c) : 0; }
        __syncthreads();
        if (used) {
            uint32_t off = base + (uint32_t)__popcll(bal & ((1ull << lane_id()) - 1ull));
            for (int w = 0; w < wave_id(); ++w) off += wcount[w];
            occ[off] = (uint32_t)s;
        }
        __syncthreads();
    }
}
// G <= 4096: rank by counting inside one workgroup
__global__ void __launch_bounds__(1024) rank_small_kernel(GTable gt, const uint32_t* __restrict__ occ, uint32_t* __restrict__ gid_of_occ,
                                                          uint32_t* __restrict__ slot_gid) {
    __shared__ uint32_t f[4096];
    uint32_t G = gt.flags[1];
    if (G > 4096) return;
    for (uint32_t i = threadIdx.x; i < G; i += blockDim.x) f[i] = (*gt.first_p(occ[i]));
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < G; i += blockDim.x) {
        uint32_t mine = f[i], r = 0;
        for (uint32_t j = 0; j < G; ++j) r += f[j] < mine;
        gid_of_occ[i] = r;
        slot_gid[occ[i]] = r;
    }
}
// any G: mark first rows in a bitmap over the n rows, prefix-count it, look the rank up
// tile_mark (sparse ranking: few groups over many rows): the tiles of 1024 words that hold a bit at all -- the others are neither
// read nor given prefixes, and the bitmap itself is not cleared with a fill but bit by bit behind the ranking (bitmap_clear_kernel):
// 1e9 rows / 1e4 groups (h2o Q2) spent 0.13 ms filling and scanning 125 MB of zeros
__global__ void __launch_bounds__(256) bitmap_set_kernel(GTable gt, const uint32_t* __restrict__ occ, uint32_t* __restrict__ bitmap, uint32_t* __restrict__ tile_mark) {
    uint32_t G = gt.flags[1];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < G; i += gridDim.x * blockDim.x) {
        uint32_t r = (*gt.first_p(occ[i]));
        atomicOr(&bitmap[r >> 5], 1u << (r & 31));
        if (tile_mark) tile_mark[r >> 15] = 1u;
    }
}
__global__ void __launch_bounds__(256) bitmap_clear_kernel(GTable gt, const uint32_t* __restrict__ occ, uint32_t* __restrict__ bitmap) {
    uint32_t G = gt.flags[1];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < G; i += gridDim.x * blockDim.x) bitmap[(*gt.first_p(occ[i])) >> 5] = 0u;
}
// tile = 1024 words (one per thread... 256 threads x 4 words): per-word exclusive prefix inside the tile + tile total
__global__ void __launch_bounds__(256) bitmap_tile_kernel(const uint32_t* __restrict__ bitmap, uint32_t nwords,
                                                          uint32_t* __restrict__ word_prefix, uint32_t* __restrict__ tile_total, const uint32_t* __restrict__ tile_mark) {
    __shared__ uint32_t wsum[4];
    uint32_t tile = blockIdx.x;
    if (tile_mark && !tile_mark[tile]) { if (threadIdx.x == 0) tile_total[tile] = 0; return; }      // (uniform over the workgroup)
    uint32_t w0 = tile * 1024 + threadIdx.x * 4;
    uint32_t c[4], tot = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { uint32_t w = w0 + j; c[j] = w < nwords ? __popc(bitmap[w]) : 0; tot += c[j]; }
    uint32_t incl = wave_scan_incl(tot, OpAdd{}, lane_id());
    if (lane_id() == 63) wsum[wave_id()] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wave_id(); ++w) wbase += wsum[w];
    uint32_t excl = wbase + incl - tot;
#pragma unroll
    for (int j = 0; j < 4; ++j) { uint32_t w = w0 + j; if (w < nwords) word_prefix[w] = excl; excl += c[j]; }
    if (threadIdx.x == 255) tile_total[tile] = wbase + incl;
}
__global__ void __launch_bounds__(1024) tile_scan_kernel(uint32_t* __restrict__ tile_total, uint32_t ntiles) {
    // single workgroup exclusive scan, in place
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < ntiles; base += 1024) {
        uint32_t i = base + threadIdx.x;
        uint32_t v = i < ntiles ? tile_total[i] : 0;
        uint32_t incl = wave_scan_incl(v, OpAdd{}, lane_id());
        if (lane_id() == 63) wsum[wave_id()] = incl;
        __syncthreads();
        uint32_t wbase = carry;
        for (int w = 0; w < wave_id(); ++w) wbase += wsum[w];
        if (i < ntiles) tile_total[i] = wbase + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = wbase + incl;
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) rank_bitmap_kernel(GTable gt, const uint32_t* __restrict__ occ, const uint32_t* __restrict__ bitmap,
                                                          const uint32_t* __restrict__ word_prefix, const uint32_t* __restrict__ tile_prefix,
                                                          uint32_t* __restrict__ gid_of_occ, uint32_t* __restrict__ slot_gid) {
    uint32_t G = gt.flags[1];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < G; i += gridDim.x * blockDim.x) {
        uint32_t r = (*gt.first_p(occ[i])), w = r >> 5;
        uint32_t rank = tile_prefix[w >> 10] + word_prefix[w] + __popc(bitmap[w] & ((1u << (r & 31)) - 1u));
        gid_of_occ[i] = rank;
        slot_gid[occ[i]] = rank;
    }
}

// `order` (large G only): order[g] = the occ index of dense id g, so that the lanes walk the OUTPUT columns (and, for wide tuples,
// the key columns at the groups' first rows) in ascending order instead of scattering eight columns at random
__global__ void __launch_bounds__(256) emit_order_kernel(const uint32_t* __restrict__ gid_of_occ, uint32_t G, uint32_t* __restrict__ order) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < G; i += gridDim.x * blockDim.x) order[gid_of_occ[i]] = i;
}
// one group: record `s` of `gt` -> row `g` of every output column.  `key`: the packed key, or (wide tuples) the group's first row
// `R` = where the record comes from: first(), count(), acc(a).  TableRecord: slot `s` of a group table; RowRecord (below): ONE ROW of
// the input taken as a whole group (every row its own group).
struct TableRecord {
    static constexpr bool inline_stores = false;
    const GTable& gt; uint32_t s;
    __device__ inline uint32_t first() const { return *gt.first_p(s); }
    __device__ inline uint32_t count() const { return gt.has_count ? *gt.count_p(s) : 0; }
    __device__ inline uint64_t acc(int a) const { return *gt.acc_p(a, s); }
};
template <bool KEYS, class R>
__device__ inline void emit_record_from(const R& rec, uint32_t g, const EmitSpec& es, uint64_t key) {
    if constexpr (KEYS) for (int k = 0; k < es.nkeys; ++k) {
        uint64_t bits = es.wide ? load_bits(es.key_dt[k], es.key_col[k], (size_t)(uint32_t)key) : key >> es.key_shift[k];
        store_sized(es.key_out[k], g, aqg_dtype_size_dev(es.key_dt[k]), bits);
    }
    // (table records store through calls -- see store_at; the streaming row map keeps its stores inline: 5.9 against 7.3 ms per 1e9 rows,
    // and tests/test_gpu_plans.py::test_every_row_its_own_group... checks every arm and value type of that kernel)
    auto put = [&](void* col, size_t i, auto v) { using T = decltype(v); if constexpr (R::inline_stores) static_cast<T*>(col)[i] = v; else store_at<T>(col, i, v); };
    es.first_out[g] = rec.first();
    uint32_t cnt = rec.count();
    if (es.count_out) es.count_out[g] = cnt;
    for (int j = 0; j < es.nagg; ++j) {
        const AggOut& a = es.agg[j];
        int vc = vclass(a.dt);
        uint64_t v0 = a.acc0 >= 0 ? rec.acc(a.acc0) : 0;
        const bool wide = a.dt == AQG_INT64 || a.dt == AQG_UINT64;
        // exact 128-bit sum (and sum of squares) of an integer column
        // (squares of a uint16 column: `x * x` is an int product that wraps negative from 46341 on, and the reference adds it SIGN-extended to
        // its 128-bit sum; the 64-bit accumulator holds the exact signed sum of those products: extended the same way, as aqg_reduce does)
        auto sum128 = [&](int lo_acc, int hi_acc, bool squares = false) -> aqg_i128 {
            uint64_t lo = rec.acc(lo_acc);
            if (!wide) return vc == VC_U && !(squares && a.dt == AQG_UINT16) ? i128_from_u64(lo) : i128_from_i64((int64_t)lo);
            uint64_t hi = rec.acc(hi_acc);                       // sum of the high halves, to be shifted by 32
            aqg_i128 h = vc == VC_U ? i128_from_u64(hi) : i128_from_i64((int64_t)hi);
            aqg_i128 sh = {h.lo << 32, (h.hi << 32) | (h.lo >> 32)};
            return i128_add(sh, i128_from_u64(lo));
        };
        auto to_double = [&](aqg_i128 v) -> double { return vc == VC_U ? u128_to_double(v.hi, v.lo) : i128_to_double(v); };
        switch (a.op) {
        case AQG_RED_SUM: case AQG_RED_SUMSQ:                           // -> GetLongType
            if (vc == VC_F) put(a.out, g, __builtin_bit_cast(double, v0));
            else put(a.out, g, sum128(a.acc0, a.acc1, a.op == AQG_RED_SUMSQ));
            break;
        case AQG_RED_COUNT: put(a.out, g, (uint64_t)cnt); break;
        case AQG_RED_AVG: {                                             // sum / (double)size
            double sd = vc == VC_F ? __builtin_bit_cast(double, v0) : to_double(sum128(a.acc0, a.acc1));
            put(a.out, g, sd / (double)cnt);
        } break;
        case AQG_RED_VAR: case AQG_RED_STDDEV: {                        // (ssq - s*s/(double)(n+1)) / (double)(n+1)
            double np1 = (double)(uint32_t)(cnt + 1), d;
            if (vc == VC_F) {
                double sd = __builtin_bit_cast(double, v0), q = __builtin_bit_cast(double, rec.acc(a.acc2));
                d = (q - sd * sd / np1) / np1;
            } else {
                aqg_i128 sm = sum128(a.acc0, a.acc1), q = sum128(a.acc2, a.acc3, true);
                aqg_i128 ss = i128_mul(sm, sm);                          // s * s in the 128-bit LongType (wraps like the reference)
                d = (to_double(q) - to_double(ss) / np1) / np1;
            }
            put(a.out, g, a.op == AQG_RED_STDDEV ? sqrt(d) : d);
        } break;
        case AQG_RED_MIN: case AQG_RED_MAX: {
            bool mx = a.op == AQG_RED_MAX;
            switch (a.dt) {
            case AQG_INT8: store_minmax<int8_t>(a.out, g, v0, mx); break;
            case AQG_INT16: store_minmax<int16_t>(a.out, g, v0, mx); break;
            case AQG_INT32: store_minmax<int32_t>(a.out, g, v0, mx); break;
            case AQG_INT64: store_minmax<int64_t>(a.out, g, v0, mx); break;
            case AQG_UINT8: store_minmax<uint8_t>(a.out, g, v0, mx); break;
            case AQG_UINT16: store_minmax<uint16_t>(a.out, g, v0, mx); break;
            case AQG_UINT32: store_minmax<uint32_t>(a.out, g, v0, mx); break;
            case AQG_UINT64: store_minmax<uint64_t>(a.out, g, v0, mx); break;
            case AQG_FLOAT: store_minmax<float>(a.out, g, v0, mx); break;
            default: store_minmax<double>(a.out, g, v0, mx); break;
            }
        } break;
        }
    }
}
template <bool KEYS = true>
__device__ inline void emit_record(const GTable& gt, uint32_t s, uint32_t g, const EmitSpec& es, uint64_t key) { emit_record_from<KEYS>(TableRecord{gt, s}, g, es, key); }

// Every row its own group (G == n: a grouping by a unique key, h2o Q10 at 1e9 rows): the groups in first-occurrence order ARE the rows in
// row order, so the result columns are a map of the input columns -- no ranking, no ordering of a billion records.  The record of
// group i is made from row i on the fly: the accumulator a table would hold after that one row (acc_init folded with the row's operand).
struct RowRecord {
    static constexpr bool inline_stores = true;
    const AccSpec& as; uint32_t i;
    __device__ inline uint32_t first() const { return i; }
    __device__ inline uint32_t count() const { return 1u; }
    __device__ inline uint64_t acc(int a) const {
        const uint64_t v = val_operand(as.dt[a], as.col[a], i, as.kind[a], as.square[a], as.part[a]);
        if (as.kind[a] == ACC_ADD_F) return __builtin_bit_cast(uint64_t, 0.0 + __builtin_bit_cast(double, v));     // (what the atomic add onto +0.0 leaves: -0.0 becomes +0.0)
        return v;                                                                                               // 0 + v; min(~0, v); max(0, v)
    }
};
// a column copied at the rate the shifts stream at (one 16-byte vector per lane, exact grid: 6.0 TB/s of combined traffic; the runtime's
// device-to-device copy moves the same bytes at 4.4)
__global__ void __launch_bounds__(256) copy_vec_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t nvec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nvec) dst[i] = src[i];
}
__global__ void __launch_bounds__(256) emit_rows_kernel(AccSpec as, EmitSpec es, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) emit_record_from<false>(RowRecord{as, i}, i, es, (uint64_t)i);     // (the key columns: plain copies)
}
__global__ void __launch_bounds__(256) emit_kernel(GTable gt, const uint32_t* __restrict__ occ, const uint32_t* __restrict__ gid_of_occ, EmitSpec es,
                                                   const uint32_t* __restrict__ order, uint32_t gmax /* 0: no bound; else give up beyond it (ranks were not computed) */,
                                                   int occ_identity /* occ[i] == i (the record tables of the partition plans) */) {
    uint32_t G = gt.flags[1];
    if (gmax && G > gmax) return;
    for (uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < G; i0 += gridDim.x * blockDim.x) {
        const uint32_t i = order ? order[i0] : i0;
        // with `order` the group id is the walk position itself (order[gid_of_occ[i]] = i), and a record table is its own occupancy
        // list: two of the three random lines a group cost at 1e7 groups are not fetched
        const uint32_t s = occ_identity ? i : occ[i], g = order ? i0 : gid_of_occ[i];
        emit_record(gt, s, g, es, s == gt.cap ? EMPTY64 : (*gt.key_p(s)));
    }
}

// Huge group tables (aqg_sorted_tail): one workgroup per partition of the record planes.  The partition holds the groups whose first
// rows lie in one interval of <= C rows, so its first group id is its start offset and a group's id is that plus the number of set
// bits below its first row in a bitmap of the interval.  The records are permuted into id order inside LDS and emitted from there:
// every output column is written front to back, the key columns (wide tuples) are read in ascending row order.
__global__ void __launch_bounds__(1024, 8) sorted_emit_kernel(SortedParts sp, uint32_t G, uint32_t n_rows, int nacc, int has_count, int wide, EmitSpec es, uint32_t* __restrict__ flags) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const uint32_t C = sp.cap, W = C / 32 + 8;
    uint64_t* sacc = reinterpret_cast<uint64_t*>(smem_raw);                 // [nacc][C]
    uint64_t* skey = sacc + (size_t)nacc * C;                               // [C] (packed keys only)
    uint32_t* sfirst = reinterpret_cast<uint32_t*>(skey + (wide ? 0 : C));  // [C]
    uint32_t* scount = sfirst + C;                                          // [C]
    uint32_t* bm = scount + C;                                              // [W] bitmap of the row interval
    uint32_t* wp = bm + W;                                                  // [W] set bits before every word
    __shared__ uint32_t wsum[16];
    const uint32_t NT = blockDim.x;
    GTable lt;
    lt.kb = reinterpret_cast<unsigned char*>(skey); lt.fb = reinterpret_cast<unsigned char*>(sfirst); lt.cb = reinterpret_cast<unsigned char*>(scount);
    lt.ab = reinterpret_cast<unsigned char*>(sacc);
    lt.kst = 8; lt.fst = 4; lt.cst = 4; lt.ast = 8; lt.astep = (uint64_t)C * 8; lt.cap = 0xFFFFFFFFu; lt.flags = nullptr; lt.has_count = has_count;
    bool k32 = wide != 0;
    for (int k = 0; k < es.nkeys; ++k) k32 = k32 && aqg_dtype_size_dev(es.key_dt[k]) == 4;
    for (uint32_t part = blockIdx.x; part < sp.nparts; part += gridDim.x) {
        const uint32_t b = sp.pstart[part], e = sp.pstart[part + 1];
        if (b >= e) continue;
        const uint64_t lo64 = (((uint64_t)part << 32) + sp.M - 1) / sp.M, hi64 = ((((uint64_t)part + 1) << 32) + sp.M - 1) / sp.M;
        const uint32_t lo = (uint32_t)lo64, hi = hi64 < n_rows ? (uint32_t)hi64 : n_rows;
        const uint32_t c = e - b, nw = (hi - lo + 31) / 32;
        if (hi - lo > C || c > C || e > G) { if (threadIdx.x == 0) flags[7] = 1; continue; }       // (the plan rules it out; the host checks the word behind this kernel)
        for (uint32_t w = threadIdx.x; w < nw; w += NT) bm[w] = 0;
        __syncthreads();
        // (four rows of a lane per step, their loads issued together from clamped indices: a partition is a chain of barriers, and a
        // loop that loads, uses and loads again puts one memory latency per row between them)
        for (uint32_t j0 = threadIdx.x; j0 < c; j0 += 4 * NT) {
            uint32_t fr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const uint32_t j = j0 + u * NT; fr[u] = sp.first[b + (j < c ? j : c - 1)]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) if (j0 + u * NT < c) { const uint32_t r = fr[u] - lo; atomicOr(&bm[r >> 5], 1u << (r & 31)); }
        }
        __syncthreads();
        {   // nw <= 512 <= NT: one word per thread
            const uint32_t t = threadIdx.x < nw ? __popc(bm[threadIdx.x]) : 0;
            const uint32_t incl = wave_scan_incl(t, OpAdd{}, lane_id());
            if (lane_id() == 63) wsum[wave_id()] = incl;
            __syncthreads();
            uint32_t base = incl - t;
            for (int w = 0; w < wave_id(); ++w) base += wsum[w];
            if (threadIdx.x < nw) wp[threadIdx.x] = base;
        }
        __syncthreads();
        for (uint32_t j0 = threadIdx.x; j0 < c; j0 += 2 * NT) {
            uint32_t fr[2], cn[2];
            uint64_t ky[2], ac[4][2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint32_t j = j0 + u * NT, jj = b + (j < c ? j : c - 1);
                fr[u] = sp.first[jj];
                cn[u] = has_count ? sp.count[jj] : 0;
                ky[u] = wide ? 0ull : sp.key[jj];
#pragma unroll
                for (int a = 0; a < 4; ++a) ac[a][u] = a < nacc ? sp.acc[a][jj] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (j0 + u * NT >= c) continue;
                const uint32_t r = fr[u] - lo;
                const uint32_t rank = wp[r >> 5] + __popc(bm[r >> 5] & ((1u << (r & 31)) - 1u));
                sfirst[rank] = fr[u];
                scount[rank] = cn[u];
                if (!wide) skey[rank] = ky[u];
#pragma unroll
                for (int a = 0; a < 4; ++a) if (a < nacc) sacc[(size_t)a * C + rank] = ac[a][u];
            }
            for (int a = 4; a < nacc; ++a)                    // (more than four accumulators: the rest one by one)
                for (int u = 0; u < 2; ++u) { const uint32_t j = j0 + u * NT; if (j < c) { const uint32_t r = fr[u] - lo; sacc[(size_t)a * C + wp[r >> 5] + __popc(bm[r >> 5] & ((1u << (r & 31)) - 1u))] = sp.acc[a][b + j]; } }
        }
        __syncthreads();
        if (k32) {      // wide tuples of 4-byte columns: the key loads of a record issued together (emit_record's run one after the other)
            for (uint32_t i0 = threadIdx.x; i0 < c; i0 += 2 * NT) {          // two records per step: up to sixteen key loads in flight
                uint32_t kv[2][MAXKEYS];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t i = i0 + u * NT, row = sfirst[i < c ? i : c - 1];
#pragma unroll
                    for (int k = 0; k < MAXKEYS; ++k) kv[u][k] = k < es.nkeys ? static_cast<const uint32_t*>(es.key_col[k])[row] : 0;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t i = i0 + u * NT, g = b + i;
                    if (i >= c) continue;
#pragma unroll
                    for (int k = 0; k < MAXKEYS; ++k) if (k < es.nkeys) static_cast<uint32_t*>(es.key_out[k])[g] = kv[u][k];
                    emit_record<false>(lt, i, g, es, 0);
                }
            }
        } else {
            for (uint32_t i = threadIdx.x; i < c; i += NT) emit_record(lt, i, b + i, es, wide ? (uint64_t)sfirst[i] : skey[i]);
        }
        __syncthreads();
    }
}

// (one lane per bitmap word of a 16384-row interval: 512 at least)
constexpr unsigned SORTED_EMIT_BLOCK = 1024;

} // namespace

// the launches of this file's kernels that the planner's phases make (agg_workspace, row_pass, pass_partitions)
void aqg_gt_init(aqg_ctx* ctx, const GTable& gt, const AccSpec& as, size_t slots) { hipLaunchKernelGGL(gt_init_kernel, dim3(aqg_grid(ctx, slots, 256, 1, 8)), dim3(256), 0, ctx->stream, gt, as); }
void aqg_collect(aqg_ctx* ctx, const GTable& gt, uint32_t* occ, size_t slots) { hipLaunchKernelGGL(collect_kernel, dim3(aqg_grid(ctx, slots, 256, 1, 8)), dim3(256), 0, ctx->stream, gt, occ); }
void aqg_occ_iota(aqg_ctx* ctx, uint32_t* occ, size_t slots) { hipLaunchKernelGGL(occ_iota_kernel, dim3(aqg_grid(ctx, slots, 256, 1, 8)), dim3(256), 0, ctx->stream, occ, (uint32_t)slots); }

// first rows (fast path), then the group order: none for a row map, the ordering tail, or ranks through a small table / the bitmap
int aqg_rank_groups(aqg_ctx* ctx, const AggPlan& p, const AggBufs& b, uint32_t G, bool row_emit, SortedParts* sparts) {
    const uint32_t n = p.n;
    const GTable& gt = b.gt;
    if ((p.defer || G) && n && p.fast) {
        // two launches: 32 workgroups over the first 32768 rows (where every group of an h2o-like column already shows up), then
        // the whole chip over the rest, whose workgroups leave at once when nothing is missing.  One launch of 256 workgroups
        // starts with 65536 lanes pushing atomicMin at ~100 addresses: 28-31 us on h2o Q1.
        const uint32_t* k0 = static_cast<const uint32_t*>(p.ks.col[0]);
        const uint32_t* k1 = p.fast_k64 && !p.fast_key8 ? static_cast<const uint32_t*>(p.ks.col[1]) : (const uint32_t*)nullptr;
        const uint32_t head_tiles = 32, head_rows = head_tiles * 1024;
        hipLaunchKernelGGL(first_rows_kernel, dim3(head_tiles), dim3(256), 0, ctx->stream, k0, k1, p.fast_key8 ? 1 : 0, 0u, n < head_rows ? n : head_rows, gt, (const uint32_t*)b.occ);
        if (n > head_rows) {
            unsigned fgrid = aqg_grid(ctx, (n - head_rows) / 4 + 1, 256, 1, 1);
            hipLaunchKernelGGL(first_rows_kernel, dim3(fgrid), dim3(256), 0, ctx->stream, k0, k1, p.fast_key8 ? 1 : 0, head_tiles, n, gt, (const uint32_t*)b.occ);
        }
        AQG_TRY(aqg_check_launch(ctx, "first_rows_kernel"));
    }
    if (row_emit) return AQG_OK;
    if (p.sorted_tail && G) return aqg_sorted_tail(ctx, gt, G, n, p.plan.as.nacc, p.ks.wide != 0, sparts);
    if (!(p.defer || G)) return AQG_OK;
    if (p.small_rank) {
        hipLaunchKernelGGL(rank_small_kernel, dim3(1), dim3(1024), 0, ctx->stream, gt, b.occ, b.gid_of_occ, b.slot_gid);
    } else {
        unsigned g1 = aqg_grid(ctx, G, 256, 1, 8);
        hipLaunchKernelGGL(bitmap_set_kernel, dim3(g1), dim3(256), 0, ctx->stream, gt, b.occ, b.bitmap, b.tile_mark);
        hipLaunchKernelGGL(bitmap_tile_kernel, dim3(p.ntiles), dim3(256), 0, ctx->stream, b.bitmap, p.nwords, b.word_prefix, b.tile_total, (const uint32_t*)b.tile_mark);
        hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, b.tile_total, p.ntiles);
        hipLaunchKernelGGL(rank_bitmap_kernel, dim3(g1), dim3(256), 0, ctx->stream, gt, b.occ, b.bitmap, b.word_prefix, b.tile_total, b.gid_of_occ, b.slot_gid);
        if (p.sparse_rank) hipLaunchKernelGGL(bitmap_clear_kernel, dim3(g1), dim3(256), 0, ctx->stream, gt, b.occ, b.bitmap);      // the context's bitmap is all zero again
    }
    return AQG_OK;
}

// the handle's result columns (sized by the table's bound while the flags are deferred), then the emit pass that fills them
int aqg_emit_outputs(aqg_ctx* ctx, const AggPlan& p, aqg_groupby* h, const AggBufs& b, uint32_t G, bool row_emit, const SortedParts& sparts) {
    const KeySpec& ks = p.ks;
    const AccSpec& as = p.plan.as;
    const uint32_t n = p.n;
    const uint32_t gupper = (uint32_t)(b.slots + 1 < 4096 ? b.slots + 1 : 4096);
    h->nkeys = ks.nkeys;
    size_t gcapn = p.defer ? gupper : (G ? G : 1);
    EmitSpec es{};
    es.nkeys = ks.nkeys; es.wide = ks.wide;
    for (int k = 0; k < ks.nkeys; ++k) {
        h->key_dt[k] = ks.dt[k];
        AQG_TRY(aqg_dev_realloc(ctx, &h->keys_out[k], &h->cap_keys[k], gcapn * 8));
        es.key_dt[k] = ks.dt[k]; es.key_shift[k] = ks.shift[k]; es.key_out[k] = h->keys_out[k]; es.key_col[k] = ks.col[k];
    }
    AQG_TRY(aqg_dev_realloc(ctx, &h->first_rows, &h->cap_first, gcapn * 4));
    AQG_TRY(aqg_dev_realloc(ctx, &h->counts, &h->cap_counts, gcapn * 4));
    es.first_out = h->first_rows;
    h->has_counts = p.plan.need_count && (!p.for_build || (p.use_part && n));
    es.count_out = h->has_counts ? h->counts : nullptr;
    es.nagg = p.plan.nagg;
    h->nagg = p.plan.nagg;
    for (int j = 0; j < p.plan.nagg; ++j) {
        es.agg[j] = p.plan.agg[j];
        h->res_dt[j] = aqg_reduce_out_dtype(p.plan.agg[j].op, p.plan.agg[j].dt);
        AQG_TRY(aqg_dev_realloc(ctx, &h->results[j], &h->cap_results[j], gcapn * 16));
        es.agg[j].out = h->results[j];
    }
    if (row_emit) {
        for (int k = 0; k < ks.nkeys; ++k) {
            const size_t bytes = (size_t)n * aqg_dtype_size(ks.dt[k]), nvec = bytes / 16;
            if (((uintptr_t)ks.col[k] & 15) == 0 && nvec && nvec <= 0x7FFFFFFFull * 256) {
                hipLaunchKernelGGL(copy_vec_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, ctx->stream, static_cast<const uint4*>(ks.col[k]), static_cast<uint4*>(h->keys_out[k]), nvec);
                if (bytes & 15) AQG_HIP(ctx, hipMemcpyAsync(static_cast<char*>(h->keys_out[k]) + nvec * 16, static_cast<const char*>(ks.col[k]) + nvec * 16, bytes & 15, hipMemcpyDeviceToDevice, ctx->stream));
            } else AQG_HIP(ctx, hipMemcpyAsync(h->keys_out[k], ks.col[k], bytes, hipMemcpyDeviceToDevice, ctx->stream));
        }
        hipLaunchKernelGGL(emit_rows_kernel, dim3(aqg_grid(ctx, n, 256, 1, 8)), dim3(256), 0, ctx->stream, as, es, n);
        return aqg_check_launch(ctx, "emit_rows_kernel");
    }
    if (p.sorted_tail && G) {
        AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(&sorted_emit_kernel), sparts.lds));
        const unsigned per_cu = sparts.lds <= 80 * 1024 ? 2 : 1;
        const unsigned sg = sparts.nparts < 4u * per_cu * ctx->num_cu ? sparts.nparts : 4u * per_cu * ctx->num_cu;
        hipLaunchKernelGGL(sorted_emit_kernel, dim3(sg), dim3(SORTED_EMIT_BLOCK), sparts.lds, ctx->stream, sparts, G, n, as.nacc, (int)b.gt.has_count, (int)(ks.wide != 0), es, b.gt.flags);
        AQG_TRY(aqg_check_launch(ctx, "sorted_emit_kernel"));
        // a partition that does not keep to the plan (more records or a longer row interval than LDS was sized for) is skipped by the kernel
        // and reported in flag word 7: the output would miss its rows, so the call waits for the word (calls of this size run for tens of
        // milliseconds) and, should it ever be set, runs once more through the bitmap tail
        uint32_t bad = 0;
        AQG_HIP(ctx, hipMemcpyAsync(&bad, b.gt.flags + 7, 4, hipMemcpyDeviceToHost, ctx->stream));
        AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (bad) { h->no_sorted_tail = true; return AQG_ERR_RANGE_MISS; }
        return AQG_OK;
    }
    if (!(p.defer || G)) return AQG_OK;
    unsigned eg = aqg_grid(ctx, p.defer ? gupper : G, 256, 1, 8);
    uint32_t* order = nullptr;
    if (p.ordered_emit && G >= (1u << 20)) {
        AQG_TRY(aqg_ws_get(ctx, b.slots, &order));
        hipLaunchKernelGGL(emit_order_kernel, dim3(eg), dim3(256), 0, ctx->stream, (const uint32_t*)b.gid_of_occ, G, order);
    }
    hipLaunchKernelGGL(emit_kernel, dim3(eg), dim3(256), 0, ctx->stream, b.gt, (const uint32_t*)b.occ, (const uint32_t*)b.gid_of_occ, es, (const uint32_t*)order, p.defer ? 4096u : 0u, (int)(n && (p.use_part || p.use_wpart)));
    return aqg_check_launch(ctx, "emit_kernel");
}
