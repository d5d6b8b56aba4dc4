// partition_wide.hip -- the wide-tuple plan of the partitioned group-by (aqg_partitionw_*): hash passes, the level loop over the tile
// scatter of tile_scatter.hip, and the aggregation of every partition inside LDS.  Behind it, for a reason of the compiler's given there,
// the grouped reduce partitioned on dense group ids (aqg_gid_reduce)
#include <vector>
#include "partition1_int.hpp"
#include "tile_scatter.hpp"
#include "dense.hpp"

namespace {

// ==== tuples wider than 8 bytes (h2o Q10: six int32 keys, nearly every row its own group) ==============================================
// Round 1 sent such rows straight to an HBM table with device-scope atomics (0.54 s per 1e9 rows).  Here the rows are partitioned on a
// 32-bit HASH of the tuple (pw_hash: one pass over the key columns), through up to three levels of the same tile scatter (a first level
// of <= 128 bins, lower levels of 64 or 128; every level: a per-segment histogram pass over the hash plane, a scan, the scatter), until
// a partition has ~1000 ROWS (pw_plan).  The key columns travel as ordinary dword planes.  pw_agg then loads a whole partition into LDS
// and groups it there: an open-addressing table of representative row indices, tuples compared LDS to LDS, accumulators indexed by
// the representative.  The record's key word is the group's first row: emit fetches the key columns through it (the wide-tuple
// convention of groupby_hashed.hip / groupby_tail.hip).  Sized by rows, not by groups: a tuple that dominates the input overflows its partition and the call
// falls back to the HBM table.
__device__ inline uint32_t pw_seeded(uint32_t h, uint32_t seed) { h ^= seed; h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; return h ^ (h >> 16); }
__global__ void __launch_bounds__(256) pw_hash_kernel(KeySpec ks, uint32_t n, uint32_t seed, uint32_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { const uint32_t h = hash_wide(ks, i); out[i] = seed ? pw_seeded(h, seed) : h; }
}
// the same for key columns that are all 4 bytes wide and 16-byte aligned (h2o Q10): four rows per lane by vector loads, 32-bit
// multiplies only (murmur3's block mix and finaliser -- NOT the chain pw_agg hashes a partition's rows with: the slots inside a
// partition must not follow from the bits that chose the partition).  (the generic pw_hash_kernel: 9.2 ms per 1e9 rows of six columns)
struct Keys32 { const uint32_t* col[MAXKEYS]; int n; };
__device__ inline uint32_t pw_mix32(uint32_t h, uint32_t k, uint32_t c1, uint32_t c2) {
    k *= c1; k = (k << 15) | (k >> 17); k *= c2;
    h ^= k; h = (h << 13) | (h >> 19);
    return h * 5u + 0xE6546B64u;
}
__device__ inline uint32_t pw_fin32(uint32_t h) { h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; return h ^ (h >> 16); }
// TWO 32-bit states with different multipliers: with one, the 1e11 distinct (id1, id2, id3) prefixes of h2o Q10 collide in the
// state after three columns and stay collided, and the partition sizes grow a tail (one partition of 1164 rows where 954 + 6.4
// sigma were allowed: the whole call fell back to the HBM table)
__device__ inline uint32_t pw_hash_row(const uint32_t* k, int nk, uint32_t seed) {
    uint32_t a = 0x2F0B4C9Du ^ seed, b = 0x8A91E5C3u + seed;
    for (int j = 0; j < nk; ++j) { a = pw_mix32(a, k[j], 0xCC9E2D51u, 0x1B873593u); b = pw_mix32(b, k[j], 0x9E3779B1u, 0x85EBCA77u); }
    return pw_fin32(a ^ pw_fin32(b));
}
// PACKW: the key columns also leave this pass PACKED -- column k as the field ((value - min[k]) & mask[k]) << shift[k] of dword plane
// word[k] -- under ranges sampled from the first 2^20 rows; every row is verified here (a miss sets *flag: the call repeats unpacked).
// The six id columns of h2o Q10 (7 + 7 + 24 + 7 + 7 + 24 bits) travel as three dword planes instead of six through every level and
// through pw_agg's LDS; tuple equality on the packed planes IS tuple equality (the map is injective on verified rows), and the result's
// key columns are fetched through the groups' first rows as before.
struct PackW { int nout; uint32_t min[MAXKEYS], mask[MAXKEYS]; int word[MAXKEYS], shift[MAXKEYS]; uint32_t* out[4]; uint32_t* flag; };
// The pass also counts the bins of the FIRST partition level (lc.cnt: <= 128 bins, counted in LDS, flushed with one atomic per bin and workgroup):
// the hash is in a register here, and pn_level_hist read the whole hash plane again for it (1.1 ms per 1e9 rows).
struct Level1Count { uint32_t* cnt; uint32_t P, shift; };
__device__ inline uint32_t pw_level1_bin(uint32_t h, const Level1Count& lc) { return __umulhi(key_hash<false>(h), lc.P) >> lc.shift; }
template <bool PACKW>
__global__ void __launch_bounds__(256) pw_hash32_kernel(Keys32 ks, uint32_t n, uint32_t seed, uint32_t* __restrict__ out, PackW pk, Level1Count lc) {
    const uint32_t nchunk = n >> 2;
    uint32_t bad = 0;
    __shared__ uint32_t lbin[128];
    if (threadIdx.x < 128) lbin[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < nchunk; c += gridDim.x * 256) {
        pack<uint32_t, 4> v[MAXKEYS];
#pragma unroll
        for (int k = 0; k < MAXKEYS; ++k) if (k < ks.n) v[k] = *reinterpret_cast<const pack<uint32_t, 4>*>(ks.col[k] + (size_t)c * 4);
        pack<uint32_t, 4> a, b, h;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a.v[j] = 0x2F0B4C9Du ^ seed; b.v[j] = 0x8A91E5C3u + seed; }
#pragma unroll
        for (int k = 0; k < MAXKEYS; ++k) {
            if (k < ks.n) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { a.v[j] = pw_mix32(a.v[j], v[k].v[j], 0xCC9E2D51u, 0x1B873593u); b.v[j] = pw_mix32(b.v[j], v[k].v[j], 0x9E3779B1u, 0x85EBCA77u); }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) h.v[j] = pw_fin32(a.v[j] ^ pw_fin32(b.v[j]));
        *reinterpret_cast<pack<uint32_t, 4>*>(out + (size_t)c * 4) = h;
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&lbin[pw_level1_bin(h.v[j], lc) & 127u], 1u);
        if constexpr (PACKW) {
#pragma unroll
            for (int k = 0; k < MAXKEYS; ++k) {
                if (k < ks.n) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[k].v[j] -= pk.min[k]; bad |= v[k].v[j] > pk.mask[k] ? 1u : 0u; v[k].v[j] = (v[k].v[j] & pk.mask[k]) << pk.shift[k]; }
                }
            }
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (o < pk.nout) {
                    pack<uint32_t, 4> w;
#pragma unroll
                    for (int j = 0; j < 4; ++j) w.v[j] = 0;
#pragma unroll
                    for (int k = 0; k < MAXKEYS; ++k) {
                        if (k < ks.n && pk.word[k] == o) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) w.v[j] |= v[k].v[j];
                        }
                    }
                    *reinterpret_cast<pack<uint32_t, 4>*>(pk.out[o] + (size_t)c * 4) = w;
                }
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = ((size_t)nchunk << 2) + threadIdx.x;
        uint32_t k[MAXKEYS];
        for (int j = 0; j < ks.n; ++j) k[j] = ks.col[j][i];
        out[i] = pw_hash_row(k, ks.n, seed);
        atomicAdd(&lbin[pw_level1_bin(out[i], lc) & 127u], 1u);
        if constexpr (PACKW) {
            for (int o = 0; o < pk.nout; ++o) {
                uint32_t w = 0;
                for (int j = 0; j < ks.n; ++j) if (pk.word[j] == o) { const uint32_t y = k[j] - pk.min[j]; bad |= y > pk.mask[j] ? 1u : 0u; w |= (y & pk.mask[j]) << pk.shift[j]; }
                pk.out[o][i] = w;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 128 && lbin[threadIdx.x]) atomicAdd(&lc.cnt[threadIdx.x], lbin[threadIdx.x]);
    if constexpr (PACKW) { if (bad) *pk.flag = 1u; }
}

struct WideIn {
    int nkd;                                  // key dwords per row
    const uint32_t* kplane[2 * MAXKEYS];      // partitioned key planes
    const uint32_t* rows;                     // partitioned global row ids
    const void* vcol[MAXACC]; int vesz[MAXACC];   // partitioned value arrays per accumulator (null: the row id)
};
constexpr uint32_t WEMPTY = 0xFFFFu, WEMPTY32 = 0xFFFFFFFFu;
// one workgroup of NT threads per partition (grid-stride); R <= 3 NT = row capacity.  LDS: acc u64[NACC][R] | keys u32[nkd][R] |
// first u32[R] | count u32[R] | table u16[2R] | rep u16[R]; a row's id and values stay in the registers of the thread that loaded it.
// The phases are separated by barriers and each is a chain of LDS round trips, so the kernel lives on workgroups per CU: the plan
// sizes a partition for three workgroups of 512 threads where the level structure allows it (pw_plan).
template <int NACC, int NT>
__global__ void __launch_bounds__(NT, NT == 512 ? 6 : 4) pw_agg_kernel(WideIn in, AccSpec as, AggOps ops, const uint32_t* __restrict__ pstart, uint32_t nparts, uint32_t ntotal,
                                                                        uint32_t R, int need_count, GTable out, uint32_t out_cap, uint8_t* __restrict__ dmark, uint32_t* __restrict__ dcount, int mode, int lazy_vals) {
    constexpr int RPT = 3;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint64_t* lacc = reinterpret_cast<uint64_t*>(smem_raw);                    // [NACC][R]
    uint32_t* lkey = reinterpret_cast<uint32_t*>(lacc + (size_t)NACC * R);     // [nkd][R]
    uint32_t* lfirst = lkey + (size_t)in.nkd * R;
    uint32_t* lcount = lfirst + R;
    uint32_t* table = lcount + R;                                              // [2R] slot -> the row that represents the slot's tuple
    uint16_t* rep = reinterpret_cast<uint16_t*>(table + 2 * R);                // [R]
    __shared__ uint32_t lemit, gbase, ngrp;
    const uint32_t T = 2 * R;
    for (uint32_t part = blockIdx.x; part < nparts; part += gridDim.x) {
        const uint32_t b = pstart[part], e = part + 1 < nparts ? pstart[part + 1] : ntotal;
        const uint32_t m = e - b;
        if (!m) continue;
        if (m > R) { if (threadIdx.x == 0) { out.flags[0] = 1; out.flags[4] = part; out.flags[5] = m; } continue; }   // a partition larger than LDS holds: the host falls back (flags 4, 5: which, how large)
        if (mode == 2 && !dmark[part]) continue;                                // second launch: only the partitions the first one put off
        const bool lazy = mode == 1 && lazy_vals;
        uint32_t myrow[RPT];
        uint64_t myval[NACC > 0 ? NACC : 1][RPT];
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const uint32_t i = threadIdx.x + q * NT;
            myrow[q] = 0;
            if (i < m) {
                // all key dwords of the row in flight together (a loop over a run-time number of planes waits for every load before
                // the LDS store behind it: 6 planes x 3 rows = 18 memory latencies in a row per partition)
                uint32_t kv[2 * MAXKEYS];
                _Pragma("unroll") for (int k = 0; k < 2 * MAXKEYS; ++k) if (k < in.nkd) kv[k] = in.kplane[k][b + i];
                _Pragma("unroll") for (int k = 0; k < 2 * MAXKEYS; ++k) if (k < in.nkd) lkey[(size_t)k * R + i] = kv[k];
                if (!lazy) {
                    lfirst[i] = NOROW; lcount[i] = 0;
                    _Pragma("unroll") for (int a = 0; a < NACC; ++a) lacc[(size_t)a * R + i] = acc_init(as.kind[a]);
                    myrow[q] = in.rows[b + i];
                    _Pragma("unroll") for (int a = 0; a < NACC; ++a)
                        myval[a][q] = !in.vcol[a] ? (uint64_t)myrow[q] : in.vesz[a] == 4 ? (uint64_t)static_cast<const uint32_t*>(in.vcol[a])[b + i] : static_cast<const uint64_t*>(in.vcol[a])[b + i];
                }
            }
        }
        for (uint32_t s = threadIdx.x; s < T; s += NT) table[s] = WEMPTY32;
        if (threadIdx.x == 0) { lemit = 0; ngrp = 0; }
        __syncthreads();
        // representative of every row: the first row index that claimed the slot of an equal tuple
        uint32_t mine = 0;
        for (uint32_t i = threadIdx.x; i < m; i += NT) {
            uint32_t h = 0x9E3779B1u;
            for (int k = 0; k < in.nkd; ++k) h = (h ^ lkey[(size_t)k * R + i]) * 0x85EBCA6Bu;
            uint32_t s = __umulhi(h ^ (h >> 15), T);
            uint32_t r = WEMPTY;
            for (uint32_t step = 0; step < T; ++step) {
                uint32_t cur = *reinterpret_cast<volatile uint32_t*>(&table[s]);
                if (cur == WEMPTY32) {                                          // claim the slot for this row (a plain 32-bit compare-and-swap: the 16-bit
                    const uint32_t got = atomicCAS(&table[s], WEMPTY32, i);     //  slots of rounds 2 - 3 took a read-modify-write loop on the pair holding them)
                    cur = got == WEMPTY32 ? i : got;
                }
                bool eq = cur == i;
                if (!eq) { eq = true; for (int k = 0; k < in.nkd && eq; ++k) eq = lkey[(size_t)k * R + cur] == lkey[(size_t)k * R + i]; }
                if (eq) { r = cur; break; }
                s = s + 1 == T ? 0 : s + 1;
            }
            rep[i] = (uint16_t)r;
            mine += r == i;                                                     // groups = rows that represent themselves
        }
        mine = wave_reduce(mine, OpAdd{});
        if (lane_id() == 0 && mine) atomicAdd(&ngrp, mine);
        __syncthreads();
        // mode 1 (the caller can emit straight from the input rows when EVERY row turns out to be its own group -- h2o Q10, any grouping by a
        // unique key): a partition of distinct rows is put off -- marked and counted, nothing accumulated, no records written (32 of the
        // 56 bytes per row this kernel moves).  All partitions put off: the records were never needed.  Otherwise the host launches mode 2
        // over the marked ones.
        if (mode == 1 && ngrp == m) {
            __syncthreads();                                                    // (everybody has read ngrp: the next partition may clear it)
            if (threadIdx.x == 0) { dmark[part] = 1; atomicAdd(dcount, m); }
            continue;
        }
        if (lazy) {                                                             // (the rows are expected to be distinct: ids and values only now, for the partition that has a duplicate)
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                const uint32_t i = threadIdx.x + q * NT;
                if (i >= m) continue;
                myrow[q] = in.rows[b + i];
                lfirst[i] = NOROW; lcount[i] = 0;
                _Pragma("unroll") for (int a = 0; a < NACC; ++a) {
                    lacc[(size_t)a * R + i] = acc_init(as.kind[a]);
                    myval[a][q] = !in.vcol[a] ? (uint64_t)myrow[q] : in.vesz[a] == 4 ? (uint64_t)static_cast<const uint32_t*>(in.vcol[a])[b + i] : static_cast<const uint64_t*>(in.vcol[a])[b + i];
                }
            }
            __syncthreads();                                                    // (the accumulators of all rows are initialised before the first is used)
        }
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
            const uint32_t i = threadIdx.x + q * NT;
            if (i >= m) continue;
            const uint32_t r = rep[i];
            atomicMin(&lfirst[r], myrow[q]);
            if (need_count) atomicAdd(&lcount[r], 1u);
            _Pragma("unroll") for (int a = 0; a < NACC; ++a) {
                uint64_t* acc = lacc + (size_t)a * R + r;
                const uint64_t x = myval[a][q];
                switch (ops.opc[a]) {
                case OPC_ADDI_I32: atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)(long long)(int32_t)(uint32_t)x); break;
                case OPC_ADDI_U32: atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)(uint32_t)x); break;
                case OPC_ADDF_F32: atomicAdd(reinterpret_cast<double*>(acc), (double)__uint_as_float((uint32_t)x)); break;
                case OPC_ADDF_F64: atomicAdd(reinterpret_cast<double*>(acc), __builtin_bit_cast(double, x)); break;
                default: acc_apply(acc, as.kind[a], val_operand_bits(as.dt[a] == AQG_NONE ? AQG_UINT32 : as.dt[a], x, as.kind[a], as.square[a], as.part[a])); break;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) gbase = atomicAdd(&out.flags[1], ngrp);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < m; i += NT) {
            if (rep[i] != i) continue;
            const uint32_t g = gbase + atomicAdd(&lemit, 1u);
            if (g >= out_cap) { out.flags[0] = 1; continue; }
            if (out.kb) *out.key_p(g) = (uint64_t)lfirst[i];                   // wide tuples: the key word is a representative ROW (null: the ordering tail takes the first-row plane)
            *out.first_p(g) = lfirst[i];
            *out.count_p(g) = need_count ? lcount[i] : 0;
            _Pragma("unroll") for (int a = 0; a < NACC; ++a) *out.acc_p(a, g) = lacc[(size_t)a * R + i];
        }
        __syncthreads();
    }
}

} // namespace

// ---- wide tuples: host ----------------------------------------------------------------------------------------------------------------
struct WidePlan { uint32_t R, P, B1; int L, nkd, low[3], nt; size_t lds; bool ok; };   // low[l]: bits of level l + 1 (the levels below the first)
static size_t pw_row_lds(int nkd, int nacc) { return 4 * (size_t)nkd + 4 + 4 + 8 * (size_t)nacc + 8 + 2; }   // key dwords | first | count | accumulators | two 4-byte slots | representative
// `hint` = the expected number of groups: with m = n / hint rows per tuple the rows of a partition are not independent -- the tuples are --
// and the spread of a partition's ROW count grows to sqrt(mean * m) (every tuple brings its m rows along); sizing by sqrt(mean) alone sent
// every table of multi-row tuples through two overflowing attempts to the HBM table (3.2e6 rows, 1.26e6 tuples: partitions at mean + 7 sigma)
static WidePlan pw_plan(const KeySpec& ks, const AccSpec& as, uint32_t n, uint32_t hint, int packed_nkd = 0 /* key dword planes when the tuple travels packed */) {
    WidePlan best;
    memset(&best, 0, sizeof best);
    int nkd = 0;
    for (int k = 0; k < ks.nkeys; ++k) nkd += aqg_dtype_size(ks.dt[k]) <= 4 ? 1 : 2;
    if (packed_nkd > 0 && packed_nkd < nkd) nkd = packed_nkd;
    if (nkd > 2 * MAXKEYS) return best;
    // workgroups per CU: three of 512 threads, two of 1024, one of 1024 -- the first that needs no more levels than the last
    // (four workgroups of 512 -- 39 KB each, 128 x 128 x 128 partitions of ~720 rows -- measured 39 ms against 24-26 for three)
    const struct { size_t budget; int nt; } shapes[3] = {{52 * 1024, 512}, {78 * 1024, 1024}, {AGG_LDS, 1024}};
    for (int si = 2; si >= 0; --si) {
        WidePlan w;
        memset(&w, 0, sizeof w);
        w.nkd = nkd; w.nt = shapes[si].nt;
        uint32_t R = (uint32_t)((shapes[si].budget - 64) / pw_row_lds(nkd, as.nacc));
        if (R > 3u * (uint32_t)w.nt) R = 3u * (uint32_t)w.nt;
        R &= ~7u;
        double mu = (double)R;
        const double sigmas = aqg_switches().pw_sigma;     // (tests: a small value makes partitions overflow by chance)
        const double mult = hint && hint < n ? (double)n / (double)hint : 1.0;
        for (int it = 0; it < 8; ++it) mu = (double)R - sigmas * sqrt((mu > 1 ? mu : 1) * mult);   // (a million partitions: five sigma leave a quarter of the calls with one partition over)
        if (mu < 64) continue;
        const uint64_t P = (uint64_t)((double)n / mu) + 1;
        w.R = R;
        w.lds = (size_t)R * pw_row_lds(nkd, as.nacc) + 64;
        int lowsum = 0;
        if (P <= 128) w.L = 1;
        else if (P <= 128 * 128) { w.L = 2; w.low[0] = P <= 128 * 64 ? 6 : 7; lowsum = w.low[0]; }
        else if (P <= 128 * 128 * 128) { w.L = 3; w.low[0] = P <= 128 * 64 * 128 ? 6 : 7; w.low[1] = P <= 128 * 64 * 64 ? 6 : 7; lowsum = w.low[0] + w.low[1]; }
        else continue;
        w.B1 = (uint32_t)((P + ((uint64_t)1 << lowsum) - 1) >> lowsum);
        w.P = w.B1 << lowsum;
        w.ok = true;
        if (!best.ok || w.L <= best.L) best = w;
    }
    return best;
}
bool aqg_partitionw_applies(const KeySpec& ks, const AccSpec& as, uint32_t n, uint32_t hint) { return ks.wide && pw_plan(ks, as, n, hint).ok; }
uint32_t aqg_partitionw_rows(const KeySpec& ks, const AccSpec& as, uint32_t n, uint32_t hint) { return pw_plan(ks, as, n, hint).R; }

size_t aqg_partitionw_ws_bytes(const aqg_ctx* ctx, const KeySpec& ks, uint32_t n, const AccSpec& as, uint32_t hint) {
    const WidePlan w = pw_plan(ks, as, n, hint);
    ValCols vc;
    p1_val_cols(as, &vc);
    size_t per_row = 4 + 2 * (4 + 4 + 4 * (size_t)w.nkd);                    // the hash column; two sets of {hash, row, key dwords}
    for (int k = 0; k < ks.nkeys; ++k) if (aqg_dtype_size(ks.dt[k]) < 4) per_row += 4;       // widened key columns
    for (int u = 0; u < vc.n; ++u) per_row += 2 * part_val_bytes(vc.dt[u]) + (aqg_dtype_size(vc.dt[u]) < 4 ? 4 : 0);
    return ((size_t)n + 64) * per_row + 256 * (16 + 8 * MAXACC + 8 * MAXKEYS) + ((size_t)w.P + 4096) * 24 + ((size_t)n / P2_PT + (size_t)w.P + 64) * 8 + ((size_t)w.P + 8192) + 65536;   // (… + the put-off marks of pw_agg)
}

// the packing of wide tuples (PackW): fields by first fit, widest first; worth it when a third of the dword planes goes
static bool plan_packw(aqg_ctx* ctx, const KeySpec& ks, uint32_t n, PackW* pk, int* err) {
    memset(pk, 0, sizeof *pk);
    *err = AQG_OK;
    if (n < (1u << 22) || ks.nkeys < 3) return false;
    for (int k = 0; k < ks.nkeys; ++k) if (!(ks.dt[k] == AQG_INT32 || ks.dt[k] == AQG_UINT32) || ((uintptr_t)ks.col[k] & 15)) return false;
    long long mins[MAXKEYS], maxs[MAXKEYS];
    bool ok = false;
    *err = aqg_key_ranges(ctx, ks, 1u << 20, mins, maxs, &ok, n);           // (a sample spread over the column: every row is verified while it is packed)
    if (*err != AQG_OK || !ok) return false;
    int bits[MAXKEYS], order[MAXKEYS];
    for (int k = 0; k < ks.nkeys; ++k) {
        // the sample rarely holds a column's extremes (ids 1 .. 1e7: the first 2^20 rows start near 10): a little room on both sides, and a
        // non-negative column that starts near zero is measured from zero -- a value BELOW the offset would wrap into a miss
        const long long span = maxs[k] - mins[k], room = span / 64 + 8;
        mins[k] = mins[k] >= 0 && mins[k] <= span + room ? 0 : mins[k] - room;
        maxs[k] += room;
        const unsigned long long range = (unsigned long long)(maxs[k] - mins[k]);
        int b = 1;
        while (b < 32 && (1ull << b) <= range) ++b;
        bits[k] = b; order[k] = k;
    }
    for (int i = 1; i < ks.nkeys; ++i) for (int j = i; j > 0 && bits[order[j]] > bits[order[j - 1]]; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
    auto fit = [&](int extra, int* word, int* shift) -> int {                // dword planes needed with `extra` bits of slack per field
        int used[MAXKEYS] = {0}, nw = 0;
        for (int i = 0; i < ks.nkeys; ++i) {
            const int k = order[i], b = bits[k] + extra > 32 ? 32 : bits[k] + extra;
            int o = 0;
            while (o < nw && used[o] + b > 32) ++o;
            if (o == nw) ++nw;
            word[k] = o; shift[k] = used[o]; used[o] += b;
        }
        return nw;
    };
    int word[MAXKEYS], shift[MAXKEYS];
    const int tight = fit(0, word, shift);
    if (tight > 4 || tight * 3 > ks.nkeys * 2) return false;
    int extra = 0;
    if (fit(1, word, shift) == tight) extra = 1; else fit(0, word, shift);     // a bit of slack per field when it costs no plane
    pk->nout = tight;
    for (int k = 0; k < ks.nkeys; ++k) {
        const int b = bits[k] + extra > 32 ? 32 : bits[k] + extra;
        pk->min[k] = (uint32_t)mins[k]; pk->mask[k] = b >= 32 ? 0xFFFFFFFFu : (1u << b) - 1; pk->word[k] = word[k]; pk->shift[k] = shift[k];
    }
    return true;
}

int aqg_partitionw_aggregate(aqg_ctx* ctx, const KeySpec& ks, const AccSpec& as, uint32_t n, int need_count, GTable out, uint32_t out_cap, uint32_t seed, uint32_t hint, int* pack, uint32_t* rows_out, bool may_defer) {
    WidePlan w = pw_plan(ks, as, n, hint);
    if (!w.ok) return aqg_fail(ctx, AQG_ERR_OVERFLOW, "wide-tuple partitioned group-by: the input does not fit 128 x 128 x 128 partitions");
    ValCols vc;
    p1_val_cols(as, &vc);
    const unsigned g4 = aqg_grid(ctx, n, 256, 4, 16);
    // the partition key: a 32-bit hash of the tuple
    uint32_t* h32;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &h32));
    PackW pk;
    bool packed = false, level1_counted = false;
    uint32_t *seg = nullptr, *tp = nullptr, *cnt = nullptr, *cur = nullptr, *bsum = nullptr;
    size_t maxseg = 0;
    {
        Keys32 k32;
        memset(&k32, 0, sizeof k32);
        bool all32 = true;
        for (int k = 0; k < ks.nkeys; ++k) {
            all32 = all32 && aqg_dtype_size(ks.dt[k]) == 4 && ((uintptr_t)ks.col[k] & 15) == 0;
            k32.col[k] = static_cast<const uint32_t*>(ks.col[k]);
        }
        k32.n = ks.nkeys;
        memset(&pk, 0, sizeof pk);
        if (all32 && pack && *pack) {
            int err = AQG_OK;
            packed = plan_packw(ctx, ks, n, &pk, &err);
            AQG_TRY(err);
        }
        if (packed) {                                     // fewer key dwords per row: more rows per partition, fewer partitions (the workspace was sized for the unpacked plan: more of each)
            const WidePlan wp = pw_plan(ks, as, n, hint, pk.nout);
            if (wp.ok && wp.P <= w.P) w = wp;
        }
        // level bookkeeping (segments of level l = the bins of level l - 1); the 32-bit hash passes count the first level's bins themselves
        maxseg = (size_t)w.P + 2;
        AQG_TRY(aqg_ws_get(ctx, maxseg, &seg));
        AQG_TRY(aqg_ws_get(ctx, maxseg, &tp));
        AQG_TRY(aqg_ws_get(ctx, maxseg, &cnt));
        AQG_TRY(aqg_ws_get(ctx, maxseg, &cur));
        AQG_TRY(aqg_ws_get(ctx, maxseg / 2048 + 64, &bsum));
        uint32_t shift1 = 0;
        for (int j = 1; j < w.L; ++j) shift1 += (uint32_t)w.low[j - 1];
        const Level1Count lc{cnt, w.P, shift1};
        level1_counted = all32 && w.B1 <= 128;
        if (level1_counted) AQG_HIP(ctx, hipMemsetAsync(cnt, 0, ((size_t)w.B1 + 1) * 4, ctx->stream));
        if (packed) {
            for (int o = 0; o < pk.nout; ++o) AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &pk.out[o]));
            pk.flag = out.flags + 6;
            hipLaunchKernelGGL(pw_hash32_kernel<true>, dim3(aqg_grid(ctx, n / 4 + 1, 256, 2, 16)), dim3(256), 0, ctx->stream, k32, n, seed, h32, pk, lc);
        }
        else if (all32) hipLaunchKernelGGL(pw_hash32_kernel<false>, dim3(aqg_grid(ctx, n / 4 + 1, 256, 2, 16)), dim3(256), 0, ctx->stream, k32, n, seed, h32, pk, lc);
        else hipLaunchKernelGGL(pw_hash_kernel, dim3(g4), dim3(256), 0, ctx->stream, ks, n, seed, h32);
    }
    if (pack) *pack = packed ? 1 : 0;
    if (rows_out) *rows_out = w.R;
    const int nkd = packed ? pk.nout : w.nkd;             // key dword planes that travel
    // source planes: the key columns as dwords (1- / 2-byte ones widened, 8-byte ones as two planes), then the distinct value columns
    struct Src { const void* p; int stride, off, bytes; };
    std::vector<Src> ksrc, vsrc;
    if (packed) for (int o = 0; o < pk.nout; ++o) ksrc.push_back({pk.out[o], 1, 0, 4});
    for (int k = 0; k < ks.nkeys && !packed; ++k) {
        const int esz = (int)aqg_dtype_size(ks.dt[k]);
        const void* col = ks.col[k];
        if (esz < 4) {
            void* wide;
            AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * 4, &wide));
            aqg_widen_column(ctx, col, esz, n, static_cast<uint32_t*>(wide));
            col = wide;
        }
        if (esz <= 4) ksrc.push_back({col, 1, 0, 4});
        else { ksrc.push_back({col, 2, 0, 4}); ksrc.push_back({col, 2, 1, 4}); }
    }
    for (int u = 0; u < vc.n; ++u) {
        const int esz = (int)aqg_dtype_size(vc.dt[u]);
        const void* col = vc.col[u];
        if (esz < 4) {
            void* wide;
            AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * 4, &wide));
            aqg_widen_column(ctx, col, esz, n, static_cast<uint32_t*>(wide));
            col = wide;
        }
        vsrc.push_back({col, 1, 0, (int)part_val_bytes(vc.dt[u])});
    }
    // two buffer sets: hash | row | key dwords | values
    struct Set { uint32_t* hash; uint32_t* rows; uint32_t* kd[2 * MAXKEYS]; void* val[MAXACC]; } set[2];
    for (int i = 0; i < 2; ++i) {
        AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &set[i].hash));
        AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &set[i].rows));
        for (int k = 0; k < nkd; ++k) AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &set[i].kd[k]));
        for (int u = 0; u < vc.n; ++u) AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * vsrc[u].bytes, &set[i].val[u]));
    }
    auto planes = [&](int level, const Set* from, const Set& to) {
        Planes pl;
        memset(&pl, 0, sizeof pl);
        pl.add(PL_LOAD, level == 1 ? h32 : from->hash, 1, 0, level == w.L ? nullptr : to.hash, 1, 0);     // (nobody reads the hash behind the last level)
        if (level == 1) pl.add(PL_ROWIDX, nullptr, 0, 0, to.rows, 1, 0); else pl.add(PL_LOAD, from->rows, 1, 0, to.rows, 1, 0);
        for (int k = 0; k < nkd; ++k) {
            if (level == 1) pl.add(PL_LOAD, ksrc[k].p, ksrc[k].stride, ksrc[k].off, to.kd[k], 1, 0);
            else pl.add(PL_LOAD, from->kd[k], 1, 0, to.kd[k], 1, 0);
        }
        for (int u = 0; u < vc.n; ++u) pl.add_column(level == 1 ? vsrc[u].p : from->val[u], to.val[u], vsrc[u].bytes);
        return pl;
    };
    if (2 + nkd + 2 * vc.n > MAXPL) return aqg_fail(ctx, AQG_ERR_ARG, "wide-tuple partitioned group-by: too many planes");
    const uint32_t h0[2] = {0u, n};
    void* st = nullptr;
    AQG_TRY(aqg_host_stage(ctx, 16, &st));
    memcpy(st, h0, 8);
    AQG_HIP(ctx, hipMemcpyAsync(seg, st, 8, hipMemcpyHostToDevice, ctx->stream));
    const LevelBufs lb{seg, tp, cnt, cur, bsum};
    uint32_t nseg = 1;
    const Set* from = nullptr;
    int to = 0;
    for (int l = 1; l <= w.L; ++l) {
        uint32_t shift = 0;
        for (int j = l; j < w.L; ++j) shift += (uint32_t)w.low[j - 1];          // bits of the levels below this one
        const uint32_t nb = l == 1 ? w.B1 : 1u << w.low[l - 2], mask = l == 1 ? 0xFFFFFFFFu : nb - 1;
        const uint32_t* keys = l == 1 ? h32 : from->hash;
        AQG_TRY(aqg_scatter_level_counted(ctx, lb, BIN_HASHED, l == 1 && level1_counted, keys, planes(l, from, set[to]), n, nseg, w.P, shift, mask, nb, "wide-tuple partition level"));
        nseg *= nb;
        from = &set[to];
        to ^= 1;
    }
    // ---- aggregate every partition inside LDS -----------------------------------------------------------------------------------------
    WideIn in;
    memset(&in, 0, sizeof in);
    in.nkd = nkd;
    for (int k = 0; k < nkd; ++k) in.kplane[k] = from->kd[k];
    in.rows = from->rows;
    AggOps ops;
    memset(&ops, 0, sizeof ops);
    for (int a = 0; a < as.nacc; ++a) {
        if (vc.of_acc[a] >= 0) { in.vcol[a] = from->val[vc.of_acc[a]]; in.vesz[a] = vsrc[vc.of_acc[a]].bytes; }
        else { in.vcol[a] = nullptr; in.vesz[a] = 4; }
        ops.opc[a] = p1_opcode(as.dt[a], as.kind[a], as.square[a], as.part[a], true);
    }
    const size_t lds = w.lds;
    unsigned per_cu = (unsigned)((160 * 1024) / (lds + 512));
    if (per_cu > 2048u / (unsigned)w.nt) per_cu = 2048u / (unsigned)w.nt;
    if (per_cu < 1) per_cu = 1;
    const unsigned grid = nseg < per_cu * (unsigned)ctx->num_cu ? nseg : per_cu * (unsigned)ctx->num_cu;
    if (aqg_switches().disable_pw_defer) may_defer = false;
    uint32_t* dwords = nullptr;                                                            // [0] rows of the partitions put off | marks, a byte per partition
    if (may_defer) {
        AQG_TRY(aqg_ws_get(ctx, (size_t)nseg / 4 + 8, &dwords));
        AQG_HIP(ctx, hipMemsetAsync(dwords, 0, ((size_t)nseg / 4 + 8) * 4, ctx->stream));
    }
    uint8_t* dmark = may_defer ? reinterpret_cast<uint8_t*>(dwords + 4) : nullptr;
    const int lazy_vals = may_defer && (uint64_t)hint * 10 >= (uint64_t)n * 9 ? 1 : 0;     // nearly as many groups expected as rows: row ids and values are read only where a partition has a duplicate
    auto launch = [&](auto kern) -> int {
        AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
        aqg_kernel_timer_begin(ctx);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(w.nt), lds, ctx->stream, in, as, ops, (const uint32_t*)seg, nseg, n, w.R, need_count, out, out_cap, dmark, dwords, may_defer ? 1 : 0, lazy_vals);
        aqg_kernel_timer_end(ctx);
        AQG_TRY(aqg_check_launch(ctx, "pw_agg_kernel"));
        if (!may_defer) return AQG_OK;
        // every row its own group?  (one host round trip on a call of tens of milliseconds)
        uint32_t fl[2] = {0, 0}, put_off = 0;
        AQG_HIP(ctx, hipMemcpyAsync(fl, out.flags, 8, hipMemcpyDeviceToHost, ctx->stream));
        AQG_HIP(ctx, hipMemcpyAsync(&put_off, dwords, 4, hipMemcpyDeviceToHost, ctx->stream));
        AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (fl[0] || !put_off) return AQG_OK;                                               // (an overflow is the caller's to judge)
        if ((uint64_t)fl[1] + put_off == n) {                                               // yes: the caller emits from the rows, the record table is not read
            AQG_HIP(ctx, hipMemcpyAsync(out.flags + 1, &n, 4, hipMemcpyHostToDevice, ctx->stream));
            AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));                                // (`n` lives on this stack frame)
            return AQG_OK;
        }
        hipLaunchKernelGGL(kern, dim3(grid), dim3(w.nt), lds, ctx->stream, in, as, ops, (const uint32_t*)seg, nseg, n, w.R, need_count, out, out_cap, dmark, dwords, 2, 0);
        return aqg_check_launch(ctx, "pw_agg_kernel (partitions put off)");
    };
    auto pick = [&](auto nacc) -> int {
        constexpr int N = decltype(nacc)::value;
        return w.nt == 512 ? launch(&pw_agg_kernel<N, 512>) : launch(&pw_agg_kernel<N, 1024>);
    };
    switch (as.nacc) {
    case 0: return pick(std::integral_constant<int, 0>{});
    case 1: return pick(std::integral_constant<int, 1>{});
    case 2: return pick(std::integral_constant<int, 2>{});
    case 3: return pick(std::integral_constant<int, 3>{});
    case 4: return pick(std::integral_constant<int, 4>{});
    default: return aqg_fail(ctx, AQG_ERR_OVERFLOW, "wide-tuple partitioned group-by: at most 4 accumulators");
    }
}

// ==== grouped reductions keyed by DENSE group ids: aqg_grouped_reduce beyond the LDS tables =============================================
// `out[g] = op(x[rows of group g])` for the generated loop (engine/ast.py:722-789) groups by the build's id column.  Those ids are dense
// and the group sizes are known, which the hashed partition plans above cannot use: here the rows {id, value} are partitioned on the id
// itself -- ORDER-PRESERVING bins umulhi(id, M), so a partition owns a contiguous id range -- with the tile scatter of the two-level
// plan, in as many levels of <= 128 bins as it takes until a partition's id range fits an LDS array of accumulators.  No histogram
// pass at any level: a partition's rows are the rows of its groups, so every segment start and write cursor is an entry of the
// build's offsets (the exclusive scan of the group sizes).  The aggregation is then DIRECT-indexed -- acc[id - first id of the
// partition], no keys, no probing -- and every workgroup writes its id range of the result column front to back: no record table, no
// ranking, no emit.  16 B/row and level + 8 B/row for the aggregation (1e9 rows, 1e7 groups: two levels).
// (In this file, not one of its own: gid_agg_kernel and pw_agg_kernel both inline val_operand_bits, and hipcc specialises a device function per
// translation unit for the arguments that file's callers pass.  Alone in a file, where every caller passes part = 0, gid_agg_kernel comes out as
// different code -- its 64-bit integer operand; next to pw_agg_kernel it is the code that has been measured.)
namespace {

__global__ void __launch_bounds__(256) gid_setup_kernel(const uint32_t* __restrict__ offsets, uint32_t G, uint32_t M, uint32_t PP,
                                                        uint32_t* __restrict__ pstart /* [PP + 1] */, uint32_t* __restrict__ pfirst /* [PP + 1] */) {
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p <= PP; p += gridDim.x * 256) {
        uint64_t g0 = p == PP ? G : (((uint64_t)p << 32) + M - 1) / M;        // smallest id whose bin is >= p
        if (g0 > G) g0 = G;
        pfirst[p] = (uint32_t)g0;
        pstart[p] = offsets ? offsets[g0] : (uint32_t)g0;
    }
}

struct GidAgg {
    const uint32_t* gid; const void* val; int vdt; int op;
    const uint32_t* pstart; const uint32_t* pfirst; const uint32_t* counts;
    void* out; uint32_t nparts, cap, ntotal; int opc;
    // the value travelled INSIDE the id word (a 4-byte integer column of a narrow sampled range above the id's bits): word = id | (v - pmin) << pshift
    uint32_t packed, idmask, pshift, pmin;
};
// value of row i as the operand of accumulator `which` (0: the value, 1: its square in the promoted type) -- wave-uniform dtype switch
__device__ inline uint64_t gid_operand(const GidAgg& a, size_t i, int kind, int square) {
    switch (a.vdt) {
    case AQG_INT8: return val_operand_t((int8_t)(uint8_t)static_cast<const uint32_t*>(a.val)[i], kind, square);      // (1- / 2-byte columns travel widened)
    case AQG_INT16: return val_operand_t((int16_t)(uint16_t)static_cast<const uint32_t*>(a.val)[i], kind, square);
    case AQG_UINT8: case AQG_BOOL: return val_operand_t((uint8_t)static_cast<const uint32_t*>(a.val)[i], kind, square);
    case AQG_UINT16: return val_operand_t((uint16_t)static_cast<const uint32_t*>(a.val)[i], kind, square);
    case AQG_INT32: return val_operand_t(static_cast<const int32_t*>(a.val)[i], kind, square);
    case AQG_UINT32: return val_operand_t(static_cast<const uint32_t*>(a.val)[i], kind, square);
    case AQG_FLOAT: return val_operand_t(static_cast<const float*>(a.val)[i], kind, square);
    case AQG_INT64: return val_operand_t(static_cast<const int64_t*>(a.val)[i], kind, square);
    case AQG_UINT64: return val_operand_t(static_cast<const uint64_t*>(a.val)[i], kind, square);
    default: return val_operand_t(static_cast<const double*>(a.val)[i], kind, square);
    }
}
// V8: 8-byte values.  A lane takes GR consecutive rows of a step by 16-byte loads (4-byte aligned: a partition starts anywhere) and the next
// step's rows are in flight while this step's are accumulated -- with four rows per lane and step by dword loads, one step at a time, the
// kernel read at 1.95 TB/s (h2o v3 at 1e9 rows / 1e7 groups: 4.1 of the call's 10.6 ms).
template <bool V8>
__global__ void __launch_bounds__(1024, 8) gid_agg_kernel(GidAgg a) {      // (eight wavefronts per SIMD: two workgroups per CU)
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint64_t* acc0 = reinterpret_cast<uint64_t*>(smem_raw);
    uint64_t* acc1 = acc0 + a.cap;
    const bool two = a.op == AQG_RED_VAR || a.op == AQG_RED_STDDEV;
    const int vc = vclass(a.vdt);
    const int kind = a.op == AQG_RED_MIN ? ACC_MIN : a.op == AQG_RED_MAX ? ACC_MAX : vc == VC_F ? ACC_ADD_F : ACC_ADD_I;
    for (uint32_t p = blockIdx.x; p < a.nparts; p += gridDim.x) {
        const uint32_t g0 = a.pfirst[p], width = a.pfirst[p + 1] - g0;
        const uint32_t r0 = a.pstart[p], r1 = a.pstart[p + 1];
        for (uint32_t j = threadIdx.x; j < width; j += 1024) { acc0[j] = acc_init(kind); if (two) acc1[j] = 0; }
        __syncthreads();
        if (r0 < r1) {
            using VT = std::conditional_t<V8, uint64_t, uint32_t>;
            constexpr int GR = V8 ? 4 : 8;
            constexpr uint32_t STEP = 1024 * GR;
            struct Batch { uint32_t w[GR]; VT x[GR]; };
            const bool has_val = !a.packed;
            auto load_full = [&](uint32_t i0, Batch& t) {
                const uint32_t o = i0 + threadIdx.x * GR;
                __builtin_memcpy(t.w, a.gid + o, sizeof t.w);
                if (has_val) __builtin_memcpy(t.x, static_cast<const VT*>(a.val) + o, sizeof t.x);
            };
            auto load_edge = [&](uint32_t i0, Batch& t) {
                const uint32_t o = i0 + threadIdx.x * GR;
#pragma unroll
                for (int k = 0; k < GR; ++k) {
                    const uint32_t i = o + k < r1 ? o + k : r1 - 1;
                    t.w[k] = a.gid[i];
                    if (has_val) t.x[k] = static_cast<const VT*>(a.val)[i];
                }
            };
            const uint32_t nfull = (r1 - r0) / STEP, nsteps = nfull + ((r1 - r0) % STEP ? 1u : 0u);
            const uint32_t safe_last = nfull ? r0 + (nfull - 1) * STEP : (r0 + STEP <= a.ntotal ? r0 : a.ntotal - STEP);   // a whole step inside the arrays, for the prefetch that has nothing left to fetch
            Batch cur;
            load_full(nfull ? r0 : safe_last, cur);
            uint32_t i0 = r0;
            for (uint32_t st = 0; st < nsteps; ++st, i0 += STEP) {
                const bool edge = st >= nfull;
                if (edge) load_edge(i0, cur);
                Batch nxt;
                load_full(st + 1 < nfull ? i0 + STEP : safe_last, nxt);
                __builtin_amdgcn_sched_barrier(0);
                const uint32_t o = i0 + threadIdx.x * GR;
                if (has_val && !two && a.opc != OPC_GENERIC) {                  // plain sums: straight-line rows (entry cap - 1 is nobody's: rows beyond the edge go there)
                    uint32_t g[GR];
#pragma unroll
                    for (int k = 0; k < GR; ++k) g[k] = edge && !(o + k < r1) ? a.cap - 1 : (cur.w[k] & a.idmask) - g0;
                    switch (a.opc) {
                    case OPC_ADDI_I32:
#pragma unroll
                        for (int k = 0; k < GR; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(&acc0[g[k]]), (unsigned long long)(long long)(int32_t)(uint32_t)cur.x[k]);
                        break;
                    case OPC_ADDI_U32:
#pragma unroll
                        for (int k = 0; k < GR; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(&acc0[g[k]]), (unsigned long long)(uint32_t)cur.x[k]);
                        break;
                    case OPC_ADDF_F32:
#pragma unroll
                        for (int k = 0; k < GR; ++k) atomicAdd(reinterpret_cast<double*>(&acc0[g[k]]), (double)__uint_as_float((uint32_t)cur.x[k]));
                        break;
                    default:
#pragma unroll
                        for (int k = 0; k < GR; ++k) atomicAdd(reinterpret_cast<double*>(&acc0[g[k]]), __builtin_bit_cast(double, (uint64_t)cur.x[k]));
                        break;
                    }
                } else
#pragma unroll
                for (int k = 0; k < GR; ++k) {
                    if (edge && !(o + k < r1)) continue;
                    const uint32_t g = (cur.w[k] & a.idmask) - g0;
                    uint64_t v, q = 0;
                    if (a.packed) {
                        const uint32_t raw = (cur.w[k] >> a.pshift) + a.pmin;
                        v = a.vdt == AQG_INT32 ? val_operand_t((int32_t)raw, kind, 0) : val_operand_t(raw, kind, 0);
                        if (two) q = a.vdt == AQG_INT32 ? val_operand_t((int32_t)raw, kind, 1) : val_operand_t(raw, kind, 1);
                    } else {
                        v = val_operand_bits(a.vdt, (uint64_t)cur.x[k], kind, 0, 0);
                        if (two) q = val_operand_bits(a.vdt, (uint64_t)cur.x[k], kind, 1, 0);
                    }
                    acc_apply(&acc0[g], kind, v);
                    if (two) acc_apply(&acc1[g], kind, q);
                }
                cur = nxt;
            }
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < width; j += 1024) {
            const uint32_t gg = g0 + j;
            const uint64_t s = acc0[j];
            switch (a.op) {
            case AQG_RED_SUM:
                if (vc == VC_F) static_cast<double*>(a.out)[gg] = __builtin_bit_cast(double, s);
                else static_cast<aqg_i128*>(a.out)[gg] = vc == VC_U ? i128_from_u64(s) : i128_from_i64((int64_t)s);
                break;
            case AQG_RED_AVG: {
                const double sd = vc == VC_F ? __builtin_bit_cast(double, s) : vc == VC_U ? (double)s : (double)(int64_t)s;
                static_cast<double*>(a.out)[gg] = sd / (double)a.counts[gg];
            } break;
            case AQG_RED_VAR: case AQG_RED_STDDEV: {                            // (ssq - s * s / (n + 1)) / (n + 1): D9 kept
                const double np1 = (double)(uint32_t)(a.counts[gg] + 1);
                double d;
                if (vc == VC_F) { const double sd = __builtin_bit_cast(double, s), qd = __builtin_bit_cast(double, acc1[j]); d = (qd - sd * sd / np1) / np1; }
                else {
                    const aqg_i128 sm = vc == VC_U ? i128_from_u64(s) : i128_from_i64((int64_t)s);
                    // (uint16: the int squares wrap negative and the reference adds them sign-extended to its unsigned 128-bit sum)
                    const aqg_i128 qq = vc == VC_U && a.vdt != AQG_UINT16 ? i128_from_u64(acc1[j]) : i128_from_i64((int64_t)acc1[j]);
                    const aqg_i128 ss = i128_mul(sm, sm);
                    const double sq = vc == VC_U ? u128_to_double(ss.hi, ss.lo) : i128_to_double(ss);
                    const double qdd = vc == VC_U ? u128_to_double(qq.hi, qq.lo) : i128_to_double(qq);
                    d = (qdd - sq / np1) / np1;
                }
                static_cast<double*>(a.out)[gg] = a.op == AQG_RED_STDDEV ? sqrt(d) : d;
            } break;
            default: {
                const bool mx = a.op == AQG_RED_MAX;
                switch (a.vdt) {
                case AQG_INT8: store_minmax<int8_t>(a.out, gg, s, mx); break;
                case AQG_INT16: store_minmax<int16_t>(a.out, gg, s, mx); break;
                case AQG_INT32: store_minmax<int32_t>(a.out, gg, s, mx); break;
                case AQG_INT64: store_minmax<int64_t>(a.out, gg, s, mx); break;
                case AQG_UINT8: case AQG_BOOL: store_minmax<uint8_t>(a.out, gg, s, mx); break;
                case AQG_UINT16: store_minmax<uint16_t>(a.out, gg, s, mx); break;
                case AQG_UINT32: store_minmax<uint32_t>(a.out, gg, s, mx); break;
                case AQG_UINT64: store_minmax<uint64_t>(a.out, gg, s, mx); break;
                case AQG_FLOAT: store_minmax<float>(a.out, gg, s, mx); break;
                default: store_minmax<double>(a.out, gg, s, mx); break;
                }
            } break;
            }
        }
        __syncthreads();
    }
}

} // namespace

// pstart / pfirst of the PP order-preserving partitions of the ids 0 .. G-1 (offsets == nullptr: the identity -- aqg_route_by_row's row indices)
void aqg_gid_setup(aqg_ctx* ctx, const uint32_t* offsets, uint32_t G, uint32_t M, uint32_t PP, uint32_t* pstart, uint32_t* pfirst) {
    hipLaunchKernelGGL(gid_setup_kernel, dim3(aqg_grid(ctx, (uint64_t)PP + 1, 256, 1, 4)), dim3(256), 0, ctx->stream, offsets, G, M, PP, pstart, pfirst);
}

// out[g] = op(x[rows whose id is g]) for dense ids 0 .. G-1 with known group sizes (offsets = their exclusive scan, G + 1 entries).
// AQG_ERR_DTYPE: this (op, dtype) is not served here (8-byte integer sums need 128 bits per group): the caller takes the hashed plans.
static int gid_reduce_impl(aqg_ctx* ctx, const uint32_t* gid, const uint32_t* offsets, const uint32_t* counts, uint32_t n, uint32_t G, int op, int t, const void* x, void* out_dev, bool allow_pack);
int aqg_gid_reduce(aqg_ctx* ctx, const uint32_t* gid, const uint32_t* offsets, const uint32_t* counts, uint32_t n, uint32_t G, int op, int t, const void* x, void* out_dev) {
    const int rc = gid_reduce_impl(ctx, gid, offsets, counts, n, G, op, t, x, out_dev, true);
    return rc == -1001 ? gid_reduce_impl(ctx, gid, offsets, counts, n, G, op, t, x, out_dev, false) : rc;     // (a value outside the sampled range of its field: once more, as its own plane)
}
static int gid_reduce_impl(aqg_ctx* ctx, const uint32_t* gid, const uint32_t* offsets, const uint32_t* counts, uint32_t n, uint32_t G, int op, int t, const void* x, void* out_dev, bool allow_pack) {
    const bool two = op == AQG_RED_VAR || op == AQG_RED_STDDEV;
    if (!(op == AQG_RED_SUM || op == AQG_RED_AVG || op == AQG_RED_MIN || op == AQG_RED_MAX || two)) return AQG_ERR_DTYPE;
    const bool wide_int = t == AQG_INT64 || t == AQG_UINT64;
    if (wide_int && op != AQG_RED_MIN && op != AQG_RED_MAX) return AQG_ERR_DTYPE;
    const int esz = (int)aqg_dtype_size(t), vsz = esz == 8 ? 8 : 4;
    // ids of one partition: at most 78 KB of accumulators (two 1024-thread workgroups per CU), and at least 1024 partitions whatever the
    // group count -- the aggregation runs one workgroup per partition (1e5 groups in 8 partitions: 119 ms; in 1024: see DESIGN.md)
    const uint32_t cap_max = two ? 4992u : 9984u;
    uint32_t bits = 10;
    while (bits < 21 && ((uint64_t)G >> bits) + 2 > cap_max) ++bits;
    if (((uint64_t)G >> bits) + 2 > cap_max || G <= (8u << bits)) return AQG_ERR_DTYPE;
    const uint32_t cap = (uint32_t)((uint64_t)G >> bits) + 2;
    const uint32_t levels = (bits + 6) / 7, PP = 1u << bits;
    const uint32_t M = (uint32_t)((((uint64_t)1 << bits) << 32) / G);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, ((size_t)n + 64) * (2 * (4 + (size_t)vsz) + (esz < 4 ? 4 : 0)) + (size_t)PP * 40 + 1048576));
    uint32_t *gA, *gB, *pstart, *pfirst, *seg, *tp, *cur;
    void *vA, *vB;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &gA));
    AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &gB));
    AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * vsz, &vA));
    AQG_TRY(aqg_ws_alloc(ctx, ((size_t)n + 64) * vsz, &vB));
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &pstart));
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &pfirst));
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &seg));
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &tp));
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &cur));
    const void* vsrc = x;
    if (esz < 4) {
        uint32_t* wide;
        AQG_TRY(aqg_ws_get(ctx, (size_t)n + 64, &wide));
        aqg_widen_column(ctx, x, esz, n, wide);
        vsrc = wide;
    }
    // a 4-byte integer value column of a narrow sampled range travels INSIDE the id word (ids below 2^24 leave eight bits: h2o v1, v2): one plane per
    // level instead of two.  Every row is verified while it is packed (p2_scatter's PL_PACK); a miss repeats the call with the value as its own plane.
    uint32_t pk_on = 0, pk_shift = 0, pk_min = 0, pk_mask = 0, *pk_flag = nullptr;
    if (allow_pack && (t == AQG_INT32 || t == AQG_UINT32) && n >= (1u << 22) && ((uintptr_t)x & 15) == 0) {
        KeySpec probe;
        memset(&probe, 0, sizeof probe);
        probe.nkeys = 1; probe.dt[0] = t; probe.col[0] = x;
        long long mn[MAXKEYS], mx[MAXKEYS];
        bool ok = false;
        AQG_TRY(aqg_key_ranges(ctx, probe, 1u << 20, mn, mx, &ok, n));
        int gbits = 1;
        while (gbits < 32 && (1ull << gbits) < (unsigned long long)G) ++gbits;
        if (ok && mx[0] >= mn[0]) {
            const unsigned long long range = (unsigned long long)(mx[0] - mn[0]);
            int fb = 1;
            while (fb < 32 && (1ull << fb) <= range) ++fb;
            if (gbits + fb <= 32) {
                pk_on = 1; pk_shift = (uint32_t)gbits; pk_min = (uint32_t)mn[0]; pk_mask = (uint32_t)((1ull << fb) - 1);
                AQG_TRY(aqg_ws_get(ctx, 16, &pk_flag));
                AQG_HIP(ctx, hipMemsetAsync(pk_flag, 0, 4, ctx->stream));
            }
        }
    }
    const uint32_t kclear = pk_on ? pk_mask << pk_shift : 0u;
    aqg_gid_setup(ctx, offsets, G, M, PP, pstart, pfirst);
    const LevelBufs lb{seg, tp, nullptr, cur, nullptr};
    uint32_t nseg = 1;
    const uint32_t* gsrc = gid;
    const void* vs = vsrc;
    for (uint32_t l = 0; l < levels; ++l) {
        uint32_t shift;
        const uint32_t nb = 1u << aqg_level_bits(bits, levels, l, &shift);
        uint32_t* gdst = (l & 1) ? gB : gA;
        void* vdst = (l & 1) ? vB : vA;
        Planes pl;
        memset(&pl, 0, sizeof pl);
        pl.add_column(gsrc, gdst, 4);
        if (pk_on) {
            if (l == 0) {
                pl.p[0].kind = PL_PACK;
                pl.pk.n = 1; pl.pk.kmax = 0xFFFFFFFFu; pl.pk.flag = pk_flag;
                pl.pk.src[0] = static_cast<const uint32_t*>(x); pl.pk.min[0] = pk_min; pl.pk.shift[0] = pk_shift; pl.pk.fmask[0] = pk_mask;
            }
        }
        else pl.add_column(vs, vdst, vsz);
        // this level's segments are the partitions of the levels before it, its cursors the starts of its own partitions: entries of pstart
        AQG_TRY(aqg_scatter_level_offsets(ctx, lb, pstart, pk_on && l == 0, l == 0 ? 0u : kclear, gsrc, pl, n, nseg, M, shift, nb, "id-partitioned grouped reduce: level"));
        if (pk_on && l == 0) {                                  // a row that did not fit its field: the caller repeats the call unpacked
            uint32_t miss = 0;
            AQG_HIP(ctx, hipMemcpyAsync(&miss, pk_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
            AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (miss) return -1001;
        }
        nseg *= nb;
        gsrc = gdst; vs = vdst;
    }
    GidAgg a;
    a.gid = gsrc; a.val = vs; a.vdt = t; a.op = op; a.pstart = pstart; a.pfirst = pfirst; a.counts = counts; a.out = out_dev; a.nparts = PP; a.cap = cap;
    a.packed = pk_on; a.idmask = pk_on ? ~kclear : 0xFFFFFFFFu; a.pshift = pk_shift; a.pmin = pk_min;
    a.ntotal = n;
    a.opc = op == AQG_RED_SUM || op == AQG_RED_AVG ? p1_opcode(t, vclass(t) == VC_F ? ACC_ADD_F : ACC_ADD_I, 0, 0, true) : OPC_GENERIC;
    if (n < 1024u * 8u) return AQG_ERR_DTYPE;                                 // (the kernel prefetches whole steps of 8192 rows; inputs this small never come here)
    const size_t lds = (size_t)cap * 8 * (two ? 2 : 1);
    auto launch = [&](auto kern) -> int {
        AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
        aqg_kernel_timer_begin(ctx);
        hipLaunchKernelGGL(kern, dim3(PP < 4096 ? PP : 4096), dim3(1024), lds, ctx->stream, a);
        aqg_kernel_timer_end(ctx);
        return aqg_check_launch(ctx, "gid_agg_kernel");
    };
    return vsz == 8 ? launch(&gid_agg_kernel<true>) : launch(&gid_agg_kernel<false>);
}
