// join.hip -- hash equi-join on one integer key column.
// New functionality: the reference emits joins as SQL for MonetDB (engine/ast.py:874-1085) and has no
// C++ join, so the contract is this library's own: inner join, pairs ordered by probe row,
// then by build row ascending (what a probe loop over an aq_map<key, rows> yields).  The reference pins none of it: the
// specification is tests/join_model.py, held to the oracle's restatement by tests/test_join_model.py and to these kernels by
// tests/test_gpu_join.py (sentinel keys, wrapping collision chains, duplicates, table routes, error returns).
//
//   aqg_join_lookup   unique-key dimension lookup (h2o join + group-by, config 4): an open-addressing
//                     table {key -> lowest build row} in HBM (L2-resident for small dimensions); the
//                     probe is one coalesced pass over the fact key column.
//   aqg_join_count / aqg_join_pairs   general inner join: group the build side (aqg_groupby_build +
//                     postproc), look each probe key up among the distinct build keys, prefix-sum the
//                     match counts, expand.
#include "aqg_internal.hpp"
#include "dev_common.hpp"

namespace {

constexpr uint64_t JEMPTY = ~0ull;
constexpr uint32_t NONE = 0xFFFFFFFFu;

// slot of a key in a table of 2^bits slots: 32-bit multiplies only (the probe loop is bound by VALU issue, and a 64-bit multiply
// costs four quarter-rate 32-bit ones); the TOP bits of the product are the well-mixed ones
__device__ inline uint32_t jslot(uint64_t k, uint32_t bits) {
    const uint32_t h = ((uint32_t)k ^ ((uint32_t)(k >> 32) * 0x85EBCA6Bu)) * 0x9E3779B1u;
    return h >> (32 - bits);
}

__device__ inline uint64_t key_bits(int dt, const void* col, size_t i) {   // sign-extended value as the join key
    switch (dt) {
    case AQG_INT8: return (uint64_t)(int64_t) static_cast<const int8_t*>(col)[i];
    case AQG_INT16: return (uint64_t)(int64_t) static_cast<const int16_t*>(col)[i];
    case AQG_INT32: return (uint64_t)(int64_t) static_cast<const int32_t*>(col)[i];
    case AQG_UINT8: case AQG_BOOL: return static_cast<const uint8_t*>(col)[i];
    case AQG_UINT16: return static_cast<const uint16_t*>(col)[i];
    case AQG_UINT32: return static_cast<const uint32_t*>(col)[i];
    default: return static_cast<const uint64_t*>(col)[i];
    }
}

template <class T> __device__ inline void key_bits4_t(const void* col, const size_t (&ix)[4], uint64_t (&k)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const T v = static_cast<const T*>(col)[ix[q]];
        if constexpr (std::is_signed_v<T>) k[q] = (uint64_t)(int64_t)v; else k[q] = (uint64_t)v;
    }
}
__device__ inline void key_bits4(int dt, const void* col, const size_t (&ix)[4], uint64_t (&k)[4]) {
    switch (dt) {
    case AQG_INT8: key_bits4_t<int8_t>(col, ix, k); break;
    case AQG_INT16: key_bits4_t<int16_t>(col, ix, k); break;
    case AQG_INT32: key_bits4_t<int32_t>(col, ix, k); break;
    case AQG_UINT8: case AQG_BOOL: key_bits4_t<uint8_t>(col, ix, k); break;
    case AQG_UINT16: key_bits4_t<uint16_t>(col, ix, k); break;
    case AQG_UINT32: key_bits4_t<uint32_t>(col, ix, k); break;
    default: key_bits4_t<uint64_t>(col, ix, k); break;
    }
}

struct JTable { uint64_t* keys; uint32_t* val; uint32_t cap; uint32_t* sentinel_val; };   // sentinel: the key equal to JEMPTY

__global__ void __launch_bounds__(256) jt_build_kernel(int dt, const void* __restrict__ col, uint32_t n, JTable t) {
    const uint32_t mask = t.cap - 1, bits = 31 - __clz(t.cap);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint64_t k = key_bits(dt, col, i);
        if (k == JEMPTY) { atomicMin(t.sentinel_val, i); continue; }
        uint32_t s = jslot(k, bits);
        for (uint32_t p = 0; p < t.cap; ++p) {
            uint64_t cur = t.keys[s];
            if (cur == JEMPTY) {
                unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&t.keys[s]), JEMPTY, k);
                cur = old == JEMPTY ? k : old;
            }
            if (cur == k) { atomicMin(&t.val[s], i); break; }
            s = (s + 1) & mask;
        }
    }
}
// Probe: R CONSECUTIVE rows per lane per step (16-byte loads of the keys, 16-byte stores of the results; R = 8 for keys up to four
// bytes), every first slot -- key and payload -- read before the first compare; only rows whose first slot holds another key walk on.
// LDS: the whole table is copied into LDS first (dimension sides of a few thousand rows: every probe is an LDS access instead of
// an L2 round trip).
template <bool LDS, class T>
__device__ inline void probe_rows(const T* __restrict__ col, uint32_t n, const JTable& t, const uint64_t* keys, const uint32_t* val, uint32_t* __restrict__ out) {
    const uint32_t mask = t.cap - 1, bits = 31 - __clz(t.cap);
    const uint32_t sentinel = *t.sentinel_val;
    auto key_of = [](T v) -> uint64_t { if constexpr (std::is_signed_v<T>) return (uint64_t)(int64_t)v; else return (uint64_t)v; };
    auto finish = [&](uint64_t k, uint32_t sl, uint64_t c) -> uint32_t {
        if (k == JEMPTY) return sentinel;
        for (uint32_t p = 0; p < t.cap; ++p) {
            if (c == k) return val[sl];
            if (c == JEMPTY) return NONE;
            sl = (sl + 1) & mask;
            c = keys[sl];
        }
        return NONE;
    };
    constexpr int KV = 16 / sizeof(T) > 4 ? 4 : 16 / sizeof(T);          // keys per vector load (at most four: one 16-byte store of results)
    constexpr int R = sizeof(T) <= 4 ? 8 : 4, NKV = R / KV;
    const uint32_t nchunk = n / R;
    const bool aligned = ((reinterpret_cast<uintptr_t>(col) & (sizeof(T) * KV - 1)) | (reinterpret_cast<uintptr_t>(out) & 15)) == 0;
    if (aligned) {
        uint32_t c_lo, c_hi;
        wg_span(nchunk, c_lo, c_hi);
        for (uint32_t c = c_lo + threadIdx.x; c < c_hi; c += blockDim.x) {
            pack<T, KV> kv[NKV];
#pragma unroll
            for (int v = 0; v < NKV; ++v) kv[v] = *reinterpret_cast<const pack<T, KV>*>(col + (size_t)c * R + v * KV);
            uint64_t k[R], cur[R];
            uint32_t s[R], o[R];
#pragma unroll
            for (int q = 0; q < R; ++q) { k[q] = key_of(kv[q / KV].v[q % KV]); s[q] = jslot(k[q], bits); cur[q] = keys[s[q]]; o[q] = val[s[q]]; }
#pragma unroll
            for (int q = 0; q < R; ++q) if (cur[q] != k[q] || k[q] == JEMPTY) o[q] = finish(k[q], s[q], cur[q]);
#pragma unroll
            for (int v = 0; v < R / 4; ++v) {
                pack<uint32_t, 4> ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov.v[e] = o[v * 4 + e];
                *reinterpret_cast<pack<uint32_t, 4>*>(out + (size_t)c * R + v * 4) = ov;
            }
        }
    }
    for (uint32_t i = (aligned ? nchunk * R : 0u) + blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t k = key_of(col[i]);
        const uint32_t sl = jslot(k, bits);
        out[i] = finish(k, sl, keys[sl]);
    }
}
template <bool LDS>
__global__ void __launch_bounds__(256) jt_probe_kernel(int dt, const void* __restrict__ col, uint32_t n, JTable t, uint32_t* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint64_t* lk = reinterpret_cast<uint64_t*>(smem_raw);
    uint32_t* lv = reinterpret_cast<uint32_t*>(lk + (LDS ? t.cap : 0));
    const uint64_t* keys = t.keys;
    const uint32_t* val = t.val;
    if constexpr (LDS) {
        for (uint32_t s = threadIdx.x; s < t.cap; s += blockDim.x) { lk[s] = t.keys[s]; lv[s] = t.val[s]; }
        __syncthreads();
        keys = lk; val = lv;
    }
    switch (dt) {       // one dtype switch per launch, not per row
    case AQG_INT8: probe_rows<LDS>(static_cast<const int8_t*>(col), n, t, keys, val, out); break;
    case AQG_INT16: probe_rows<LDS>(static_cast<const int16_t*>(col), n, t, keys, val, out); break;
    case AQG_INT32: probe_rows<LDS>(static_cast<const int32_t*>(col), n, t, keys, val, out); break;
    case AQG_UINT8: case AQG_BOOL: probe_rows<LDS>(static_cast<const uint8_t*>(col), n, t, keys, val, out); break;
    case AQG_UINT16: probe_rows<LDS>(static_cast<const uint16_t*>(col), n, t, keys, val, out); break;
    case AQG_UINT32: probe_rows<LDS>(static_cast<const uint32_t*>(col), n, t, keys, val, out); break;
    case AQG_INT64: probe_rows<LDS>(static_cast<const int64_t*>(col), n, t, keys, val, out); break;
    default: probe_rows<LDS>(static_cast<const uint64_t*>(col), n, t, keys, val, out); break;
    }
}
__global__ void __launch_bounds__(256) match_count_kernel(const uint32_t* __restrict__ gid, uint32_t np, const uint32_t* __restrict__ counts, uint32_t* __restrict__ cnt) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= np; i += gridDim.x * blockDim.x)
        cnt[i] = (i < np && gid[i] != NONE) ? counts[gid[i]] : 0;
}
// 64-bit total of the per-probe-row match counts (their 32-bit exclusive scan wraps beyond 2^32 matches: 70,000 x 70,000 equal keys)
__global__ void __launch_bounds__(256) match_total_kernel(const uint32_t* __restrict__ cnt, uint32_t np, unsigned long long* __restrict__ total) {
    unsigned long long s = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) s += cnt[i];
    s = wave_reduce(s, OpAdd{});
    if (lane_id() == 0 && s) atomicAdd(total, s);
}
__global__ void __launch_bounds__(256) expand_kernel(const uint32_t* __restrict__ gid, uint32_t np, const uint32_t* __restrict__ out_off,
                                                     const uint32_t* __restrict__ grp_off, const uint32_t* __restrict__ rows_desc,
                                                     uint32_t* __restrict__ probe_rows, uint32_t* __restrict__ build_rows) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) {
        uint32_t g = gid[i];
        if (g == NONE) continue;
        uint32_t b = grp_off[g], e = grp_off[g + 1], o = out_off[i];
        for (uint32_t t = 0; t < e - b; ++t) { probe_rows[o + t] = i; build_rows[o + t] = rows_desc[e - 1 - t]; }   // ascending build rows
    }
}

uint32_t pow2_at_least(uint64_t v) { uint64_t p = 16; while (p < v) p <<= 1; return (uint32_t)p; }
bool key_dtype_ok(int t) {
    switch (t) { case AQG_INT8: case AQG_INT16: case AQG_INT32: case AQG_INT64: case AQG_UINT8: case AQG_UINT16: case AQG_UINT32: case AQG_UINT64: case AQG_BOOL: return true; }
    return false;
}

// table over (col, n) in the workspace: keys -> lowest row
int make_table(aqg_ctx* ctx, int t, const void* col, uint32_t n, JTable* jt) {
    jt->cap = pow2_at_least((uint64_t)n * 2);
    AQG_TRY(aqg_ws_get(ctx, (size_t)jt->cap, &jt->keys));
    AQG_TRY(aqg_ws_get(ctx, (size_t)jt->cap + 1, &jt->val));
    jt->sentinel_val = jt->val + jt->cap;
    AQG_HIP(ctx, hipMemsetAsync(jt->keys, 0xFF, (size_t)jt->cap * 8, ctx->stream));
    AQG_HIP(ctx, hipMemsetAsync(jt->val, 0xFF, ((size_t)jt->cap + 1) * 4, ctx->stream));
    if (n) hipLaunchKernelGGL(jt_build_kernel, dim3(aqg_grid(ctx, n, 256, 4, 8)), dim3(256), 0, ctx->stream, t, col, n, *jt);
    return aqg_check_launch(ctx, "jt_build_kernel");
}

void launch_probe(aqg_ctx* ctx, int t, const void* pk, uint32_t np, const JTable& jt, uint32_t* out) {
    const size_t lds = (size_t)jt.cap * 12;
    if (lds <= 48 * 1024 && np >= (1u << 16)) {
        hipLaunchKernelGGL((jt_probe_kernel<true>), dim3(aqg_grid(ctx, np / 4 + 1, 256, 2, lds <= 20 * 1024 ? 8 : 3)), dim3(256), lds, ctx->stream, t, pk, np, jt, out);
    } else {
        hipLaunchKernelGGL((jt_probe_kernel<false>), dim3(aqg_grid(ctx, np / 4 + 1, 256, 2, 8)), dim3(256), 0, ctx->stream, t, pk, np, jt, out);
    }
}

int join_core(aqg_ctx* ctx, int t, const void* bk, uint32_t nb, const void* pk, uint32_t np, uint32_t* probe_rows, uint32_t* build_rows,
              uint64_t capacity, uint64_t* m_host) {
    *m_host = 0;
    if (!key_dtype_ok(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "join: integer key columns only");
    AQG_CHECK_ROWS(ctx, nb, "join");
    AQG_CHECK_ROWS(ctx, np, "join");
    if (nb == 0 || np == 0) return AQG_OK;
    // 1. group the build side (dense ids, counts, descending row lists)
    aqg_groupby* gb = nullptr;
    const void* kcols[1] = {bk};
    AQG_TRY(aqg_groupby_build(ctx, 1, &t, kcols, nb, 0, &gb));
    const uint32_t G = aqg_groupby_ngroups(gb);
    uint32_t *grp_off = nullptr, *rows_desc = nullptr;
    void* dkeys = nullptr;
    int rc = aqg_malloc(ctx, ((size_t)G + 1) * 4, (void**)&grp_off);
    if (rc == AQG_OK) rc = aqg_malloc(ctx, (size_t)nb * 4, (void**)&rows_desc);
    if (rc == AQG_OK) rc = aqg_malloc(ctx, (size_t)G * 8, &dkeys);
    if (rc == AQG_OK) rc = aqg_groupby_postproc(gb, grp_off, rows_desc);
    if (rc == AQG_OK) rc = aqg_groupby_keys(gb, 0, dkeys);
    auto cleanup = [&]() { aqg_free(ctx, grp_off); aqg_free(ctx, rows_desc); aqg_free(ctx, dkeys); aqg_groupby_destroy(gb); };
    if (rc != AQG_OK) { cleanup(); return rc; }
    // 2. distinct build key -> group id, probe
    rc = aqg_ws_reset(ctx);
    size_t need = (size_t)pow2_at_least((uint64_t)G * 2) * 12 + ((size_t)np + 1) * 8 + (((size_t)np + 1) / 2048 + 2) * 4 + 16384 + 256;
    if (rc == AQG_OK) rc = aqg_ws_ensure(ctx, need);
    JTable jt;
    uint32_t *gid = nullptr, *cnt = nullptr, *bsum = nullptr;
    unsigned long long* total = nullptr;
    if (rc == AQG_OK) rc = make_table(ctx, t, dkeys, G, &jt);
    if (rc == AQG_OK) rc = aqg_ws_get(ctx, 1, &total);
    if (rc == AQG_OK) rc = aqg_ws_get(ctx, (size_t)np + 1, &gid);
    if (rc == AQG_OK) rc = aqg_ws_get(ctx, (size_t)np + 1, &cnt);
    if (rc == AQG_OK) rc = aqg_ws_get(ctx, ((size_t)np + 1) / 2048 + 2, &bsum);
    if (rc != AQG_OK) { cleanup(); return rc; }
    unsigned pg = aqg_grid(ctx, np, 256, 4, 8);
    launch_probe(ctx, t, pk, np, jt, gid);
    hipLaunchKernelGGL(match_count_kernel, dim3(pg), dim3(256), 0, ctx->stream, gid, np, aqg_groupby_counts(gb), cnt);
    // the number of matches in 64 bits, BEFORE the 32-bit offsets are trusted: with duplicate keys it passes 2^32 at small inputs
    rc = hipMemsetAsync(total, 0, 8, ctx->stream) == hipSuccess ? AQG_OK : AQG_ERR_HIP;
    if (rc == AQG_OK) hipLaunchKernelGGL(match_total_kernel, dim3(pg), dim3(256), 0, ctx->stream, (const uint32_t*)cnt, np, total);
    unsigned long long m64 = 0;
    if (rc == AQG_OK) rc = aqg_d2h(ctx, &m64, total, 8);
    if (rc != AQG_OK) { cleanup(); return rc; }
    *m_host = m64;
    if (probe_rows && build_rows && m64) {
        // pairs are addressed by uint32 offsets like every row index of this library
        if (m64 > (unsigned long long)AQG_MAX_ROWS) { cleanup(); return aqg_fail(ctx, AQG_ERR_OVERFLOW, "aqg_join_pairs: more than AQG_MAX_ROWS matching pairs (*m_host holds the count)"); }
        if (capacity < m64) { cleanup(); return aqg_fail(ctx, AQG_ERR_OVERFLOW, "aqg_join_pairs: output capacity too small"); }
        rc = aqg_exclusive_scan_u32(ctx, cnt, (uint64_t)np + 1, bsum);
        if (rc != AQG_OK) { cleanup(); return rc; }
        hipLaunchKernelGGL(expand_kernel, dim3(pg), dim3(256), 0, ctx->stream, gid, np, cnt, grp_off, rows_desc, probe_rows, build_rows);
        rc = aqg_check_launch(ctx, "expand_kernel");
        if (rc == AQG_OK) rc = aqg_sync(ctx);
    }
    cleanup();
    return rc;
}

} // namespace

extern "C" {

int aqg_join_lookup(aqg_ctx* ctx, int t, const void* bk, uint32_t nb, const void* pk, uint32_t np, uint32_t* out) {
    if (!ctx || (!bk && nb) || (!pk && np) || (!out && np)) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_lookup: bad argument");
    if (!key_dtype_ok(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_join_lookup: integer key columns only");
    AQG_CHECK_ROWS(ctx, nb, "aqg_join_lookup");
    AQG_CHECK_ROWS(ctx, np, "aqg_join_lookup");
    if (np == 0) return AQG_OK;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)pow2_at_least((uint64_t)nb * 2) * 12 + 8192));
    JTable jt;
    AQG_TRY(make_table(ctx, t, bk, nb, &jt));
    aqg_kernel_timer_begin(ctx);
    launch_probe(ctx, t, pk, np, jt, out);
    aqg_kernel_timer_end(ctx);
    return aqg_check_launch(ctx, "jt_probe_kernel");
}

int aqg_join_count(aqg_ctx* ctx, int t, const void* bk, uint32_t nb, const void* pk, uint32_t np, uint64_t* m_host) {
    if (!ctx || !m_host || (!bk && nb) || (!pk && np)) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_count: bad argument");
    return join_core(ctx, t, bk, nb, pk, np, nullptr, nullptr, 0, m_host);
}

int aqg_join_pairs(aqg_ctx* ctx, int t, const void* bk, uint32_t nb, const void* pk, uint32_t np, uint32_t* probe_rows, uint32_t* build_rows,
                   uint64_t capacity, uint64_t* m_host) {
    if (!ctx || !m_host || (!bk && nb) || (!pk && np)) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_pairs: bad argument");
    return join_core(ctx, t, bk, nb, pk, np, probe_rows, build_rows, capacity, m_host);
}

} // extern "C"
