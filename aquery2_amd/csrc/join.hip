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
//   aqg_join_count / aqg_join_pairs   general inner join: group the build side (JoinBuild: aqg_groupby_build, the row lists only
//                     when pairs are written), look each probe key up among the distinct build keys into gid[np];
//                     count, 64-bit total, scan and emit are aqg_join_tail's (join_tail.hip), shared with join_keys.hip.
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "join_tail.hpp"

namespace {

constexpr uint64_t JEMPTY = ~0ull;

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

// make_table's share of the workspace: keys, then payloads with the sentinel's behind them, each aligned to 256 bytes
size_t table_bytes(uint32_t n) { return (size_t)pow2_at_least((uint64_t)n * 2) * 12 + 4 + 2 * 256; }

// returns whether the LDS route ran
bool launch_probe(aqg_ctx* ctx, int t, const void* pk, uint32_t np, const JTable& jt, uint32_t* out) {
    const size_t lds = (size_t)jt.cap * 12;
    const bool use_lds = join_lds_route(lds, np);
    const unsigned grid = join_probe_grid(ctx, np, 4, use_lds, lds);
    if (use_lds) hipLaunchKernelGGL((jt_probe_kernel<true>), dim3(grid), dim3(256), lds, ctx->stream, t, pk, np, jt, out);
    else hipLaunchKernelGGL((jt_probe_kernel<false>), dim3(grid), dim3(256), 0, ctx->stream, t, pk, np, jt, out);
    return use_lds;
}

int join_core(aqg_ctx* ctx, int t, const void* bk, uint32_t nb, const void* pk, uint32_t np, uint32_t* probe_rows, uint32_t* build_rows,
              uint64_t capacity, uint64_t* m_host) {
    *m_host = 0;
    if (!key_dtype_ok(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "join: integer key columns only");
    AQG_CHECK_ROWS(ctx, nb, "join");
    AQG_CHECK_ROWS(ctx, np, "join");
    if (nb == 0 || np == 0) return AQG_OK;
    if (!build_rows) probe_rows = nullptr;             // pairs are written into both outputs or not at all
    // 1. group the build side (dense ids, counts, distinct keys; descending row lists for the pairs)
    JoinBuild build(ctx);
    AQG_TRY(build.setup(1, &t, &bk, nb, probe_rows != nullptr));
    AQG_TRY(build.keys0());
    // 2. distinct build key -> group id, probe
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, table_bytes(build.G) + (size_t)np * 4 + 256 + aqg_join_tail_ws_bytes(np)));
    JTable jt;
    uint32_t* gid = nullptr;
    AQG_TRY(make_table(ctx, t, build.dkeys, build.G, &jt));
    AQG_TRY(aqg_ws_get(ctx, (size_t)np, &gid));
    launch_probe(ctx, t, pk, np, jt, gid);
    AQG_TRY(aqg_check_launch(ctx, "jt_probe_kernel"));
    // 3. count, total, scan, emit
    return aqg_join_tail(ctx, AQG_JOIN_INNER, gid, np, build, probe_rows, build_rows, capacity, m_host, "aqg_join_pairs");
}

} // namespace

int aqg_join_lookup_routed(aqg_ctx* ctx, int t, const void* bk, uint32_t nb, const void* pk, uint32_t np, uint32_t* out, uint32_t* table_slots, bool* lds) {
    if (!ctx || (!bk && nb) || (!pk && np) || (!out && np)) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_lookup: bad argument");
    if (!key_dtype_ok(t)) return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_join_lookup: integer key columns only");
    AQG_CHECK_ROWS(ctx, nb, "aqg_join_lookup");
    AQG_CHECK_ROWS(ctx, np, "aqg_join_lookup");
    if (np == 0) return AQG_OK;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, table_bytes(nb)));
    JTable jt;
    AQG_TRY(make_table(ctx, t, bk, nb, &jt));
    aqg_kernel_timer_begin(ctx);
    *lds = launch_probe(ctx, t, pk, np, jt, out);
    aqg_kernel_timer_end(ctx);
    *table_slots = jt.cap;
    return aqg_check_launch(ctx, "jt_probe_kernel");
}

extern "C" {

int aqg_join_lookup(aqg_ctx* ctx, int t, const void* bk, uint32_t nb, const void* pk, uint32_t np, uint32_t* out) {
    uint32_t slots = 0;
    bool lds = false;
    return aqg_join_lookup_routed(ctx, t, bk, nb, pk, np, out, &slots, &lds);
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
