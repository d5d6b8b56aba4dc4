// aqg_internal.hpp -- host-side internals of libaqg (context, workspace, dtype dispatch).
// gfx950 only: no portability layer, no CPU fallback (the product fails loudly without a GPU).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/aqg.h"
#include "ws_guard.hpp"

// device mirror of a borrowed host column: `regs` = the host ranges page-locked for its upload (released at unpin), `ev` = upload done
struct aqg_pin { void* dptr; size_t bytes; std::vector<std::pair<void*, size_t>> regs; hipEvent_t ev; };

struct aqg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cu = 256;
    std::string err;
    // workspace arena: one allocation, bump-allocated per API call
    char* ws = nullptr;
    size_t ws_cap = 0, ws_off = 0;
    ws_guard_book guard;                         // AQG_WS_GUARD (test aid): ws_off is then the LOGICAL bump offset, ws_cap the physical size (ws_guard.hpp)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t evk0 = nullptr, evk1 = nullptr;   // bracket the dominant kernel of the last call
    hipEvent_t ev_flags = nullptr;               // recorded behind the copy of a group table's flag words (run_agg)
    hipStream_t copy_stream = nullptr;           // uploads of borrowed host columns (aqg_col_pin), created on first use
    void* up_buf[2] = {nullptr, nullptr};        // pinned staging of the fallback upload path (ranges the runtime refuses to copy directly)
    // device buffers of destroyed / outgrown result handles, kept for the next handle (a fresh handle per query -- what the header
    // layer does -- paid five hipMalloc + five hipFree, the latter each a device-wide synchronisation: ~0.1 ms of a 1.5 ms Q1 call)
    std::vector<std::pair<void*, size_t>> pool;
    size_t pool_bytes = 0;
    void* pool_big = nullptr; size_t pool_big_cap = 0;      // ONE large buffer (a row-to-group map of a build: 4 bytes per row) kept for the next handle
    uint32_t* rank_bm = nullptr;                 // a bitmap over row ids that is ALL ZERO between calls (group ranking of mid-size tables sets and clears only its own bits)
    size_t rank_bm_words = 0;
    hipEvent_t up_ev[2] = {nullptr, nullptr};
    bool tail_in_flight = false;                 // the last group-by returned with its tail kernels still queued (stream-ordered)
    bool evk_valid = false;
    bool evk_frozen = false;                     // the exchange's re-aggregation must not replace the row pass as "the dominant kernel"
    std::unordered_map<const void*, aqg_pin> pins;
    std::vector<std::pair<void*, size_t>> fetch_regs;   // host ranges page-locked for egress in flight (aqg_col_fetch), released by aqg_col_fetch_wait
    bool fetch_pending = false;
    hipEvent_t ev_fetch = nullptr;
    uint32_t pin_chunks[3] = {0, 0, 0};          // chunks of the last aqg_col_pin upload: page-locked + DMA / staged through pinned buffers / plain pageable copy
    std::unordered_map<const void*, int> max_lds;   // largest dynamic LDS size already granted per kernel (aqg_allow_lds)
    // aqg_sort_rows: digit passes of the last call (host), or in sort_passes_dev when the one-workgroup sort ran
    uint32_t sort_passes = 0;
    bool sort_passes_on_dev = false;
    uint32_t* sort_passes_dev = nullptr;
    uint32_t* select_ctl = nullptr;              // aqg_median / aqg_grouped_median: control words of the last call (routes, passes, the flat call's result)
    // aqg_count_distinct / aqg_grouped_count_distinct: control words of the last call (pairs, crossing groups, the flat call's offsets and
    // result), the pair list (grow-only) and the flat call's handle for the group-by over it
    uint32_t* distinct_ctl = nullptr;
    void* distinct_pairs = nullptr;
    size_t distinct_pairs_cap = 0;
    struct aqg_groupby* distinct_scratch = nullptr;
    uint32_t join_routes = 0, join_groups = 0, join_slots = 0;   // aqg_join_keys_*: form and route, distinct build tuples and table slots of the last call (aqg_join_last)
    uint32_t asof_routes = 0, asof_groups = 0, asof_passes = 0;   // aqg_join_asof: routes, distinct build tuples and the ordering step's digit passes of the last call (aqg_join_asof_last)
    uint32_t wj_routes = 0, wj_groups = 0, wj_passes = 0;         // aqg_join_window* / aqg_interval_fold: the same of the last call, plus the fold's route (aqg_join_window_last)
    uint32_t rank_routes = 0, rank_tile = 0;    // aqg_rank*: routes of the last call and the sorted entries one workgroup of its emit kernel owns (aqg_rank_last)
    uint32_t scan2_route = 0, scan2_tile = 0;   // aqg_scan2*: the route of the last call and the rows one workgroup of it owns (aqg_scan2_last)
    uint32_t winq_tile = 0, winq_halo = 0;      // aqg_window_quantiles*: rows per workgroup and halo rows of the last call (aqg_window_quantiles_last)
    // aqg_rangew*: the packed step counters of the last bounds call (rising steps in the low word, falling in the high one) and the
    // row count of the last fold, from which aqg_rangew_last derives the block tree's geometry
    unsigned long long* rangew_steps = nullptr;
    uint32_t rangew_fold_n = 0;
    uint32_t str_route = 0, str_mismatch = 0;   // aqg_str_encode: the route of the last call and whether its verify kernel saw a mismatch (aqg_str_encode_last)
    // pinned host staging for small results
    void* host_stage = nullptr;
    size_t host_stage_cap = 0;
};

#define AQG_HIP(ctx, call)                                                                     \
    do {                                                                                       \
        hipError_t _e = (call);                                                                \
        if (_e != hipSuccess) {                                                                \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(_e);                    \
            (void)hipGetLastError(); /* do not leave a sticky error for the next launch check */ \
            return AQG_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

#define AQG_TRY(expr)                          \
    do {                                       \
        int _rc = (expr);                      \
        if (_rc != AQG_OK) return _rc;         \
    } while (0)

static inline int aqg_fail(aqg_ctx* ctx, int code, const char* msg) {
    if (ctx) ctx->err = msg;
    return code;
}
#define AQG_CHECK_ROWS(ctx, n, what) do { if ((uint64_t)(n) > (uint64_t)AQG_MAX_ROWS) return aqg_fail(ctx, AQG_ERR_ARG, what ": more than AQG_MAX_ROWS rows"); } while (0)
static inline uint32_t aqg_ceil_div(uint32_t n, uint32_t d) { return (uint32_t)(((uint64_t)n + d - 1) / d); }
// do the byte ranges [a, a + abytes) and [b, b + bbytes) share a byte?  (a null or empty range shares none)
inline bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes) {
    if (!a || !b || !abytes || !bbytes) return false;
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}

// the environment switches of the README (measurement and test aids), read once per process: the tests start a fresh process to force a plan
struct aqg_switch_set {
    uint32_t p1_max, sorted_tail_min;   // AQG_P1_MAX (1024), AQG_SORTED_TAIL_MIN (2^24)
    int p1_bins;                        // AQG_P1_BINS (0: planned)
    uint32_t select_small_max, select_split_min;   // AQG_SELECT_SMALL_MAX (256), AQG_SELECT_SPLIT_MIN (2^20): the route thresholds of select.hip
    double pw_sigma;                    // AQG_PW_SIGMA (6)
    bool disable_p1, disable_p1_cursors, disable_ranged, disable_pw_defer, disable_build_partition, debug_flags, str_host;
    int ws_guard;                       // AQG_WS_GUARD=<byte>: poison, red zones and exact sizing of the scratch memory (-1: unset)
};
const aqg_switch_set& aqg_switches();
// AQG_WS_GUARD: fill fresh or recycled device scratch of the library with the poison byte (nothing when the switch is unset)
static inline void aqg_guard_fill(aqg_ctx* ctx, void* p, size_t bytes) {
    if (ctx->guard.on && p && bytes) (void)hipMemsetAsync(p, ctx->guard.pattern, bytes, ctx->stream);
}
// hipMalloc of device scratch the library keeps for itself (control words, grow-only lists): poisoned under AQG_WS_GUARD
static inline hipError_t aqg_scratch_malloc(aqg_ctx* ctx, void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) aqg_guard_fill(ctx, *p, bytes);
    return e;
}
template <class T> static inline hipError_t aqg_scratch_malloc(aqg_ctx* ctx, T** p, size_t bytes) { return aqg_scratch_malloc(ctx, reinterpret_cast<void**>(p), bytes); }

// workspace: reset at the start of an API call, then bump.  Growing synchronises the
// stream (earlier kernels may still read the old arena) -- call aqg_reserve_workspace
// ahead of timed regions.
int aqg_ws_reset(aqg_ctx* ctx);
// small-buffer pool of a context (stream-ordered reuse: every user of these buffers runs on ctx->stream)
static inline void* aqg_pool_take(aqg_ctx* ctx, size_t need, size_t* cap) {
    if (ctx->pool_big && ctx->pool_big_cap >= need && ctx->pool_big_cap <= 2 * need) { void* p = ctx->pool_big; *cap = ctx->pool_big_cap; ctx->pool_big = nullptr; ctx->pool_big_cap = 0; return p; }
    int best = -1;
    const size_t slack = need * 4 > ((size_t)64 << 10) ? need * 4 : ((size_t)64 << 10);
    for (int i = 0; i < (int)ctx->pool.size(); ++i)
        if (ctx->pool[i].second >= need && ctx->pool[i].second <= slack && (best < 0 || ctx->pool[i].second < ctx->pool[best].second)) best = i;
    if (best < 0) return nullptr;
    void* p = ctx->pool[best].first;
    *cap = ctx->pool[best].second;
    ctx->pool_bytes -= *cap;
    ctx->pool[best] = ctx->pool.back();
    ctx->pool.pop_back();
    return p;
}
static inline void aqg_pool_give(aqg_ctx* ctx, void* p, size_t cap) {
    if (!p) return;
    if (ctx && cap && cap <= ((size_t)64 << 20) && ctx->pool.size() < 64 && ctx->pool_bytes + cap <= ((size_t)512 << 20)) { ctx->pool.emplace_back(p, cap); ctx->pool_bytes += cap; return; }
    if (ctx && cap > ((size_t)64 << 20) && cap <= ((size_t)8 << 30) && cap > ctx->pool_big_cap) {        // the larger one stays
        if (ctx->pool_big) (void)hipFree(ctx->pool_big);
        ctx->pool_big = p; ctx->pool_big_cap = cap;
        return;
    }
    (void)hipFree(p);
}
// `need` bytes from the pool, else from hipMalloc (*err: its status); nullptr, and no error left behind for the next launch check, when there is no memory
static inline void* aqg_pool_alloc(aqg_ctx* ctx, size_t need, size_t* cap, hipError_t* err = nullptr) {
    if (void* q = aqg_pool_take(ctx, need, cap)) { aqg_guard_fill(ctx, q, *cap); return q; }
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, need);
    if (err) *err = e;
    if (e != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    *cap = need;
    aqg_guard_fill(ctx, q, need);
    return q;
}
// a device buffer from the context's pool, given back when the call ends (for what must outlive a workspace reset between the steps of a call)
struct PoolBuf {
    aqg_ctx* ctx;
    void* p = nullptr;
    size_t cap = 0;
    explicit PoolBuf(aqg_ctx* c) : ctx(c) {}
    PoolBuf(const PoolBuf&) = delete;
    PoolBuf& operator=(const PoolBuf&) = delete;
    ~PoolBuf() { aqg_pool_give(ctx, p, cap); }
    int get(size_t bytes) {
        hipError_t e = hipSuccess;
        p = aqg_pool_alloc(ctx, bytes < 256 ? 256 : bytes, &cap, &e);
        if (!p) { ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e); return AQG_ERR_NOMEM; }
        return AQG_OK;
    }
};
// grow-only device buffer of a handle: *p holds at least `need` bytes afterwards (its contents are not kept)
template <class T> static inline int aqg_dev_realloc(aqg_ctx* ctx, T** p, size_t* cap, size_t need) {
    if (need <= *cap && *p) return AQG_OK;
    if (*p) { aqg_pool_give(ctx, *p, *cap); *p = nullptr; *cap = 0; }        // (stream-ordered reuse; a buffer too large for the pool is freed, which synchronises)
    hipError_t e = hipSuccess;
    void* q = aqg_pool_alloc(ctx, need < 256 ? 256 : need, cap, &e);
    if (!q) { ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e); return AQG_ERR_NOMEM; }
    *p = static_cast<T*>(q);
    return AQG_OK;
}
int aqg_ws_alloc(aqg_ctx* ctx, size_t bytes, void** out);
int aqg_ws_ensure(aqg_ctx* ctx, size_t bytes);
template <class T> static inline int aqg_ws_get(aqg_ctx* ctx, size_t count, T** out) {
    void* p = nullptr;
    int rc = aqg_ws_alloc(ctx, count * sizeof(T), &p);
    *out = static_cast<T*>(p);
    return rc;
}
int aqg_host_stage(aqg_ctx* ctx, size_t bytes, void** out);
// in-place exclusive scan of `count` uint32 words; bsum: scratch of ceil(count/2048) words (postproc.hip)
int aqg_exclusive_scan_u32(aqg_ctx* ctx, uint32_t* d, uint64_t count, uint32_t* bsum);

// postproc.hip: the stable radix passes over a build's group-id column.  x == nullptr: descending row ids per group -> row_ids_dev; else the
// `esz`-byte elements of column x in the flat row-list layout -> xout.  ws_managed: the caller reset the workspace and sized it with
// aqg_postproc_ws_bytes (so that its own sub-allocations survive)
struct aqg_groupby;
size_t aqg_postproc_ws_bytes(uint32_t n, uint32_t G, int esz);
int aqg_radix_by_group(aqg_ctx* ctx, aqg_groupby* g, uint32_t* row_ids_dev, const void* x, int esz, void* xout, bool ws_managed);
int aqg_group_offsets(aqg_ctx* ctx, const aqg_groupby* g, uint32_t* offsets_dev, uint32_t* bsum);
// segscan.hip: *gid = the group index of every position of the flat layout (n elements, owned and cached by the handle)
int aqg_flat_gid(aqg_ctx* ctx, aqg_groupby* g, const uint32_t** gid);
// grouped_reduce.hip: out[g] = op(x[rows whose id in gid_col is g]) through the group-by plans (gid_col: n dense ids in first-occurrence order)
extern "C" int aqg_grouped_reduce_keyed(aqg_ctx* ctx, aqg_groupby* g, const uint32_t* gid_col, int op, int t, const void* x, void* out_dev);

// exchange.hip: the all-gather of a communicator (`bytes` bytes of every rank, rank order, on / ordered behind the context's stream)
struct aqg_comm;
int aqg_comm_allgather_internal(aqg_comm* c, const void* send_dev, void* recv_dev, size_t bytes);
aqg_ctx* aqg_comm_ctx(aqg_comm* c);
// scan.hip: running min / max of one row-range shard, seeded with the fold of the earlier shards
extern "C" int aqg_scan_minmax_seeded(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, const void* seed_host, void* out);

// reduce.hip: raw moments of a column / of a pair of columns left in device memory (the sharded reductions ship them)
extern "C" int aqg_stats_dev(aqg_ctx* ctx, int t, const void* x, uint32_t n, int flags, void* out_dev48);
extern "C" int aqg_corr_sums_dev(aqg_ctx* ctx, int tx, const void* x, int ty, const void* y, uint32_t n, void* out_dev80);
// exchange.hip: grow-only device scratch of a communicator (send / receive sides of its small exchanges)
int aqg_comm_scratch(aqg_comm* c, size_t send_bytes, size_t recv_bytes, void** send, void** recv);

// internal aggregate of aqg_groupby_agg (not in aqg.h): the sum of squares, typed like SUM -- the second moment the sharded call ships for VAR / STDDEV
constexpr int AQG_RED_SUMSQ = 64;

// HIP events around the dominant kernel of a call (read back by aqg_last_kernel_ms)
static inline void aqg_kernel_timer_begin(aqg_ctx* ctx) { if (!ctx->evk_frozen) (void)hipEventRecord(ctx->evk0, ctx->stream); }
static inline void aqg_kernel_timer_end(aqg_ctx* ctx) { if (!ctx->evk_frozen) { (void)hipEventRecord(ctx->evk1, ctx->stream); ctx->evk_valid = true; } }

// launch check
static inline int aqg_check_launch(aqg_ctx* ctx, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ctx->err = std::string(what) + ": " + hipGetErrorString(e);
        return AQG_ERR_HIP;
    }
    return AQG_OK;
}

// grid sizing for memory-bound grid-stride kernels: enough blocks to fill 256 CUs,
// capped (guide: Guideline 11)
// hipFuncAttributeMaxDynamicSharedMemorySize once per kernel and size, not on every launch (a few microseconds of host time each)
static inline int aqg_allow_lds(aqg_ctx* ctx, const void* kernel, size_t lds) {
    auto it = ctx->max_lds.find(kernel);
    if (it != ctx->max_lds.end() && (size_t)it->second >= lds) return AQG_OK;
    AQG_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ctx->max_lds[kernel] = (int)lds;
    return AQG_OK;
}

static inline unsigned aqg_grid(const aqg_ctx* ctx, uint64_t work_items, unsigned block, unsigned items_per_thread,
                                unsigned blocks_per_cu = 8) {
    uint64_t per_block = (uint64_t)block * items_per_thread;
    uint64_t need = (work_items + per_block - 1) / per_block;
    uint64_t cap = (uint64_t)ctx->num_cu * blocks_per_cu;
    if (need < 1) need = 1;
    return (unsigned)(need < cap ? need : cap);
}

// ---- dtype helpers (host) ----------------------------------------------------------------
static inline size_t dt_size(int dt) { return aqg_dtype_size(dt); }
static inline bool dt_is_fp(int dt) { return dt == AQG_FLOAT || dt == AQG_DOUBLE; }
static inline bool dt_is_unsigned(int dt) {
    return dt == AQG_UINT8 || dt == AQG_UINT16 || dt == AQG_UINT32 || dt == AQG_UINT64 || dt == AQG_UINT128 || dt == AQG_BOOL;
}
static inline bool dt_is_num(int dt) {
    switch (dt) {
    case AQG_INT8: case AQG_INT16: case AQG_INT32: case AQG_INT64: case AQG_UINT8: case AQG_UINT16:
    case AQG_UINT32: case AQG_UINT64: case AQG_FLOAT: case AQG_DOUBLE: return true;
    }
    return false;
}

// Dispatch a generic lambda on the C type of a numeric dtype tag.
template <class T> struct aqg_tag { using type = T; };
template <class F> static inline int aqg_dispatch_num(int dt, F&& f) {
    switch (dt) {
    case AQG_INT8: return f(aqg_tag<int8_t>{});
    case AQG_INT16: return f(aqg_tag<int16_t>{});
    case AQG_INT32: return f(aqg_tag<int32_t>{});
    case AQG_INT64: return f(aqg_tag<int64_t>{});
    case AQG_UINT8: return f(aqg_tag<uint8_t>{});
    case AQG_UINT16: return f(aqg_tag<uint16_t>{});
    case AQG_UINT32: return f(aqg_tag<uint32_t>{});
    case AQG_UINT64: return f(aqg_tag<uint64_t>{});
    case AQG_FLOAT: return f(aqg_tag<float>{});
    case AQG_DOUBLE: return f(aqg_tag<double>{});
    }
    return AQG_ERR_DTYPE;
}
