// join_tail.hpp -- what join.hip (one integer key) and join_keys.hip (tuples of typed keys) share: everything but the table and the
// probe.  Both group the build side with aqg_groupby_build, probe into gid[np] = {group id | NONE} and hand gid to aqg_join_tail.
#pragma once
#include "aqg_internal.hpp"

constexpr uint32_t NONE = 0xFFFFFFFFu;                 // a probe row without a partner
inline uint32_t pow2_at_least(uint64_t v) { uint64_t p = 16; while (p < v) p <<= 1; return (uint32_t)p; }

// The route of both probes: a table (with whatever the probe reads beside it) of `table_bytes` is copied into LDS when it fits 48 KB
// under at least 2^16 probe rows; otherwise it is read in place (HBM, L2-resident for small dimensions).
constexpr size_t JOIN_LDS_LIMIT = 48 * 1024;
constexpr uint32_t JOIN_LDS_MIN_ROWS = 1u << 16;
inline bool join_lds_route(size_t table_bytes, uint32_t np) { return table_bytes <= JOIN_LDS_LIMIT && np >= JOIN_LDS_MIN_ROWS; }
// The grid of a probe kernel of 256 threads with `rows_per_lane` consecutive probe rows per lane, two such chunks per thread: 8
// workgroups per CU reading in place or with up to 20 KB of LDS each, 3 with more (`lds`: the bytes the LDS route stages).
inline unsigned join_probe_grid(const aqg_ctx* ctx, uint32_t np, int rows_per_lane, bool use_lds, size_t lds) {
    return aqg_grid(ctx, np / rows_per_lane + 1, 256, 2, use_lds ? (lds <= 20 * 1024 ? 8 : 3) : 8);
}

// The grouped build side of one call: the handle and the device buffers a join holds until it returns, freed in the destructor.
struct JoinBuild {
    aqg_ctx* ctx;
    aqg_groupby* gb = nullptr;                         // stays null for an empty build side
    uint32_t G = 0;
    uint32_t *grp_off = nullptr, *rows_desc = nullptr; // [G + 1] offsets, [nb] descending row lists: only when build rows are emitted
    void* dkeys = nullptr;                             // keys0(): the distinct keys of key column 0, in group order
    explicit JoinBuild(aqg_ctx* c) : ctx(c) {}
    JoinBuild(const JoinBuild&) = delete;
    JoinBuild& operator=(const JoinBuild&) = delete;
    ~JoinBuild();
    // groups the nb > 0 build rows; the row lists (two buffers, aqg_groupby_postproc's three radix passes) only where `emit_build_rows`
    int setup(int nkeys, const int* dts, const void* const* cols, uint32_t nb, bool emit_build_rows);
    int keys0();
    const uint32_t* counts() const { return gb ? aqg_groupby_counts(gb) : nullptr; }
};

// The phase behind the probe, from the caller's workspace (reset, sized ONCE with its table + gid + aqg_join_tail_ws_bytes, table and
// gid carved first): output rows per probe row by `kind` -> 64-bit total -> *m_host -> refusals -> exclusive scan -> emit -> sync.
// probe_rows == nullptr: the count alone.  `who`: the public entry the refusal messages name.
size_t aqg_join_tail_ws_bytes(uint32_t np);
int aqg_join_tail(aqg_ctx* ctx, int kind, const uint32_t* gid, uint32_t np, const JoinBuild& build, uint32_t* probe_rows, uint32_t* build_rows,
                  uint64_t capacity, uint64_t* m_host, const char* who);

// join_keys.hip: the tuple probe for the joins that search behind it (asof.hip).  aqg_jk_check: the argument, dtype, tuple-width and
// row-count checks of aqg_join_keys_lookup.  aqg_jk_probe_gid: gid[i] = the group of `gb` (the grouped build side) whose tuple equals
// probe row i, else NONE; its table comes from the caller's workspace (reset, sized with aqg_jk_table_bytes beside the caller's own needs).
int aqg_jk_check(aqg_ctx* ctx, int nkeys, const int* dts, const void* const* bk, uint32_t nb, const void* const* pk, uint32_t np);
size_t aqg_jk_table_bytes(int nkeys, const int* dts, uint32_t G);
int aqg_jk_probe_gid(aqg_ctx* ctx, int nkeys, const int* dts, const void* const* bk, const void* const* pk, uint32_t np, aqg_groupby* gb, uint32_t* gid);

// join.hip: aqg_join_lookup, which also says what it ran (the slots of its table over the build ROWS, and the route of its probe)
int aqg_join_lookup_routed(aqg_ctx* ctx, int t, const void* bk, uint32_t nb, const void* pk, uint32_t np, uint32_t* out, uint32_t* table_slots, bool* lds);
