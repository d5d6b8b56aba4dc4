// groupby_plan.hpp -- host-side vocabulary of the group-by: what a call asks for (Plan), every decision of one attempt (AggPlan), its
// buffers (AggBufs), and the phases of an attempt that live in files of their own.  The planner and run_agg: groupby.hip.
#pragma once
#include "groupby_dev.hpp"
#include "groupby_fast.hpp"
#include "dense.hpp"
#include "partition1.hpp"

// the fused star join (groupby_starjoin.hip): the dimension side {key -> w} and the fact columns
struct StarJoin {
    const uint32_t* dim_keys; const uint32_t* dim_vals; uint32_t nb; uint32_t dcap;   // dcap: power of two >= 2 * nb
    const uint32_t* fk; const uint32_t* vals; int val_signed; int dim_signed;
};

// what each requested aggregate reads from the accumulators
struct AggOut { int op; int dt; int acc0; int acc1; int acc2; int acc3; void* out; };   // wide (8-byte integer) sums: acc0/acc2 = low, acc1/acc3 = high halves
struct EmitSpec { int nagg; AggOut agg[MAXAGG]; int nkeys; int key_dt[MAXKEYS]; int key_shift[MAXKEYS]; void* key_out[MAXKEYS]; int wide; const void* key_col[MAXKEYS];
                  uint32_t* first_out; uint32_t* count_out; };

struct Plan {
    AccSpec as;
    int need_count;
    int nagg;
    AggOut agg[MAXAGG];
    const StarJoin* sj;        // aqg_join_groupby_sum: the row pass is starjoin_kernel
};

struct DenseOut { bool used; DenseSpec spec; };      // tells aqg_groupby_build that the table is the direct-indexed one
constexpr int AQG_ERR_RANGE_MISS = -1001;            // internal: sampled key ranges missed a value; run_with_retry repeats the attempt

// the row pass of an attempt
enum class RowPass { STARJOIN, FAST_LDS, FEW_LDS, DENSE, PART_WIDE, PART_ONE, PART_TWO, PART_ROUND1, HASHED };

// every decision of one attempt (make_agg_plan)
struct AggPlan {
    uint32_t n, hint;                 // hint: a tiny dense domain replaces the caller's
    bool for_build, k32;              // k32: one 4-byte key column
    KeySpec ks;                       // packed keys of many expected groups are promoted to wide tuples
    Plan plan;                        // the partitioned build also counts the groups
    bool use_lds, big_lds, dense, build_part, use_part, lookup_build, use_wpart, rows_possible, sorted_tail, small_rank, sparse_rank, ordered_emit;
    bool fast, fast_k64, fast_key8, fast_v8, defer;      // defer: the flags are judged behind the queued tail (fast path and star join, small tables)
    uint32_t lcap, npass, lk_min, lk_D, pbits, part_lcap, p1_bins, p2_parts, gcap, nwords, ntiles;
    int part_layout;
    size_t lds_slot_bytes;
    uint64_t lds_group_cap;
    DenseSpec dspec;
    FastVals fv;
    RowPass pass;
};

// the attempt's buffers, carved from the workspace arena in a fixed order (timings depend on where they land)
struct AggBufs {
    GTable gt;
    size_t slots;
    uint32_t *occ, *gid_of_occ, *slot_gid, *bitmap, *word_prefix, *tile_total, *tile_mark, *pinned_flags;   // pinned_flags: defer's copy of the flag words
    PartRows prows;
};

static inline uint32_t next_pow2(uint64_t v) { uint64_t p = 1; while (p < v) p <<= 1; return (uint32_t)(p > 0x80000000ull ? 0x80000000ull : p); }

// The result handle of a call: the caller's (*out), or a new one -- which is destroyed again unless the call hands it over.
// A caller's own handle is never destroyed.
struct aqg_handle_guard {
    aqg_groupby** out;
    aqg_groupby* h;
    explicit aqg_handle_guard(aqg_groupby** o) : out(o), h(*o ? *o : new aqg_groupby()) {}
    ~aqg_handle_guard() { if (h != *out) aqg_groupby_destroy(h); }
    int hand_over() { *out = h; return AQG_OK; }
};

// groupby.hip
int aqg_make_keyspec(aqg_ctx* ctx, int nkeys, const int* dts, const void* const* keys, uint32_t n, KeySpec* ks);
int aqg_add_acc(Plan* p, int kind, int dt, const void* col, int square, int part = 0);
int aqg_make_plan(aqg_ctx* ctx, int naggs, const int* ops, const int* dts, const void* const* vals, uint32_t n, Plan* p);
int aqg_run_with_retry(aqg_ctx* ctx, const KeySpec& ks, const Plan& plan, uint32_t n, uint32_t hint, bool for_build, aqg_groupby* h,
                       GTable* gt_out, uint32_t** slot_gid_out, uint32_t** occ_out = nullptr, DenseOut* dense_out = nullptr);
// groupby_keys.hip: the integer columns (ndt / ncol, *nn of them) that stand for the caller's key columns; bookkeeping for aqg_groupby_keys in `h`
int aqg_normalize_keys(aqg_ctx* ctx, aqg_groupby* h, int nkeys, const int* dts, const void* const* keys, uint32_t n, int* nn, int* ndt, const void** ncol);
// groupby_estimate.hip: the number of groups of `n` rows, estimated from a spread sample; 0: no estimate
uint64_t aqg_estimate_groups(aqg_ctx* ctx, const KeySpec& ks, uint32_t n);
// the row passes with kernels of their own: groupby_starjoin.hip, groupby_hashed.hip
int aqg_pass_starjoin(aqg_ctx* ctx, const AggPlan& p, const GTable& gt);
int aqg_pass_hashed(aqg_ctx* ctx, const AggPlan& p, const GTable& gt);
// groupby_tail.hip: table initialisation and the ids of the occupied slots (`slots` = capacity + 1), then the tail's two phases
void aqg_gt_init(aqg_ctx* ctx, const GTable& gt, const AccSpec& as, size_t slots);
void aqg_collect(aqg_ctx* ctx, const GTable& gt, uint32_t* occ, size_t slots);
void aqg_occ_iota(aqg_ctx* ctx, uint32_t* occ, size_t slots);
int aqg_rank_groups(aqg_ctx* ctx, const AggPlan& p, const AggBufs& b, uint32_t G, bool row_emit, SortedParts* sparts);
int aqg_emit_outputs(aqg_ctx* ctx, const AggPlan& p, aqg_groupby* h, const AggBufs& b, uint32_t G, bool row_emit, const SortedParts& sparts);
// groupby_build.hip: the id of every row of a build that took a partition plan
int aqg_assign_build_ids(aqg_ctx* ctx, const AggPlan& p, aqg_groupby* h, const AggBufs& b, uint32_t G);
