// groupby.hip -- hash group-by and grouped aggregation: the planner, the phases of an attempt, aqg_groupby_agg and aqg_join_groupby_sum.
//
// Replaces AQHashTable (reference server/hasher.h:146-199), set::hashtable_push
// (server/unordered_dense.h:1117-1147), ht_postproc (:181-198) and the generated per-group loop
// `out[g] = op(col[vecs[g]])` (engine/ast.py:722-789).
//
// Contract kept from the only executable path of the reference: group ids are dense and numbered by
// FIRST OCCURRENCE of the key tuple; row-id lists are DESCENDING inside a group.  The hash function
// is not observable in results (only dense ids are), so the device uses its own.
//
// Plans (make_agg_plan picks by the group-count hint, key shape and row count)
//   agg32_kernel       (groupby_fast.hip) one or two 4-byte keys or one 8-byte key, up to four accumulators over 1- to 8-byte values,
//                      <= 3072 groups: LDS table, 8 probes in flight (h2o Q4)
//   few32_kernel       (groupby_few.hip) one 4-byte key, 4-byte values, the plain call: the rows stream into LDS by DMA (h2o Q1)
//   agg_kernel<LDS>    (groupby_hashed.hip) any dtypes / MIN / MAX / VAR, packed tuples: {key, first_row, accumulators} open-addressing
//                      table in LDS (64 KB tables, several workgroups per CU; or one 150 KB table per CU and up to 4 passes over
//                      the rows), merged into the global table with device-scope atomics
//   dense.hip          small key DOMAIN (product of the column ranges): direct-indexed LDS tables (h2o Q2)
//   partition1.hip     more groups than LDS holds: the rows partitioned in one or two levels of the tile scatter, every partition
//                      aggregated in LDS (h2o Q3/Q5/Q7); beyond 4096 partitions the round-1 pipeline of partition.hip
//   partition_wide.hip tuples wider than 8 bytes with many groups: hash-partitioned rows, grouped inside LDS (h2o Q10)
//   agg_kernel<HBM>    (groupby_hashed.hip) rows straight to the global table (wide sparse tuples, the build path at high cardinality)
//   starjoin_kernel    (groupby_starjoin.hip) aqg_join_groupby_sum: the join's dimension side and the group table both in LDS
// Behind the row pass (run_agg):
//   groupby_tail.hip   collect / rank / emit: occupied slots -> dense ids ordered by first row -> output columns
//   groupby_build.hip  aqg_groupby_build's second pass: reversemap[i] = dense id, counts
// Around it: groupby_keys.hip (key columns that are not plain integers), groupby_estimate.hip (calls without a hint),
// groupby_merge.hip (row-sharded group-bys), grouped_reduce.hip (accumulators indexed by a build's dense ids), postproc.hip
// (aqg_groupby_postproc: stable partition of row ids by group id).
// HBM roofline: agg = sum of key and value bytes per row (h2o Q1: 8 B/row); build = 12 B/row.
#include "groupby_plan.hpp"

// partition.hip
size_t aqg_partition_ws_bytes(uint32_t n, int ksz, const AccSpec& as, uint32_t pbits);
int aqg_partition_aggregate(aqg_ctx* ctx, const KeySpec& ks, const AccSpec& as, uint32_t n, uint32_t pbits, uint32_t lcap, int need_count, GTable out, uint32_t out_cap);

int aqg_make_keyspec(aqg_ctx* ctx, int nkeys, const int* dts, const void* const* keys, uint32_t n, KeySpec* ks) {
    if (nkeys < 1 || nkeys > MAXKEYS) return aqg_fail(ctx, AQG_ERR_ARG, "group-by: 1..8 key columns");
    int bits = 0;
    ks->nkeys = nkeys;
    ks->range_known = 0; ks->range_lo = ks->range_hi = 0;
    for (int j = 0; j < nkeys; ++j) {
        if (!(dt_is_num(dts[j]) || dts[j] == AQG_BOOL)) return aqg_fail(ctx, AQG_ERR_DTYPE, "group-by: key dtype");
        if (dt_is_fp(dts[j])) return aqg_fail(ctx, AQG_ERR_DTYPE, "group-by: internal: floating key column reached the packed-key layer");
        if (!keys[j] && n) return aqg_fail(ctx, AQG_ERR_ARG, "group-by: null key column");
        ks->dt[j] = dts[j]; ks->col[j] = keys[j]; ks->shift[j] = bits;
        bits += 8 * (int)aqg_dtype_size(dts[j]);
    }
    ks->wide = bits > 64;
    if (ks->wide) for (int j = 0; j < nkeys; ++j) ks->shift[j] = 0;
    ks->total_bytes = bits / 8;
    return AQG_OK;
}

int aqg_add_acc(Plan* p, int kind, int dt, const void* col, int square, int part) {
    for (int a = 0; a < p->as.nacc; ++a)
        if (p->as.kind[a] == kind && p->as.dt[a] == dt && p->as.col[a] == col && p->as.square[a] == square && p->as.part[a] == part) return a;
    if (p->as.nacc >= MAXACC) return -1;
    int a = p->as.nacc++;
    p->as.kind[a] = kind; p->as.dt[a] = dt; p->as.col[a] = col; p->as.square[a] = square; p->as.part[a] = part;
    return a;
}

int aqg_make_plan(aqg_ctx* ctx, int naggs, const int* ops, const int* dts, const void* const* vals, uint32_t n, Plan* p) {
    memset(p, 0, sizeof *p);
    if (naggs < 0 || naggs > MAXAGG) return aqg_fail(ctx, AQG_ERR_ARG, "group-by: 0..8 aggregates");
    p->nagg = naggs;
    for (int j = 0; j < naggs; ++j) {
        int op = ops[j], dt = dts[j];
        if (!dt_is_num(dt)) return aqg_fail(ctx, AQG_ERR_DTYPE, "group-by: value dtype");
        if (!vals[j] && n && op != AQG_RED_COUNT) return aqg_fail(ctx, AQG_ERR_ARG, "group-by: null value column");
        bool fp = dt_is_fp(dt);
        AggOut& a = p->agg[j];
        a.op = op; a.dt = dt; a.acc0 = a.acc1 = a.acc2 = a.acc3 = -1; a.out = nullptr;
        const bool wide = dt == AQG_INT64 || dt == AQG_UINT64;
        const int addk = fp ? ACC_ADD_F : ACC_ADD_I;
        bool ok = true;
        switch (op) {
        case AQG_RED_SUM: case AQG_RED_AVG: case AQG_RED_VAR: case AQG_RED_STDDEV:
            if (wide) { a.acc0 = aqg_add_acc(p, addk, dt, vals[j], 0, 1); a.acc1 = aqg_add_acc(p, addk, dt, vals[j], 0, 2); ok = a.acc0 >= 0 && a.acc1 >= 0; }
            else { a.acc0 = aqg_add_acc(p, addk, dt, vals[j], 0); ok = a.acc0 >= 0; }
            if (op == AQG_RED_VAR || op == AQG_RED_STDDEV) {
                if (wide) { a.acc2 = aqg_add_acc(p, addk, dt, vals[j], 1, 1); a.acc3 = aqg_add_acc(p, addk, dt, vals[j], 1, 2); ok = ok && a.acc2 >= 0 && a.acc3 >= 0; }
                else { a.acc2 = aqg_add_acc(p, addk, dt, vals[j], 1); ok = ok && a.acc2 >= 0; }
            }
            if (op != AQG_RED_SUM) p->need_count = 1;
            break;
        case AQG_RED_SUMSQ:                                               // (internal: the accumulators VAR calls acc2 / acc3, emitted like a SUM)
            if (wide) { a.acc0 = aqg_add_acc(p, addk, dt, vals[j], 1, 1); a.acc1 = aqg_add_acc(p, addk, dt, vals[j], 1, 2); ok = a.acc0 >= 0 && a.acc1 >= 0; }
            else { a.acc0 = aqg_add_acc(p, addk, dt, vals[j], 1); ok = a.acc0 >= 0; }
            break;
        case AQG_RED_MIN: a.acc0 = aqg_add_acc(p, ACC_MIN, dt, vals[j], 0); ok = a.acc0 >= 0; break;
        case AQG_RED_MAX: a.acc0 = aqg_add_acc(p, ACC_MAX, dt, vals[j], 0); ok = a.acc0 >= 0; break;
        case AQG_RED_COUNT: p->need_count = 1; break;
        default: return aqg_fail(ctx, AQG_ERR_DTYPE, "group-by: FIRST/LAST need row lists (use aqg_grouped_reduce)");
        }
        if (!ok) return aqg_fail(ctx, AQG_ERR_ARG, "group-by: too many accumulators (8 per call)");
    }
    return AQG_OK;
}

namespace {

// LDS mode, small: one workgroup's table (75 % load) fits 64 KB, several workgroups per CU.
// LDS mode, big:   one 1024-thread workgroup per CU with a table of up to 150 KB, and up to MAX_PASSES passes over the
//                  rows, each aggregating the keys of one hash class (agg_kernel).  Beyond that rows go straight to HBM.
constexpr uint32_t MAX_PASSES = 4;
constexpr size_t LDS_SMALL = 76 * 1024, LDS_BIG = 150 * 1024;      // small: two workgroups per CU still fit
// LDS table of one round-1 partition: as many slots as fit the budget (the slot of a hash is a multiply-shift, so the capacity need not
// be a power of two).  Partitions are sized for a LOW load factor: probe sequences are walked by whole wavefronts, and measured at 1e9
// rows / 1e7 groups the LDS aggregation takes 3.9 ms at load 0.20, 5.6 ms at 0.22-0.25, 6.7-7.2 ms at 0.30-0.33 and 18 ms at 0.6 (two
// accumulators), while one more partition bit costs the two scatter passes 1-2 ms.
constexpr size_t PART_LDS_BYTES = 60 * 1024;
constexpr uint64_t PART_LF1000 = 210;

// dense key domain (dense.hip): direct-indexed tables when the product of the key columns' value ranges is small --
// also for tuples wider than 64 bits.  Costs one more pass over the key columns, so it is only tried where the
// alternatives are the multi-pass hashed table or the partition pipeline.
int plan_dense(aqg_ctx* ctx, aqg_groupby* h, AggPlan& p) {
    const KeySpec& ks = p.ks;
    long long mins[MAXKEYS], maxs[MAXKEYS];
    bool ok = false;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, 4096));
    // large inputs: ranges from the first 2^20 rows (a full pass over the key columns costs a third of Q2); the kernels check
    // every row against them and flag a miss, which re-runs the call once with exact ranges (and remembers it in the handle)
    const bool sampled = p.n >= (1u << 22) && !h->dense_exact;
    bool cached = sampled && h->range_valid && h->range_nkeys == ks.nkeys && h->range_n == p.n;
    for (int c = 0; c < ks.nkeys && cached; ++c) cached = h->range_col[c] == ks.col[c] && h->range_dt[c] == ks.dt[c];
    if (cached) { for (int c = 0; c < ks.nkeys; ++c) { mins[c] = h->range_min[c]; maxs[c] = h->range_max[c]; } ok = true; }
    else {
        AQG_TRY(aqg_key_ranges(ctx, ks, sampled ? (1u << 20) : p.n, mins, maxs, &ok, sampled ? p.n : 0u));
        h->range_valid = sampled && ok;
        if (h->range_valid) {
            h->range_nkeys = ks.nkeys; h->range_n = p.n;
            for (int c = 0; c < ks.nkeys; ++c) { h->range_col[c] = ks.col[c]; h->range_dt[c] = ks.dt[c]; h->range_min[c] = mins[c]; h->range_max[c] = maxs[c]; }
        }
    }
    p.dense = ok && aqg_dense_plan(ks, mins, maxs, p.plan.as, p.plan.need_count, &p.dspec);
    p.dspec.sampled = sampled;
    if (p.dense && p.dspec.D <= 1536) {          // (ranges from a sample are fine here: the hashed table takes any key)
        // a tiny domain under a large hint: the small hashed table after all (1024 lanes on a hundred hot direct-indexed
        // slots serialise on LDS atomics: 6.2 ms per 1e9 rows against 2.7 ms)
        const uint32_t small_cap = next_pow2((uint64_t)(p.dspec.D < 64 ? 64 : p.dspec.D) * 4 / 3 + 1);
        if ((size_t)(small_cap + 1) * p.lds_slot_bytes <= LDS_SMALL) { p.dense = false; p.use_lds = true; p.lcap = small_cap < 256 ? 256 : small_cap; p.hint = p.dspec.D; }
    }
    if (p.dense) p.gcap = p.dspec.D;
    return AQG_OK;
}

// fast path eligibility: LDS mode, 16-byte aligned columns, one or two 4-byte integer keys or one 8-byte key, up to four accumulators
// of any kind over integer / floating value columns (also the first pass of aqg_groupby_build: no accumulators, only the distinct keys)
void plan_fast(AggPlan& p) {
    const KeySpec& ks = p.ks;
    const AccSpec& as = p.plan.as;
    auto key32 = [&](int j) { return (ks.dt[j] == AQG_INT32 || ks.dt[j] == AQG_UINT32) && ((uintptr_t)ks.col[j] & 15) == 0; };
    // two 4-byte key columns, or one 8-byte key column whose bits are the packed key
    p.fast_key8 = ks.nkeys == 1 && !ks.wide && (ks.dt[0] == AQG_INT64 || ks.dt[0] == AQG_UINT64) && ((uintptr_t)ks.col[0] & 15) == 0;
    p.fast_k64 = (ks.nkeys == 2 && !ks.wide && ks.total_bytes == 8 && key32(0) && key32(1)) || p.fast_key8;
    p.fast = p.use_lds && !p.plan.sj && !p.big_lds && ((p.k32 && key32(0)) || p.fast_k64) && p.n >= 8 && (as.nacc >= 1 || p.plan.need_count || p.for_build) && as.nacc <= 4;
    // value columns: 4 bytes wide, or 4 and 8 bytes wide (an int64 sum takes two accumulators)
    auto wide_dt = [](int dt) { return dt == AQG_INT64 || dt == AQG_UINT64 || dt == AQG_DOUBLE; };
    auto narrow_dt = [](int dt) { return dt == AQG_INT32 || dt == AQG_UINT32 || dt == AQG_FLOAT; };
    auto tiny_dt = [](int dt) { return dt == AQG_INT8 || dt == AQG_UINT8 || dt == AQG_BOOL || dt == AQG_INT16 || dt == AQG_UINT16; };
    // some value column is 1, 2 or 8 bytes wide: the VW = 8 instantiation (it takes 4-byte ones, too)
    for (int a = 0; a < as.nacc; ++a) p.fast_v8 = p.fast_v8 || wide_dt(as.dt[a]) || tiny_dt(as.dt[a]);
    FastVals& fv = p.fv;
    for (int a = 0; a < as.nacc && p.fast; ++a) {
        const int dt = as.dt[a];
        if ((uintptr_t)as.col[a] & 15) p.fast = false;
        if (p.fast_v8) { if (!wide_dt(dt) && !narrow_dt(dt) && !tiny_dt(dt)) p.fast = false; }
        else if (as.part[a] || !narrow_dt(dt)) p.fast = false;
        fv.col[a] = as.col[a];
        fv.vkind[a] = dt == AQG_INT32 ? 0 : dt == AQG_UINT32 ? 1 : dt == AQG_FLOAT ? 2 : dt == AQG_INT64 ? 3 : dt == AQG_UINT64 ? 4 : dt == AQG_DOUBLE ? 5 :
                      dt == AQG_INT8 ? 6 : (dt == AQG_UINT8 || dt == AQG_BOOL) ? 7 : dt == AQG_INT16 ? 8 : 9;
        fv.kind[a] = as.kind[a];
        fv.square[a] = as.square[a];
        fv.part[a] = as.part[a];
    }
}

// Every decision of one attempt, with the device sampling they need (dense key ranges, the look-up build's domain).
// table_out: the caller takes the group table itself; dense_out: the caller takes a direct-indexed table
int make_agg_plan(aqg_ctx* ctx, const KeySpec& ks_in, const Plan& plan_in, uint32_t n, uint32_t hint, bool for_build, bool table_out, bool dense_out,
                  aqg_groupby* h, AggPlan* out) {
    const aqg_switch_set& sw = aqg_switches();
    AggPlan& p = *out;
    p = AggPlan{};
    p.n = n; p.for_build = for_build; p.ks = ks_in; p.plan = plan_in; p.hint = hint;
    KeySpec& ks = p.ks;
    const AccSpec& as = p.plan.as;
    // Packed keys (<= 8 bytes) with more groups expected than their partition plans reach (2^25) are handled as WIDE tuples: that plan
    // partitions on a hash of the tuple and compares tuples through representative rows, whatever the key width, up to one group per row
    // (2e8 unique 4-byte keys: 107 ms through the HBM table of scattered device atomics they fell to before)
    if (!ks.wide && !for_build && hint > (1u << 25) && n >= (1u << 20) && !p.plan.sj && as.nacc <= 4) {
        ks.wide = 1;
        for (int j = 0; j < ks.nkeys; ++j) ks.shift[j] = 0;
    }
    // A BUILD above the LDS tables takes the partition plans too (partition1.hip, partition_assign.hip: the group table with counts, then one more pass over the
    // partitioned rows for the id of every row) instead of inserting every row into an HBM table and looking every row up again
    p.build_part = for_build && !sw.disable_build_partition && !ks.wide && n >= (1u << 20) && hint > 3072 && hint <= (1u << 25) && hint < sw.sorted_tail_min;
    if (p.build_part) p.plan.need_count = 1;          // the group sizes come out of the partition aggregation
    p.k32 = ks.nkeys == 1 && ks.total_bytes == 4;
    p.gcap = next_pow2((uint64_t)(hint < 512 ? 512 : hint) * 2);
    p.use_lds = hint <= 3072 && !ks.wide;   // wide tuples compare against HBM-resident rows: HBM mode
    p.lcap = p.use_lds ? next_pow2((uint64_t)(hint < 64 ? 64 : hint) * 4 / 3 + 1) : 0;
    if (p.use_lds && p.lcap < 256) p.lcap = 256;
    // the star join's LDS also holds the dimension side (up to 64 KiB): its group table stops at 2048 slots, and the groups beyond its
    // load limit (1536) are summed in the global table -- correct up to the 3072 groups the call promises, slower beyond 1536
    if (p.plan.sj && p.lcap > 2048) p.lcap = 2048;
    p.lds_slot_bytes = 8 + 8 * (size_t)as.nacc + (p.k32 ? 0 : 4) + (p.plan.need_count ? 4 : 0);
    if (p.use_lds && (size_t)(p.lcap + 1) * p.lds_slot_bytes > LDS_SMALL) { p.use_lds = false; p.lcap = 0; }
    if (p.plan.sj && !(p.use_lds && p.k32))
        return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_groupby_sum: needs one 4-byte group key and at most 3072 groups (compose aqg_join_lookup / aqg_gather / aqg_ewise / aqg_groupby_agg beyond that)");
    p.npass = 1;
    if (!p.plan.sj && !p.use_lds && (!for_build || dense_out) && n >= (1u << 20) &&
        (uint64_t)hint <= (uint64_t)(DENSE_LDS_BYTES / aqg_dense_slot_bytes(as, p.plan.need_count)) * DENSE_MAX_PASSES)
        AQG_TRY(plan_dense(ctx, h, p));
    hint = p.hint;                                    // (from here on the effective hint)
    if (!p.dense && !p.use_lds && !ks.wide && n >= (1u << 20)) {
        const uint32_t max_slots = (uint32_t)(LDS_BIG / p.lds_slot_bytes) - 1;
        const uint32_t per_pass = max_slots - (max_slots >> 2);
        const uint64_t want = ((uint64_t)hint + per_pass - 1) / per_pass;
        if (want <= MAX_PASSES) { p.use_lds = p.big_lds = true; p.npass = (uint32_t)want; p.lcap = max_slots; }
    }
    p.lds_group_cap = p.use_lds ? (uint64_t)p.npass * (p.lcap - (p.lcap >> 2)) : 0;
    p.small_rank = hint <= 4096;
    p.nwords = aqg_ceil_div(n, 32); p.ntiles = aqg_ceil_div(p.nwords, 1024);
    // groups beyond the LDS tables: partition the rows instead of hammering an HBM table with scattered atomics
    // (partition.hip: h2o Q5, 1e9 rows, 1e7 groups: 42 ms against 141 ms); the build path keeps the HBM table because
    // its second pass looks keys up in it
    const int ksz = ks.total_bytes <= 4 ? 4 : 8;
    const uint32_t record_cap = (uint32_t)((uint64_t)hint + hint / 4 + 4096 > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : (uint64_t)hint + hint / 4 + 4096);   // compact record table
    p.use_part = !p.dense && !p.use_lds && !ks.wide && (!for_build || p.build_part) && n >= (1u << 20) && hint <= (1u << 25);
    if (p.use_part && for_build) {                  // (the build's id pass knows the one- and two-level plans only)
        const uint32_t bp = aqg_partition_parts(ksz, as, p.plan.need_count, hint);
        if (!bp || bp > AQG_P2_MAXPARTS) p.use_part = false;
    }
    // the build over a dense key domain small enough for a key -> id look-up table (lookup_assign_kernel): no partitioned rows kept, no routing
    if (p.use_part && for_build && !h->no_lookup_build && ks.nkeys == 1 && (ks.dt[0] == AQG_INT32 || ks.dt[0] == AQG_UINT32) &&
        ((uintptr_t)ks.col[0] & 15) == 0 && n >= (1u << 22)) {
        long long mn[MAXKEYS], mx[MAXKEYS];
        bool ok = false;
        AQG_TRY(aqg_ws_reset(ctx));
        AQG_TRY(aqg_ws_ensure(ctx, 4096));
        AQG_TRY(aqg_key_ranges(ctx, ks, 1u << 20, mn, mx, &ok, n));         // (a sample spread over the column: the look-up pass checks every row)
        if (ok && mx[0] >= mn[0]) {
            const long long span = mx[0] - mn[0] + 1, room = span / 64 + 1024, lo = mn[0] - room, hi = mx[0] + room;
            if (hi - lo + 1 <= (1ll << 21)) { p.lookup_build = true; p.lk_min = (uint32_t)lo; p.lk_D = (uint32_t)(hi - lo + 1); }
        }
    }
    if (p.use_part) {
        p.part_lcap = (uint32_t)(PART_LDS_BYTES / (16 + 8 * (size_t)as.nacc)) - 1;
        p.pbits = 10;                                  // at least 1024 partitions: every CU gets several
        while (p.pbits < 16 && ((uint64_t)hint >> p.pbits) * 1000 > (uint64_t)p.part_lcap * PART_LF1000) ++p.pbits;
        p.gcap = record_cap;
    }
    // partition1.hip: ONE level up to ~1000 partitions (every plane moves once), two levels of <= 64 bins up to 4096 (the runs a
    // tile writes stay a kilobyte long); beyond that the round-1 pipeline of partition.hip
    const bool p1_off = sw.disable_p1 && !for_build;
    p.part_layout = AQG_P1_LAYOUT_DENSE_IDS;
    const uint32_t parts = p.use_part && !p1_off ? aqg_partition_parts(ksz, as, p.plan.need_count, hint, &p.part_layout) : 0;
    p.p1_bins = parts && parts <= sw.p1_max && parts <= AQG_P1_MAXBINS ? parts : 0;
    p.p2_parts = parts && !p.p1_bins && parts <= AQG_P2_MAXPARTS ? parts : 0;
    // every row its own group out of a partition plan: the result can be written from the input rows (emit_rows_kernel) -- when nobody asks for the table itself
    p.rows_possible = n >= (1u << 16) && !for_build && !p.plan.sj && !table_out;
    // tuples wider than 8 bytes with many groups (h2o Q10): hash-partitioned rows, every partition grouped inside LDS
    p.use_wpart = !p1_off && !p.dense && !p.use_lds && ks.wide && !for_build && !p.plan.sj && n >= (1u << 20) && hint > (1u << 20) && as.nacc <= 4 &&
                  !h->no_wide_part && aqg_partitionw_applies(ks, as, n, hint);
    if (p.use_wpart) p.gcap = record_cap;
    // more than ~1.6e7 groups expected out of a partition plan: the records are ORDERED (aqg_sorted_tail) instead of ranked through a
    // bitmap over the rows and gathered (h2o Q10, 1e9 groups: that tail took 219 of 317 ms and fetched 900 GB)
    p.sorted_tail = (p.use_part || p.use_wpart) && !for_build && hint >= sw.sorted_tail_min && !h->no_sorted_tail && aqg_sorted_tail_plan(n, as.nacc, ks.wide != 0, nullptr);
    p.ordered_emit = !p.small_rank && hint >= (1u << 20) && !p.sorted_tail;
    // few groups over many rows: the context's all-zero bitmap, only the tiles that hold a bit are scanned (bitmap_set_kernel)
    p.sparse_rank = !p.small_rank && !p.sorted_tail && p.nwords >= (1u << 16) && (uint64_t)hint * 64 < p.nwords;
    plan_fast(p);
    p.pass = p.plan.sj ? RowPass::STARJOIN : p.fast ? RowPass::FAST_LDS : p.dense ? RowPass::DENSE : p.use_wpart ? RowPass::PART_WIDE :
             p.p1_bins ? RowPass::PART_ONE : p.p2_parts ? RowPass::PART_TWO : p.use_part ? RowPass::PART_ROUND1 : RowPass::HASHED;
    p.defer = n && (p.pass == RowPass::FAST_LDS || p.pass == RowPass::STARJOIN) && p.small_rank;
    // the plain call over one 4-byte key and 4-byte values streams its rows by LDS-DMA (groupby_few.hip); builds, callers that take
    // the table and every other fast shape keep agg32_kernel
    if (p.pass == RowPass::FAST_LDS && p.defer && !for_build && !table_out && !p.fast_k64 && !p.fast_v8 && as.nacc >= 1 &&
        aqg_few_fits(as.nacc, p.plan.need_count != 0, p.lcap))
        p.pass = RowPass::FEW_LDS;
    return AQG_OK;
}

// the workspace of an attempt: the group table, the ids of its occupied slots, the ranking bitmap, the partition or ordering buffers
int agg_workspace(aqg_ctx* ctx, const AggPlan& p, AggBufs* out) {
    const KeySpec& ks = p.ks;
    const AccSpec& as = p.plan.as;
    AggBufs& b = *out;
    b = AggBufs{};
    const size_t slots = b.slots = (size_t)p.gcap + 1;
    uint32_t stride = 16;
    while (stride < 16 + 8 * (uint32_t)as.nacc) stride <<= 1;
    size_t need = slots * (size_t)stride + 4096 + 256 * 16;
    if (!p.sorted_tail) need += slots * (4 + 4 + 4);
    if (!p.small_rank && !p.sorted_tail) need += (size_t)p.nwords * 8 + (size_t)p.ntiles * 8 + 8192;
    if (p.ordered_emit) need += slots * 4 + 4096;
    size_t part_need = 0;
    if (p.use_wpart) part_need = aqg_partitionw_ws_bytes(ctx, ks, p.n, as, p.hint) + 65536;
    else if (p.p1_bins) part_need = aqg_partition1_ws_bytes(ctx, ks, p.n, as, p.p1_bins) + 65536;
    else if (p.p2_parts) part_need = aqg_partition2_ws_bytes(ctx, ks, p.n, as, p.p2_parts) + 65536;
    else if (p.use_part) part_need = aqg_partition_ws_bytes(p.n, ks.total_bytes <= 4 ? 4 : 8, as, p.pbits) + 65536;
    // (the partition buffers are dead once the record table is written: the ordering pass takes their place in the arena)
    const size_t sort_need = p.sorted_tail ? aqg_sorted_tail_ws_bytes(p.gcap, p.n, as.nacc, ks.wide != 0) : 0;
    need += part_need > sort_need ? part_need : sort_need;
    if (p.for_build && p.use_part) need += p.lookup_build ? ((size_t)p.lk_D + 64) * 4 + 4096 : aqg_partition_assign_ws_bytes(p.n);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, need));
    GTable& gt = b.gt;
    gt.cap = p.gcap;
    gt.has_count = p.plan.need_count;
    unsigned char* base = nullptr;
    AQG_TRY(aqg_ws_get(ctx, slots * stride, &base));
    const bool records = (p.use_part || p.use_wpart || p.hint > (1u << 17)) && !p.sorted_tail;   // (the ordering pass moves column planes)
    if (records) {
        gt.kb = base; gt.fb = base + 8; gt.cb = base + 12; gt.ab = base + 16;
        gt.kst = gt.fst = gt.cst = gt.ast = stride; gt.astep = 8;
    } else {
        gt.kb = base; gt.fb = base + slots * 8; gt.cb = gt.fb + slots * 4; gt.ab = gt.cb + slots * 4;
        gt.kst = 8; gt.fst = 4; gt.cst = 4; gt.ast = 8; gt.astep = (uint64_t)slots * 8;
    }
    AQG_TRY(aqg_ws_get(ctx, 64, &gt.flags));
    if (p.sorted_tail && p.use_wpart) gt.kb = nullptr;       // wide tuples through the ordering tail: the key word would repeat the first-row plane
    if (!p.sorted_tail) {
        AQG_TRY(aqg_ws_get(ctx, slots, &b.occ));
        AQG_TRY(aqg_ws_get(ctx, slots, &b.gid_of_occ));
        AQG_TRY(aqg_ws_get(ctx, slots, &b.slot_gid));
    }
    if (!p.small_rank && !p.sorted_tail) {
        if (p.sparse_rank) {
            if (ctx->rank_bm_words < p.nwords) {
                if (ctx->rank_bm) { AQG_HIP(ctx, hipStreamSynchronize(ctx->stream)); AQG_HIP(ctx, hipFree(ctx->rank_bm)); ctx->rank_bm = nullptr; ctx->rank_bm_words = 0; }
                if (aqg_scratch_malloc(ctx, &ctx->rank_bm, (size_t)p.nwords * 4) != hipSuccess) { (void)hipGetLastError(); return aqg_fail(ctx, AQG_ERR_NOMEM, "group-by: no memory for the ranking bitmap"); }
                ctx->rank_bm_words = p.nwords;
                AQG_HIP(ctx, hipMemsetAsync(ctx->rank_bm, 0, (size_t)p.nwords * 4, ctx->stream));
            }
            b.bitmap = ctx->rank_bm;
            AQG_TRY(aqg_ws_get(ctx, p.ntiles + 1, &b.tile_mark));
        } else AQG_TRY(aqg_ws_get(ctx, p.nwords, &b.bitmap));
        AQG_TRY(aqg_ws_get(ctx, p.nwords, &b.word_prefix));
        AQG_TRY(aqg_ws_get(ctx, p.ntiles + 1, &b.tile_total));
    }
    if (!p.use_part && !p.use_wpart) aqg_gt_init(ctx, gt, as, slots);
    else AQG_HIP(ctx, hipMemsetAsync(gt.flags, 0, 64 * 4, ctx->stream));
    if (b.bitmap && !p.sparse_rank) AQG_HIP(ctx, hipMemsetAsync(b.bitmap, 0, (size_t)p.nwords * 4, ctx->stream));
    if (b.tile_mark) AQG_HIP(ctx, hipMemsetAsync(b.tile_mark, 0, ((size_t)p.ntiles + 1) * 4, ctx->stream));
    return AQG_OK;
}

int pass_fast(aqg_ctx* ctx, const AggPlan& p, const GTable& gt) {
    const size_t lds = (size_t)(p.lcap + 1) * ((p.fast_k64 ? 8 : 4) + 8 * (size_t)p.plan.as.nacc + (p.plan.need_count ? 4 : 0)) + 64;
    // the table is sized by the hint, not by the groups that show up: a large one leaves room for few workgroups per CU, and with 256
    // threads each the LDS round trips of two accumulators per row are no longer hidden (var(v1), 100 groups, hint 1024: two
    // workgroups = 8 wavefronts per CU ran at 43 % of the HBM roofline).  So the workgroup grows with the table: 32 wavefronts per CU.
    const unsigned block = lds <= 20 * 1024 ? 256 : lds <= 40 * 1024 ? 512 : 1024;
    const unsigned bpc = lds <= 20 * 1024 ? 8 : lds <= 40 * 1024 ? 4 : lds <= 78 * 1024 ? 2 : 1;
    const unsigned grid = aqg_grid(ctx, p.n / 8 + 1, block, 2, bpc);
    // (more workgroups than fit the chip cost more in table merges than they gain: 8192 -> +3 %, 32768 -> +30 % on Q1)
    const uint32_t* khi = p.fast_k64 && !p.fast_key8 ? static_cast<const uint32_t*>(p.ks.col[1]) : nullptr;
    return aqg_fast_aggregate(ctx, static_cast<const uint32_t*>(p.ks.col[0]), khi, p.fast_k64, p.fast_v8, p.plan.as.nacc, p.plan.need_count != 0, p.fv, gt, p.n, p.lcap, lds, grid, block);
}

// the partition plans; the packing and range-partition bits of h->plan_bits are learned here
int pass_partitions(aqg_ctx* ctx, const AggPlan& p, aqg_groupby* h, AggBufs& b) {
    const KeySpec& ks = p.ks;
    const AccSpec& as = p.plan.as;
    const size_t mark = ctx->ws_off;
    PartRows* rows = p.for_build && !p.lookup_build ? &b.prows : nullptr;       // the build's id pass reads the partitioned rows
    int pack = h->no_pack ? 0 : 1;
    switch (p.pass) {
    case RowPass::PART_WIDE:
        AQG_TRY(aqg_partitionw_aggregate(ctx, ks, as, p.n, p.plan.need_count, b.gt, p.gcap, h->wide_seed, p.hint, &pack, &h->wide_rows, p.rows_possible));
        if (pack) h->plan_bits |= AQG_PLAN_PACKED_KEYS;
        break;
    case RowPass::PART_ONE:
        AQG_TRY(aqg_partition1_aggregate(ctx, ks, as, p.n, p.p1_bins, p.plan.need_count, b.gt, p.gcap, rows, p.part_layout, &pack));
        if (pack & 2) h->plan_bits |= AQG_PLAN_RANGE_PARTITIONS;
        if (pack & 1) h->plan_bits |= AQG_PLAN_PACKED_VALUES;
        break;
    case RowPass::PART_TWO:
        AQG_TRY(aqg_partition2_aggregate(ctx, ks, as, p.n, p.p2_parts, p.plan.need_count, b.gt, p.gcap, rows, &pack, p.part_layout));
        if (pack & 1) h->plan_bits |= AQG_PLAN_PACKED_VALUES;
        if (pack & 2) h->plan_bits |= AQG_PLAN_RANGE_PARTITIONS;
        break;
    default: AQG_TRY(aqg_partition_aggregate(ctx, ks, as, p.n, p.pbits, p.part_lcap, p.plan.need_count, b.gt, p.gcap));
    }
    if (p.sorted_tail) ctx->ws_off = mark;       // stream order: whatever is allocated there next is written after these kernels
    else aqg_occ_iota(ctx, b.occ, b.slots);
    return AQG_OK;
}

// the plan a row pass stands for in h->plan_bits (the star join has no bit of its own)
uint32_t row_pass_bits(const AggPlan& p) {
    constexpr uint32_t bits[] = {0, AQG_PLAN_FAST_LDS, AQG_PLAN_FAST_LDS, AQG_PLAN_DENSE, AQG_PLAN_PART_WIDE, AQG_PLAN_PART_ONE, AQG_PLAN_PART_TWO, AQG_PLAN_PART_ROUND1};   // (RowPass order)
    if (p.pass == RowPass::HASHED) return p.big_lds ? AQG_PLAN_BIG_LDS : p.use_lds ? AQG_PLAN_SMALL_LDS : AQG_PLAN_HBM_TABLE;
    return bits[(int)p.pass] | (p.sorted_tail ? AQG_PLAN_SORTED_TAIL : 0u);      // (only partition plans order their records)
}

// the pass over the rows, then collect: the ids of the occupied slots (the partition plans wrote them already)
int row_pass(aqg_ctx* ctx, const AggPlan& p, aqg_groupby* h, AggBufs& b) {
    if (p.n) {
        if (p.pass != RowPass::STARJOIN) h->plan_bits = row_pass_bits(p);
        switch (p.pass) {
        case RowPass::STARJOIN: AQG_TRY(aqg_pass_starjoin(ctx, p, b.gt)); break;
        case RowPass::FAST_LDS: AQG_TRY(pass_fast(ctx, p, b.gt)); break;
        case RowPass::FEW_LDS:
            AQG_TRY(aqg_few_aggregate(ctx, static_cast<const uint32_t*>(p.ks.col[0]), p.plan.as.nacc, p.plan.need_count != 0, p.fv, b.gt, p.n, p.lcap));
            break;
        case RowPass::DENSE: AQG_TRY(aqg_dense_aggregate(ctx, p.ks, p.dspec, p.plan.as, p.n, p.plan.need_count, b.gt)); break;
        case RowPass::HASHED: AQG_TRY(aqg_pass_hashed(ctx, p, b.gt)); break;
        default: AQG_TRY(pass_partitions(ctx, p, h, b));
        }
    }
    if (!(p.n && (p.use_part || p.use_wpart))) aqg_collect(ctx, b.gt, b.occ, b.slots);
    return AQG_OK;
}

// The flag words ([0] overflow, [1] occupied slots, [3] a row outside the sampled key ranges, [4], [5] diagnostics, [6] a value outside
// its packed field): a retry -- remembered in the handle -- an overflow, or the group count *G
int judge_flags(const AggPlan& p, const uint32_t* fl, aqg_groupby* h, uint32_t* G) {
    if (p.dense && fl[3]) { h->dense_exact = true; h->range_valid = false; return AQG_ERR_RANGE_MISS; }
    if (p.use_wpart && fl[6]) { h->no_pack = true; return AQG_ERR_RANGE_MISS; }      // a key outside the sampled range of its packed field: once more, unpacked
    if (p.use_wpart && fl[0]) {
        // a partition larger than LDS holds (fl[5] rows).  A little over: chance (a million partitions sized at mean + 6 sigma) --
        // ONE more try with another seed of the partition hash; far over, or over again: a tuple that dominates the input, which no
        // seed spreads -- the HBM table, same hint
        if (aqg_switches().debug_flags) fprintf(stderr, "aqg: wide partition plan gave up: flags %u %u %u %u, partition %u holds %u rows (n %u, hint %u, seed %u)\n", fl[0], fl[1], fl[2], fl[3], fl[4], fl[5], p.n, p.hint, h->wide_seed);
        const uint32_t rcap = h->wide_rows ? h->wide_rows : aqg_partitionw_rows(p.ks, p.plan.as, p.n, p.hint);
        if (!fl[5]) return AQG_ERR_OVERFLOW;     // no partition was too large: the record table (out_cap) was -- more groups than hinted, the caller grows the hint
        if (h->wide_seed == 0 && fl[5] <= rcap + rcap / 2) h->wide_seed = 0x5BD1E995u; else h->no_wide_part = true;
        return AQG_ERR_RANGE_MISS;
    }
    if ((p.use_part || p.use_wpart) && fl[6]) { h->no_pack = true; return AQG_ERR_RANGE_MISS; }     // a value outside the sampled range of its packed field: once more, unpacked
    if (fl[0]) return AQG_ERR_OVERFLOW;
    *G = fl[1];
    if (p.small_rank && *G > 4096) return AQG_ERR_OVERFLOW;
    if (p.use_lds && *G > p.lds_group_cap && *G > p.hint) return AQG_ERR_OVERFLOW;   // correct but slow (overflow rows took the HBM path): re-plan
    return AQG_OK;
}

// The fast kernel or the fused star join with a small table (h2o Q1 / Q4, config 4): every kernel of the tail reads the group count from the device flags and
// the outputs are sized by the table, so nothing on the host stands between collect and emit (a round trip there cost 26 us
// of a 1.45 ms step).  The flag words -- final once collect has run -- are copied to pinned memory right here, behind
// collect and in FRONT of the tail, and the host waits for that copy only: the call returns with first rows / rank / emit
// still queued (stream-ordered, like every device result of this library), so the host's way to the next call overlaps them.
// An overflow is noticed with the tail already queued on it: those kernels are bounded by the table and by `gmax`, their
// results are discarded and the call re-plans as before.
int read_flags(aqg_ctx* ctx, const AggPlan& p, aqg_groupby* h, AggBufs& b, uint32_t* G) {
    if (p.defer) {
        AQG_TRY(aqg_host_stage(ctx, 16, reinterpret_cast<void**>(&b.pinned_flags)));
        AQG_HIP(ctx, hipMemcpyAsync(b.pinned_flags, b.gt.flags, 16, hipMemcpyDeviceToHost, ctx->stream));
        AQG_HIP(ctx, hipEventRecord(ctx->ev_flags, ctx->stream));
        return AQG_OK;
    }
    uint32_t fl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    AQG_HIP(ctx, hipMemcpyAsync(fl, b.gt.flags, 32, hipMemcpyDeviceToHost, ctx->stream));
    AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return judge_flags(p, fl, h, G);
}

// One attempt at a given global capacity.  Returns AQG_ERR_OVERFLOW when the table filled up.
int run_agg(aqg_ctx* ctx, const KeySpec& ks_in, const Plan& plan_in, uint32_t n, uint32_t hint, bool for_build, aqg_groupby* h,
            GTable* gt_out, uint32_t** slot_gid_out, uint32_t** occ_out = nullptr, DenseOut* dense_out = nullptr) {
    AggPlan p;
    AQG_TRY(make_agg_plan(ctx, ks_in, plan_in, n, hint, for_build, gt_out || slot_gid_out || occ_out, dense_out != nullptr, h, &p));
    AggBufs b;
    AQG_TRY(agg_workspace(ctx, p, &b));
    AQG_TRY(row_pass(ctx, p, h, b));
    uint32_t G = 0;                                   // (deferred: unknown until the tail is queued)
    AQG_TRY(read_flags(ctx, p, h, b, &G));
    // every row its own group: the result is a map of the input (emit_rows_kernel) -- nothing to rank or order
    const bool row_emit = p.rows_possible && !p.defer && G == n && (p.use_part || p.use_wpart);
    if (row_emit) h->plan_bits |= AQG_PLAN_ROW_EMIT;
    SortedParts sparts;
    AQG_TRY(aqg_rank_groups(ctx, p, b, G, row_emit, &sparts));
    AQG_TRY(aqg_emit_outputs(ctx, p, h, b, G, row_emit, sparts));
    if (p.defer) {
        uint32_t fl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        AQG_HIP(ctx, hipEventSynchronize(ctx->ev_flags));
        memcpy(fl, b.pinned_flags, 16);
        AQG_TRY(judge_flags(p, fl, h, &G));
        ctx->tail_in_flight = true;
    }
    AQG_TRY(aqg_assign_build_ids(ctx, p, h, b, G));
    h->ngroups = G;
    if (gt_out) *gt_out = b.gt;
    if (dense_out) { dense_out->used = p.dense; if (p.dense) dense_out->spec = p.dspec; }
    if (slot_gid_out) *slot_gid_out = b.slot_gid;
    if (occ_out) *occ_out = b.occ;
    return AQG_OK;
}

} // namespace

int aqg_run_with_retry(aqg_ctx* ctx, const KeySpec& ks, const Plan& plan, uint32_t n, uint32_t hint, bool for_build, aqg_groupby* h,
                   GTable* gt_out, uint32_t** slot_gid_out, uint32_t** occ_out, DenseOut* dense_out) {
    uint64_t cur = hint ? hint : (h->hint_used ? h->hint_used : 1024);
    if (plan.sj && !hint && cur > 3072) cur = 3072;                   // (a handle that served a larger group-by before)
    if (!hint && !h->hint_used && n >= (1u << 22) && !plan.sj) { const uint64_t e = aqg_estimate_groups(ctx, ks, n); if (e > cur) cur = e; }
    for (int attempt = 0; attempt < 12; ++attempt) {
        if (cur > n && n) cur = n;
        int rc = run_agg(ctx, ks, plan, n, (uint32_t)cur, for_build, h, gt_out, slot_gid_out, occ_out, dense_out);
        // (exact key ranges now; or the wide-tuple plan with another hash seed, then without it: at most three repeats)
        for (int again = 0; again < 3 && rc == AQG_ERR_RANGE_MISS; ++again) rc = run_agg(ctx, ks, plan, n, (uint32_t)cur, for_build, h, gt_out, slot_gid_out, occ_out, dense_out);
        if (rc != AQG_ERR_OVERFLOW) { if (rc == AQG_OK) h->hint_used = (uint32_t)cur; return rc; }
        if (n && cur >= n) return aqg_fail(ctx, AQG_ERR_OVERFLOW, "group-by: table overflow at full capacity");
        // (x16 -- but not past 2^25 in one step: beyond it packed keys leave the partition plans)
        const uint64_t next = cur < (1ull << 25) && cur * 16 > (1ull << 25) ? (1ull << 25) : cur * 16;
        cur = plan.sj && cur < 3072 && next > 3072 ? 3072 : next;     // (the star join takes no more: its last step is its limit, whatever the hint was)
    }
    return aqg_fail(ctx, AQG_ERR_OVERFLOW, "group-by: table overflow");
}

extern "C" {

void aqg_groupby_destroy(aqg_groupby* g) {
    if (!g) return;
    // result columns go back to the context's pool (the next handle takes them without a hipMalloc / hipFree pair); what does not
    // fit there is freed, and hipFree waits for the device
    aqg_ctx* ctx = g->ctx;
    for (int k = 0; k < MAXKEYS; ++k) aqg_pool_give(ctx, g->keys_out[k], g->cap_keys[k]);
    for (int j = 0; j < MAXAGG; ++j) aqg_pool_give(ctx, g->results[j], g->cap_results[j]);
    aqg_pool_give(ctx, g->first_rows, g->cap_first);
    aqg_pool_give(ctx, g->counts, g->cap_counts);
    aqg_pool_give(ctx, g->reversemap, g->cap_rows * 4);
    if (g->scratch) aqg_groupby_destroy(g->scratch);
    if (g->scratch2) aqg_groupby_destroy(g->scratch2);
    if (g->scratch3) aqg_groupby_destroy(g->scratch3);
    aqg_pool_give(ctx, g->flat_off, g->cap_flat_off);
    aqg_pool_give(ctx, g->flat_heads, g->cap_flat_heads);
    aqg_pool_give(ctx, g->flat_short, g->cap_flat_short);
    aqg_pool_give(ctx, g->flat_gid, g->cap_flat_gid);
    if (g->first_rows64) hipFree(g->first_rows64);
    for (int i = 0; i < 2 * MAXKEYS; ++i) if (g->norm_buf[i]) hipFree(g->norm_buf[i]);
    if (g->xkeys) hipFree(g->xkeys);
    if (g->xvals) hipFree(g->xvals);
    delete g;
}
uint32_t aqg_groupby_ngroups(const aqg_groupby* g) { return g ? g->ngroups : 0; }
uint32_t aqg_groupby_nrows(const aqg_groupby* g) { return g ? g->n : 0; }
const uint32_t* aqg_groupby_reversemap(const aqg_groupby* g) { return g && g->has_reversemap ? g->reversemap : nullptr; }
const uint32_t* aqg_groupby_counts(const aqg_groupby* g) { return g && g->has_counts ? g->counts : nullptr; }
const uint32_t* aqg_groupby_first_rows(const aqg_groupby* g) { return g && !g->sharded ? g->first_rows : nullptr; }
uint32_t aqg_groupby_plan(const aqg_groupby* g) { return g ? g->plan_bits : 0; }
const void* aqg_groupby_agg_result(const aqg_groupby* g, int j) { return g && j >= 0 && j < g->nagg ? g->results[j] : nullptr; }

int aqg_groupby_agg(aqg_ctx* ctx, int nkeys, const int* key_dtypes, const void* const* keys, int naggs, const int* ops,
                    const int* val_dtypes, const void* const* vals, uint32_t n, uint32_t max_groups_hint, aqg_groupby** out) {
    if (!ctx || !out || !key_dtypes || !keys) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_groupby_agg: bad argument");
    AQG_CHECK_ROWS(ctx, n, "aqg_groupby_agg");
    Plan plan;
    AQG_TRY(aqg_make_plan(ctx, naggs, ops, val_dtypes, vals, n, &plan));
    aqg_handle_guard hg(out);
    aqg_groupby* h = hg.h;
    h->ctx = ctx; h->n = n; h->has_reversemap = false; h->sharded = false;
    ctx->tail_in_flight = false;
    KeySpec ks;
    int nn = 0, ndt[MAXKEYS];
    const void* ncol[MAXKEYS];
    AQG_TRY(aqg_normalize_keys(ctx, h, nkeys, key_dtypes, keys, n, &nn, ndt, ncol));
    AQG_TRY(aqg_make_keyspec(ctx, nn, ndt, ncol, n, &ks));
    AQG_TRY(aqg_run_with_retry(ctx, ks, plan, n, max_groups_hint, false, h, nullptr, nullptr));
    if (!ctx->tail_in_flight) AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (small tables: the group count is known, the tail is stream-ordered)
    return hg.hand_over();
}

int aqg_join_groupby_sum(aqg_ctx* ctx, int key_dtype, const void* dim_keys, int dim_val_dtype, const void* dim_vals, uint32_t nb,
                         const void* fact_fk, int group_key_dtype, const void* group_keys, int val_dtype, const void* fact_vals, uint32_t n,
                         uint32_t max_groups_hint, aqg_groupby** out) {
    if (!ctx || !out || ((!dim_keys || !dim_vals) && nb) || ((!fact_fk || !group_keys || !fact_vals) && n))
        return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_groupby_sum: bad argument");
    auto i32 = [](int t) { return t == AQG_INT32 || t == AQG_UINT32; };
    if (!i32(key_dtype) || !i32(dim_val_dtype) || !i32(group_key_dtype) || !i32(val_dtype))
        return aqg_fail(ctx, AQG_ERR_DTYPE, "aqg_join_groupby_sum: 4-byte integer columns only");
    if (nb > 4096) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_join_groupby_sum: the dimension side must fit LDS (<= 4096 rows)");
    AQG_CHECK_ROWS(ctx, n, "aqg_join_groupby_sum");
    StarJoin sj;
    sj.dim_keys = static_cast<const uint32_t*>(dim_keys); sj.dim_vals = static_cast<const uint32_t*>(dim_vals); sj.nb = nb;
    sj.dcap = next_pow2((uint64_t)(nb < 8 ? 8 : nb) * 2);
    sj.fk = static_cast<const uint32_t*>(fact_fk); sj.vals = static_cast<const uint32_t*>(fact_vals);
    sj.val_signed = val_dtype == AQG_INT32; sj.dim_signed = dim_val_dtype == AQG_INT32;
    KeySpec ks;
    const void* kcols[1] = {group_keys};
    AQG_TRY(aqg_make_keyspec(ctx, 1, &group_key_dtype, kcols, n, &ks));
    // the sum of the exact products is an 8-byte-integer SUM: two accumulators (low / high halves), emitted as 128 bits;
    // unsigned x unsigned products are summed as unsigned
    Plan plan;
    const int op = AQG_RED_SUM, pdt = (sj.val_signed || sj.dim_signed) ? AQG_INT64 : AQG_UINT64;
    const void* pv[1] = {fact_vals};
    AQG_TRY(aqg_make_plan(ctx, 1, &op, &pdt, pv, n, &plan));
    plan.sj = &sj;
    aqg_handle_guard hg(out);
    aqg_groupby* h = hg.h;
    h->ctx = ctx; h->n = n; h->has_reversemap = false;
    ctx->tail_in_flight = false;
    AQG_TRY(aqg_run_with_retry(ctx, ks, plan, n, max_groups_hint, false, h, nullptr, nullptr));
    if (!ctx->tail_in_flight) AQG_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (small tables: the group count is known, the tail is stream-ordered)
    return hg.hand_over();
}

} // extern "C"
