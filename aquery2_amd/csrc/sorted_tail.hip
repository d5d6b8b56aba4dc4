// sorted_tail.hip -- the ordering tail for huge group tables (aqg_sorted_tail*), on the tile scatter of tile_scatter.hip
#include "partition1_int.hpp"
#include "tile_scatter.hpp"

// ==== ordering a huge group table (G ~ N: h2o Q10) ========================================================================================
// Group ids are ranks of first rows.  For <= 1e7 groups groupby_tail.hip ranks through a bitmap over the rows and gathers the records in id
// order; at 1e9 groups those gathers fetch 600 GB.  Here the RECORDS are ordered instead, with the same tile scatter keyed on the first
// row through an ORDER-PRESERVING bin f = umulhi(first_row, M), M = floor(P * 2^32 / rows): up to three levels of <= 64 bins leave P
// partitions, partition p holding exactly the groups whose first rows fall into its row interval -- so its start is the id of its first
// group -- and few enough of them that groupby_tail.hip's sorted_emit_kernel ranks a partition inside LDS (bitmap of the interval) and
// emits the final columns from there.  (host side: aqg_sorted_tail below)

// ---- ordering a huge group table: host ------------------------------------------------------------------------------------------------
// LDS of sorted_emit_kernel per record: key (packed keys only) | first | count | accumulators, plus two bits per row of the interval
static size_t sorted_rec_bytes(int nacc, bool wide) { return (wide ? 0 : 8) + 8 + 8 * (size_t)nacc; }
bool aqg_sorted_tail_plan(uint32_t n_rows, int nacc, bool wide, SortedPlan* out) {
    if (n_rows <= 8192) return false;
    SortedPlan best;
    memset(&best, 0, sizeof best);
    for (size_t budget : {(size_t)64 * 1024, (size_t)150 * 1024}) {
        uint32_t iv = (uint32_t)((budget - 1024) / (sorted_rec_bytes(nacc, wide) + 1)) & ~31u;   // rows (= records at most) one partition may span
        if (iv > 16384) iv = 16384;                                   // one thread per bitmap word, 512 threads
        if (iv < 64) continue;
        uint32_t bits = 1;
        while (bits <= 18 && ((uint64_t)n_rows + ((uint64_t)1 << bits) - 1) / ((uint64_t)1 << bits) + 4 > iv) ++bits;
        if (bits > 18) continue;
        const uint32_t levels = (bits + 5) / 6;
        while (bits < 6 * levels && ((uint64_t)1 << (bits + 1)) <= n_rows / 64) ++bits;   // the levels are paid for: use their bins
        if (best.levels && best.levels <= levels) continue;
        best.levels = levels; best.bits = bits; best.cap = iv;
        best.M = (uint32_t)((((uint64_t)1 << bits) << 32) / n_rows);
        best.lds = (size_t)iv * sorted_rec_bytes(nacc, wide) + 2 * ((size_t)iv / 32 + 8) * 4 + 64;
    }
    if (!best.levels) return false;
    if (out) *out = best;
    return true;
}
size_t aqg_sorted_tail_ws_bytes(uint32_t gcap, uint32_t n_rows, int nacc, bool wide) {
    SortedPlan sp;
    if (!aqg_sorted_tail_plan(n_rows, nacc, wide, &sp)) return 0;
    const size_t per = 2 * (4 + 4 + (wide ? 0 : 8) + 8 * (size_t)nacc);                    // two plane sets
    return ((size_t)gcap + 64) * per + 256 * (16 + 4 * MAXACC) + (size_t)5 * (((size_t)1 << sp.bits) + 64) * 4 + 65536;
}
// records 0 .. G-1 of `gt` (column layout: keys | first rows | counts | accumulators) -> the same planes partitioned by first row
int aqg_sorted_tail(aqg_ctx* ctx, const GTable& gt, uint32_t G, uint32_t n_rows, int nacc, bool wide, SortedParts* out) {
    SortedPlan sp;
    if (!aqg_sorted_tail_plan(n_rows, nacc, wide, &sp)) return aqg_fail(ctx, AQG_ERR_ARG, "ordered group table: no plan for this shape");
    if (gt.fst != 4 || gt.cst != 4 || gt.kst != 8 || gt.ast != 8) return aqg_fail(ctx, AQG_ERR_ARG, "ordered group table: column layout expected");
    const uint32_t PP = 1u << sp.bits, M = sp.M;
    struct Set { uint32_t* first; uint32_t* count; uint64_t* key; uint64_t* acc[MAXACC]; } set[3];
    memset(set, 0, sizeof set);
    set[2].first = reinterpret_cast<uint32_t*>(gt.fb); set[2].count = reinterpret_cast<uint32_t*>(gt.cb); set[2].key = reinterpret_cast<uint64_t*>(gt.kb);
    for (int a = 0; a < nacc; ++a) set[2].acc[a] = reinterpret_cast<uint64_t*>(gt.ab + (size_t)a * gt.astep);
    for (int i = 0; i < 2; ++i) {
        AQG_TRY(aqg_ws_get(ctx, (size_t)G + 64, &set[i].first));
        AQG_TRY(aqg_ws_get(ctx, (size_t)G + 64, &set[i].count));
        if (!wide) AQG_TRY(aqg_ws_get(ctx, (size_t)G + 64, &set[i].key));
        for (int a = 0; a < nacc; ++a) AQG_TRY(aqg_ws_get(ctx, (size_t)G + 64, &set[i].acc[a]));
    }
    auto planes = [&](const Set& from, const Set& to) {
        Planes pl;
        memset(&pl, 0, sizeof pl);
        pl.add_column(from.first, to.first, 4);
        pl.add_column(from.count, to.count, 4);
        if (!wide) pl.add_column(from.key, to.key, 8);
        for (int a = 0; a < nacc; ++a) pl.add_column(from.acc[a], to.acc[a], 8);
        return pl;
    };
    uint32_t *seg, *tp, *cnt, *cur, *bsum;
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &seg));
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &tp));
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &cnt));
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP + 2, &cur));
    AQG_TRY(aqg_ws_get(ctx, (size_t)PP / 1024 + 64 + 8, &bsum));
    const uint32_t h0[2] = {0u, G};
    void* st = nullptr;
    AQG_TRY(aqg_host_stage(ctx, 16, &st));
    memcpy(st, h0, 8);
    AQG_HIP(ctx, hipMemcpyAsync(seg, st, 8, hipMemcpyHostToDevice, ctx->stream));
    const LevelBufs lb{seg, tp, cnt, cur, bsum};
    uint32_t nseg = 1;
    const Set* from = &set[2];
    for (uint32_t l = 0; l < sp.levels; ++l) {
        uint32_t shift;
        const uint32_t nb = 1u << aqg_level_bits(sp.bits, sp.levels, l, &shift);
        const Set& to = set[l & 1];
        AQG_TRY(aqg_scatter_level_counted(ctx, lb, BIN_RAW, false, from->first, planes(*from, to), G, nseg, M, shift, nb - 1, nb, "ordered group table: level"));
        nseg *= nb;
        from = &to;
    }
    memset(out, 0, sizeof *out);
    out->first = from->first; out->count = from->count; out->key = from->key;
    for (int a = 0; a < nacc; ++a) out->acc[a] = from->acc[a];
    out->pstart = seg; out->nparts = nseg; out->M = M; out->cap = sp.cap; out->lds = sp.lds;
    return AQG_OK;
}
