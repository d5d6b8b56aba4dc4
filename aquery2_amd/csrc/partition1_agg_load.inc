// partition1_agg_load.inc -- a step's rows in registers (Batch) and the two loaders of the per-partition aggregation kernels of
// partition1_agg.hip, included as text by the shared row loop (partition1_agg_rows.inc) and by the written-out p1_agg_kernel, with
// K, VT, NA, rkeys, rrows and in in scope.
struct Batch { K key[AR]; uint32_t row[AR]; VT v[NA][AR]; };
// A step = SB * AR consecutive rows of the partition, AR per lane.  load_full: a step that lies wholly inside the planes -- vector
// loads, no branch, no clamp.  It is the ONLY form used for the prefetch of the next step: a loader with two code paths (or a
// conditional call) makes hipcc wait for the loads right behind them -- the paths meet in the same registers -- and the
// "prefetch" then overlaps nothing (seen in the ISA: vmcnt(0) ten instructions behind the loads; 5.5 ms per 1e9 rows of Q5).
auto load_full = [&](uint32_t i0, Batch& t) {
    const uint32_t o = i0 + threadIdx.x * AR;
    __builtin_memcpy(t.key, static_cast<const K*>(rkeys) + o, sizeof t.key);
    __builtin_memcpy(t.row, rrows + o, sizeof t.row);
    _Pragma("unroll") for (int a = 0; a < NACC; ++a) {
        if (!in.col[a]) continue;                            // row-index operand (the carried row id) or a field of the key word: taken at the use (a copy here would wait for the load)
        if (!V8 || in.esz[a] == 4) {
            uint32_t w[AR];
            __builtin_memcpy(w, static_cast<const uint32_t*>(in.col[a]) + o, sizeof w);
            _Pragma("unroll") for (int q = 0; q < AR; ++q) t.v[a][q] = w[q];
        } else {
            if constexpr (V8) __builtin_memcpy(t.v[a], static_cast<const uint64_t*>(in.col[a]) + o, sizeof(uint64_t) * AR);
        }
    }
};
// the last, partial step of a partition: row by row from clamped indices (every load is issued; the caller masks rows >= e)
auto load_edge = [&](uint32_t i0, uint32_t e, Batch& t) {
    const uint32_t o = i0 + threadIdx.x * AR;
    _Pragma("unroll") for (int q = 0; q < AR; ++q) {
        const uint32_t i = o + q < e ? o + q : e - 1;
        t.key[q] = static_cast<const K*>(rkeys)[i]; t.row[q] = rrows[i];
        _Pragma("unroll") for (int a = 0; a < NACC; ++a) {
            if (!in.col[a]) continue;
            if (!V8 || in.esz[a] == 4) t.v[a][q] = static_cast<const uint32_t*>(in.col[a])[i];
            else if constexpr (V8) t.v[a][q] = static_cast<const uint64_t*>(in.col[a])[i];
        }
    }
};
