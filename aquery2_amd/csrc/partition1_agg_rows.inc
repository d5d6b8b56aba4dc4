// partition1_agg_rows.inc -- the body of p1_agg_slot_kernel and p1_agg_direct_kernel of partition1_agg.hip, which include it with
//   L               the layout: P1_SLOT or P1_DIRECT
//   NACC, K64, V8   accumulators, 8-byte key word, some value plane has 8-byte elements (then every value travels as 64 bits)
// and their arguments in scope; what a layout has no argument for it declares as a constant (cap, ds).
// It is text, not a __device__ function: a body inlined from a function -- even one that is only moved there, unchanged, and called
// from its one kernel -- is simplified on its own before it is inlined, and every instantiation then differs from the written-out
// kernels in instruction and operand order (profiles/r9_p1_agg_merge.md).  Included, every kernel compiles as it did written out.
// The dense-id layout (p1_agg_kernel) is not in here: see partition1_agg.hip.
using K = key_t_<K64>;
using VT = std::conditional_t<V8, uint64_t, uint32_t>;
constexpr int NA = NACC ? NACC : 1;
extern __shared__ __align__(16) unsigned char smem_raw[];
const uint32_t E = L == P1_SLOT ? cap + 2 : ds.W + 1;                         // entries of the per-group arrays
const uint32_t T = L == P1_SLOT ? E : 0;                                      // entries of the key table
uint64_t* lacc = reinterpret_cast<uint64_t*>(smem_raw);                       // [NACC][E]
K* ktab = reinterpret_cast<K*>(lacc + (size_t)NACC * E);                      // [T] (8-byte keys: behind the accumulators, aligned)
uint32_t* lfirst = reinterpret_cast<uint32_t*>(ktab + T);                     // [E]
uint32_t* lcount = lfirst + E;                                                // [E] (only when need_count)
__shared__ uint32_t lused, lemit, gbase, lins;
const K EMPTYK = empty_key<K64>();
#include "partition1_agg_load.inc"
const uint32_t limit = cap - (cap >> 3);                   // slot layout: more keys than this in one partition and the host re-plans (probe chains grow without bound towards a full table)
for (uint32_t part = blockIdx.x; part < NB; part += gridDim.x) {
    const uint32_t b = pstart[(size_t)part * pstride];
    const uint32_t e = part + 1 < NB ? pstart[(size_t)(part + 1) * pstride] : ntotal;
    if (b == e) continue;
    uint32_t lo = 0, width = 0;
    if constexpr (L == P1_DIRECT) {
        // the piece of the domain this partition owns: x in [lo, hi), lo = the smallest x with umulhi(x, M) >= part
        uint64_t lo64 = (((uint64_t)part << 32) + ds.M - 1) / ds.M, hi64 = ((((uint64_t)part + 1) << 32) + ds.M - 1) / ds.M;
        if (hi64 > ds.D) hi64 = ds.D;
        if (lo64 > hi64) lo64 = hi64;
        lo = (uint32_t)lo64;
        width = (uint32_t)(hi64 - lo64);
        if (width > ds.W) { if (threadIdx.x == 0) out.flags[0] = 1; continue; }   // (the host sized W for every piece)
    }
    constexpr uint32_t STEP = SB * AR;
    const uint32_t nfull = (e - b) / STEP, nsteps = nfull + ((e - b) % STEP ? 1u : 0u);
    // where a prefetch may always read a whole step: the last full step of this partition, or (a partition shorter than a step)
    // any step inside the planes -- what it fetches then is never used
    const uint32_t safe_last = nfull ? b + (nfull - 1) * STEP : (b + STEP <= ntotal ? b : ntotal - STEP);
    Batch cur;
    load_full(nfull ? b : safe_last, cur);                 // in flight while the tables are cleared
    for (uint32_t g = threadIdx.x; g < E; g += SB) {
        if constexpr (L == P1_DIRECT) { if (g >= width && g != ds.W) continue; }
        if constexpr (L == P1_SLOT) ktab[g] = EMPTYK;
        lfirst[g] = NOROW;
        if (need_count) lcount[g] = 0;
        _Pragma("unroll") for (int a = 0; a < NACC; ++a) lacc[(size_t)a * E + g] = acc_init(as.kind[a]);
    }
    if (threadIdx.x == 0) { lused = 0; lemit = 0; if constexpr (L == P1_SLOT) lins = 0; }
    __syncthreads();
    const uint32_t base = ds.kmin + lo;                    // direct: key of entry 0
    uint32_t miss = 0;
    uint32_t i0 = b;
    for (uint32_t st = 0; st < nsteps; ++st) {
        const bool edge = st >= nfull;
        if (edge) load_edge(i0, e, cur);                   // (the last, partial step: nothing was prefetched for it)
        Batch nxt;
        { const uint32_t inext = i0 + STEP; load_full(inext <= safe_last && st + 1 < nfull ? inext : safe_last, nxt); }   // in flight while this step is aggregated
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t o = i0 + threadIdx.x * AR;
        // ---- where the rows accumulate: entry at[q] (slot: where the row's probe ends); a row to drop goes to a dummy entry
        uint32_t at[AR];
        K key[AR], w[AR];                                                  // (cur.key stays as it travelled, value fields included)
        uint32_t pend = 0;
        if constexpr (L == P1_DIRECT) {
#pragma unroll
            for (int q = 0; q < AR; ++q) {
                const uint32_t x = (cur.key[q] & ~in.kclear) - base;
                const bool live = !edge || o + q < e;
                miss |= live && x >= width ? 1u : 0u;
                at[q] = live && x < width ? x : ds.W;
            }
        } else {
#pragma unroll
            for (int q = 0; q < AR; ++q) {
                key[q] = cur.key[q];
                if constexpr (!K64) key[q] &= ~in.kclear;
                at[q] = __umulhi(key_hash<K64>(key[q]) * NB, cap); w[q] = ktab[at[q]];   // AR probes in flight
            }
#pragma unroll
            for (int q = 0; q < AR; ++q) {
                if (edge && !(o + q < e)) at[q] = cap + 1;                 // (masked)
                else if (key[q] == EMPTYK) at[q] = cap;                    // the key that doubles as the empty mark
                else if (w[q] != key[q]) pend |= 1u << q;
            }
            // rows that missed on their first probe walk their probe sequences together: one LDS round trip per step
            for (uint32_t step = 0; pend && step <= cap; ++step) {
#pragma unroll
                for (int q = 0; q < AR; ++q) {
                    if (!(pend & (1u << q))) continue;
                    K c = w[q];
                    if (c == EMPTYK) {
                        if constexpr (K64) c = atomicCAS(reinterpret_cast<unsigned long long*>(&ktab[at[q]]), (unsigned long long)EMPTYK, (unsigned long long)key[q]);
                        else c = atomicCAS(&ktab[at[q]], EMPTYK, key[q]);
                        if (c == EMPTYK) { c = key[q]; if (atomicAdd(&lins, 1u) >= limit) out.flags[0] = 1; }
                    }
                    if (c == key[q]) { pend &= ~(1u << q); continue; }
                    at[q] = at[q] + 1 == cap ? 0 : at[q] + 1;
                }
#pragma unroll
                for (int q = 0; q < AR; ++q) if (pend & (1u << q)) w[q] = ktab[at[q]];
            }
            if (pend) {                                                    // a full table: the host re-plans
                out.flags[0] = 1;
#pragma unroll
                for (int q = 0; q < AR; ++q) if (pend & (1u << q)) at[q] = cap + 1;
            }
        }
        // ---- first row, count, accumulators: fire-and-forget atomics on entry at[q]
#pragma unroll
        for (int q = 0; q < AR; ++q) atomicMin(&lfirst[at[q]], cur.row[q]);
        if (need_count) {
#pragma unroll
            for (int q = 0; q < AR; ++q) atomicAdd(&lcount[at[q]], 1u);
        }
        _Pragma("unroll") for (int a = 0; a < NACC; ++a) {
            uint64_t* acc = lacc + (size_t)a * E;
            // the operand: a packed field of the key word as it travelled (4-byte key words only), the value plane, or the row id
            VT x[AR];
            bool from_key = false;
            if constexpr (!K64) from_key = in.packed[a] != 0;
            if (from_key) { if constexpr (!K64) { _Pragma("unroll") for (int q = 0; q < AR; ++q) x[q] = (VT)((((uint32_t)cur.key[q] >> in.pshift[a]) & in.pmask[a]) + in.pmin[a]); } }
            else if (in.col[a]) { _Pragma("unroll") for (int q = 0; q < AR; ++q) x[q] = cur.v[a][q]; }
            else { _Pragma("unroll") for (int q = 0; q < AR; ++q) x[q] = (VT)cur.row[q]; }
#define AQG_ROWS(expr) _Pragma("unroll") for (int q = 0; q < AR; ++q) { expr; } break
            switch (ops.opc[a]) {
            case OPC_ADDI_I32: AQG_ROWS(atomicAdd(reinterpret_cast<unsigned long long*>(acc + at[q]), (unsigned long long)(long long)(int32_t)(uint32_t)x[q]));
            case OPC_ADDI_U32: AQG_ROWS(atomicAdd(reinterpret_cast<unsigned long long*>(acc + at[q]), (unsigned long long)(uint32_t)x[q]));
            case OPC_ADDF_F32: AQG_ROWS(atomicAdd(reinterpret_cast<double*>(acc + at[q]), (double)__uint_as_float((uint32_t)x[q])));
            case OPC_ADDF_F64: AQG_ROWS(atomicAdd(reinterpret_cast<double*>(acc + at[q]), __builtin_bit_cast(double, (uint64_t)x[q])));
            case OPC_MIN_I32: AQG_ROWS(atomicMin(reinterpret_cast<unsigned long long*>(acc + at[q]), (unsigned long long)map_i((int32_t)(uint32_t)x[q])));
            case OPC_MAX_I32: AQG_ROWS(atomicMax(reinterpret_cast<unsigned long long*>(acc + at[q]), (unsigned long long)map_i((int32_t)(uint32_t)x[q])));
            case OPC_MIN_U32: AQG_ROWS(atomicMin(reinterpret_cast<unsigned long long*>(acc + at[q]), (unsigned long long)(uint32_t)x[q]));
            case OPC_MAX_U32: AQG_ROWS(atomicMax(reinterpret_cast<unsigned long long*>(acc + at[q]), (unsigned long long)(uint32_t)x[q]));
            case OPC_MIN_F32: AQG_ROWS(atomicMin(reinterpret_cast<unsigned long long*>(acc + at[q]), (unsigned long long)map_f((double)__uint_as_float((uint32_t)x[q]))));
            case OPC_MAX_F32: AQG_ROWS(atomicMax(reinterpret_cast<unsigned long long*>(acc + at[q]), (unsigned long long)map_f((double)__uint_as_float((uint32_t)x[q]))));
            default: AQG_ROWS(acc_apply(acc + at[q], as.kind[a], val_operand_bits(as.dt[a] == AQG_NONE ? AQG_UINT32 : as.dt[a], (uint64_t)x[q], as.kind[a], as.square[a], as.part[a])));
            }
#undef AQG_ROWS
        }
        cur = nxt;
        i0 += STEP;
    }
    if constexpr (L == P1_DIRECT) { if (miss) *ds.miss = 1u; }
    __syncthreads();
    // ---- the entries that saw a row become records, reserved with one global atomic per partition: [0, cap] of a slot table,
    // [0, width) of a direct one
    {
        uint32_t mine = 0;
        for (uint32_t j = threadIdx.x; L == P1_DIRECT ? j < width : j <= cap; j += SB) mine += lfirst[j] != NOROW ? 1u : 0u;
        mine = wave_reduce(mine, OpAdd{});
        if (lane_id() == 0 && mine) atomicAdd(&lused, mine);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t used = lused;
        gbase = atomicAdd(&out.flags[1], used);
        if (part_base) { part_base[2 * (size_t)part] = gbase; part_base[2 * (size_t)part + 1] = used; }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; L == P1_DIRECT ? j < width : j <= cap; j += SB) {
        if (lfirst[j] == NOROW) continue;
        const uint32_t g = gbase + atomicAdd(&lemit, 1u);
        if (g >= out_cap) { out.flags[0] = 1; continue; }
        constexpr uint64_t EMPTYWORD = K64 ? EMPTY64 : (uint64_t)EMPTY32;
        uint64_t k;                                        // entry `cap` of a slot table: the key that equals the empty mark
        if constexpr (L == P1_SLOT) k = j == cap ? EMPTYWORD : (uint64_t)ktab[j];
        else k = (uint64_t)(base + j);
        *out.key_p(g) = k;
        *out.first_p(g) = lfirst[j];
        *out.count_p(g) = need_count ? lcount[j] : 0;
        _Pragma("unroll") for (int a = 0; a < NACC; ++a) *out.acc_p(a, g) = lacc[(size_t)a * E + j];
    }
    __syncthreads();
}
