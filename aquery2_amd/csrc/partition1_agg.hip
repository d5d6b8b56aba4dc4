// partition1_agg.hip -- the per-partition aggregation of the partition plans (partition1.hip): the kernels of the three LDS layouts -- the
// hashed table with dense ids (p1_agg_kernel), with the accumulators inside the table (p1_agg_slot_kernel), and the direct-indexed form
// over range partitions (p1_agg_direct_kernel) -- and ONE launcher (p1_launch) behind p1_launch_agg / p1_launch_agg_direct.  The slot and
// direct kernels include ONE row loop (partition1_agg_rows.inc), to which a layout contributes where a row accumulates and which entries
// become records; the dense-id kernel is written out.  All three share the loaders (partition1_agg_load.inc).
// Reference: AQHashTable's build (server/hasher.h:146-199) and the generated per-group loop (engine/ast.py:722-789), for the groups
// of ONE partition at a time.
#include "partition1_int.hpp"

namespace {

// ---- aggregate each partition in LDS ---------------------------------------------------------------------------------------------
struct AggIn {
    const void* col[MAXACC]; int esz[MAXACC];    // partitioned value arrays (4- or 8-byte elements); null: the row id, or a packed field
    int packed[MAXACC]; uint32_t pshift[MAXACC], pmask[MAXACC], pmin[MAXACC];   // the operand is a field of the key word: ((key >> pshift) & pmask) + pmin
    uint32_t kclear;                             // the packed fields' bits of the key word (0: none)
};
constexpr uint32_t ID_PENDING = 0xFFFFu, ID_OVER = 0xFFFEu;
struct DirectSpec { uint32_t M, kmin, D, W; uint32_t* miss; };

constexpr int AR = 4;      // consecutive rows per lane and step (one 16-byte load per 4-byte plane)

// The three layouts of a partition's groups in LDS.  E entries of first row / count / accumulators, and for the hashed two a key table:
//
// P1_DENSE_IDS  acc u64[NACC][gmax] | keytab K[cap] | first u32[gmax] | count u32[gmax] (need_count) | idtab u16[cap]
//   The accumulators are dense (a 2-byte id per slot, accumulators per id), so that the table's slack does not multiply them; the price
//   is the chain probe -> id -> first row -> atomics, three dependent LDS round trips per row, a spin on ids not yet published and a
//   counter every insertion passes through.  Dense id 0 is reserved for the group whose packed key equals the empty mark.
//
// P1_SLOT       acc u64[NACC][cap + 2] | keytab K[cap + 2] | first u32[cap + 2] | count u32[cap + 2] (need_count)
//   Where the groups of a partition still fit with the accumulators INSIDE the table (key | first row | count | accumulators per slot at
//   load 0.6: h2o Q5's three sums up to ~1e7 groups in 4096 partitions), a row needs ONE dependent round trip -- its probe -- and
//   everything behind it is a fire-and-forget atomic on the slot found.  Slot `cap` belongs to the key that equals the empty mark, slot
//   `cap + 1` takes the masked rows.
//
// P1_DIRECT     acc u64[NACC][W + 1] | first u32[W + 1] | count u32[W + 1] (need_count); entry W is the dummy.
//   When the key is one 4-byte integer column whose values fill their range (h2o id3 / id6: 1 .. 1e7), the two-level plan bins the rows
//   by RANGE -- bin = umulhi(key - kmin, M), order-preserving, so a partition owns a contiguous piece of the domain -- and the
//   aggregation is direct-indexed: acc[key - first key of the partition].  No probe, no compare-and-swap, no dense-id indirection: every
//   LDS operation of a row is a fire-and-forget atomic, nothing in the row loop waits for LDS (the dense-id layout: three dependent LDS
//   round trips per row, ~1000 instructions per 256 rows; h2o Q5 at 1e9 rows: 5.3 ms for 12 GB).  Rows beyond the end of a partial step
//   and keys outside the partition's piece (only possible when the sampled range missed a value: flagged, the call repeats hashed) go
//   to the dummy entry.
enum : int { P1_SLOT, P1_DIRECT };                 // the layouts of the shared body

// The dense-id kernel (layout P1_DENSE_IDS above) is written out: merged into the shared body, three of its instantiations -- seven and
// eight accumulators over a 4-byte key -- compiled with one more s_waitcnt vmcnt(0) than in this form (profiles/r9_p1_agg_merge.md).
// It shares the loaders.
// V8: some value plane has 8-byte elements (then every value travels through the loop as 64 bits)
template <int NACC, bool K64, bool V8>
__global__ void __launch_bounds__(SB) p1_agg_kernel(const void* __restrict__ rkeys, const uint32_t* __restrict__ rrows, AccSpec as, AggIn in, AggOps ops,
                                                    const uint32_t* __restrict__ pstart, uint32_t pstride, uint32_t NB, uint32_t ntotal, uint32_t cap, uint32_t gmax, int need_count,
                                                    GTable out, uint32_t out_cap, uint32_t* __restrict__ part_base /* null, or [2 NB]: {first record, records} of every partition */) {
    using K = key_t_<K64>;
    using VT = std::conditional_t<V8, uint64_t, uint32_t>;
    constexpr int NA = NACC ? NACC : 1;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    uint64_t* lacc = reinterpret_cast<uint64_t*>(smem_raw);                       // [NACC][gmax]
    K* ktab = reinterpret_cast<K*>(lacc + (size_t)NACC * gmax);                   // [cap]
    uint32_t* lfirst = reinterpret_cast<uint32_t*>(ktab + cap);                   // [gmax]
    uint32_t* lcount = lfirst + gmax;                                             // [gmax] (only when need_count)
    uint16_t* idtab = reinterpret_cast<uint16_t*>(lcount + (need_count ? gmax : 0));   // [cap]
    __shared__ uint32_t lused, lemit, gbase;
    const K EMPTYK = empty_key<K64>();
#include "partition1_agg_load.inc"
    for (uint32_t part = blockIdx.x; part < NB; part += gridDim.x) {
        const uint32_t b = pstart[(size_t)part * pstride];
        const uint32_t e = part + 1 < NB ? pstart[(size_t)(part + 1) * pstride] : ntotal;
        if (b == e) continue;
        constexpr uint32_t STEP = SB * AR;
        const uint32_t nfull = (e - b) / STEP, nsteps = nfull + ((e - b) % STEP ? 1u : 0u);
        // where a prefetch may always read a whole step: the last full step of this partition, or (a partition shorter than a step)
        // any step inside the planes -- what it fetches then is never used
        const uint32_t safe_last = nfull ? b + (nfull - 1) * STEP : (b + STEP <= ntotal ? b : ntotal - STEP);
        Batch cur;
        load_full(nfull ? b : safe_last, cur);                 // in flight while the tables are cleared
        for (uint32_t s = threadIdx.x; s < cap; s += SB) { ktab[s] = EMPTYK; idtab[s] = (uint16_t)ID_PENDING; }
        for (uint32_t g = threadIdx.x; g < gmax; g += SB) {
            lfirst[g] = NOROW;
            if (need_count) lcount[g] = 0;
            _Pragma("unroll") for (int a = 0; a < NACC; ++a) lacc[(size_t)a * gmax + g] = acc_init(as.kind[a]);
        }
        if (threadIdx.x == 0) { lused = 1; lemit = 0; }
        __syncthreads();
        uint32_t i0 = b;
        for (uint32_t st = 0; st < nsteps; ++st) {
            if (st >= nfull) load_edge(i0, e, cur);            // (the last, partial step: nothing was prefetched for it)
            Batch nxt;
            { const uint32_t inext = i0 + STEP; load_full(inext <= safe_last && st + 1 < nfull ? inext : safe_last, nxt); }   // in flight while this step is aggregated
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t o = i0 + threadIdx.x * AR;
            uint32_t slot[AR];
            K w[AR];
            K raw[AR];                                                    // the key word as it travelled (value fields included)
            if constexpr (!K64) {
#pragma unroll
                for (int q = 0; q < AR; ++q) { raw[q] = cur.key[q]; cur.key[q] &= ~in.kclear; }
            }
#pragma unroll
            for (int q = 0; q < AR; ++q) { slot[q] = __umulhi(key_hash<K64>(cur.key[q]) * NB, cap); w[q] = ktab[slot[q]]; }   // AR probes in flight
            uint32_t pend = 0, special = 0;
#pragma unroll
            for (int q = 0; q < AR; ++q) {
                if (!(o + q < e)) slot[q] = FAIL;
                else if (cur.key[q] == EMPTYK) special |= 1u << q;
                else if (w[q] != cur.key[q]) pend |= 1u << q;
            }
            // rows that missed on their first probe walk their probe sequences together: one LDS round trip per step
            for (uint32_t step = 0; pend && step <= cap; ++step) {
#pragma unroll
                for (int q = 0; q < AR; ++q) {
                    if (!(pend & (1u << q))) continue;
                    K c = w[q];
                    if (c == EMPTYK) {
                        if constexpr (K64) c = atomicCAS(reinterpret_cast<unsigned long long*>(&ktab[slot[q]]), (unsigned long long)EMPTYK, (unsigned long long)cur.key[q]);
                        else c = atomicCAS(&ktab[slot[q]], EMPTYK, cur.key[q]);
                        if (c == EMPTYK) {
                            const uint32_t id = atomicAdd(&lused, 1u);
                            idtab[slot[q]] = (uint16_t)(id < gmax ? id : ID_OVER);
                            c = cur.key[q];
                        }
                    }
                    if (c == cur.key[q]) { pend &= ~(1u << q); continue; }
                    slot[q] = slot[q] + 1 == cap ? 0 : slot[q] + 1;
                }
#pragma unroll
                for (int q = 0; q < AR; ++q) if (pend & (1u << q)) w[q] = ktab[slot[q]];
            }
            uint32_t id[AR];
            bool ok[AR];
#pragma unroll
            for (int q = 0; q < AR; ++q) {
                if (special & (1u << q)) { id[q] = 0; ok[q] = true; continue; }
                if (slot[q] == FAIL || (pend & (1u << q))) { id[q] = 0; ok[q] = false; if (slot[q] != FAIL) out.flags[0] = 1; continue; }
                const volatile uint16_t* ip = idtab + slot[q];
                uint32_t v = *ip;
                while (v == ID_PENDING) { __builtin_amdgcn_s_sleep(1); v = *ip; }   // the inserting lane (of another wavefront) is about to publish it
                ok[q] = v != ID_OVER;
                id[q] = ok[q] ? v : 0;
                if (!ok[q]) out.flags[0] = 1;                                      // more groups than the dense arrays hold: the host re-plans
            }
#pragma unroll
            for (int q = 0; q < AR; ++q) if (ok[q] && cur.row[q] < lfirst[id[q]]) atomicMin(&lfirst[id[q]], cur.row[q]);
            if (need_count) {
#pragma unroll
                for (int q = 0; q < AR; ++q) if (ok[q]) atomicAdd(&lcount[id[q]], 1u);
            }
            _Pragma("unroll") for (int a = 0; a < NACC; ++a) {
                uint64_t* acc = lacc + (size_t)a * gmax;
#define AQG_ROWS(expr) _Pragma("unroll") for (int q = 0; q < AR; ++q) if (ok[q]) { VT x = in.col[a] ? cur.v[a][q] : (VT)cur.row[q]; \
                if constexpr (!K64) { if (in.packed[a]) x = (VT)((((uint32_t)raw[q] >> in.pshift[a]) & in.pmask[a]) + in.pmin[a]); } (void)x; expr; } break
                switch (ops.opc[a]) {
                case OPC_ADDI_I32: AQG_ROWS(atomicAdd(reinterpret_cast<unsigned long long*>(acc + id[q]), (unsigned long long)(long long)(int32_t)(uint32_t)x));
                case OPC_ADDI_U32: AQG_ROWS(atomicAdd(reinterpret_cast<unsigned long long*>(acc + id[q]), (unsigned long long)(uint32_t)x));
                case OPC_ADDF_F32: AQG_ROWS(atomicAdd(reinterpret_cast<double*>(acc + id[q]), (double)__uint_as_float((uint32_t)x)));
                case OPC_ADDF_F64: AQG_ROWS(atomicAdd(reinterpret_cast<double*>(acc + id[q]), __builtin_bit_cast(double, (uint64_t)x)));
                case OPC_MIN_I32: AQG_ROWS(atomicMin(reinterpret_cast<unsigned long long*>(acc + id[q]), (unsigned long long)map_i((int32_t)(uint32_t)x)));
                case OPC_MAX_I32: AQG_ROWS(atomicMax(reinterpret_cast<unsigned long long*>(acc + id[q]), (unsigned long long)map_i((int32_t)(uint32_t)x)));
                case OPC_MIN_U32: AQG_ROWS(atomicMin(reinterpret_cast<unsigned long long*>(acc + id[q]), (unsigned long long)(uint32_t)x));
                case OPC_MAX_U32: AQG_ROWS(atomicMax(reinterpret_cast<unsigned long long*>(acc + id[q]), (unsigned long long)(uint32_t)x));
                case OPC_MIN_F32: AQG_ROWS(atomicMin(reinterpret_cast<unsigned long long*>(acc + id[q]), (unsigned long long)map_f((double)__uint_as_float((uint32_t)x))));
                case OPC_MAX_F32: AQG_ROWS(atomicMax(reinterpret_cast<unsigned long long*>(acc + id[q]), (unsigned long long)map_f((double)__uint_as_float((uint32_t)x))));
                default: AQG_ROWS(acc_apply(acc + id[q], as.kind[a], val_operand_bits(as.dt[a] == AQG_NONE ? AQG_UINT32 : as.dt[a], (uint64_t)x, as.kind[a], as.square[a], as.part[a])));
                }
#undef AQG_ROWS
            }
            cur = nxt;
            i0 += STEP;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t used = (lused < gmax ? lused : gmax) - 1 + (lfirst[0] != NOROW ? 1u : 0u);
            gbase = atomicAdd(&out.flags[1], used);
            if (part_base) { part_base[2 * (size_t)part] = gbase; part_base[2 * (size_t)part + 1] = used; }
        }
        __syncthreads();
        for (uint32_t s = threadIdx.x; s <= cap; s += SB) {
            uint32_t id; uint64_t k;
            if (s == cap) { if (lfirst[0] == NOROW) continue; id = 0; k = K64 ? EMPTY64 : (uint64_t)EMPTY32; }
            else { if (ktab[s] == EMPTYK) continue; id = idtab[s]; k = (uint64_t)ktab[s]; if (id >= gmax) continue; }
            const uint32_t g = gbase + atomicAdd(&lemit, 1u);
            if (g >= out_cap) { out.flags[0] = 1; continue; }
            *out.key_p(g) = k;
            *out.first_p(g) = lfirst[id];
            *out.count_p(g) = need_count ? lcount[id] : 0;
            _Pragma("unroll") for (int a = 0; a < NACC; ++a) *out.acc_p(a, g) = lacc[(size_t)a * gmax + id];
        }
        __syncthreads();
    }
}

// The slot and direct kernels: one body (partition1_agg_rows.inc), a workgroup per partition at a time.
template <int NACC, bool K64, bool V8>
__global__ void __launch_bounds__(SB) p1_agg_slot_kernel(const void* __restrict__ rkeys, const uint32_t* __restrict__ rrows, AccSpec as, AggIn in, AggOps ops,
                                                         const uint32_t* __restrict__ pstart, uint32_t pstride, uint32_t NB, uint32_t ntotal, uint32_t cap, int need_count,
                                                         GTable out, uint32_t out_cap, uint32_t* __restrict__ part_base) {
    constexpr int L = P1_SLOT;
    const DirectSpec ds{};
#include "partition1_agg_rows.inc"
}
template <int NACC, bool V8>
__global__ void __launch_bounds__(SB) p1_agg_direct_kernel(const uint32_t* __restrict__ rkeys, const uint32_t* __restrict__ rrows, AccSpec as, AggIn in, AggOps ops,
                                                           const uint32_t* __restrict__ pstart, uint32_t pstride, uint32_t NB, uint32_t ntotal, DirectSpec ds, int need_count,
                                                           GTable out, uint32_t out_cap) {
    constexpr int L = P1_DIRECT;
    constexpr bool K64 = false;
    constexpr uint32_t cap = 0;
    uint32_t* const part_base = nullptr;
#include "partition1_agg_rows.inc"
}

} // namespace

// LDS of one partition.  Every layout has, per entry of its per-group arrays, first row | count | accumulators; the dense-id layout
// adds a key and a 2-byte id per table slot, the slot layout a key per entry.  The capacities below and the launchers both size the
// arrays from these (the 16: the kernels' own counters).
static size_t p1_entry_bytes(const AccSpec& as, int need_count) { return 4 + (need_count ? 4 : 0) + 8 * (size_t)as.nacc; }
static size_t p1_table_slot_bytes(int ksz) { return (size_t)ksz + 2; }
static size_t p1_slot_bytes(int ksz, const AccSpec& as, int need_count) { return (size_t)ksz + p1_entry_bytes(as, need_count); }
static size_t p1_dense_lds(int ksz, const AccSpec& as, int need_count, uint32_t gmax, uint32_t cap) { return gmax * p1_entry_bytes(as, need_count) + cap * p1_table_slot_bytes(ksz) + 16; }
static size_t p1_slot_lds(int ksz, const AccSpec& as, int need_count, uint32_t cap) { return ((size_t)cap + 2) * p1_slot_bytes(ksz, as, need_count) + 16; }
static size_t p1_direct_lds(const AccSpec& as, int need_count, uint32_t W) { return ((size_t)W + 1) * p1_entry_bytes(as, need_count) + 16; }

// groups one partition's LDS holds, and its key-table capacity, for (ksz, as, need_count)
static void p1_capacity(int ksz, const AccSpec& as, int need_count, uint32_t* gmax, uint32_t* cap) {
    const double dense = (double)p1_entry_bytes(as, need_count);
    const double slot = (double)p1_table_slot_bytes(ksz) * 1000.0 / LF1000;
    uint32_t g = (uint32_t)((double)(AGG_LDS - 64) / (dense + slot));
    if (g > 65000) g = 65000;                 // dense ids are 16 bits
    g &= ~3u;
    *gmax = g;
    *cap = ((uint32_t)((uint64_t)g * 1000 / LF1000) + 7) & ~7u;
}

// the slot-indexed layout (p1_agg_slot_kernel): slots one partition's LDS holds, and the groups it is planned for (load 0.6)
static void p1_slot_capacity(int ksz, const AccSpec& as, int need_count, uint32_t* cap, uint32_t* groups) {
    size_t c = (AGG_LDS - 64) / p1_slot_bytes(ksz, as, need_count);
    if (c > 32768) c = 32768;
    *cap = (uint32_t)(c > 16 ? c - 2 : 0) & ~7u;
    *groups = (uint32_t)((uint64_t)*cap * 600 / 1000);
}
uint32_t p1_direct_capacity(const AccSpec& as, int need_count) {
    size_t w = (AGG_LDS - 64) / p1_entry_bytes(as, need_count);
    if (w > 32768) w = 32768;
    return (uint32_t)w - 1;                        // (one entry is the dummy)
}
// number of partitions for `hint` expected groups: mean + 5 sigma of a partition's group count must fit gmax (0: no plan).
// *layout (optional): AQG_P1_LAYOUT_SLOT when the accumulators can sit inside the key table within the two-level plan's partition limit
// (one dependent LDS round trip per row instead of three), else AQG_P1_LAYOUT_DENSE_IDS (fewer, fuller partitions)
uint32_t aqg_partition_parts(int ksz, const AccSpec& as, int need_count, uint32_t hint, int* layout) {
    if (layout) {
        *layout = AQG_P1_LAYOUT_DENSE_IDS;
        uint32_t scap, sgroups;
        p1_slot_capacity(ksz, as, need_count, &scap, &sgroups);
        if (!aqg_switches().p1_bins && sgroups >= 256) {
            double mu = (double)sgroups;
            for (int it = 0; it < 8; ++it) mu = (double)sgroups - 5.0 * sqrt(mu);
            uint64_t bins = (uint64_t)((double)hint / mu) + 1;
            if (bins < 256) bins = 256;
            if (bins <= AQG_P2_MAXPARTS - 64) { *layout = AQG_P1_LAYOUT_SLOT; return (uint32_t)bins; }
        }
    }
    uint32_t gmax, cap;
    p1_capacity(ksz, as, need_count, &gmax, &cap);
    // mu + 5 sqrt(mu) <= gmax - 1
    double mu = (double)gmax - 1.0;
    for (int it = 0; it < 8; ++it) mu = (double)gmax - 1.0 - 5.0 * sqrt(mu);
    if (mu < 16) return 0;
    uint64_t bins = (uint64_t)((double)hint / mu) + 1;
    if (bins < 256) bins = 256;               // every CU gets a partition
    if (aqg_switches().p1_bins > 0) bins = (uint64_t)aqg_switches().p1_bins;   // measurements only
    return bins <= (1u << 20) ? (uint32_t)bins : 0;
}

// what the kernels need to know about the accumulators' operands: where each one's values lie, and its opcode
static void p1_agg_args(const AccSpec& as, const ValCols& vc, void* const* pvals, const PackPlan* pp, AggIn* inp, AggOps* opsp, bool* v8p) {
    AggIn& in = *inp;
    memset(&in, 0, sizeof in);
    if (pp) in.kclear = pp->kclear;
    AggOps& ops = *opsp;
    memset(&ops, 0, sizeof ops);
    bool v8 = false;
    for (int a = 0; a < as.nacc; ++a) {
        const int f = pp && as.dt[a] != AQG_NONE ? pack_field_of(*pp, as.col[a]) : -1;
        if (f >= 0) { in.col[a] = nullptr; in.esz[a] = 4; in.packed[a] = 1; in.pshift[a] = pp->shift[f]; in.pmask[a] = pp->fmask[f]; in.pmin[a] = pp->min[f]; }
        else if (vc.of_acc[a] >= 0) { in.col[a] = pvals[vc.of_acc[a]]; in.esz[a] = (int)part_val_bytes(vc.dt[vc.of_acc[a]]); }
        else { in.col[a] = nullptr; in.esz[a] = 4; }     // row-index operands: the carried row id
        ops.opc[a] = p1_opcode(as.dt[a], as.kind[a], as.square[a], as.part[a]);
        v8 = v8 || in.esz[a] == 8;
    }
    *v8p = v8;
}

// the build: where the partitioned rows lie, and (*part_base, zeroed here, written by the kernel) which records every partition wrote
static int p1_part_rows(aqg_ctx* ctx, PartRows* pr, int ksz, const void* pkeys, const void* prows, const uint32_t* pstart, uint32_t pstride, uint32_t nparts, uint32_t n, uint32_t cap, uint32_t** part_base) {
    *part_base = nullptr;
    if (!pr) return 0;
    AQG_TRY(aqg_ws_get(ctx, 2 * (size_t)nparts + 2, part_base));
    AQG_HIP(ctx, hipMemsetAsync(*part_base, 0, (2 * (size_t)nparts + 2) * 4, ctx->stream));
    pr->keys = pkeys; pr->rows = static_cast<const uint32_t*>(prows); pr->pstart = pstart; pr->pstride = pstride; pr->nparts = nparts; pr->ntotal = n;
    pr->ksz = ksz; pr->part_base = *part_base; pr->cap = cap; pr->valid = true;
    return 0;
}

// Launch the instantiation of one of the three kernels for (nacc, ksz, v8), a workgroup per partition up to one per CU.
// kernel_of(N, K64, V8) returns the instantiation for these three integral constants.
template <class KernelOf, class... Args>
static int p1_launch(aqg_ctx* ctx, const char* name, KernelOf kernel_of, int nacc, int ksz, bool v8, size_t lds, uint32_t nparts, Args... args) {
    const unsigned grid = nparts < (unsigned)ctx->num_cu ? nparts : (unsigned)ctx->num_cu;
    auto launch = [&](auto kern) -> int {
        AQG_TRY(aqg_allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
        aqg_kernel_timer_begin(ctx);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(SB), lds, ctx->stream, args...);
        aqg_kernel_timer_end(ctx);
        return aqg_check_launch(ctx, name);
    };
    auto pick = [&](auto nacc_c) -> int {
        if (ksz == 4) return v8 ? launch(kernel_of(nacc_c, std::false_type{}, std::true_type{})) : launch(kernel_of(nacc_c, std::false_type{}, std::false_type{}));
        return v8 ? launch(kernel_of(nacc_c, std::true_type{}, std::true_type{})) : launch(kernel_of(nacc_c, std::true_type{}, std::false_type{}));
    };
#define AQG_P1_CASE(N) case N: return pick(std::integral_constant<int, N>{});
    switch (nacc) {
    AQG_P1_CASE(0) AQG_P1_CASE(1) AQG_P1_CASE(2) AQG_P1_CASE(3) AQG_P1_CASE(4) AQG_P1_CASE(5) AQG_P1_CASE(6) AQG_P1_CASE(7)
    default: return pick(std::integral_constant<int, 8>{});
    }
#undef AQG_P1_CASE
}

int p1_launch_agg_direct(aqg_ctx* ctx, const AccSpec& as, const ValCols& vc, const void* pkeys, const void* prows, void* const* pvals,
                                const uint32_t* pstart, uint32_t pstride, uint32_t n, int need_count, GTable out, uint32_t out_cap, const PackPlan* pp, const RangePlan& rp) {
    AggIn in; AggOps ops; bool v8;
    p1_agg_args(as, vc, pvals, pp, &in, &ops, &v8);
    DirectSpec ds{rp.M, rp.kmin, rp.D, rp.W, out.flags + 6};
    return p1_launch(ctx, "p1_agg_direct_kernel", [](auto N, auto, auto V8) { return &p1_agg_direct_kernel<N(), V8()>; }, as.nacc, 4, v8, p1_direct_lds(as, need_count, rp.W), rp.P,
                     static_cast<const uint32_t*>(pkeys), static_cast<const uint32_t*>(prows), as, in, ops, pstart, pstride, rp.P, n, ds, need_count, out, out_cap);
}

// aggregate the partitions [pstart[p * pstride], pstart[(p + 1) * pstride]) (the last one ends at n) of the partitioned planes
int p1_launch_agg(aqg_ctx* ctx, int ksz, const AccSpec& as, const ValCols& vc, const void* pkeys, const void* prows, void* const* pvals,
                  const uint32_t* pstart, uint32_t pstride, uint32_t nparts, uint32_t n, int need_count, GTable out, uint32_t out_cap, PartRows* pr,
                  const PackPlan* pp, int layout) {
    AggIn in; AggOps ops; bool v8;
    p1_agg_args(as, vc, pvals, pp, &in, &ops, &v8);
    uint32_t* part_base;
    if (layout == AQG_P1_LAYOUT_SLOT) {
        uint32_t scap, sgroups;
        p1_slot_capacity(ksz, as, need_count, &scap, &sgroups);
        AQG_TRY(p1_part_rows(ctx, pr, ksz, pkeys, prows, pstart, pstride, nparts, n, scap, &part_base));
        return p1_launch(ctx, "p1_agg_slot_kernel", [](auto N, auto K64, auto V8) { return &p1_agg_slot_kernel<N(), K64(), V8()>; }, as.nacc, ksz, v8, p1_slot_lds(ksz, as, need_count, scap), nparts,
                         pkeys, static_cast<const uint32_t*>(prows), as, in, ops, pstart, pstride, nparts, n, scap, need_count, out, out_cap, part_base);
    }
    uint32_t gmax, cap;
    p1_capacity(ksz, as, need_count, &gmax, &cap);
    AQG_TRY(p1_part_rows(ctx, pr, ksz, pkeys, prows, pstart, pstride, nparts, n, cap, &part_base));
    return p1_launch(ctx, "p1_agg_kernel", [](auto N, auto K64, auto V8) { return &p1_agg_kernel<N(), K64(), V8()>; }, as.nacc, ksz, v8, p1_dense_lds(ksz, as, need_count, gmax, cap), nparts,
                     pkeys, static_cast<const uint32_t*>(prows), as, in, ops, pstart, pstride, nparts, n, cap, gmax, need_count, out, out_cap, part_base);
}
