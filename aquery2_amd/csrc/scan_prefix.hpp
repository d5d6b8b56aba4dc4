// scan_prefix.hpp -- the ordered prefix scans, written once for scan.hip (whole columns), segscan.hip (the flat row-list layout of a
// grouping) and ema.hip (affine recurrences in either layout): reduce-then-scan over 2048-row tiles,
//   K1 prefix_reduce_kernel  the fold of every tile
//   K2 launch_agg_scan       the exclusive scan of those folds (scan_dev.hpp)
//   K3 prefix_scan_kernel    every tile again from its carry-in, results through one writer (emit)
// A kernel takes its ROWS as a type: what a lane holds of its 8 positions, where the group starts among them are and how row j lifts
// into the algebra.  SEG = false instantiations hold no load, branch or LDS for group starts (the rule of scan_window.hpp's
// whole_column); what only one layout has -- the carry of a resumed column, the rounding of its first row -- rides in slice_of<SEG>,
// an argument of K3 alone.  prefix_pass() is the one host sequence.
// Everything sits in an unnamed namespace like the kernels of the .hip files (scan_dev.hpp says why).
#pragma once
#include "scan_dev.hpp"

namespace {
using namespace aqgscan;

struct none_alg {                              // position-only scans (group index / distance to the group start of every position)
    using A = uint32_t;
    __device__ static uint32_t identity() { return 0; }
    __device__ static uint32_t lift(uint8_t) { return 0; }
    __device__ static uint32_t op(uint32_t a, uint32_t) { return a; }
};
// the carry between lanes and tiles: the algebra's own value, or per group {value, last group start, groups so far}
template <class ALG, bool SEG> using carry_alg = std::conditional_t<SEG, seg_alg<ALG>, ALG>;

// ---- rows ------------------------------------------------------------------------------------------------------------------------
// the lane's block of IT positions and, per group, the start bits of the eight (SEG = false: no such member)
template <bool SEG> struct start_bits { uint32_t hb; };
template <> struct start_bits<false> {};
template <bool SEG> struct lane_block : start_bits<SEG> {
    uint32_t base, cnt;
    __device__ void place(uint32_t n) {
        base = blockIdx.x * TS + threadIdx.x * IT;
        cnt = base >= n ? 0 : (n - base < (uint32_t)IT ? n - base : IT);
    }
    __device__ void starts(const uint8_t* __restrict__ heads8) { if constexpr (SEG) this->hb = cnt ? heads8[base >> 3] : 0u; }
    __device__ bool head(int j) const { if constexpr (SEG) return (this->hb >> j) & 1u; else return false; }
    // the block's elements of one column.  Through a local array: loaded straight into a member, the eight stay one register tuple
    // for the whole kernel (the per-group variance of int32, W_RED_VAR: 90 VGPRs against 54)
    // (with the installed compiler: tools/isa_compare.py against the previous build says whether a later one still needs it)
    template <class E> __device__ void fetch(const E* __restrict__ col, uint32_t n, E (&dst)[IT]) const {
        E t[IT];
        uint32_t c;
        load_tile_items(col, n, base, t, c);
#pragma unroll
        for (int j = 0; j < IT; ++j) dst[j] = t[j];
    }
};
// one input column: row j lifts to ALG::lift(v[j])
template <class T, class ALG_, bool SEG_> struct value_rows : lane_block<SEG_> {
    using In = T;
    using ALG = ALG_;
    static constexpr bool SEG = SEG_;
    struct args { const T* x; const uint8_t* heads8; /* SEG */ };
    const T* x;
    T v[IT];
    __device__ void load(const args& a, uint32_t n) {
        this->place(n);
        x = a.x;
        this->fetch(a.x, n, v);
        this->starts(a.heads8);
    }
    __device__ typename ALG::A lift(int j) const { return ALG::lift(v[j]); }
    __device__ T first(uint32_t s) const { return x[s - 1]; }        // the row at the start of a slice (s = its position + 1)
};
// no input column: the start bits alone (distance to the group start, group index)
struct position_rows : lane_block<true> {
    using In = uint8_t;
    using ALG = none_alg;
    static constexpr bool SEG = true;
    struct args { const uint8_t* heads8; };
    __device__ void load(const args& a, uint32_t n) { place(n); starts(a.heads8); }
    __device__ uint32_t lift(int) const { return 0; }
};
// the lane's serial fold of its rows, in order, restarting at a start bit
template <class ROWS> __device__ inline typename carry_alg<typename ROWS::ALG, ROWS::SEG>::A fold_rows(const ROWS& r) {
    using ALG = typename ROWS::ALG;
    auto a = carry_alg<ALG, ROWS::SEG>::identity();
#pragma unroll
    for (int j = 0; j < IT; ++j) if ((uint32_t)j < r.cnt) {
        if constexpr (ROWS::SEG) {
            if (r.head(j)) { a.v = ALG::identity(); a.s = r.base + j + 1; ++a.c; }
            a.v = ALG::op(a.v, r.lift(j));
        } else a = ALG::op(a, r.lift(j));
    }
    return a;
}

// ---- the writer ------------------------------------------------------------------------------------------------------------------
// W_MAXP / W_MINP: running max / min without the reference's seed (maxw / minw, w >= n); W_RAW / W_MOM: the prefix in accumulator form
// (wide windows); W_CO3 / W_CO5 / W_CO4: the first 3 / 5 / 4 anchored co-moment sums of a pair of columns (wide pair windows: cov / corr /
// beta), W_COVS / W_CORRS / W_BETAS: the running pair statistics; W_RED_*: one result per group, stored where the group ends (the flat
// layout only)
enum : int { W_SUMS = 0, W_AVGS, W_MINS, W_MAXS, W_MAXP, W_MINP, W_VARS, W_STDDEVS, W_RAW, W_MOM, W_DIST, W_GID, W_EMA,
             W_CO3, W_CO5, W_CO4, W_COVS, W_CORRS, W_BETAS,
             W_RED_SUM, W_RED_AVG, W_RED_MIN, W_RED_MAX, W_RED_VAR, W_RED_STDDEV };
template <class T, int WR> struct prefix_out {
    using type = std::conditional_t<WR == W_SUMS || WR == W_RED_SUM, std::conditional_t<std::is_floating_point_v<T>, double, aqg_i128>,
                 std::conditional_t<WR == W_AVGS || WR == W_VARS || WR == W_STDDEVS || WR == W_EMA || WR == W_RED_AVG || WR == W_RED_VAR || WR == W_RED_STDDEV, double,
                 std::conditional_t<WR == W_RAW, typename sum_alg<T>::A, std::conditional_t<WR == W_MOM, dpair,
                 std::conditional_t<WR == W_CO3, dsums<3>, std::conditional_t<WR == W_CO4, dsums<4>, std::conditional_t<WR == W_CO5, dsums<5>,
                 std::conditional_t<WR == W_COVS || WR == W_CORRS || WR == W_BETAS, double,
                 std::conditional_t<WR == W_DIST || WR == W_GID, uint32_t, T>>>>>>>>>;
};
// a scan that resumes a column sharded by row range (aqg_scan_resume): the sum of every earlier row in the result's LongType
// and the number of earlier rows.  Kept apart from the tile accumulator, which is 64 bits wide for <= 4-byte integer columns
// while the carry of a table of more than 2^32 rows is not.
struct ScanSeed {
    aqg_i128 i = {0, 0};   // integer columns
    double d = -0.0;       // floating columns (-0.0 when there is nothing to add: the only value that leaves every double unchanged)
    uint64_t row0 = 0;     // rows before this shard (avgs divide by row0 + i + 1)
};
// Results leave through store_tile_striped, but for the per-group reductions and a whole column's W_RAW, which stores lane-blocked
// without dynamic LDS as it always did (raw_rows)
template <int WR, bool SEG> constexpr bool striped = WR < W_RED_SUM && !(WR == W_RAW && !SEG);
// avgs of 8-byte integers start from the slice's first row rounded to double (first_row_rounding)
template <class T, int WR> constexpr bool avg8 = WR == W_AVGS && sizeof(T) == 8 && std::is_integral_v<T>;

// the output element of one row: `run` = the fold of its slice up to and including it, `pos` = its position in the slice, `rows` =
// rows so far (the earlier shards' included), `gid` = slices before it; LEAD: sums start from `lead` (a resumed column, avg8)
template <class T, class ALG, int WR, bool LEAD>
__device__ inline typename prefix_out<T, WR>::type emit(const typename ALG::A& run, uint32_t pos, double rows, uint32_t gid, const ScanSeed& lead) {
    if constexpr (WR == W_SUMS || WR == W_RED_SUM) {
        if constexpr (std::is_floating_point_v<T>) { if constexpr (LEAD) return lead.d + run; else return run; }
        else if constexpr (LEAD) return i128_add(lead.i, sum_alg<T>::to_i128(run));
        else return sum_alg<T>::to_i128(run);
    } else if constexpr (WR == W_AVGS || WR == W_RED_AVG) {                        // (s += arr[i]) / (double)(i + 1)
        double sum;
        if constexpr (!LEAD) sum = sum_alg<T>::to_double(run);
        else if constexpr (std::is_floating_point_v<T>) sum = lead.d + run;
        else {
            const aqg_i128 t = i128_add(lead.i, sum_alg<T>::to_i128(run));
            if constexpr (std::is_unsigned_v<T>) sum = u128_to_double(t.hi, t.lo); else sum = i128_to_double(t);
        }
        return sum / rows;
    } else if constexpr (WR == W_MAXP || WR == W_MINP || WR == W_RAW) return run;
    else if constexpr (WR == W_MINS || WR == W_RED_MIN) { const T seed = dlimits<T>::max(); return seed < run ? seed : run; }    // min / mins seed with max(): +Inf rows come out as max()
    else if constexpr (WR == W_MAXS || WR == W_RED_MAX) { const T seed = dlimits<T>::min(); return seed > run ? seed : run; }    // max / maxs seed with numeric_limits<T>::min() (D8)
    else if constexpr (WR == W_VARS || WR == W_STDDEVS) {                         // anchored moments of the slice so far (mom_alg)
        const double var = var_from(run.s, run.q, (double)run.n);
        return WR == W_STDDEVS ? sqrt(var) : var;
    } else if constexpr (WR == W_RED_VAR || WR == W_RED_STDDEV) {                 // (ssq - s * s / (FPType)(len + 1)) / (FPType)(len + 1): D9 kept
        const double np1 = (double)(uint32_t)(pos + 2);
        double d;
        if constexpr (std::is_floating_point_v<T>) d = (run.q - run.s * run.s / np1) / np1;
        else {
            const __int128 ss = (__int128)run.s * (__int128)run.s;                   // the reference's 128-bit LongType product (|s| < 2^63: no wrap)
            // (uint16: the reference's sum of squares is an UNSIGNED 128-bit integer, and the int squares that wrapped negative are added
            // to it sign-extended -- a negative 64-bit sum stands for 2^128 minus its magnitude; the rule of groupby_tail.hip's sum128)
            double q;
            if constexpr (std::is_same_v<T, uint16_t>) q = u128_to_double((uint64_t)(run.q >> 63), (uint64_t)run.q); else q = (double)run.q;
            d = (q - i128_to_double(aqg_i128{(uint64_t)ss, (uint64_t)(ss >> 64)}) / np1) / np1;
        }
        return WR == W_RED_STDDEV ? sqrt(d) : d;
    } else if constexpr (WR == W_MOM) return dpair{run.s, run.q};
    else if constexpr (WR == W_CO3) return dsums<3>{{run.sx, run.sy, run.sxy}};
    else if constexpr (WR == W_CO4) return dsums<4>{{run.sx, run.sy, run.sxy, run.sxx}};
    else if constexpr (WR == W_CO5) return dsums<5>{{run.sx, run.sy, run.sxy, run.sxx, run.syy}};
    else if constexpr (WR == W_COVS || WR == W_CORRS || WR == W_BETAS) return pair_value<WR - W_COVS>(run.sx, run.sy, run.sxy, run.sxx, run.syy, (double)run.n);
    else if constexpr (WR == W_DIST) return pos;
    else if constexpr (WR == W_GID) return gid;
    else return ALG::value(run);                                                   // W_EMA: b, or num / den
}

// ---- what K3 knows of the slices ------------------------------------------------------------------------------------------------------
template <bool SEG> struct slice_of;
template <> struct slice_of<false> {           // a whole column is one slice, possibly the continuation of earlier shards
    ScanSeed seed;
    template <int WR, class ROWS> __device__ void begin(const ROWS& r) {
        // the column's own first row (a resumed shard's carry is the caller's)
        if constexpr (avg8<typename ROWS::In, WR>) { if (seed.row0 == 0) seed.i = i128_add(seed.i, first_row_rounding(r.first(1))); }
    }
    template <int WR, class ROWS> __device__ ScanSeed lead(const ROWS&, uint32_t, bool) const { return seed; }
    __device__ double rows(uint32_t p, uint32_t) const { return (double)(seed.row0 + p + 1); }
};
template <> struct slice_of<true> {            // the groups of a flat layout: s = position + 1 of the slice's start
    template <int WR, class ROWS> __device__ void begin(const ROWS&) {}
    template <int WR, class ROWS> __device__ ScanSeed lead(const ROWS& r, uint32_t s, bool live) const {
        ScanSeed l;
        if constexpr (avg8<typename ROWS::In, WR>) { if (live) l.i = first_row_rounding(r.first(s)); }
        return l;
    }
    __device__ double rows(uint32_t p, uint32_t s) const { return (double)(p - s + 2); }
};

// a whole column's W_RAW: the accumulator itself, stored lane-blocked, row J + 1 nested inside row J's `J < cnt` as the rolled loop of
// tile_scan_raw_kernel was (in the masked loop of the other writers the eight lifts are hoisted: 90 VGPRs for int64 against 78)
template <int J, class ROWS, class A> __device__ inline void raw_rows(const ROWS& r, A run, A* __restrict__ out) {
    if constexpr (J < IT) {
        if ((uint32_t)J < r.cnt) {
            run = ROWS::ALG::op(run, r.lift(J));
            out[r.base + J] = run;
            raw_rows<J + 1>(r, run, out);
        }
    }
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------------
// Both go through the ordered parts only -- the lane's serial loop (fold_rows), block_scan_excl, launch_agg_scan, seg_alg -- and never
// through block_fold or a chained look-back: the affine maps of ema_alg do not commute.
// K1: the fold of each tile (per group: of the rows behind its last group start, with the start)
template <class ROWS>
__global__ void __launch_bounds__(SB) prefix_reduce_kernel(typename ROWS::args ra, uint32_t n, typename carry_alg<typename ROWS::ALG, ROWS::SEG>::A* __restrict__ tile_agg) {
    using SA = carry_alg<typename ROWS::ALG, ROWS::SEG>;
    using C = typename SA::A;
    __shared__ C lds_w[8];
    ROWS r;
    r.load(ra, n);
    C total;
    block_scan_excl<SA>(fold_rows(r), lds_w, total);
    if (threadIdx.x == 0) tile_agg[blockIdx.x] = total;
}
// K3: the rows of a tile from its carry-in
template <class ROWS, int WR>
__global__ void __launch_bounds__(SB) prefix_scan_kernel(typename ROWS::args ra, uint32_t n, const typename carry_alg<typename ROWS::ALG, ROWS::SEG>::A* __restrict__ tile_prefix,
                                                         void* __restrict__ out, slice_of<ROWS::SEG> sl) {
    using T = typename ROWS::In;
    using ALG = typename ROWS::ALG;
    using SA = carry_alg<ALG, ROWS::SEG>;
    using C = typename SA::A;
    using O = typename prefix_out<T, WR>::type;
    constexpr bool SEG = ROWS::SEG, RED = WR >= W_RED_SUM;
    static_assert(!RED || SEG, "one result per group: the flat layout only");
    __shared__ C lds_w[8];
    extern __shared__ __align__(16) unsigned char stage_raw[];
    ROWS r;
    r.load(ra, n);
    uint32_t hnext = 0;                                                  // start bit of the position behind this lane's block
    if constexpr (RED) hnext = r.cnt ? (ra.heads8[(r.base >> 3) + 1] & 1u) : 0u;
    C total;
    const C pre = SA::op(tile_prefix[blockIdx.x], block_scan_excl<SA>(fold_rows(r), lds_w, total));
    typename ALG::A run;
    uint32_t s = 1, c = 1;                                               // a whole column: one slice from position 0
    if constexpr (SEG) { run = pre.v; s = pre.s; c = pre.c; } else run = pre;
    sl.template begin<WR>(r);
    if constexpr (!RED && !striped<WR, SEG>) { raw_rows<0>(r, run, static_cast<O*>(out)); return; }
    O o[IT];
#pragma unroll
    for (int j = 0; j < IT; ++j) {
        const bool live = (uint32_t)j < r.cnt;
        if (live) {
            if constexpr (SEG) { if (r.head(j)) { run = ALG::identity(); s = r.base + j + 1; ++c; } }
            run = ALG::op(run, r.lift(j));
        }
        const uint32_t p = r.base + j;
        o[j] = emit<T, ALG, WR, !SEG || avg8<T, WR>>(run, p - (s - 1), sl.rows(p, s), c - 1, sl.template lead<WR>(r, s, live));
        if constexpr (RED) {
            const uint32_t last = j + 1 < IT ? ((r.hb >> (j + 1)) & 1u) : hnext;   // the next position starts a group (bit n is set): p ends its group
            if (live && last) static_cast<O*>(out)[c - 1] = o[j];
        }
    }
    if constexpr (!RED) store_tile_striped(static_cast<O*>(out), blockIdx.x * TS, o, n, reinterpret_cast<O*>(stage_raw));
}

// ---- host: the one pass (workspace sized and reset by the caller) -----------------------------------------------------------------------
// carries -> their scan -> results.  CHUNKED = false keeps the aggregates' scan in one workgroup whatever their number: the callers
// whose floating results were pinned with that bracketing, or whose algebra has no other use for the chunk kernels
template <class ROWS, int WR, bool CHUNKED = true>
int prefix_pass(aqg_ctx* ctx, const typename ROWS::args& ra, uint32_t n, const slice_of<ROWS::SEG>& sl, void* out, const char* what, bool timed = true) {
    using SA = carry_alg<typename ROWS::ALG, ROWS::SEG>;
    using C = typename SA::A;
    using O = typename prefix_out<typename ROWS::In, WR>::type;
    const uint32_t ntiles = aqg_ceil_div(n, TS);
    C *carry, *chunk_tot;
    AQG_TRY(aqg_ws_get(ctx, ntiles, &carry));
    if constexpr (CHUNKED) AQG_TRY(aqg_ws_get(ctx, (size_t)ntiles / CH + 2, &chunk_tot));
    hipLaunchKernelGGL((prefix_reduce_kernel<ROWS>), dim3(ntiles), dim3(SB), 0, ctx->stream, ra, n, carry);
    if constexpr (CHUNKED) launch_agg_scan<SA>(ctx, carry, ntiles, chunk_tot);
    else hipLaunchKernelGGL((agg_scan_kernel<SA>), dim3(1), dim3(SB), 0, ctx->stream, carry, ntiles);
    constexpr size_t lds = striped<WR, ROWS::SEG> ? (size_t)TS * sizeof(O) : 0;
    if (timed) aqg_kernel_timer_begin(ctx);
    hipLaunchKernelGGL((prefix_scan_kernel<ROWS, WR>), dim3(ntiles), dim3(SB), lds, ctx->stream, ra, n, carry, out, sl);
    if (timed) aqg_kernel_timer_end(ctx);
    return what ? aqg_check_launch(ctx, what) : AQG_OK;                  // (null: the caller checks its own last launch, under its own message)
}

} // namespace
