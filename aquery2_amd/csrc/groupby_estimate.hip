// groupby_estimate.hip -- the group-count estimate of a call without a hint (run_with_retry, groupby.hip).
#include "groupby_plan.hpp"

// No hint and a large input: count the distinct tuples of the first 2^20 rows (a group-by without aggregates over a sample: well
// under a millisecond) and size the plan from that, instead of discovering the cardinality by running -- and overflowing --
// one plan after the other over all the rows (1e9 rows, 1e7 groups, hint 0: ~600 ms of escalations before).
// Uniformly spread keys: d = G (1 - exp(-s / G)) distinct tuples among s sampled rows; solved for G.  An estimate that is too
// small only costs the usual re-plan; one that is too large picks a plan for more groups than there are (still exact).
// The sample: 1024 blocks of 1024 consecutive rows spread evenly over the table, gathered into columns of their own.  Two counts come out of it:
// d = the distinct tuples of the whole sample (a group-by without aggregates), and D2 = the sum over the blocks of the distinct tuples INSIDE each
// block (sample_block_distinct_kernel).  Keys spread at random: d = G (1 - exp(-s / G)), solved for G, as before.  Keys CLUSTERED -- a table sorted
// by its key, or arriving key by key -- show themselves by blocks that share no tuples (d ~ D2) although rows repeat inside the blocks (D2 < s):
// every run of equal keys is then seen about once per n / s rows, G ~ d n / s.  (With the first 2^20 rows as the sample, 1e9 rows sorted by a key
// of 1e7 values were estimated at 13,000 groups; the escalation behind that ended in the HBM table: 7.9 s for a 21 ms call.)
// Both counts from ONE kernel over the rows where they lie (block b = sample block b, 1024 consecutive rows from row (b * total) >> 10): the
// tuples go into an open-addressing table in HBM (2^21 8-byte slots for 2^20 rows; wide tuples by their 32-bit hash: an estimate) and into one of
// 2048 slots in LDS; the first of every tuple is counted.  One launch, one host round trip: ~50 us.  (Before: the sample gathered into columns of its
// own, a quadratic per-block distinct count -- 69 us -- and a count-only group-by through the one-level partition plan: ~0.3 ms with its three host
// round trips, a fifth of h2o Q1's first call at 1e9 rows.)
namespace {
constexpr uint32_t SAMPLE_ROWS = 1u << 20, SAMPLE_SLOTS = 1u << 21;
__device__ inline uint32_t sample_mix(uint64_t k) { k ^= k >> 33; k *= 0xFF51AFD7ED558CCDull; k ^= k >> 33; k *= 0xC4CEB9FE1A85EC53ull; return (uint32_t)(k >> 32); }
__global__ void __launch_bounds__(1024) sample_distinct_kernel(KeySpec ks, uint32_t total, unsigned long long* __restrict__ table /* [SAMPLE_SLOTS], all ones */,
                                                               uint32_t* __restrict__ out /* [0] distinct in the sample, [1] sum of the blocks' distinct counts, [2] the all-ones tuple seen */) {
    constexpr unsigned long long NONE = ~0ull;
    __shared__ unsigned long long lkey[2048];
    __shared__ uint32_t cnt[2];
    lkey[threadIdx.x] = NONE; lkey[threadIdx.x + 1024] = NONE;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t row = (size_t)(((uint64_t)blockIdx.x * total) >> 10) + threadIdx.x;
    const unsigned long long k = ks.wide ? (unsigned long long)hash_wide(ks, row) : (unsigned long long)pack_key(ks, row);
    bool first_here = false, first_all = false;
    if (k == NONE) atomicOr(&out[2], 1u);                       // (the empty mark itself: counted once by the host)
    else {
        const uint32_t h = sample_mix(k);
        for (uint32_t s = h & 2047u, p = 0; p < 2048; ++p, s = (s + 1) & 2047u) {
            const unsigned long long old = atomicCAS(&lkey[s], NONE, k);
            if (old == NONE) { first_here = true; break; }
            if (old == k) break;
        }
        if (first_here) {                                       // (only a block's first row of a tuple goes to the shared table)
            for (uint32_t s = (h >> 11) & (SAMPLE_SLOTS - 1), p = 0; p < SAMPLE_SLOTS; ++p, s = (s + 1) & (SAMPLE_SLOTS - 1)) {
                const unsigned long long old = atomicCAS(&table[s], NONE, k);
                if (old == NONE) { first_all = true; break; }
                if (old == k) break;
            }
        }
    }
    const uint64_t mh = __ballot(first_here), ma = __ballot(first_all);
    if (lane_id() == 0) { atomicAdd(&cnt[0], (uint32_t)__popcll(ma)); atomicAdd(&cnt[1], (uint32_t)__popcll(mh)); }
    __syncthreads();
    if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&out[threadIdx.x], cnt[threadIdx.x]);
}
} // namespace

uint64_t aqg_estimate_groups(aqg_ctx* ctx, const KeySpec& ks, uint32_t n) {
    const uint32_t s = SAMPLE_ROWS;
    const size_t need = (size_t)SAMPLE_SLOTS * 8 + 64;
    size_t cap = 0;
    void* buf = aqg_pool_alloc(ctx, need, &cap);
    if (!buf) return 0;
    unsigned long long* table = static_cast<unsigned long long*>(buf);
    uint32_t* dout = reinterpret_cast<uint32_t*>(static_cast<char*>(buf) + (size_t)SAMPLE_SLOTS * 8);
    uint32_t got[4] = {0, 0, 0, 0};
    bool ok = hipMemsetAsync(table, 0xFF, (size_t)SAMPLE_SLOTS * 8, ctx->stream) == hipSuccess && hipMemsetAsync(dout, 0, 16, ctx->stream) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(sample_distinct_kernel, dim3(1024), dim3(1024), 0, ctx->stream, ks, n, table, dout);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(got, dout, 16, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    }
    uint64_t est = 0;
    if (ok) {
        const double d = (double)got[0] + (got[2] ? 1.0 : 0.0), sd = (double)s, D2 = (double)got[1] + (got[2] ? 1.0 : 0.0);
        if (d <= 0.5 * sd) est = (uint64_t)(d * 1.25) + 64;                 // the sample has seen (nearly) every group
        else if (d >= 0.999 * sd) est = n;                                  // (nearly) all distinct
        else {
            double lo = d, hi = 1e12;                                       // d / G = 1 - exp(-s / G), monotone in G
            for (int it = 0; it < 60; ++it) { double g = 0.5 * (lo + hi); if (g * (1.0 - exp(-sd / g)) < d) lo = g; else hi = g; }
            est = (uint64_t)(hi * 1.25) + 64;
        }
        if (D2 > 0 && d >= 0.8 * D2 && D2 <= 0.9 * sd) {                    // clustered keys: blocks share (nearly) no tuples, rows repeat inside them
            const uint64_t clustered = (uint64_t)(d * ((double)n / sd) * 1.1) + 64;
            if (clustered > est) est = clustered;
        }
        if (est > n) est = n;
    }
    aqg_pool_give(ctx, buf, cap);
    return est;
}
