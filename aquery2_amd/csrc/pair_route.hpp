// pair_route.hpp -- host-only route and workspace arithmetic of the pair windows (pair_window.hip: covw / corrw / betaw and the running
// covs / corrs / betas).  No HIP in here: pair_window.hip takes its decisions from this header, tests/pair_route_selftest.cpp drives it on
// the CPU under the sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace aqgpair {

constexpr uint32_t TILE_ROWS = 2048;          // rows per workgroup (scan_dev.hpp TS; pair_window.hip asserts the three)
constexpr uint32_t REG_MAX_W = 8;             // VAR_REG_W
constexpr uint32_t LDS_MAX_W = 64;            // VAR_DIRECT_MAX_W
constexpr uint32_t CHUNK = 2048;              // scan_dev.hpp CH: tile aggregates per chunk of the chunked aggregate scan
enum : uint32_t { ROUTE_REG = 1, ROUTE_LDS = 2, ROUTE_PREFIX = 4 };              // AQG_SCAN2_ROUTE_*
enum : int { OP_COVS = 0, OP_CORRS = 1, OP_BETAS = 2, OP_COVW = 3, OP_CORRW = 4, OP_BETAW = 5, OP_COUNT = 6 };   // aqg_scan2op

inline bool op_known(int op) { return op >= 0 && op < OP_COUNT; }
inline bool op_running(int op) { return op < OP_COVW; }
inline int op_family(int op) { return op % 3; }                                   // 0 cov, 1 corr, 2 beta
inline uint32_t family_sums(int fam) { return fam == 0 ? 3u : (fam == 1 ? 5u : 4u); }
// the window the kernels see: a window is clamped by the column (or the group) anyway, so one longer than n rows is one of n rows
inline uint32_t clamp_window(uint32_t w, uint32_t n) { return w > n ? n : w; }
// n >= 1; w >= 1 for the window ops
inline uint32_t route_of(int op, uint32_t n, uint32_t w) {
    if (op_running(op)) return ROUTE_PREFIX;
    const uint32_t ww = clamp_window(w, n);
    return ww <= REG_MAX_W ? ROUTE_REG : (ww <= LDS_MAX_W ? ROUTE_LDS : ROUTE_PREFIX);
}

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t tiles_of(uint32_t n) { return ((size_t)n + TILE_ROWS - 1) / TILE_ROWS; }
// what one call asks of the arena, every sub-allocation rounded as the bump allocator rounds it (0: the short routes take none):
//   the tile aggregates of the co-moment pass (carry_bytes each: the aggregate, per group with the carry of a segmented scan),
//   windows: the prefix (family_sums doubles a row); per group also the distance column with its own pass (dist_carry_bytes per
//   aggregate, scanned in chunks: tiles / CHUNK + 2 chunk totals)
inline size_t ws_bytes(int op, uint32_t n, uint32_t w, bool grouped, size_t carry_bytes, size_t dist_carry_bytes) {
    if (n == 0 || route_of(op, n, w) != ROUTE_PREFIX) return 0;
    const size_t nt = tiles_of(n);
    size_t need = round256(nt * carry_bytes);
    if (!op_running(op)) {
        need += round256((size_t)n * family_sums(op_family(op)) * sizeof(double));
        if (grouped) need += round256((size_t)n * 4) + round256(nt * dist_carry_bytes) + round256((nt / CHUNK + 2) * dist_carry_bytes);
    }
    return need;
}

} // namespace aqgpair
