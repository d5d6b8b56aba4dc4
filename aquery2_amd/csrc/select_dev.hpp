// select_dev.hpp -- what the radix selections (select.hip, topk.hip, quantile.hip and window_quantile.hip, through select_radix.hpp) and
// distinct.hip (count distinct) share: the workgroup scan, the element size of a dtype they accept, and the offsets {0, n} that turn a
// whole column into the one group of a flat call.
#pragma once
#include "aqg_internal.hpp"
#include "dev_common.hpp"
#include "key_image.hpp"

namespace seldev {

// inclusive sum over the lanes of a workgroup (wsum: one word of LDS per wavefront)
__device__ inline uint32_t block_scan_incl(uint32_t v, uint32_t* wsum) {
    const int lane = lane_id(), wid = wave_id();
    const uint32_t incl = wave_scan_incl(v, OpAdd{}, lane);
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wid; ++w) base += wsum[w];
    __syncthreads();
    return base + incl;
}

static __global__ void flat_offsets_kernel(uint32_t* off, uint32_t n) { off[0] = 0; off[1] = n; }

// bytes per element of the dtypes both take (the 1-, 2-, 4- and 8-byte numeric columns and BOOL), 0 for every other dtype
inline int esz_of(int t) {
    switch (t) {
    case AQG_INT8: case AQG_UINT8: case AQG_BOOL: return 1;
    case AQG_INT16: case AQG_UINT16: return 2;
    case AQG_INT32: case AQG_UINT32: case AQG_FLOAT: return 4;
    case AQG_INT64: case AQG_UINT64: case AQG_DOUBLE: return 8;
    }
    return 0;
}

} // namespace seldev
