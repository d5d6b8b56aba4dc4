// window_quantile.hip -- aqg_window_quantiles / aqg_grouped_window_quantiles(_flat): up to AQG_QUANTILES_MAX ranks of every row's window
// (medianw, quantilew), per group and flat (include/aqg.h, moving quantiles section, the contract).
//
// Rank tracking, O(w) per row, no sort and no atomics.  A workgroup owns WQ_TILE outputs and holds the order-preserving images
// (select_radix.hpp) of its rows and of the w - 1 rows in front of them (the halo) in LDS.  With the total order
//     b < a  :=  img[b] < img[a], or img[b] == img[a] and b in front of a
// the ranks of a window's rows are a permutation, so exactly one row holds each rank.  One lane per row a -- tile and halo rows alike --
// follows a through the outputs i of this tile whose window holds a: it counts the rows before a in the first of those windows (at most
// w - 1 LDS reads), and from i to i + 1 the rank moves by the row that enters (behind a: +1 iff its image is less) and the row that
// leaves (in front of a: -1 iff its image is less or equal).  Where the rank is r_j(len of the window) the lane writes a's element to
// plane j: one writer per output.  Adjacent lanes read adjacent LDS addresses at every step.
// r_j(len) comes from a table of w x nq 16-bit ranks that one small launch builds in workspace with exact 64-bit arithmetic; the kernel
// copies it into LDS and keeps the ranks of the full window in registers.
// Both layouts are one kernel (scan_window.hpp's whole_column / by_group): by_group holds the length of every output's window in LDS
// (by_group::len, the rule of sumw / minw), whole_column computes it and loads nothing for groups.
#include "scan_window.hpp"
#include "select_host.hpp"

namespace {
using aqgscan::by_group;
using aqgscan::whole_column;
using selradix::image_is_shared;
using selradix::image_of;
using selradix::QArgs;
using selradix::QMAX;
using selradix::value_of;

constexpr int WQ_SB = 256;                        // lanes per workgroup
constexpr uint32_t WQ_TILE = 2048;                // outputs per workgroup: the halo of the longest window is a third of the rows it holds
constexpr uint32_t NO_RANK = 0xFFFFFFFFu;
static_assert(AQG_WINQ_MAX_W <= 0xFFFF, "16-bit ranks and window lengths");

// LDS bytes of the images of a tile and its halo (whole 16 bytes: the 16-bit arrays follow)
__host__ __device__ constexpr size_t img_bytes(size_t esz, uint32_t w) { return (((size_t)w - 1 + WQ_TILE) * esz + 15) & ~(size_t)15; }

// R[(len - 1) * nq + j] = rank of quantile j in a window of len rows, 1 <= len <= w
__global__ void __launch_bounds__(WQ_SB) winq_ranks_kernel(QArgs qa, uint32_t w, uint16_t* __restrict__ R) {
    const uint32_t k = blockIdx.x * WQ_SB + threadIdx.x;
    if (k >= w * qa.nq) return;
    const uint64_t p = (uint64_t)qa.num[k % qa.nq] * (k / qa.nq);
    R[k] = (uint16_t)(p / qa.den + (qa.which && p % qa.den != 0 ? 1u : 0u));
}

// LDS position p <-> row t0 - H + p, with the halo H = w - 1; positions in front of row 0 or behind row n - 1 are never read
template <class U, int KIND, class M>
__global__ void __launch_bounds__(WQ_SB) winq_kernel(const U* __restrict__ x, uint32_t n, uint32_t w, M seg, uint32_t nq, const uint16_t* __restrict__ R, U* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const uint32_t t0 = blockIdx.x * WQ_TILE, rows = n - t0 < WQ_TILE ? n - t0 : WQ_TILE;     // t0 < n
    const uint32_t H = w - 1, L = H + rows;
    U* img = reinterpret_cast<U*>(smem_raw);
    uint16_t* Rl = reinterpret_cast<uint16_t*>(smem_raw + img_bytes(sizeof(U), w));            // the rank table
    uint16_t* LEN = Rl + (size_t)w * nq;                                                      // by_group: rows of the window of every output
    for (uint32_t p = threadIdx.x; p < L; p += WQ_SB) {
        const int64_t r = (int64_t)t0 - (int64_t)H + p;
        img[p] = r >= 0 ? image_of<U, KIND>(x[r]) : U(0);                                     // r < t0 + rows <= n
    }
    for (uint32_t k = threadIdx.x; k < w * nq; k += WQ_SB) Rl[k] = R[k];
    if constexpr (M::SEG) {
        for (uint32_t p = threadIdx.x; p < rows; p += WQ_SB) LEN[p] = (uint16_t)seg.len(t0 + p, w);
    }
    __syncthreads();
    auto len_at = [&](uint32_t q) -> uint32_t {                                               // q >= H: the output at position q
        if constexpr (M::SEG) return LEN[q - H]; else return seg.len(t0 + (q - H), w);
    };
    uint32_t rw[QMAX];                                                                        // the ranks of a full window
#pragma unroll
    for (uint32_t j = 0; j < QMAX; ++j) rw[j] = j < nq ? (uint32_t)Rl[(size_t)(w - 1) * nq + j] : NO_RANK;

    for (uint32_t pa = threadIdx.x; pa < L; pa += WQ_SB) {
        uint32_t q = pa < H ? H : pa;                                                         // the first output of this tile at or behind a
        uint32_t len = len_at(q);
        if (q - pa >= len) continue;                                                          // a halo row whose group ends before the tile, or rows in front of row 0
        const U ia = img[pa];
        uint32_t rank = 0;
        for (uint32_t b = q + 1 - len; b < pa; ++b) rank += img[b] <= ia ? 1u : 0u;
        for (uint32_t b = pa + 1; b <= q; ++b) rank += img[b] < ia ? 1u : 0u;
        const size_t ra = (size_t)t0 + pa - H;                                                // a's row (pa >= q + 1 - len: not in front of row 0)
        const U val = image_is_shared<U, KIND>(ia) ? x[ra] : value_of<U, KIND>(ia);
        for (;;) {
            const size_t i = (size_t)t0 + (q - H);
            if (len == w) {
#pragma unroll
                for (uint32_t j = 0; j < QMAX; ++j)
                    if (rank == rw[j]) out[(size_t)j * n + i] = val;
            } else {
                const uint16_t* rl = Rl + (size_t)(len - 1) * nq;
                for (uint32_t j = 0; j < nq; ++j)
                    if (rank == rl[j]) out[(size_t)j * n + i] = val;
            }
            if (++q == L) break;
            const uint32_t nlen = len_at(q);
            if (q - pa >= nlen) break;                                                        // a has left the window, or a new group starts
            rank += img[q] < ia ? 1u : 0u;                                                    // the row that enters lies behind a
            if (len == w) rank -= img[q - w] <= ia ? 1u : 0u;                                 // the row that leaves lies in front of a
            len = nlen;
        }
    }
}

size_t winq_lds_bytes(size_t esz, uint32_t w, uint32_t nq, bool seg) { return img_bytes(esz, w) + (size_t)w * nq * 2 + (seg ? (size_t)WQ_TILE * 2 : 0); }
size_t winq_ws_bytes(uint32_t w, uint32_t nq) { return (size_t)w * nq * 2 + 4096; }

template <class U, int KIND, class M>
int run_winq(aqg_ctx* ctx, const QArgs& qa, const void* x, uint32_t n, uint32_t w, M seg, void* out) {
    uint16_t* R;
    AQG_TRY(aqg_ws_get(ctx, (size_t)w * qa.nq, &R));
    hipLaunchKernelGGL(winq_ranks_kernel, dim3(aqg_ceil_div(w * qa.nq, WQ_SB)), dim3(WQ_SB), 0, ctx->stream, qa, w, R);
    return aqgscan::launch_window(ctx, &winq_kernel<U, KIND, M>, aqg_ceil_div(n, WQ_TILE), WQ_SB, winq_lds_bytes(sizeof(U), w, qa.nq, M::SEG), "winq_kernel",
                                  static_cast<const U*>(x), n, w, seg, qa.nq, (const uint16_t*)R, static_cast<U*>(out));
}
template <class M>
int dispatch_winq(aqg_ctx* ctx, const QArgs& qa, int t, const void* x, uint32_t n, uint32_t w, M seg, void* out) {
    return selradix::dispatch_kind(t, [&]<class U, int KIND>() { return run_winq<U, KIND>(ctx, qa, x, n, w, seg, out); });
}

// the checks every entry shares; fills qa and the effective window *ww = min(w, n)
int check_winq(aqg_ctx* ctx, int which, uint32_t nq, const uint32_t* num, uint32_t den, int t, const void* x, uint32_t n, uint32_t w, const void* out, QArgs* qa, uint32_t* ww) {
    AQG_TRY(selradix::check_quant(ctx, "window quantiles", which, nq, num, den, qa));
    if (w < 1) return aqg_fail(ctx, AQG_ERR_ARG, "window quantiles: w >= 1");
    const int esz = seldev::esz_of(t);
    if (!esz) return aqg_fail(ctx, AQG_ERR_DTYPE, "window quantiles: 1-, 2-, 4- and 8-byte numeric columns and BOOL");
    if ((!x || !out) && n) return aqg_fail(ctx, AQG_ERR_ARG, "window quantiles: null column");
    AQG_CHECK_ROWS(ctx, n, "window quantiles");
    *ww = w < n ? w : n;
    if (*ww > AQG_WINQ_MAX_W) return aqg_fail(ctx, AQG_ERR_ARG, "window quantiles: the effective window min(w, n) exceeds AQG_WINQ_MAX_W");
    const uintptr_t xb = reinterpret_cast<uintptr_t>(x), ob = reinterpret_cast<uintptr_t>(out);
    if (n && xb < ob + (uint64_t)nq * n * esz && ob < xb + (uint64_t)n * esz) return aqg_fail(ctx, AQG_ERR_ARG, "window quantiles: out overlaps x");
    ctx->winq_tile = WQ_TILE;
    ctx->winq_halo = *ww ? *ww - 1 : 0;
    return AQG_OK;
}
int check_grouped(aqg_ctx* ctx, const aqg_groupby* g) {
    if (!ctx || !g) return aqg_fail(ctx, AQG_ERR_ARG, "grouped window quantiles: bad argument");
    if (!g->has_reversemap || !g->has_counts) return aqg_fail(ctx, AQG_ERR_ARG, "grouped window quantiles: the handle was not made by aqg_groupby_build");
    return AQG_OK;
}

} // namespace

extern "C" {

int aqg_window_quantiles(aqg_ctx* ctx, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, uint32_t n, uint32_t w, void* out_dev) {
    if (!ctx) return AQG_ERR_ARG;
    QArgs qa;
    uint32_t ww;
    AQG_TRY(check_winq(ctx, which, nq, num_host, den, t, x, n, w, out_dev, &qa, &ww));
    if (n == 0) return AQG_OK;
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, winq_ws_bytes(ww, nq)));
    return dispatch_winq(ctx, qa, t, x, n, ww, whole_column{}, out_dev);
}

int aqg_grouped_window_quantiles_flat(aqg_ctx* ctx, aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* xflat, uint32_t w, void* out_flat_dev) {
    AQG_TRY(check_grouped(ctx, g));
    QArgs qa;
    uint32_t ww;
    AQG_TRY(check_winq(ctx, which, nq, num_host, den, t, xflat, g->n, w, out_flat_dev, &qa, &ww));
    if (g->n == 0 || g->ngroups == 0) return AQG_OK;
    if (!aqg_groupby_offsets(g)) return AQG_ERR_HIP;                      // makes the start bitmap of the flat layout on first use
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, winq_ws_bytes(ww, nq)));
    return dispatch_winq(ctx, qa, t, xflat, g->n, ww, by_group{g->flat_heads, nullptr}, out_flat_dev);
}

int aqg_grouped_window_quantiles(aqg_ctx* ctx, aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, uint32_t w, void* out_flat_dev) {
    AQG_TRY(check_grouped(ctx, g));
    QArgs qa;
    uint32_t ww;
    AQG_TRY(check_winq(ctx, which, nq, num_host, den, t, x, g->n, w, out_flat_dev, &qa, &ww));
    const uint32_t n = g->n;
    if (n == 0 || g->ngroups == 0) return AQG_OK;
    if (!aqg_groupby_offsets(g)) return AQG_ERR_HIP;
    const int esz = seldev::esz_of(t);
    AQG_TRY(aqg_ws_reset(ctx));
    AQG_TRY(aqg_ws_ensure(ctx, (size_t)n * esz + 4096 + aqg_postproc_ws_bytes(n, g->ngroups, esz) + winq_ws_bytes(ww, nq)));
    unsigned char* xs;
    AQG_TRY(aqg_ws_get(ctx, (size_t)n * esz + 64, &xs));
    AQG_TRY(aqg_radix_by_group(ctx, g, nullptr, x, esz, xs, /*ws_managed=*/true));
    return dispatch_winq(ctx, qa, t, xs, n, ww, by_group{g->flat_heads, nullptr}, out_flat_dev);
}

int aqg_window_quantiles_last(aqg_ctx* ctx, uint32_t* tile_rows, uint32_t* halo_rows) {
    if (!ctx || !tile_rows || !halo_rows) return aqg_fail(ctx, AQG_ERR_ARG, "aqg_window_quantiles_last: bad argument");
    *tile_rows = ctx->winq_tile;
    *halo_rows = ctx->winq_halo;
    return AQG_OK;
}

} // extern "C"
