// tile_scatter.hpp -- the tile scatter all partition plans move their rows with (tile_scatter.hip): what a caller fills in, and one host
// function per launch sequence.  Callers: partition1.hip, partition_wide.hip, sorted_tail.hip, partition_assign.hip
#pragma once
#include "groupby_dev.hpp"

namespace aqgdev {

constexpr int MAXPL = 4 + 2 * MAXACC;
constexpr int P2_TB = 1024, P2_TR = 16, P2_PT = P2_TB * P2_TR;     // 16384-row tiles: 64 KB of staging, two workgroups per CU
// Everything the scatter moves is a DWORD PLANE: one 32-bit word per row, read from a column of 4-byte elements (stride 1) or
// from one half of a column of 8-byte elements (stride 2 dwords), or made from the row index, and written at a dword stride.
// The key is one column of key words (4 or 8 bytes): tuples of several columns and 1- / 2-byte values are packed / widened into
// such columns first (p1_pack_keys_kernel, p1_widen_kernel).
enum : int { PL_LOAD = 0, PL_ROWIDX = 1, PL_PACK = 2 };
struct Plane {
    const uint32_t* src; int src_stride_dw; int src_off_dw;
    uint32_t* dst; int dst_stride_dw; int dst_off_dw;
    int kind;
};
// Narrow integer value columns travelling INSIDE the 4-byte key word (h2o: id6 < 2^24 leaves eight bits; v1 in 1..5 and v2 in 1..15 need
// seven): the first level's key plane is made as key | (v - min) << shift per field (PL_PACK), every later user of the word masks the
// fields off before hashing / comparing and the aggregation unpacks them -- Q5 moves three planes per level instead of five, Q7 two
// instead of four.  Ranges come from a sample of the rows; every row is verified while it is packed and a miss fails the call over to
// the unpacked plan (`flag`).
struct PackSpec { int n; const uint32_t* src[2]; uint32_t min[2], shift[2], fmask[2]; uint32_t kmax; uint32_t* flag; };
struct Planes {
    int n; Plane p[MAXPL]; PackSpec pk;
    void add(int kind, const void* s, int sstride, int soff, void* d, int dstride, int doff) {
        Plane& Q = p[n++];
        Q.kind = kind; Q.src = static_cast<const uint32_t*>(s); Q.src_stride_dw = sstride; Q.src_off_dw = soff;
        Q.dst = static_cast<uint32_t*>(d); Q.dst_stride_dw = dstride; Q.dst_off_dw = doff;
    }
    // a column of 4-byte elements as one plane, of 8-byte elements as its two halves
    void add_column(const void* s, void* d, int bytes) {
        if (bytes == 4) add(PL_LOAD, s, 1, 0, d, 1, 0);
        else { add(PL_LOAD, s, 2, 0, d, 2, 0); add(PL_LOAD, s, 2, 1, d, 2, 1); }
    }
};

struct P2Level {
    const uint32_t* seg_start;    // [nseg + 1] rows of every segment (level 1: the whole input; level 2: the coarse partitions)
    const uint32_t* tile_prefix;  // [nseg + 1] first tile of every segment
    uint32_t* cursor;             // write cursors: level 1 [B1], level 2 [P]
    uint32_t nseg, P, shift, mask, nbins, cursor_per_seg;
    uint32_t kclear;              // bits of the key word that are not key (packed value fields): cleared before hashing (0: none)
    uint32_t kmin, xmax;          // BIN_RANGED: the bin is umulhi(key - kmin, P) -- order-preserving bins over a dense key domain
    uint32_t* flag;               // BIN_RANGED: set when a key lies outside [kmin, kmin + xmax] (the range came from a sample)
    // XCD-local segments (null: off).  Workgroups go to the eight XCDs round-robin (blockIdx & 7), every XCD has its own L2, and a tile
    // writes one run per bin at an arbitrary alignment: the partial lines at the ends of neighbouring runs meet in ONE L2 -- and leave it
    // as whole lines -- only if the same XCD writes both.  With this map XCD x takes the segments x, x + 8, ... one after the other:
    // xtp[x * XTP_STRIDE + j] = tiles of its first j segments, xtp[8 * XTP_STRIDE] = 1 when the launch grid covers the fullest XCD.
    const uint32_t* xtp;
    uint32_t* xq;                 // the eight queue heads (one per 128-byte line, zeroed by the setup)
};
constexpr uint32_t XTP_STRIDE = 16;   // (<= 128 segments: up to 16 per XCD)
// how a key word becomes a bin: BIN_RAW umulhi(word, P) (dense group ids, row ids), BIN_HASHED umulhi(hash(word), P), BIN_RANGED
enum : int { BIN_RAW = 0, BIN_HASHED = 1, BIN_RANGED = 2 };

} // namespace aqgdev

// buffers of a segmented level: [nseg + 1] segment starts, their tile prefixes, [nseg * bins] write cursors; cnt (bin counts, [nseg * bins + 1])
// and bsum (scratch of the scan) serve the counted level only
struct LevelBufs { uint32_t *seg, *tp, *cnt, *cur, *bsum; };
// what the whole-column histogram and p2_setup_kernel leave: partition sizes and starts, segments / tile prefixes / cursors of both levels, the XCD map
struct ColumnBins { uint32_t *ftot, *fstart, *cur2, *seg1, *tp1, *cur1, *seg2, *tp2, *xtp; };

// a 1- / 2-byte column as dwords
void aqg_widen_column(aqg_ctx* ctx, const void* col, int esz, uint32_t n, uint32_t* out);
// bits of level l when `bits` bits are split over `levels` levels, most significant first; *shift: the bits of the levels below it
static inline uint32_t aqg_level_bits(uint32_t bits, uint32_t levels, uint32_t l, uint32_t* shift) {
    uint32_t lb = 0;
    for (uint32_t i = 0; i <= l; ++i) { lb = (bits + (levels - i) - 1) / (levels - i); bits -= lb; }
    *shift = bits;
    return lb;
}
// The scatter pair of one level: the whole tiles on `tiles` workgroups, then the partial tile of every segment on `tails`.  kbytes: width of the
// key word (4 / 8); mode: BIN_*; pack: plane 0 is made with the PackSpec's fields; nbmax: 128 or 256 bins.  AQG_ERR_ARG: no such kernel.
int aqg_scatter_pair(aqg_ctx* ctx, int kbytes, int mode, bool pack, int nbmax, const void* keys, const Planes& pl, const P2Level& lv, unsigned tiles, unsigned tails);
// One level over b.seg's nseg segments of n rows in all, bins counted here (counted: b.cnt already holds the counts, the wide plan's first level):
// tile prefixes, counts, scan, cursors, the scatter pair; b.seg then holds the nseg * nb segments of the next level.  mode: BIN_HASHED / BIN_RAW
int aqg_scatter_level_counted(aqg_ctx* ctx, const LevelBufs& b, int mode, bool counted, const uint32_t* keys, const Planes& pl, uint32_t n, uint32_t nseg,
                              uint32_t P, uint32_t shift, uint32_t mask, uint32_t nb, const char* what);
// One level whose segments and cursors are entries of `pstart` (order-preserving BIN_RAW bins of known sizes: no counting)
int aqg_scatter_level_offsets(aqg_ctx* ctx, const LevelBufs& b, const uint32_t* pstart, bool pack, uint32_t kclear, const uint32_t* keys, const Planes& pl,
                              uint32_t n, uint32_t nseg, uint32_t P, uint32_t shift, uint32_t nb, const char* what);
// Sizes of the P partitions of a whole key column (bin = umulhi(hash or key - kmin, scale)) and everything p2_setup_kernel derives from them, in
// workspace taken here.  xgrid: workgroups per XCD of the XCD-mapped second level (0: no map)
int aqg_scatter_column_bins(aqg_ctx* ctx, int kbytes, bool ranged, const void* keys, uint32_t n, uint32_t P, uint32_t scale, uint32_t kmin, uint32_t xmax,
                            unsigned xgrid, ColumnBins* c);
