/*
 * aqg.h -- C-ABI of the MI355X (gfx950) AQuery execution library.
 *
 * This is the drop-in boundary for the column-batch hot path of the AQuery
 * "AQuery Library" headers (reference: server/vector_type.hpp, server/table.h,
 * server/aggregations.h, server/hasher.h).  Everything above this header is
 * host C++ (include/aquery/ *.h mirror the reference's header-level API);
 * everything below it is hand-written HIP for CDNA4.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types cross this boundary.
 *   - every column pointer is a DEVICE pointer (HBM) unless the parameter is
 *     documented "host".  Sizes are uint32_t like the reference
 *     (server/vector_type.hpp:66: `uint32_t size, capacity`).
 *   - dtype tags are the reference's own (server/aquery_types.h:1-5).
 *   - every entry point returns an int status (0 = AQG_OK).  The reference has
 *     no error channel on this path; a non-zero status here means
 *     "nothing was written, caller may fall back".
 *   - kernels are enqueued on the context's HIP stream.  Entry points that
 *     return a host value synchronise that stream before returning; all others
 *     are asynchronous (call aqg_sync).
 *   - __int128 results (reference: types::GetLongType, server/types.h:205-210)
 *     are written as 16-byte little-endian two's complement.
 */
#ifndef AQG_H
#define AQG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dtype tags: reference server/aquery_types.h:1-5 (same order) -------- */
typedef enum aqg_dtype {
    AQG_INT32 = 0, AQG_FLOAT = 1, AQG_STR = 2, AQG_DOUBLE = 3, AQG_LDOUBLE = 4,
    AQG_INT64 = 5, AQG_INT128 = 6, AQG_INT16 = 7, AQG_DATE = 8, AQG_TIME = 9,
    AQG_INT8 = 10, AQG_UINT32 = 11, AQG_UINT64 = 12, AQG_UINT128 = 13,
    AQG_UINT16 = 14, AQG_UINT8 = 15, AQG_BOOL = 16, AQG_VECTOR = 17,
    AQG_TIMESTAMP = 18, AQG_CHAR = 19, AQG_SV = 20, AQG_NONE = 21, AQG_ERROR = 22
} aqg_dtype;

/* ---- status codes --------------------------------------------------------- */
enum {
    AQG_OK = 0,
    AQG_ERR_HIP = 1,       /* a HIP runtime call failed (see aqg_last_error)  */
    AQG_ERR_DTYPE = 2,     /* dtype / op combination not implemented on device */
    AQG_ERR_ARG = 3,       /* bad argument                                     */
    AQG_ERR_NOMEM = 4,     /* device allocation failed                         */
    AQG_ERR_NODEVICE = 5,  /* no gfx950 device visible                         */
    AQG_ERR_OVERFLOW = 6   /* table / workspace capacity exceeded              */
};

/* Largest supported row count of one column.  Sizes are uint32_t like the reference's (server/vector_type.hpp:66); the tile
 * kernels compute row indices in 32 bits with up to one tile / one grid stride of slack, so counts within 2^20 of 2^32 are
 * rejected with AQG_ERR_ARG instead of wrapping. */
#define AQG_MAX_ROWS 4293918720u   /* 2^32 - 2^20 */

typedef struct aqg_ctx aqg_ctx;

/* ---- type rules (host, pure) ----------------------------------------------
 * Replace the reference's compile-time type functions so that every caller
 * (templates, tests, other languages) derives result dtypes the same way.   */
size_t aqg_dtype_size(int dt);           /* types::AType_sizes, server/types.h:192-193 */
int aqg_long_type(int dt);               /* types::GetLongType, server/types.h:205-210 */
int aqg_fp_type(int dt);                 /* types::GetFPType,   server/types.h:199-204 */
int aqg_coercion(int dt1, int dt2);      /* types::Coercion,    server/types.h:264-275 */

/* ---- context / stream / memory --------------------------------------------
 * One context per (process, GPU).  `stream` may be an existing hipStream_t
 * (e.g. torch's current stream) or NULL to let the library create its own.   */
int aqg_device_count(void);
int aqg_ctx_create(int device, void* hip_stream, aqg_ctx** out);
void aqg_ctx_destroy(aqg_ctx* ctx);
const char* aqg_last_error(aqg_ctx* ctx);
void* aqg_ctx_stream(aqg_ctx* ctx);
int aqg_sync(aqg_ctx* ctx);
/* pre-size the internal workspace arena (block partials, hash tables) so that
 * later calls never allocate: call once before a timed / graph-captured region */
int aqg_reserve_workspace(aqg_ctx* ctx, size_t bytes);

/* Replaces malloc/GC::reg/ScratchSpace for device temporaries
 * (server/vector_type.hpp:70-80,367-371; server/gc.h:7-41).                  */
int aqg_malloc(aqg_ctx* ctx, size_t bytes, void** dptr);
int aqg_free(aqg_ctx* ctx, void* dptr);
int aqg_h2d(aqg_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int aqg_d2h(aqg_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* device-to-device copy on the context's stream (vector_type::subvec_memcpy / the copy constructors, vector_type.hpp:83-135,228-240) */
int aqg_d2d(aqg_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
int aqg_memset(aqg_ctx* ctx, void* dst_dev, int byte, size_t bytes);

/* Device mirror of a borrowed host column (the ColRef<T>(len, server->getCol(i)) binding, engine/ast.py:367-370; the data
 * source hands out zero-copy pointers into its own result memory, server/monetdb_conn.cpp:203-224): on first sight of
 * (host_ptr, bytes) the column is uploaded, afterwards the cached device pointer is returned; aqg_col_unpin_all drops the
 * cache (the reference's per-dll session end).  The upload is ASYNCHRONOUS: the host range is page-locked chunk by chunk and
 * copied by DMA on a copy stream while the call returns; the context's stream waits for its completion, so every later call
 * of this library (and aqg_sync) is ordered behind it.  The host memory must stay valid and unchanged until then -- the
 * reference's borrowed columns live as long as the query.  PCIe line rate (56-57 GB/s measured on the MI355X box).          */
int aqg_col_pin(aqg_ctx* ctx, const void* host_ptr, size_t bytes, void** dptr);
/* how the chunks of the most recent upload of this context travelled: page-locked + DMA; staged through the library's own pinned buffers
 * (the chunk touches pages that are already page-locked -- by another column or context of this library, or by somebody else, which a
 * direct copy or a second registration must not touch: profiles/r3_hostregister_abort.md); plain pageable copy (short columns)       */
int aqg_col_pin_last(aqg_ctx* ctx, uint32_t* registered_chunks, uint32_t* staged_chunks, uint32_t* pageable_chunks);
/* Egress of a result column into caller-owned host memory (the write-back half of the seam: TableInfo::monetdb_append_table hands the
 * data source pointers to the result columns, server/table_ext_monetdb.hpp:34-87): asynchronous, ordered behind everything queued on the
 * context's stream, destination page-locked chunk by chunk + DMA on the copy stream; several columns overlap each other and the query's
 * tail kernels.  aqg_col_fetch_wait: every fetch of this context is complete and its pages are unlocked.                            */
int aqg_col_fetch(aqg_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int aqg_col_fetch_wait(aqg_ctx* ctx);
int aqg_col_unpin(aqg_ctx* ctx, const void* host_ptr);
int aqg_col_unpin_all(aqg_ctx* ctx);

/* ---- element-wise column arithmetic / compare ------------------------------
 * Replaces the free operators server/table.h:820-937 and aqop_* :954-973.
 * ret[i] = l[i] OP r[i] evaluated in the C++ usual-arithmetic-conversion type
 * of (lt, rt) exactly as the reference loop body does, then converted to `ot`.
 * `ot` is the caller's result dtype: Coercion for + and -, GetLongType for *,
 * GetFPType for / (so int32/int32 is an INTEGER quotient stored as float),
 * AQG_BOOL for comparisons.                                                   */
typedef enum aqg_binop {
    AQG_OP_ADD = 0, AQG_OP_SUB = 1, AQG_OP_MUL = 2, AQG_OP_DIV = 3, AQG_OP_MOD = 4,
    AQG_OP_AND = 5, AQG_OP_OR = 6, AQG_OP_XOR = 7,
    AQG_OP_GT = 8, AQG_OP_LT = 9, AQG_OP_GE = 10, AQG_OP_LE = 11, AQG_OP_EQ = 12, AQG_OP_NE = 13
} aqg_binop;
enum { AQG_VEC_VEC = 0, AQG_VEC_SCALAR = 1, AQG_SCALAR_VEC = 2 };
/* for *_SCALAR kinds the scalar side is a HOST pointer to one value of its dtype */
int aqg_ewise(aqg_ctx* ctx, int op, int kind, int lt, const void* l, int rt, const void* r,
              int ot, void* out, uint32_t n);
/* result dtype of the reference's FREE operator for (op, lt, rt): table.h:779-818 */
int aqg_ewise_out_dtype(int op, int lt, int rt);

/* sqrt (server/aggregations.h:34-46) / truncate (:57-69) */
typedef enum aqg_unop { AQG_UN_SQRT = 0, AQG_UN_TRUNCATE = 1 } aqg_unop;
int aqg_unary(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, uint32_t param, int ot, void* out);

/* ---- full-column reductions: server/aggregations.h:10-32,71-86,332-348,383-416,487-497
 * `out_host` receives 16 bytes: SUM -> GetLongType (int128/uint128/double),
 * MIN/MAX/FIRST/LAST -> T, COUNT -> uint64, AVG/VAR/STDDEV -> double.
 * Reference quirks kept on purpose: max seeds with numeric_limits<T>::min()
 * (:73, D8), var divides by len+1 (:347, D9).
 * NaN rows: min / max, and sum / avg of floating columns, depend on the order of evaluation once a column holds a NaN (the
 * reference's folds forget what came before it).  The call succeeds; the value is unspecified.  Of 0.0 and
 * -0.0 either may come back as a min / max.  +-Inf rows are ordinary values.                                                  */
typedef enum aqg_redop {
    AQG_RED_SUM = 0, AQG_RED_MIN = 1, AQG_RED_MAX = 2, AQG_RED_COUNT = 3, AQG_RED_AVG = 4,
    AQG_RED_VAR = 5, AQG_RED_STDDEV = 6, AQG_RED_FIRST = 7, AQG_RED_LAST = 8
} aqg_redop;
int aqg_reduce(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, void* out_host16);
int aqg_reduce_out_dtype(int op, int t);
/* asynchronous form: 16-byte result left in device memory */
int aqg_reduce_dev(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, void* out_dev16);
/* corr(x, y): server/aggregations.h:383-407 */
int aqg_corr(aqg_ctx* ctx, int tx, const void* x, int ty, const void* y, uint32_t n, double* out_host);

/* ---- prefix scans, sliding windows, shifts ---------------------------------
 * sums/avgs/mins/maxs  server/aggregations.h:89-125,203-236
 * sumw/avgw/minw/maxw/ratiow :127-191,238-281 ; varw/stddevw :283-330 (D9: out-of-bounds read in the reference;
 *   here the population variance of the last min(w, i+1) rows, held to tests/test_gpu_variance.py)
 * deltas/prev/aggnext :439-485 ; ratios = ratiow(1) :193-201 ; vars/stddevs :350-381
 * window = elements [i-w+1, i]; growing prefix for i < w.
 * NaN rows: mins / maxs / minw / maxw, and sums / avgs / sumw / avgw of floating columns, are specified for every output row strictly
 * before the column's first NaN row (sumw / avgw: before the reference's first NaN output, which an Inf row leaving the window causes
 * too); behind it the values are unspecified and the call still succeeds.  Shifts and ratios move / divide NaNs like any value.
 * avgs of an 8-byte integer column sums from its first row rounded to double, like the reference (`s = ret[0] = arr[0]`).     */
typedef enum aqg_scanop {
    AQG_SCAN_SUMS = 0, AQG_SCAN_AVGS = 1, AQG_SCAN_MINS = 2, AQG_SCAN_MAXS = 3,
    AQG_SCAN_SUMW = 4, AQG_SCAN_AVGW = 5, AQG_SCAN_MINW = 6, AQG_SCAN_MAXW = 7,
    AQG_SCAN_RATIOW = 8, AQG_SCAN_DELTAS = 9, AQG_SCAN_PREV = 10, AQG_SCAN_NEXT = 11,
    AQG_SCAN_VARS = 12, AQG_SCAN_STDDEVS = 13, AQG_SCAN_VARW = 14, AQG_SCAN_STDDEVW = 15
} aqg_scanop;
int aqg_scan(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, uint32_t w, void* out);
int aqg_scan_out_dtype(int op, int t);
/* sums / avgs of one row-range shard of a column: rows [row_offset, row_offset + n) of the whole column.
 * `carry_host16` = the sum of every earlier row in the result's LongType (server/types.h:152-160): 16 bytes holding an
 * __int128 / unsigned __int128 for integer columns, a double in the first 8 bytes for floating ones; NULL = nothing before.
 * Element i is carry + x[0..i] (sums, aggregations.h:89-103) or that over (row_offset + i + 1) (avgs, :105-125), i.e. the
 * rows the whole-column scan would have produced.  Integer results are bit-identical to the unsharded scan.  */
int aqg_scan_resume(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, const void* carry_host16, uint64_t row_offset, void* out);

/* ---- gather / mask filter ---------------------------------------------------
 * ColRef::operator[](vector_type<uint32_t>&)  server/table.h:184-189
 * ColRef::operator[](const std::vector<bool>&) server/table.h:190-198 (as a true
 * stream compaction; the reference's N-junk prefix, defect D11, is not kept)   */
int aqg_gather(aqg_ctx* ctx, int t, const void* x, const uint32_t* idx, uint32_t m, void* out);
/* the gather that knows about missing rows (the build columns of a LEFT join, of a look-up with misses):
 * out[i] = idx[i] == 0xFFFFFFFF ? *fill_host : x[idx[i]]   (elements of 1, 2, 4, 8, 16 bytes; fill_host NULL = zero bytes) */
int aqg_gather_fill(aqg_ctx* ctx, int t, const void* x, const uint32_t* idx, uint32_t m, const void* fill_host, void* out);
int aqg_compact(aqg_ctx* ctx, int t, const void* x, const uint8_t* mask, uint32_t n,
                void* out, uint32_t* m_host);
/* row ids of set mask entries, ascending (selection vector for multi-column filters) */
int aqg_mask_to_index(aqg_ctx* ctx, const uint8_t* mask, uint32_t n, uint32_t* idx_out, uint32_t* m_host);

/* ---- sort --------------------------------------------------------------------
 * TableInfo::order_by  server/table.h:447-465 (a host std::sort over a tuple comparator there).
 * keys[j]: device columns of n rows, key 0 most significant; INT8/16/32/64/128, UINT8/16/32/64/128, BOOL, FLOAT, DOUBLE
 * (other dtypes: AQG_ERR_DTYPE, nothing written).  rows_in: m device row ids below n, repeats allowed; NULL = identity, m == n.
 * rows_out receives m ids; it may equal or overlap rows_in and must not overlap a key column.  STABLE: ties keep the order of rows_in.
 * ASC / DESC: ascending / descending value.  NEG: ascending two's-complement negation in the key's own width (the header
 * layer's `-col[i]` key of unsigned 32/64/128-bit columns: 0 first, the rest descending); not for floating keys (AQG_ERR_ARG).
 * Floating keys: -0.0 == +0.0 (the next key or the input order breaks the tie); every NaN is one key, after +inf under ASC,
 * before it under DESC.  1 <= nkeys <= 8.  Asynchronous, scratch from the context workspace.                     */
enum { AQG_ORDER_ASC = 0, AQG_ORDER_DESC = 1, AQG_ORDER_NEG = 2 };
int aqg_sort_rows(aqg_ctx* ctx, int nkeys, const int* key_dtypes, const void* const* keys, const int* orders,
                  uint32_t n, const uint32_t* rows_in, uint32_t m, uint32_t* rows_out);
/* digit passes the last aqg_sort_rows on this context actually ran (skipped passes not counted) */
int aqg_sort_last_passes(aqg_ctx* ctx, uint32_t* passes_host);

/* ---- median ------------------------------------------------------------------
 * `median`, a built-in aggregate of the query language (common/types.py:343: fnmedian, result type "as is"); the reference's
 * server/aggregations.h has no body for it and its h2o file leaves the query commented out (benchmark/h2o/groupby.sql:11-12:
 * `median(v3), stddev(v3) ... GROUP BY id4, id5`).  A device radix SELECTION over order-preserving images, not a sort.
 * Result: the column's own dtype `t`, an ELEMENT OF THE INPUT bit for bit -- the row of rank (c-1)/2 (AQG_SEL_LOWER) or c/2
 * (AQG_SEL_UPPER), integer division, of the c rows in ascending order.  AQG_SEL_LOWER is what `median` means here: an odd count gives
 * the middle element, an even count the lower of the two middle ones (meant to match a SQL engine's "element, rounded down" median;
 * PARITY UNPINNED: no executable reference median exists).  AQG_SEL_UPPER lets a caller form h2o's averaged
 * median as (lower + upper) / 2 with aqg_ewise.
 * Order: that of aqg_sort_rows under AQG_ORDER_ASC.  Integers and BOOL by value.  Floating columns: -0.0 and +0.0 are one value
 * (which zero comes back is unspecified when the slice holds both); every NaN is one value above +inf, and when the rank falls
 * among the NaNs the result is a NaN of unspecified sign and payload -- the call succeeds.
 * Dtypes: INT8/16/32/64, UINT8/16/32/64, BOOL, FLOAT, DOUBLE; anything else (the 128-bit integers too: the flat layout does not
 * carry 16-byte elements) returns AQG_ERR_DTYPE with nothing written.
 *   aqg_median               the whole column; sizeof(T) bytes at the start of 16 zeroed HOST bytes.  n == 0: AQG_OK and 16 zero bytes.
 *   aqg_grouped_median       out_dev[g] for all G groups in group order, x in ROW layout (brought into the flat layout in workspace)
 *   aqg_grouped_median_flat  the same over a column already in the FLAT LAYOUT of the build (see the per-group scans below)
 * The grouped forms need a handle of aqg_groupby_build (as aqg_grouped_scan); G == 0 returns AQG_OK.  The input is never modified.
 * Asynchronous on the context's stream (aqg_median synchronises for its host result: the call's one round trip), scratch from
 * the context workspace, no allocation in steady state, and a number of launches that does not depend on the group count.
 * aqg_select_last_routes (diagnostic, like aqg_sort_last_passes): a mask of the routes the groups of the last call took
 * (1 SMALL, 2 GROUP, 4 SPLIT) and the largest number of digit passes any group needed.               */
enum { AQG_SEL_LOWER = 0, AQG_SEL_UPPER = 1 };
int aqg_median(aqg_ctx* ctx, int which, int t, const void* x, uint32_t n, void* out_host16);
struct aqg_groupby;
int aqg_grouped_median(aqg_ctx* ctx, struct aqg_groupby* g, int which, int t, const void* x, void* out_dev);
int aqg_grouped_median_flat(aqg_ctx* ctx, struct aqg_groupby* g, int which, int t, const void* xflat, void* out_dev);
int aqg_select_last_routes(aqg_ctx* ctx, uint32_t* routes_host, uint32_t* passes_host);

/* ---- top-k -------------------------------------------------------------------
 * The k largest or k smallest elements of a column, of every group: h2o Q8 (`-- select top 2 from each grp`,
 * benchmark/h2o/groupby.sql:16-17, where the emitted `v3[val].subvec(0, 2)` returns the first two entries of the group's row list
 * instead) and `ORDER BY x DESC LIMIT k` (engine/ast.py:451-454 sorts every row to print k).  A device SELECTION built on the median's
 * radix selection: rows are never moved.
 * Order: that of aqg_sort_rows.  AQG_ORDER_DESC: the k largest, largest first; AQG_ORDER_ASC: the k smallest, smallest first;
 * AQG_ORDER_NEG: AQG_ERR_ARG.  Integers and BOOL by value.  Floating columns: -0.0 and +0.0 are one value; every NaN is one value
 * above +inf, so NaNs come first under DESC.
 * Output, for group g of c rows and m = min(k, c) (aqg_topk: "group 0" is the whole column, c = n, and rows_out takes the place of
 * pos_out and holds row indices):
 *   vals_out[g*k + j], j < m   the j-th row of the group in that order, AN ELEMENT OF THE INPUT bit for bit
 *   pos_out[g*k + j],  j < m   that element's position (pos_out may be NULL).  Grouped calls: a position of the FLAT LAYOUT, in
 *                              [offsets[g], offsets[g+1]); the row id is row_ids[pos] of aqg_groupby_postproc.  vals_out[g*k+j] is
 *                              bitwise the column's element at pos_out[g*k+j]; the positions of a group are distinct, and among
 *                              slots of equal image (equal values; the two zeros; the NaNs) they ascend.
 *   slots j >= m               zero bytes in vals_out, 0xFFFFFFFF in pos_out (the missing-row marker of aqg_gather_fill)
 * When more rows tie on the k-th image than there are slots left, which of them are taken is unspecified (it may differ between
 * calls); the slots still hold distinct, ascending positions of rows with that image.
 * 1 <= k <= AQG_TOPK_MAX, anything else AQG_ERR_ARG.  Dtypes: those of aqg_median (INT8/16/32/64, UINT8/16/32/64, BOOL, FLOAT,
 * DOUBLE); anything else returns AQG_ERR_DTYPE with nothing written.
 *   aqg_topk               the whole column; vals_out_dev: k elements, rows_out_dev: k uint32 or NULL.  n == 0: AQG_OK, k empty slots.
 *   aqg_grouped_topk       G*k elements for all G groups in group order, x in ROW layout (brought into the flat layout in workspace)
 *   aqg_grouped_topk_flat  the same over a column already in the FLAT LAYOUT of the build
 * The grouped forms need a handle of aqg_groupby_build (a handle of aqg_groupby_agg: AQG_ERR_ARG, as the median); G == 0 or n == 0
 * returns AQG_OK.  The input is never modified.  Asynchronous on the context's stream with no host round trip (aqg_topk too: the
 * host knows min(k, n)), scratch from the context workspace, no allocation in steady state, and a number of launches that does not
 * depend on the group count.  Routes and thresholds are the median's (AQG_SELECT_SMALL_MAX, AQG_SELECT_SPLIT_MIN; DESIGN.md section
 * 4.11); aqg_select_last_routes reports, for these calls too, the mask of routes taken and the largest number of passes over its
 * rows any group needed -- here the digit passes of the threshold search plus the one pass that collects (SMALL: 1).            */
enum { AQG_TOPK_MAX = 1024 };
int aqg_topk(aqg_ctx* ctx, int order, int t, const void* x, uint32_t n, uint32_t k, void* vals_out_dev, uint32_t* rows_out_dev);
int aqg_grouped_topk(aqg_ctx* ctx, struct aqg_groupby* g, int order, int t, const void* x, uint32_t k, void* vals_out_dev, uint32_t* pos_out_dev);
int aqg_grouped_topk_flat(aqg_ctx* ctx, struct aqg_groupby* g, int order, int t, const void* xflat, uint32_t k, void* vals_out_dev, uint32_t* pos_out_dev);

/* ---- quantiles ---------------------------------------------------------------
 * Several ranks of a column, of every group, in ONE selection: `p95 / p99 of price by symbol`, the quartiles, or min, median and
 * max in one go.  The median's radix selection with up to AQG_QUANTILES_MAX states per group: every pass over a group's rows serves
 * all of its ranks, so nq ranks cost the passes of one.
 * Rank: quantile j of a slice of c >= 1 rows is the row of rank r_j in ascending order -- the order of aqg_sort_rows under
 * AQG_ORDER_ASC and of aqg_median (-0.0 and +0.0 one value, every NaN one value above +inf) -- with
 *   r_j = floor(num[j] * (c - 1) / den)   AQG_SEL_LOWER
 *   r_j = ceil (num[j] * (c - 1) / den)   AQG_SEL_UPPER
 * exact (unsigned 64-bit arithmetic on the device, per group; nothing comes back to the host).  num[j] == 0 is the least row,
 * num[j] == den the greatest, num = 1, den = 2 is aqg_median exactly for both values of `which`.  num may come in any order and may
 * repeat; out[g * nq + j] answers num[j].  1 <= nq <= AQG_QUANTILES_MAX, den >= 1 and num[j] <= den, anything else AQG_ERR_ARG
 * with nothing written.  num_host is read during the call and may be freed on return.
 * Result: AN ELEMENT OF THE INPUT bit for bit, in the column's own dtype `t`, with the median's two caveats and no others: when the
 * rank lands on a zero of a slice that holds both zeros, which zero comes back is unspecified; when it lands among the NaNs, some
 * NaN comes back.  Interpolating quantiles (numpy's `linear`) stay with the caller: lower, upper and aqg_ewise, as for h2o's
 * averaged median.
 * Dtypes: those of aqg_median (INT8/16/32/64, UINT8/16/32/64, BOOL, FLOAT, DOUBLE); anything else (the 128-bit integers too) returns
 * AQG_ERR_DTYPE with nothing written.
 *   aqg_quantiles               the whole column; nq elements of dtype t in HOST memory.  n == 0: AQG_OK and nq zeroed elements.
 *   aqg_grouped_quantiles       out_dev[g * nq + j] for all G groups in group order, x in ROW layout (brought into the flat layout in
 *                               workspace, once whatever nq is)
 *   aqg_grouped_quantiles_flat  the same over a column already in the FLAT LAYOUT of the build
 * The grouped forms need a handle of aqg_groupby_build (a handle of aqg_groupby_agg: AQG_ERR_ARG, as the median); G == 0 returns
 * AQG_OK.  The input is never modified.  Asynchronous on the context's stream (aqg_quantiles synchronises once for its host result),
 * scratch from the context workspace, no allocation in steady state, and a number of launches that depends on the dtype's width
 * only -- not on G and not on nq.  Routes and thresholds are the median's.  aqg_select_last_routes reports for these calls too: the
 * route mask, and the largest number of passes over its rows any group needed -- a pass that serves several ranks counts once.   */
enum { AQG_QUANTILES_MAX = 8 };
int aqg_quantiles(aqg_ctx* ctx, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, uint32_t n, void* out_host);
int aqg_grouped_quantiles(aqg_ctx* ctx, struct aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, void* out_dev);
int aqg_grouped_quantiles_flat(aqg_ctx* ctx, struct aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* xflat, void* out_dev);

/* ---- moving quantiles ----------------------------------------------------------
 * The windowed order statistics beside minw / maxw / avgw / varw: `medianw(21, price)` by symbol, a rolling p95 of a latency column --
 * up to AQG_QUANTILES_MAX ranks of every row's window in one pass.
 * Window: that of row i is rows [i - w + 1, i] of its SLICE -- the whole column, or the row's group in the flat layout -- clamped at the
 * slice's first row: len = min(w, predecessors of i in the slice + 1), the growing prefix of sumw / minw.
 * Rank: quantile j of row i is the row of rank r_j of that window in ascending order -- the order of aqg_median and of aqg_sort_rows
 * under AQG_ORDER_ASC (-0.0 and +0.0 one value, every NaN one value above +inf) -- with
 *   r_j = floor(num[j] * (len - 1) / den)   AQG_SEL_LOWER
 *   r_j = ceil (num[j] * (len - 1) / den)   AQG_SEL_UPPER
 * exact (unsigned 64-bit arithmetic on the device; nothing about the ranks comes from or goes to the host but num and den).  num = 1,
 * den = 2, AQG_SEL_LOWER is the moving median, `medianw`; num[j] == 0 is minw, num[j] == den maxw; w == 1 returns the input; a window
 * that is its whole slice gives aqg_quantiles of that slice.  num may come in any order and may repeat.
 * Result: nq planes of n elements of the column's own dtype `t`, out[j * n + i] answers num[j] for row i; the grouped forms in the flat
 * layout, like aqg_grouped_scan.  AN ELEMENT OF THE WINDOW bit for bit, with the median's two caveats and no others: when the rank lands
 * on a zero of a window that holds both zeros, which zero comes back is unspecified; when it lands among the NaNs, some NaN comes back.
 * Errors: 1 <= nq <= AQG_QUANTILES_MAX, den >= 1, num[j] <= den, w >= 1, else AQG_ERR_ARG.  The effective window is min(w, n); beyond
 * AQG_WINQ_MAX_W rows it returns AQG_ERR_ARG: the work is O(w) per row, a longer window wants another algorithm (unbuilt, DESIGN.md
 * section 4.14) -- the limit is a property of the interface, not a measurement.  `out` overlapping `x`: AQG_ERR_ARG.  Dtypes: those of
 * aqg_median; anything else returns AQG_ERR_DTYPE.  Every error returns with nothing written.  n == 0 or G == 0: AQG_OK.
 *   aqg_window_quantiles               the whole column
 *   aqg_grouped_window_quantiles       every group's rows, x in ROW layout (brought into the flat layout in workspace, once whatever nq is)
 *   aqg_grouped_window_quantiles_flat  the same over a column already in the FLAT LAYOUT of the build
 * The grouped forms need a handle of aqg_groupby_build (a handle of aqg_groupby_agg: AQG_ERR_ARG, as the median).  The input is never
 * modified.  Asynchronous on the context's stream, no host round trip, scratch from the context workspace, no allocation in steady
 * state; two launches (the rank table and the windows) whatever n, G, w and nq are, the row-layout form adds the flatten.
 * aqg_window_quantiles_last: the rows a workgroup owns (its tile) and the rows in front of a tile it reads as well (the halo, effective
 * w - 1) of the last such call on this context -- a diagnostic: the tests put slice starts on the kernel's real tile edges with it.   */
enum { AQG_WINQ_MAX_W = 1024 };
int aqg_window_quantiles(aqg_ctx* ctx, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, uint32_t n, uint32_t w, void* out_dev);
int aqg_grouped_window_quantiles(aqg_ctx* ctx, struct aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* x, uint32_t w, void* out_flat_dev);
int aqg_grouped_window_quantiles_flat(aqg_ctx* ctx, struct aqg_groupby* g, int which, uint32_t nq, const uint32_t* num_host, uint32_t den, int t, const void* xflat, uint32_t w, void* out_flat_dev);
int aqg_window_quantiles_last(aqg_ctx* ctx, uint32_t* tile_rows, uint32_t* halo_rows);

/* ---- ranking -------------------------------------------------------------------
 * Where every row stands in its slice: SQL's RANK / DENSE_RANK / ROW_NUMBER / PERCENT_RANK / CUME_DIST / NTILE(k) OVER (PARTITION BY
 * ... ORDER BY x), pandas' groupby().rank(method=...), kdb's rank / xrank -- for all groups in one call, rows never moved (DESIGN.md
 * section 4.19).  THE REFERENCE HAS NO SUCH FUNCTION; the contract is this comment, held by the exact model tests/rank_model.py.
 * Slice: the whole column, or a group's range [offsets[g], offsets[g+1]) of the flat layout; c is its row count.  Ranks are 1-based.
 * out[i] answers row i of the layout scanned; the grouped forms write the FLAT LAYOUT, like aqg_grouped_scan.
 * Order: that of aqg_sort_rows under AQG_ORDER_ASC or AQG_ORDER_DESC (AQG_ORDER_NEG: AQG_ERR_ARG, as for top-k).  Integers and BOOL by
 * value.  Floating columns: -0.0 and +0.0 tie; every NaN is one value and all NaNs tie; NaN sorts after +inf under ASC and before it
 * under DESC -- pandas' na_option='bottom' (ASC) resp. 'top' (DESC).  Under DESC, FIRST still breaks ties by ascending position.
 * NTILE(k): with q = c / k, r = c % k and o the 0-based FIRST rank, the bucket is o / (q + 1) + 1 when o < r (q + 1), else
 * r + (o - r (q + 1)) / q + 1 (SQL's distribution: the first r buckets hold one row more).  k >= 1, else AQG_ERR_ARG; k > c gives
 * bucket o + 1.  Every other method ignores k.
 * Exactness: the integer methods are exact.  AVERAGE is exact in double (min + max < 2^33).  PERCENT and CUME_DIST are ONE IEEE double
 * division of two exactly converted integers.  Results are bit-reproducible from call to call.
 * Dtypes: those of aqg_median; anything else, the 128-bit integers included, returns AQG_ERR_DTYPE.  AQG_ERR_ARG: a handle of
 * aqg_groupby_agg, `out` overlapping `x`, an unknown method or order, a NULL column with rows.  Every error returns with nothing
 * written; n == 0 or G == 0: AQG_OK.
 *   aqg_rank               the whole column
 *   aqg_grouped_rank       every group's rows, x in ROW layout (brought into the flat layout in workspace)
 *   aqg_grouped_rank_flat  the same over a column already in the FLAT LAYOUT of the build
 * The input is never modified.  Asynchronous on the context's stream, no allocation in steady state, one writer per output element, no
 * atomics on the result, and a number of launches that does not depend on G.  Groups of up to AQG_SELECT_SMALL_MAX rows are ranked by
 * comparison in LDS (SMALL); every other group through the stable sort of (group, x) and one rank-emit pass over the order (SORTED,
 * which reads the sort's digit histogram back as aqg_sort_rows does); one call takes both routes when its groups ask for both.  The
 * number of rows in groups above the SMALL threshold is read from the device ONCE PER HANDLE and cached in it.
 * aqg_rank_last: the mask of routes the last call on this context took (AQG_RANK_ROUTE_*) and the entries of the sorted order one
 * workgroup of the emit kernel owns -- a diagnostic: the tests put tie runs and group starts on the kernel's real tile edges with it. */
enum { AQG_RANK_MIN = 0,       /* SQL RANK, pandas 'min': 1 + rows of the slice that sort strictly before       -> uint32 */
       AQG_RANK_MAX = 1,       /* pandas 'max': rows that sort before or tie                                    -> uint32 */
       AQG_RANK_DENSE = 2,     /* DENSE_RANK: 1 + distinct values that sort strictly before                     -> uint32 */
       AQG_RANK_FIRST = 3,     /* ROW_NUMBER, pandas 'first': ties by ascending position in the layout scanned  -> uint32 */
       AQG_RANK_AVERAGE = 4,   /* pandas default: (min + max) / 2, exact                                        -> double */
       AQG_RANK_PERCENT = 5,   /* PERCENT_RANK: (min - 1) / (c - 1), 0 when c == 1                              -> double */
       AQG_RANK_CUME_DIST = 6, /* CUME_DIST: max / c                                                            -> double */
       AQG_RANK_NTILE = 7 };   /* NTILE(k): bucket 1..k of the FIRST rank, SQL's distribution (above)           -> uint32 */
enum { AQG_RANK_ROUTE_SMALL = 1, AQG_RANK_ROUTE_SORTED = 2 };
int aqg_rank_out_dtype(int method);   /* AQG_UINT32 or AQG_DOUBLE; -1 for an unknown method */
int aqg_rank(aqg_ctx* ctx, int method, int order, uint32_t k, int t, const void* x, uint32_t n, void* out_dev);
int aqg_grouped_rank(aqg_ctx* ctx, struct aqg_groupby* g, int method, int order, uint32_t k, int t, const void* x, void* out_flat_dev);
int aqg_grouped_rank_flat(aqg_ctx* ctx, struct aqg_groupby* g, int method, int order, uint32_t k, int t, const void* xflat, void* out_flat_dev);
int aqg_rank_last(aqg_ctx* ctx, uint32_t* routes_host, uint32_t* tile_rows_host);

/* ---- pair windows: moving and running statistics of two columns ------------------
 * covw / corrw / betaw and the running covs / corrs / betas of two columns, per group and flat: aqg_scan2, aqg_grouped_scan2,
 * aqg_grouped_scan2_flat, aqg_scan2_last.  Their contract and declarations are a header of their own, part of this one. */
#include "aqg_pair.h"

/* ---- exponential moving averages ------------------------------------------------
 * The decayed averages beside avgs / avgw: kdb's `ema`, pandas' `ewm(...).mean()`, "decayed price by symbol".  THE REFERENCE HAS NO SUCH
 * FUNCTION (server/aggregations.h stops at the windows): these entries stand in for the host loop per group a user would otherwise
 * write, and their contract is this comment, held by the exact model tests/ema_model.py.
 * Rows are taken in the order of the layout scanned: the column's own order, or the order of vecs[g] (the flat layout of a build,
 * descending row ids, like every grouped scan).  x is converted to double by round-to-nearest (exact but for 64-bit integers); results
 * are doubles; i counts from the first row of the SLICE (the column, or the row's group), which has no predecessor.
 *   AQG_EMA_RECURSIVE   y[0] = x[0], y[i] = b_i x[i] + a_i y[i-1]                                     (kdb ema, pandas adjust=False)
 *   AQG_EMA_ADJUSTED    N[0] = x[0], D[0] = 1, N[i] = a_i N[i-1] + x[i], D[i] = a_i D[i-1] + 1, y[i] = N[i] / D[i]     (pandas adjust=True)
 * Decay: a constant alpha, 0 < alpha <= 1 (anything else, NaN included: AQG_ERR_ARG) -- a_i = fl(1 - alpha), b_i = alpha -- or, when
 * `decay` is not NULL (alpha is then ignored), a device column of n doubles in the layout of x: a_i = decay[i] in [0, 1],
 * b_i = fl(1 - decay[i]).  The decay of a slice's first row is never read into the result.
 * Non-finite rows: from the first row of a slice whose x is NaN or +-Inf, or whose decay is NaN or outside [0, 1], to the slice's end
 * every output is non-finite (WHICH non-finite value is unspecified); rows before it and every other group are unaffected.  There is no
 * NULL-skipping -- pandas' ignore_na has no counterpart here, because the reference has no nulls.
 * The maps are composed in a tree order fixed by n, the group starts and the tile geometry: results are bit-reproducible from call to
 * call and within 4 (i + 2) 2^-53 max|x| (RECURSIVE) / 9 (i + 2) 2^-53 max|x| (ADJUSTED) of the exact value (max over the slice's rows
 * up to i); the flat and the grouped call need not agree bit for bit.
 *   aqg_scan_ema          the whole column
 *   aqg_grouped_ema       every group's rows, x (and decay) in ROW layout (brought into the flat layout in workspace, like aqg_grouped_scan)
 *   aqg_grouped_ema_flat  the same over columns already in the FLAT LAYOUT of the build; out in the flat layout either way
 * Dtypes: those of aqg_scan (every numeric type); 128-bit and non-numeric types: AQG_ERR_DTYPE.  A bad mode, a handle not made by
 * aqg_groupby_build, a NULL column with rows, `out` overlapping an input: AQG_ERR_ARG.  Every error returns with nothing written;
 * n == 0 or G == 0: AQG_OK.  Asynchronous on the context's stream, scratch from the context workspace, three to five launches whatever
 * n and G are (the row-layout form adds the flattens).
 * aqg_decay_from_times: decay[i] = 2^(-|t[i] - t[i-1]| / halflife), decay[0] = 1 -- a time-decayed average without a host pass (pandas
 * ewm(halflife=h, times=t)).  The absolute difference serves ascending columns and the descending order of vecs[g] alike, and group
 * borders need no care because a group's first decay is not read.  t: numeric (64-bit integers subtract in integer arithmetic before
 * the conversion), AQG_DATE (differences in days) or AQG_TIME (in milliseconds); anything else AQG_ERR_DTYPE.  halflife > 0 and
 * finite, in the unit of the differences, else AQG_ERR_ARG.  One element-wise launch.  aqg_grouped_decay_from_times_flat is the same over
 * a column in the flat layout of a build with decay = 1 at every group's first row (what the header layer hands out as a group's slice). */
enum { AQG_EMA_RECURSIVE = 0, AQG_EMA_ADJUSTED = 1 };
int aqg_scan_ema(aqg_ctx* ctx, int mode, int t, const void* x, uint32_t n, double alpha, const double* decay_dev /* NULL: constant alpha */, double* out);
int aqg_grouped_ema(aqg_ctx* ctx, struct aqg_groupby* g, int mode, int t, const void* x /* row layout */, double alpha, const double* decay_row /* row layout or NULL */, double* out_flat);
int aqg_grouped_ema_flat(aqg_ctx* ctx, struct aqg_groupby* g, int mode, int t, const void* xflat, double alpha, const double* decay_flat, double* out_flat);
int aqg_decay_from_times(aqg_ctx* ctx, int t, const void* times, uint32_t n, double halflife, double* decay_out);
int aqg_grouped_decay_from_times_flat(aqg_ctx* ctx, struct aqg_groupby* g, int t, const void* times_flat, double halflife, double* decay_flat);

/* ---- time-range windows: sumr / avgr / minr / maxr / countr ------------------
 * Windows measured in TIME, not in rows: "traded volume of the last 5 s by symbol", SQL RANGE BETWEEN :span PRECEDING AND CURRENT ROW,
 * pandas rolling("5s"), the window half of kdb's wj.  THE REFERENCE HAS NO SUCH FUNCTION; the contract is this comment, held by the
 * exact model tests/timewin_model.py.
 *
 * SLICE   the whole column, or one group's rows in the flat layout of an aqg_groupby_build handle (descending row ids, as every grouped
 *         scan sees them).
 * WINDOW  of row i: the rows [lo_i, i] of its slice, lo_i = the smallest position of the slice from which EVERY row up to i lies within
 *         `span` of t[i].  The window ends at row i itself (pandas rolling, kdb): later rows with the same stamp -- the peers a SQL RANGE
 *         frame would add -- are NOT in it.  Row i is always in its own window.
 * DISTANCE d(i, j) = |t[i] - t[j]|.  Integer, AQG_DATE (days) and AQG_TIME (milliseconds) stamps: exact in unsigned 64-bit arithmetic,
 *         larger minus smaller, never t[i] - span (nothing wraps at the ends of int64 / uint64).  Floating stamps: the one rounded
 *         subtraction in double, which is monotone in t[j].  The absolute value lets ascending columns and descending ones (the order
 *         of a group's rows in the flat layout of an ascending column) go through one code path.
 * FRAME   AQG_RANGEW_OPEN: d < span (pandas closed="right", the default); AQG_RANGEW_CLOSED: d <= span (SQL RANGE .. PRECEDING, pandas
 *         closed="both").  For integer / DATE / TIME stamps the span becomes ONE exact limit "in window <=> d <= dmax": CLOSED dmax =
 *         floor(span), OPEN dmax = ceil(span) - 1, both saturated at 2^64 - 1.  CLOSED needs span >= 0, OPEN span > 0; +Inf is allowed
 *         (the running sums / mins / maxs of the slice); NaN or anything else AQG_ERR_ARG.
 * ORDER   within one call the stamps of every slice run in one direction, all non-decreasing or all non-increasing.  When they do
 *         not, every lo still lies in [slice start, i], the outputs are unspecified and nothing is read out of bounds.  The bounds pass
 *         counts the rising and the falling steps inside slices; aqg_rangew_last returns both, and a caller who cares checks that one
 *         of them is 0.
 * AGGREGATES, folded by COMBINING ONLY -- nothing is subtracted back out, no prefix difference is taken; len_i = i - lo_i + 1:
 *   AQG_RANGEW_COUNT   AQG_UINT32        len_i (x may be NULL, t is ignored)
 *   AQG_RANGEW_SUM     aqg_long_type(t)  integers exact (128 bits); floating: a sum of exactly the window's rows in double, in a
 *                                        bracketing fixed by n and the positions: |got - exact| <= m u / (1 - m u) sum |x_j| over the
 *                                        window, m = len_i - 1, u = 2^-53 (the bound of ANY order of summation), while sum |x_j| < 2^1023
 *   AQG_RANGEW_AVG     AQG_DOUBLE        integers: the exact sum rounded to double, over len_i; floating: the SUM value over len_i
 *   AQG_RANGEW_MIN/MAX t                 an element of the window, bit for bit (which zero of -0.0 / +0.0 is unspecified)
 *   Non-finite rows act on exactly the windows that hold them: a NaN row gives NaN, +Inf and -Inf together NaN, one kind of Inf that
 *   Inf; every other window is unaffected (what sumw cannot promise, and a rolling add-and-remove gets wrong after a large value
 *   leaves).  MIN / MAX of a window that holds a NaN are unspecified.  Results are bit-reproducible from call to call; the column
 *   form and the grouped form need not agree bit for bit on floating sums.
 * x: the dtypes of aqg_scan; t (stamps): those of aqg_decay_from_times; anything else AQG_ERR_DTYPE.  AQG_ERR_ARG: out overlapping an
 * input, a handle not made by aqg_groupby_build, a bad op or frame, a NULL column with rows.  Every error returns with nothing
 * written; n == 0 or G == 0 is AQG_OK.  Asynchronous on the context's stream, no host round trip, scratch from the context workspace,
 * and the number of launches does not depend on n, G or the window lengths.
 *   aqg_rangew_bounds / aqg_grouped_rangew_bounds_flat   lo[i] = first position of row i's window, in the layout the stamps are in
 *   aqg_rangew_fold         out[i] = op over x[lo[i] .. i]; knows nothing of groups, the bounds carry them; lo[i] > i is clamped to i.
 *                           Public so that several aggregates over one frame share one search.
 *   aqg_rangew              bounds + fold of a column
 *   aqg_grouped_rangew      the same per group, stamps and values in ROW layout (brought into the flat layout in workspace)
 *   aqg_grouped_rangew_flat the same over columns already in the flat layout; out in the flat layout either way
 *   aqg_rangew_last         synchronises the stream; the geometry of the last fold -- *nlevels levels, level k in blocks of
 *                           block_rows[k] rows (8 words, 0 beyond the levels), the top level one block -- and the steps of the last
 *                           bounds pass                                                                                          */
enum { AQG_RANGEW_COUNT = 0, AQG_RANGEW_SUM = 1, AQG_RANGEW_AVG = 2, AQG_RANGEW_MIN = 3, AQG_RANGEW_MAX = 4 };
enum { AQG_RANGEW_OPEN = 0, AQG_RANGEW_CLOSED = 1 };
int aqg_rangew_out_dtype(int op, int t);
int aqg_rangew_bounds(aqg_ctx* ctx, int tt, const void* times, uint32_t n, double span, int frame, uint32_t* lo_out);
int aqg_grouped_rangew_bounds_flat(aqg_ctx* ctx, struct aqg_groupby* g, int tt, const void* times_flat, double span, int frame, uint32_t* lo_flat_out);
int aqg_rangew_fold(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, const uint32_t* lo, void* out);
int aqg_rangew(aqg_ctx* ctx, int op, int tt, const void* times, double span, int frame, int t, const void* x, uint32_t n, void* out);
int aqg_grouped_rangew(aqg_ctx* ctx, struct aqg_groupby* g, int op, int tt, const void* times_row, double span, int frame, int t, const void* x_row, void* out_flat);
int aqg_grouped_rangew_flat(aqg_ctx* ctx, struct aqg_groupby* g, int op, int tt, const void* times_flat, double span, int frame, int t, const void* xflat, void* out_flat);
int aqg_rangew_last(aqg_ctx* ctx, uint32_t* nlevels, uint32_t* block_rows /* [8] */, uint32_t* steps_up, uint32_t* steps_down);

/* ---- count distinct ----------------------------------------------------------
 * `count(distinct x)`: the generator emits `(x).distinct_size()` (common/types.py:271-277), under GROUP BY `(x[val]).distinct_size()`
 * inside the generated loop (engine/ast.py:749-784).  Replaces vector_type::distinct_size (server/vector_type.hpp:153-174) and
 * ColRef::distinct_size (server/table.h:328-332): a std::unordered_set<T> built per call there, per GROUP in the loop.
 * Result: the size of that set, a uint32_t -- equality by C++ ==, the rule of floating group-by keys above (probed against the
 * reference headers, tests/golden/ref_distinct.json): integers and BOOL by value; FLOAT / DOUBLE: -0.0 and +0.0 are one value and
 * every NaN ROW is a value of its own whatever its sign or payload, so the count is (distinct non-NaN values) + (NaN rows).
 * An empty slice counts 0.
 * Dtypes: INT8/16/32/64, UINT8/16/32/64, BOOL, FLOAT, DOUBLE; anything else (128-bit integers, dates, strings) returns
 * AQG_ERR_DTYPE with nothing written.
 *   aqg_count_distinct               the whole column -> *out_host.  n == 0: AQG_OK and 0.
 *   aqg_grouped_count_distinct       out_dev[g] for all G groups in group order, x in ROW layout (brought into the flat layout in
 *                                    workspace first, like aqg_grouped_median)
 *   aqg_grouped_count_distinct_flat  the same over a column already in the FLAT LAYOUT of the build
 * The grouped forms need a handle of aqg_groupby_build (as aqg_grouped_scan); a handle of aqg_groupby_agg: AQG_ERR_ARG; G == 0
 * returns AQG_OK.  The input is never modified.  One algorithm: a pass over tiles of the flat layout counts
 * every group that lies inside one tile; the groups that cross a tile edge leave (group, value) pairs, which a count-only
 * aqg_groupby_agg over the pair list folds.  The launches do not depend on the group count.  Asynchronous on the context's stream
 * except for ONE host round trip per call, the number of pairs (aqg_count_distinct's result rides along; it takes a second one
 * only when pairs were left).  The pair list
 * (worst case one pair per row: 4 + sizeof(T) bytes each) is kept by the context and only grows: no allocation in steady state;
 * when it cannot be had the call returns AQG_ERR_NOMEM with nothing written.
 * aqg_distinct_last (diagnostic, like aqg_select_last_routes), for the last call on this context: the tile size in rows (a constant,
 * valid before any call), how many groups crossed a tile edge, and the number of pairs they left.                              */
int aqg_count_distinct(aqg_ctx* ctx, int t, const void* x, uint32_t n, uint32_t* out_host);
int aqg_grouped_count_distinct(aqg_ctx* ctx, struct aqg_groupby* g, int t, const void* x, uint32_t* out_dev);
int aqg_grouped_count_distinct_flat(aqg_ctx* ctx, struct aqg_groupby* g, int t, const void* xflat, uint32_t* out_dev);
int aqg_distinct_last(aqg_ctx* ctx, uint32_t* tile_rows, uint32_t* crossing_groups, uint64_t* pairs);

/* ---- hash group-by -----------------------------------------------------------
 * Replaces AQHashTable (server/hasher.h:146-199) + set::hashtable_push
 * (server/unordered_dense.h:1117-1147) + HashTableFactory::get (:327-357).
 * Contract (the only executable one in the reference):
 *   group ids are dense, numbered by FIRST OCCURRENCE of the key tuple;
 *   ht_postproc row-id lists are DESCENDING row id within each group.
 * Up to 8 key columns; tuples of up to 8 bytes are packed into one word, wider ones compare through a representative row.       */
typedef struct aqg_groupby aqg_groupby;
int aqg_groupby_build(aqg_ctx* ctx, int nkeys, const int* key_dtypes, const void* const* keys,
                      uint32_t n, uint32_t max_groups_hint, aqg_groupby** out);
void aqg_groupby_destroy(aqg_groupby* g);
uint32_t aqg_groupby_ngroups(const aqg_groupby* g);
uint32_t aqg_groupby_nrows(const aqg_groupby* g);
/* device views owned by the handle (valid until destroy) */
const uint32_t* aqg_groupby_reversemap(const aqg_groupby* g); /* [n] group id of row      (hasher.h:149 reversemap) */
const uint32_t* aqg_groupby_counts(const aqg_groupby* g);     /* [G] rows per group       (ht_base before postproc) */
const uint32_t* aqg_groupby_first_rows(const aqg_groupby* g); /* [G] first row of group                            */
/* key column k of every group, in group order (AQHashTable::values()) */
int aqg_groupby_keys(aqg_groupby* g, int k, void* out_dev);
/* ht_postproc (hasher.h:181-198): offsets[G+1] (exclusive scan of counts; the
 * reference's ht_base after postproc is offsets[0..G)), row_ids[n] descending   */
int aqg_groupby_postproc(aqg_groupby* g, uint32_t* offsets_dev, uint32_t* row_ids_dev);

/* Key columns need not be plain integers (the reference hashes astring_view, date_t, time_t, timestamp_t and 128-bit integers too,
 * server/hasher.h:97-144, and groups by tuple ==): AQG_DATE (4-byte elements), AQG_TIME (8-byte elements, the 8th byte is padding
 * and ignored), AQG_TIMESTAMP (12-byte elements), AQG_INT128 / AQG_UINT128, and AQG_FLOAT / AQG_DOUBLE -- by value like the
 * reference's ==: 0.0 and -0.0 are one group, every NaN is a group of its own (probed against the reference headers,
 * tests/golden).  aqg_groupby_keys returns, for such a column, the caller's element at every group's first row (the column
 * must still be alive).  `const char*` keys are pointers in the reference (8-byte integers: pass AQG_UINT64); astring_view keys
 * compare string contents: aqg_str_encode turns the host strings into a uint32 code column (dense ids in first-occurrence order).  */
int aqg_str_encode(aqg_ctx* ctx, const char* const* strs_host, uint32_t n, uint32_t* codes_dev, uint32_t* ndistinct_host);
/* the same over a table sharded by row range (aqg_comm_* below): codes of ONE dictionary over all shards in GLOBAL first-occurrence order,
 * the uint32 key column aqg_groupby_agg_sharded takes -- every rank encodes its rows, the ranks all-gather their dictionaries' strings
 * (two small collectives), merge them in rank order and remap their code columns on the device                                        */
struct aqg_comm;
int aqg_str_encode_sharded(struct aqg_comm* comm, const char* const* strs_host, uint32_t n, uint32_t* codes_dev, uint32_t* ndistinct_global_host);
/* diagnostic of the last aqg_str_encode on this context (like aqg_join_last; the tests pin every route with it, the product does not
 * look at it): the route -- HOST: the host map (fewer than 2^16 rows, or AQG_STR_HOST); DEVICE: the device dictionary was accepted;
 * FALLBACK: the device dictionary was built, a row differed from its group's first row (two strings of one length under one 64-bit
 * hash) and the call was redone by the host map -- and *mismatch = 1 when the verify kernel saw such a row, else 0.  The local
 * encode inside aqg_str_encode_sharded is the last aqg_str_encode of that rank's context.  Both zero before any call, after an
 * argument error and after a call that failed.                                                                                      */
enum { AQG_STR_ROUTE_HOST = 1, AQG_STR_ROUTE_DEVICE = 2, AQG_STR_ROUTE_FALLBACK = 4 };
int aqg_str_encode_last(aqg_ctx* ctx, uint32_t* route, uint32_t* mismatch);

/* one aggregate over all groups in ONE pass over the value column: the device
 * form of the generated per-group loop `out[g] = op(col[vecs[g]])`
 * (engine/ast.py:722-789, mem_opt.cpp:50-65).  Output dtype as aqg_reduce.     */
int aqg_grouped_reduce(aqg_ctx* ctx, const aqg_groupby* g, int op, int t, const void* x, void* out_dev);

/* ---- per-group scans / windows / two-column aggregates: what the reference's own queries put inside the generated group loop -------
 * `SELECT sym, avgs(5, price) ... ASSUMING ASC time GROUP BY sym` (benchmark/quries/Aquery/q7.a), `mins(2, sales) ... group by Mont`
 * (tests/moving_avg.a:13), `max(ratios(x)) ... group by ID` (tests/q4.a:23), `pow(corr(v1, v2), 2) BY id2, id4`
 * (benchmark/h2o/groupby.sql:20) are emitted as  for g: out[g] = f(col[vecs[g]], ...)  (engine/ast.py:722-789); the frozen sample
 * mem_opt.cpp:53-63 writes vector results into ONE flat buffer sliced by the group offsets: `col[i].init_from(vecs[i].size, buf + offsets[i])`.
 * The FLAT LAYOUT of a build is that buffer's: position offsets[g] + i <-> element i of vecs[g] (ht_postproc order: DESCENDING row id
 * inside a group, hasher.h:192-196).  Every call below handles ALL groups in a number of launches that does not depend on the group count.
 *   aqg_groupby_offsets      device offsets[G+1] (exclusive scan of the group sizes; owned by the handle)
 *   aqg_grouped_flatten      out_flat[offsets[g] + i] = x[vecs[g][i]]: a column (1-, 2-, 4-, 8-byte elements) brought into the flat layout by
 *                            value-carrying radix passes over the group ids (no row lists, no gather)
 *   aqg_grouped_scan_flat    out_flat = the scan `op` (aqg_scan's ops, window w) of every group's slice of xflat, restarted at every
 *                            group start; result dtype aqg_scan_out_dtype.  Integer results are exact, as for aqg_scan.
 *   aqg_grouped_scan         flatten + scan_flat in one call (x in row layout)
 *   aqg_grouped_reduce_flat  out[g] = op(xflat[offsets[g] .. offsets[g+1])): reductions OF scan results (aqg_reduce's ops and dtypes)
 *   aqg_grouped_corr         out[g] = corr(x[vecs[g]], y[vecs[g]]) (aggregations.h:383-407: five 128-bit sums, the products in the C++ type
 *                            of the operands), x / y in ROW layout, integer columns of up to four bytes; doubles in out_dev[G]           */
const uint32_t* aqg_groupby_offsets(aqg_groupby* g);
int aqg_grouped_flatten(aqg_ctx* ctx, aqg_groupby* g, int t, const void* x, void* out_flat);
int aqg_grouped_scan_flat(aqg_ctx* ctx, aqg_groupby* g, int op, int t, const void* xflat, uint32_t w, void* out_flat);
int aqg_grouped_scan(aqg_ctx* ctx, aqg_groupby* g, int op, int t, const void* x, uint32_t w, void* out_flat);
int aqg_grouped_reduce_flat(aqg_ctx* ctx, aqg_groupby* g, int op, int t, const void* xflat, void* out_dev);
int aqg_grouped_corr(aqg_ctx* ctx, aqg_groupby* g, int tx, const void* x, int ty, const void* y, double* out_dev);
/* `x[val] OP agg(x[val])` of the generated loop (`price - min(price)`, `price / first(price)` under GROUP BY) for all groups in ONE launch:
 * out[i] = v[i] OP s[gid(i)]  (kind AQG_VEC_SCALAR)   or   s[gid(i)] OP v[i]  (kind AQG_SCALAR_VEC)
 * v, out: n = aqg_groupby_nrows(g) elements in ROW layout (gid = the build's reversemap) or in the FLAT layout
 * (gid = group index of the flat position); s: DEVICE column of G elements of dtype st, one per group.
 * Every group's slice of `out` equals, bit for bit, aqg_ewise over that group's slice of v with the host scalar s[g]: the same compute
 * type, operators (aqg_ewise's ops), division rules and result conversion, every result dtype aqg_ewise accepts.  vt / st: numeric or
 * bool (128-bit operands: AQG_ERR_DTYPE); a handle of aqg_groupby_agg or kind AQG_VEC_VEC: AQG_ERR_ARG; G == 0: AQG_OK, nothing written.
 * AQG_LAYOUT_FLAT: the first such call through a handle makes the group index of every flat position (n * 4 bytes kept by the handle, one
 * segmented pass) and, like the grouped scans, resets the context's workspace for it; later calls launch the one kernel only. */
enum { AQG_LAYOUT_ROW = 0, AQG_LAYOUT_FLAT = 1 };
int aqg_grouped_ewise(aqg_ctx* ctx, aqg_groupby* g, int layout, int op, int kind,
                      int vt, const void* v, int st, const void* s_dev, int ot, void* out);

/* fused single-pass group-by + aggregates (h2o Q1..Q5 shape): reads each key and value
 * column exactly once.  Group order = first occurrence, as aqg_groupby_build.  Result j
 * (aqg_groupby_agg_result) has ngroups elements of aqg_reduce_out_dtype(ops[j], val_dtypes[j])
 * and lives in the handle, like keys / first_rows (and counts when an op needs them); no
 * reversemap / postproc on such a handle.  ops: SUM MIN MAX COUNT AVG VAR STDDEV.
 * `*out` is in/out: pass NULL to create a handle, or an earlier handle to reuse its buffers
 * (steady-state calls then allocate nothing).  max_groups_hint sizes the hash tables
 * (0 = unknown: start small and grow); the call retries internally when the hint is too low.
 * Floating-point SUM / AVG / VAR accumulate with atomic adds (LDS and HBM), in whatever order the hardware schedules the rows:
 * results are NOT bit-reproducible from run to run (the reference adds the rows of a group in one fixed order); every result lies
 * within (n_g - 1) 2^-53 sum|x| of the exactly rounded sum of its group (n_g rows), which is what the parity tests assert.
 * Integer aggregates, counts, MIN / MAX, keys, first rows and the group order are exact and deterministic.
 * MIN / MAX of floating columns start from the reference's seeds, as in aqg_reduce: MAX from numeric_limits<T>::min() (a group of negative
 * rows gives the smallest positive normal value), MIN from max() (a group whose rows are all +Inf gives the largest finite value); the same holds
 * for aqg_grouped_reduce.  VAR / STDDEV of a uint16 column add the int squares sign-extended to the unsigned 128-bit sum, as the reference does.
 * On return the handle's ngroups is final; the device columns behind the handle (keys, first rows,
 * counts, results) may still be being written by kernels queued on the context's stream: read
 * them through this library (aqg_groupby_keys, aqg_d2h, ...: all ordered behind those kernels),
 * from the same stream, or after aqg_sync.                                                       */
int aqg_groupby_agg(aqg_ctx* ctx, int nkeys, const int* key_dtypes, const void* const* keys,
                    int naggs, const int* ops, const int* val_dtypes, const void* const* vals,
                    uint32_t n, uint32_t max_groups_hint, aqg_groupby** out);
const void* aqg_groupby_agg_result(const aqg_groupby* g, int j);
/* diagnostic: which plan the last aqg_groupby_agg / aqg_groupby_build through this handle took; the tests pin every
 * plan with it, the product does not look at it                                                                                         */
enum { AQG_PLAN_FAST_LDS = 1, AQG_PLAN_SMALL_LDS = 2, AQG_PLAN_BIG_LDS = 4, AQG_PLAN_DENSE = 8, AQG_PLAN_PART_ONE = 16, AQG_PLAN_PART_TWO = 32,
       AQG_PLAN_PART_ROUND1 = 64, AQG_PLAN_PART_WIDE = 128, AQG_PLAN_SORTED_TAIL = 256, AQG_PLAN_HBM_TABLE = 512, AQG_PLAN_BUILD_PARTITIONED = 1024, AQG_PLAN_GID_PARTITION = 2048 /* aqg_grouped_reduce: rows partitioned on the dense group id */,
       AQG_PLAN_PACKED_VALUES = 4096 /* narrow value columns travelled inside the 4-byte key word of a two-level partition plan */,
       AQG_PLAN_RANGE_PARTITIONS = 8192 /* a dense 4-byte key domain: order-preserving range partitions, direct-indexed LDS accumulators */,
       AQG_PLAN_ROW_EMIT = 16384 /* every row turned out to be its own group: the result columns are written as a map of the input */,
       AQG_PLAN_PACKED_KEYS = 32768 /* the key columns of a wide tuple travelled packed into fewer dword planes (sampled ranges, every row verified) */,
       AQG_PLAN_BUILD_LOOKUP = 65536 /* aqg_groupby_build: row ids through a key -> group id look-up table (a dense key domain of up to 2^21 values) */ };
uint32_t aqg_groupby_plan(const aqg_groupby* g);

/* ---- hash join (new functionality; reference runs joins in MonetDB)
 * inner equi-join on one integer key: build on (build_keys, nb), probe with
 * (probe_keys, np).  Emits matching row-id pairs ordered by probe row, then by
 * build row ascending.  Two-call protocol: pass NULL outputs to get the count.  The count is exact in 64 bits (duplicate keys
 * pass 2^32 pairs at small inputs: 70,000 x 70,000 equal keys); aqg_join_pairs addresses its outputs with uint32 offsets and
 * returns AQG_ERR_OVERFLOW (with *m_host = the count, nothing written) beyond AQG_MAX_ROWS pairs.                          */
int aqg_join_count(aqg_ctx* ctx, int t, const void* build_keys, uint32_t nb,
                   const void* probe_keys, uint32_t np, uint64_t* m_host);
int aqg_join_pairs(aqg_ctx* ctx, int t, const void* build_keys, uint32_t nb,
                   const void* probe_keys, uint32_t np,
                   uint32_t* probe_rows_out, uint32_t* build_rows_out, uint64_t capacity, uint64_t* m_host);
/* unique-build-key lookup join fused with nothing: idx[i] = build row whose key
 * equals probe_keys[i], or 0xFFFFFFFF                                            */
int aqg_join_lookup(aqg_ctx* ctx, int t, const void* build_keys, uint32_t nb,
                    const void* probe_keys, uint32_t np, uint32_t* build_row_of_probe);

/* ---- joins on composite and typed keys: inner, left outer, semi, anti (the contract: tests/join_keys_model.py)
 * A key is a tuple of 1..8 columns; ONE dtype list serves both sides (column k of the build side and of the probe side have
 * key_dtypes[k]).  Accepted: INT8/16/32/64, UINT8/16/32/64, BOOL, FLOAT, DOUBLE, DATE, TIME, TIMESTAMP, INT128, UINT128 -- anything
 * else (AQG_STR included) returns AQG_ERR_DTYPE with nothing written; string keys join through codes: ONE aqg_str_encode call over
 * both tables' strings (build rows first, then probe rows), the two halves of the code column passed as UINT32.  A tuple that
 * normalises to more than eight integer columns (TIMESTAMP and 128-bit count two) returns AQG_ERR_ARG, as the group-by does.
 * Equality is the group-by's, column by column: integers and BOOL by value, DATE its 4 bytes, TIME its 7 field bytes (the padding
 * byte may differ between the sides), TIMESTAMP date plus time, 128-bit all 16 bytes, FLOAT / DOUBLE by C++ `==`: -0.0 equals
 * +0.0 and a NaN equals NOTHING -- a probe row with a NaN in any floating key matches no build row (it is unmatched under LEFT and
 * ANTI), a build row with one is in no pair.  No key value is reserved (the all-ones tuples are ordinary keys).
 * With c_i = the number of build rows equal to probe row i:
 *   INNER  every matching pair, by probe row, then by ascending build row (one integer key: identical to aqg_join_pairs); m = sum c_i
 *   LEFT   as INNER, plus one pair (i, 0xFFFFFFFF) in probe-row order for every probe row with c_i == 0;          m = sum max(c_i, 1)
 *   SEMI   the probe rows with c_i > 0, ascending, each once; build_rows_out is neither read nor written and may be NULL
 *   ANTI   the probe rows with c_i == 0, ascending; build_rows_out as for SEMI
 * nb == 0: INNER and SEMI give 0, LEFT np pairs (i, 0xFFFFFFFF), ANTI all np rows; np == 0: 0 for every kind.
 * *m_host is exact in 64 bits.  aqg_join_keys_pairs with probe_rows_out == NULL only counts; beyond AQG_MAX_ROWS output rows, or
 * beyond `capacity`, it returns AQG_ERR_OVERFLOW with *m_host = the count and nothing written.
 * aqg_join_keys_lookup: the LOWEST build row whose tuple equals probe row i, else 0xFFFFFFFF; build keys need not be unique.  */
enum { AQG_JOIN_INNER = 0, AQG_JOIN_LEFT = 1, AQG_JOIN_SEMI = 2, AQG_JOIN_ANTI = 3 };
int aqg_join_keys_count(aqg_ctx* ctx, int kind, int nkeys, const int* key_dtypes,
                        const void* const* build_keys, uint32_t nb,
                        const void* const* probe_keys, uint32_t np, uint64_t* m_host);
int aqg_join_keys_pairs(aqg_ctx* ctx, int kind, int nkeys, const int* key_dtypes,
                        const void* const* build_keys, uint32_t nb,
                        const void* const* probe_keys, uint32_t np,
                        uint32_t* probe_rows_out, uint32_t* build_rows_out, uint64_t capacity, uint64_t* m_host);
int aqg_join_keys_lookup(aqg_ctx* ctx, int nkeys, const int* key_dtypes,
                         const void* const* build_keys, uint32_t nb,
                         const void* const* probe_keys, uint32_t np, uint32_t* build_row_of_probe);
/* diagnostics of the last aqg_join_keys_* call on this context (like aqg_select_last_routes): the tuple form (PACKED: at most 8
 * bytes, one 64-bit word; WIDE: compared column by column) and the table route (LDS: table and group keys copied into LDS; HBM:
 * read in place) of its probe, the distinct build tuples G and the slots of the table (the power of two >= 2G, at least 16).
 * All zero when the call ran no probe (an empty side, an argument error).  aqg_join_keys_lookup on ONE plain integer key runs the
 * probe of aqg_join_lookup, whose table is over the build rows: build_groups reads 0, table_slots the power of two >= 2 nb.      */
enum { AQG_JOIN_ROUTE_PACKED = 1, AQG_JOIN_ROUTE_WIDE = 2, AQG_JOIN_ROUTE_LDS = 4, AQG_JOIN_ROUTE_HBM = 8 };
int aqg_join_last(aqg_ctx* ctx, uint32_t* routes, uint32_t* build_groups, uint32_t* table_slots);
/* host, pure (like aqg_dtype_size): the first slot the kernels try for each of n tuples given as HOST columns, in a table of
 * `table_slots` (a power of two) slots -- lets a test build collision chains without knowing the hash */
int aqg_join_tuple_slots(int nkeys, const int* key_dtypes, const void* const* host_keys, uint32_t n, uint32_t table_slots,
                         uint32_t* slots_out_host);

/* ---- as-of join: the nearest earlier or later build row per key tuple (the contract: tests/asof_model.py)
 * For each probe row, the build row of the same key tuple whose `on` value is nearest at or before (BACKWARD) or at or after
 * (FORWARD) the probe row's: for each trade the last quote of its symbol.  The reference has no counterpart.
 * Equality keys: nkeys in 0..8; dtypes, tuple limits and equality exactly those of aqg_join_keys_* (-0.0 == +0.0, a NaN key equals
 * nothing, no reserved values, strings through one dictionary's codes).  nkeys == 0 is a pure as-of on `on`: key_dtypes and both key
 * lists may be NULL, every row is in one group and no hash probe runs.  Dtype and tuple-width errors return as they do from
 * aqg_join_keys_lookup, with nothing written.
 * `on`: one dtype for both sides, INT8/16/32/64, UINT8/16/32/64, FLOAT or DOUBLE; anything else (BOOL, 128-bit, DATE / TIME /
 * TIMESTAMP included) is AQG_ERR_DTYPE with nothing written.  Order is numeric; -0.0 == +0.0.  A probe row whose `on` is NaN has no
 * partner; a build row whose `on` is NaN is nobody's partner.
 * Result, with B(i) = the build rows whose key tuple equals probe row i's and whose `on` is not NaN:
 *   BACKWARD  the row of B(i) with the largest `on` <= probe `on` (< under AQG_ASOF_STRICT); among rows of that `on` the HIGHEST row id
 *   FORWARD   the row of B(i) with the smallest `on` >= probe `on` (> under AQG_ASOF_STRICT); among rows of that `on` the LOWEST row id
 *   no such row: 0xFFFFFFFF (the missing-row marker of aqg_gather_fill)
 * -- the ties of kdb's `aj` and of pandas `merge_asof`.  Neither side needs to be sorted; a build side whose `on` is already
 * non-decreasing (NaNs, if any, last) is noticed and spared the sort on `on`.  nb == 0: all 0xFFFFFFFF; np == 0: nothing written,
 * AQG_OK.  `direction` or `flags` outside the enums, a NULL column with rows, an output overlapping an input: AQG_ERR_ARG; row
 * counts beyond AQG_MAX_ROWS likewise.  Returns after the stream has drained and the call's temporaries are released.
 * aqg_join_asof_last (diagnostic, like aqg_join_last): the routes of the last call on the context -- LDS / HBM: the search read the
 * ordered build side from LDS / in place; NOKEYS: no key columns, no hash probe; PRESORTED: the build side's `on` was in order --
 * the distinct build tuples (1 without key columns) and the digit passes the ordering step ran (aqg_sort_last_passes; 0 when
 * nothing was sorted).  All zero when no probe ran (an empty side, an argument error).                                              */
enum { AQG_ASOF_BACKWARD = 0, AQG_ASOF_FORWARD = 1 };
enum { AQG_ASOF_STRICT = 1 };                       /* flags */
int aqg_join_asof(aqg_ctx* ctx, int direction, int flags,
                  int nkeys, const int* key_dtypes,
                  const void* const* build_keys, const void* build_on, uint32_t nb,
                  const void* const* probe_keys, const void* probe_on, uint32_t np,
                  int on_dtype, uint32_t* build_row_of_probe);
enum { AQG_ASOF_ROUTE_LDS = 1, AQG_ASOF_ROUTE_HBM = 2, AQG_ASOF_ROUTE_NOKEYS = 4, AQG_ASOF_ROUTE_PRESORTED = 8 };
int aqg_join_asof_last(aqg_ctx* ctx, uint32_t* routes, uint32_t* build_groups, uint32_t* sort_passes);

/* ---- window join: an aggregate of the build rows in a time window per key tuple (the contract: tests/wj_model.py)
 * For each probe row, an aggregate over the build rows of the same key tuple whose `on` lies in an interval around the probe row's
 * own: for each trade the max bid, the average spread, the number of quotes of its symbol in the 5 s before it.  kdb's wj / wj1, an
 * interval join followed by an aggregate elsewhere; the other half of the time-range windows above, which stay inside one table.
 * The reference has no counterpart.
 * KEYS    equality, dtypes, tuple limits and nkeys == 0 exactly as for aqg_join_asof.
 * `on`    one dtype for both sides, those of aqg_join_asof; anything else AQG_ERR_DTYPE with nothing written.
 * WINDOW  with B(i) = the build rows whose key tuple equals probe row i's: build row j of B(i) is in the window of probe row i iff
 *         neither `on` is NaN and b_j == p_i, or b_j < p_i and p_i - b_j is within `before`, or b_j > p_i and b_j - p_i is within
 *         `after`.  Rows with the probe row's own stamp are therefore always inside.  Windows that do not hold the probe stamp
 *         (kdb's (t - 5; t - 1)) are out of scope.
 * DISTANCE  integer `on`: larger minus smaller in unsigned 64-bit arithmetic, never p +- span (nothing wraps at the ends of int64 /
 *         uint64).  Floating `on`: the one rounded subtraction in double (FLOAT widened first, exactly), which is monotone in b_j.
 *         -0.0 == +0.0.
 * WITHIN  a closed side: d <= span, and span >= 0; an open side (AQG_WJ_OPEN_LO for `before`, AQG_WJ_OPEN_HI for `after`): d < span,
 *         and span > 0.  +Inf is allowed.  NaN, a negative span or unknown flag bits: AQG_ERR_ARG.  For integer `on` each span becomes
 *         ONE exact limit dmax = floor(span) (closed) or ceil(span) - 1 (open), saturated at 2^64 - 1, as for the time-range windows.
 * AQG_WJ_PREVAILING (kdb wj, as against wj1): the window additionally holds the one row of B(i) directly in front of it in
 *         (`on`, row) order -- the as-of BACKWARD partner of the window's start, on ties the highest row id -- even when the window
 *         is otherwise empty; never for a NaN probe stamp or an absent key.
 * ORDER   inside a window: ascending (`on`, row id).  It matters for the bracketing of floating sums and for PREVAILING only.
 * AGGREGATES  the AQG_RANGEW_* enums with the result dtype of aqg_rangew_out_dtype, folded by COMBINING ONLY as above: integer sums
 *         exact in 128 bits; floating sums a sum of exactly the window's rows with |got - exact| <= m u / (1 - m u) sum |x_j|,
 *         m = len - 1, u = 2^-53; MIN / MAX an element of the window bit for bit; non-finite rows act on exactly the windows that hold
 *         them; results are bit-reproducible from call to call.
 * EMPTY   an empty window: COUNT 0 and SUM 0; AVG / MIN / MAX write *fill_host, an element of the output dtype (NULL: zero bytes --
 *         the convention of aqg_gather_fill).  nb == 0: every window is empty.  np == 0: nothing written, AQG_OK.
 * AQG_ERR_ARG: an output overlapping an input, a NULL column with rows, more than AQG_MAX_ROWS rows; every error returns with nothing
 * written.
 *   aqg_join_window_bounds  order_out[nb] = the build rows by (group, `on`, row); window i is the positions [lo_i, hi_i) of that order,
 *                           lo_i == hi_i: empty.  Public so that several aggregates and several value columns share one ordering and
 *                           one search: a value column materialises with aqg_gather(x, order_out).  First / last of a window are
 *                           aqg_gather_fill over order[lo] / order[hi - 1] and stay with the caller.  Returns after the stream has
 *                           drained.
 *   aqg_interval_fold       out[i] = op over x[lo[i] .. min(hi[i], n)) for m queries over a column of n rows in any layout; it knows
 *                           nothing of joins, stamps or groups; lo[i] >= hi[i] is the empty interval.  x: the dtypes of
 *                           aqg_rangew_fold.  Asynchronous on the context's stream, scratch from the context workspace, and the
 *                           number of launches does not depend on n or m.
 *   aqg_join_window         bounds + aqg_gather of build_x + fold; returns after the stream has drained, like aqg_join_asof.
 *   aqg_join_window_last    (diagnostic, like aqg_join_asof_last) the AQG_ASOF_ROUTE_* bits of the last call's search, with
 *                           AQG_WJ_FOLD_STAGED (the fold copied the column and its level 1 into LDS) or AQG_WJ_FOLD_INPLACE (it read
 *                           them in place) for the fold; the distinct build tuples; the digit passes of the ordering step.  All zero
 *                           when nothing ran.                                                                                    */
enum { AQG_WJ_OPEN_LO = 1, AQG_WJ_OPEN_HI = 2, AQG_WJ_PREVAILING = 4 };   /* flags */
int aqg_join_window_bounds(aqg_ctx* ctx, int flags, int nkeys, const int* key_dtypes,
                           const void* const* build_keys, const void* build_on, uint32_t nb,
                           const void* const* probe_keys, const void* probe_on, uint32_t np,
                           int on_dtype, double before, double after,
                           uint32_t* order_out /* [nb] */, uint32_t* lo_out /* [np] */, uint32_t* hi_out /* [np] */);
int aqg_interval_fold(aqg_ctx* ctx, int op, int t, const void* x, uint32_t n, const uint32_t* lo, const uint32_t* hi, uint32_t m,
                      const void* fill_host, void* out /* [m] */);
int aqg_join_window(aqg_ctx* ctx, int op, int flags, int nkeys, const int* key_dtypes,
                    const void* const* build_keys, const void* build_on, uint32_t nb,
                    const void* const* probe_keys, const void* probe_on, uint32_t np,
                    int on_dtype, double before, double after, int t, const void* build_x, const void* fill_host, void* out /* [np] */);
enum { AQG_WJ_FOLD_STAGED = 16, AQG_WJ_FOLD_INPLACE = 32 };
int aqg_join_window_last(aqg_ctx* ctx, uint32_t* routes, uint32_t* build_groups, uint32_t* sort_passes);

/* ---- the exchange step of row-sharded group-bys -------------------------------------------------
 * Tables shard by row range, one process per GPU; every shard groups its own rows and the shards' group tables are merged
 * by ONE all_gather (RCCL) of a fixed-size payload followed by a re-aggregation.  Because shards are contiguous row
 * ranges gathered in rank order, first occurrence in the concatenation is the global first occurrence.
 *   aqg_groupby_pack          writes the payload of this shard: (gmax + 1) int64 pairs -- {ngroups, 0} then per group
 *                             {key, low 64 bits of aggregate `agg_index`} (one key column; integer SUM / COUNT / MIN / MAX)
 *   aqg_groupby_merge_packed  takes the `world` gathered payloads (rank order, (gmax + 1) * 2 int64 each) and returns the
 *                             merged group-by: keys of `key_dtype`, one aggregate combined with `op` (COUNT -> SUM of counts),
 *                             result dtype as for an AQG_INT64 value column
 * (the generated code of the reference has no distributed form; this replaces nothing there)                       */
int aqg_groupby_pack(aqg_groupby* g, int agg_index, uint32_t gmax, int64_t* out_dev);
int aqg_groupby_merge_packed(aqg_ctx* ctx, const int64_t* gathered_dev, uint32_t world, uint32_t gmax, int key_dtype, int op,
                             aqg_groupby** out);

/* ---- the exchange inside the library: communicators and the sharded group-by ----------------------------------------
 * One communicator per (process, GPU).  aqg_comm_init_rccl: RCCL -- rank 0 makes an id with aqg_comm_unique_id (ncclGetUniqueId),
 * the host ships its AQG_COMM_ID_BYTES bytes to the other ranks by any side channel (file, socket, torch.distributed, MPI) and
 * every rank calls aqg_comm_init_rccl (ncclCommInitRank on the context's device); the all-gather is ncclAllGather on the
 * context's stream, over xGMI inside a node.  librccl is opened on first use (dlopen), single-GPU users never load it.
 * aqg_comm_init_custom: the caller supplies the all-gather (`bytes` bytes of every rank's device buffer `send_dev` into
 * `recv_dev`, rank order, ordered on `hip_stream` or complete on return; 0 = success) -- hosts with a transport of their own,
 * and the one-GPU rehearsals / tests of the sharded path.                                                                          */
typedef struct aqg_comm aqg_comm;
#define AQG_COMM_ID_BYTES 128
typedef int (*aqg_allgather_fn)(void* user, const void* send_dev, void* recv_dev, size_t bytes, void* hip_stream);
int aqg_comm_unique_id(void* id_out /* AQG_COMM_ID_BYTES, host */);
int aqg_comm_init_rccl(aqg_ctx* ctx, int rank, int world, const void* id, aqg_comm** out);
int aqg_comm_init_custom(aqg_ctx* ctx, int rank, int world, aqg_allgather_fn fn, void* user, aqg_comm** out);
void aqg_comm_destroy(aqg_comm* comm);
int aqg_comm_rank(const aqg_comm* comm);
int aqg_comm_world(const aqg_comm* comm);
/* aqg_groupby_agg over a table sharded by ROW RANGE: this rank holds rows [row_base, row_base + n) of every column.  Every rank
 * groups its own rows, ONE all-gather moves the shards' group tables (k key columns, the global first row and one partial per
 * aggregate: SUM -> sum, COUNT -> count, MIN / MAX -> itself, AVG -> sum and count, VAR / STDDEV -> sum, sum of squares and count;
 * a partial that needs 128 bits per shard -- sums of 8-byte integers, sums of squares -- as two 8-byte columns), every rank re-aggregates the concatenation
 * and gets the same merged result: keys / aggregates of all groups in GLOBAL first-occurrence order (shards are contiguous and
 * gathered in rank order, so first occurrence in the concatenation is the global one: server/hasher.h:176-198 semantics).
 * Integer sums are exact (128-bit results), AVG of integers is the exact sum over the count, as in the single-GPU call.
 * gmax: upper bound of a shard's group count (fixed-size payload, nothing but the one all-gather crosses the wire: h2o Q1 / Q4 /
 * config 4), or 0: the ranks first exchange their group counts (one 8-byte all-gather) and size the payload by the largest.
 * ops: SUM / COUNT / MIN / MAX / AVG / VAR / STDDEV over integer columns of 1 to 8 bytes and floating columns (VAR / STDDEV use the
 * reference's formula on the merged moments, bit-identical to the single-GPU call for integers; up to 8 distinct partials per call).
 * The result handle has no 32-bit first rows (aqg_groupby_first_rows returns NULL):
 * aqg_groupby_first_rows64 gives the global row id of every group's first row.  `*out` is in/out like aqg_groupby_agg.             */
int aqg_groupby_agg_sharded(aqg_comm* comm, int nkeys, const int* key_dtypes, const void* const* keys,
                            int naggs, const int* ops, const int* val_dtypes, const void* const* vals,
                            uint32_t n, uint64_t row_base, uint32_t max_groups_hint, uint32_t gmax, aqg_groupby** out);
const int64_t* aqg_groupby_first_rows64(const aqg_groupby* g);
/* The exchange alone, over a shard table the caller already has (any aqg_groupby_agg / aqg_join_groupby_sum handle whose first
 * `nparts` aggregates are decomposable partials): partial p combines with merge_ops[p] (SUM / MIN / MAX; counts and sums combine
 * with SUM).  128-bit integer sums travel as their low 64 bits (exact while a SHARD's sum fits 64 bits) and come back as the exact
 * 128-bit total; counts come back as 128-bit totals.  Result: keys, aqg_groupby_first_rows64 and aggregates 0 .. nparts-1 of the
 * merged table in global first-occurrence order, as aqg_groupby_agg_sharded.                                                      */
int aqg_groupby_exchange(aqg_comm* comm, aqg_groupby* local, int nparts, const int* merge_ops, uint64_t row_base, uint32_t gmax, aqg_groupby** out);

/* ---- reductions and scans of a column sharded by ROW RANGE ---------------------------------------------------------
 * This rank holds `n` rows (0 allowed) of a column whose shards, laid end to end in rank order, are the whole column.  Every call
 * makes ONE all-gather of a small record per rank -- raw moments, first / last row, the shard's last w rows -- and answers as the
 * single-GPU call over the whole column would (server/aggregations.h:19-32,71-86,332-407; :89-281,439-485):
 *   aqg_reduce_sharded   SUM / MIN / MAX / COUNT / AVG / VAR / STDDEV / FIRST / LAST; the same 16 bytes on every rank; integer results
 *                        bit-identical to aqg_reduce over the whole column, floating sums = the rank-order sum of the shards' sums
 *   aqg_corr_sharded     corr(x, y): the five 128-bit sums folded exactly (integer columns, as aqg_corr)
 *   aqg_scan_sharded     out = this rank's rows of aqg_scan over the whole column: sums / avgs resume from the earlier shards' exact
 *                        total and row count, mins / maxs from their min / max, windows and shifts take the last rows of the shards
 *                        before them (neighbour rows for deltas / prev / aggnext).  vars / stddevs are not offered.
 * A rank whose local part fails still joins the all-gather and EVERY rank returns its status.                                      */
int aqg_reduce_sharded(aqg_comm* comm, int op, int t, const void* x, uint32_t n, void* out_host16);
int aqg_corr_sharded(aqg_comm* comm, int tx, const void* x, int ty, const void* y, uint32_t n, double* out_host);
int aqg_scan_sharded(aqg_comm* comm, int op, int t, const void* x, uint32_t n, uint32_t w, void* out);

/* Fused star join + grouped sum (BASELINE config 4: `fact JOIN small(key, w) ON fact.fk = small.key`, then
 * `sum(fact.val * small.w) BY fact.gkey`): one pass over fk, gkey and val (12 B/row) instead of lookup -> gather ->
 * multiply -> group-by (44 B/row).  The reference emits this as SQL for MonetDB (engine/ast.py:874-1085) followed by
 * the generated group loop (engine/ast.py:722-789); `val * w` is the free operator* of table.h:866-876 (exact product in
 * GetLongType) and the sum is aggregations.h:62-70.  All five columns are 4-byte integers; the dimension side has at
 * most 4096 rows (it lives in LDS), unique keys (of duplicates the lowest row wins, as in aqg_join_lookup); fact rows
 * without a partner are dropped (inner join).  Result: a group-by handle whose keys / first rows are in first-occurrence
 * order among the JOINED rows and whose aqg_groupby_agg_result(h, 0) is the 128-bit sum per group.  At most 3072 groups,
 * counted among the joined rows (group keys of rows without a partner do not count), whatever max_groups_hint says: 0 or a hint
 * that turns out too small is grown up to 3072; more groups than that return AQG_ERR_ARG, and so does a hint above 3072 unless
 * the call has fewer rows than that (a hint is never taken to be larger than n).                                                  */
int aqg_join_groupby_sum(aqg_ctx* ctx, int key_dtype, const void* dim_keys, int dim_val_dtype, const void* dim_vals, uint32_t nb,
                         const void* fact_fk, int group_key_dtype, const void* group_keys, int val_dtype, const void* fact_vals,
                         uint32_t n, uint32_t max_groups_hint, aqg_groupby** out);

/* ---- synthetic h2o / time-series columns (bench + parity inputs) ---
 * Counter-based: row i of column `col` depends only on (seed, col, row_base+i),
 * so shards are reproducible independent of the GPU count.  The oracle carries
 * the same generator for the CPU side.                                          */
typedef enum aqg_gencol {
    AQG_GEN_ID1 = 0, AQG_GEN_ID2 = 1, AQG_GEN_ID3 = 2, AQG_GEN_ID4 = 3, AQG_GEN_ID5 = 4, AQG_GEN_ID6 = 5,
    AQG_GEN_V1 = 6, AQG_GEN_V2 = 7, AQG_GEN_V3 = 8, AQG_GEN_TIMESTAMP = 9, AQG_GEN_PRICE = 10
} aqg_gencol;
int aqg_gen_column(aqg_ctx* ctx, int col, uint64_t seed, uint64_t row_base, uint32_t n,
                   uint64_t n_total, uint32_t K, void* out_dev);

/* ---- HIP-event timing on the context's stream (bench.py roofline leg) ------ */
int aqg_timer_start(aqg_ctx* ctx);
int aqg_timer_stop_ms(aqg_ctx* ctx, float* ms_host);
/* duration of the DOMINANT kernel of the most recent call (group-by: the pass over the rows;
 * scans: the scan pass), bracketed by HIP events on the context's stream inside the library */
int aqg_last_kernel_ms(aqg_ctx* ctx, float* ms_host);

const char* aqg_version(void);

/* ---- test aids ---------------------------------------------------------------
 * The scratch-memory guard (DESIGN.md "Scratch memory"), on in a process started with AQG_WS_GUARD=<byte>: the workspace arena, the
 * pooled handle buffers and the library's own control words are filled with that byte before every use; every sub-allocation of the
 * arena is preceded by a 256-byte red zone (physical offset = logical offset + 256 * (index + 1)); the arena's logical capacity is
 * exactly the largest size a call has asked for, rounded up to 256.  At every reset of the arena, and on demand, the arena is copied
 * to the host: every byte outside the sub-allocations made since the last reset must still hold the byte, and the ranking bitmap
 * must be all zero.  The FIRST violation is latched in the context and stays.
 *   aqg_debug_ws_check  synchronises, runs the check and returns the latched report (kind AQG_WS_CLEAN: none).  AQG_ERR_ARG when the
 *                       switch is not set.
 *   aqg_debug_ws_info   the arena of the last use; with `allocs` != NULL the first max_allocs logged sub-allocations as
 *                       (physical offset, bytes) pairs of uint64.  Works without the switch too (no log then).                    */
enum { AQG_WS_CLEAN = 0, AQG_WS_ZONE = 1, AQG_WS_PADDING = 2, AQG_WS_TAIL = 3, AQG_WS_RANK_BM = 4 };
typedef struct aqg_ws_report {
    uint32_t kind;          /* AQG_WS_*: what the first damaged byte belongs to                                              */
    int32_t alloc_index;    /* the logged sub-allocation the byte follows, -1: none                                           */
    uint64_t offset;        /* physical offset of the byte in the arena (AQG_WS_RANK_BM: byte offset into the bitmap)          */
    uint64_t alloc_offset, alloc_bytes;   /* that sub-allocation                                                              */
    uint8_t expected, found;
    uint8_t pad_[6];
} aqg_ws_report;
typedef struct aqg_ws_info {
    void* base;             /* device address of the arena                                                                    */
    uint64_t physical_bytes, logical_bytes;
    void* rank_bm;          /* the ranking bitmap of the few-pass group-by (NULL: never allocated)                              */
    uint64_t rank_bm_bytes;
    uint32_t nallocs;       /* sub-allocations logged since the last reset                                                     */
    uint8_t guard, pattern;
    uint8_t pad_[2];
} aqg_ws_info;
int aqg_debug_ws_check(aqg_ctx* ctx, aqg_ws_report* out);
int aqg_debug_ws_info(aqg_ctx* ctx, aqg_ws_info* out, uint64_t* allocs, uint32_t max_allocs);

#ifdef __cplusplus
}
#endif
#endif /* AQG_H */
