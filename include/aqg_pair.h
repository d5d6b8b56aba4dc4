/* aqg_pair.h -- the pair windows of the C-ABI: moving and running statistics of two columns.
 * Part of aqg.h, which includes it where the scans are declared (inside its extern "C" block, behind aqg_ctx and aqg_groupby); include
 * aqg.h, not this file.  tests/test_pairwin_cabi.py holds these declarations to the library and to the scratch-guard calls of
 * tests/pairwin_scratch.py, as tests/test_cabi.py and tests/test_scratch_catalogue.py hold aqg.h's own. */
#ifndef AQG_PAIR_H
#define AQG_PAIR_H
#ifndef AQG_H
#error "include aqg.h: aqg_pair.h is a part of it"
#endif

/* ---- pair windows: moving and running statistics of two columns ------------------
 * pandas' rolling(w, min_periods=1).cov(ddof=0) / .corr(), expanding().cov / .corr, the rolling beta of one series against another --
 * for all groups in one call.  THE REFERENCE HAS NO SUCH FUNCTION; the contract is this comment, held by the
 * exact rational model tests/pair_moments.py.
 * Window: that of varw -- rows [i - w + 1, i], clamped at the start of the column or of the row's group; the running ops (*S) take the
 * group so far and ignore w.  Moments are POPULATION moments (divided by the window's length L), so covw(w, x, x) is varw(w, x):
 *   cov  = mean((x - mean x)(y - mean y))
 *   corr = cov / sqrt(var_x var_y), clamped to [-1, 1]; NaN where either computed variance is not positive
 *   beta = cov / var_x, the slope of y on x; NaN where the computed var_x is not positive
 * so the first row of every group and every constant window give NaN for corr and beta.  out[i] answers row i of the layout scanned, as
 * double; the grouped forms write the FLAT LAYOUT, like aqg_grouped_scan.
 * Accuracy (the variance scans' rule: no cancellation against anything wider than it must be): windows of up to 64 rows are two direct
 * passes about an anchor inside the window, |cov - exact| <= 1e-9 |exact| + 1e-12 Rx Ry with Rx, Ry the WINDOW's ranges; longer windows
 * are differences of prefix co-moments about the group's first row, with 1e-10 Rx Ry over the GROUP's ranges so far; the running ops
 * are those prefixes themselves, 1e-12 Rx Ry.  corr and beta inherit the three moments' bounds (tests/pair_moments.py).
 * Non-finite rows (the rule of aqg_scan's varw): outputs are specified for every row strictly before the first non-finite row of either
 * column in its group; behind it they are unspecified and the call still succeeds.  Windows of up to 64 rows are direct sums: there a
 * non-finite row acts on the windows that hold it and on no other.
 * Dtypes: tx and ty are each any of the ten numeric dtypes, independently; anything else: AQG_ERR_DTYPE.  AQG_ERR_ARG: w == 0 for a *W
 * op (any other w is accepted, however wide), an unknown op, a handle of aqg_groupby_agg, a NULL column with rows.  Every error
 * returns with nothing written; n == 0 or G == 0: AQG_OK, nothing written.
 *   aqg_scan2               the whole column
 *   aqg_grouped_scan2       every group's rows, x and y in ROW layout (both brought into the flat layout, then the flat form)
 *   aqg_grouped_scan2_flat  the same over columns already in the FLAT LAYOUT of the build
 * The inputs are never modified.  Asynchronous on the context's stream, workspace from the context's arena, one writer per output
 * element, no atomics, bit-reproducible from call to call, and a number of launches that does not depend on G.
 * aqg_scan2_last: the route the last call on this context took and the rows one workgroup of it owns -- a diagnostic for the tests. */
typedef enum aqg_scan2op { AQG_SCAN2_COVS = 0, AQG_SCAN2_CORRS = 1, AQG_SCAN2_BETAS = 2,      /* running: the group so far   */
                           AQG_SCAN2_COVW = 3, AQG_SCAN2_CORRW = 4, AQG_SCAN2_BETAW = 5 } aqg_scan2op;   /* last min(w, i+1) rows */
enum { AQG_SCAN2_ROUTE_REG = 1,      /* w <= 8: the window's differences in registers            */
       AQG_SCAN2_ROUTE_LDS = 2,      /* w <= 64: two passes over the window in LDS               */
       AQG_SCAN2_ROUTE_PREFIX = 4 }; /* longer windows and the running ops: prefix co-moments    */
int aqg_scan2(aqg_ctx* ctx, int op, int tx, const void* x, int ty, const void* y, uint32_t n, uint32_t w, double* out);
int aqg_grouped_scan2(aqg_ctx* ctx, struct aqg_groupby* g, int op, int tx, const void* x_row, int ty, const void* y_row, uint32_t w, double* out_flat);
int aqg_grouped_scan2_flat(aqg_ctx* ctx, struct aqg_groupby* g, int op, int tx, const void* xflat, int ty, const void* yflat, uint32_t w, double* out_flat);
int aqg_scan2_last(aqg_ctx* ctx, uint32_t* route, uint32_t* tile_rows);

#endif /* AQG_PAIR_H */
