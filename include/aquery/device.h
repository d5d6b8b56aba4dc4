// device.h -- host-side runtime that ties the header-level API (vector_type / ColRef / aggregations /
// hasher) to the C-ABI of the MI355X library (include/aqg.h).  Header-only; state lives in one
// process-wide Runtime (the reference's post-processor is single-caller: one engine thread,
// SURVEY 8b).
//
// Model: a column keeps the reference's 16-byte {container, size, capacity} triple.  Device residency
// is tracked out of band, keyed by the HOST address range of the buffer:
//   PINNED  a borrowed host column (capacity == 0: `ColRef<T>(len, server->getCol(i))`) uploaded on first
//           use and cached -- the reference's zero-copy view of the data source becomes a device mirror;
//           the host data is assumed immutable while the mirror exists (drop_pins() at session end).
//   RESULT  a column produced by a device kernel.  Its host buffer is allocated exactly as the reference
//           would (malloc / scratch arena) but filled lazily: the first host access (operator[], begin(),
//           out(), ...) downloads it AND DROPS THE DEVICE COPY -- vector_type hands out mutable host access
//           (operator[] returns _Ty&), so a mirror kept past that point could go stale behind a host write
//           (`auto x = a + b; x[0] = 5; auto y = x * c;`): a later device use uploads the host data again.
//           Chained expressions such as max(price - mins(price)) never touch the host and never leave HBM.
//           (A grouping's row-id buffer keeps its registration after a download: `col[vecs[g]]` is recognised through it.
//           Generated code only reads vecs[g]; its device copy and the per-grouping aggregate cache assume that, like PINNED.)
// There is no CPU fallback: without the library or a GPU every operation aborts with a message.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <map>
#include <utility>
#include <vector>

#include "../aqg.h"

namespace aq {
namespace dev {

[[noreturn]] inline void die(const char* what, int rc, aqg_ctx* ctx) {
    std::fprintf(stderr, "[aquery-mi355x] %s failed (status %d): %s\n", what, rc, ctx ? aqg_last_error(ctx) : "no context");
    std::abort();
}

// A column that exists (or can be made) for ALL groups of one grouping at once -- what a per-group temporary of the generated loop
// (`col[vecs[g]]`, `avgw(5, col[vecs[g]])`, `a[vecs[g]] - mins(a[vecs[g]])`, engine/ast.py:749-784) is a slice of.
//   layout ROW   n elements in row order: a source column, or an element-wise result of row-order columns
//                (gather commutes with element-wise operators: f(a[val], b[val]) = f(a, b)[val])
//   layout FLAT  n elements in the flat layout of the grouping: position offsets[g] + i <-> row vecs[g][i]; what the per-group scans
//                produce (aqg_grouped_scan_flat) and what the generated code's `buf + offsets[g]` output buffers are laid out as
struct VCol {
    int layout = 0, tag = 0;
    void* dptr = nullptr;                                    // computed columns: owned device column of n elements
    const void* src = nullptr; size_t src_bytes = 0; bool src_borrowed = false;   // source columns: host address, resolved at every use
    void* flat = nullptr;                                    // ROW columns: their flat form (aqg_grouped_flatten), made when first scanned
    std::vector<unsigned char> host; bool host_valid = false;   // host copy of the FLAT form, downloaded once, serves every group's slice
};

// One device group-by (the table behind HashTableFactory::get / AQHashTable).  Its row-id buffer is registered like any
// other RESULT; `vecs[g]` views into it let the runtime recognise `col[vecs[g]]` as "group g of this grouping".
struct GroupCtx {
    aqg_groupby* handle = nullptr;
    uint32_t n = 0, G = 0;
    uint32_t* offsets = nullptr;   // [G+1] host
    uint32_t* counts = nullptr;    // [G]   host
    uint32_t* row_ids = nullptr;   // [n]   host address (device copy registered)
    std::vector<VCol> vcols;
    std::map<std::array<uint64_t, 6>, int> memo;             // (kind, op, operand columns, window / scalar bits) -> column, made once for all groups
    // element-wise (column OP scalar).  The first group's scalar makes a constant-scalar column; once a later group's scalar differs the
    // use `varies`, and either the scalar's source was found among the cached per-group aggregates (`gvcol`: the column made by
    // aqg_grouped_ewise from `scol`, the G scalars it was computed with) or every later group takes the per-group path
    struct ScalarUse { uint64_t bits[2]; int vcol; bool varies; uint32_t g0; int gvcol; std::vector<unsigned char> scol; };
    std::map<std::array<uint64_t, 4>, ScalarUse> smemo;
    // (column, op) -> G result slots of 16 bytes, filled for ALL groups by one kernel on first request
    std::map<std::pair<int, int>, std::vector<unsigned char>> cache;
    std::map<std::pair<int, int>, std::vector<double>> corr_cache;
    // (column, order, k) -> the G x k values of maxk / mink, filled for ALL groups by one aqg_grouped_topk on first request
    std::map<std::array<uint32_t, 3>, std::vector<unsigned char>> topk_cache;
    // (column, which, den, the num list) -> the G x nq values of quantile / quantiles, filled for ALL groups by one aqg_grouped_quantiles
    std::map<std::vector<uint32_t>, std::vector<unsigned char>> quant_cache;
};

struct Entry {
    void* dptr = nullptr;
    size_t bytes = 0;
    bool host_stale = false;   // RESULT not yet downloaded
    bool pinned = false;       // PINNED borrowed column
    GroupCtx* gctx = nullptr;  // set on a grouping's row-id buffer
    // DEFERRED per-group temporary: group `dg`'s slice of column `dv` of grouping `dgroup`; nothing per group has run.  Reductions,
    // scans and element-wise operators on it are answered for all groups at once; anything else materialises the slice first
    bool deferred = false;
    GroupCtx* dgroup = nullptr;
    uint32_t dg = 0;
    int dv = -1;
};

class Runtime {
public:
    static Runtime& get() {
        static Runtime r;
        return r;
    }
    aqg_ctx* ctx() {
        if (!ctx_) {
            int dev = 0;
            if (const char* e = std::getenv("AQ_GPU_DEVICE")) dev = std::atoi(e);
            int rc = aqg_ctx_create(dev, nullptr, &ctx_);
            if (rc != AQG_OK) die("aqg_ctx_create (no MI355X visible; this library has no CPU fallback)", rc, nullptr);
        }
        return ctx_;
    }
    size_t stale = 0;   // number of entries whose host copy is stale (fast path test in operator[])

    // containing entry of a host address, or end()
    std::map<uintptr_t, Entry>::iterator find(const void* p) {
        if (map_.empty()) return map_.end();
        auto it = map_.upper_bound((uintptr_t)p);
        if (it == map_.begin()) return map_.end();
        --it;
        if ((uintptr_t)p < it->first + it->second.bytes || ((uintptr_t)p == it->first && it->second.bytes == 0)) return it;
        return map_.end();
    }
    bool end(std::map<uintptr_t, Entry>::iterator it) { return it == map_.end(); }

    // device address of `bytes` bytes of host data at p.  borrowed != 0: cache the upload (PINNED).
    // `temp_out` receives a temporary device buffer the caller must release() when the data was not cacheable.
    const void* input(const void* p, size_t bytes, bool borrowed, void** temp_out) {
        *temp_out = nullptr;
        if (bytes == 0) return nullptr;
        auto it = find(p);
        if (it != map_.end() && it->second.deferred) materialize(it);
        if (it != map_.end() && it->second.gctx && !it->second.dptr) fill_rows(it->second);
        if (it != map_.end() && (uintptr_t)p + bytes <= it->first + it->second.bytes)
            return static_cast<char*>(it->second.dptr) + ((uintptr_t)p - it->first);
        void* d = nullptr;
        int rc = aqg_malloc(ctx(), bytes, &d);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        rc = aqg_h2d(ctx_, d, p, bytes);
        if (rc != AQG_OK) die("aqg_h2d", rc, ctx_);
        if (borrowed) {
            Entry e; e.dptr = d; e.bytes = bytes; e.pinned = true;
            map_[(uintptr_t)p] = e;
        } else *temp_out = d;
        return d;
    }
    void release(void* temp) { if (temp) aqg_free(ctx(), temp); }
    // register a host buffer whose device copy already exists (ownership of dptr moves to the registry)
    void adopt(void* p, size_t bytes, void* dptr, bool host_valid) {
        forget_range(p, bytes);
        Entry e; e.dptr = dptr; e.bytes = bytes; e.host_stale = !host_valid;
        map_[(uintptr_t)p] = e;
        if (!host_valid) ++stale;
    }

    // register a fresh RESULT buffer for the host range [p, p+bytes); returns its device address
    void* result(void* p, size_t bytes) {
        forget_range(p, bytes);
        void* d = nullptr;
        int rc = aqg_malloc(ctx(), bytes ? bytes : 16, &d);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        Entry e; e.dptr = d; e.bytes = bytes; e.host_stale = true;
        map_[(uintptr_t)p] = e;
        ++stale;
        return d;
    }
    // ---- grouped fast path ------------------------------------------------------------------------------------
    // The row-id lists of a grouping (aqg_groupby_postproc: a radix pass over the group-id column, 4.7 ms per 1e9 rows) are made
    // the first time somebody needs them on the device or on the host.  `col[vecs[g]]` followed by a reduction -- the shape the
    // code generator emits -- never does: it is answered by aqg_grouped_reduce from the group-id column of the build.
    void adopt_group(GroupCtx* g, void* drows) {
        adopt(g->row_ids, (size_t)g->n * 4, drows, /*host_valid=*/false);
        auto it = map_.find((uintptr_t)g->row_ids);
        if (it != map_.end()) it->second.gctx = g;
    }
    void fill_rows(Entry& e) {
        GroupCtx* c = e.gctx;
        void *doff = nullptr, *drows = nullptr;
        int rc = aqg_malloc(ctx(), ((size_t)c->G + 1) * 4, &doff);
        if (rc == AQG_OK) rc = aqg_malloc(ctx_, ((size_t)c->n + 1) * 4, &drows);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        rc = aqg_groupby_postproc(c->handle, static_cast<uint32_t*>(doff), static_cast<uint32_t*>(drows));
        if (rc != AQG_OK) die("aqg_groupby_postproc", rc, ctx_);
        aqg_free(ctx_, doff);
        e.dptr = drows;
    }
    // is [idx, idx+count) exactly the row list of one group of a registered grouping?
    bool group_of(const uint32_t* idx, uint32_t count, GroupCtx** gc, uint32_t* g) {
        auto it = find(idx);
        if (it == map_.end() || !it->second.gctx) return false;
        GroupCtx* c = it->second.gctx;
        uint32_t off = (uint32_t)(idx - c->row_ids);
        uint32_t lo = 0, hi = c->G;                       // largest g with offsets[g] <= off
        while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (c->offsets[mid] <= off) lo = mid; else hi = mid; }
        if (c->G == 0 || c->offsets[lo] != off || c->counts[lo] != count) return false;
        *gc = c; *g = lo;
        return true;
    }
    // ---- columns of a grouping (VCol) ----------------------------------------------------------------------------------------------
    static size_t esz(int tag) { return aqg_dtype_size(tag); }
    int vcol_new(GroupCtx* c, const std::array<uint64_t, 6>& key, const VCol& v) {
        c->vcols.push_back(v);
        const int id = (int)c->vcols.size() - 1;
        c->memo[key] = id;
        return id;
    }
    // the source column behind `col[vecs[g]]`
    int vcol_source(GroupCtx* c, const void* src, size_t src_bytes, bool borrowed, int tag) {
        const std::array<uint64_t, 6> key{0, (uint64_t)(uintptr_t)src, (uint64_t)tag, 0, 0, 0};
        auto it = c->memo.find(key);
        if (it != c->memo.end()) return it->second;
        VCol v; v.layout = 0; v.tag = tag; v.src = src; v.src_bytes = src_bytes; v.src_borrowed = borrowed;
        return vcol_new(c, key, v);
    }
    // device address of a ROW column (`*tmp` must be release()d by the caller)
    const void* vcol_row_ptr(GroupCtx* c, int v, void** tmp) {
        *tmp = nullptr;
        VCol& col = c->vcols[v];
        if (col.dptr) return col.dptr;
        return input(col.src, col.src_bytes, col.src_borrowed, tmp);
    }
    // device address of the FLAT form of a column (a ROW column is flattened once: value-carrying radix passes, no row lists)
    const void* vcol_flat_ptr(GroupCtx* c, int v) {
        if (c->vcols[v].layout == 1) return c->vcols[v].dptr;
        if (!c->vcols[v].flat) {
            void* tmp = nullptr;
            const void* d = vcol_row_ptr(c, v, &tmp);
            void* f = nullptr;
            int rc = aqg_malloc(ctx(), (size_t)c->n * esz(c->vcols[v].tag) + 16, &f);
            if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
            rc = aqg_grouped_flatten(ctx_, c->handle, c->vcols[v].tag, d, f);
            if (rc != AQG_OK) die("aqg_grouped_flatten", rc, ctx_);
            release(tmp);
            c->vcols[v].flat = f;
        }
        return c->vcols[v].flat;
    }
    // scan(op, w) of every group's slice: one segmented scan over the flat column
    int vcol_scan(GroupCtx* c, int v, int op, uint32_t w) {
        const std::array<uint64_t, 6> key{1, (uint64_t)op, (uint64_t)v, w, 0, 0};
        auto it = c->memo.find(key);
        if (it != c->memo.end()) return it->second;
        VCol r; r.layout = 1; r.tag = aqg_scan_out_dtype(op, c->vcols[v].tag);
        const void* xf = vcol_flat_ptr(c, v);
        int rc = aqg_malloc(ctx(), (size_t)c->n * esz(r.tag) + 16, &r.dptr);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        rc = aqg_grouped_scan_flat(ctx_, c->handle, op, c->vcols[v].tag, xf, w, r.dptr);
        if (rc != AQG_OK) die("aqg_grouped_scan_flat", rc, ctx_);
        return vcol_new(c, key, r);
    }
    // quantile num / den (which: AQG_SEL_LOWER / UPPER) of the window of w rows that ends at every row of every group's slice (medianw /
    // quantilew of a per-group temporary): ONE aqg_grouped_window_quantiles_flat over the flat column, whatever the number of groups
    size_t grouped_window_quantile_calls = 0;   // aqg_grouped_window_quantiles_flat calls made so far (the tests count them)
    int vcol_window_quantile(GroupCtx* c, int v, uint32_t w, int which, uint32_t num, uint32_t den) {
        const std::array<uint64_t, 6> key{4, (uint64_t)which, (uint64_t)v, w, num, den};
        auto it = c->memo.find(key);
        if (it != c->memo.end()) return it->second;
        VCol r; r.layout = 1; r.tag = c->vcols[v].tag;
        const void* xf = vcol_flat_ptr(c, v);
        int rc = aqg_malloc(ctx(), (size_t)c->n * esz(r.tag) + 16, &r.dptr);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        ++grouped_window_quantile_calls;
        rc = aqg_grouped_window_quantiles_flat(ctx_, c->handle, which, 1, &num, den, r.tag, xf, w, r.dptr);
        if (rc != AQG_OK) die("aqg_grouped_window_quantiles_flat", rc, ctx_);
        return vcol_new(c, key, r);
    }
    // ema / ewma of every group's slice (mode: AQG_EMA_RECURSIVE / AQG_EMA_ADJUSTED): ONE aqg_grouped_ema_flat over the flat column, whatever
    // the number of groups.  vdecay < 0: the constant alpha; else the decay column `vdecay` of the SAME grouping (alpha is then ignored and
    // left out of the key).
    size_t grouped_ema_calls = 0;               // aqg_grouped_ema_flat calls made so far (the tests count them)
    int vcol_ema(GroupCtx* c, int v, int mode, double alpha, int vdecay) {
        uint64_t abits = 0;
        if (vdecay < 0) std::memcpy(&abits, &alpha, 8);
        const std::array<uint64_t, 6> key{5, (uint64_t)mode, (uint64_t)v, abits, (uint64_t)(vdecay + 1), 0};
        auto it = c->memo.find(key);
        if (it != c->memo.end()) return it->second;
        VCol r; r.layout = 1; r.tag = AQG_DOUBLE;
        const void* xf = vcol_flat_ptr(c, v);
        const void* df = vdecay < 0 ? nullptr : vcol_flat_ptr(c, vdecay);
        int rc = aqg_malloc(ctx(), (size_t)c->n * 8 + 16, &r.dptr);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        ++grouped_ema_calls;
        rc = aqg_grouped_ema_flat(ctx_, c->handle, mode, c->vcols[v].tag, xf, alpha, static_cast<const double*>(df), static_cast<double*>(r.dptr));
        if (rc != AQG_OK) die("aqg_grouped_ema_flat", rc, ctx_);
        return vcol_new(c, key, r);
    }
    // the rank (method: AQG_RANK_*, order: AQG_ORDER_ASC / DESC, k: NTILE's buckets) of every row of every group's slice: ONE
    // aqg_grouped_rank_flat over the flat column per (column, method, order, k), whatever the number of groups
    size_t grouped_rank_calls = 0;              // aqg_grouped_rank_flat calls made so far (the tests count them)
    int vcol_rank(GroupCtx* c, int v, int method, int order, uint32_t k) {
        const std::array<uint64_t, 6> key{9, (uint64_t)method, (uint64_t)v, (uint64_t)order, method == AQG_RANK_NTILE ? k : 0u, 0};
        auto it = c->memo.find(key);
        if (it != c->memo.end()) return it->second;
        VCol r; r.layout = 1; r.tag = aqg_rank_out_dtype(method);
        const void* xf = vcol_flat_ptr(c, v);
        int rc = aqg_malloc(ctx(), (size_t)c->n * esz(r.tag) + 16, &r.dptr);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        ++grouped_rank_calls;
        rc = aqg_grouped_rank_flat(ctx_, c->handle, method, order, k, c->vcols[v].tag, xf, r.dptr);
        if (rc != AQG_OK) die("aqg_grouped_rank_flat", rc, ctx_);
        return vcol_new(c, key, r);
    }
    // the pair statistic op (AQG_SCAN2_*: covw / corrw / betaw over w rows, or the running covs / corrs / betas) of the columns vx, vy of
    // every group's slice: ONE aqg_grouped_scan2_flat over the two flat columns per (op, vx, vy, w), whatever the number of groups (the
    // running ops ignore w, which is left out of their key)
    size_t grouped_scan2_calls = 0;             // aqg_grouped_scan2_flat calls made so far (the tests count them)
    int vcol_scan2(GroupCtx* c, int op, int vx, int vy, uint32_t w) {
        const std::array<uint64_t, 6> key{10, (uint64_t)op, (uint64_t)vx, (uint64_t)vy, op >= AQG_SCAN2_COVW ? w : 0u, 0};
        auto it = c->memo.find(key);
        if (it != c->memo.end()) return it->second;
        VCol r; r.layout = 1; r.tag = AQG_DOUBLE;
        const void* xf = vcol_flat_ptr(c, vx);
        const void* yf = vcol_flat_ptr(c, vy);
        int rc = aqg_malloc(ctx(), (size_t)c->n * 8 + 16, &r.dptr);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        ++grouped_scan2_calls;
        rc = aqg_grouped_scan2_flat(ctx_, c->handle, op, c->vcols[vx].tag, xf, c->vcols[vy].tag, yf, w, static_cast<double*>(r.dptr));
        if (rc != AQG_OK) die("aqg_grouped_scan2_flat", rc, ctx_);
        return vcol_new(c, key, r);
    }
    // decay(halflife, t) of every group's slice: one aqg_grouped_decay_from_times_flat over the flat column
    int vcol_decay(GroupCtx* c, int v, double halflife) {
        uint64_t hbits;
        std::memcpy(&hbits, &halflife, 8);
        const std::array<uint64_t, 6> key{6, hbits, (uint64_t)v, 0, 0, 0};
        auto it = c->memo.find(key);
        if (it != c->memo.end()) return it->second;
        VCol r; r.layout = 1; r.tag = AQG_DOUBLE;
        const void* tf = vcol_flat_ptr(c, v);
        int rc = aqg_malloc(ctx(), (size_t)c->n * 8 + 16, &r.dptr);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        rc = aqg_grouped_decay_from_times_flat(ctx_, c->handle, c->vcols[v].tag, tf, halflife, static_cast<double*>(r.dptr));
        if (rc != AQG_OK) die("aqg_grouped_decay_from_times_flat", rc, ctx_);
        return vcol_new(c, key, r);
    }
    // sumr / avgr / minr / maxr / countr of every group's slice (include/aqg.h, time-range windows section): the bounds of a (stamps, span,
    // frame) are searched ONCE for all groups (aqg_grouped_rangew_bounds_flat) and memoised apart from the folds over them, so that
    // `sumr(40, t, c)`, `maxr(40, t, c)` and `countr(40, t)` in one loop cost one search and one aqg_rangew_fold each.  vx < 0: COUNT.
    size_t grouped_rangew_bounds_calls = 0, grouped_rangew_fold_calls = 0;      // calls made so far (the tests count them)
    int vcol_rangew(GroupCtx* c, int op, int vt, int vx, double span, int frame) {
        uint64_t sbits;
        std::memcpy(&sbits, &span, 8);
        const std::array<uint64_t, 6> bkey{7, sbits, (uint64_t)vt, (uint64_t)frame, 0, 0};
        int lo;
        auto bt = c->memo.find(bkey);
        if (bt != c->memo.end()) lo = bt->second;
        else {
            VCol b; b.layout = 1; b.tag = AQG_UINT32;
            const void* tf = vcol_flat_ptr(c, vt);
            int rc = aqg_malloc(ctx(), (size_t)c->n * 4 + 16, &b.dptr);
            if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
            ++grouped_rangew_bounds_calls;
            rc = aqg_grouped_rangew_bounds_flat(ctx_, c->handle, c->vcols[vt].tag, tf, span, frame, static_cast<uint32_t*>(b.dptr));
            if (rc != AQG_OK) die("aqg_grouped_rangew_bounds_flat", rc, ctx_);
            lo = vcol_new(c, bkey, b);
        }
        const std::array<uint64_t, 6> key{8, (uint64_t)op, (uint64_t)lo, (uint64_t)(vx + 1), 0, 0};
        auto it = c->memo.find(key);
        if (it != c->memo.end()) return it->second;
        const int xtag = vx < 0 ? (int)AQG_INT32 : c->vcols[vx].tag;
        VCol r; r.layout = 1; r.tag = aqg_rangew_out_dtype(op, xtag);
        const void* xf = vx < 0 ? nullptr : vcol_flat_ptr(c, vx);
        int rc = aqg_malloc(ctx(), (size_t)c->n * esz(r.tag) + 16, &r.dptr);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        ++grouped_rangew_fold_calls;
        rc = aqg_rangew_fold(ctx_, op, xtag, xf, c->n, static_cast<const uint32_t*>(c->vcols[lo].dptr), r.dptr);
        if (rc != AQG_OK) die("aqg_rangew_fold", rc, ctx_);
        return vcol_new(c, key, r);
    }
    // l OP r of two columns of the grouping: in row order when both are (one pass over the whole columns), else in the flat layout
    int vcol_ewise(GroupCtx* c, int op, int l, int r, int ot) {
        const std::array<uint64_t, 6> key{2, (uint64_t)op, (uint64_t)l, (uint64_t)r, (uint64_t)ot, 0};
        auto it = c->memo.find(key);
        if (it != c->memo.end()) return it->second;
        VCol o; o.tag = ot;
        o.layout = (c->vcols[l].layout == 0 && c->vcols[r].layout == 0) ? 0 : 1;
        void *tl = nullptr, *tr = nullptr;
        const void* dl = o.layout ? vcol_flat_ptr(c, l) : vcol_row_ptr(c, l, &tl);
        const void* dr = o.layout ? vcol_flat_ptr(c, r) : vcol_row_ptr(c, r, &tr);
        int rc = aqg_malloc(ctx(), (size_t)c->n * esz(ot) + 16, &o.dptr);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        rc = aqg_ewise(ctx_, op, AQG_VEC_VEC, c->vcols[l].tag, dl, c->vcols[r].tag, dr, ot, o.dptr, c->n);
        if (rc != AQG_OK) die("aqg_ewise", rc, ctx_);
        release(tl); release(tr);
        return vcol_new(c, key, o);
    }
    // column OP scalar (kind: AQG_VEC_SCALAR / AQG_SCALAR_VEC) for group g, whose slice has `vsize` elements.  A scalar that is the same for
    // every group gives ONE constant-scalar column.  A scalar that differs between the groups (`x[val] - min(x[val])`) is looked up among
    // the per-group aggregates this grouping already holds: found, the operator runs once for all groups with a per-group scalar column
    // (vcol_ewise_grouped); not found (a scalar derived on the host), -1 and the caller takes the per-group path
    size_t grouped_ewise_calls = 0;   // aqg_grouped_ewise calls made so far
    size_t scalar_fallbacks = 0;      // times vcol_ewise_scalar sent its caller to the per-group path
    int vcol_ewise_scalar(GroupCtx* c, int op, int kind, int v, int st, const void* scalar, size_t ssz, int ot, uint32_t g, uint32_t vsize) {
        uint64_t bits[2] = {0, 0};
        std::memcpy(bits, scalar, ssz < 16 ? ssz : 16);
        const std::array<uint64_t, 4> key{(uint64_t)op | ((uint64_t)kind << 32), (uint64_t)v, (uint64_t)st, (uint64_t)ot};
        auto it = c->smemo.find(key);
        if (it != c->smemo.end()) {
            GroupCtx::ScalarUse& u = it->second;
            if (!u.varies) {
                if (u.bits[0] == bits[0] && u.bits[1] == bits[1]) return u.vcol;
                u.varies = true;
                if (ssz <= 8 && vsize == c->counts[g]) u.gvcol = vcol_ewise_grouped(c, op, kind, v, st, ssz, ot, u, g, scalar);
            }
            // answered from the expanded column only when this group's scalar IS the element the column was computed with
            if (u.gvcol >= 0 && vsize == c->counts[g] && std::memcmp(&u.scol[(size_t)g * ssz], scalar, ssz) == 0) return u.gvcol;
            ++scalar_fallbacks;
            return -1;
        }
        VCol o; o.tag = ot; o.layout = c->vcols[v].layout;
        void* tv = nullptr;
        const void* dv = o.layout ? c->vcols[v].dptr : vcol_row_ptr(c, v, &tv);
        int rc = aqg_malloc(ctx(), (size_t)c->n * esz(ot) + 16, &o.dptr);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        if (kind == AQG_VEC_SCALAR) rc = aqg_ewise(ctx_, op, kind, c->vcols[v].tag, dv, st, scalar, ot, o.dptr, c->n);
        else rc = aqg_ewise(ctx_, op, kind, st, scalar, c->vcols[v].tag, dv, ot, o.dptr, c->n);
        if (rc != AQG_OK) die("aqg_ewise", rc, ctx_);
        release(tv);
        c->vcols.push_back(o);
        const int id = (int)c->vcols.size() - 1;
        c->smemo[key] = GroupCtx::ScalarUse{{bits[0], bits[1]}, id, false, g, -1, {}};
        return id;
    }
    // The scalar of group u.g0 was u.bits and that of group g is `scalar`: the cached aggregate (column, op) whose slots hold exactly those
    // two values is taken for the scalar's source, its G slots become the scalar column (u.scol, uploaded once) and aqg_grouped_ewise runs
    // over the whole column in its layout.  A wrong guess is harmless: the caller compares every group's scalar with u.scol before it
    // uses the result.  Returns the column, or -1 when no aggregate matches.  Called once per ScalarUse (when it starts to vary).
    // Only the first ssz bytes of a 16-byte slot are compared, whatever the slot's own type: an int scalar can match the low half of a
    // 64-bit or double slot.  That is still sound -- u.scol then holds those very bytes, and the per-group comparison decides.
    int vcol_ewise_grouped(GroupCtx* c, int op, int kind, int v, int st, size_t ssz, int ot, GroupCtx::ScalarUse& u, uint32_t g, const void* scalar) {
        const std::pair<const std::pair<int, int>, std::vector<unsigned char>>* src = nullptr;
        for (const auto& kv : c->cache)
            if (std::memcmp(&kv.second[(size_t)u.g0 * 16], u.bits, ssz) == 0 && std::memcmp(&kv.second[(size_t)g * 16], scalar, ssz) == 0) { src = &kv; break; }
        if (!src) return -1;
        u.scol.resize((size_t)c->G * ssz);
        for (uint32_t k = 0; k < c->G; ++k) std::memcpy(&u.scol[(size_t)k * ssz], &src->second[(size_t)k * 16], ssz);
        const std::array<uint64_t, 6> key{3, (uint64_t)op | ((uint64_t)kind << 32) | ((uint64_t)st << 40), (uint64_t)v,
                                          (uint64_t)(uint32_t)src->first.first, (uint64_t)(uint32_t)src->first.second, (uint64_t)ot};
        VCol o; o.tag = ot; o.layout = c->vcols[v].layout;
        void *tv = nullptr, *ds = nullptr;
        const void* dv = o.layout ? c->vcols[v].dptr : vcol_row_ptr(c, v, &tv);
        int rc = aqg_malloc(ctx(), (size_t)c->n * esz(ot) + 16, &o.dptr);
        if (rc == AQG_OK) rc = aqg_malloc(ctx_, u.scol.size() + 16, &ds);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        rc = aqg_h2d(ctx_, ds, u.scol.data(), u.scol.size());
        if (rc != AQG_OK) die("aqg_h2d", rc, ctx_);
        ++grouped_ewise_calls;
        rc = aqg_grouped_ewise(ctx_, c->handle, o.layout ? AQG_LAYOUT_FLAT : AQG_LAYOUT_ROW, op, kind, c->vcols[v].tag, dv, st, ds, ot, o.dptr);
        if (rc != AQG_OK) die("aqg_grouped_ewise", rc, ctx_);
        release(tv);
        aqg_free(ctx_, ds);
        return vcol_new(c, key, o);
    }
    void free_vcols(GroupCtx* c) {
        for (auto& v : c->vcols) { if (v.dptr) aqg_free(ctx(), v.dptr); if (v.flat) aqg_free(ctx(), v.flat); }
        c->vcols.clear(); c->memo.clear(); c->smemo.clear(); c->cache.clear(); c->corr_cache.clear(); c->topk_cache.clear(); c->quant_cache.clear();
    }

    // the deferred entry AT host address p (a per-group temporary), or nullptr
    Entry* deferred_at(const void* p) {
        auto it = map_.find((uintptr_t)p);
        return (it != map_.end() && it->second.deferred) ? &it->second : nullptr;
    }
    // host buffer [host_out, +bytes) := group g's slice of column v (nothing runs)
    void defer_slice(void* host_out, size_t bytes, GroupCtx* gc, uint32_t g, int v) {
        forget_range(host_out, bytes);
        Entry e; e.bytes = bytes; e.host_stale = true; e.deferred = true; e.dgroup = gc; e.dg = g; e.dv = v;
        map_[(uintptr_t)host_out] = e;
        ++stale;
    }
    void defer_gather(void* host_out, size_t bytes, GroupCtx* gc, uint32_t g, const void* src, size_t src_bytes, bool src_borrowed, int tag) {
        defer_slice(host_out, bytes, gc, g, vcol_source(gc, src, src_bytes, src_borrowed, tag));
    }
    // a device buffer holding just this group's slice (consumers that know nothing about groupings)
    void materialize(std::map<uintptr_t, Entry>::iterator it) {
        Entry& e = it->second;
        GroupCtx* c = e.dgroup;
        const int v = e.dv;
        void* d = nullptr;
        int rc = aqg_malloc(ctx(), e.bytes ? e.bytes : 16, &d);
        if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
        e.deferred = false;                                // (before input(): the source may be this very registry)
        e.dptr = d;
        const size_t es = esz(c->vcols[v].tag);
        if (c->vcols[v].layout == 1 || c->vcols[v].flat) {
            const char* f = static_cast<const char*>(vcol_flat_ptr(c, v));
            rc = aqg_d2d(ctx_, d, f + (size_t)c->offsets[e.dg] * es, (size_t)c->counts[e.dg] * es);
            if (rc != AQG_OK) die("aqg_d2d", rc, ctx_);
            return;
        }
        void* tmp = nullptr;
        const void* dsrc = vcol_row_ptr(c, v, &tmp);
        void* tmp2 = nullptr;
        const void* drows = input(c->row_ids + c->offsets[e.dg], (size_t)c->counts[e.dg] * 4, false, &tmp2);
        rc = aqg_gather(ctx_, c->vcols[v].tag, dsrc, static_cast<const uint32_t*>(drows), c->counts[e.dg], d);
        if (rc != AQG_OK) die("aqg_gather", rc, ctx_);
        release(tmp); release(tmp2);
    }
    // op(<per-group temporary>) at p: answered from the per-grouping cache (one kernel for all groups).  op: an aqg_redop, or
    // DEFERRED_MEDIAN (`median(col[vecs[g]])`: aqg_grouped_median / aqg_grouped_median_flat, result in the column's own type)
    // DEFERRED_DISTINCT (`(col[vecs[g]]).distinct_size()`: aqg_grouped_count_distinct / _flat, a uint32 per group)
    static constexpr int DEFERRED_MEDIAN = 1000, DEFERRED_DISTINCT = 1001;
    size_t grouped_calls = 0;      // aqg_grouped_reduce / _reduce_flat / _median / _median_flat / _count_distinct / _count_distinct_flat / _topk / _topk_flat / _quantiles / _quantiles_flat calls made so far (the tests count them)
    // the vector of `size` elements at p is a per-group temporary AND all of its group (a shorter view -- subvec shares the address -- is not)
    bool deferred_whole(const void* p, uint32_t size) {
        Entry* e = deferred_at(p);
        return e && e->dgroup->counts[e->dg] == size;
    }
    bool deferred_reduce(const void* p, int op, void* out16) {
        Entry* ep = deferred_at(p);
        if (!ep) return false;
        Entry& e = *ep;
        GroupCtx* c = e.dgroup;
        auto key = std::make_pair(e.dv, op);
        auto hit = c->cache.find(key);
        if (hit == c->cache.end()) {
            const int tag = c->vcols[e.dv].tag;
            const bool med = op == DEFERRED_MEDIAN, dis = op == DEFERRED_DISTINCT;
            const int ot = med ? tag : dis ? (int)AQG_UINT32 : aqg_reduce_out_dtype(op, tag);
            const size_t osz = aqg_dtype_size(ot);
            void* dout = nullptr;
            int rc = aqg_malloc(ctx(), (size_t)c->G * 16 + 16, &dout);
            if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
            ++grouped_calls;
            if (c->vcols[e.dv].layout == 1) {
                rc = med ? aqg_grouped_median_flat(ctx_, c->handle, AQG_SEL_LOWER, tag, c->vcols[e.dv].dptr, dout)
                   : dis ? aqg_grouped_count_distinct_flat(ctx_, c->handle, tag, c->vcols[e.dv].dptr, static_cast<uint32_t*>(dout))
                         : aqg_grouped_reduce_flat(ctx_, c->handle, op, tag, c->vcols[e.dv].dptr, dout);
                if (rc != AQG_OK) die(med ? "aqg_grouped_median_flat" : dis ? "aqg_grouped_count_distinct_flat" : "aqg_grouped_reduce_flat", rc, ctx_);
            } else {
                void* tmp = nullptr;
                const void* dsrc = vcol_row_ptr(c, e.dv, &tmp);
                rc = med ? aqg_grouped_median(ctx_, c->handle, AQG_SEL_LOWER, tag, dsrc, dout)
                   : dis ? aqg_grouped_count_distinct(ctx_, c->handle, tag, dsrc, static_cast<uint32_t*>(dout)) : aqg_grouped_reduce(ctx_, c->handle, op, tag, dsrc, dout);
                if (rc != AQG_OK) die(med ? "aqg_grouped_median" : dis ? "aqg_grouped_count_distinct" : "aqg_grouped_reduce", rc, ctx_);
                release(tmp);
            }
            std::vector<unsigned char> packed((size_t)c->G * osz), slots((size_t)c->G * 16, 0);
            rc = aqg_d2h(ctx_, packed.data(), dout, packed.size());
            if (rc != AQG_OK) die("aqg_d2h", rc, ctx_);
            for (uint32_t g = 0; g < c->G; ++g) std::memcpy(&slots[(size_t)g * 16], &packed[(size_t)g * osz], osz);
            aqg_free(ctx_, dout);
            hit = c->cache.emplace(key, std::move(slots)).first;
        }
        std::memcpy(out16, &hit->second[(size_t)e.dg * 16], 16);
        return true;
    }
    // maxk / mink (order: AQG_ORDER_DESC / ASC, 1 <= k <= AQG_TOPK_MAX) of the per-group temporary of `size` elements at p, when it is all
    // of its group (deferred_whole): ONE aqg_grouped_topk (a table column) or aqg_grouped_topk_flat (a virtual column) for all groups, the
    // G x k values brought to the host once and cached under (column, order, k); out receives this group's min(k, size) elements
    bool deferred_topk(const void* p, uint32_t size, int order, uint32_t k, void* out) {
        if (!deferred_whole(p, size)) return false;
        Entry& e = *deferred_at(p);
        GroupCtx* c = e.dgroup;
        const int tag = c->vcols[e.dv].tag;
        const size_t es = esz(tag);
        const std::array<uint32_t, 3> key{(uint32_t)e.dv, (uint32_t)order, k};
        auto hit = c->topk_cache.find(key);
        if (hit == c->topk_cache.end()) {
            void* dout = nullptr;
            int rc = aqg_malloc(ctx(), (size_t)c->G * k * es + 16, &dout);
            if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
            ++grouped_calls;
            if (c->vcols[e.dv].layout == 1) {
                rc = aqg_grouped_topk_flat(ctx_, c->handle, order, tag, c->vcols[e.dv].dptr, k, dout, nullptr);
                if (rc != AQG_OK) die("aqg_grouped_topk_flat", rc, ctx_);
            } else {
                void* tmp = nullptr;
                const void* dsrc = vcol_row_ptr(c, e.dv, &tmp);
                rc = aqg_grouped_topk(ctx_, c->handle, order, tag, dsrc, k, dout, nullptr);
                if (rc != AQG_OK) die("aqg_grouped_topk", rc, ctx_);
                release(tmp);
            }
            std::vector<unsigned char> vals((size_t)c->G * k * es);
            rc = aqg_d2h(ctx_, vals.data(), dout, vals.size());
            if (rc != AQG_OK) die("aqg_d2h", rc, ctx_);
            aqg_free(ctx_, dout);
            hit = c->topk_cache.emplace(key, std::move(vals)).first;
        }
        std::memcpy(out, &hit->second[(size_t)e.dg * k * es], (size_t)(size < k ? size : k) * es);
        return true;
    }
    // quantile / quantiles (which: AQG_SEL_LOWER / UPPER, 1 <= nq <= AQG_QUANTILES_MAX ranks num[j] / den) of the per-group temporary of
    // `size` elements at p, when it is all of its group (deferred_whole): ONE aqg_grouped_quantiles (a table column) or
    // aqg_grouped_quantiles_flat (a virtual column) for all groups, the G x nq values brought to the host once and cached under
    // (column, which, den, the num list); out receives this group's nq elements
    bool deferred_quantiles(const void* p, uint32_t size, int which, uint32_t den, const uint32_t* num, uint32_t nq, void* out) {
        if (!deferred_whole(p, size)) return false;
        Entry& e = *deferred_at(p);
        GroupCtx* c = e.dgroup;
        const int tag = c->vcols[e.dv].tag;
        const size_t es = esz(tag);
        std::vector<uint32_t> key{(uint32_t)e.dv, (uint32_t)which, den};
        key.insert(key.end(), num, num + nq);
        auto hit = c->quant_cache.find(key);
        if (hit == c->quant_cache.end()) {
            void* dout = nullptr;
            int rc = aqg_malloc(ctx(), (size_t)c->G * nq * es + 16, &dout);
            if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
            ++grouped_calls;
            if (c->vcols[e.dv].layout == 1) {
                rc = aqg_grouped_quantiles_flat(ctx_, c->handle, which, nq, num, den, tag, c->vcols[e.dv].dptr, dout);
                if (rc != AQG_OK) die("aqg_grouped_quantiles_flat", rc, ctx_);
            } else {
                void* tmp = nullptr;
                const void* dsrc = vcol_row_ptr(c, e.dv, &tmp);
                rc = aqg_grouped_quantiles(ctx_, c->handle, which, nq, num, den, tag, dsrc, dout);
                if (rc != AQG_OK) die("aqg_grouped_quantiles", rc, ctx_);
                release(tmp);
            }
            std::vector<unsigned char> vals((size_t)c->G * nq * es);
            rc = aqg_d2h(ctx_, vals.data(), dout, vals.size());
            if (rc != AQG_OK) die("aqg_d2h", rc, ctx_);
            aqg_free(ctx_, dout);
            hit = c->quant_cache.emplace(std::move(key), std::move(vals)).first;
        }
        std::memcpy(out, &hit->second[(size_t)e.dg * nq * es], (size_t)nq * es);
        return true;
    }
    // corr(<temporary>, <temporary>) of the same group, both row-order columns: aqg_grouped_corr once for all groups
    bool deferred_corr(const void* px, const void* py, double* out) {
        Entry *ex = deferred_at(px), *ey = deferred_at(py);
        if (!ex || !ey || ex->dgroup != ey->dgroup || ex->dg != ey->dg) return false;
        GroupCtx* c = ex->dgroup;
        if (c->vcols[ex->dv].layout != 0 || c->vcols[ey->dv].layout != 0) return false;
        auto key = std::make_pair(ex->dv, ey->dv);
        auto hit = c->corr_cache.find(key);
        if (hit == c->corr_cache.end()) {
            void *tx = nullptr, *ty = nullptr, *dout = nullptr;
            const void* dx = vcol_row_ptr(c, ex->dv, &tx);
            const void* dy = vcol_row_ptr(c, ey->dv, &ty);
            int rc = aqg_malloc(ctx(), (size_t)c->G * 8 + 16, &dout);
            if (rc != AQG_OK) die("aqg_malloc", rc, ctx_);
            rc = aqg_grouped_corr(ctx_, c->handle, c->vcols[ex->dv].tag, dx, c->vcols[ey->dv].tag, dy, static_cast<double*>(dout));
            release(tx); release(ty);
            if (rc == AQG_ERR_DTYPE) { aqg_free(ctx_, dout); return false; }     // (8-byte / floating columns: per group through aqg_corr)
            if (rc != AQG_OK) die("aqg_grouped_corr", rc, ctx_);
            std::vector<double> r(c->G);
            rc = aqg_d2h(ctx_, r.data(), dout, (size_t)c->G * 8);
            if (rc != AQG_OK) die("aqg_d2h", rc, ctx_);
            aqg_free(ctx_, dout);
            hit = c->corr_cache.emplace(key, std::move(r)).first;
        }
        *out = hit->second[ex->dg];
        return true;
    }
    // host copy of a per-group temporary: beyond a handful of groups the whole flat column comes down ONCE and every slice is a memcpy
    bool touch_deferred(std::map<uintptr_t, Entry>::iterator it) {
        Entry& e = it->second;
        GroupCtx* c = e.dgroup;
        if (c->G <= 8 && c->vcols[e.dv].layout == 0 && !c->vcols[e.dv].flat) return false;
        const size_t es = esz(c->vcols[e.dv].tag);
        if (!c->vcols[e.dv].host_valid) {
            const void* f = vcol_flat_ptr(c, e.dv);
            c->vcols[e.dv].host.resize((size_t)c->n * es);
            int rc = aqg_d2h(ctx(), c->vcols[e.dv].host.data(), f, (size_t)c->n * es);
            if (rc != AQG_OK) die("aqg_d2h", rc, ctx_);
            c->vcols[e.dv].host_valid = true;
        }
        std::memcpy((void*)it->first, c->vcols[e.dv].host.data() + (size_t)c->offsets[e.dg] * es, (size_t)c->counts[e.dg] * es);
        --stale;
        map_.erase(it);
        return true;
    }

    // make the host copy of the buffer containing p valid
    void touch(const void* p) {
        auto it = find(p);
        if (it != map_.end() && it->second.deferred) { if (touch_deferred(it)) return; materialize(it); }
        if (it == map_.end() || !it->second.host_stale) return;
        if (it->second.gctx && !it->second.dptr) fill_rows(it->second);
        int rc = aqg_d2h(ctx(), (void*)it->first, it->second.dptr, it->second.bytes);
        if (rc != AQG_OK) die("aqg_d2h", rc, ctx_);
        it->second.host_stale = false;
        --stale;
        // mutable host access follows: a RESULT's device copy cannot be trusted from here on
        if (!it->second.pinned && !it->second.gctx) { if (it->second.dptr) aqg_free(ctx_, it->second.dptr); map_.erase(it); }
    }
    // write-back: the host copies of several RESULT columns at once -- asynchronous egress of all of them (aqg_col_fetch: page-locked
    // destination, DMA on the copy stream, the copies overlap each other and the tail kernels still queued), ONE wait
    void fetch_all(const std::vector<const void*>& ps) {
        std::vector<std::map<uintptr_t, Entry>::iterator> pending;
        for (const void* p : ps) {
            if (!stale) break;
            auto it = find(p);
            if (it == map_.end() || !it->second.host_stale) continue;
            if (it->second.deferred || (it->second.gctx && !it->second.dptr)) { touch(p); continue; }
            int rc = aqg_col_fetch(ctx(), (void*)it->first, it->second.dptr, it->second.bytes);
            if (rc != AQG_OK) die("aqg_col_fetch", rc, ctx_);
            pending.push_back(it);
        }
        if (pending.empty()) return;
        int rc = aqg_col_fetch_wait(ctx());
        if (rc != AQG_OK) die("aqg_col_fetch_wait", rc, ctx_);
        for (auto it : pending) {
            it->second.host_stale = false;
            --stale;
            if (!it->second.pinned && !it->second.gctx) { if (it->second.dptr) aqg_free(ctx_, it->second.dptr); map_.erase(it); }
        }
    }
    // the host buffer at p is going away / being rewritten by the host
    void forget(const void* p) {
        auto it = map_.find((uintptr_t)p);
        if (it == map_.end()) return;
        if (it->second.host_stale) --stale;
        if (it->second.dptr) aqg_free(ctx(), it->second.dptr);
        map_.erase(it);
    }
    void forget_range(const void* p, size_t bytes) {
        if (map_.empty()) return;
        auto it = map_.lower_bound((uintptr_t)p);
        while (it != map_.end() && it->first < (uintptr_t)p + (bytes ? bytes : 1)) {
            if (it->second.host_stale) --stale;
            if (it->second.dptr) aqg_free(ctx(), it->second.dptr);
            it = map_.erase(it);
        }
    }
    void drop_pins() {
        for (auto it = map_.begin(); it != map_.end();) {
            if (it->second.pinned) { aqg_free(ctx(), it->second.dptr); it = map_.erase(it); } else ++it;
        }
    }
    void sync() { aqg_sync(ctx()); }

    // Groupings made through HashTableFactory::get belong to the SESSION of the module that made them (the reference leaks them:
    // "Memory leak here, cleanup after module is done", hasher.h:255): device handle, row ids, offsets / counts, the key vector and
    // the vecs array are released by Context::end_session() / the module's __AQ_End_Session__ hook / the unload of the module.
    struct SessionItem { GroupCtx* table; void* keys; void (*free_keys)(void*); void* vecs; };
    std::vector<SessionItem> session_items;
    void release_session() {
        for (auto& it : session_items) {
            if (it.table) {
                free_vcols(it.table);
                if (it.table->row_ids) { forget(it.table->row_ids); std::free(it.table->row_ids); }
                if (it.table->handle) aqg_groupby_destroy(it.table->handle);
                std::free(it.table->offsets); std::free(it.table->counts);
                delete it.table;
            }
            if (it.keys && it.free_keys) it.free_keys(it.keys);
            std::free(it.vecs);
        }
        session_items.clear();
    }

private:
    Runtime() = default;
    ~Runtime() {
        release_session();
        if (ctx_) {
            for (auto& kv : map_) if (kv.second.dptr) aqg_free(ctx_, kv.second.dptr);
            aqg_ctx_destroy(ctx_);
        }
    }
    aqg_ctx* ctx_ = nullptr;
    std::map<uintptr_t, Entry> map_;
};

inline void host_touch(const void* p) {
    Runtime& r = Runtime::get();
    if (r.stale) r.touch(p);
}

inline void check(int rc, const char* what) {
    if (rc != AQG_OK) die(what, rc, Runtime::get().ctx());
}

// dtype tag of a C++ element type (reference server/types.h:162-190 mapping)
template <class T> struct tag_of { static constexpr int value = AQG_ERROR; };
#define AQ_TAG(T, V) template <> struct tag_of<T> { static constexpr int value = V; };
AQ_TAG(int, AQG_INT32) AQ_TAG(float, AQG_FLOAT) AQ_TAG(double, AQG_DOUBLE) AQ_TAG(long, AQG_INT64) AQ_TAG(long long, AQG_INT64)
AQ_TAG(short, AQG_INT16) AQ_TAG(signed char, AQG_INT8) AQ_TAG(char, AQG_INT8) AQ_TAG(unsigned char, AQG_UINT8)
AQ_TAG(unsigned short, AQG_UINT16) AQ_TAG(unsigned int, AQG_UINT32) AQ_TAG(unsigned long, AQG_UINT64) AQ_TAG(unsigned long long, AQG_UINT64)
AQ_TAG(bool, AQG_BOOL)
#ifdef __SIZEOF_INT128__
AQ_TAG(__int128, AQG_INT128) AQ_TAG(unsigned __int128, AQG_UINT128)
#endif
#undef AQ_TAG
template <class T> constexpr bool on_device = tag_of<std::remove_cv_t<T>>::value != AQG_ERROR;

// RAII view of a column's device address for the duration of one call
struct In {
    const void* d = nullptr;
    void* temp = nullptr;
    In(const void* host, size_t bytes, bool borrowed) { d = Runtime::get().input(host, bytes, borrowed, &temp); }
    ~In() { Runtime::get().release(temp); }
    In(const In&) = delete;
    In& operator=(const In&) = delete;
};

// distinct_size() of the `size` elements at `host` (vector_type / ColRef): *out = the size of the reference's std::unordered_set over
// them (include/aqg.h, count distinct section).  A per-group temporary `col[vecs[g]]` is answered for ALL groups by one grouped call
// (deferred_reduce); any other vector of a 1-, 2-, 4- or 8-byte numeric type or bool by aqg_count_distinct.  false: the caller keeps
// its host set -- other element types, and a view SHORTER than its group (it shares the temporary's address)
template <class T> inline bool count_distinct(const T* host, uint32_t size, bool borrowed, uint32_t* out) {
    using E = std::remove_cv_t<T>;
    if constexpr (!on_device<E> || sizeof(E) > 8) return false;
    else {
        if (!size) { *out = 0; return true; }
        Runtime& rt = Runtime::get();
        if (rt.deferred_at(host)) {
            alignas(16) unsigned char buf[16];
            if (!rt.deferred_whole(host, size) || !rt.deferred_reduce(host, Runtime::DEFERRED_DISTINCT, buf)) return false;
            std::memcpy(out, buf, 4);
            return true;
        }
        In in(host, (size_t)size * sizeof(E), borrowed);
        check(aqg_count_distinct(rt.ctx(), tag_of<E>::value, in.d, size, out), "aqg_count_distinct");
        return true;
    }
}

} // namespace dev
} // namespace aq
