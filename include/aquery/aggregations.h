// aggregations.h -- reductions, prefix scans, sliding windows and shifts of the AQuery library API
// (names, argument order and result types of the reference's server/aggregations.h; `avgs(w, x)` in SQL is
// emitted as `avgw(w, x)`, `next` as `aggnext`: common/types.py:285-290,334).  Every vector argument is
// reduced / scanned by one HIP kernel through the C-ABI; scalars fall through to the identity overloads
// at the bottom exactly like the reference's.
#pragma once
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <limits>
#include <utility>
#include <vector>

#include "gc.h"
#include "types.h"
#include "vector_type.hpp"
#undef max
#undef min

namespace aq {

template <template <typename...> class VT, class T> constexpr bool is_vt = std::is_base_of_v<vector_base<T>, VT<T>>;

template <class R, class T, template <typename...> class VT> inline R device_reduce(int op, const VT<T>& v) {
    auto& rt = dev::Runtime::get();
    alignas(16) unsigned char buf[16];
    if (!rt.deferred_reduce(v.container, op, buf)) {      // not a deferred `col[vecs[g]]`: reduce this very vector
        dev::In in(v.container, (size_t)v.size * sizeof(T), v.capacity == 0);
        dev::check(aqg_reduce(rt.ctx(), op, dev::tag_of<T>::value, in.d, v.size, buf), "aqg_reduce");
    }
    R r;
    std::memcpy(&r, buf, sizeof(R));
    return r;
}

// ret = scan(op, w, arr): `ret` may be a fresh vector or the caller's out-parameter
template <class T, template <typename...> class VT, class Ret> inline void device_scan(int op, uint32_t w, const VT<T>& arr, Ret& ret) {
    using RT = std::remove_cv_t<std::remove_pointer_t<decltype(ret.container)>>;
    auto& rt = dev::Runtime::get();
    const uint32_t n = arr.size;
    if (n == 0) return;
    const int want = aqg_scan_out_dtype(op, dev::tag_of<T>::value);
    if (want != dev::tag_of<RT>::value) { std::fprintf(stderr, "[aquery-mi355x] scan result element type mismatch (op %d)\n", op); std::abort(); }
    // a per-group temporary of the generated loop (`avgw(10, sales[vecs[i]], col[i])`, mem_opt.cpp:61; engine/ast.py:749-784): the scan
    // runs ONCE for all groups over the flat layout (aqg_grouped_scan_flat) and `ret` becomes this group's slice of that result
    if (dev::Entry* e = rt.deferred_at(arr.container)) {
        dev::GroupCtx* gc = e->dgroup;
        const uint32_t g = e->dg;
        const int r = rt.vcol_scan(gc, e->dv, op, w);
        rt.defer_slice(ret.container, (size_t)n * sizeof(RT), gc, g, r);
        if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
        return;
    }
    void* dout = rt.result(ret.container, (size_t)n * sizeof(RT));
    dev::In in(arr.container, (size_t)n * sizeof(T), arr.capacity == 0);
    dev::check(aqg_scan(rt.ctx(), op, dev::tag_of<T>::value, in.d, n, w, dout), "aqg_scan");
    if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
}
template <class T> using fp_of_long = types::GetFPType<types::GetLongType<T>>;   // double for every numeric T

// ret[0, m) = the m = min(k, arr.size) largest (AQG_ORDER_DESC) / smallest (AQG_ORDER_ASC) elements of arr, in that order (include/aqg.h,
// top-k section); `ret` holds at least m elements.  A per-group temporary of the generated loop that is all of its group is answered for
// ALL groups by one grouped call (Runtime::deferred_topk) and copied on the host; any other vector goes through aqg_topk.  k above
// AQG_TOPK_MAX, and the 128-bit element types, sort that vector's rows (aqg_sort_rows) and gather the first m.
template <class T, template <typename...> class VT, class Ret> inline void device_topk(int order, uint32_t k, const VT<T>& arr, Ret& ret) {
    using RT = std::remove_cv_t<std::remove_pointer_t<decltype(ret.container)>>;
    static_assert(std::is_same_v<RT, std::remove_cv_t<T>>, "maxk / mink: the result holds elements of the input");
    auto& rt = dev::Runtime::get();
    const uint32_t n = arr.size, m = n < k ? n : k;
    if (m == 0) return;
    constexpr bool selectable = sizeof(T) <= 8;
    if (selectable && k <= AQG_TOPK_MAX && rt.deferred_topk(arr.container, n, order, k, ret.container)) {
        rt.forget_range(ret.container, (size_t)m * sizeof(T));         // (host memory written here: no device result stands behind it)
        return;
    }
    void* dout = rt.result(ret.container, (size_t)m * sizeof(T));
    dev::In in(arr.container, (size_t)n * sizeof(T), arr.capacity == 0);
    if (selectable && k <= AQG_TOPK_MAX) {
        dev::check(aqg_topk(rt.ctx(), order, dev::tag_of<T>::value, in.d, n, m, dout, nullptr), "aqg_topk");
    } else {
        void* rows = nullptr;
        dev::check(aqg_malloc(rt.ctx(), (size_t)n * 4, &rows), "aqg_malloc");
        const int tag = dev::tag_of<T>::value;
        const void* keys[1] = {in.d};
        dev::check(aqg_sort_rows(rt.ctx(), 1, &tag, keys, &order, n, nullptr, n, static_cast<uint32_t*>(rows)), "aqg_sort_rows");
        dev::check(aqg_gather(rt.ctx(), tag, in.d, static_cast<const uint32_t*>(rows), m, dout), "aqg_gather");
        aqg_free(rt.ctx(), rows);
    }
    if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
}
// out[0, nq) = the rows of rank floor (AQG_SEL_LOWER) / ceil (AQG_SEL_UPPER) of nums[j] (arr.size - 1) / den of arr in ascending order
// (include/aqg.h, quantiles section), in the order of `nums`; `out` is host memory.  A per-group temporary of the generated loop that is
// all of its group is answered for ALL groups by one grouped call (Runtime::deferred_quantiles); any other vector goes through
// aqg_quantiles.  A list longer than AQG_QUANTILES_MAX is asked for in runs of that many.  Empty input: zeros.
template <class T, template <typename...> class VT> inline void device_quantiles(int which, uint32_t den, const uint32_t* nums, uint32_t nq, const VT<T>& arr, T* out) {
    auto& rt = dev::Runtime::get();
    if (!arr.size) { for (uint32_t j = 0; j < nq; ++j) out[j] = T(0); return; }
    for (uint32_t b = 0; b < nq; b += AQG_QUANTILES_MAX) {
        const uint32_t m = nq - b < (uint32_t)AQG_QUANTILES_MAX ? nq - b : (uint32_t)AQG_QUANTILES_MAX;
        if (rt.deferred_quantiles(arr.container, arr.size, which, den, nums + b, m, out + b)) continue;
        dev::In in(arr.container, (size_t)arr.size * sizeof(T), arr.capacity == 0);     // not a deferred `col[vecs[g]]`: this very vector
        dev::check(aqg_quantiles(rt.ctx(), which, m, nums + b, den, dev::tag_of<T>::value, in.d, arr.size, out + b), "aqg_quantiles");
    }
}
// ret = ema / ewma of arr (include/aqg.h, exponential moving averages section): mode AQG_EMA_RECURSIVE / AQG_EMA_ADJUSTED, a constant alpha
// (dec == nullptr) or a decay column `dec` of arr.size doubles.  A per-group temporary of the generated loop that is ALL of its group is
// answered for all groups by one aqg_grouped_ema_flat (Runtime::vcol_ema) and `ret` becomes this group's slice of that result; the decay
// form takes that path only when the decay column is such a temporary of the SAME group.  Any other vector -- a view shorter than its
// group (`subvec` shares the temporary's address) among them -- goes through aqg_scan_ema on its own rows.
template <class T, template <typename...> class VT, class Ret> inline void device_ema(int mode, double alpha, const double* dec, bool dec_borrowed, const VT<T>& arr, Ret& ret) {
    using RT = std::remove_cv_t<std::remove_pointer_t<decltype(ret.container)>>;
    static_assert(std::is_same_v<RT, double>, "ema / ewma: the result holds doubles");
    auto& rt = dev::Runtime::get();
    const uint32_t n = arr.size;
    if (n == 0) return;
    if (rt.deferred_whole(arr.container, n)) {
        dev::Entry* e = rt.deferred_at(arr.container);
        dev::Entry* ed = dec ? (rt.deferred_whole(dec, n) ? rt.deferred_at(dec) : nullptr) : nullptr;
        if (!dec || (ed && ed->dgroup == e->dgroup && ed->dg == e->dg && ed->dgroup->vcols[ed->dv].tag == AQG_DOUBLE)) {
            dev::GroupCtx* gc = e->dgroup;
            const uint32_t g = e->dg;
            const int r = rt.vcol_ema(gc, e->dv, mode, alpha, ed ? ed->dv : -1);
            rt.defer_slice(ret.container, (size_t)n * sizeof(RT), gc, g, r);
            if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
            return;
        }
    }
    void* dout = rt.result(ret.container, (size_t)n * sizeof(RT));
    dev::In in(arr.container, (size_t)n * sizeof(T), arr.capacity == 0);
    if (dec) {
        dev::In ind(dec, (size_t)n * sizeof(double), dec_borrowed);
        dev::check(aqg_scan_ema(rt.ctx(), mode, dev::tag_of<std::remove_cv_t<T>>::value, in.d, n, alpha, static_cast<const double*>(ind.d), static_cast<double*>(dout)), "aqg_scan_ema");
    } else dev::check(aqg_scan_ema(rt.ctx(), mode, dev::tag_of<std::remove_cv_t<T>>::value, in.d, n, alpha, nullptr, static_cast<double*>(dout)), "aqg_scan_ema");
    if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
}
// ret = the rank of every element of arr in arr (include/aqg.h, ranking section): method AQG_RANK_*, order AQG_ORDER_ASC / DESC, k the
// buckets of NTILE; `ret` holds uint32_t, or doubles for AVERAGE / PERCENT / CUME_DIST.  A per-group temporary of the generated loop that
// is ALL of its group is answered for all groups by one aqg_grouped_rank_flat (Runtime::vcol_rank) and `ret` becomes this group's slice
// of that result; any other vector goes through aqg_rank on its own rows.
template <class T, template <typename...> class VT, class Ret> inline void device_rank(int method, int order, uint32_t k, const VT<T>& arr, Ret& ret) {
    using RT = std::remove_cv_t<std::remove_pointer_t<decltype(ret.container)>>;
    static_assert(std::is_same_v<RT, uint32_t> || std::is_same_v<RT, double>, "rank: the result holds uint32_t or doubles");
    if ((aqg_rank_out_dtype(method) == AQG_DOUBLE) != std::is_same_v<RT, double>) dev::check(AQG_ERR_ARG, "rank: the result's element type does not fit the method");
    auto& rt = dev::Runtime::get();
    const uint32_t n = arr.size;
    if (n == 0) return;
    if (rt.deferred_whole(arr.container, n)) {
        dev::Entry* e = rt.deferred_at(arr.container);
        dev::GroupCtx* gc = e->dgroup;
        const uint32_t g = e->dg;
        rt.defer_slice(ret.container, (size_t)n * sizeof(RT), gc, g, rt.vcol_rank(gc, e->dv, method, order, k));
        if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
        return;
    }
    void* dout = rt.result(ret.container, (size_t)n * sizeof(RT));
    dev::In in(arr.container, (size_t)n * sizeof(T), arr.capacity == 0);
    dev::check(aqg_rank(rt.ctx(), method, order, k, dev::tag_of<std::remove_cv_t<T>>::value, in.d, n, dout), "aqg_rank");
    if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
}
// ret = the pair statistic op (AQG_SCAN2_*) of x and y (include/aqg_pair.h): n doubles.  When both columns are per-group
// temporaries of the generated loop that are ALL of one group of the same grouping, the call is answered for all groups by one
// aqg_grouped_scan2_flat (Runtime::vcol_scan2) and `ret` becomes this group's slice of that result; any other pair of vectors goes
// through aqg_scan2 on its own rows.
template <class Ret> inline void device_scan2(int op, uint32_t w, const void* x, bool x_borrowed, int xtag, size_t xsz,
                                              const void* y, bool y_borrowed, int ytag, size_t ysz, uint32_t n, Ret& ret) {
    using RT = std::remove_cv_t<std::remove_pointer_t<decltype(ret.container)>>;
    static_assert(std::is_same_v<RT, double>, "covw / corrw / betaw: the result holds doubles");
    auto& rt = dev::Runtime::get();
    if (n == 0) return;
    if (rt.deferred_whole(x, n) && rt.deferred_whole(y, n)) {
        dev::Entry* ex = rt.deferred_at(x);
        dev::Entry* ey = rt.deferred_at(y);
        if (ex->dgroup == ey->dgroup && ex->dg == ey->dg) {
            dev::GroupCtx* gc = ex->dgroup;
            const uint32_t g = ex->dg;
            const int r = rt.vcol_scan2(gc, op, ex->dv, ey->dv, w);
            rt.defer_slice(ret.container, (size_t)n * sizeof(RT), gc, g, r);
            if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
            return;
        }
    }
    void* dout = rt.result(ret.container, (size_t)n * sizeof(RT));
    dev::In ix(x, (size_t)n * xsz, x_borrowed);
    dev::In iy(y, (size_t)n * ysz, y_borrowed);
    dev::check(aqg_scan2(rt.ctx(), op, xtag, ix.d, ytag, iy.d, n, w, static_cast<double*>(dout)), "aqg_scan2");
    if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
}
// ret = decay(halflife, t): 2^(-|t[i] - t[i-1]| / halflife), 1 at the first element; a per-group temporary that is all of its group: one
// aqg_grouped_decay_from_times_flat for all groups (Runtime::vcol_decay)
template <class T, template <typename...> class VT, class Ret> inline void device_decay(double halflife, const VT<T>& t, Ret& ret) {
    using RT = std::remove_cv_t<std::remove_pointer_t<decltype(ret.container)>>;
    static_assert(std::is_same_v<RT, double>, "decay: the result holds doubles");
    auto& rt = dev::Runtime::get();
    const uint32_t n = t.size;
    if (n == 0) return;
    if (rt.deferred_whole(t.container, n)) {
        dev::Entry* e = rt.deferred_at(t.container);
        dev::GroupCtx* gc = e->dgroup;
        const uint32_t g = e->dg;
        const int r = rt.vcol_decay(gc, e->dv, halflife);
        rt.defer_slice(ret.container, (size_t)n * sizeof(RT), gc, g, r);
        if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
        return;
    }
    void* dout = rt.result(ret.container, (size_t)n * sizeof(RT));
    dev::In in(t.container, (size_t)n * sizeof(T), t.capacity == 0);
    dev::check(aqg_decay_from_times(rt.ctx(), dev::tag_of<std::remove_cv_t<T>>::value, in.d, n, halflife, static_cast<double*>(dout)), "aqg_decay_from_times");
    if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
}
// ret = op over every row's time window (include/aqg.h, time-range windows section): the rows within `span` of t[i], ending at row i.
// x == nullptr: AQG_RANGEW_COUNT.  When the stamps (and the values) are per-group temporaries of the generated loop that are ALL of one
// group of the same grouping, the call is answered for all groups at once (Runtime::vcol_rangew: one search per (t, span, frame), one
// fold per aggregate) and `ret` becomes this group's slice; any other vector -- a `subvec` view shorter than its group among them --
// goes through aqg_rangew on its own rows.
template <class Ret> inline void device_rangew(int op, double span, bool closed, const void* t, bool t_borrowed, int ttag, size_t tsz,
                                               const void* x, bool x_borrowed, int xtag, size_t xsz, uint32_t n, Ret& ret) {
    using RT = std::remove_cv_t<std::remove_pointer_t<decltype(ret.container)>>;
    auto& rt = dev::Runtime::get();
    if (n == 0) return;
    const int frame = closed ? AQG_RANGEW_CLOSED : AQG_RANGEW_OPEN;
    if (aqg_rangew_out_dtype(op, x ? xtag : (int)AQG_INT32) != dev::tag_of<RT>::value) { std::fprintf(stderr, "[aquery-mi355x] time-range window result element type mismatch (op %d)\n", op); std::abort(); }
    if (rt.deferred_whole(t, n) && (!x || rt.deferred_whole(x, n))) {
        dev::Entry* et = rt.deferred_at(t);
        dev::Entry* ex = x ? rt.deferred_at(x) : nullptr;
        if (!ex || (ex->dgroup == et->dgroup && ex->dg == et->dg)) {
            dev::GroupCtx* gc = et->dgroup;
            const uint32_t g = et->dg;
            const int r = rt.vcol_rangew(gc, op, et->dv, ex ? ex->dv : -1, span, frame);
            rt.defer_slice(ret.container, (size_t)n * sizeof(RT), gc, g, r);
            if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
            return;
        }
    }
    void* dout = rt.result(ret.container, (size_t)n * sizeof(RT));
    dev::In it(t, (size_t)n * tsz, t_borrowed);
    if (x) {
        dev::In ix(x, (size_t)n * xsz, x_borrowed);
        dev::check(aqg_rangew(rt.ctx(), op, ttag, it.d, span, frame, xtag, ix.d, n, dout), "aqg_rangew");
    } else dev::check(aqg_rangew(rt.ctx(), op, ttag, it.d, span, frame, AQG_INT32, nullptr, n, dout), "aqg_rangew");
    if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
}
// ret[i] = the row of rank floor (AQG_SEL_LOWER) / ceil (AQG_SEL_UPPER) of num (len - 1) / den of the last len = min(w, i + 1) elements of
// arr in ascending order (include/aqg.h, moving quantiles section).  A per-group temporary of the generated loop is answered for ALL groups
// by one aqg_grouped_window_quantiles_flat (Runtime::vcol_window_quantile) and `ret` becomes this group's slice of that result, exactly as
// device_scan does; any other vector goes through aqg_window_quantiles.
// THE SLOW PATH: an effective window min(w, arr.size) above AQG_WINQ_MAX_W is beyond the device call (O(w) per row there; the wide-window
// algorithm is unbuilt).  The vector is brought to the host and every window answered by std::nth_element on a
// copy, under the same order (NaNs above +inf, the two zeros one value): O(w) per row on one core.
template <class T, template <typename...> class VT, class Ret> inline void device_window_quantile(int which, uint32_t w, uint32_t num, uint32_t den, const VT<T>& arr, Ret& ret) {
    using RT = std::remove_cv_t<std::remove_pointer_t<decltype(ret.container)>>;
    using E = std::remove_cv_t<T>;
    static_assert(std::is_same_v<RT, E>, "medianw / quantilew: the result holds elements of the input");
    auto& rt = dev::Runtime::get();
    const uint32_t n = arr.size;
    if (n == 0) return;
    if (w <= (uint32_t)AQG_WINQ_MAX_W) {
        if (dev::Entry* e = rt.deferred_at(arr.container)) {
            dev::GroupCtx* gc = e->dgroup;
            const uint32_t g = e->dg;
            const int r = rt.vcol_window_quantile(gc, e->dv, w, which, num, den);
            rt.defer_slice(ret.container, (size_t)n * sizeof(RT), gc, g, r);
            if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
            return;
        }
    }
    if ((w < n ? w : n) <= (uint32_t)AQG_WINQ_MAX_W) {
        dev::In in(arr.container, (size_t)n * sizeof(T), arr.capacity == 0);
        void* dout = rt.result(ret.container, (size_t)n * sizeof(RT));
        dev::check(aqg_window_quantiles(rt.ctx(), which, 1, &num, den, dev::tag_of<E>::value, in.d, n, w, dout), "aqg_window_quantiles");
        if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
        return;
    }
    if (den < 1 || num > den || (which != AQG_SEL_LOWER && which != AQG_SEL_UPPER)) dev::check(AQG_ERR_ARG, "medianw / quantilew: num / den");
    const E* x = arr.begin();                                  // (host access: downloads a device result)
    rt.forget_range(ret.container, (size_t)n * sizeof(RT));    // (host memory written here: no device result stands behind it)
    auto before = [](const E& a, const E& b) {
        if constexpr (std::is_floating_point_v<E>) { if (b != b) return a == a; if (a != a) return false; }
        return a < b;
    };
    std::vector<E> win(w < n ? w : n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = i + 1 < w ? i + 1 : w;
        std::copy(x + (i + 1 - len), x + i + 1, win.begin());
        const uint64_t p = (uint64_t)num * (len - 1);
        const uint32_t k = (uint32_t)(p / den + (which == AQG_SEL_UPPER && p % den != 0 ? 1u : 0u));
        std::nth_element(win.begin(), win.begin() + k, win.begin() + len, before);
        ret.container[i] = win[k];
    }
}
} // namespace aq

// ---- reductions ---------------------------------------------------------------------------------------------------
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
size_t count(const VT<T>& v) { return v.size; }

template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
types::GetLongType<T> sum(const VT<T>& v) { return aq::device_reduce<types::GetLongType<T>>(AQG_RED_SUM, v); }

template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
double avg(const VT<T>& v) { return aq::device_reduce<double>(AQG_RED_AVG, v); }

// max seeds with numeric_limits<T>::min() like the reference (defect D8 kept: max({-1.,-2.}) == DBL_MIN)
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
T max(const VT<T>& v) { return aq::device_reduce<T>(AQG_RED_MAX, v); }
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
T min(const VT<T>& v) { return aq::device_reduce<T>(AQG_RED_MIN, v); }

template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
aq::fp_of_long<decays<T>> var(const VT<T>& v) { return aq::device_reduce<double>(AQG_RED_VAR, v); }
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
aq::fp_of_long<decays<T>> stddev(const VT<T>& v) { return aq::device_reduce<double>(AQG_RED_STDDEV, v); }

template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
T first(const VT<T>& v) { return v.size ? aq::device_reduce<T>(AQG_RED_FIRST, v) : T(0); }
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
T last(const VT<T>& v) { return v.size ? aq::device_reduce<T>(AQG_RED_LAST, v) : T(0); }

// median (common/types.py:343: fnmedian, result type "as is"; benchmark/h2o/groupby.sql:11-12): the LOWER median, an element of the
// input (include/aqg.h, median section); the reference's header declares no body for it.  Empty input: T(0), like first / last.
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
T median(const VT<T>& v) {
    if (!v.size) return T(0);
    auto& rt = aq::dev::Runtime::get();
    alignas(16) unsigned char buf[16];
    if (!rt.deferred_reduce(v.container, aq::dev::Runtime::DEFERRED_MEDIAN, buf)) {      // not a deferred `col[vecs[g]]`: this very vector
        aq::dev::In in(v.container, (size_t)v.size * sizeof(T), v.capacity == 0);
        aq::dev::check(aqg_median(rt.ctx(), AQG_SEL_LOWER, aq::dev::tag_of<T>::value, in.d, v.size, buf), "aqg_median");
    }
    T r;
    std::memcpy(&r, buf, sizeof(T));
    return r;
}

// maxk(k, v) / mink(k, v): the min(k, v.size) largest / smallest elements of v, largest / smallest first (h2o Q8 `largest two v3 by id6`;
// the order of aqg_sort_rows: NaNs above +inf, the two zeros one value).  The reference's header has neither; they stand in the family of
// maxw / minw (the count first).  The out-parameter form fills the first min(k, v.size) elements of `ret`.  Empty input: an empty vector.
template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
void maxk(uint32_t k, const VT<T>& v, Ret& ret) { aq::device_topk(AQG_ORDER_DESC, k, v, ret); }
template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
void mink(uint32_t k, const VT<T>& v, Ret& ret) { aq::device_topk(AQG_ORDER_ASC, k, v, ret); }
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
inline decayed_t<VT, T> maxk(uint32_t k, const VT<T>& v) { decayed_t<VT, T> ret(v.size < k ? v.size : k); aq::device_topk(AQG_ORDER_DESC, k, v, ret); return ret; }
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
inline decayed_t<VT, T> mink(uint32_t k, const VT<T>& v) { decayed_t<VT, T> ret(v.size < k ? v.size : k); aq::device_topk(AQG_ORDER_ASC, k, v, ret); return ret; }

// quantile(num, den, v): the row of rank floor(num (v.size - 1) / den) of v in ascending order -- the LOWER rank, an element of the input
// (include/aqg.h, quantiles section); quantile(1, 2, v) is median(v).  Empty input: T(0), like median.
// quantiles(den, {num...}, v): one element per num, in the order given, from ONE selection (p5 / p50 / p95 in the passes of one); the
// out-parameter form fills the first nums.size() elements of `ret`.  Interpolated quantiles stay with the caller.
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
T quantile(uint32_t num, uint32_t den, const VT<T>& v) {
    std::remove_cv_t<T> r;
    aq::device_quantiles(AQG_SEL_LOWER, den, &num, 1, v, &r);
    return r;
}
template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
void quantiles(uint32_t den, std::initializer_list<uint32_t> nums, const VT<T>& v, Ret& ret) {
    using RT = std::remove_cv_t<std::remove_pointer_t<decltype(ret.container)>>;
    static_assert(std::is_same_v<RT, std::remove_cv_t<T>>, "quantiles: the result holds elements of the input");
    aq::dev::Runtime::get().forget_range(ret.container, nums.size() * sizeof(T));      // (host memory written here: no device result stands behind it)
    aq::device_quantiles(AQG_SEL_LOWER, den, nums.begin(), (uint32_t)nums.size(), v, ret.container);
}
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
inline decayed_t<VT, T> quantiles(uint32_t den, std::initializer_list<uint32_t> nums, const VT<T>& v) {
    decayed_t<VT, T> ret((uint32_t)nums.size());
    quantiles(den, nums, v, ret);
    return ret;
}

template <class T, template <typename...> class VT, class T2, template <typename...> class VT2,
          std::enable_if_t<aq::is_vt<VT, T> && aq::is_vt<VT2, T2>>* = nullptr>
double corr(const VT<T>& x, const VT2<T2>& y) {
    auto& rt = aq::dev::Runtime::get();
    double r = 0;
    if (rt.deferred_corr(x.container, y.container, &r)) return r;      // `corr(v1[val], v2[val])` (h2o Q9): one grouped pass for all groups
    aq::dev::In a(x.container, (size_t)x.size * sizeof(T), x.capacity == 0), b(y.container, (size_t)y.size * sizeof(T2), y.capacity == 0);
    aq::dev::check(aqg_corr(rt.ctx(), aq::dev::tag_of<T>::value, a.d, aq::dev::tag_of<T2>::value, b.d, x.size, &r), "aqg_corr");
    return r;
}

// ---- element-wise ----------------------------------------------------------------------------------------------------
template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
void sqrt(const VT<T>& v, Ret& ret) {
    auto& rt = aq::dev::Runtime::get();
    if (!v.size) return;
    void* dout = rt.result(ret.container, (size_t)v.size * sizeof(double));
    aq::dev::In in(v.container, (size_t)v.size * sizeof(T), v.capacity == 0);
    aq::dev::check(aqg_unary(rt.ctx(), AQG_UN_SQRT, aq::dev::tag_of<T>::value, in.d, v.size, 0, AQG_DOUBLE, dout), "aqg_unary");
    if (ret.capacity == 0 && GC::scratch_space == nullptr) rt.touch(ret.container);
}
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
VT<double> sqrt(const VT<T>& v) { VT<double> ret(v.size); sqrt(v, ret); return ret; }

template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr>
T truncate(const T& v, const uint32_t precision) {
    auto m = std::pow(10, precision);
    if (v >= std::numeric_limits<T>::max() / m || aq_fp_precision<T> <= precision) return v;
    return std::round(v * m) / m;
}
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
VT<T> truncate(const VT<T>& v, const uint32_t precision) {
    VT<T> ret(v.size);
    if (!v.size) return ret;
    auto& rt = aq::dev::Runtime::get();
    void* dout = rt.result(ret.container, (size_t)v.size * sizeof(T));
    aq::dev::In in(v.container, (size_t)v.size * sizeof(T), v.capacity == 0);
    aq::dev::check(aqg_unary(rt.ctx(), AQG_UN_TRUNCATE, aq::dev::tag_of<T>::value, in.d, v.size, precision, aq::dev::tag_of<T>::value, dout), "aqg_unary");
    return ret;
}
template <class X, class Y, class Z> void pow(X x, Y y, Z& z) { z = std::pow(x, y); }

// ---- scans, windows, shifts: out-parameter form + value-returning form -------------------------------------------------
#define AQ_SCAN(name, code, RET_T)                                                                   \
    template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr> \
    void name(const VT<T>& arr, Ret& ret) { aq::device_scan(code, 0, arr, ret); }                    \
    template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr> \
    inline decayed_t<VT, RET_T> name(const VT<T>& arr) { decayed_t<VT, RET_T> ret(arr.size); aq::device_scan(code, 0, arr, ret); return ret; }
#define AQ_WINDOW(name, code, RET_T)                                                                 \
    template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr> \
    void name(uint32_t w, const VT<T>& arr, Ret& ret) { aq::device_scan(code, w, arr, ret); }        \
    template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr> \
    inline decayed_t<VT, RET_T> name(uint32_t w, const VT<T>& arr) { decayed_t<VT, RET_T> ret(arr.size); aq::device_scan(code, w, arr, ret); return ret; }

AQ_SCAN(mins, AQG_SCAN_MINS, T)
AQ_SCAN(maxs, AQG_SCAN_MAXS, T)
AQ_SCAN(sums, AQG_SCAN_SUMS, types::GetLongType<T>)
AQ_SCAN(avgs, AQG_SCAN_AVGS, aq::fp_of_long<T>)
AQ_SCAN(vars, AQG_SCAN_VARS, aq::fp_of_long<T>)
AQ_SCAN(stddevs, AQG_SCAN_STDDEVS, aq::fp_of_long<T>)
AQ_SCAN(deltas, AQG_SCAN_DELTAS, T)
AQ_SCAN(prev, AQG_SCAN_PREV, T)
AQ_SCAN(aggnext, AQG_SCAN_NEXT, T)
AQ_WINDOW(minw, AQG_SCAN_MINW, T)
AQ_WINDOW(maxw, AQG_SCAN_MAXW, T)
AQ_WINDOW(sumw, AQG_SCAN_SUMW, types::GetLongType<T>)
AQ_WINDOW(avgw, AQG_SCAN_AVGW, aq::fp_of_long<T>)
AQ_WINDOW(varw, AQG_SCAN_VARW, aq::fp_of_long<T>)
AQ_WINDOW(stddevw, AQG_SCAN_STDDEVW, aq::fp_of_long<T>)
AQ_WINDOW(ratiow, AQG_SCAN_RATIOW, types::GetFPType<T>)
#undef AQ_SCAN
#undef AQ_WINDOW

// medianw(w, v) / quantilew(w, num, den, v): the moving median / the moving quantile num / den of the last min(w, i + 1) elements -- the
// LOWER rank, an element of the window (include/aqg.h, moving quantiles section); they fill the hole between minw / maxw and avgw / varw,
// the count first.  The reference's header has neither.  medianw(w, v) is quantilew(w, 1, 2, v).
template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
void quantilew(uint32_t w, uint32_t num, uint32_t den, const VT<T>& arr, Ret& ret) { aq::device_window_quantile(AQG_SEL_LOWER, w, num, den, arr, ret); }
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
inline decayed_t<VT, T> quantilew(uint32_t w, uint32_t num, uint32_t den, const VT<T>& arr) { decayed_t<VT, T> ret(arr.size); aq::device_window_quantile(AQG_SEL_LOWER, w, num, den, arr, ret); return ret; }
template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
void medianw(uint32_t w, const VT<T>& arr, Ret& ret) { aq::device_window_quantile(AQG_SEL_LOWER, w, 1, 2, arr, ret); }
template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
inline decayed_t<VT, T> medianw(uint32_t w, const VT<T>& arr) { decayed_t<VT, T> ret(arr.size); aq::device_window_quantile(AQG_SEL_LOWER, w, 1, 2, arr, ret); return ret; }

// ema(alpha, v) / ewma(alpha, v): the exponential moving average y[i] = alpha v[i] + (1 - alpha) y[i-1], y[0] = v[0] (kdb's ema, pandas'
// ewm(adjust=False)) and its bias-corrected form (pandas' default, adjust=True); emad(decay, v) / ewmad(decay, v) take a decay COLUMN in
// place of 1 - alpha, and decay(halflife, t) = decayt(halflife, t) makes one from a time column: 2^(-|t[i] - t[i-1]| / halflife).  Doubles; the reference's header
// has none of them (include/aqg.h, exponential moving averages section).  Integer alphas and halflives convert.
#define AQ_EMA(name, mode)                                                                                        \
    template <class A, class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T> && std::is_arithmetic_v<A>>* = nullptr> \
    void name(A alpha, const VT<T>& arr, Ret& ret) { aq::device_ema(mode, (double)alpha, nullptr, false, arr, ret); }   \
    template <class A, class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T> && std::is_arithmetic_v<A>>* = nullptr> \
    inline decayed_t<VT, double> name(A alpha, const VT<T>& arr) { decayed_t<VT, double> ret(arr.size); aq::device_ema(mode, (double)alpha, nullptr, false, arr, ret); return ret; } \
    template <class A, class T, std::enable_if_t<std::is_arithmetic_v<A> && std::is_arithmetic_v<T>>* = nullptr> constexpr T name(A, const T& v) { return v; }
#define AQ_EMAD(name, mode)                                                                                       \
    template <template <typename...> class VD, class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T> && aq::is_vt<VD, double>>* = nullptr> \
    void name(const VD<double>& dec, const VT<T>& arr, Ret& ret) {                                              \
        if (dec.size != arr.size) aq::dev::check(AQG_ERR_ARG, #name ": the decay column and the values differ in length"); \
        aq::device_ema(mode, 0.0, dec.container, dec.capacity == 0, arr, ret);                                                       \
    }                                                                                                             \
    template <template <typename...> class VD, class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T> && aq::is_vt<VD, double>>* = nullptr> \
    inline decayed_t<VT, double> name(const VD<double>& dec, const VT<T>& arr) { decayed_t<VT, double> ret(arr.size); name(dec, arr, ret); return ret; }
AQ_EMA(ema, AQG_EMA_RECURSIVE)
AQ_EMA(ewma, AQG_EMA_ADJUSTED)
AQ_EMAD(emad, AQG_EMA_RECURSIVE)
AQ_EMAD(ewmad, AQG_EMA_ADJUSTED)
#undef AQ_EMA
#undef AQ_EMAD
// rank(v) / dense_rank(v) / row_number(v) / avg_rank(v) / percent_rank(v) / cume_dist(v) / ntile(k, v): where every element stands in v, 1-based
// -- SQL's RANK, DENSE_RANK, ROW_NUMBER, PERCENT_RANK, CUME_DIST and NTILE(k) OVER (ORDER BY v), pandas' rank(method='min' / 'dense' /
// 'first' / 'average'), with ties and NaNs as order_by sorts them; a trailing `true` ranks in descending order.  uint32_t, or doubles for
// avg_rank / percent_rank / cume_dist; the reference's header has none of them (include/aqg.h, ranking section).  rankof is the name
// generated code can use for rank: under its `using namespace std` a call to `rank` is ambiguous with std::rank.
#define AQ_RANK(name, method, R)                                                                                   \
    template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T> && !std::is_arithmetic_v<Ret>>* = nullptr> \
    void name(const VT<T>& arr, Ret& ret, bool desc = false) { aq::device_rank(method, desc ? AQG_ORDER_DESC : AQG_ORDER_ASC, 0, arr, ret); } \
    template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>             \
    inline decayed_t<VT, R> name(const VT<T>& arr, bool desc = false) { decayed_t<VT, R> ret(arr.size); name(arr, ret, desc); return ret; }
AQ_RANK(rank, AQG_RANK_MIN, uint32_t)
AQ_RANK(rankof, AQG_RANK_MIN, uint32_t)
AQ_RANK(dense_rank, AQG_RANK_DENSE, uint32_t)
AQ_RANK(row_number, AQG_RANK_FIRST, uint32_t)
AQ_RANK(avg_rank, AQG_RANK_AVERAGE, double)
AQ_RANK(percent_rank, AQG_RANK_PERCENT, double)
AQ_RANK(cume_dist, AQG_RANK_CUME_DIST, double)
#undef AQ_RANK
template <class K, class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T> && std::is_integral_v<K> && !std::is_arithmetic_v<Ret>>* = nullptr>
void ntile(K k, const VT<T>& arr, Ret& ret, bool desc = false) { aq::device_rank(AQG_RANK_NTILE, desc ? AQG_ORDER_DESC : AQG_ORDER_ASC, (uint32_t)k, arr, ret); }
template <class K, class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T> && std::is_integral_v<K>>* = nullptr>
inline decayed_t<VT, uint32_t> ntile(K k, const VT<T>& arr, bool desc = false) { decayed_t<VT, uint32_t> ret(arr.size); ntile(k, arr, ret, desc); return ret; }
// covw(w, x, y) / corrw(w, x, y) / betaw(w, x, y): the population covariance, the correlation and the slope of y on x over the last
// min(w, i + 1) elements; covs(x, y) / corrs(x, y) / betas(x, y): the same over the elements so far -- pandas' rolling(w).cov(ddof=0) /
// .corr() and expanding().  Doubles; corr and beta are NaN where a variance they divide by is not positive (the first element, constant
// windows).  The reference's header has none of them (include/aqg_pair.h).  Scalars: one element has no spread.
#define AQ_PAIR_CALL(op, w)                                                                                       \
    aq::device_scan2(op, (uint32_t)(w), x.container, x.capacity == 0, aq::dev::tag_of<std::remove_cv_t<TX>>::value, sizeof(TX),   \
                     y.container, y.capacity == 0, aq::dev::tag_of<std::remove_cv_t<TY>>::value, sizeof(TY), x.size, ret)
#define AQ_PAIRW(name, op, scalar)                                                                                \
    template <class W, class TX, template <typename...> class VX, class TY, template <typename...> class VY, class Ret,           \
              std::enable_if_t<aq::is_vt<VX, TX> && aq::is_vt<VY, TY> && std::is_integral_v<W> && !std::is_arithmetic_v<Ret>>* = nullptr> \
    void name(W w, const VX<TX>& x, const VY<TY>& y, Ret& ret) {                                                  \
        if (x.size != y.size) aq::dev::check(AQG_ERR_ARG, #name ": the two columns differ in length");            \
        if (!(w > 0)) aq::dev::check(AQG_ERR_ARG, #name ": the window must hold a row");                          \
        AQ_PAIR_CALL(op, w);                                                                                      \
    }                                                                                                             \
    template <class W, class TX, template <typename...> class VX, class TY, template <typename...> class VY,      \
              std::enable_if_t<aq::is_vt<VX, TX> && aq::is_vt<VY, TY> && std::is_integral_v<W>>* = nullptr>       \
    inline decayed_t<VX, double> name(W w, const VX<TX>& x, const VY<TY>& y) { decayed_t<VX, double> ret(x.size); name(w, x, y, ret); return ret; } \
    template <class W, class TX, class TY, std::enable_if_t<std::is_integral_v<W> && std::is_arithmetic_v<TX> && std::is_arithmetic_v<TY>>* = nullptr> \
    constexpr double name(W, const TX&, const TY&) { return scalar; }
#define AQ_PAIRS(name, op, scalar)                                                                                \
    template <class TX, template <typename...> class VX, class TY, template <typename...> class VY, class Ret,    \
              std::enable_if_t<aq::is_vt<VX, TX> && aq::is_vt<VY, TY> && !std::is_arithmetic_v<Ret>>* = nullptr>  \
    void name(const VX<TX>& x, const VY<TY>& y, Ret& ret) {                                                       \
        if (x.size != y.size) aq::dev::check(AQG_ERR_ARG, #name ": the two columns differ in length");            \
        AQ_PAIR_CALL(op, 0);                                                                                      \
    }                                                                                                             \
    template <class TX, template <typename...> class VX, class TY, template <typename...> class VY,               \
              std::enable_if_t<aq::is_vt<VX, TX> && aq::is_vt<VY, TY>>* = nullptr>                                \
    inline decayed_t<VX, double> name(const VX<TX>& x, const VY<TY>& y) { decayed_t<VX, double> ret(x.size); name(x, y, ret); return ret; } \
    template <class TX, class TY, std::enable_if_t<std::is_arithmetic_v<TX> && std::is_arithmetic_v<TY>>* = nullptr> \
    constexpr double name(const TX&, const TY&) { return scalar; }
AQ_PAIRW(covw, AQG_SCAN2_COVW, 0.0)
AQ_PAIRW(corrw, AQG_SCAN2_CORRW, std::numeric_limits<double>::quiet_NaN())
AQ_PAIRW(betaw, AQG_SCAN2_BETAW, std::numeric_limits<double>::quiet_NaN())
AQ_PAIRS(covs, AQG_SCAN2_COVS, 0.0)
AQ_PAIRS(corrs, AQG_SCAN2_CORRS, std::numeric_limits<double>::quiet_NaN())
AQ_PAIRS(betas, AQG_SCAN2_BETAS, std::numeric_limits<double>::quiet_NaN())
#undef AQ_PAIRW
#undef AQ_PAIRS
#undef AQ_PAIR_CALL
// (decayt is the name generated code can use: under its `using namespace std` a call to `decay` is ambiguous with std::decay)
#define AQ_DECAY(name)                                                                                            \
    template <class H, class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T> && std::is_arithmetic_v<H>>* = nullptr> \
    void name(H halflife, const VT<T>& t, Ret& ret) { aq::device_decay((double)halflife, t, ret); }              \
    template <class H, class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T> && std::is_arithmetic_v<H>>* = nullptr> \
    inline decayed_t<VT, double> name(H halflife, const VT<T>& t) { decayed_t<VT, double> ret(t.size); aq::device_decay((double)halflife, t, ret); return ret; } \
    template <class H, class T, std::enable_if_t<std::is_arithmetic_v<H> && std::is_arithmetic_v<T>>* = nullptr> constexpr double name(H, const T&) { return 1.0; }
AQ_DECAY(decay)
AQ_DECAY(decayt)
#undef AQ_DECAY

// sumr / avgr / minr / maxr(span, t, x [, closed]) and countr(span, t [, closed]): the aggregates of the rows within `span` of t[i] that
// end at row i -- windows measured in time, not rows (pandas rolling("5s"), SQL RANGE BETWEEN span PRECEDING AND CURRENT ROW, kdb's wj);
// closed = false: |t[i] - t[j]| < span, true: <= span.  The reference's header has none of them (include/aqg.h, time-range windows section).
#define AQ_RANGEW(name, code, RET_T)                                                                              \
    template <class S, class TT, template <typename...> class VTT, class T, template <typename...> class VT, class Ret,           \
              std::enable_if_t<aq::is_vt<VT, T> && aq::is_vt<VTT, TT> && std::is_arithmetic_v<S> && !std::is_same_v<std::decay_t<Ret>, bool>>* = nullptr> \
    void name(S span, const VTT<TT>& t, const VT<T>& x, Ret& ret, bool closed = false) {                          \
        if (t.size != x.size) aq::dev::check(AQG_ERR_ARG, #name ": the stamps and the values differ in length");  \
        aq::device_rangew(code, (double)span, closed, t.container, t.capacity == 0, aq::dev::tag_of<std::remove_cv_t<TT>>::value, sizeof(TT), \
                          x.container, x.capacity == 0, aq::dev::tag_of<std::remove_cv_t<T>>::value, sizeof(T), x.size, ret);   \
    }                                                                                                             \
    template <class S, class TT, template <typename...> class VTT, class T, template <typename...> class VT,      \
              std::enable_if_t<aq::is_vt<VT, T> && aq::is_vt<VTT, TT> && std::is_arithmetic_v<S>>* = nullptr>     \
    inline decayed_t<VT, RET_T> name(S span, const VTT<TT>& t, const VT<T>& x, bool closed = false) { decayed_t<VT, RET_T> ret(x.size); name(span, t, x, ret, closed); return ret; }
AQ_RANGEW(sumr, AQG_RANGEW_SUM, types::GetLongType<T>)
AQ_RANGEW(avgr, AQG_RANGEW_AVG, aq::fp_of_long<T>)
AQ_RANGEW(minr, AQG_RANGEW_MIN, T)
AQ_RANGEW(maxr, AQG_RANGEW_MAX, T)
#undef AQ_RANGEW
template <class S, class TT, template <typename...> class VTT, class Ret, std::enable_if_t<aq::is_vt<VTT, TT> && std::is_arithmetic_v<S> && !std::is_same_v<std::decay_t<Ret>, bool>>* = nullptr>
void countr(S span, const VTT<TT>& t, Ret& ret, bool closed = false) {
    aq::device_rangew(AQG_RANGEW_COUNT, (double)span, closed, t.container, t.capacity == 0, aq::dev::tag_of<std::remove_cv_t<TT>>::value, sizeof(TT),
                      nullptr, false, AQG_INT32, 0, t.size, ret);
}
template <class S, class TT, template <typename...> class VTT, std::enable_if_t<aq::is_vt<VTT, TT> && std::is_arithmetic_v<S>>* = nullptr>
inline decayed_t<VTT, uint32_t> countr(S span, const VTT<TT>& t, bool closed = false) { decayed_t<VTT, uint32_t> ret(t.size); countr(span, t, ret, closed); return ret; }

template <class T, template <typename...> class VT, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
inline decayed_t<VT, types::GetFPType<T>> ratios(const VT<T>& arr) { return ratiow(1, arr); }
template <class T, template <typename...> class VT, class Ret, std::enable_if_t<aq::is_vt<VT, T>>* = nullptr>
inline void ratios(const VT<T>& arr, Ret& ret) { ratiow(1, arr, ret); }

// ---- scalar fall-backs (non-vector arguments): identity-like, as in the reference (:499-527) --------------------------
template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr size_t count(const T&) { return 1; }
#define AQ_SCALAR_ID(name) template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr T name(const T& v) { return v; }
#define AQ_SCALAR_ZERO(name) template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr T name(const T&) { return 0; }
#define AQ_SCALAR_WID(name) template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr T name(uint32_t, const T& v) { return v; }
AQ_SCALAR_ID(max) AQ_SCALAR_ID(min) AQ_SCALAR_ID(avg) AQ_SCALAR_ID(sum) AQ_SCALAR_ID(maxs) AQ_SCALAR_ID(mins) AQ_SCALAR_ID(avgs)
AQ_SCALAR_ID(sums) AQ_SCALAR_ID(last) AQ_SCALAR_ID(first) AQ_SCALAR_ID(prev) AQ_SCALAR_ID(aggnext) AQ_SCALAR_ID(median)
AQ_SCALAR_ZERO(var) AQ_SCALAR_ZERO(vars) AQ_SCALAR_ZERO(stddev) AQ_SCALAR_ZERO(stddevs) AQ_SCALAR_ZERO(deltas)
AQ_SCALAR_WID(maxw) AQ_SCALAR_WID(minw) AQ_SCALAR_WID(avgw) AQ_SCALAR_WID(sumw) AQ_SCALAR_WID(maxk) AQ_SCALAR_WID(mink) AQ_SCALAR_WID(medianw)
template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr T varw(uint32_t, const T&) { return 0; }
template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr T stddevw(uint32_t, const T&) { return 0; }
template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr T ratiow(uint32_t, const T&) { return 1; }
template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr T ratios(const T&) { return 1; }
template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr T quantile(uint32_t, uint32_t, const T& v) { return v; }
template <class T, std::enable_if_t<std::is_arithmetic_v<T>>* = nullptr> constexpr T quantilew(uint32_t, uint32_t, uint32_t, const T& v) { return v; }
#undef AQ_SCALAR_ID
#undef AQ_SCALAR_ZERO
#undef AQ_SCALAR_WID
