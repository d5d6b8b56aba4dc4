// Hand-recorded modules in the shape the reference's code generator emits (engine/ast.py:722-789) for element-wise operators whose scalar
// operand is a per-group aggregate: under GROUP BY, `price - min(price)` becomes `price[val] - min(price[val])` inside the group loop
// (engine/ast.py:749-784).  Over host_main's `trade` / `trade_small` (stocksymbol, price) and `synthetic` (a, b, c, d: grouped by a, the
// value column is c) datasets: column 0 is the key, column AQ_VALUE_COL the value.
//   dll_gs_demean   SELECT stocksymbol, sum(price - min(price)), max(price - avg(price)) FROM trade GROUP BY stocksymbol
//   dll_gs_norm     SELECT stocksymbol, max(price / first(price)), min(max(price) - price) ...
//   dll_gs_flat     SELECT stocksymbol, max(maxs(price) - min(price)), last(avgs(3, price) - avg(price)) ...      (scan results: flat layout)
//   dll_gs_cov      SELECT stocksymbol, covariance(price, price) ...   with tests/funcs.a's FUNCTION covariance (funcs_udf.cpp)
//   dll_gs_derived  SELECT stocksymbol, sum(price - (max(price) - min(price))) ...      a scalar made on the host: the per-group path
// Every module writes, next to the dumped columns, <out>.calls: grouped_ewise_calls, scalar_fallbacks, grouped_calls, groups.
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"

// the value column of the dataset: price (column 1) of `trade`, c (column 2) of `synthetic`
static int aq_value_col(DataSource* server) { return server->getCol(2, types::Type_t::AINT32) ? 2 : 1; }

auto covariance = [](const auto& x, const auto& y) {
	auto xmean = avg(x);
	auto ymean = avg(y);
	return avg(((x - xmean) * (y - ymean)));
};

__AQEXPORT__(int) dll_gs_demean(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto stocksymbol_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto price_3c = ColRef<int>(len_1a, server->getCol(aq_value_col(server), types::Type_t::AINT32));
const char* names_6f[] = {"stocksymbol", "c0", "c1"};
auto out_7g = new TableInfo<int,value_type<decays<decltype(sum((price_3c - min(price_3c))))>>,value_type<decays<decltype(max((price_3c - avg(price_3c))))>>>("out_7g", names_6f);
decltype(auto) col_8h = out_7g->get_col<0>();
decltype(auto) col_9i = out_7g->get_col<1>();
decltype(auto) col_10i = out_7g->get_col<2>();
uint32_t len_11k = stocksymbol_2b.size;
typedef record<decays<decltype(stocksymbol_2b)>::value_t> record_type12l;
auto g13m = HashTableFactory<record_type12l, transTypes<record_type12l, hasher>>::get<decays<decltype(stocksymbol_2b)>>(stocksymbol_2b);
auto sz_g13m = g13m.size;
auto vecs_14n = g13m.values;
col_8h.resize(sz_g13m);
col_9i.resize(sz_g13m);
col_10i.resize(sz_g13m);
auto& rt_calls = aq::dev::Runtime::get();
const size_t ge_before = rt_calls.grouped_ewise_calls, fb_before = rt_calls.scalar_fallbacks, gc_before = rt_calls.grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i15 = 0; i15 < sz_g13m; ++i15) {
auto &key_16o = (*g13m.keys)[i15];
auto &val_17p = vecs_14n[i15];
col_8h[i15] = (get<0>(key_16o));

col_9i[i15] = (sum((price_3c[val_17p] - min(price_3c[val_17p]))));

col_10i[i15] = (max((price_3c[val_17p] - avg(price_3c[val_17p]))));

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("gs_demean.out", *out_7g);
{ FILE* f = fopen("gs_demean.calls", "w"); fprintf(f, "%zu %zu %zu %u\n", rt_calls.grouped_ewise_calls - ge_before, rt_calls.scalar_fallbacks - fb_before, rt_calls.grouped_calls - gc_before, (unsigned)sz_g13m); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_gs_norm(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto stocksymbol_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto price_3c = ColRef<int>(len_1a, server->getCol(aq_value_col(server), types::Type_t::AINT32));
const char* names_6f[] = {"stocksymbol", "c0", "c1"};
auto out_7g = new TableInfo<int,value_type<decays<decltype(max((price_3c / first(price_3c))))>>,value_type<decays<decltype(min((max(price_3c) - price_3c)))>>>("out_7g", names_6f);
decltype(auto) col_8h = out_7g->get_col<0>();
decltype(auto) col_9i = out_7g->get_col<1>();
decltype(auto) col_10i = out_7g->get_col<2>();
uint32_t len_11k = stocksymbol_2b.size;
typedef record<decays<decltype(stocksymbol_2b)>::value_t> record_type12l;
auto g13m = HashTableFactory<record_type12l, transTypes<record_type12l, hasher>>::get<decays<decltype(stocksymbol_2b)>>(stocksymbol_2b);
auto sz_g13m = g13m.size;
auto vecs_14n = g13m.values;
col_8h.resize(sz_g13m);
col_9i.resize(sz_g13m);
col_10i.resize(sz_g13m);
auto& rt_calls = aq::dev::Runtime::get();
const size_t ge_before = rt_calls.grouped_ewise_calls, fb_before = rt_calls.scalar_fallbacks, gc_before = rt_calls.grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i15 = 0; i15 < sz_g13m; ++i15) {
auto &key_16o = (*g13m.keys)[i15];
auto &val_17p = vecs_14n[i15];
col_8h[i15] = (get<0>(key_16o));

col_9i[i15] = (max((price_3c[val_17p] / first(price_3c[val_17p]))));

col_10i[i15] = (min((max(price_3c[val_17p]) - price_3c[val_17p])));

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("gs_norm.out", *out_7g);
{ FILE* f = fopen("gs_norm.calls", "w"); fprintf(f, "%zu %zu %zu %u\n", rt_calls.grouped_ewise_calls - ge_before, rt_calls.scalar_fallbacks - fb_before, rt_calls.grouped_calls - gc_before, (unsigned)sz_g13m); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_gs_flat(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto stocksymbol_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto price_3c = ColRef<int>(len_1a, server->getCol(aq_value_col(server), types::Type_t::AINT32));
const char* names_6f[] = {"stocksymbol", "c0", "c1"};
auto out_7g = new TableInfo<int,value_type<decays<decltype(max((maxs(price_3c) - min(price_3c))))>>,value_type<decays<decltype(last((avgw(3, price_3c) - avg(price_3c))))>>>("out_7g", names_6f);
decltype(auto) col_8h = out_7g->get_col<0>();
decltype(auto) col_9i = out_7g->get_col<1>();
decltype(auto) col_10i = out_7g->get_col<2>();
uint32_t len_11k = stocksymbol_2b.size;
typedef record<decays<decltype(stocksymbol_2b)>::value_t> record_type12l;
auto g13m = HashTableFactory<record_type12l, transTypes<record_type12l, hasher>>::get<decays<decltype(stocksymbol_2b)>>(stocksymbol_2b);
auto sz_g13m = g13m.size;
auto vecs_14n = g13m.values;
col_8h.resize(sz_g13m);
col_9i.resize(sz_g13m);
col_10i.resize(sz_g13m);
auto& rt_calls = aq::dev::Runtime::get();
const size_t ge_before = rt_calls.grouped_ewise_calls, fb_before = rt_calls.scalar_fallbacks, gc_before = rt_calls.grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i15 = 0; i15 < sz_g13m; ++i15) {
auto &key_16o = (*g13m.keys)[i15];
auto &val_17p = vecs_14n[i15];
col_8h[i15] = (get<0>(key_16o));

col_9i[i15] = (max((maxs(price_3c[val_17p]) - min(price_3c[val_17p]))));

col_10i[i15] = (last((avgw(3, price_3c[val_17p]) - avg(price_3c[val_17p]))));

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("gs_flat.out", *out_7g);
{ FILE* f = fopen("gs_flat.calls", "w"); fprintf(f, "%zu %zu %zu %u\n", rt_calls.grouped_ewise_calls - ge_before, rt_calls.scalar_fallbacks - fb_before, rt_calls.grouped_calls - gc_before, (unsigned)sz_g13m); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_gs_cov(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto stocksymbol_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto price_3c = ColRef<int>(len_1a, server->getCol(aq_value_col(server), types::Type_t::AINT32));
const char* names_6f[] = {"stocksymbol", "c0"};
auto out_7g = new TableInfo<int,value_type<decays<decltype(covariance(price_3c, price_3c))>>>("out_7g", names_6f);
decltype(auto) col_8h = out_7g->get_col<0>();
decltype(auto) col_9i = out_7g->get_col<1>();
uint32_t len_11k = stocksymbol_2b.size;
typedef record<decays<decltype(stocksymbol_2b)>::value_t> record_type12l;
auto g13m = HashTableFactory<record_type12l, transTypes<record_type12l, hasher>>::get<decays<decltype(stocksymbol_2b)>>(stocksymbol_2b);
auto sz_g13m = g13m.size;
auto vecs_14n = g13m.values;
col_8h.resize(sz_g13m);
col_9i.resize(sz_g13m);
auto& rt_calls = aq::dev::Runtime::get();
const size_t ge_before = rt_calls.grouped_ewise_calls, fb_before = rt_calls.scalar_fallbacks, gc_before = rt_calls.grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i15 = 0; i15 < sz_g13m; ++i15) {
auto &key_16o = (*g13m.keys)[i15];
auto &val_17p = vecs_14n[i15];
col_8h[i15] = (get<0>(key_16o));

col_9i[i15] = (covariance(price_3c[val_17p], price_3c[val_17p]));

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("gs_cov.out", *out_7g);
{ FILE* f = fopen("gs_cov.calls", "w"); fprintf(f, "%zu %zu %zu %u\n", rt_calls.grouped_ewise_calls - ge_before, rt_calls.scalar_fallbacks - fb_before, rt_calls.grouped_calls - gc_before, (unsigned)sz_g13m); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_gs_derived(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto stocksymbol_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto price_3c = ColRef<int>(len_1a, server->getCol(aq_value_col(server), types::Type_t::AINT32));
const char* names_6f[] = {"stocksymbol", "c0"};
auto out_7g = new TableInfo<int,value_type<decays<decltype(sum((price_3c - (max(price_3c) - min(price_3c)))))>>>("out_7g", names_6f);
decltype(auto) col_8h = out_7g->get_col<0>();
decltype(auto) col_9i = out_7g->get_col<1>();
uint32_t len_11k = stocksymbol_2b.size;
typedef record<decays<decltype(stocksymbol_2b)>::value_t> record_type12l;
auto g13m = HashTableFactory<record_type12l, transTypes<record_type12l, hasher>>::get<decays<decltype(stocksymbol_2b)>>(stocksymbol_2b);
auto sz_g13m = g13m.size;
auto vecs_14n = g13m.values;
col_8h.resize(sz_g13m);
col_9i.resize(sz_g13m);
auto& rt_calls = aq::dev::Runtime::get();
const size_t ge_before = rt_calls.grouped_ewise_calls, fb_before = rt_calls.scalar_fallbacks, gc_before = rt_calls.grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i15 = 0; i15 < sz_g13m; ++i15) {
auto &key_16o = (*g13m.keys)[i15];
auto &val_17p = vecs_14n[i15];
col_8h[i15] = (get<0>(key_16o));

col_9i[i15] = (sum((price_3c[val_17p] - (max(price_3c[val_17p]) - min(price_3c[val_17p])))));

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("gs_derived.out", *out_7g);
{ FILE* f = fopen("gs_derived.calls", "w"); fprintf(f, "%zu %zu %zu %u\n", rt_calls.grouped_ewise_calls - ge_before, rt_calls.scalar_fallbacks - fb_before, rt_calls.grouped_calls - gc_before, (unsigned)sz_g13m); fclose(f); }
puts("done.");
return 0;
}
