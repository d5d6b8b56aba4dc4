// Hand-recorded modules in the shape the reference's code generator emits for an aggregate under GROUP BY (engine/ast.py:722-789; the loop
// of median_q6.cpp and topk_q8.cpp), over host_main's `synthetic` dataset (a, b, c, d): the percentile questions a median cannot answer.
//   dll_qt        SELECT a, quantile(95, 100, c), quantile(1, 4, c) FROM source GROUP BY a      a table column: two aqg_grouped_quantiles
//   dll_qt_multi  SELECT a, quantiles(100, {5, 50, 95}, c + a) FROM source GROUP BY a           a virtual per-group column: ONE
//                                                                                               aqg_grouped_quantiles_flat for three ranks
// Both write, next to the dumped columns, how many grouped calls the loop cost (<out>.calls: calls, groups).
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"

__AQEXPORT__(int) dll_qt(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto a_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"a", "p95", "q1"};
auto out_5e = new TableInfo<int,value_type<decays<decltype(quantile(95, 100, c_3c))>>,value_type<decays<decltype(quantile(1, 4, c_3c))>>>("out_5e", names_4d);
decltype(auto) col_6f = out_5e->get_col<0>();
decltype(auto) col_7g = out_5e->get_col<1>();
decltype(auto) col_8h = out_5e->get_col<2>();
uint32_t len_9i = a_2b.size;
typedef record<decays<decltype(a_2b)>::value_t> record_type10j;
auto g11k = HashTableFactory<record_type10j, transTypes<record_type10j, hasher>>::get<decays<decltype(a_2b)>>(a_2b);
auto sz_g11k = g11k.size;
auto vecs_12l = g11k.values;
col_6f.resize(sz_g11k);
col_7g.resize(sz_g11k);
col_8h.resize(sz_g11k);
const size_t calls_before = aq::dev::Runtime::get().grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i13 = 0; i13 < sz_g11k; ++i13) {
auto &key_14m = (*g11k.keys)[i13];
auto &val_15n = vecs_12l[i13];
col_6f[i13] = (get<0>(key_14m));

col_7g[i13] = (quantile(95, 100, c_3c[val_15n]));

col_8h[i13] = (quantile(1, 4, c_3c[val_15n]));

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("qt.out", *out_5e);
{ FILE* f = fopen("qt.calls", "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_calls - calls_before, (unsigned)sz_g11k); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_qt_multi(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto a_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"a", "e"};
auto out_5e = new TableInfo<int,vector_type<value_type<decays<decltype(quantiles(100, {5, 50, 95}, (c_3c + a_2b)))>>>>("out_5e", names_4d);
decltype(auto) col_6f = out_5e->get_col<0>();
decltype(auto) col_7g = out_5e->get_col<1>();
uint32_t len_9i = a_2b.size;
typedef record<decays<decltype(a_2b)>::value_t> record_type10j;
auto g11k = HashTableFactory<record_type10j, transTypes<record_type10j, hasher>>::get<decays<decltype(a_2b)>>(a_2b);
auto sz_g11k = g11k.size;
auto vecs_12l = g11k.values;
col_6f.resize(sz_g11k);
col_7g.resize(sz_g11k);
const size_t calls_before = aq::dev::Runtime::get().grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i13 = 0; i13 < sz_g11k; ++i13) {
auto &key_14m = (*g11k.keys)[i13];
auto &val_15n = vecs_12l[i13];
col_6f[i13] = (get<0>(key_14m));

col_7g[i13] = (quantiles(100, {5, 50, 95}, (c_3c[val_15n] + a_2b[val_15n])));

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("qtm.out", *out_5e);
{ FILE* f = fopen("qtm.calls", "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_calls - calls_before, (unsigned)sz_g11k); fclose(f); }
puts("done.");
return 0;
}
