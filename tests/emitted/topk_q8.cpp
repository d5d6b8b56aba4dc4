// Hand-recorded modules in the shape the reference's code generator emits for a vector-valued aggregate under GROUP BY (engine/ast.py:722-789;
// the same loop as group_scans.cpp's dll_q8, whose `subvec(v3,0,2)` is what benchmark/h2o/groupby.sql:16-17 writes under the comment
// `-- select top 2 from each grp`).  h2o's own Q8 asks for the LARGEST two v3 by id6: `maxk(2, v3)`.
//   dll_q8_top / dll_q8_top_c    SELECT k, maxk(2, v) FROM source GROUP BY k        a table column: aqg_grouped_topk
//   dll_q8_expr / dll_q8_expr_c  SELECT k, mink(3, v + k) FROM source GROUP BY k    a virtual per-group column: aqg_grouped_topk_flat
// k is column 0; v is column 1 (host_main's `trade` datasets: stocksymbol, price) or, for the _c entries, column 2 (`synthetic`: a, b, c, d).
// All write, next to the dumped columns, how many grouped calls the loop cost (<out>.calls: calls, groups).
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"

static int q8_top(Context* cxt, int vcol, const char* out) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto id6_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto v3_3c = ColRef<int>(len_1a, server->getCol(vcol, types::Type_t::AINT32));
const char* names_4d[] = {"id6", "v3"};
auto out_5e = new TableInfo<int,vector_type<value_type<decays<decltype(maxk(2, v3_3c))>>>>("out_5e", names_4d);
decltype(auto) col_6f = out_5e->get_col<0>();
decltype(auto) col_7g = out_5e->get_col<1>();
uint32_t len_8h = id6_2b.size;
typedef record<decays<decltype(id6_2b)>::value_t> record_type9i;
auto g10j = HashTableFactory<record_type9i, transTypes<record_type9i, hasher>>::get<decays<decltype(id6_2b)>>(id6_2b);
auto sz_g10j = g10j.size;
auto vecs_11k = g10j.values;
col_6f.resize(sz_g10j);
col_7g.resize(sz_g10j);
const size_t calls_before = aq::dev::Runtime::get().grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i13 = 0; i13 < sz_g10j; ++i13) {
auto &key_14l = (*g10j.keys)[i13];
auto &val_15m = vecs_11k[i13];
col_6f[i13] = (get<0>(key_14l));

col_7g[i13] = (maxk(2, v3_3c[val_15m]));

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table(out, *out_5e);
{ FILE* f = fopen((string(out).substr(0, string(out).size() - 4) + ".calls").c_str(), "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_calls - calls_before, (unsigned)sz_g10j); fclose(f); }
puts("done.");
return 0;
}

static int q8_expr(Context* cxt, int vcol, const char* out) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto id6_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto v3_3c = ColRef<int>(len_1a, server->getCol(vcol, types::Type_t::AINT32));
const char* names_4d[] = {"id6", "e"};
auto out_5e = new TableInfo<int,vector_type<value_type<decays<decltype(mink(3, (v3_3c + id6_2b)))>>>>("out_5e", names_4d);
decltype(auto) col_6f = out_5e->get_col<0>();
decltype(auto) col_7g = out_5e->get_col<1>();
uint32_t len_8h = id6_2b.size;
typedef record<decays<decltype(id6_2b)>::value_t> record_type9i;
auto g10j = HashTableFactory<record_type9i, transTypes<record_type9i, hasher>>::get<decays<decltype(id6_2b)>>(id6_2b);
auto sz_g10j = g10j.size;
auto vecs_11k = g10j.values;
col_6f.resize(sz_g10j);
col_7g.resize(sz_g10j);
const size_t calls_before = aq::dev::Runtime::get().grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i13 = 0; i13 < sz_g10j; ++i13) {
auto &key_14l = (*g10j.keys)[i13];
auto &val_15m = vecs_11k[i13];
col_6f[i13] = (get<0>(key_14l));

col_7g[i13] = (mink(3, (v3_3c[val_15m] + id6_2b[val_15m])));

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table(out, *out_5e);
{ FILE* f = fopen((string(out).substr(0, string(out).size() - 4) + ".calls").c_str(), "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_calls - calls_before, (unsigned)sz_g10j); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_q8_top(Context* cxt) { return q8_top(cxt, 1, "q8t.out"); }
__AQEXPORT__(int) dll_q8_top_c(Context* cxt) { return q8_top(cxt, 2, "q8t.out"); }
__AQEXPORT__(int) dll_q8_expr(Context* cxt) { return q8_expr(cxt, 1, "q8e.out"); }
__AQEXPORT__(int) dll_q8_expr_c(Context* cxt) { return q8_expr(cxt, 2, "q8e.out"); }
