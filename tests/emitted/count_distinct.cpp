// Hand-recorded modules in the shape the reference's code generator emits for count(distinct x), over host_main's `h2o9` dataset
// (id2, id4, v1, v2).  The generator spells it `(x).distinct_size()` (common/types.py:271-277: count_behavior); under GROUP BY the
// column becomes `x[val]` inside the group loop of engine/ast.py:722-789, and a projection without GROUP BY binds the scalar with
// `out->get_col<k>().initfrom(<expr>, "name")` (engine/ast.py:440-447).
//   dll_cd       SELECT id2, id4, count(distinct v1) FROM source GROUP BY id2, id4               a table column: aqg_grouped_count_distinct
//   dll_cd_expr  SELECT id2, id4, count(distinct (v1 * 0.5 + v2)) FROM source GROUP BY id2, id4  a virtual per-group column: aqg_grouped_count_distinct_flat
//   dll_cd_flat  SELECT count(distinct v2) FROM source                                          the whole column: aqg_count_distinct
// The grouped ones write, next to the dumped columns, how many grouped calls the loop cost (<out>.calls: calls, groups).
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"

__AQEXPORT__(int) dll_cd(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto id2_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto id4_3c = ColRef<int>(len_1a, server->getCol(1, types::Type_t::AINT32));
auto v1_4d = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
auto v2_5e = ColRef<int>(len_1a, server->getCol(3, types::Type_t::AINT32));
const char* names_6f[] = {"id2", "id4", "cd_v1"};
auto out_7g = new TableInfo<int,int,value_type<decays<decltype((v1_4d).distinct_size())>>>("out_7g", names_6f);
decltype(auto) col_8h = out_7g->get_col<0>();
decltype(auto) col_9i = out_7g->get_col<1>();
decltype(auto) col_10j = out_7g->get_col<2>();
uint32_t len_11k = id2_2b.size;
typedef record<decays<decltype(id2_2b)>::value_t,decays<decltype(id4_3c)>::value_t> record_type12l;
auto g13m = HashTableFactory<record_type12l, transTypes<record_type12l, hasher>>::get<decays<decltype(id2_2b)>, decays<decltype(id4_3c)>>(id2_2b, id4_3c);
auto sz_g13m = g13m.size;
auto vecs_14n = g13m.values;
col_8h.resize(sz_g13m);
col_9i.resize(sz_g13m);
col_10j.resize(sz_g13m);
const size_t calls_before = aq::dev::Runtime::get().grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i15 = 0; i15 < sz_g13m; ++i15) {
auto &key_16o = (*g13m.keys)[i15];
auto &val_17p = vecs_14n[i15];
col_8h[i15] = (get<0>(key_16o));

col_9i[i15] = (get<1>(key_16o));

col_10j[i15] = ((v1_4d[val_17p]).distinct_size());

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("cd.out", *out_7g);
{ FILE* f = fopen("cd.calls", "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_calls - calls_before, (unsigned)sz_g13m); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_cd_expr(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto id2_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto id4_3c = ColRef<int>(len_1a, server->getCol(1, types::Type_t::AINT32));
auto v1_4d = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
auto v2_5e = ColRef<int>(len_1a, server->getCol(3, types::Type_t::AINT32));
const char* names_6f[] = {"id2", "id4", "cd_e"};
auto out_7g = new TableInfo<int,int,value_type<decays<decltype((((v1_4d * 0.5f) + v2_5e)).distinct_size())>>>("out_7g", names_6f);
decltype(auto) col_8h = out_7g->get_col<0>();
decltype(auto) col_9i = out_7g->get_col<1>();
decltype(auto) col_10j = out_7g->get_col<2>();
uint32_t len_11k = id2_2b.size;
typedef record<decays<decltype(id2_2b)>::value_t,decays<decltype(id4_3c)>::value_t> record_type12l;
auto g13m = HashTableFactory<record_type12l, transTypes<record_type12l, hasher>>::get<decays<decltype(id2_2b)>, decays<decltype(id4_3c)>>(id2_2b, id4_3c);
auto sz_g13m = g13m.size;
auto vecs_14n = g13m.values;
col_8h.resize(sz_g13m);
col_9i.resize(sz_g13m);
col_10j.resize(sz_g13m);
const size_t calls_before = aq::dev::Runtime::get().grouped_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i15 = 0; i15 < sz_g13m; ++i15) {
auto &key_16o = (*g13m.keys)[i15];
auto &val_17p = vecs_14n[i15];
col_8h[i15] = (get<0>(key_16o));

col_9i[i15] = (get<1>(key_16o));

col_10j[i15] = ((((v1_4d[val_17p] * 0.5f) + v2_5e[val_17p])).distinct_size());

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("cde.out", *out_7g);
{ FILE* f = fopen("cde.calls", "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_calls - calls_before, (unsigned)sz_g13m); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_cd_flat(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto v2_5e = ColRef<int>(len_1a, server->getCol(3, types::Type_t::AINT32));
const char* names_6f[] = {"cd_v2"};
auto out_7g = new TableInfo<value_type<decays<decltype((v2_5e).distinct_size())>>>("out_7g", names_6f);
out_7g->get_col<0>().initfrom((v2_5e).distinct_size(), "cd_v2");
aqtest::dump_table("cdf.out", *out_7g);
puts("done.");
return 0;
}
