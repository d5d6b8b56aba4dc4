// Hand-recorded modules in the shape the reference's code generator emits (engine/ast.py:340-447 flat, :722-789 the group loop; the
// shapes of moving_avg.cpp and group_scans.cpp), over host_main's `synthetic` dataset (a, b, c, d): the moving order statistics.
//   dll_wq_flat   SELECT medianw(5, price) FROM source                                             one aqg_window_quantiles
//   dll_wq_group  SELECT a, medianw(5, c), quantilew(20, 9, 10, c + a) FROM source GROUP BY a      per-group windows into flat buffers: ONE
//                                                                                                  aqg_grouped_window_quantiles_flat each
//   dll_wq_wide   SELECT medianw(1100, price) FROM source                                          a window beyond AQG_WINQ_MAX_W: the header
//                                                                                                  layer's host loop (the slow path)
// dll_wq_group writes, next to the dumped columns, how many grouped window-quantile calls the loop cost (wqg.calls: calls, groups).
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"

__AQEXPORT__(int) dll_wq_flat(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto price_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"medianw5yprice"};
auto out_5e = new TableInfo<value_type<decays<decltype(medianw(5, price_3c))>>>("out_5e", names_4d);
out_5e->get_col<0>().initfrom(medianw(5, price_3c), "medianw5yprice");
aqtest::dump_table("wqf.out", *out_5e);
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_wq_wide(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto price_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"medianw1100yprice"};
auto out_5e = new TableInfo<value_type<decays<decltype(medianw(1100, price_3c))>>>("out_5e", names_4d);
out_5e->get_col<0>().initfrom(medianw(1100, price_3c), "medianw1100yprice");
aqtest::dump_table("wqw.out", *out_5e);
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_wq_group(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto a_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"a", "medianw5yc", "quantilew20y9y10"};
auto out_5e = new TableInfo<int,vector_type<value_type<decays<decltype(medianw(5, c_3c))>>>,vector_type<value_type<decays<decltype(quantilew(20, 9, 10, (c_3c + a_2b)))>>>>("out_5e", names_4d);
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
typedef value_type<decays<decltype(medianw(5, c_3c))>> elem_7g;
typedef value_type<decays<decltype(quantilew(20, 9, 10, (c_3c + a_2b)))>> elem_8h;
auto buf_col_7g = static_cast<elem_7g *>(calloc(len_9i, sizeof(elem_7g)));
auto buf_col_8h = static_cast<elem_8h *>(calloc(len_9i, sizeof(elem_8h)));
for (uint32_t i12 = 0; i12 < sz_g11k; ++i12) {
col_7g[i12].init_from(vecs_12l[i12].size, buf_col_7g + g11k.offsets[i12]);
col_8h[i12].init_from(vecs_12l[i12].size, buf_col_8h + g11k.offsets[i12]);
}
const size_t calls_before = aq::dev::Runtime::get().grouped_window_quantile_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i13 = 0; i13 < sz_g11k; ++i13) {
auto &key_14m = (*g11k.keys)[i13];
auto &val_15n = vecs_12l[i13];
col_6f[i13] = (get<0>(key_14m));

medianw(5, c_3c[val_15n], col_7g[i13]);

quantilew(20, 9, 10, (c_3c[val_15n] + a_2b[val_15n]), col_8h[i13]);

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table("wqg.out", *out_5e);
{ FILE* f = fopen("wqg.calls", "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_window_quantile_calls - calls_before, (unsigned)sz_g11k); fclose(f); }
puts("done.");
return 0;
}
