// Hand-recorded modules in the shape the reference's code generator emits (engine/ast.py:340-447 flat, :722-789 the group loop; the
// shapes of ranks.cpp and ema.cpp), over host_main's `synthetic` dataset (a, b, c, d): the pair windows.
//   dll_pair_flat      SELECT corrw(20, c, a), covs(c, a), betaw(100, c, a) FROM source                          three aqg_scan2
//   dll_pair_group100  SELECT a % 100, corrw(20, c, a), covs(c, a), betaw(100, c, a), corrw(20, c, a) FROM source GROUP BY a % 100
//                      per-group results into flat buffers: ONE aqg_grouped_scan2_flat per (op, x, y, w) -- three here, the repeated
//                      corrw is the first one's result -- whatever the number of groups
//   dll_pair_group10   the same grouped by a % 10
// dll_pair_group* write, next to the dumped columns, how many aqg_grouped_scan2_flat calls the loop cost (pairg*.calls: calls, groups).
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"
#include <vector>

__AQEXPORT__(int) dll_pair_flat(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto a_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"corrw20yca", "covsyca", "betaw100yca"};
auto out_5e = new TableInfo<value_type<decays<decltype(corrw(20, c_3c, a_2b))>>,value_type<decays<decltype(covs(c_3c, a_2b))>>,value_type<decays<decltype(betaw(100, c_3c, a_2b))>>>("out_5e", names_4d);
out_5e->get_col<0>().initfrom(corrw(20, c_3c, a_2b), "corrw20yca");
out_5e->get_col<1>().initfrom(covs(c_3c, a_2b), "covsyca");
out_5e->get_col<2>().initfrom(betaw(100, c_3c, a_2b), "betaw100yca");
aqtest::dump_table("pairf.out", *out_5e);
puts("done.");
return 0;
}

static int pair_group(Context* cxt, int modulus, const char* out_name, const char* calls_name) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
// (a borrowed column is mirrored on the device by host address and assumed immutable: each grouping keeps a key column of its own)
static std::vector<int> key_hosts[2];
std::vector<int> &key_host = key_hosts[modulus == 10];
const int* a_raw = static_cast<const int*>(server->getCol(0, types::Type_t::AINT32));
key_host.resize(len_1a);
for (uint32_t i = 0; i < len_1a; ++i) key_host[i] = a_raw[i] % modulus;
auto k_1b = ColRef<int>(len_1a, key_host.data());
auto a_2b = ColRef<int>(len_1a, server->getCol(0, types::Type_t::AINT32));
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"k", "corrw20yca", "covsyca", "betaw100yca", "corrw20yca2"};
auto out_5e = new TableInfo<int,vector_type<double>,vector_type<double>,vector_type<double>,vector_type<double>>("out_5e", names_4d);
decltype(auto) col_6f = out_5e->get_col<0>();
decltype(auto) col_7g = out_5e->get_col<1>();
decltype(auto) col_8h = out_5e->get_col<2>();
decltype(auto) col_9p = out_5e->get_col<3>();
decltype(auto) col_10n = out_5e->get_col<4>();
uint32_t len_9i = k_1b.size;
typedef record<decays<decltype(k_1b)>::value_t> record_type10j;
auto g11k = HashTableFactory<record_type10j, transTypes<record_type10j, hasher>>::get<decays<decltype(k_1b)>>(k_1b);
auto sz_g11k = g11k.size;
auto vecs_12l = g11k.values;
col_6f.resize(sz_g11k);
col_7g.resize(sz_g11k);
col_8h.resize(sz_g11k);
col_9p.resize(sz_g11k);
col_10n.resize(sz_g11k);
auto buf_col_7g = static_cast<double *>(calloc(len_9i, sizeof(double)));
auto buf_col_8h = static_cast<double *>(calloc(len_9i, sizeof(double)));
auto buf_col_9p = static_cast<double *>(calloc(len_9i, sizeof(double)));
auto buf_col_10n = static_cast<double *>(calloc(len_9i, sizeof(double)));
for (uint32_t i12 = 0; i12 < sz_g11k; ++i12) {
col_7g[i12].init_from(vecs_12l[i12].size, buf_col_7g + g11k.offsets[i12]);
col_8h[i12].init_from(vecs_12l[i12].size, buf_col_8h + g11k.offsets[i12]);
col_9p[i12].init_from(vecs_12l[i12].size, buf_col_9p + g11k.offsets[i12]);
col_10n[i12].init_from(vecs_12l[i12].size, buf_col_10n + g11k.offsets[i12]);
}
const size_t calls_before = aq::dev::Runtime::get().grouped_scan2_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i13 = 0; i13 < sz_g11k; ++i13) {
auto &key_14m = (*g11k.keys)[i13];
auto &val_15n = vecs_12l[i13];
col_6f[i13] = (get<0>(key_14m));

corrw(20, c_3c[val_15n], a_2b[val_15n], col_7g[i13]);

covs(c_3c[val_15n], a_2b[val_15n], col_8h[i13]);

betaw(100, c_3c[val_15n], a_2b[val_15n], col_9p[i13]);

corrw(20, c_3c[val_15n], a_2b[val_15n], col_10n[i13]);

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table(out_name, *out_5e);
{ FILE* f = fopen(calls_name, "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_scan2_calls - calls_before, (unsigned)sz_g11k); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_pair_group100(Context* cxt) { return pair_group(cxt, 100, "pairg100.out", "pairg100.calls"); }
__AQEXPORT__(int) dll_pair_group10(Context* cxt) { return pair_group(cxt, 10, "pairg10.out", "pairg10.calls"); }
