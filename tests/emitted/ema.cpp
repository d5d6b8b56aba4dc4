// Hand-recorded modules in the shape the reference's code generator emits (engine/ast.py:340-447 flat, :722-789 the group loop; the
// shapes of moving_avg.cpp and window_quantiles.cpp), over host_main's `synthetic` dataset (a, b, c, d): the exponential moving averages.
//   dll_ema_flat     SELECT ema(0.25, c), ewma(0.25, c) FROM source                                       two aqg_scan_ema
//   dll_ema_group    SELECT a, ema(0.25, c), ewmad(decayt(40, t), c), ema(0.25, subvec(c, 0, 2)), decayt(40, t) FROM source GROUP BY a
//                    per-group results into flat buffers: ONE aqg_grouped_ema_flat for each of the first two, whatever the number of
//                    groups; the view of two rows is shorter than its group and takes the per-group path
//   dll_ema_group10  the same grouped by a % 10
// `t` is a time column made here (an ascending walk with steps 1 + c % 5; ema.t holds it).  dll_ema_group* write, next to the dumped
// columns, how many aqg_grouped_ema_flat calls the loop cost (emag.calls: calls, groups).
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"
#include <vector>

__AQEXPORT__(int) dll_ema_flat(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"ema025yc", "ewma025yc"};
auto out_5e = new TableInfo<value_type<decays<decltype(ema(0.25, c_3c))>>,value_type<decays<decltype(ewma(0.25, c_3c))>>>("out_5e", names_4d);
out_5e->get_col<0>().initfrom(ema(0.25, c_3c), "ema025yc");
out_5e->get_col<1>().initfrom(ewma(0.25, c_3c), "ewma025yc");
aqtest::dump_table("emaf.out", *out_5e);
puts("done.");
return 0;
}

static int ema_group(Context* cxt, int modulus, const char* out_name, const char* calls_name) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
// (a borrowed column is mirrored on the device by host address and assumed immutable: each grouping keeps columns of its own)
static std::vector<int> key_hosts[2], t_hosts[2];
std::vector<int> &key_host = key_hosts[modulus == 10], &t_host = t_hosts[modulus == 10];
const int* a_raw = static_cast<const int*>(server->getCol(0, types::Type_t::AINT32));
const int* c_raw = static_cast<const int*>(server->getCol(2, types::Type_t::AINT32));
key_host.resize(len_1a); t_host.resize(len_1a);
int walk = 0;
for (uint32_t i = 0; i < len_1a; ++i) { key_host[i] = a_raw[i] % modulus; walk += 1 + c_raw[i] % 5; t_host[i] = walk; }
{ FILE* f = fopen("ema.t", "wb"); fwrite(t_host.data(), 4, len_1a, f); fclose(f); }
auto a_2b = ColRef<int>(len_1a, key_host.data());
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
auto t_4t = ColRef<int>(len_1a, t_host.data());
const char* names_4d[] = {"a", "ema025yc", "ewmadyc", "ema025ysub", "decay40yt"};
auto out_5e = new TableInfo<int,vector_type<double>,vector_type<double>,vector_type<double>,vector_type<double>>("out_5e", names_4d);
decltype(auto) col_6f = out_5e->get_col<0>();
decltype(auto) col_7g = out_5e->get_col<1>();
decltype(auto) col_8h = out_5e->get_col<2>();
decltype(auto) col_9s = out_5e->get_col<3>();
decltype(auto) col_10d = out_5e->get_col<4>();
uint32_t len_9i = a_2b.size;
typedef record<decays<decltype(a_2b)>::value_t> record_type10j;
auto g11k = HashTableFactory<record_type10j, transTypes<record_type10j, hasher>>::get<decays<decltype(a_2b)>>(a_2b);
auto sz_g11k = g11k.size;
auto vecs_12l = g11k.values;
col_6f.resize(sz_g11k);
col_7g.resize(sz_g11k);
col_8h.resize(sz_g11k);
col_9s.resize(sz_g11k);
col_10d.resize(sz_g11k);
auto buf_col_7g = static_cast<double *>(calloc(len_9i, sizeof(double)));
auto buf_col_8h = static_cast<double *>(calloc(len_9i, sizeof(double)));
auto buf_col_10d = static_cast<double *>(calloc(len_9i, sizeof(double)));
auto buf_col_9s = static_cast<double *>(calloc(2 * (size_t)sz_g11k, sizeof(double)));
for (uint32_t i12 = 0; i12 < sz_g11k; ++i12) {
col_7g[i12].init_from(vecs_12l[i12].size, buf_col_7g + g11k.offsets[i12]);
col_8h[i12].init_from(vecs_12l[i12].size, buf_col_8h + g11k.offsets[i12]);
col_10d[i12].init_from(vecs_12l[i12].size, buf_col_10d + g11k.offsets[i12]);
col_9s[i12].init_from(vecs_12l[i12].size < 2 ? vecs_12l[i12].size : 2, buf_col_9s + 2 * (size_t)i12);
}
const size_t calls_before = aq::dev::Runtime::get().grouped_ema_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i13 = 0; i13 < sz_g11k; ++i13) {
auto &key_14m = (*g11k.keys)[i13];
auto &val_15n = vecs_12l[i13];
col_6f[i13] = (get<0>(key_14m));

ema(0.25, c_3c[val_15n], col_7g[i13]);

ewmad(decayt(40, t_4t[val_15n]), c_3c[val_15n], col_8h[i13]);

ema(0.25, c_3c[val_15n].subvec(0, col_9s[i13].size), col_9s[i13]);

decayt(40, t_4t[val_15n], col_10d[i13]);

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table(out_name, *out_5e);
{ FILE* f = fopen(calls_name, "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_ema_calls - calls_before, (unsigned)sz_g11k); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_ema_group(Context* cxt) { return ema_group(cxt, 1 << 30, "emag.out", "emag.calls"); }
__AQEXPORT__(int) dll_ema_group10(Context* cxt) { return ema_group(cxt, 10, "emag10.out", "emag10.calls"); }
