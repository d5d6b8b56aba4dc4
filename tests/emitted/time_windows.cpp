// Hand-recorded modules in the shape the reference's code generator emits (engine/ast.py:340-447 flat, :722-789 the group loop; the
// shape of ema.cpp), over host_main's `synthetic` dataset (a, b, c, d): the time-range windows.
//   dll_tw_flat     SELECT sumr(40, t, c), maxr(40, t, c), countr(40, t) FROM source                        three aqg_rangew
//   dll_tw_group    SELECT a, sumr(40, t, c), maxr(40, t, c), countr(40, t), sumr(40, subvec(t, 0, 2), subvec(c, 0, 2)) FROM source GROUP BY a
//                   per-group results into flat buffers: ONE bounds search and ONE fold per aggregate for all groups, whatever their
//                   number; the views of two rows are shorter than their group and take the per-group path
//   dll_tw_group10  the same grouped by a % 10
// `t` is a time column made here (an ascending walk with steps 1 + c % 5; tw.t holds it).  dll_tw_group* write, next to the dumped
// columns, what the loop cost (twg.calls: bounds calls, fold calls, groups).
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"
#include <vector>

typedef types::GetLongType<int> tw_long_t;

static std::vector<int>& tw_times(Context* cxt, int slot) {
	static std::vector<int> hosts[3];
	auto server = static_cast<DataSource*>(cxt->curr_server);
	const int* c_raw = static_cast<const int*>(server->getCol(2, types::Type_t::AINT32));
	std::vector<int>& t_host = hosts[slot];
	t_host.resize(server->cnt);
	int walk = 0;
	for (uint32_t i = 0; i < server->cnt; ++i) { walk += 1 + c_raw[i] % 5; t_host[i] = walk; }
	return t_host;
}

__AQEXPORT__(int) dll_tw_flat(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
std::vector<int>& t_host = tw_times(cxt, 2);
{ FILE* f = fopen("tw.t", "wb"); fwrite(t_host.data(), 4, len_1a, f); fclose(f); }
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
auto t_4t = ColRef<int>(len_1a, t_host.data());
const char* names_4d[] = {"sumr40ytyc", "maxr40ytyc", "countr40yt"};
auto out_5e = new TableInfo<value_type<decays<decltype(sumr(40, t_4t, c_3c))>>,value_type<decays<decltype(maxr(40, t_4t, c_3c))>>,value_type<decays<decltype(countr(40, t_4t))>>>("out_5e", names_4d);
out_5e->get_col<0>().initfrom(sumr(40, t_4t, c_3c), "sumr40ytyc");
out_5e->get_col<1>().initfrom(maxr(40, t_4t, c_3c), "maxr40ytyc");
out_5e->get_col<2>().initfrom(countr(40, t_4t), "countr40yt");
aqtest::dump_table("twf.out", *out_5e);
puts("done.");
return 0;
}

static int tw_group(Context* cxt, int modulus, const char* out_name, const char* calls_name) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
// (a borrowed column is mirrored on the device by host address and assumed immutable: each grouping keeps columns of its own)
static std::vector<int> key_hosts[2];
std::vector<int> &key_host = key_hosts[modulus == 10], &t_host = tw_times(cxt, modulus == 10);
const int* a_raw = static_cast<const int*>(server->getCol(0, types::Type_t::AINT32));
key_host.resize(len_1a);
for (uint32_t i = 0; i < len_1a; ++i) key_host[i] = a_raw[i] % modulus;
auto a_2b = ColRef<int>(len_1a, key_host.data());
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
auto t_4t = ColRef<int>(len_1a, t_host.data());
const char* names_4d[] = {"a", "sumr40ytyc", "maxr40ytyc", "countr40yt", "sumr40ysub"};
auto out_5e = new TableInfo<int,vector_type<tw_long_t>,vector_type<int>,vector_type<uint32_t>,vector_type<tw_long_t>>("out_5e", names_4d);
decltype(auto) col_6f = out_5e->get_col<0>();
decltype(auto) col_7g = out_5e->get_col<1>();
decltype(auto) col_8h = out_5e->get_col<2>();
decltype(auto) col_9s = out_5e->get_col<4>();
decltype(auto) col_10d = out_5e->get_col<3>();
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
auto buf_col_7g = static_cast<tw_long_t *>(calloc(len_9i, sizeof(tw_long_t)));
auto buf_col_8h = static_cast<int *>(calloc(len_9i, sizeof(int)));
auto buf_col_10d = static_cast<uint32_t *>(calloc(len_9i, sizeof(uint32_t)));
auto buf_col_9s = static_cast<tw_long_t *>(calloc(2 * (size_t)sz_g11k, sizeof(tw_long_t)));
for (uint32_t i12 = 0; i12 < sz_g11k; ++i12) {
col_7g[i12].init_from(vecs_12l[i12].size, buf_col_7g + g11k.offsets[i12]);
col_8h[i12].init_from(vecs_12l[i12].size, buf_col_8h + g11k.offsets[i12]);
col_10d[i12].init_from(vecs_12l[i12].size, buf_col_10d + g11k.offsets[i12]);
col_9s[i12].init_from(vecs_12l[i12].size < 2 ? vecs_12l[i12].size : 2, buf_col_9s + 2 * (size_t)i12);
}
const size_t bounds_before = aq::dev::Runtime::get().grouped_rangew_bounds_calls, folds_before = aq::dev::Runtime::get().grouped_rangew_fold_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i13 = 0; i13 < sz_g11k; ++i13) {
auto &key_14m = (*g11k.keys)[i13];
auto &val_15n = vecs_12l[i13];
col_6f[i13] = (get<0>(key_14m));

sumr(40, t_4t[val_15n], c_3c[val_15n], col_7g[i13]);

maxr(40, t_4t[val_15n], c_3c[val_15n], col_8h[i13]);

countr(40, t_4t[val_15n], col_10d[i13]);

sumr(40, t_4t[val_15n].subvec(0, col_9s[i13].size), c_3c[val_15n].subvec(0, col_9s[i13].size), col_9s[i13]);

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table(out_name, *out_5e);
{ FILE* f = fopen(calls_name, "w"); fprintf(f, "%zu %zu %u\n", aq::dev::Runtime::get().grouped_rangew_bounds_calls - bounds_before,
                                            aq::dev::Runtime::get().grouped_rangew_fold_calls - folds_before, (unsigned)sz_g11k); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_tw_group(Context* cxt) { return tw_group(cxt, 1 << 30, "twg.out", "twg.calls"); }
__AQEXPORT__(int) dll_tw_group10(Context* cxt) { return tw_group(cxt, 10, "twg10.out", "twg10.calls"); }
