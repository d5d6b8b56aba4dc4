// Hand-recorded modules in the shape the reference's code generator emits (engine/ast.py:340-447 flat, :722-789 the group loop; the
// shapes of moving_avg.cpp and ema.cpp), over host_main's `synthetic` dataset (a, b, c, d): the ranking functions.
//   dll_rank_flat     SELECT rankof(c), avg_rank(c), ntile(7, c), row_number(c, true) FROM source              four aqg_rank
//   dll_rank_group    SELECT a, rankof(c), dense_rank(c, true), percent_rank(c), ntile(4, c), rankof(subvec(c, 0, 2)), rankof(c) FROM source GROUP BY a
//                     per-group results into flat buffers: ONE aqg_grouped_rank_flat per (column, method, order) -- four here, the
//                     repeated rankof(c) is the first one's result -- whatever the number of groups; the view of two rows is shorter
//                     than its group and takes the per-group path
//   dll_rank_group10  the same grouped by a % 10
// dll_rank_group* write, next to the dumped columns, how many aqg_grouped_rank_flat calls the loop cost (rankg.calls: calls, groups).
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"
#include <vector>

__AQEXPORT__(int) dll_rank_flat(Context* cxt) {
	using namespace std;
	using namespace types;
	auto server = static_cast<DataSource*>(cxt->curr_server);
auto len_1a = server->cnt;
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"rankyc", "avgrankyc", "ntile7yc", "rownumberdyc"};
auto out_5e = new TableInfo<value_type<decays<decltype(rankof(c_3c))>>,value_type<decays<decltype(avg_rank(c_3c))>>,value_type<decays<decltype(ntile(7, c_3c))>>,value_type<decays<decltype(row_number(c_3c, true))>>>("out_5e", names_4d);
out_5e->get_col<0>().initfrom(rankof(c_3c), "rankyc");
out_5e->get_col<1>().initfrom(avg_rank(c_3c), "avgrankyc");
out_5e->get_col<2>().initfrom(ntile(7, c_3c), "ntile7yc");
out_5e->get_col<3>().initfrom(row_number(c_3c, true), "rownumberdyc");
aqtest::dump_table("rankf.out", *out_5e);
puts("done.");
return 0;
}

static int rank_group(Context* cxt, int modulus, const char* out_name, const char* calls_name) {
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
auto a_2b = ColRef<int>(len_1a, key_host.data());
auto c_3c = ColRef<int>(len_1a, server->getCol(2, types::Type_t::AINT32));
const char* names_4d[] = {"a", "rankyc", "denserankdyc", "percentrankyc", "ntile4yc", "rankysub", "rankyc2"};
auto out_5e = new TableInfo<int,vector_type<uint32_t>,vector_type<uint32_t>,vector_type<double>,vector_type<uint32_t>,vector_type<uint32_t>,vector_type<uint32_t>>("out_5e", names_4d);
decltype(auto) col_6f = out_5e->get_col<0>();
decltype(auto) col_7g = out_5e->get_col<1>();
decltype(auto) col_8h = out_5e->get_col<2>();
decltype(auto) col_9p = out_5e->get_col<3>();
decltype(auto) col_10n = out_5e->get_col<4>();
decltype(auto) col_11s = out_5e->get_col<5>();
decltype(auto) col_12r = out_5e->get_col<6>();
uint32_t len_9i = a_2b.size;
typedef record<decays<decltype(a_2b)>::value_t> record_type10j;
auto g11k = HashTableFactory<record_type10j, transTypes<record_type10j, hasher>>::get<decays<decltype(a_2b)>>(a_2b);
auto sz_g11k = g11k.size;
auto vecs_12l = g11k.values;
col_6f.resize(sz_g11k);
col_7g.resize(sz_g11k);
col_8h.resize(sz_g11k);
col_9p.resize(sz_g11k);
col_10n.resize(sz_g11k);
col_11s.resize(sz_g11k);
col_12r.resize(sz_g11k);
auto buf_col_7g = static_cast<uint32_t *>(calloc(len_9i, sizeof(uint32_t)));
auto buf_col_8h = static_cast<uint32_t *>(calloc(len_9i, sizeof(uint32_t)));
auto buf_col_9p = static_cast<double *>(calloc(len_9i, sizeof(double)));
auto buf_col_10n = static_cast<uint32_t *>(calloc(len_9i, sizeof(uint32_t)));
auto buf_col_12r = static_cast<uint32_t *>(calloc(len_9i, sizeof(uint32_t)));
auto buf_col_11s = static_cast<uint32_t *>(calloc(2 * (size_t)sz_g11k, sizeof(uint32_t)));
for (uint32_t i12 = 0; i12 < sz_g11k; ++i12) {
col_7g[i12].init_from(vecs_12l[i12].size, buf_col_7g + g11k.offsets[i12]);
col_8h[i12].init_from(vecs_12l[i12].size, buf_col_8h + g11k.offsets[i12]);
col_9p[i12].init_from(vecs_12l[i12].size, buf_col_9p + g11k.offsets[i12]);
col_10n[i12].init_from(vecs_12l[i12].size, buf_col_10n + g11k.offsets[i12]);
col_12r[i12].init_from(vecs_12l[i12].size, buf_col_12r + g11k.offsets[i12]);
col_11s[i12].init_from(vecs_12l[i12].size < 2 ? vecs_12l[i12].size : 2, buf_col_11s + 2 * (size_t)i12);
}
const size_t calls_before = aq::dev::Runtime::get().grouped_rank_calls;
GC::scratch_space = GC::gc_handle ? &(GC::gc_handle->scratch) : nullptr;
for (uint32_t i13 = 0; i13 < sz_g11k; ++i13) {
auto &key_14m = (*g11k.keys)[i13];
auto &val_15n = vecs_12l[i13];
col_6f[i13] = (get<0>(key_14m));

rankof(c_3c[val_15n], col_7g[i13]);

dense_rank(c_3c[val_15n], col_8h[i13], true);

percent_rank(c_3c[val_15n], col_9p[i13]);

ntile(4, c_3c[val_15n], col_10n[i13]);

rankof(c_3c[val_15n].subvec(0, col_11s[i13].size), col_11s[i13]);

rankof(c_3c[val_15n], col_12r[i13]);

GC::scratch_space->release();
}
GC::scratch_space = nullptr;
aqtest::dump_table(out_name, *out_5e);
{ FILE* f = fopen(calls_name, "w"); fprintf(f, "%zu %u\n", aq::dev::Runtime::get().grouped_rank_calls - calls_before, (unsigned)sz_g11k); fclose(f); }
puts("done.");
return 0;
}

__AQEXPORT__(int) dll_rank_group(Context* cxt) { return rank_group(cxt, 1 << 30, "rankg.out", "rankg.calls"); }
__AQEXPORT__(int) dll_rank_group10(Context* cxt) { return rank_group(cxt, 10, "rankg10.out", "rankg10.calls"); }
