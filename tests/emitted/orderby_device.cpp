// Emitted shape of `SELECT a, b, c FROM t ORDER BY a DESC, b DESC, c` over about 1e6 rows (server/table.h:447-465 order_by, then
// materialize_copy): `order_by<-1, -2, 2>` over long / unsigned int / double columns with many ties.  All three types have device
// tags, so the order comes from one aqg_sort_rows call; the module prints the digit passes it ran (0 would mean the host sort) and
// dumps the input table, the ids and the sorted table for tests/test_gpu_orderby_device.py.  Then it rewrites the ids on the host and
// materialises through them again: that gather must see the new ids.
#include "header.cxx"
#include "./server/monetdb_conn.h"
#include "./server/aggregations.h"
#include "./server/hasher.h"
#include "dump_cols.h"

__AQEXPORT__(int) dll_orderby_device(Context* cxt) {
	using namespace std;
	using namespace types;
const uint32_t n = 1000003;
const char* names_1[] = {"a", "b", "c"};
auto t_2 = new TableInfo<long, unsigned int, double>("t_2", names_1);
t_2->get_col<0>().resize(n);
t_2->get_col<1>().resize(n);
t_2->get_col<2>().resize(n);
unsigned long long x = 987654321;
for (uint32_t i = 0; i < n; ++i) {
	x = x * 6364136223846793005ull + 1442695040888963407ull;
	t_2->get_col<0>()[i] = (long)((x >> 33) % 1000) - 500;                     // clear of LONG_MIN: -a is defined
	const unsigned r = (unsigned)(x >> 20);
	t_2->get_col<1>()[i] = r % 5 == 0 ? 0u : r % 5 == 1 ? 4294967295u - r % 3 : r % 40;
	t_2->get_col<2>()[i] = (x >> 45) % 3 == 0 ? -0.0 : ((double)((x >> 50) % 7) - 3.0) * 0.5;
}
auto ord_3 = t_2->order_by<-1, -2, 2>();
uint32_t passes_4 = 0;
aqg_sort_last_passes(aq::dev::Runtime::get().ctx(), &passes_4);
auto sorted_5 = t_2->materialize_copy(*ord_3);
printf("rows %u\n", ord_3->size);
printf("passes %u\n", passes_4);
aqtest::dump_table("orderby_in", *t_2);
aqtest::dump_table("orderby_sorted", *sorted_5);
FILE* f_6 = fopen("orderby_ids", "wb");
fwrite(ord_3->begin(), 4, ord_3->size, f_6);
fclose(f_6);
// the ids belong to the module: rewritten on the host, the next gather through them must see the new ids, not a device copy of the old
std::reverse(ord_3->begin(), ord_3->end());
(*ord_3)[0] = 7;
auto rev_7 = t_2->materialize_copy(*ord_3);
aqtest::dump_table("orderby_rev", *rev_7);
puts("done.");
return 0;
}
