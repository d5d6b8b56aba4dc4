// Stand-alone self-test of aquery2_amd/csrc/pair_route.hpp (the host-only route and workspace arithmetic of the pair windows), built
// with -fsanitize=address,undefined by tests/test_pair_route_host.py.  Own main, no HIP, nothing loaded into another process.
// The workspace sum is replayed through the guard's own bump allocator (ws_guard.hpp): every sub-allocation pair_window.hip makes, in
// its order, must fit the capacity ws_bytes asked for -- exactly.
#include "../aquery2_amd/csrc/pair_route.hpp"
#include "../aquery2_amd/csrc/ws_guard.hpp"
#include <cstdio>
#include <cstdlib>

using namespace aqgpair;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// the sub-allocations of one call in the order pair_window.hip makes them; returns the logical end
static size_t replay(int op, uint32_t n, uint32_t w, bool grouped, size_t carry, size_t dcarry, bool* fits) {
    ws_guard_book g;
    g.on = true;
    g.reset();
    const size_t need = ws_bytes(op, n, w, grouped, carry, dcarry);
    CHECK(g.want(need));
    size_t off = 0, phys = 0;
    *fits = true;
    auto take = [&](size_t bytes) { if (g.alloc(&off, bytes, &phys) != 0) *fits = false; };
    if (route_of(op, n, w) != ROUTE_PREFIX) return 0;
    const size_t nt = tiles_of(n);
    if (!op_running(op)) take((size_t)n * family_sums(op_family(op)) * 8);
    take(nt * carry);
    if (!op_running(op) && grouped) { take((size_t)n * 4); take(nt * dcarry); take((nt / CHUNK + 2) * dcarry); }
    CHECK(ws_guard_book::round256(off) == ws_guard_book::round256(need));        // exact: nothing asked for that is not handed out
    return off;
}

int main() {
    // routes: both sides of every switch, the clamp by the column, the running ops
    CHECK(route_of(OP_COVW, 100000, 1) == ROUTE_REG && route_of(OP_CORRW, 100000, 8) == ROUTE_REG);
    CHECK(route_of(OP_BETAW, 100000, 9) == ROUTE_LDS && route_of(OP_COVW, 100000, 64) == ROUTE_LDS);
    CHECK(route_of(OP_COVW, 100000, 65) == ROUTE_PREFIX && route_of(OP_CORRW, 100000, 0xFFFFFFFFu) == ROUTE_PREFIX);
    CHECK(route_of(OP_COVW, 2, 1000) == ROUTE_REG && route_of(OP_COVW, 64, 0xFFFFFFFFu) == ROUTE_LDS && route_of(OP_COVW, 65, 0xFFFFFFFFu) == ROUTE_PREFIX);
    for (int op = OP_COVS; op <= OP_BETAS; ++op) CHECK(op_running(op) && route_of(op, 1, 0) == ROUTE_PREFIX && route_of(op, 100000, 3) == ROUTE_PREFIX);
    CHECK(!op_known(-1) && !op_known(OP_COUNT) && op_known(OP_COVS) && op_known(OP_BETAW));
    CHECK(op_family(OP_COVS) == 0 && op_family(OP_CORRS) == 1 && op_family(OP_BETAS) == 2 && op_family(OP_COVW) == 0 && op_family(OP_CORRW) == 1 && op_family(OP_BETAW) == 2);
    CHECK(family_sums(0) == 3 && family_sums(1) == 5 && family_sums(2) == 4);
    CHECK(clamp_window(0xFFFFFFFFu, 7) == 7 && clamp_window(3, 7) == 3);
    // workspace: exact under the guard's allocator, at the tile edges, at the largest column, flat and grouped
    const uint32_t sizes[] = {1, 2, 2047, 2048, 2049, 6145, 300001, (1u << 31) + 5, 0xFFFFFFFFu};
    const uint32_t windows[] = {1, 8, 9, 64, 65, 1000, 0xFFFFFFFFu};
    size_t calls = 0;
    for (uint32_t n : sizes) for (uint32_t w : windows) for (int op = 0; op < OP_COUNT; ++op) for (int grouped = 0; grouped < 2; ++grouped) {
        bool fits = false;
        const size_t end = replay(op, n, w, grouped != 0, grouped ? 72 : 64, 12, &fits);
        CHECK(fits);
        CHECK((route_of(op, n, w) == ROUTE_PREFIX) == (end != 0));
        ++calls;
    }
    CHECK(ws_bytes(OP_COVW, 0, 100, true, 72, 12) == 0);
    // no 32-bit overflow: five doubles a row at 2^32 - 1 rows
    CHECK(ws_bytes(OP_CORRW, 0xFFFFFFFFu, 100, false, 64, 12) > (size_t)0xFFFFFFFFu * 40);
    std::printf("pair_route selftest ok (%zu sizings)\n", calls);
    return 0;
}
