// Host self-test of the workspace guard's bookkeeping (aquery2_amd/csrc/ws_guard.hpp): offsets, exact capacity, and the scan of a host
// copy of an arena.  No GPU, no HIP; built with -fsanitize=address,undefined and run by tests/test_ws_guard_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../aquery2_amd/csrc/ws_guard.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
    const uint8_t PAT = 0xA5;
    // ---- logical versus physical offsets ------------------------------------------------------------------------------------------
    ws_guard_book g;
    g.on = true; g.pattern = PAT;
    CHECK(g.want(1000));                     // 1000 -> 1024 logical bytes
    CHECK(g.logical_cap == 1024);
    CHECK(g.want(1024) && g.want(7) && g.logical_cap == 1024);      // within one use a smaller or equal request changes nothing
    CHECK(g.physical_cap() == 1024 + AQG_WS_GUARD_ZONE * AQG_WS_GUARD_ZONES);
    size_t off = 0, p0 = 0, p1 = 0, p2 = 0, p3 = 0, p4 = 0;
    CHECK(g.alloc(&off, 100, &p0) == 0 && p0 == 256 && off == 100);              // logical 0   -> 0 + 256 * 1
    CHECK(g.alloc(&off, 300, &p1) == 0 && p1 == 256 + 512 && off == 556);        // logical 256 -> 256 + 256 * 2
    CHECK(g.alloc(&off, 0, &p2) == 0 && p2 == 768 + 768 && off == 768);          // an empty one still gets its zone
    CHECK(p0 % 256 == 0 && p1 % 256 == 0 && p2 % 256 == 0);
    // ---- exact capacity -------------------------------------------------------------------------------------------------------------
    const size_t keep = off;
    CHECK(g.alloc(&off, 257, &p4) == 1 && off == keep && g.log.size() == 3);     // logical 768 + 257 > 1024: the sizing bug
    CHECK(g.alloc(&off, 256, &p3) == 0 && p3 == 768 + 1024 && off == 1024);      // exactly full is fine
    CHECK(g.alloc(&off, 1, &p4) == 1);
    CHECK(g.alloc(&off, 0, &p4) == 0 && p4 == 1024 + 1280);                                          // nothing asked for at the very end
    // ---- the scan ---------------------------------------------------------------------------------------------------------------------
    const size_t cap = g.physical_cap();
    std::vector<uint8_t> arena(cap, PAT);
    for (const auto& a : g.log) for (size_t i = 0; i < a.bytes; ++i) arena[a.off + i] = (uint8_t)(i * 7 + 1);    // payloads: anything
    CHECK(ws_guard_scan(arena.data(), cap, PAT, g.log).kind == WS_GUARD_CLEAN);
    auto plant = [&](size_t at) { auto copy = arena; copy[at] ^= 0x10; return ws_guard_scan(copy.data(), cap, PAT, g.log); };
    {   // a zone: the byte just in front of the second payload, and the very first byte of the arena
        ws_guard_report r = plant(p1 - 1);
        CHECK(r.kind == WS_GUARD_ZONE && r.offset == p1 - 1 && r.after == 0 && r.after_off == p0 && r.after_bytes == 100);
        CHECK(r.expected == PAT && r.found == (PAT ^ 0x10));
        r = plant(0);
        CHECK(r.kind == WS_GUARD_ZONE && r.offset == 0 && r.after == -1);
    }
    {   // the padding: the first byte behind the first payload (what a one-past-the-end store hits)
        ws_guard_report r = plant(p0 + 100);
        CHECK(r.kind == WS_GUARD_PADDING && r.offset == p0 + 100 && r.after == 0);
        r = plant(p1 + 300);
        CHECK(r.kind == WS_GUARD_PADDING && r.offset == p1 + 300 && r.after == 1);
    }
    {   // the tail: its first and its last byte
        const size_t tail = ws_guard_book::round256(g.log.back().off + g.log.back().bytes);
        ws_guard_report r = plant(cap - 1);
        CHECK(r.kind == WS_GUARD_TAIL && r.offset == cap - 1);
        r = plant(tail);
        CHECK(r.kind == WS_GUARD_TAIL && r.offset == tail);
    }
    {   // a payload byte is the call's own business
        CHECK(plant(p0).kind == WS_GUARD_CLEAN);
        CHECK(plant(p1 + 299).kind == WS_GUARD_CLEAN);
        CHECK(plant(p3 + 255).kind == WS_GUARD_CLEAN);
    }
    {   // the first violation in address order is the one reported, and a latch keeps the first report
        auto copy = arena;
        copy[p1 + 300] = 0; copy[p0 + 100] = 0;
        ws_guard_report r = ws_guard_scan(copy.data(), cap, PAT, g.log);
        CHECK(r.offset == p0 + 100);
        g.latch(r);
        g.latch(plant(0));
        g.latch(ws_guard_report{});
        CHECK(g.latched.kind == WS_GUARD_PADDING && g.latched.offset == p0 + 100);
    }
    {   // an empty log: the whole arena is tail
        std::vector<ws_guard_alloc> none;
        auto copy = std::vector<uint8_t>(cap, PAT);
        CHECK(ws_guard_scan(copy.data(), cap, PAT, none).kind == WS_GUARD_CLEAN);
        copy[5] = 0;
        ws_guard_report r = ws_guard_scan(copy.data(), cap, PAT, none);
        CHECK(r.kind == WS_GUARD_TAIL && r.offset == 5 && r.after == -1);
    }
    {   // a rewound bump offset (the group-by's ordering tail gives its partition scratch back): payloads overlap, nothing is misreported
        ws_guard_book h;
        h.on = true; h.pattern = 0;
        h.want(4096);
        size_t o = 0, a = 0, b = 0, c = 0;
        CHECK(h.alloc(&o, 512, &a) == 0);
        const size_t mark = o;
        CHECK(h.alloc(&o, 1024, &b) == 0);
        o = mark;
        CHECK(h.alloc(&o, 2048, &c) == 0 && c == 512 + 768);
        std::vector<uint8_t> ar(h.physical_cap(), 0);
        for (const auto& x : h.log) for (size_t i = 0; i < x.bytes; ++i) ar[x.off + i] = 0xEE;
        CHECK(ws_guard_scan(ar.data(), ar.size(), 0, h.log).kind == WS_GUARD_CLEAN);
        ar[a + 512] = 1;
        CHECK(ws_guard_scan(ar.data(), ar.size(), 0, h.log).offset == a + 512);
    }
    {   // the zone budget
        ws_guard_book z;
        z.on = true;
        z.want(256);
        size_t o = 0, q = 0;
        int rc = 0;
        for (size_t i = 0; i < AQG_WS_GUARD_ZONES + 4 && rc == 0; ++i) rc = z.alloc(&o, 0, &q);
        CHECK(rc == 2 && q + AQG_WS_GUARD_ZONE <= z.physical_cap());
    }
    {   // a larger request under live sub-allocations would move them: refused; an empty sub-allocation is not live
        CHECK(g.live() && !g.want(2048) && g.logical_cap == 1024);
        ws_guard_book e;
        size_t o = 0, q = 0;
        CHECK(e.alloc(&o, 0, &q) == 0 && !e.live() && e.want(512) && e.logical_cap == 512);
    }
    {   // the capacity belongs to ONE arena use: the reset forgets log and capacity (the latch stays), and a later, smaller use of the same
        // context is held to its own request, not to the earlier, larger one
        g.reset();
        CHECK(g.log.empty() && g.logical_cap == 0 && g.latched.kind == WS_GUARD_PADDING);
        size_t o = 0, q = 0;
        CHECK(g.alloc(&o, 1, &q) == 1);                  // nothing asked for yet: no capacity
        CHECK(g.want(300) && g.logical_cap == 512);
        CHECK(g.alloc(&o, 512, &q) == 0 && q == 256);
        CHECK(g.alloc(&o, 1, &q) == 1);                  // 1024 bytes were enough for the last use; this one asked for 300
        g.reset();
        CHECK(g.want(100) && g.want(4000) && g.logical_cap == 4096);      // several requests before the first sub-allocation: the largest
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("ws_guard selftest ok\n");
    return 0;
}
