// ws_guard.hpp -- host-only bookkeeping of the workspace guard (AQG_WS_GUARD, a test aid; DESIGN.md "Scratch memory").
// No HIP in here: ctx.hip drives the device side (fills, the copy back), tests/ws_guard_selftest.cpp drives this header on the CPU.
//
// Layout of a guarded arena.  A call sees LOGICAL offsets: the bump allocator of the unguarded library (every sub-allocation
// starts at a multiple of 256), held to a logical capacity that is EXACTLY what aqg_ws_ensure was asked for SINCE THE LAST RESET, rounded
// up to 256 -- no doubling, no floor, and nothing inherited from an earlier, larger use of the same context (only the physical
// arena is grow-only).  Sub-allocation number i (counted from the last reset) lives at
//     physical offset = logical offset + 256 * (i + 1)
// so that a 256-byte red zone that is never handed out precedes every payload and alignment is unchanged.  The arena has room for
// AQG_WS_GUARD_ZONES zones on top of the logical capacity.  Everything outside the logged payloads -- zones, alignment padding, the
// tail behind the last payload -- holds the poison byte and is compared against it by ws_guard_scan.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

constexpr size_t AQG_WS_GUARD_ZONE = 256;
constexpr size_t AQG_WS_GUARD_ZONES = 1024;      // sub-allocations one arena use may make under the guard

// what a violation damaged (aqg_ws_report::kind of include/aqg.h)
enum { WS_GUARD_CLEAN = 0, WS_GUARD_ZONE = 1, WS_GUARD_PADDING = 2, WS_GUARD_TAIL = 3, WS_GUARD_RANK_BM = 4 };

struct ws_guard_alloc { size_t off, bytes; };    // physical offset of the payload, its size

struct ws_guard_report {
    int kind = WS_GUARD_CLEAN;
    size_t offset = 0;          // physical offset of the first damaged byte (RANK_BM: byte offset into the bitmap)
    int after = -1;             // index of the logged sub-allocation whose payload ends at or before `offset` and is nearest to it; -1: none
    size_t after_off = 0, after_bytes = 0;
    uint8_t expected = 0, found = 0;
};

struct ws_guard_book {
    bool on = false;
    uint8_t pattern = 0;
    size_t logical_cap = 0;     // largest request since the last reset, rounded up to 256
    std::vector<ws_guard_alloc> log;
    ws_guard_report latched;    // the FIRST violation; later calls do not clear it

    static size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }
    static size_t physical_bytes(size_t logical) { return logical + AQG_WS_GUARD_ZONE * AQG_WS_GUARD_ZONES; }
    size_t physical_cap() const { return physical_bytes(logical_cap); }
    bool live() const { for (const auto& a : log) if (a.bytes) return true; return false; }      // (an empty sub-allocation has nothing to move)
    // aqg_ws_ensure.  true: the use's capacity now covers `bytes` (the caller grows the physical arena to physical_cap() when it is
    // smaller); false: a larger request while sub-allocations of this use are live -- it would move them: the caller's sizing bug
    bool want(size_t bytes) {
        const size_t r = round256(bytes);
        if (r <= logical_cap) return true;
        if (live()) return false;
        logical_cap = r;
        return true;
    }
    // aqg_ws_reset: a new arena use starts with no capacity at all; what the last use asked for does not carry over
    void reset() { log.clear(); logical_cap = 0; }
    // aqg_ws_alloc.  *logical_off: the bump offset before the call, the payload's logical end after it.  0: done, *phys = the payload's
    // physical offset; 1: the logical end exceeds the capacity (the caller's sizing bug); 2: more sub-allocations than zones.
    int alloc(size_t* logical_off, size_t bytes, size_t* phys) {
        const size_t off = round256(*logical_off);
        if (off + bytes > logical_cap || off + bytes < off) return 1;
        if (log.size() + 1 >= AQG_WS_GUARD_ZONES) return 2;
        *phys = off + AQG_WS_GUARD_ZONE * (log.size() + 1);
        log.push_back({*phys, bytes});
        *logical_off = off + bytes;
        return 0;
    }
    void latch(const ws_guard_report& r) { if (latched.kind == WS_GUARD_CLEAN && r.kind != WS_GUARD_CLEAN) latched = r; }
};

namespace ws_guard_detail {
// first byte of [b, e) of `host` that is not `pat`, or e
inline size_t first_mismatch(const uint8_t* host, size_t b, size_t e, uint8_t pat) {
    uint64_t w;
    memset(&w, pat, 8);
    size_t i = b;
    for (; i < e && (i & 7); ++i) if (host[i] != pat) return i;
    for (; i + 8 <= e; i += 8) {
        uint64_t v;
        memcpy(&v, host + i, 8);
        if (v != w) break;
    }
    for (; i < e; ++i) if (host[i] != pat) return i;
    return e;
}
} // namespace ws_guard_detail

// `host`: a copy of the arena's `cap` physical bytes.  The first byte outside every logged payload that is not `pattern`, classified:
// ZONE, the 256 bytes in front of a payload; TAIL, behind the 256-rounded end of the payload that ends last; PADDING, the rest.
inline ws_guard_report ws_guard_scan(const uint8_t* host, size_t cap, uint8_t pattern, const std::vector<ws_guard_alloc>& log) {
    ws_guard_report r;
    std::vector<std::pair<size_t, size_t>> iv;           // payloads as [begin, end), sorted and merged (a rewound bump offset lets them overlap)
    iv.reserve(log.size());
    size_t last_end = 0;
    for (const auto& a : log) {
        const size_t e = std::min(cap, a.off + a.bytes);
        if (a.bytes && a.off < cap) iv.emplace_back(a.off, e);
        last_end = std::max(last_end, e);
    }
    std::sort(iv.begin(), iv.end());
    size_t pos = 0, bad = cap;
    for (size_t k = 0; k <= iv.size() && bad == cap; ++k) {
        const size_t gap_end = k < iv.size() ? iv[k].first : cap;
        if (gap_end > pos) {
            const size_t m = ws_guard_detail::first_mismatch(host, pos, gap_end, pattern);
            if (m < gap_end) bad = m;
        }
        if (k < iv.size()) pos = std::max(pos, iv[k].second);
    }
    if (bad == cap) return r;
    r.offset = bad;
    r.expected = pattern;
    r.found = host[bad];
    r.kind = bad >= ws_guard_book::round256(last_end) ? WS_GUARD_TAIL : WS_GUARD_PADDING;
    size_t best_end = 0;
    for (size_t i = 0; i < log.size(); ++i) {
        const auto& a = log[i];
        if (bad < a.off && bad + AQG_WS_GUARD_ZONE >= a.off) r.kind = WS_GUARD_ZONE;
        if (a.off + a.bytes <= bad && (r.after < 0 || a.off + a.bytes >= best_end)) { r.after = (int)i; best_end = a.off + a.bytes; }
    }
    if (r.after >= 0) { r.after_off = log[r.after].off; r.after_bytes = log[r.after].bytes; }
    return r;
}
