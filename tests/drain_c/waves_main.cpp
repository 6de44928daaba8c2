// tests/drain_c/waves_main.cpp -- property check of the drainer's wave colouring on the
// CPU: tests/test_abi.py::test_drain_wave_colouring compiles this against the shipped
// cocytus_amd/csrc/cec_hostplan.hpp (radix_sort, colour_intervals, overlap_waves) under
// ASan + UBSan.  No two overlapping updates may share a wave; a batch of distinct values is
// one wave; without empty updates the wave count is the deepest overlap; the address sort
// is ordered.  The same colouring over unit-aligned tile intervals, as the recovery pool's
// fold_updates feeds it, has the same two properties.  Last, a batch against the drainer's own
// staging area (inside_area, meets_area, split_by_area): check_areas below.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "cec_hostplan.hpp"

using namespace cec;

// The deepest overlap of the non-empty intervals [lo[i], hi[i]): reached at some start.
static int depth_of(const std::vector<uint64_t> &lo, const std::vector<uint64_t> &hi) {
    int depth = 0;
    for (size_t i = 0; i < lo.size(); ++i) {
        if (hi[i] <= lo[i]) continue;
        int d = 0;
        for (size_t j = 0; j < lo.size(); ++j) d += lo[j] <= lo[i] && lo[i] < hi[j];
        depth = std::max(depth, d);
    }
    return depth;
}

// A batch against the drainer's staging area (addresses only: nothing is dereferenced).  An
// area of 8192 bytes at 1 MiB: a buffer is inside it from its first byte to one that ends on
// its last; one byte before or one byte beyond is outside but meets it; split_by_area sends
// the first kind to `in` with their span, every other non-empty one to `rest` in pieces of at
// most `piece` bytes that tile it exactly, both in list order.
static int check_areas() {
    const uintptr_t base = 1u << 20;
    const size_t cap = 8192;
    auto at = [&](long off) { return reinterpret_cast<const void *>(base + off); };
    struct { long off; size_t len; bool inside, meets; } probe[] = {
        {0, 1, true, true},       {0, 8192, true, true},   {8191, 1, true, true},    {4096, 4096, true, true},
        {-1, 2, false, true},     {-1, 1, false, false},   {8191, 2, false, true},   {8192, 1, false, false},
        {-100, 9000, false, true}, {0, 8193, false, true}, {-5000, 4096, false, false}, {100, 0, true, false},
        {-1, 0, false, false},
    };
    for (const auto &p : probe) {
        if (inside_area(at(p.off), p.len, at(0), cap) != p.inside) return 1;
        if (meets_area(at(p.off), p.len, at(0), cap) != p.meets) return 2;
    }
    std::mt19937_64 r(11);
    for (int t = 0; t < 2000; ++t) {
        const int n = 1 + r() % 40;
        const uint32_t piece = 1 + r() % 5000;
        std::vector<cec_host_update> u(n), in, rest;
        for (auto &x : u) {
            x.len = r() % 5 ? static_cast<uint32_t>(r() % 12000) : 0;
            x.buf = at(static_cast<long>(r() % 24000) - 8000);
            x.addr = r() % (1ull << 34);
            x.src_lid = r() % 3;
        }
        uint64_t lo, hi;
        split_by_area(u.data(), n, at(0), cap, piece, in, rest, &lo, &hi);
        size_t ii = 0, ri = 0;
        uint64_t want_lo = UINT64_MAX, want_hi = 0;
        for (const auto &x : u) {
            if (!x.len) continue;
            const uintptr_t b = reinterpret_cast<uintptr_t>(x.buf);
            if (b >= base && b + x.len <= base + cap) {
                if (ii >= in.size() || in[ii].buf != x.buf || in[ii].addr != x.addr || in[ii].len != x.len ||
                    in[ii].src_lid != x.src_lid)
                    return 3;
                ++ii;
                want_lo = std::min<uint64_t>(want_lo, b - base);
                want_hi = std::max<uint64_t>(want_hi, b - base + x.len);
                continue;
            }
            for (uint32_t o = 0; o < x.len;) {  // its pieces, in order, none empty, none above `piece`
                if (ri >= rest.size()) return 4;
                const cec_host_update &p = rest[ri++];
                if (reinterpret_cast<uintptr_t>(p.buf) != b + o || p.addr != x.addr + o || p.src_lid != x.src_lid) return 5;
                if (!p.len || p.len > piece || p.len > x.len - o) return 6;
                if (p.len < piece && o + p.len != x.len) return 7;  // (only the last may be short)
                o += p.len;
            }
        }
        if (ii != in.size() || ri != rest.size()) return 8;
        if (lo != want_lo || hi != want_hi) return 9;
    }
    return 0;
}

int main() {
    std::mt19937_64 r(5);
    for (int t = 0; t < 4000; ++t) {  // (the last 1,000 batches: no empty update)
        int n = 1 + r() % 200;
        std::vector<cec_host_update> u(n);
        const uint64_t span = 1 + r() % (1ull << (r() % 34));
        for (auto &x : u) { x.addr = r() % span; x.len = r() % 4 ? (uint32_t)(r() % 5000) : 0; x.src_lid = 0; x.buf = nullptr; }
        if (t >= 3000) for (auto &x : u) if (!x.len) x.len = 1 + (uint32_t)(r() % 5000);
        if (t % 3 == 0) for (int i = 0; i < n; ++i) { u[i].addr = (uint64_t)i * 4098 + (t % 7) * (1ull << 33); u[i].len = 4098; }
        std::vector<int> w;
        int nw = overlap_waves(u.data(), n, w);
        int mx = 0;
        for (int i = 0; i < n; ++i) mx = std::max(mx, w[i]);
        if (mx >= nw) { printf("wave out of range\n"); return 1; }
        for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) {
            if (!u[i].len || !u[j].len || w[i] != w[j]) continue;
            bool ov = u[i].addr < u[j].addr + u[j].len && u[j].addr < u[i].addr + u[i].len;
            if (ov) { printf("overlap in wave t=%d\n", t); return 1; }
        }
        if (t % 3 == 0 && nw != 1) { printf("fast path missed\n"); return 1; }
        bool any_empty = false;
        std::vector<uint64_t> lo(n), hi(n);
        for (int i = 0; i < n; ++i) { lo[i] = u[i].addr; hi[i] = u[i].addr + u[i].len; any_empty |= !u[i].len; }
        if (!any_empty && nw != depth_of(lo, hi)) { printf("waves %d != depth %d t=%d\n", nw, depth_of(lo, hi), t); return 1; }
    }
    // the pool's feed: the 4 KiB-cut tiles of pieces inside slots of 1-4 units, sorted by offset
    for (int t = 0; t < 2000; ++t) {
        const int slots = 1 + r() % 8, pieces = 1 + r() % 64;
        std::vector<uint64_t> slot_off(slots), slot_len(slots), lo, hi;
        uint64_t at = 0;
        for (int s = 0; s < slots; ++s) { slot_off[s] = at; slot_len[s] = (1 + r() % 4) * 4096; at += slot_len[s]; }
        std::vector<std::pair<uint64_t, uint64_t>> tiles;
        for (int p = 0; p < pieces; ++p) {
            const int s = r() % slots;
            const uint64_t a = r() % slot_len[s], b = a + 1 + r() % (slot_len[s] - a);
            for (uint64_t o = slot_off[s] + a, e = slot_off[s] + b; o < e;) {  // append_tiles' cut
                const uint64_t step = std::min<uint64_t>(4096 - o % 4096, e - o);
                tiles.emplace_back(o, o + step);
                o += step;
            }
        }
        std::sort(tiles.begin(), tiles.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
        std::vector<int> w(tiles.size(), -1);
        const int nw = colour_intervals(tiles.size(), [&](size_t i) { return tiles[i]; }, [&](size_t i, int x) { w[i] = x; });
        for (size_t i = 0; i < tiles.size(); ++i) {
            if (w[i] < 0 || w[i] >= nw) { printf("tile wave out of range t=%d\n", t); return 1; }
            for (size_t j = i + 1; j < tiles.size(); ++j)
                if (w[i] == w[j] && tiles[i].first < tiles[j].second && tiles[j].first < tiles[i].second) {
                    printf("tiles overlap in wave t=%d\n", t);
                    return 1;
                }
            lo.push_back(tiles[i].first);
            hi.push_back(tiles[i].second);
        }
        if (nw != depth_of(lo, hi)) { printf("tile waves %d != depth %d t=%d\n", nw, depth_of(lo, hi), t); return 1; }
    }
    std::vector<cec_host_update> u(70000);
    std::mt19937 g(1); std::vector<int> p(u.size()); for (size_t i=0;i<p.size();++i) p[i]=i; std::shuffle(p.begin(),p.end(),g);
    for (size_t i=0;i<u.size();++i) u[i] = {nullptr, (uint64_t)p[i]*4098, 4098, 0};
    std::vector<std::pair<uint64_t,int>> s(u.size());
    for (size_t i=0;i<u.size();++i) s[i] = {u[i].addr, (int)i};
    radix_sort(s);
    for (size_t i=1;i<s.size();++i) if (s[i-1].first > s[i].first) { printf("not sorted\n"); return 1; }
    for (size_t i=0;i<s.size();++i) if (u[s[i].second].addr != s[i].first) { printf("index lost\n"); return 1; }
    if (int bad = check_areas()) { printf("area check %d\n", bad); return 1; }
    printf("ok\n");
}
