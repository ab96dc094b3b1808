// stage_layout_check.cpp -- the layout of a host form's staging frame (StageLayout, csrc/kdf_engine_priv.h): where the items
// of one call lie in the engine's one staging arena.
// A stand-alone program (tests/test_stage_layout_host.py builds it with a host compiler and -fsanitize=address,undefined and
// runs it as a subprocess).  It includes the header's host-only part alone -- no HIP -- and checks, over random item lists
// of 1 to 16 items: every non-empty item starts at a multiple of 256 bytes, no two items overlap, the total is at least the
// sum of the sizes and at most that plus 256 bytes of padding per item, an empty item resolves to null, and nothing wraps
// for items of up to 2^33 bytes (offsets are size_t).
//
//   stage_layout_check         prints one summary line; exit status 0 = every list within the rules
#include <cstdint>
#include <cstdio>

#include "kdf_engine_priv.h"

static_assert(sizeof(size_t) == 8, "offsets of 2^33-byte items need a 64-bit size_t");
static_assert(sizeof(((StageLayout *)nullptr)->off[0]) == sizeof(size_t) && sizeof(((StageLayout *)nullptr)->total) == sizeof(size_t), "offsets are size_t");

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                                   // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}

int main() {
    const size_t fixed[9] = {0, 1, 15, 16, 255, 256, 257, 4095, 4096};
    unsigned long long lists = 0, items = 0, empty = 0, huge = 0, bad = 0;
    auto report = [&](const char *what, int i, const StageLayout &l) {
        if (bad++ < 20) std::fprintf(stderr, "%s: item %d of %d (offset %zu, size %zu, total %zu)\n", what, i, l.n, l.off[i], l.size[i], l.total);
    };
    char *const base = (char *)(uintptr_t)0x7f0000000000ull;          // (never dereferenced: hipMalloc aligns the real one to 256 too)
    for (int round = 0; round < 6000; ++round) {
        StageLayout l;
        const int n = 1 + (int)(rnd() % 16);
        size_t want[StageLayout::MAX_ITEMS], sum = 0;
        for (int i = 0; i < n; ++i) {
            const uint64_t pick = rnd() % 10;
            want[i] = pick < 9 ? fixed[pick] : (size_t)(rnd() % ((1ull << 33) + 1));
            if (round % 64 == 0 && i == n / 2) want[i] = (size_t)1 << 33;                  // the largest item, at times
            sum += want[i];
            if (l.add(want[i]) != i) report("add() did not return the item's index", i, l);
        }
        ++lists; items += n;
        if (l.n != n) report("item count", 0, l);
        size_t end = 0;                                                // where the previous non-empty item ended
        for (int i = 0; i < n; ++i) {
            if (l.size[i] != want[i]) report("size not kept", i, l);
            void *p = l.at(base, i);
            if (want[i] == 0) { ++empty; if (p) report("an empty item has an address", i, l); continue; }
            huge += want[i] >= (1ull << 32);
            if ((char *)p != base + l.off[i]) report("address is not base + offset", i, l);
            if (l.off[i] % 256) report("not 256-aligned", i, l);
            if (l.off[i] < end) report("overlaps the item before it", i, l);
            if (l.off[i] + l.size[i] < l.off[i] || l.off[i] + l.size[i] > l.total) report("ends past the total", i, l);
            end = l.off[i] + l.size[i];
        }
        if (l.total < sum) report("total below the sum of the sizes", 0, l);
        if (l.total > sum + (size_t)256 * n) report("more than 256 bytes of padding per item", 0, l);
    }
    std::printf("stage_layout: %llu lists, %llu items, %llu empty, %llu of 4 GB and more, %llu broken rules\n", lists, items, empty, huge, bad);
    return bad ? 1 : 0;
}
