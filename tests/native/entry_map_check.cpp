// entry_map_check.cpp -- the entry map of the binned path's two gathers (kb_entry_off, csrc/kdf_device.h): lane l = g S + j
// of a wave reads, at step q, the entry at offset g (S E) + q S + j of the wave's block of 64 E entries.
// A stand-alone program (tests/test_entry_map_host.py builds it with a host compiler and -fsanitize=address,undefined and
// runs it as a subprocess).  For S in {8, 16, 32, 64} and E in {8, 12, 16}:
//   (1) (lane, step) -> offset is a bijection onto [0, 64 E);
//   (2) S = 64 is the plain map 64 q + l;
//   (3) the offset is affine in q, S entries per step (the kernels add S q to a lane's first entry), and grows with q;
//   (4) for a block cut at any `live` in [0, 64 E] (the entries below `total`), the steps with at least one live lane are
//       exactly the prefix q < min(E, ceil(live / S)) -- what the wave-uniform exits of kernel C's resolve loop assume --
//       and the smallest offset of step q is S q, that of lane 0: `wbase + S q0 >= total` ends the wave's batch.
//
//   entry_map_check            prints one summary line per (S, E); exit status 0 = every property holds
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kdf_device.h"

static unsigned long long g_bad = 0;
static void fail(const char *what, uint32_t S, uint32_t E, uint32_t a, uint32_t b) {
    if (g_bad++ < 20) std::fprintf(stderr, "S = %u, E = %u: %s (%u, %u)\n", S, E, what, a, b);
}

template <uint32_t S>
static void check(uint32_t E) {
    const uint32_t N = 64 * E;
    unsigned long long cases = 0;
    // (1) bijection, (2) S = 64, (3) affine and increasing in q
    std::vector<uint8_t> seen(N, 0);
    for (uint32_t l = 0; l < 64; ++l)
        for (uint32_t q = 0; q < E; ++q) {
            const uint32_t o = kb_entry_off<S>(E, l, q);
            ++cases;
            if (o >= N) { fail("offset past the block", S, E, l, q); continue; }
            if (seen[o]++) fail("offset taken twice", S, E, l, q);
            if (S == 64 && o != 64 * q + l) fail("S = 64 is not 64 q + l", S, E, l, q);
            if (o != kb_entry_off<S>(E, l, 0) + S * q) fail("not first entry + S q", S, E, l, q);
            if (o != (l / S) * (S * E) + q * S + l % S) fail("not g S E + q S + j", S, E, l, q);
        }
    for (uint32_t o = 0; o < N; ++o)
        if (!seen[o]) fail("offset never taken", S, E, o, 0);
    // (4) live steps of a cut block
    for (uint32_t live = 0; live <= N; ++live) {
        const uint32_t want = (live + S - 1) / S < E ? (live + S - 1) / S : E;
        for (uint32_t q = 0; q < E; ++q) {
            uint32_t lowest = N; bool any = false;
            for (uint32_t l = 0; l < 64; ++l) {
                const uint32_t o = kb_entry_off<S>(E, l, q);
                if (o < lowest) lowest = o;
                any = any || o < live;
            }
            ++cases;
            if (lowest != S * q || lowest != kb_entry_off<S>(E, 0, q)) fail("first entry of a step is not lane 0's, S q", S, E, q, lowest);
            if (any != (q < want)) fail("live steps are not the prefix q < ceil(live / S)", S, E, live, q);
            if (any != (S * q < live)) fail("the exit test S q >= live disagrees", S, E, live, q);
        }
        // a lane with its first entry dead has no live entry at all (the once-per-batch search is skipped for it)
        for (uint32_t l = 0; l < 64; ++l)
            if (kb_entry_off<S>(E, l, 0) >= live)
                for (uint32_t q = 1; q < E; ++q)
                    if (kb_entry_off<S>(E, l, q) < live) fail("live entry behind a dead first one", S, E, live, l);
    }
    std::printf("kb_entry_off S = %u E = %u: %llu cases\n", S, E, cases);
}

int main() {
    for (uint32_t E : {8u, 12u, 16u}) {
        check<8>(E); check<16>(E); check<32>(E); check<64>(E);
    }
    std::printf("kb_entry_off: %llu failures\n", g_bad);
    return g_bad ? 1 : 0;
}
