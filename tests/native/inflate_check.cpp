// inflate_check.cpp -- the DEFLATE decoder of the device BAM feeder (csrc/kdf_inflate.h) on the CPU, one lane.
//
// A stand-alone program (tests/test_inflate_core.py builds it with a host compiler and -fsanitize=address,undefined and
// runs it as a subprocess).  Input file: records of
//     u32 comp_len | u32 isize | u32 valid | comp bytes | isize expected bytes (valid records only)
// Every buffer is a heap block of exactly the stated size, so a read past the payload or a write past ISIZE is a
// sanitizer report.
//   1. every record is decoded; one line "case <i> status <s> equal <0|1>" each.  A valid record must decode to the
//      expected bytes; exit code 1 otherwise.
//   2. with a second argument N: N seeded corruptions of the valid payloads (bit flips, truncations, swapped NLEN,
//      altered ISIZE); each must come back with a status.  One summary line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kdf_inflate.h"

struct Case { std::vector<uint8_t> comp, want; uint32_t isize; bool valid; };

static int decode(const uint8_t *comp, uint32_t n, uint32_t isize, std::vector<uint8_t> *got) {
    uint8_t *in = (uint8_t *)malloc(n ? n : 1), *out = (uint8_t *)malloc(isize ? isize : 1);
    if (n) memcpy(in, comp, n);
    memset(out, 0xA5, isize);
    KdfInfTables *T = new KdfInfTables();
    const int st = kdf_inflate_block(KdfLaneHost{}, in, n, out, isize, *T);
    if (got) got->assign(out, out + isize);
    delete T; free(in); free(out);
    return st;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: inflate_check cases.bin [n_corruptions]\n"); return 2; }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<Case> cases;
    for (;;) {
        uint32_t h[3];
        if (fread(h, 4, 3, fp) != 3) break;
        Case c; c.isize = h[1]; c.valid = h[2] != 0;
        c.comp.resize(h[0]);
        if (h[0] && fread(c.comp.data(), 1, h[0], fp) != h[0]) return 2;
        if (c.valid) { c.want.resize(h[1]); if (h[1] && fread(c.want.data(), 1, h[1], fp) != h[1]) return 2; }
        cases.push_back(std::move(c));
    }
    fclose(fp);
    int bad = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        std::vector<uint8_t> got;
        const int st = decode(cases[i].comp.data(), (uint32_t)cases[i].comp.size(), cases[i].isize, &got);
        const bool eq = cases[i].valid && st == KDF_INF_OK && got == cases[i].want;
        printf("case %zu status %d equal %d\n", i, st, eq ? 1 : 0);
        if (cases[i].valid && !eq) ++bad;
    }
    const long n_fuzz = argc > 2 ? atol(argv[2]) : 0;
    long rejected = 0, accepted = 0;
    std::vector<size_t> pool;
    for (size_t i = 0; i < cases.size(); ++i) if (cases[i].valid && !cases[i].comp.empty()) pool.push_back(i);
    for (long f = 0; f < n_fuzz && !pool.empty(); ++f) {
        const Case &c = cases[pool[rng() % pool.size()]];
        std::vector<uint8_t> m = c.comp;
        uint32_t isize = c.isize;
        switch (rng() % 5) {
        case 0: { const int flips = 1 + (int)(rng() % 4); for (int j = 0; j < flips; ++j) m[rng() % m.size()] ^= (uint8_t)(1u << (rng() % 8)); break; }
        case 1: m.resize(rng() % m.size()); break;                                     // truncation
        case 2: if (m.size() >= 5) { std::swap(m[1], m[3]); std::swap(m[2], m[4]); } break;   // LEN <-> NLEN of a leading stored block
        case 3: isize = (uint32_t)(rng() % 65537); break;                              // a lying ISIZE
        default: { const size_t at = rng() % m.size(); for (size_t j = at; j < m.size() && j < at + 8; ++j) m[j] = (uint8_t)rng(); break; }
        }
        const int st = decode(m.data(), (uint32_t)m.size(), isize, nullptr);
        if (st == KDF_INF_OK) ++accepted; else ++rejected;
    }
    printf("fuzz %ld rejected %ld accepted %ld\n", n_fuzz, rejected, accepted);
    return bad ? 1 : 0;
}
