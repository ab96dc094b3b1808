// run_guess_check.cpp -- the run guesses of the binned path (kb_guess_scale / kb_guess_scaled / kb_guess_run, csrc/kdf_device.h)
// against the exact integer divisions they replaced.
// A stand-alone program (tests/test_run_guess_host.py builds it with a host compiler and -fsanitize=address,undefined and
// runs it as a subprocess).  Every guess must lie in [0, nruns - 1] and differ from the exact one by at most ONE run: that
// is what kernel C's window rpw[gu .. gu + 3] absorbs without its walk.  The device takes its reciprocal from v_rcp_f32
// (1 ulp), the host from a division: every case is run with the reciprocal as divided and one ulp to either side of it.
//
//   run_guess_check            prints one summary line per part; exit status 0 = every case within the bound
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "kdf_device.h"

static unsigned long long g_cases = 0, g_off_by_one = 0, g_bad = 0;

static void report(const char *what, unsigned long long a, unsigned long long b, unsigned long long c, uint32_t got, uint32_t want) {
    if (g_bad++ < 20) std::fprintf(stderr, "%s(%llu, %llu, %llu): guess %u, exact %u\n", what, a, b, c, got, want);
}
static inline void judge(const char *what, unsigned long long a, unsigned long long b, unsigned long long c, uint32_t got, uint32_t want, uint32_t n) {
    ++g_cases;
    const uint32_t d = got > want ? got - want : want - got;
    if (got >= n || d > 1) report(what, a, b, c, got, want);
    g_off_by_one += d;
}

// ---- kernel C: (ei * scale) >> 32 with scale = (nruns << 32) / total ----------------------------------------------------
static void scale_case(uint32_t nruns, uint32_t total) {
    const unsigned long long exact = ((unsigned long long)nruns << 32) / total;
    // entries: both ends, the middle, and the entries on either side of where the true quotient ei * nruns / total steps
    uint32_t ei[16]; int n = 0;
    ei[n++] = 0; ei[n++] = total - 1; ei[n++] = total / 2; ei[n++] = total > 1 ? 1 : 0;
    const uint32_t ks[5] = {1u, 2u, nruns / 2, nruns - 1, (uint32_t)((total * 2654435761ull) % nruns)};
    for (uint32_t k : ks) {
        if (k == 0 || k >= nruns) continue;
        const unsigned long long b = ((unsigned long long)k * total + nruns - 1) / nruns;       // first entry of run k
        if (b < total) ei[n++] = (uint32_t)b;
        if (b >= 1 && b - 1 < total) ei[n++] = (uint32_t)(b - 1);
    }
    const float r = 1.0f / (float)total;
    const float rs[3] = {r, std::nextafterf(r, 0.0f), std::nextafterf(r, 2.0f)};
    for (int v = 0; v < 3; ++v) {
        const unsigned long long scale = v == 0 ? kb_guess_scale(nruns, total) : kb_guess_scale_rcp(nruns, rs[v]);
        for (int i = 0; i < n; ++i) {
            const uint32_t want = kb_guess_scaled(ei[i], exact, nruns);
            judge("kb_guess_scale", nruns, total, ei[i], kb_guess_scaled(ei[i], scale, nruns), want, nruns);
        }
    }
}

// ---- piece sort: e * ns / n_pair -------------------------------------------------------------------------------------------
static inline void run_case(uint32_t e, uint32_t ns, uint32_t n_pair, const float (&rs)[3]) {
    const unsigned long long q = (unsigned long long)e * ns / n_pair;
    const uint32_t want = q < ns ? (uint32_t)q : ns - 1;
    judge("kb_guess_run", e, ns, n_pair, kb_guess_run(e, ns, n_pair), want, ns);
    judge("kb_guess_run-", e, ns, n_pair, kb_guess_run_rcp(e, ns, rs[1]), want, ns);
    judge("kb_guess_run+", e, ns, n_pair, kb_guess_run_rcp(e, ns, rs[2]), want, ns);
}

int main() {
    const uint32_t NR[9] = {1, 2, 3, 255, 256, 257, 511, 512, 1024};
    // (1) every total up to 2^20
    for (uint32_t total = 1; total <= (1u << 20); ++total)
        for (uint32_t nruns : NR) scale_case(nruns, total);
    // (2) powers of two and their neighbours, up to 2^32 - 1
    for (int b = 20; b <= 32; ++b)
        for (long long d = -1; d <= 1; ++d) {
            const unsigned long long t = (1ull << b) + d;
            if (t > 0xFFFFFFFFull) continue;
            for (uint32_t nruns : NR) scale_case(nruns, (uint32_t)t);
        }
    for (uint32_t nruns : NR)
        if (kb_guess_scale(nruns, 0) != 0) report("kb_guess_scale", nruns, 0, 0, 1, 0);
    std::printf("kb_guess_scale: %llu cases, %llu one run off, %llu out of bounds\n", g_cases, g_off_by_one, g_bad);
    const unsigned long long bad1 = g_bad;
    g_cases = g_off_by_one = 0;

    const uint32_t NS[11] = {1, 2, 3, 31, 255, 256, 257, 1023, 1024, 2047, 2048};
    auto rcps = [](uint32_t n_pair, float (&rs)[3]) {
        rs[0] = 1.0f / (float)n_pair; rs[1] = std::nextafterf(rs[0], 0.0f); rs[2] = std::nextafterf(rs[0], 2.0f);
    };
    // (3) small pairs: every entry of every pair of up to 2100 entries
    for (uint32_t n_pair = 1; n_pair <= 2100; ++n_pair) {
        float rs[3]; rcps(n_pair, rs);
        for (uint32_t ns : NS)
            for (uint32_t e = 0; e < n_pair; ++e) run_case(e, ns, n_pair, rs);
    }
    // (4) large pairs: the first 65 536 entries (a first piece is at most that long), then the pair's last entries and the
    // entries around the middle -- the further pieces of a skewed pair (kb_sort_piece with p > 0)
    for (int b = 12; b <= 32; ++b)
        for (long long d : {-1ll, 0ll, 1ll, (1ll << b) / 3}) {
            const unsigned long long t = (1ull << b) + d;
            if (t > 0xFFFFFFFFull) continue;
            const uint32_t n_pair = (uint32_t)t;
            float rs[3]; rcps(n_pair, rs);
            for (uint32_t ns : NS) {
                const uint32_t top = n_pair < 65536u ? n_pair : 65536u;
                for (uint32_t e = 0; e < top; ++e) run_case(e, ns, n_pair, rs);
                for (uint32_t i = 1; i <= 256 && i <= n_pair; ++i) {
                    run_case(n_pair - i, ns, n_pair, rs);
                    run_case(n_pair / 2 + i - 1 < n_pair ? n_pair / 2 + i - 1 : n_pair - 1, ns, n_pair, rs);
                }
            }
        }
    for (uint32_t ns : NS)
        if (kb_guess_run(7, ns, 0) != 0) report("kb_guess_run", 7, ns, 0, 1, 0);
    std::printf("kb_guess_run: %llu cases, %llu one run off, %llu out of bounds\n", g_cases, g_off_by_one, g_bad - bad1);
    return g_bad ? 1 : 0;
}
