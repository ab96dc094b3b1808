// text_tile_check.hip -- what the text kernels share (csrc/kdf_text.h) against the host.  Stand-alone (hipcc
// --offload-arch=gfx950 -O3 -I<csrc>): exit status 0 = every case equal.
//
// Granule load, kt_load_granule: texts of 0, 1, 15, 16, 17, 4095, 4096 and 4097 random bytes at 0, 1 and 15 bytes behind a
// 16-byte boundary, the granules at text offset -15, at 0 and the granule of the memory that holds the last byte; bounds
// [0, n), `aligned` as the address is; and the granule at 0 once more with the bounds [3, n) and another fill value.  Byte
// for byte: the text inside the bounds, the fill value outside (the memory around the text holds other bytes).
// Backward search, kt_last_outside: texts of 0, 1, 255, 256, 257 and 513 bytes that end in a run of line ends -- the whole
// text, none, a run that ends on a round boundary (256 bytes), a run that crosses one (300 bytes; a shorter text: all but
// its first byte) -- through every thread of the workgroup.
// Base code, kdf_base_code: all 256 byte values on the device against the same function on the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "kdf_text.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(2); } } while (0)

constexpr uint32_t FILL = 0x5A;
constexpr int MAX_TEXT = 4097, TEXT_ROOM = 16 + MAX_TEXT + 47;         // 16 bytes in front of the text, its skew, 32 and more behind
struct GranuleCase { int64_t s0, lo, n; uint32_t skew, aligned, fill; };   // bounds [lo, n)

// thread per case; mem: one TEXT_ROOM per skew, the text at 16 + skew
__global__ void k_granule(const uint8_t *mem, const GranuleCase *cases, int nc, uint4 *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const GranuleCase c = cases[i];
    const uint8_t *t = mem + (size_t)(c.skew == 0 ? 0 : c.skew == 1 ? 1 : 2) * TEXT_ROOM + 16 + c.skew;
    out[i] = kt_load_granule(t, c.s0, c.lo, c.n, c.aligned != 0, c.fill);
}

// workgroup per case
__global__ __launch_bounds__(256) void k_last(const uint8_t *texts, const uint64_t *first, const uint64_t *len, unsigned long long *out) {
    const uint64_t r = kt_last_outside(texts + first[blockIdx.x], len[blockIdx.x], [](uint8_t c) { return c == '\n' || c == '\r'; });
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = r;
}

__global__ void k_codes(uint32_t *out) { out[threadIdx.x] = kdf_base_code(threadIdx.x); }

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint32_t rnd() {                                                  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static long check_granules(long &wrong) {
    static const int64_t NS[8] = {0, 1, 15, 16, 17, 4095, 4096, 4097};
    static const uint32_t SKEWS[3] = {0, 1, 15};
    std::vector<uint8_t> mem(3 * TEXT_ROOM);
    for (auto &b : mem) b = (uint8_t)rnd();
    uint8_t *d_mem;
    CK(hipMalloc(&d_mem, mem.size()));                                   // (16-byte aligned, and TEXT_ROOM is a multiple of 16)
    static_assert(TEXT_ROOM % 16 == 0, "every skew's text starts its skew behind a 16-byte boundary");
    if ((uintptr_t)d_mem & 15) { printf("hipMalloc returned an address that is not 16-byte aligned\n"); exit(2); }
    std::vector<GranuleCase> cases;
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 8; ++j) {
            const int64_t n = NS[j], skew = SKEWS[k];
            const int64_t last = n ? (skew + n - 1) / 16 * 16 - skew : 0;                  // the granule of the memory that holds byte n - 1
            const int64_t s0s[3] = {-15, 0, last};
            for (int q = 0; q < 3; ++q) cases.push_back(GranuleCase{s0s[q], 0, n, (uint32_t)skew, (uint32_t)(((skew + s0s[q]) & 15) == 0), FILL});
            // a lower bound inside the granule at 0 (3, or n for a shorter text: empty bounds) and another fill value
            cases.push_back(GranuleCase{0, n < 3 ? n : 3, n, (uint32_t)skew, (uint32_t)((skew & 15) == 0), 0xC3u});
        }
    const int nc = (int)cases.size();
    GranuleCase *d_cases; uint4 *d_out;
    CK(hipMalloc(&d_cases, nc * sizeof(GranuleCase))); CK(hipMalloc(&d_out, nc * sizeof(uint4)));
    CK(hipMemcpy(d_mem, mem.data(), mem.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_cases, cases.data(), nc * sizeof(GranuleCase), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xA5, nc * sizeof(uint4)));
    hipLaunchKernelGGL(k_granule, dim3((nc + 63) / 64), dim3(64), 0, 0, d_mem, d_cases, nc, d_out);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    std::vector<uint8_t> out(nc * 16);
    CK(hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost));
    CK(hipFree(d_mem)); CK(hipFree(d_cases)); CK(hipFree(d_out));
    for (int c = 0; c < nc; ++c) {
        const GranuleCase &g = cases[c];
        const uint8_t *t = mem.data() + (size_t)(g.skew == 0 ? 0 : g.skew == 1 ? 1 : 2) * TEXT_ROOM + 16 + g.skew;
        for (int i = 0; i < 16; ++i) {
            const int64_t p = g.s0 + i;
            const uint8_t want = p >= g.lo && p < g.n ? t[p] : (uint8_t)g.fill;
            if (out[c * 16 + i] != want && ++wrong <= 10)
                printf("granule, bounds [%lld, %lld), skew %u, s0 %lld, byte %d: %02x, expected %02x\n", (long long)g.lo, (long long)g.n, g.skew, (long long)g.s0, i, out[c * 16 + i], want);
        }
    }
    return nc;
}

static long check_last_outside(long &wrong) {
    static const uint64_t NS[6] = {0, 1, 255, 256, 257, 513};
    std::vector<uint8_t> texts;
    std::vector<uint64_t> first, len, want;
    for (int j = 0; j < 6; ++j)
        for (int shape = 0; shape < 4; ++shape) {
            const uint64_t n = NS[j], most = n ? n - 1 : 0;
            const uint64_t run = shape == 0 ? n : shape == 1 ? 0 : shape == 2 ? (most < 256 ? most : 256) : (most < 300 ? most : 300);
            first.push_back(texts.size()); len.push_back(n); want.push_back(n - run);
            for (uint64_t i = 0; i < n; ++i) {
                uint8_t c = rnd() % 5 == 0 ? '\n' : (uint8_t)('A' + rnd() % 26);            // line ends in front of the run too
                if (i + run + 1 == n) c = 'A';                                               // the last byte outside the set
                if (i + run >= n) c = (n - i) & 1 ? '\n' : '\r';
                texts.push_back(c);
            }
        }
    const size_t nc = first.size();
    texts.push_back(0);                                                  // (no empty allocation)
    uint8_t *d_t; uint64_t *d_first, *d_len; unsigned long long *d_out;
    CK(hipMalloc(&d_t, texts.size())); CK(hipMalloc(&d_first, nc * 8)); CK(hipMalloc(&d_len, nc * 8)); CK(hipMalloc(&d_out, nc * 256 * 8));
    CK(hipMemcpy(d_t, texts.data(), texts.size(), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_first, first.data(), nc * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_len, len.data(), nc * 8, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xA5, nc * 256 * 8));
    hipLaunchKernelGGL(k_last, dim3((unsigned)nc), dim3(256), 0, 0, d_t, d_first, d_len, d_out);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    std::vector<unsigned long long> out(nc * 256);
    CK(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
    CK(hipFree(d_t)); CK(hipFree(d_first)); CK(hipFree(d_len)); CK(hipFree(d_out));
    for (size_t c = 0; c < nc; ++c)
        for (int i = 0; i < 256; ++i)
            if (out[c * 256 + i] != want[c] && ++wrong <= 10)
                printf("last outside, n %llu, shape %zu, thread %d: %llu, expected %llu\n", (unsigned long long)len[c], c % 4, i, out[c * 256 + i], (unsigned long long)want[c]);
    return (long)nc;
}

static long check_codes(long &wrong) {
    uint32_t *d_out;
    std::vector<uint32_t> out(256);
    CK(hipMalloc(&d_out, 256 * 4));
    hipLaunchKernelGGL(k_codes, dim3(1), dim3(256), 0, 0, d_out);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    CK(hipMemcpy(out.data(), d_out, 256 * 4, hipMemcpyDeviceToHost));
    CK(hipFree(d_out));
    for (uint32_t c = 0; c < 256; ++c)
        if (out[c] != kdf_base_code(c) && ++wrong <= 10) printf("base code of %u: %u, on the host %u\n", c, out[c], kdf_base_code(c));
    return 256;
}

int main() {
    long wrong = 0;
    const long ng = check_granules(wrong), nl = check_last_outside(wrong), nb = check_codes(wrong);
    printf("granules: %ld cases\nlast outside: %ld cases\nbase codes: %ld cases\n%ld wrong\n", ng, nl, nb, wrong);
    return wrong ? 1 : 0;
}
