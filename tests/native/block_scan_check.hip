// block_scan_check.hip -- the wave / block prefix sums of csrc/kdf_scan.h and kernel A's strip scan against host prefix
// sums.  Stand-alone (hipcc --offload-arch=gfx950 -O3 -I<csrc>): exit status 0 = every case equal.
//
// Block scans, kb_block_exscan (prefix and total) and kb_block_exscan_lds<NT> (prefix), workgroups of 64, 128, 256, 512,
// 768 and 1024 threads: all zeros, all ones, the lane index, random values whose sum stays below 2^32, random values whose
// sum wraps (results modulo 2^32), and one non-zero value at lane 0, 15, 16, 31, 32, 47, 48 or 63 (both ends of every DPP
// row) of the first, a middle and the last wave.
// Strip scan, kb_strip_exscan by wave 0 of a 1024-thread workgroup as in kb_slabsort_kernel: nb = 1, 2, 4 .. 1024; all
// zeros, all ones, a slab's 16 384 windows in the first bin / in the last bin / spread at random / at random over every
// third bin; nothing past offs[nb] may be written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "kdf_scan.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(2); } } while (0)

// one workgroup per case: in / out [case][nt], tot [case]
__global__ void k_block(const uint32_t *in, uint32_t *out, uint32_t *tot) {
    __shared__ uint32_t wsum[32];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t t = 0xDEADBEEFu;
    out[i] = kb_block_exscan(in[i], wsum, &t);
    if (threadIdx.x == blockDim.x - 1) tot[blockIdx.x] = t;
}
template <int NT>
__global__ __launch_bounds__(NT) void k_block_lds(const uint32_t *in, uint32_t *out) {
    __shared__ uint32_t wsum[32];
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    const uint32_t v = in[i];
    // twice, as the piece sort calls it back to back on one wsum; the second scan is the one that is kept
    const uint32_t a = kb_block_exscan_lds<NT>(v ^ 0x5Au, wsum, threadIdx.x);
    const uint32_t b = kb_block_exscan_lds<NT>(v, wsum, threadIdx.x);
    out[i] = b + (a & 0u);
}

constexpr int NB_MAX = 1024, STRIP_WORDS = NB_MAX + 1 + 15;            // offs[0 .. nb] and a guard behind them
__global__ __launch_bounds__(1024) void k_strip(const uint32_t *in, uint32_t *out, int nb) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[NB_MAX];
    __shared__ __attribute__((aligned(16))) uint32_t offs[STRIP_WORDS];
    const uint32_t *src = in + (size_t)blockIdx.x * NB_MAX;
    for (int i = threadIdx.x; i < NB_MAX; i += blockDim.x) hist[i] = src[i];
    for (int i = threadIdx.x; i < STRIP_WORDS; i += blockDim.x) offs[i] = 0xFEEDF00Du;
    kb_lds_barrier();
    if (threadIdx.x < 64) kb_strip_exscan(hist, offs, nb, threadIdx.x);
    kb_lds_barrier();
    uint32_t *dst = out + (size_t)blockIdx.x * STRIP_WORDS;
    for (int i = threadIdx.x; i < STRIP_WORDS; i += blockDim.x) dst[i] = offs[i];
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {                                                  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static long check_blocks(int nt, long &wrong) {
    static const int LANES[8] = {0, 15, 16, 31, 32, 47, 48, 63};
    const int nw = nt / 64, waves[3] = {0, nw / 2, nw - 1};
    std::vector<std::vector<uint32_t>> cases;
    cases.emplace_back(nt, 0u);
    cases.emplace_back(nt, 1u);
    { std::vector<uint32_t> v(nt); for (int i = 0; i < nt; ++i) v[i] = i & 63; cases.push_back(v); }
    { std::vector<uint32_t> v(nt); for (int i = 0; i < nt; ++i) v[i] = rnd() >> 12; cases.push_back(v); }        // < 2^20 each: sum < 2^30
    { std::vector<uint32_t> v(nt); for (int i = 0; i < nt; ++i) v[i] = rnd() | 0x80000000u; cases.push_back(v); } // wraps from the second value on
    for (int w = 0; w < 3; ++w)
        for (int l = 0; l < 8; ++l) { std::vector<uint32_t> v(nt, 0u); v[waves[w] * 64 + LANES[l]] = 0x9E3779B1u; cases.push_back(v); }
    const size_t nc = cases.size(), n = nc * nt;
    std::vector<uint32_t> in(n), out(n), out2(n), tot(nc);
    for (size_t c = 0; c < nc; ++c) for (int i = 0; i < nt; ++i) in[c * nt + i] = cases[c][i];
    uint32_t *d_in, *d_out, *d_out2, *d_tot;
    CK(hipMalloc(&d_in, n * 4)); CK(hipMalloc(&d_out, n * 4)); CK(hipMalloc(&d_out2, n * 4)); CK(hipMalloc(&d_tot, nc * 4));
    CK(hipMemcpy(d_in, in.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xA5, n * 4)); CK(hipMemset(d_out2, 0xA5, n * 4)); CK(hipMemset(d_tot, 0xA5, nc * 4));
    hipLaunchKernelGGL(k_block, dim3((unsigned)nc), dim3(nt), 0, 0, d_in, d_out, d_tot);
    switch (nt) {
    case 64:   hipLaunchKernelGGL(k_block_lds<64>, dim3((unsigned)nc), dim3(nt), 0, 0, d_in, d_out2); break;
    case 128:  hipLaunchKernelGGL(k_block_lds<128>, dim3((unsigned)nc), dim3(nt), 0, 0, d_in, d_out2); break;
    case 256:  hipLaunchKernelGGL(k_block_lds<256>, dim3((unsigned)nc), dim3(nt), 0, 0, d_in, d_out2); break;
    case 512:  hipLaunchKernelGGL(k_block_lds<512>, dim3((unsigned)nc), dim3(nt), 0, 0, d_in, d_out2); break;
    case 768:  hipLaunchKernelGGL(k_block_lds<768>, dim3((unsigned)nc), dim3(nt), 0, 0, d_in, d_out2); break;
    case 1024: hipLaunchKernelGGL(k_block_lds<1024>, dim3((unsigned)nc), dim3(nt), 0, 0, d_in, d_out2); break;
    default: printf("no instantiation for %d threads\n", nt); exit(2);
    }
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    CK(hipMemcpy(out.data(), d_out, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(out2.data(), d_out2, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(tot.data(), d_tot, nc * 4, hipMemcpyDeviceToHost));
    CK(hipFree(d_in)); CK(hipFree(d_out)); CK(hipFree(d_out2)); CK(hipFree(d_tot));
    for (size_t c = 0; c < nc; ++c) {
        uint32_t run = 0;                                                // (wraps, as the device sums do)
        for (int i = 0; i < nt; ++i) {
            const uint32_t a = out[c * nt + i], b = out2[c * nt + i];
            if (a != run || b != run) {
                if (++wrong <= 10) printf("block scan, %d threads, case %zu, thread %d: %u (lds: %u), expected %u\n", nt, c, i, a, b, run);
            }
            run += in[c * nt + i];
        }
        if (tot[c] != run && ++wrong <= 10) printf("block scan, %d threads, case %zu: total %u, expected %u\n", nt, c, tot[c], run);
    }
    return (long)nc * 2;
}

static long check_strips(long &wrong) {
    constexpr uint32_t SLAB = 16384;
    std::vector<int> nbs; std::vector<std::vector<uint32_t>> cases;
    for (int nb = 1; nb <= NB_MAX; nb <<= 1) {
        for (int pat = 0; pat < 6; ++pat) {
            std::vector<uint32_t> h(NB_MAX, 0x01010101u);                // (what lies past nb must not be read into the sums)
            for (int i = 0; i < nb; ++i) h[i] = 0;
            if (pat == 1) for (int i = 0; i < nb; ++i) h[i] = 1;
            if (pat == 2) h[0] = SLAB;
            if (pat == 3) h[nb - 1] = SLAB;
            if (pat == 4) for (uint32_t j = 0; j < SLAB; ++j) ++h[rnd() % nb];
            if (pat == 5) for (uint32_t j = 0; j < SLAB - 3; ++j) ++h[(rnd() % nb) / 3 * 3];
            nbs.push_back(nb); cases.push_back(h);
        }
    }
    const size_t nc = cases.size();
    std::vector<uint32_t> in(nc * NB_MAX), out(nc * STRIP_WORDS);
    for (size_t c = 0; c < nc; ++c) for (int i = 0; i < NB_MAX; ++i) in[c * NB_MAX + i] = cases[c][i];
    uint32_t *d_in, *d_out;
    CK(hipMalloc(&d_in, in.size() * 4)); CK(hipMalloc(&d_out, out.size() * 4));
    CK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xA5, out.size() * 4));
    // one launch per case (nb is a kernel argument, as the plan is in the product); blockIdx.x is 0: the case's arrays are passed
    for (size_t c = 0; c < nc; ++c)
        hipLaunchKernelGGL(k_strip, dim3(1), dim3(1024), 0, 0, d_in + c * NB_MAX, d_out + c * STRIP_WORDS, nbs[c]);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    CK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CK(hipFree(d_in)); CK(hipFree(d_out));
    for (size_t c = 0; c < nc; ++c) {
        const int nb = nbs[c];
        uint32_t run = 0;
        for (int i = 0; i <= nb; ++i) {
            const uint32_t a = out[c * STRIP_WORDS + i];
            if (a != run && ++wrong <= 10) printf("strip scan, nb %d, case %zu, offs[%d] = %u, expected %u\n", nb, c % 6, i, a, run);
            if (i < nb) run += cases[c][i];
        }
        for (int i = nb + 1; i < STRIP_WORDS; ++i)
            if (out[c * STRIP_WORDS + i] != 0xFEEDF00Du && ++wrong <= 10) printf("strip scan, nb %d, case %zu: offs[%d] was written\n", nb, c % 6, i);
    }
    return (long)nc;
}

int main() {
    long wrong = 0, nblock = 0;
    static const int NTS[6] = {64, 128, 256, 512, 768, 1024};
    for (int i = 0; i < 6; ++i) nblock += check_blocks(NTS[i], wrong);
    const long nstrip = check_strips(wrong);
    printf("block scans: %ld cases\nstrip scans: %ld cases\n%ld wrong\n", nblock, nstrip, wrong);
    return wrong ? 1 : 0;
}
