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
// Block sums, kb_block_sum (uint32 and 64-bit) and kb_block_max, workgroups of 64, 256 and 1024 threads; the scan of 64-bit
// block sums by one workgroup, kb_sums_exscan: see check_sums and check_sums_scan.
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

// one workgroup per case; every thread writes what it got
__global__ void k_sum32(const uint32_t *in, uint32_t *out) {
    __shared__ uint32_t wsum[16];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = kb_block_sum(in[i], wsum);
}
__global__ void k_sum64(const unsigned long long *in, unsigned long long *out, unsigned long long *out_max) {
    __shared__ unsigned long long wsum[16], wmax[16];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = kb_block_sum(in[i], wsum);
    out_max[i] = kb_block_max(in[i], wmax);
}

// kb_block_sum (uint32 and 64-bit; the 64-bit cases also through kb_block_max): all zeros, all ones, one non-zero value at
// lane 0 and at lane 63 of the first and of the last wave, a 32-bit sum that wraps, a 64-bit sum beyond 2^32
static long check_sums(int nt, long &wrong) {
    const int spots[4] = {0, 63, nt - 64, nt - 1};
    std::vector<std::vector<uint32_t>> c32;
    std::vector<std::vector<unsigned long long>> c64;
    c32.emplace_back(nt, 0u); c32.emplace_back(nt, 1u);
    c64.emplace_back(nt, 0ull); c64.emplace_back(nt, 1ull);
    for (int s = 0; s < 4; ++s) {
        std::vector<uint32_t> a(nt, 0u); a[spots[s]] = 0x9E3779B1u; c32.push_back(a);
        std::vector<unsigned long long> b(nt, 0ull); b[spots[s]] = 0x9E3779B97F4A7C15ull; c64.push_back(b);
    }
    { std::vector<uint32_t> a(nt); for (int i = 0; i < nt; ++i) a[i] = rnd() | 0x80000000u; c32.push_back(a); }                  // wraps from the second value on
    { std::vector<unsigned long long> b(nt); for (int i = 0; i < nt; ++i) b[i] = (unsigned long long)rnd() << 8 | 0x8000000000ull; c64.push_back(b); }   // 2^39 and more each
    const size_t n32 = c32.size(), n64 = c64.size();
    std::vector<uint32_t> in32(n32 * nt), out32(n32 * nt);
    std::vector<unsigned long long> in64(n64 * nt), out64(n64 * nt), max64(n64 * nt);
    for (size_t c = 0; c < n32; ++c) for (int i = 0; i < nt; ++i) in32[c * nt + i] = c32[c][i];
    for (size_t c = 0; c < n64; ++c) for (int i = 0; i < nt; ++i) in64[c * nt + i] = c64[c][i];
    uint32_t *d_in32, *d_out32;
    unsigned long long *d_in64, *d_out64, *d_max64;
    CK(hipMalloc(&d_in32, in32.size() * 4)); CK(hipMalloc(&d_out32, in32.size() * 4));
    CK(hipMalloc(&d_in64, in64.size() * 8)); CK(hipMalloc(&d_out64, in64.size() * 8)); CK(hipMalloc(&d_max64, in64.size() * 8));
    CK(hipMemcpy(d_in32, in32.data(), in32.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_in64, in64.data(), in64.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemset(d_out32, 0xA5, in32.size() * 4)); CK(hipMemset(d_out64, 0xA5, in64.size() * 8)); CK(hipMemset(d_max64, 0xA5, in64.size() * 8));
    hipLaunchKernelGGL(k_sum32, dim3((unsigned)n32), dim3(nt), 0, 0, d_in32, d_out32);
    hipLaunchKernelGGL(k_sum64, dim3((unsigned)n64), dim3(nt), 0, 0, d_in64, d_out64, d_max64);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    CK(hipMemcpy(out32.data(), d_out32, in32.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(out64.data(), d_out64, in64.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(max64.data(), d_max64, in64.size() * 8, hipMemcpyDeviceToHost));
    CK(hipFree(d_in32)); CK(hipFree(d_out32)); CK(hipFree(d_in64)); CK(hipFree(d_out64)); CK(hipFree(d_max64));
    for (size_t c = 0; c < n32; ++c) {
        uint32_t sum = 0;                                                // (wraps, as the device sum does)
        for (int i = 0; i < nt; ++i) sum += c32[c][i];
        for (int i = 0; i < nt; ++i)
            if (out32[c * nt + i] != sum && ++wrong <= 10) printf("block sum, %d threads, case %zu, thread %d: %u, expected %u\n", nt, c, i, out32[c * nt + i], sum);
    }
    for (size_t c = 0; c < n64; ++c) {
        unsigned long long sum = 0, mx = 0;
        for (int i = 0; i < nt; ++i) { sum += c64[c][i]; mx = c64[c][i] > mx ? c64[c][i] : mx; }
        for (int i = 0; i < nt; ++i) {
            if (out64[c * nt + i] != sum && ++wrong <= 10) printf("block sum (64), %d threads, case %zu, thread %d: %llu, expected %llu\n", nt, c, i, out64[c * nt + i], sum);
            if (max64[c * nt + i] != mx && ++wrong <= 10) printf("block max (64), %d threads, case %zu, thread %d: %llu, expected %llu\n", nt, c, i, max64[c * nt + i], mx);
        }
    }
    return (long)(n32 + n64);
}

// kb_sums_exscan by one workgroup of 256: the total comes back through every thread
constexpr int SUMS_GUARD = 8;
__global__ __launch_bounds__(256) void k_sums(unsigned long long *sums, uint64_t n, unsigned long long *tot) {
    __shared__ unsigned long long ws[4];
    tot[threadIdx.x] = kb_sums_exscan(sums, n, ws);
}

// n = 0, 1, 255, 256, 257, 511, 513, 65 537; random values below 2^40, and values 1 << 32 | len, len < 2^20, as the FASTQ
// extract scans them (records in the high half, bytes in the low half: the halves scan independently while the lengths
// sum to less than 2^32, which they do up to n = 513).  Nothing at or past sums[n] may be written.
static long check_sums_scan(long &wrong) {
    static const uint64_t NS[8] = {0, 1, 255, 256, 257, 511, 513, 65537};
    long cases = 0;
    for (int form = 0; form < 2; ++form) {
        for (int c = 0; c < 8; ++c, ++cases) {
            const uint64_t n = NS[c];
            std::vector<unsigned long long> in(n + SUMS_GUARD, 0xFEEDF00DFEEDF00Dull), out(n + SUMS_GUARD), tot(256);
            for (uint64_t i = 0; i < n; ++i)
                in[i] = form ? 1ull << 32 | (rnd() >> 12) : (unsigned long long)rnd() << 8 | (rnd() & 0xFFu);
            unsigned long long *d_s, *d_t;
            CK(hipMalloc(&d_s, in.size() * 8)); CK(hipMalloc(&d_t, 256 * 8));
            CK(hipMemcpy(d_s, in.data(), in.size() * 8, hipMemcpyHostToDevice)); CK(hipMemset(d_t, 0xA5, 256 * 8));
            hipLaunchKernelGGL(k_sums, dim3(1), dim3(256), 0, 0, d_s, n, d_t);
            CK(hipGetLastError()); CK(hipDeviceSynchronize());
            CK(hipMemcpy(out.data(), d_s, in.size() * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(tot.data(), d_t, 256 * 8, hipMemcpyDeviceToHost));
            CK(hipFree(d_s)); CK(hipFree(d_t));
            unsigned long long run = 0, bytes = 0;
            for (uint64_t i = 0; i < n; ++i) {
                if (out[i] != run && ++wrong <= 10) printf("sums scan, form %d, n %llu: [%llu] = %llu, expected %llu\n", form, (unsigned long long)n, (unsigned long long)i, out[i], run);
                if (form && n <= 513 && (out[i] >> 32 != i || (out[i] & 0xFFFFFFFFull) != bytes) && ++wrong <= 10)
                    printf("sums scan, n %llu: the halves of [%llu] = %llx are not (%llu, %llu)\n", (unsigned long long)n, (unsigned long long)i, out[i], (unsigned long long)i, bytes);
                run += in[i]; bytes += in[i] & 0xFFFFFFFFull;
            }
            for (int i = 0; i < SUMS_GUARD; ++i)
                if (out[n + i] != 0xFEEDF00DFEEDF00Dull && ++wrong <= 10) printf("sums scan, form %d, n %llu: [n + %d] was written\n", form, (unsigned long long)n, i);
            for (int i = 0; i < 256; ++i)
                if (tot[i] != run && ++wrong <= 10) printf("sums scan, form %d, n %llu: thread %d got the total %llu, expected %llu\n", form, (unsigned long long)n, i, tot[i], run);
        }
    }
    return cases;
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
    long nsum = 0;
    static const int SUM_NTS[3] = {64, 256, 1024};
    for (int i = 0; i < 3; ++i) nsum += check_sums(SUM_NTS[i], wrong);
    const long nscan = check_sums_scan(wrong);
    printf("block scans: %ld cases\nstrip scans: %ld cases\nblock sums: %ld cases\nsums scans: %ld cases\n%ld wrong\n", nblock, nstrip, nsum, nscan, wrong);
    return wrong ? 1 : 0;
}
