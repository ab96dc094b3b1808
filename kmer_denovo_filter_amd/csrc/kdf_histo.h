// kdf_histo.h -- the count histogram and the table statistics (`jellyfish histo` / `jellyfish stats` on a finished
// table), one pass over the 4-byte count array for every key width.
//
// The distribution is as skewed as a histogram gets: at load <= 0.5 half of the slots are empty, and most of the
// rest hold 1 (sequencing errors).  So the values nearly every slot has -- empty, 0, 1 .. KH_REG - 1 -- are tallied in
// registers per thread and never touch LDS; counts from KH_REG up to KH_LDS_BINS - 1 go to a workgroup-private LDS
// histogram (uint32: a workgroup sees far fewer than 2^32 slots), counts above that but <= high straight to the global
// bins (repeats: rare), counts above `high` to a register again.  A persistent grid strides over the table with 16-byte
// loads of four counts per lane; at its end a workgroup flushes its NON-ZERO bins with one global atomic each.
//
// A slot with count > 0 is occupied by construction (km_count_kernel relies on the same fact), so the key words are
// read only for a slot whose count is 0, and only when `occ` is given: the host passes the array of the word that
// tells an empty slot (t.lo narrow, t.hi wide, the top word of long keys) only for a table that can hold keys with
// count 0 at all (a count --if filter, added pairs, reset or set counts).  An ordinary insert-mode table is described
// from 4 bytes per slot.
#pragma once
#include "kdf_device.h"

#define KH_THREADS   256
#define KH_WG_PER_CU 6                    // what 76 VGPRs admit (6 waves per SIMD); 6 x 16 KB of LDS bins per CU
#define KH_UNROLL    4                    // 16-byte loads in flight per lane
#define KH_REG       4u                   // counts below this are tallied in registers
#define KH_LDS_BINS  4096u                // counts below this (and <= high) in the workgroup's LDS bins
#define KH_MAX_HIGH  ((1u << 24) - 1)     // largest `high` kdf_histogram* accept (128 MB of bins)

// bins[high + 2] and stats[2] = {sum of all counts, largest count} must be zero at launch; cap is a multiple of 4.
__global__ __launch_bounds__(KH_THREADS) void kdf_histo_kernel(
    const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ occ, uint64_t cap, uint32_t high,
    unsigned long long *__restrict__ bins, unsigned long long *__restrict__ stats)
{
    __shared__ uint32_t lbin[KH_LDS_BINS];
    __shared__ unsigned long long wred[KH_THREADS / 64][KH_REG + 3];
    for (uint32_t i = threadIdx.x; i < KH_LDS_BINS; i += KH_THREADS) lbin[i] = 0;
    __syncthreads();

    uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0, over = 0, mx = 0;    // per thread: < 2^32 slots each
    unsigned long long total = 0;
    const uint64_t nvec = cap >> 2, stride = (uint64_t)gridDim.x * KH_THREADS;
    for (uint64_t v0 = (uint64_t)blockIdx.x * KH_THREADS + threadIdx.x; v0 < nvec; v0 += stride * KH_UNROLL) {
        uint4 q[KH_UNROLL];
#pragma unroll
        for (int u = 0; u < KH_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)u * stride;
            q[u] = v < nvec ? ((const uint4 *)cnt)[v] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < KH_UNROLL; ++u) {
            const uint64_t v = v0 + (uint64_t)u * stride;
            const uint32_t c4[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t c = c4[j];
                if (c == 0) {                                     // empty, or a stored key never counted
                    if (occ && v < nvec) n0 += occ[v * 4 + j] != KDF_EMPTY ? 1u : 0u;
                    continue;
                }
                total += c;
                mx = max(mx, c);
                n1 += c == 1 ? 1u : 0u; n2 += c == 2 ? 1u : 0u; n3 += c == 3 ? 1u : 0u;
                if (c < KH_REG) continue;
                if (c > high) over++;
                else if (c < KH_LDS_BINS) atomicAdd(&lbin[c], 1u);
                else atomicAdd(&bins[c], 1ull);
            }
        }
    }

    unsigned long long r[KH_REG + 2] = {n0, n1, n2, n3, over, total};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < (int)KH_REG + 2; ++i) r[i] += __shfl_xor(r[i], o);
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < (int)KH_REG + 2; ++i) wred[threadIdx.x >> 6][i] = r[i];
        wred[threadIdx.x >> 6][KH_REG + 2] = mx;
    }
    __syncthreads();
    if (threadIdx.x < KH_REG + 3) {                               // one lane per tally: n0..n3, over, total, max
        const uint32_t i = threadIdx.x;
        unsigned long long s = 0;
        for (int w = 0; w < KH_THREADS / 64; ++w) s = i == KH_REG + 2 ? max(s, wred[w][i]) : s + wred[w][i];
        if (s) {
            if (i < KH_REG) atomicAdd(&bins[min(i, high + 1)], s);        // a register bin above `high` is overflow
            else if (i == KH_REG) atomicAdd(&bins[high + 1], s);
            else if (i == KH_REG + 1) atomicAdd(&stats[0], s);
            else atomicMax(&stats[1], s);
        }
    }
    for (uint32_t i = threadIdx.x; i < KH_LDS_BINS; i += KH_THREADS) {    // only counts <= high were binned here
        const uint32_t x = lbin[i];
        if (x) atomicAdd(&bins[i], (unsigned long long)x);
    }
}
