// kdf_text.h -- what the kernels that read raw text share (the FASTA and FASTQ feeders, the k-mer FASTA parse, the ALT
// alleles of kdf_variants.h): the base code, the 16-byte granule load and the backward search for the end of the text
// proper.  Stand-alone program: tests/native/text_tile_check.hip.
#pragma once
#include "kdf_device.h"

// A/C/G/T in either case -> 0 .. 3, anything else -> 4
KDF_HD uint32_t kdf_base_code(uint8_t c) {
    const uint32_t u = c & 0xDFu, x = (u >> 1) & 3u;
    return (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? x ^ (x >> 1) : 4u;
}

#if defined(__HIP__)

// The 16 text bytes [s0, s0 + 16) as four little-endian words; s0 may be negative, and a byte outside [lo, hi) reads as
// `fill`.  A granule that lies inside the bounds is ONE 16-byte load when the caller vouches for its address (`aligned`:
// t + s0 is a multiple of 16); any other granule is read byte by byte, inside the bounds only.
__device__ __forceinline__ uint4 kt_load_granule(const uint8_t *__restrict__ t, int64_t s0, int64_t lo, int64_t hi, bool aligned, uint32_t fill) {
    if (aligned && s0 >= lo && s0 + 16 <= hi) return *reinterpret_cast<const uint4 *>(t + s0);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t p = s0 + i;
        if (p >= lo && p < hi) w[i >> 2] |= (uint32_t)t[p] << (8 * (i & 3));
        else w[i >> 2] |= fill << (8 * (i & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// The offset just behind the last byte of t[0 .. n) for which pred is FALSE, 0 when it holds for every byte: the end of
// the text in front of a trailing run.  A backward search, 256 bytes a round; every thread gets the result.
// REQUIRES blockDim.x == 256 and a block-uniform call that every thread of the workgroup reaches (barriers inside).  The
// LDS word is the function's own: one call per kernel, or a barrier of the caller's between two.
template <class Pred>
__device__ __forceinline__ uint64_t kt_last_outside(const uint8_t *__restrict__ t, uint64_t n, Pred pred) {
    __shared__ unsigned long long last;
    if (threadIdx.x == 0) last = 0;
    __syncthreads();
    unsigned long long found = 0;
    for (uint64_t end = n; end > 0 && !found; end -= end < 256 ? end : 256) {
        if (threadIdx.x < end && !pred(t[end - 1 - threadIdx.x])) atomicMax(&last, (unsigned long long)(end - threadIdx.x));
        __syncthreads();
        found = last;
        __syncthreads();                                               // (nobody raises it again before everybody has read it)
    }
    return found;
}

#endif  // __HIP__
