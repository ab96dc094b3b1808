// kdf_scan.h -- the block-level sums of every kernel: wave and block prefix sums on DPP (the binned pipeline, kdf_binned.h,
// the feeders, and the list kernels of hits, coverage, regions, the spool and the k-mer FASTA parse), block sums, and the
// single-workgroup scan of 64-bit block sums.  Self-contained (HIP runtime only), so that a stand-alone program can include
// it: tests/native/block_scan_check.hip.
//
// A wave64 scan by __shfl_up is six ds_bpermute_b32, each a dependent round trip through the LDS pipe -- the pipe the
// partition kernels are bound by.  The same scan on DPP is six v_add_u32_dpp and no LDS traffic: row_shr:1/2/4/8 inside
// the rows of 16 lanes, then lane 15 of a row added to the next row (row_bcast:15, rows 1 and 3), then lane 31 to rows 2
// and 3 (row_bcast:31).  A lane whose DPP source does not exist, or whose row is masked off, adds `old` = 0.  The compiler
// inserts the wait states DPP needs.  uint32 arithmetic wraps, as it did in the shuffles.
// EVERY lane of the wave must be active at the call (a disabled source lane would add 0 instead of its value).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t kb_dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// inclusive prefix sum inside every row of 16 lanes
__device__ __forceinline__ uint32_t kb_row_incl_scan(uint32_t v) {
    v = kb_dpp_add<0x111, 0xf>(v);                                      // row_shr:1
    v = kb_dpp_add<0x112, 0xf>(v);                                      // row_shr:2
    v = kb_dpp_add<0x114, 0xf>(v);                                      // row_shr:4
    v = kb_dpp_add<0x118, 0xf>(v);                                      // row_shr:8
    return v;
}
// inclusive / exclusive prefix sum over the 64 lanes of the wave
__device__ __forceinline__ uint32_t kb_wave_incl_scan(uint32_t v) {
    v = kb_row_incl_scan(v);
    v = kb_dpp_add<0x142, 0xa>(v);                                      // row_bcast:15 into rows 1 and 3
    v = kb_dpp_add<0x143, 0xc>(v);                                      // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ uint32_t kb_wave_excl_scan(uint32_t v) { return kb_wave_incl_scan(v) - v; }

// Barrier that orders LDS traffic only.  __syncthreads() also drains vmcnt(0),
// i.e. waits for every outstanding global store; in the slab kernel that would
// serialise a slab's write-out with the next slab's compute.  The barriers there protect LDS data only.
__device__ __forceinline__ void kb_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// Second level of a block scan: the nw <= 16 wave totals lie in wsum[0 .. nw).  EVERY wave reads them (one broadcast read
// per row of 16 lanes) and scans them inside its rows -- no hop through wave 0 and no barrier for it.  Returns the sum of
// the waves before `wave` (wave-uniform), the block's total through tot.
__device__ __forceinline__ uint32_t kb_wave_sums_before(const uint32_t *wsum, uint32_t tid, uint32_t nw, uint32_t &tot) {
    const uint32_t l16 = tid & 15u;
    const uint32_t sv = l16 < nw ? wsum[l16] : 0u, si = kb_row_incl_scan(sv);
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    tot = (uint32_t)__builtin_amdgcn_readlane((int)si, 15);
    return (uint32_t)__builtin_amdgcn_readlane((int)(si - sv), wave);
}

// block-wide exclusive scan of n <= blockDim.x uint32 values held one per
// thread (threads >= n pass 0); returns the exclusive prefix, total via *tot.
// (blockDim.x: a multiple of 64, at most 1024)
__device__ __forceinline__ uint32_t kb_block_exscan(uint32_t v, uint32_t *wsum /* >= 17 words LDS */, uint32_t *tot) {
    const uint32_t inc = kb_wave_incl_scan(v);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t total;
    const uint32_t r = kb_wave_sums_before(wsum, threadIdx.x, blockDim.x >> 6, total) + inc - v;
    if (tot) *tot = total;
    __syncthreads();                                                    // (wsum is written again by the caller's next scan)
    return r;
}

// the same for a workgroup of NT threads between barriers that order LDS traffic only; tid: the thread index
template <int NT>
__device__ __forceinline__ uint32_t kb_block_exscan_lds(uint32_t v, uint32_t *wsum /* >= 17 words LDS */, uint32_t tid) {
    const uint32_t inc = kb_wave_incl_scan(v);
    if ((tid & 63u) == 63u) wsum[tid >> 6] = inc;
    kb_lds_barrier();
    uint32_t total;
    const uint32_t r = kb_wave_sums_before(wsum, tid, NT >> 6, total) + inc - v;
    kb_lds_barrier();                                  // (not needed by the pipelined piece sort, whose stages put barriers of their own before
                                                       // wsum is written again -- but without it, and without the barrier that ends an iteration,
                                                       // the kernel measured 4.65-4.67 against 4.59 ms: waves that stay in phase share the LDS better)
    return r;
}

// The same scan in two halves around a barrier that the CALLER places, for a loop whose stages have barriers of their own
// (the pipelined piece sort, kdf_binned.h): kb_block_exscan_publish before the barrier (returns the lane's inclusive wave
// prefix, which the caller keeps), kb_block_exscan_finish after it.  No barrier inside: the caller's barriers also keep
// wsum from being written again before every wave has read it.  Several scans share one barrier, each with its own wsum.
__device__ __forceinline__ uint32_t kb_block_exscan_publish(uint32_t v, uint32_t *wsum /* >= 16 words LDS */, uint32_t tid) {
    const uint32_t inc = kb_wave_incl_scan(v);
    if ((tid & 63u) == 63u) wsum[tid >> 6] = inc;
    return inc;
}
template <int NT>
__device__ __forceinline__ uint32_t kb_block_exscan_finish(uint32_t v, uint32_t inc, const uint32_t *wsum, uint32_t tid) {
    uint32_t total;
    return kb_wave_sums_before(wsum, tid, NT >> 6, total) + inc - v;
}

// Kernel A's strip scan, by ONE wave with all its lanes (lane = 0 .. 63): offs[0 .. nb) = the exclusive prefix of
// hist[0 .. nb), offs[nb] = the total.  nb = 1, 2, 4 .. 1024; hist and offs are 16-byte aligned.  A lane owns
// per = max(1, nb / 64) consecutive bins: 16-byte LDS reads and writes from per = 4 on.  Its first four bins stay in
// registers across the wave scan (nb = 256, the bench geometry: one read, one write per lane); the further ones of
// nb = 512 and 1024 are read again, one quad at a time, rather than held -- kernel A has no register to spare.
__device__ __forceinline__ void kb_strip_exscan(const uint32_t *hist, uint32_t *offs, int nb, uint32_t lane) {
    if (nb >= 256) {
        const int nq = nb >> 8;                                         // quads per lane: 1, 2, 4
        const uint4 *h4 = (const uint4 *)hist + lane * nq;
        uint4 *o4 = (uint4 *)offs + lane * nq;
        const uint4 q = h4[0];
        uint32_t sum = q.x + q.y + q.z + q.w;
#pragma unroll 1
        for (int i = 1; i < nq; ++i) { const uint4 t = h4[i]; sum += t.x + t.y + t.z + t.w; }
        const uint32_t inc = kb_wave_incl_scan(sum);
        uint32_t run = inc - sum;
        o4[0] = make_uint4(run, run + q.x, run + q.x + q.y, run + q.x + q.y + q.z);
        run += q.x + q.y + q.z + q.w;
#pragma unroll 1
        for (int i = 1; i < nq; ++i) {
            const uint4 t = h4[i];
            o4[i] = make_uint4(run, run + t.x, run + t.x + t.y, run + t.x + t.y + t.z);
            run += t.x + t.y + t.z + t.w;
        }
        if (lane == 63) offs[nb] = inc;
    } else if (nb == 128) {
        const uint2 q = ((const uint2 *)hist)[lane];
        const uint32_t sum = q.x + q.y, inc = kb_wave_incl_scan(sum);
        ((uint2 *)offs)[lane] = make_uint2(inc - sum, inc - sum + q.x);
        if (lane == 63) offs[nb] = inc;
    } else {                                                            // nb <= 64: a bin per lane
        const uint32_t v = (int)lane < nb ? hist[lane] : 0u, inc = kb_wave_incl_scan(v);
        if ((int)lane < nb) offs[lane] = inc - v;
        if (lane == 63) offs[nb] = inc;                                 // (the lanes from nb on added nothing)
    }
}

// Sum of v over the workgroup, to every thread.  ONE barrier: the caller puts a barrier of its own before wsum is written
// again.  uint32 on the DPP scan (every lane active, blockDim.x a multiple of 64, at most 1024; the sum wraps); 64-bit
// values, which DPP does not add, on a butterfly of shuffles -- also in max form.
__device__ __forceinline__ uint32_t kb_block_sum(uint32_t v, uint32_t *wsum /* blockDim.x / 64 words LDS */) {
    const uint32_t inc = kb_wave_incl_scan(v);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t total;
    kb_wave_sums_before(wsum, threadIdx.x, blockDim.x >> 6, total);
    return total;
}
template <bool MAX>
__device__ __forceinline__ unsigned long long kb_block_reduce64(unsigned long long v, unsigned long long *wsum /* blockDim.x / 64 words LDS */) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_xor(v, o); v = MAX ? (y > v ? y : v) : v + y; }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    v = wsum[0];
    for (uint32_t j = 1; j < blockDim.x >> 6; ++j) { const unsigned long long y = wsum[j]; v = MAX ? (y > v ? y : v) : v + y; }
    return v;
}
__device__ __forceinline__ unsigned long long kb_block_sum(unsigned long long v, unsigned long long *wsum) { return kb_block_reduce64<false>(v, wsum); }
__device__ __forceinline__ unsigned long long kb_block_max(unsigned long long v, unsigned long long *wsum) { return kb_block_reduce64<true>(v, wsum); }

// The scan of the 64-bit sums of a grid's workgroups by ONE workgroup of 256 threads: sums[0 .. n) -> their exclusive
// prefix sums, in place, 256 at a time; returns the total to every thread.  Writes nothing but sums[0 .. n).  Sums of two
// 32-bit halves that never carry into each other (kdf_fastqfeed.h: kept << 32 | bytes) scan as two independent sums.
__device__ __forceinline__ unsigned long long kb_sums_exscan(unsigned long long *__restrict__ sums, uint64_t n, unsigned long long *ws /* 4 words LDS */) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n; base += 256) {
        const uint64_t i = base + threadIdx.x;
        const unsigned long long v = i < n ? sums[i] : 0;
        unsigned long long inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_up(inc, o); if (lane >= o) inc += y; }
        if (lane == 63) ws[wv] = inc;
        __syncthreads();
        unsigned long long pre = 0, total = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const unsigned long long s = ws[j]; pre += j < wv ? s : 0; total += s; }
        if (i < n) sums[i] = carry + pre + inc - v;
        carry += total;
        __syncthreads();
    }
    return carry;
}
