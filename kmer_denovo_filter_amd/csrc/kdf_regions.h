// kdf_regions.h -- the last step of Module 3 on the device (kdf_cluster_intervals*, kdf_group_distinct*): informative
// reads to regions, and the distinct k-mers of every region.  The table and the stream are not touched; both take
// plain arrays.  The SORT is the library sort (kdf_sort_perm_device, kdf_sort.h: stable LSD radix passes that carry a
// uint32 permutation); the kernels here run over the sorted order, LANE PER SORTED ENTRY, and reach the caller's arrays
// through the permutation -- nothing is gathered into a sorted copy.
//
// Clustering (order: start, then stably chrom; skipped intervals carry the top chrom key and end up behind the rest):
//   1. kr_chrom_key_kernel   the chrom word of the sort: rank, or the top key for chrom < 0
//   2. kr_max_block_kernel   per workgroup of KR_BLOCK sorted entries: the maximum of (chrom + 1, end), compared as a
//                            PAIR, chrom first.  The order is chrom ascending, so the running maximum of the pair is the
//                            running maximum of `end` within the current chrom: it restarts at a contig change by
//                            itself, without a segmented scan, and 31 + 62 bits need no packing into one word.
//   3. kr_max_scan_kernel    exclusive scan of the block maxima with that operator (one workgroup, rounds of 256)
//   4. kr_flag_kernel        apply: the exclusive prefix E_i of every entry -> its boundary flag (first of its chrom, or
//                            start > E_i + merge_distance), and the flags per block for the next scan
//   5. kh_scan_kernel        (kdf_hits.h) exclusive sums of the block flag counts; the total is the number of regions
//   6. kr_regions_kernel     region index = flags before and at the entry - 1; region_of through the permutation, the
//                            boundary lane writes (chrom, start), and runs of equal region inside a wave (neighbours:
//                            the order is sorted) are reduced on shuffles and ballots and send ONE atomicMax (end) and
//                            ONE atomicAdd (members) per (wave, region).  A region of any size spans any number of
//                            workgroups; no lane walks its region.
// Distinct rows per group (order: rows of words + 1 words, the group on top, ignored entries in a top group):
//   7. kr_group_key_kernel   the group word of the sort: group, or n_groups for an entry that is ignored
//   8. kr_distinct_kernel    head = the row or the group differs from the predecessor's in ANY word (the full rows are
//                            compared, never a hash); heads of a run of equal group inside a wave are counted on
//                            ballots: one atomicAdd per (wave, group).
// All results are integer sums and maxima: they do not depend on the order the atomics land in.
#pragma once
#include "kdf_device.h"
#include "kdf_scan.h"

#define KR_BLOCK 256                      // sorted entries per workgroup, one per thread

// (chrom + 1, end) of a sorted entry; c == 0: none (a skipped interval, past n, nothing before)
struct KrMax { uint32_t c; unsigned long long e; };
__device__ __forceinline__ KrMax kr_max(const KrMax a, const KrMax b) { return (b.c > a.c || (b.c == a.c && b.e > a.e)) ? b : a; }
__device__ __forceinline__ KrMax kr_shfl_up(const KrMax v, int o) { return KrMax{(uint32_t)__shfl_up(v.c, o), (unsigned long long)__shfl_up(v.e, o)}; }
// chrom ranks are below 2^31 (a precondition): the low 31 bits are the sort key and the scan's first word alike
__device__ __forceinline__ uint32_t kr_rank(int64_t chrom) { return (uint32_t)chrom & 0x7FFFFFFFu; }

__device__ __forceinline__ KrMax kr_load(const int64_t *__restrict__ chrom, const int64_t *__restrict__ end, const uint32_t *__restrict__ perm,
                                         uint64_t n, uint64_t i) {
    if (i >= n) return KrMax{0, 0};
    const uint32_t e = perm[i];
    const int64_t c = chrom[e];
    return c < 0 ? KrMax{0, 0} : KrMax{kr_rank(c) + 1, (unsigned long long)end[e]};
}

// the maximum over the threads before this one in the workgroup, and over all of them; ws: 4 KrMax of LDS
__device__ __forceinline__ KrMax kr_block_excl(const KrMax v, KrMax *ws, KrMax &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    KrMax inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const KrMax y = kr_shfl_up(inc, o); if (lane >= o) inc = kr_max(y, inc); }
    if (lane == 63) ws[wv] = inc;
    KrMax ex = kr_shfl_up(inc, 1);
    if (lane == 0) ex = KrMax{0, 0};
    __syncthreads();
    KrMax pre{0, 0};
    total = KrMax{0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) { const KrMax s = ws[j]; if (j < wv) pre = kr_max(pre, s); total = kr_max(total, s); }
    __syncthreads();
    return kr_max(pre, ex);
}

__global__ __launch_bounds__(256) void kr_chrom_key_kernel(const int64_t *__restrict__ chrom, uint64_t n, uint64_t *__restrict__ key) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const int64_t c = chrom[i]; key[i] = c < 0 ? 0x80000000ull : (uint64_t)kr_rank(c); }
}

__global__ __launch_bounds__(256) void kr_max_block_kernel(const int64_t *__restrict__ chrom, const int64_t *__restrict__ end,
                                                           const uint32_t *__restrict__ perm, uint64_t n, KrMax *__restrict__ agg) {
    __shared__ KrMax ws[4];
    KrMax total;
    kr_block_excl(kr_load(chrom, end, perm, n, (uint64_t)blockIdx.x * KR_BLOCK + threadIdx.x), ws, total);
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// agg[0 .. n) -> the maximum of the blocks before each; ONE workgroup
__global__ __launch_bounds__(256) void kr_max_scan_kernel(KrMax *__restrict__ agg, uint64_t n) {
    __shared__ KrMax ws[4];
    KrMax carry{0, 0};
    for (uint64_t base = 0; base < n; base += 256) {
        const uint64_t i = base + threadIdx.x;
        KrMax total;
        const KrMax ex = kr_block_excl(i < n ? agg[i] : KrMax{0, 0}, ws, total);
        if (i < n) agg[i] = kr_max(carry, ex);
        carry = kr_max(carry, total);
    }
}

// flags[i] = sorted entry i opens a region; block_sums[b] = the flags of workgroup b
__global__ __launch_bounds__(256) void kr_flag_kernel(const int64_t *__restrict__ chrom, const int64_t *__restrict__ start,
                                                      const int64_t *__restrict__ end, const uint32_t *__restrict__ perm, uint64_t n,
                                                      uint64_t merge_distance, const KrMax *__restrict__ agg, uint8_t *__restrict__ flags,
                                                      unsigned long long *__restrict__ block_sums) {
    __shared__ KrMax ws[4];
    __shared__ uint32_t wc[17];
    const uint64_t i = (uint64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
    const KrMax v = kr_load(chrom, end, perm, n, i);
    KrMax total;
    const KrMax ex = kr_max(agg[blockIdx.x], kr_block_excl(v, ws, total));
    uint32_t f = 0, nf;
    if (v.c) f = ex.c != v.c || (unsigned long long)start[perm[i]] > ex.e + merge_distance;
    if (i < n) flags[i] = (uint8_t)f;
    kb_block_exscan(f, wc, &nf);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = nf;
}

// regions: cap rows of 4 words, words 2 and 3 of the first min(cap, regions) rows zeroed by the caller
__global__ __launch_bounds__(256) void kr_regions_kernel(const int64_t *__restrict__ chrom, const int64_t *__restrict__ start,
                                                         const int64_t *__restrict__ end, const uint32_t *__restrict__ perm,
                                                         const uint8_t *__restrict__ flags, uint64_t n,
                                                         const unsigned long long *__restrict__ block_off, int64_t *__restrict__ region_of,
                                                         unsigned long long *__restrict__ regions, uint64_t cap) {
    __shared__ uint32_t wc[17];
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * KR_BLOCK + threadIdx.x;
    const uint32_t f = i < n ? flags[i] : 0;
    uint32_t nf;
    const uint32_t before = kb_block_exscan(f, wc, &nf);
    long long g = -1;
    unsigned long long en = 0;
    if (i < n) {
        const uint32_t e = perm[i];
        const int64_t c = chrom[e];
        if (c >= 0) {
            g = (long long)(block_off[blockIdx.x] + before + f) - 1;      // (>= 0: the first entry of the order has its flag set)
            en = (unsigned long long)end[e];
            if (f && (uint64_t)g < cap) { regions[(uint64_t)g * 4] = (unsigned long long)c; regions[(uint64_t)g * 4 + 1] = (unsigned long long)start[e]; }
        }
        region_of[e] = g;
    }
    // neighbours in the same region: the maximum end of each run moves to its first lane
    const long long prev = __shfl_up(g, 1);
    const bool head = lane == 0 || prev != g;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_down(en, o);
        const long long gy = __shfl_down(g, o);
        if (lane + o < 64 && gy == g && y > en) en = y;
    }
    const unsigned long long heads = __ballot(head);
    if (head && g >= 0 && (uint64_t)g < cap) {
        atomicMax(&regions[(uint64_t)g * 4 + 2], en);
        atomicAdd(&regions[(uint64_t)g * 4 + 3], (unsigned long long)kdf_wave_run(heads, lane).len);
    }
}

// key[e] = group[e], or n_groups when entry e is ignored: group out of [0, n_groups), or a row of all-ones words
__global__ __launch_bounds__(256) void kr_group_key_kernel(const int64_t *__restrict__ group, const uint64_t *__restrict__ keys, int words,
                                                           uint64_t n, uint64_t n_groups, uint64_t *__restrict__ key) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int64_t g = group[e];
    bool ones = true;
    for (int j = 0; j < words; ++j) ones = ones && keys[e * words + j] == ~0ull;
    key[e] = (g < 0 || (uint64_t)g >= n_groups || ones) ? n_groups : (uint64_t)g;
}

// counts[g] += the heads among the sorted entries of group g; counts zeroed by the caller
__global__ __launch_bounds__(256) void kr_distinct_kernel(const uint64_t *__restrict__ gkey, const uint64_t *__restrict__ keys, int words,
                                                          const uint32_t *__restrict__ perm, uint64_t n, uint64_t n_groups,
                                                          unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const uint64_t e = in ? perm[i] : 0;
    const uint64_t g = in ? gkey[e] : n_groups;
    // the predecessor's words come from the neighbour lane; a wave's first lane reads them
    const bool fetch = in && lane == 0 && i > 0;
    const uint64_t ep = fetch ? perm[i - 1] : 0;
    uint64_t gp = __shfl_up(g, 1);
    if (fetch) gp = gkey[ep];
    bool differs = i == 0 || gp != g;
    for (int j = 0; j < words; ++j) {
        const uint64_t w = in ? keys[e * words + j] : 0;
        uint64_t wp = __shfl_up(w, 1);
        if (fetch) wp = keys[ep * words + j];
        differs = differs || wp != w;
    }
    const bool counted = in && g < n_groups && differs;
    // neighbours in the same group: the first lane of each run adds the run's heads
    const uint64_t gl = __shfl_up(g, 1);
    const bool head = lane == 0 || gl != g;
    const unsigned long long heads = __ballot(head), news = __ballot(counted);
    if (head && g < n_groups) {
        const unsigned long long c = (unsigned long long)__popcll(news & kdf_wave_run(heads, lane).mask);
        if (c) atomicAdd(&counts[g], c);
    }
}
