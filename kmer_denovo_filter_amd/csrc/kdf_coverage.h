// kdf_coverage.h -- the hits of the Module-3 scan in reference coordinates (kdf_hit_coverage*, kdf_coverage_list*,
// kdf_hit_keys*): from a hit mask, the read offsets and the reads' CIGARs to the two per-position sums Module 3 writes
// out (hit k-mers covering a reference base, reads that brought one), to their ascending list, and to the canonical
// keys of listed hits.  The kernels only READ the stream, the mask and the alignment arrays; the table is not touched.
//
// As in kdf_hits.h the mask is compacted first (kh_count / kh_scan / kh_write over the first n_bases - k + 1 bits: a
// bit past that is no hit) and the work runs LANE PER HIT:
//   1. kc_prefix_kernel  thread per read that is not skipped and holds a hit: one walk over its CIGAR writes, for every
//                        operation, the query and reference bases consumed BEFORE it (2 x uint64 per operation), so
//                        that the operation holding a query index is found by binary search.
//   2. kc_accum_kernel   lane per hit.  In the ascending list the hits of a read are neighbours.  The largest hit <= q
//                        of the read OWNS stream position q, so hit i owns [p, min(p + k, next hit of the read, end of
//                        the read)): every covered position has exactly one owner and is added ONCE per read -- a run
//                        of k hits (a SNV) costs about 2k atomics per array, not k^2.  depth(q) = entries of the same
//                        read in (q - k, q]: the owner steps back at most k - 1 entries once and moves that edge forward
//                        as q grows.  The operation of q's query index: one binary search for p, then forward with q.
//                        Per owned aligned position one atomicAdd to kmer_cov (the depth) and one to read_cov (1); the
//                        results are not used, so they are plain vector atomics without return.
//   Work: hits x k steps plus the operations of the reads that hold hits.  Integer sums: the result does not depend on
//   the order the adds arrive in.
// Bounds, whatever the offsets hold: a read comes from kh_read_of (-1 or in [0, n_reads)), operation indices are
// clamped to [0, n_cigar), and an add is issued only for g = ref_start + d < span.
//   3. kc_list_*         order-preserving compaction of the positions with read_cov >= a threshold: count per block of
//                        KC_BLOCK_ELEMS positions, kh_scan_kernel over the block sums, write.
//   4. kc_keys_kernel    thread per listed position: kd_window_key, W words per row.
#pragma once
#include "kdf_hits.h"

#define KC_BLOCK_ELEMS 1024               // positions per workgroup of the list kernels: 4 consecutive per thread

__device__ __forceinline__ int64_t kc_clamp(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }
// M, = and X pair a query base with a reference base
__device__ __forceinline__ bool kc_aligned(uint32_t op) { return op == 0 || op == 7 || op == 8; }

// pre[2 i], pre[2 i + 1] = query / reference bases consumed by the operations of the read before operation i
__global__ __launch_bounds__(256) void kc_prefix_kernel(
    const uint64_t *__restrict__ pos, uint64_t n_hits, const int64_t *__restrict__ offs, int64_t n_reads,
    const int64_t *__restrict__ ref_start, const uint32_t *__restrict__ cigar, uint64_t n_cigar,
    const int64_t *__restrict__ cig_offs, unsigned long long *__restrict__ pre)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_reads || ref_start[r] < 0) return;
    const int64_t b = offs[r], e = offs[r + 1];
    if (e <= b || e <= 0) return;
    const uint64_t first = kh_lower_bound(pos, n_hits, b < 0 ? 0ull : (uint64_t)b);
    if (first >= n_hits || pos[first] >= (uint64_t)e) return;        // no hit in the read: nobody asks for its prefix
    const int64_t cb = kc_clamp(cig_offs[r], 0, (int64_t)n_cigar), ce = kc_clamp(cig_offs[r + 1], cb, (int64_t)n_cigar);
    unsigned long long qc = 0, rc = 0;
    for (int64_t i = cb; i < ce; ++i) {
        pre[2 * i] = qc;
        pre[2 * i + 1] = rc;
        const uint32_t w = cigar[i], op = w & 15u;
        const unsigned long long len = w >> 4;
        if (kc_aligned(op)) { qc += len; rc += len; }
        else if (op == 1 || op == 4) qc += len;
        else if (op == 2 || op == 3) rc += len;
    }
}

__global__ __launch_bounds__(256) void kc_accum_kernel(
    const uint64_t *__restrict__ pos, uint64_t n_hits, int k, const int64_t *__restrict__ offs, int64_t n_reads,
    const int64_t *__restrict__ ref_start, const uint32_t *__restrict__ cigar, uint64_t n_cigar,
    const int64_t *__restrict__ cig_offs, const unsigned long long *__restrict__ pre,
    uint32_t *__restrict__ kmer_cov, uint32_t *__restrict__ read_cov, uint64_t span)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_hits) return;
    const uint64_t p = pos[i];
    const int64_t r = kh_read_of(offs, n_reads, (int64_t)p);
    if (r < 0) return;
    const int64_t rs = ref_start[r];
    if (rs < 0) return;
    const int64_t cb = kc_clamp(cig_offs[r], 0, (int64_t)n_cigar), ce = kc_clamp(cig_offs[r + 1], cb, (int64_t)n_cigar);
    if (ce == cb) return;                                             // an empty CIGAR aligns nothing
    const uint64_t b = (uint64_t)offs[r];                             // 0 <= b <= p < offs[r + 1] (kh_read_of)
    uint64_t end = (uint64_t)offs[r + 1];
    if (p + (uint64_t)k < end) end = p + (uint64_t)k;
    if (i + 1 < n_hits && pos[i + 1] < end) end = pos[i + 1];         // (behind p and before the read's end: the same read)
    uint64_t j = i;                                                   // the first entry of the read in (p - k, p]
    while (j > 0 && pos[j - 1] + (uint64_t)k > p && pos[j - 1] >= b) --j;
    // the last operation whose query prefix is <= the query index: the only one that can hold it
    int64_t lo = cb, hi = ce - 1;
    while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (pre[2 * mid] <= p - b) lo = mid; else hi = mid - 1; }
    int64_t op = lo;
    for (uint64_t q = p; q < end; ++q) {
        while (pos[j] + (uint64_t)k <= q) ++j;                        // (stops at i at the latest: pos[i] = p > q - k)
        const uint64_t c = q - b;
        while (op + 1 < ce && pre[2 * (op + 1)] <= c) ++op;
        const uint32_t w = cigar[op];
        const uint64_t qp = pre[2 * op];
        if (!kc_aligned(w & 15u) || c < qp || c - qp >= (uint64_t)(w >> 4)) continue;
        const uint64_t d = pre[2 * op + 1] + (c - qp);
        if (d >= span || (uint64_t)rs >= span - d) continue;          // g = rs + d >= span: dropped, never wrapped
        const uint64_t g = (uint64_t)rs + d;
        atomicAdd(&kmer_cov[g], (uint32_t)(i - j + 1));
        atomicAdd(&read_cov[g], 1u);
    }
}

// block_sums[block] = positions g of the block's KC_BLOCK_ELEMS with rc[g] >= thr; rc: the n words of the window
__global__ __launch_bounds__(256) void kc_list_count_kernel(const uint32_t *__restrict__ rc, uint64_t n, uint32_t thr,
                                                            unsigned long long *__restrict__ block_sums) {
    __shared__ uint32_t ws[17];
    const uint64_t g0 = (uint64_t)blockIdx.x * KC_BLOCK_ELEMS + threadIdx.x * 4;
    uint32_t c = 0, total;
#pragma unroll
    for (int j = 0; j < 4; ++j) c += g0 + j < n && rc[g0 + j] >= thr;
    kb_block_exscan(c, ws, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// entry e < cap of the list: pos_out[e] = first + g, kmer_out[e] = kc[g], read_out[e] = rc[g] (either may be NULL)
__global__ __launch_bounds__(256) void kc_list_write_kernel(
    const uint32_t *__restrict__ kc, const uint32_t *__restrict__ rc, uint64_t first, uint64_t n, uint32_t thr,
    const unsigned long long *__restrict__ block_off, uint64_t *__restrict__ pos_out, uint32_t *__restrict__ kmer_out,
    uint32_t *__restrict__ read_out, uint64_t cap)
{
    __shared__ uint32_t ws[17];
    const uint64_t g0 = (uint64_t)blockIdx.x * KC_BLOCK_ELEMS + threadIdx.x * 4;
    uint32_t v[4], c = 0, total;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = g0 + j < n ? rc[g0 + j] : 0u; c += g0 + j < n && v[j] >= thr; }
    uint64_t o = block_off[blockIdx.x] + kb_block_exscan(c, ws, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (g0 + j >= n || v[j] < thr) continue;
        if (o < cap) {
            pos_out[o] = first + g0 + j;
            if (kmer_out) kmer_out[o] = kc[g0 + j];
            if (read_out) read_out[o] = v[j];
        }
        ++o;
    }
}

// keys_out[e * W ..] = canonical key of the window at positions[e], all ones when the window ends past n_bases
template <int W>
__global__ __launch_bounds__(256) void kc_keys_kernel(const uint64_t *__restrict__ packed, uint64_t n_bases, int k,
                                                      const uint64_t *__restrict__ positions, uint64_t n, uint64_t *__restrict__ keys_out) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const uint64_t p = positions[e];
    uint64_t key[W];
    if (p > n_bases || p + (uint64_t)k > n_bases) {
#pragma unroll
        for (int j = 0; j < W; ++j) key[j] = ~0ull;
    } else {
        kd_window_key<W>(packed, kdf_stream_geom(n_bases).packed_words, p, k, key);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) keys_out[e * W + j] = key[j];
}
