// kdf_hits.h -- the per-read reduction of the Module-3 scan on the device (kdf_read_hits*, kdf_hit_list*): from the hit
// mask kdf_scan_reads_dev writes to `hits` and `distinct` per read and to the ascending list of hit positions.  The
// kernels only READ the table and the stream.
//
// Hits are sparse in the real workload (a few thousand informative reads out of hundreds of millions), so the mask is
// compacted first and everything after that runs LANE PER HIT, not lane per window:
//   1. kh_count_kernel   popcount of KH_BLOCK_WORDS mask words per workgroup -> block sums
//   2. kh_scan_kernel    exclusive scan of the block sums (one workgroup), the total behind them
//   3. kh_write_kernel   the same words again, a workgroup scan of the per-thread popcounts, then every thread writes
//                        the positions of its 4 words: the list is in ASCENDING position order whatever the scheduling
//   4. kh_hits_kernel    thread per read: hits[r] = lower_bound(list, offsets[r + 1]) - lower_bound(list, offsets[r]).
//                        No atomics, so a contig-length read costs what a 150-base read costs.
//   5. kh_distinct_kernel  lane per hit: the read that holds the position (binary search of the offsets), the window's
//                        canonical key (kd_window_key, as the count profile cuts it), its table slot (kdf_find_*).  A
//                        stored key and its slot are one-to-one, so the distinct keys of read r are the distinct pairs
//                        (r, slot): the pair, r << log2cap | slot, goes into an open-addressing set in HBM with one
//                        64-bit atomicCAS per probe, and a lane whose pair was new counts 1 for its read.  The set has
//                        at least 2 slots per hit (load <= 0.5), is owned by the engine and kept between calls.  Lanes
//                        of a wave that sit in the same read (the list is sorted, so they are neighbours) are summed on
//                        ballots and send ONE atomic add: a read of any length gets at most one add per wave of hits.
// Exact for any read length (no per-read state anywhere), work linear in the hits, and the result is a set size: it
// does not depend on which lane wins a CAS.  No lane waits for another inside the probe loop.
#pragma once
#include "kdf_depth.h"
#include "kdf_scan.h"

#define KH_BLOCK_WORDS 1024               // mask words per workgroup: 4 consecutive words per thread
// (KH_ROW_WORDS = 2 -- hits, distinct (uint32): kdf_device.h, shared with kdf_spool.h; the block scan kb_block_exscan: kdf_scan.h)

// mask word w with the bits at and past n_bases cleared; n_words = ceil(n_bases / 64)
__device__ __forceinline__ uint64_t kh_word(const uint64_t *__restrict__ bits, uint64_t w, uint64_t n_words, uint64_t n_bases) {
    if (w >= n_words) return 0;
    const uint64_t rem = n_bases - w * 64;                            // >= 1
    return rem < 64 ? bits[w] & ((1ull << rem) - 1) : bits[w];
}

// the read that holds position p: r with offs[r] <= p < offs[r + 1], or -1.  Whatever the offsets hold, the result is
// -1 or in [0, n_reads) and only offs[0 .. n_reads] are read.
__device__ __forceinline__ int64_t kh_read_of(const int64_t *__restrict__ offs, int64_t n_reads, int64_t p) {
    if (n_reads <= 0 || p < 0 || offs[0] > p) return -1;
    int64_t lo = 0, hi = n_reads - 1;                                 // the last r with offs[r] <= p (empty reads before it are skipped)
    while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (offs[mid] <= p) lo = mid; else hi = mid - 1; }
    return p < offs[lo + 1] ? lo : -1;
}

__global__ __launch_bounds__(256) void kh_count_kernel(const uint64_t *__restrict__ bits, uint64_t n_bases,
                                                       unsigned long long *__restrict__ block_sums) {
    __shared__ uint32_t ws[17];
    const uint64_t n_words = (n_bases + 63) / 64;
    const uint64_t w0 = (uint64_t)blockIdx.x * KH_BLOCK_WORDS + threadIdx.x * 4;
    uint32_t c = 0, total;
#pragma unroll
    for (int j = 0; j < 4; ++j) c += (uint32_t)__popcll(kh_word(bits, w0 + j, n_words, n_bases));
    kb_block_exscan(c, ws, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// sums[0 .. n) -> their exclusive prefix sums, sums[n] = the total; ONE workgroup
__global__ __launch_bounds__(256) void kh_scan_kernel(unsigned long long *__restrict__ sums, uint64_t n) {
    __shared__ unsigned long long ws[4];
    const unsigned long long total = kb_sums_exscan(sums, n, ws);
    if (threadIdx.x == 0) sums[n] = total;
}

// entry e of the list, e < cap: pos_out[e] = position of the e-th set bit, reads_out[e] (may be NULL) = its read or -1
__global__ __launch_bounds__(256) void kh_write_kernel(
    const uint64_t *__restrict__ bits, uint64_t n_bases, const unsigned long long *__restrict__ block_off,
    uint64_t *__restrict__ pos_out, int64_t *__restrict__ reads_out, const int64_t *__restrict__ offs, int64_t n_reads, uint64_t cap)
{
    __shared__ uint32_t ws[17];
    const uint64_t n_words = (n_bases + 63) / 64;
    const uint64_t w0 = (uint64_t)blockIdx.x * KH_BLOCK_WORDS + threadIdx.x * 4;
    uint64_t x[4];
    uint32_t c = 0, total;
#pragma unroll
    for (int j = 0; j < 4; ++j) { x[j] = kh_word(bits, w0 + j, n_words, n_bases); c += (uint32_t)__popcll(x[j]); }
    uint64_t o = block_off[blockIdx.x] + kb_block_exscan(c, ws, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint64_t y = x[j];
        while (y) {
            const uint64_t p = (w0 + j) * 64 + (uint64_t)__builtin_ctzll(y);
            y &= y - 1;
            if (o < cap) {
                pos_out[o] = p;
                if (reads_out) reads_out[o] = kh_read_of(offs, n_reads, (int64_t)p);
            }
            ++o;
        }
    }
}

// first i in [0, n) with pos[i] >= x, n when there is none
__device__ __forceinline__ uint64_t kh_lower_bound(const uint64_t *__restrict__ pos, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (pos[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// rows[r * 2] = entries of the list in [offs[r], offs[r + 1]); thread per read
__global__ __launch_bounds__(256) void kh_hits_kernel(const uint64_t *__restrict__ pos, uint64_t n_hits, const int64_t *__restrict__ offs,
                                                      int64_t n_reads, uint32_t *__restrict__ rows) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_reads) return;
    const int64_t b = offs[r], e = offs[r + 1];
    uint64_t n = 0;
    if (e > b && e > 0) n = kh_lower_bound(pos, n_hits, (uint64_t)e) - kh_lower_bound(pos, n_hits, b < 0 ? 0ull : (uint64_t)b);
    rows[(uint64_t)r * KH_ROW_WORDS] = (uint32_t)n;
}

template <int W>
__device__ __forceinline__ uint64_t kh_find(const KdfTable &t, uint64_t h, const uint64_t (&key)[W]) {
    if constexpr (W == 1) return kdf_find_narrow(t, h);
    else if constexpr (W == 2) return kdf_find_wide(t, h, key[1]);
    else return kdf_find_long<W>(t, h, key);
}

// rows[r * 2 + 1] += the pairs (r, slot) of the listed hits that were not in `set` yet; set: 2^log2set words of
// KDF_EMPTY, 2^log2set >= 2 n_hits.  The host checked that r << log2cap | slot stays below 2^63 (so no pair is KDF_EMPTY).
template <int W>
__global__ __launch_bounds__(256) void kh_distinct_kernel(
    const uint64_t *__restrict__ packed, uint64_t n_bases, int k, KdfTable t, const uint64_t *__restrict__ pos, uint64_t n_hits,
    const int64_t *__restrict__ offs, int64_t n_reads, unsigned long long *__restrict__ set, uint32_t log2set, uint32_t *__restrict__ rows)
{
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t pw = kdf_stream_geom(n_bases).packed_words;
    long long r = -1;
    bool isnew = false;
    if (i < n_hits) {
        const uint64_t p = pos[i];
        if (p + (uint64_t)k <= n_bases) r = kh_read_of(offs, n_reads, (int64_t)p);
        if (r >= 0) {
            uint64_t key[W];
            kd_window_key<W>(packed, pw, p, k, key);
            const uint64_t slot = kh_find<W>(t, kd_hash<W>(key), key);
            if (slot != ~0ull) {
                const unsigned long long pair = ((unsigned long long)r << t.log2cap) | slot;
                const uint64_t smask = (1ull << log2set) - 1;
                uint64_t j = kdf_mix64(pair) >> (64 - log2set);
                for (uint64_t n = 0; n <= smask; ++n) {              // (ends at an empty word: the set is at most half full)
                    const unsigned long long old = atomicCAS(&set[j], (unsigned long long)KDF_EMPTY, pair);
                    if (old == KDF_EMPTY) { isnew = true; break; }
                    if (old == pair) break;
                    j = (j + 1) & smask;
                }
            }
        }
    }
    // neighbours in the same read: the first lane of each run adds the run's new pairs
    const long long prev = __shfl_up(r, 1);
    const bool head = lane == 0 || prev != r;
    const unsigned long long heads = __ballot(head), news = __ballot(isnew);
    if (head && r >= 0) {
        const uint32_t c = (uint32_t)__popcll(news & kdf_wave_run(heads, lane).mask);
        if (c) atomicAdd(&rows[(uint64_t)r * KH_ROW_WORDS + 1], c);
    }
}
