// kdf_long_merge.h -- long keys across ranks: the sender's dump grouped by owner rank, and set_counts for the
// count --if merge.  Templated on W like kdf_long.h; kdf_engine.hip instantiates W = 3 .. 7.
//
// Owner rule.  owner(key) = (((h >> 16) & 0xFFFF) * parts) >> 16 with h = kdf_long_hash<W>(words), the stored form in
// t.lo[slot]: bits 16..31 of the hash.  The home slot takes the TOP log2cap bits and the key_parts slice the LOW 16, so
// an owner's keys spread over the whole of any table of up to 2^32 slots, an owner table needs no hash_shift, and the
// rule does not depend on the active key slice.  (Above 2^32 slots -- more than a long table fits in 288 GB -- one or
// two owner bits would be home bits too: that costs probe locality, never correctness.)  A bucket holds keys of every
// owner, so the dump groups by each key's own owner, in two passes over the table:
//   1. kdf_long_parts_count_kernel: kept entries per owner (an LDS histogram per workgroup, one global atomic per
//      owner present);
//   host: byte offsets of the `parts` segments from the totals;
//   2. kdf_long_parts_write_kernel: a wave owns KDF_EXPORT_ROWS x 64 slots (as kdf_long_export_kernel), counts them per
//      owner in LDS, lane p reserves the wave's range in segment p with ONE returning atomic on that owner's cursor and
//      keeps the running position in a register; every row is then resolved in a wave-uniform loop -- the first pending
//      lane's owner, a ballot of the lanes that share it, positions by popcount -- and written once the loop is over, by
//      all kept lanes together.
// Segment p: [keys: n_p x W uint64 row-major | counts: n_p uint32], starts aligned to 8 bytes.  Scratch: O(parts) words.
#pragma once
#include "kdf_long.h"

#define KLM_MAX_PARTS 64                   // one lane of a wave per owner

__host__ __device__ __forceinline__ uint32_t kdf_long_owner(uint64_t h, uint32_t parts) {
    return (uint32_t)((((h >> 16) & 0xFFFFull) * parts) >> 16);
}

// is slot i part of the dump, and whose is it?  (top: the top-word array, the occupancy test of kdf_long_export_kernel)
__device__ __forceinline__ bool klm_keep(const KdfTable &t, const uint64_t *__restrict__ top, uint64_t i, uint64_t cap,
                                         uint32_t min_count, uint32_t parts, uint32_t &own, uint32_t &c) {
    own = 0; c = 0;
    if (i >= cap) return false;
    c = t.cnt[i];
    if (top[i] == KDF_EMPTY || c < min_count) return false;
    own = kdf_long_owner(t.lo[i], parts);
    return true;
}

// pass 1: part_cnt[p] += kept entries of owner p
__global__ __launch_bounds__(256) void kdf_long_parts_count_kernel(
    KdfTable t, const uint64_t *__restrict__ top, uint32_t min_count, uint32_t parts, unsigned long long *__restrict__ part_cnt)
{
    __shared__ uint32_t hist[KLM_MAX_PARTS];
    if (threadIdx.x < KLM_MAX_PARTS) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t cap = 1ull << t.log2cap;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t first = wave * (KDF_EXPORT_ROWS * 64);
    if (first < cap) {
        for (int r = 0; r < KDF_EXPORT_ROWS; ++r) {
            uint32_t own, c;
            if (klm_keep(t, top, first + (uint64_t)r * 64 + lane, cap, min_count, parts, own, c)) atomicAdd(&hist[own], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < parts && hist[threadIdx.x]) atomicAdd(&part_cnt[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

// pass 2: part_base[p] = byte offset of segment p in buf, part_cnt[p] = its entries (pass 1), cursor[p] = entries
// reserved so far (zeroed by the host).  An entry whose position is not below part_cnt[owner] is not written (the
// table cannot change between the passes; the test keeps every store inside the segment whatever happens).
template <int W>
__global__ __launch_bounds__(256) void kdf_long_parts_write_kernel(
    KdfTable t, uint32_t min_count, uint32_t parts, const unsigned long long *__restrict__ part_cnt,
    const unsigned long long *__restrict__ part_base, unsigned long long *__restrict__ cursor, unsigned char *__restrict__ buf)
{
    __shared__ uint32_t hist[4][KLM_MAX_PARTS];
    __shared__ unsigned long long seg_n[KLM_MAX_PARTS], seg_base[KLM_MAX_PARTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    hist[wv][lane] = 0;
    if (threadIdx.x < KLM_MAX_PARTS) {
        seg_n[threadIdx.x] = threadIdx.x < parts ? part_cnt[threadIdx.x] : 0ull;
        seg_base[threadIdx.x] = threadIdx.x < parts ? part_base[threadIdx.x] : 0ull;
    }
    __syncthreads();
    const uint64_t cap = 1ull << t.log2cap;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const uint64_t first = wave * (KDF_EXPORT_ROWS * 64);
    const bool live = first < cap;
    const uint64_t *top = t.hi + ((uint64_t)(W - 2) << t.log2cap);
    if (live) {
        for (int r = 0; r < KDF_EXPORT_ROWS; ++r) {
            uint32_t own, c;
            if (klm_keep(t, top, first + (uint64_t)r * 64 + lane, cap, min_count, parts, own, c)) atomicAdd(&hist[wv][own], 1u);
        }
    }
    __syncthreads();
    if (!live) return;
    // lane p: this wave's range in owner p's segment
    const uint32_t mine = (uint32_t)lane < parts ? hist[wv][lane] : 0u;
    unsigned long long pos_p = 0;
    if (mine) pos_p = atomicAdd(&cursor[lane], (unsigned long long)mine);
    if (!__any(mine != 0)) return;
    for (int r = 0; r < KDF_EXPORT_ROWS; ++r) {
        const uint64_t i = first + (uint64_t)r * 64 + lane;
        uint32_t own, c;
        const bool keep = klm_keep(t, top, i, cap, min_count, parts, own, c);
        unsigned long long pos = 0;
        unsigned long long pend = __ballot(keep);
        while (pend) {                                            // wave-uniform: one turn per owner present in the row
            const int leader = __ffsll((long long)pend) - 1;
            const uint32_t o = (uint32_t)__shfl((int)own, leader);
            const bool in = keep && own == o;
            const unsigned long long same = __ballot(in);
            const unsigned long long base = __shfl(pos_p, (int)o);        // lane o holds owner o's running position
            if ((uint32_t)lane == o) pos_p += (unsigned long long)__popcll(same);
            if (in) pos = base + (unsigned long long)__popcll(same & ((1ull << lane) - 1));
            pend &= ~same;
        }
        if (keep) {                                               // the rows leave with every kept lane of the wave active
            const unsigned long long n_o = seg_n[own], b_o = seg_base[own];
            if (pos < n_o) {
                uint64_t w[W];
                w[0] = 0;
#pragma unroll
                for (int j = 1; j < W; ++j) w[j] = *kdf_long_word<W>(t, j, i);
                w[0] = kdf_unmix64(t.lo[i]) ^ kdf_long_fold<W>(w);        // w0 back from the stored form
                uint64_t *okeys = (uint64_t *)(buf + b_o);
                uint32_t *ocnt = (uint32_t *)(buf + b_o + n_o * (8ull * W));
#pragma unroll
                for (int j = 0; j < W; ++j) okeys[pos * W + j] = w[j];
                ocnt[pos] = c;
            }
        }
    }
}

// thread per key: the count of a STORED key becomes counts[i] (kdf_set_counts_kernel for W-word rows).  A key that is
// not stored -- or whose top word has a bit at or above tb = 2k - 64 (W - 1): no k-mer -- raises error bit 2.
template <int W>
__global__ __launch_bounds__(256) void kdf_long_set_counts_kernel(
    const uint64_t *__restrict__ keys, const uint32_t *__restrict__ counts, uint64_t n, KdfTable t, KdfCtl *ctl, int tb)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t w[W];
    kdf_long_read_key<W>(keys, keys + 1, W, 1, i, w);
    const uint64_t s = (w[W - 1] >> tb) ? ~0ull : kdf_find_long<W>(t, kdf_long_hash<W>(w), w);
    if (s == ~0ull) atomicOr(&ctl->error, 2u);
    else t.cnt[s] = counts[i];
}
