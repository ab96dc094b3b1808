// kdf_spool.h -- the read spool's kernels (kdf.h "read spool"; the host side is in kdf_spool.hip).
//
// A spool keeps the batches of a read stream resident, packed as they arrive (3 bits per position), as a list of SEGMENTS.
// A segment is one read stream in the layout of kdf.h "Read streams"; a batch of n_bases positions occupies
// n_bases / 64 + 1 tiles of it (a tile = 64 positions = one mask word + two packed words), so that at least one invalid
// position -- for a batch that fills its last tile, a whole all-invalid tile -- lies between two batches and no window runs
// from one into the next (the rule of l1_append, kdf_engine.hip).
#ifndef KDF_SPOOL_H
#define KDF_SPOOL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kdf_device.h"
#include "kdf_scan.h"            // kb_block_exscan: the block scan of the ks_select_* kernels (their scan of the block sums,
                                 // kh_scan_kernel of kdf_hits.h, belongs to kdf_engine_reads.hip: the spool runs it through kh_scan_launch)

#define KS_THREADS 256
#define KS_MAX_BLOCKS 2048u      // a streaming copy: 8 workgroups per CU fill the device, the rest is a grid stride

// ks_append_kernel: normalise one batch into its place in a segment.  dp / dm point at the batch's first tile in the
// segment (16-byte aligned: a tile is 16 bytes of packed words and the segment buffers come from hipMalloc).  Item i is
// tile i of the batch: ONE mask word and its TWO packed words, one 16-byte store and one 8-byte store per lane, lanes on
// consecutive tiles.
//   i < ceil(n_bases / 64)   the source's words; in the tile that holds position n_bases the mask bits at and past it are
//                            set and the bases there zeroed, in registers
//   i < n_tiles              (n_bases a multiple of 64: the padding tile) all invalid, bases 0 -- nothing is loaded
//   i < n_tiles + 2          the 2 mask / 4 packed padding words of kdf_stream_words behind the segment's last batch;
//                            the next batch, if one comes, overwrites them (appends are ordered by the spool's event)
// Source loads: mask words 0 .. ceil(n_bases / 64) - 1 and packed words 0 .. 2 ceil(n_bases / 64) - 1 only, which
// kdf_stream_words(n_bases) covers.  src16: the packed source is 16-byte aligned (one 16-byte load per lane; two 8-byte
// loads otherwise).  The room behind dp / dm is the host's to check (spool_place).
__global__ __launch_bounds__(KS_THREADS) void ks_append_kernel(uint64_t *__restrict__ dp, uint64_t *__restrict__ dm,
                                                               const uint64_t *__restrict__ sp, const uint64_t *__restrict__ sm,
                                                               uint64_t n_bases, uint64_t n_tiles, int src16) {
    const uint64_t src_tiles = (n_bases + 63) >> 6;
    const uint64_t cut = n_bases >> 6;                 // the tile that holds position n_bases
    const uint32_t r = (uint32_t)(n_bases & 63);
    const uint64_t stride = (uint64_t)gridDim.x * KS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x; i < n_tiles + 2; i += stride) {
        uint64_t m = ~0ull, p0 = 0ull, p1 = 0ull;
        if (i < src_tiles) {
            m = sm[i];
            if (src16) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(sp + 2 * i);
                p0 = v.x; p1 = v.y;
            } else {
                p0 = sp[2 * i]; p1 = sp[2 * i + 1];
            }
            if (i == cut) {                             // (r != 0 here: cut < src_tiles)
                m |= ~0ull << r;
                if (r < 32) { p0 &= (1ull << (2 * r)) - 1; p1 = 0ull; }
                else if (r > 32) p1 &= (1ull << (2 * (r - 32))) - 1;
                else p1 = 0ull;
            }
        }
        ulonglong2 o; o.x = p0; o.y = p1;
        *reinterpret_cast<ulonglong2 *>(dp + 2 * i) = o;
        dm[i] = m;
    }
}

// ks_offsets_kernel: rebase one batch's read offsets into SEGMENT coordinates.  dst points at the batch's first entry in
// the segment's offsets array (the entry the batch before it wrote last, which this batch owns now), src at the batch's
// n = n_reads + 1 offsets, base = 64 x the batch's first tile.  One 8-byte load and one 8-byte store per lane; entries
// dst[0 .. n) are written and nothing else, whatever src holds.
__global__ __launch_bounds__(KS_THREADS) void ks_offsets_kernel(int64_t *__restrict__ dst, const int64_t *__restrict__ src,
                                                                uint64_t n, int64_t base) {
    const uint64_t stride = (uint64_t)gridDim.x * KS_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * KS_THREADS + threadIdx.x; i < n; i += stride) dst[i] = src[i] + base;
}

// ks_select_*: the reads whose `distinct` (the second uint32 of a kdf_read_hits row) is at least min_distinct, as the
// ASCENDING list of their indices -- an order-preserving compaction in the shape of kh_count / kh_scan / kh_write:
//   1. ks_select_count_kernel   KS_SELECT_ROWS rows per workgroup, 4 consecutive rows per thread -> block sums
//   2. kh_scan_kernel           exclusive scan of the block sums, the total behind them
//   3. ks_select_write_kernel   the same rows again, a workgroup scan of the per-thread counts, every thread writes the
//                               indices of its rows: entry e < cap only
// A row is one 8-byte word (hits in the low half, distinct in the high half); rows16: the rows are 16-byte aligned, so a
// thread's 4 rows (row index a multiple of 4) are two 16-byte loads.  Rows at and past n_rows are not loaded.
#define KS_SELECT_ROWS 1024

__device__ __forceinline__ uint32_t ks_select_mask(const uint64_t *__restrict__ rows, uint64_t r0, uint64_t n_rows, uint32_t min_distinct,
                                                   int rows16) {
    uint64_t x[4] = {0, 0, 0, 0};
    if (r0 + 4 <= n_rows && rows16) {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(rows + r0), b = *reinterpret_cast<const ulonglong2 *>(rows + r0 + 2);
        x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (r0 + j < n_rows) x[j] = rows[r0 + j];
    }
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (r0 + j < n_rows && (uint32_t)(x[j] >> 32) >= min_distinct) m |= 1u << j;
    return m;
}

__global__ __launch_bounds__(256) void ks_select_count_kernel(const uint64_t *__restrict__ rows, uint64_t n_rows, uint32_t min_distinct,
                                                              int rows16, unsigned long long *__restrict__ block_sums) {
    __shared__ uint32_t ws[17];
    const uint64_t r0 = (uint64_t)blockIdx.x * KS_SELECT_ROWS + threadIdx.x * 4;
    uint32_t total;
    kb_block_exscan((uint32_t)__popc(ks_select_mask(rows, r0, n_rows, min_distinct, rows16)), ws, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void ks_select_write_kernel(const uint64_t *__restrict__ rows, uint64_t n_rows, uint32_t min_distinct,
                                                              int rows16, const unsigned long long *__restrict__ block_off,
                                                              uint64_t *__restrict__ out, uint64_t cap) {
    __shared__ uint32_t ws[17];
    const uint64_t r0 = (uint64_t)blockIdx.x * KS_SELECT_ROWS + threadIdx.x * 4;
    const uint32_t m = ks_select_mask(rows, r0, n_rows, min_distinct, rows16);
    uint32_t total;
    uint64_t o = block_off[blockIdx.x] + kb_block_exscan((uint32_t)__popc(m), ws, &total);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (m >> j & 1) { if (o < cap) out[o] = r0 + j; ++o; }
}

#endif /* KDF_SPOOL_H */
