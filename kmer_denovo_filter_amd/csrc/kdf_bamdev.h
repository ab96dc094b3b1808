// kdf_bamdev.h -- the device half of the device BAM feeder (include/kdf.h "device BAM feeder"): the
// kernels that turn a planned batch of COMPRESSED BGZF blocks (kdf_bamraw_next, kdf_host.cpp) into the engine's packed
// read stream in HBM.
//
//   a. inflate  kdf_bd_inflate_kernel   one WAVE per BGZF block (blocks are independent and <= 64 KB); the decoder is
//                                       kdf_inflate.h with a wavefront as its lane group, its tables in LDS
//                                       (KDF_BD_WAVES x sizeof(KdfInfTables) = 4 x 3.7 KB per workgroup)
//   b. walk     kdf_bd_walk_kernel      one THREAD per sub-range: bam_next_raw + bam_pump + flush_run of kdf_host.cpp,
//                                       sequence only.  Runs twice: COUNT (reads, stream positions, status per
//                                       sub-range), then, after the scan, WRITE (each read's stream offset and where
//                                       its 4-bit sequence lies in the inflated span)
//   c. scan     kdf_bd_scan_kernel      per-sub-range counts -> bases of the sub-ranges in the stream, up to the first
//                                       sub-range that is not done; the totals the host reads back
//   d. pack     kdf_bd_pack_kernel      one thread per 64 stream positions = one mask word and two packed words, which
//                                       no other thread writes: 4-bit BAM bases -> 2-bit codes + invalid bits, one
//                                       invalid separator behind every read, everything at and past n_bases invalid / 0
//
// Bounds hold by construction: the inflate kernel checks every table entry against the output buffer before it reads a
// byte; the walker reads record bytes only after it has checked that the whole record lies inside the inflated span,
// and advances >= 36 bytes per record; the writers index by counts the host has checked against the caller's capacities.
#pragma once
#include "kdf.h"
#include "kdf_inflate.h"

#define KDF_BD_WAVES 4                       // BGZF blocks (waves) per workgroup of the inflate kernel
#define KDF_BGZF_MAX_ISIZE 65536u            // the format's limit on a block's inflated size

struct KdfLaneWave {                         // kdf_inflate.h's lane group on the device: one wavefront
    unsigned lane;
    __device__ __forceinline__ unsigned id() const { return lane; }
    __device__ __forceinline__ unsigned count() const { return 64; }
    // the lanes of a wave run in lockstep and its memory operations are performed in order: only the compiler needs telling
    __device__ __forceinline__ void sync() const { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); }
};

__global__ __launch_bounds__(64 * KDF_BD_WAVES) void kdf_bd_inflate_kernel(
    const uint8_t *__restrict__ comp, const kdf_bgzf_block *__restrict__ blocks, uint64_t n_blocks, uint8_t *out, uint64_t out_cap,
    uint32_t *__restrict__ status)
{
    __shared__ KdfInfTables tables[KDF_BD_WAVES];
    const unsigned wave = threadIdx.x >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * KDF_BD_WAVES + wave;
    if (b >= n_blocks) return;                                           // (wave-uniform)
    const kdf_bgzf_block blk = blocks[b];
    int st;
    if (blk.isize > KDF_BGZF_MAX_ISIZE || blk.out_off > out_cap || blk.isize > out_cap - blk.out_off) st = KDF_INF_BOUNDS;
    else st = kdf_inflate_block(KdfLaneWave{threadIdx.x & 63u}, comp + blk.comp_off, blk.comp_len, out + blk.out_off, blk.isize, tables[wave]);
    if ((threadIdx.x & 63u) == 0) status[b] = (uint32_t)st;
}

// ---- walk ---------------------------------------------------------------------------------------------------------------
struct KdfBdSubCount { uint64_t reads, bases; };                      // per sub-range: records emitted, stream positions (bases + separators)

__device__ __forceinline__ int32_t kdf_bd_le32(const uint8_t *p) { return (int32_t)(p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24)); }

template <bool WRITE>
__global__ __launch_bounds__(64) void kdf_bd_walk_kernel(
    const uint8_t *__restrict__ buf, const kdf_bgzf_block *__restrict__ blocks, uint64_t n_blocks, uint64_t buf_cap,
    const kdf_bam_subrange *__restrict__ subs, uint64_t n_sub, uint32_t flag_off, int collapse,
    KdfBdSubCount *__restrict__ counts, uint32_t *__restrict__ sub_status,           // COUNT: out
    const KdfBdSubCount *__restrict__ bases, int64_t *__restrict__ offsets, uint64_t *__restrict__ src, uint64_t cap_reads)   // WRITE
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_sub) return;
    uint64_t span = n_blocks ? blocks[n_blocks - 1].out_off + blocks[n_blocks - 1].isize : 0;   // inflated bytes of the batch
    if (span > buf_cap) span = buf_cap;
    const kdf_bam_subrange sr = subs[j];
    const bool at_eof = sr.flags & KDF_SUB_AT_EOF;
    uint64_t reads = 0, nb = 0;
    const uint64_t rbase = WRITE ? bases[j].reads : 0, pbase = WRITE ? bases[j].bases : 0;
    uint32_t status = KDF_SUB_DONE;
    // the best record per read part of the open QNAME run (0 other, 1 READ1, 2 READ2): where its sequence lies, its length
    uint64_t best_sq[3] = {0, 0, 0}; int32_t best_len[3] = {0, 0, 0}; int score[3] = {-1, -1, -1};
    uint64_t run_name = 0; uint32_t run_len = 0; bool have_run = false;
    auto emit = [&](uint64_t sq, int32_t l_seq) {
        if (WRITE && rbase + reads < cap_reads) { offsets[rbase + reads] = (int64_t)(pbase + nb); src[rbase + reads] = sq; }
        ++reads; nb += (uint64_t)l_seq + 1;
    };
    auto flush = [&]() {
#pragma unroll
        for (int i = 0; i < 3; ++i) if (score[i] >= 0) { emit(best_sq[i], best_len[i]); score[i] = -1; }
        have_run = false;
    };
    uint64_t q = sr.start;
    if (q != KDF_SUB_NONE) {
        for (;;) {
            // (every turn advances q by 4 + block_size >= 36 bytes, or leaves)
            if (q > span || span - q < 4) { if (!at_eof) status = KDF_SUB_UNFINISHED; else if (have_run) flush(); break; }
            const int32_t bs = kdf_bd_le32(buf + q);
            if (bs < 32) { status = KDF_SUB_CORRUPT; break; }
            if (span - q - 4 < (uint64_t)bs) { status = at_eof ? KDF_SUB_CORRUPT : KDF_SUB_UNFINISHED; break; }
            const uint8_t *p = buf + q + 4;
            const uint32_t l_rn = p[8], n_cig = p[12] | (p[13] << 8), flag = p[14] | (p[15] << 8);
            const int32_t l_seq = kdf_bd_le32(p + 16);
            if (l_seq < 0) { status = KDF_SUB_CORRUPT; break; }
            const uint64_t need = 32 + (uint64_t)l_rn + 4 * (uint64_t)n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
            if (need > (uint64_t)bs) { status = KDF_SUB_CORRUPT; break; }
            const bool zone = sr.stop != KDF_SUB_NONE && q >= sr.stop;   // past the sub-range's end: only the run that straddles it is finished
            const uint64_t at = q;
            q += 4 + (uint64_t)bs;
            if (zone && !collapse) break;
            if (flag & flag_off) continue;
            const uint64_t sq = at + 4 + 32 + l_rn + 4 * (uint64_t)n_cig;
            if (!collapse) { emit(sq, l_seq); continue; }
            const uint32_t nl = l_rn ? l_rn - 1 : 0;
            bool same = have_run && nl == run_len;
            for (uint32_t i = 0; same && i < nl; ++i) same = buf[run_name + i] == p[32 + i];
            if (!same) {
                if (have_run) flush();
                if (zone) break;                                          // the next sub-range's first run
                run_name = at + 4 + 32; run_len = nl; have_run = true;
            }
            const bool r1 = flag & 0x40, r2 = flag & 0x80;
            const int part = (r1 && !r2) ? 1 : (r2 && !r1) ? 2 : 0;
            const int sc = (l_seq > 0 && buf[sq + ((uint64_t)l_seq + 1) / 2] != 0xFF) ? 2 : 1;
#pragma unroll
            for (int i = 0; i < 3; ++i) if (i == part && sc > score[i]) { best_sq[i] = sq; best_len[i] = l_seq; score[i] = sc; }
        }
    }
    if (!WRITE) { counts[j] = KdfBdSubCount{reads, nb}; sub_status[j] = status; }
}

// ---- scan -----------------------------------------------------------------------------------------------------------------
// One thread (launched as <<<1, 1>>>): a batch has as many sub-ranges as it has MiB of file, a few hundred.  totals: 0 reads, 1 stream positions of
// the sub-ranges before the first that is not done, 2 that sub-range's index (n_sub: all done).
__global__ void kdf_bd_scan_kernel(const KdfBdSubCount *__restrict__ counts, const uint32_t *__restrict__ sub_status, uint64_t n_sub,
                                   KdfBdSubCount *__restrict__ bases, uint64_t *__restrict__ totals, int64_t *__restrict__ offsets, uint64_t cap_reads)
{
    if (blockIdx.x | threadIdx.x) return;
    uint64_t r = 0, p = 0, j = 0;
    for (; j < n_sub && sub_status[j] == KDF_SUB_DONE; ++j) { bases[j] = KdfBdSubCount{r, p}; r += counts[j].reads; p += counts[j].bases; }
    totals[0] = r; totals[1] = p; totals[2] = j;
    if (r <= cap_reads) offsets[r] = (int64_t)p;
}

// ---- pack -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kdf_bd_pack_kernel(
    const uint8_t *__restrict__ buf, const int64_t *__restrict__ offsets, const uint64_t *__restrict__ src, uint64_t n_reads, uint64_t n_bases,
    uint64_t n_words, uint64_t *__restrict__ packed, uint64_t *__restrict__ invalid)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;                                            // n_words = mask words of the stream; packed words = 2 x that
    uint64_t lo = 0, hi = 0, inv = ~0ull;
    const uint64_t p0 = w * 64;
    if (p0 < n_bases) {
        uint64_t a = 0, b = n_reads;                                      // the read that holds p0: the last r with offsets[r] <= p0
        while (a + 1 < b) { const uint64_t m = (a + b) >> 1; if ((uint64_t)offsets[m] <= p0) a = m; else b = m; }
        uint64_t r = a, r0 = (uint64_t)offsets[r], r1 = (uint64_t)offsets[r + 1], sq = src[r];
        const uint64_t pe = n_bases - p0 < 64 ? n_bases - p0 : 64;
        inv = pe < 64 ? ~0ull << pe : 0;
        for (uint64_t t = 0; t < pe; ++t) {
            const uint64_t p = p0 + t;
            if (p >= r1) { ++r; r0 = r1; r1 = (uint64_t)offsets[r + 1]; sq = src[r]; }       // (every read holds >= 1 position: its separator)
            const uint64_t i = p - r0;
            if (i + 1 == r1 - r0) { inv |= 1ull << t; continue; }        // the separator
            const uint32_t byte = buf[sq + (i >> 1)], nib = (i & 1) ? (byte & 15u) : (byte >> 4);
            if (nib == 0 || (nib & (nib - 1))) { inv |= 1ull << t; continue; }               // anything but A C G T (1 2 4 8)
            const uint64_t code = (nib >> 1) - (nib >> 3);
            if (t < 32) lo |= code << (2 * t); else hi |= code << (2 * (t - 32));
        }
    }
    invalid[w] = inv; packed[2 * w] = lo; packed[2 * w + 1] = hi;
}
