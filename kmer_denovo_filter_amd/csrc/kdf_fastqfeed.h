// kdf_fastqfeed.h -- the device FASTQ feeder (include/kdf.h, "device FASTQ feeder"): the raw text of a four-line FASTQ in
// HBM -> the packed 2-bit stream, its invalid mask (low qualities included) and the record offsets, by the per-byte rule
// of the header.  A line's role follows only from its number, and '@' and '+' are legal quality bytes, so nothing is
// classified byte-locally: the line ends are numbered first, the records are read off them, and the pack is driven by
// the OUTPUT:
//   1. kfq_end_kernel      one workgroup: the end of the text in front of its trailing '\n' / '\r' (a call that is not the
//                          last keeps the first line end of them); resets the control words
//   2. kfq_count_kernel    per tile of KDF_FASTQ_TILE_BYTES = 256 lanes x 16 bytes (aligned 16-byte loads at any alignment of
//                          the text: the tiles are laid over the memory, not over the text): its line ends
//   3. kfq_scan_kernel     one workgroup: the tiles' first line numbers, the number of lines and of records, and how many
//                          of the records the capacities admit: those are examined
//   4. kfq_lines_kernel    per tile: nl[i] = the offset of line end i (the final call's text end closes the last line)
//   5. kfq_records_kernel  a thread per record: the four rules, an atomic minimum of (offset << 3 | rule) over the bad
//                          records, the record's positions (bases + separator) and their sum per block of 256 records
//   6. kfq_total_kernel    one workgroup: scans the block sums, decides the verdict, writes the results
//   7. kfq_offsets_kernel  per block of 256 records: the offsets (to the scratch and the caller), and word_rec[w] = the
//                          record that position 64 w lies in -- a record of more than 8 words is spread by its whole block
//   8. kfq_pack_kernel     a wave per 64 positions: record of the first position from word_rec, the next 64 offsets in
//                          the lanes (offsets rise by >= 1: a record's separator), an OR over the wave marks the positions
//                          where records begin, a popcount gives each lane its record; base byte and quality byte are
//                          loaded; three ballots are the mask word and, interleaved, the two packed words.  The waves
//                          behind the last position write the padding words of kdf_stream_words.
// 7 and 8 read the verdict of 6 and do nothing after a refusal, so the host synchronises once.
//
// kdf_fq_extract (include/kdf.h, "FASTQ record extract") shares 1 .. 5 -- the records are the feeder's -- and goes on with
//   6x. kfx_len_kernel     a thread per record: (kept << 32 | bytes the record takes in the output), 0 for a dropped one,
//                          and their sum per block of 256 records; the last record of a final call fixes where its text ends
//   7x. kfq_total_kernel   its EXTRACT form: scans the block sums, decides the verdict, writes the results
//   8x. kfx_offsets_kernel per block of 256 records: the byte offset of every record in the output (a plateau over dropped
//                          records), the caller's offsets of the kept ones, and tile_rec[T] = the record that the first
//                          byte of output tile T lies in
//   9x. kfx_copy_kernel    output-driven: a workgroup per tile of 256 granules of 16 bytes of the OUTPUT's memory, a lane
//                          per granule; the record by a binary search between tile_rec[T] and tile_rec[T + 1]; a granule
//                          inside one record's text is two aligned 16-byte loads shifted together and ONE 16-byte store,
//                          any other granule goes byte by byte
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kdf.h"
#include "kdf_scan.h"
#include "kdf_text.h"

#define KFQ_TILE KDF_FASTQ_TILE_BYTES
static_assert(KFQ_TILE == 256 * 16, "a tile is 256 lanes of 16 bytes");
#define KFQ_REC_BLOCK 256                      // records per workgroup of the record passes
#define KFQ_SELF_WORDS 8                       // a record of more words of 64 positions is spread over word_rec by its block
// control words (uint64)
// (KFX_LAST_END: kdf_fq_extract's, the end of the last record's text on a final call)
enum { KFQ_N_EFF = 0, KFQ_NL, KFQ_LINES, KFQ_N_REC, KFQ_N_CHK, KFQ_FIRST_BAD, KFQ_ROOM, KFX_LAST_END, KFQ_RES = 8, KFQ_CTL_WORDS = 12 };
// the results, ctl[KFQ_RES ..]: [0] n_bases [1] n_reads [2] consumed [3] verdict | (offset << 3 | rule) << 8
// (kdf_fq_extract: [0] out_bytes [1] n_kept | records << 32); KFX_ERR_COUNT: the caller's n_reads is not the records'
enum { KFQ_OK = 0, KFQ_ERR_ROOM = 1, KFQ_ERR_FORMAT = 2, KFQ_NOTHING = 3, KFX_ERR_COUNT = 4 };

// the arrays of one call in the engine's scratch
struct KfqScratchView {
    unsigned long long *ctl;                   // [KFQ_CTL_WORDS]
    uint32_t *tile_nl;                         // [tiles]: line ends of a tile, then the number of the tile's first
    uint32_t *nl;                              // [4 r_cap]: offsets of the line ends
    unsigned long long *off;                   // [r_cap + 1]: positions of a record, then its offset
    unsigned long long *bsum;                  // [ceil(r_cap / KFQ_REC_BLOCK)]: positions of a block of records, then its offset
    uint32_t *word_rec;                        // [ceil(pos_cap / 64)] (kdf_fastq_pack)
    uint32_t *tile_rec;                        // [output tiles + 1] (kdf_fq_extract), in the place of word_rec: a call has one or the other
};

// The text as 16-byte granules of the memory it lies in: granule g holds the text offsets [16 g - skew, 16 g - skew + 16),
// skew = the text's address mod 16, so a granule that lies wholly inside the text is ONE aligned 16-byte load at any
// alignment of the text; the first and the last granule are read byte by byte.  s0: the text offset of the granule's first
// byte (negative in the first granule of a skewed text).  -> bit i: byte s0 + i is a '\n' below n_eff
__device__ __forceinline__ uint32_t kfq_line_ends(const uint8_t *__restrict__ t, uint64_t n, uint64_t n_eff, int64_t s0) {
    if (s0 >= (int64_t)n_eff) return 0;
    const uint4 v = kt_load_granule(t, s0, 0, (int64_t)n, true, 0u);   // (the bytes from n_eff on are masked off below)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = w[j] ^ 0x0A0A0A0Au;                         // a zero byte where a '\n' was
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu) >> 7;      // bit 0 / 8 / 16 / 24
        m |= ((z | z >> 7 | z >> 14 | z >> 21) & 0xFu) << (4 * j);
    }
    const int64_t left = (int64_t)n_eff - s0;
    return left >= 16 ? m : m & ((1u << left) - 1u);
}

__global__ __launch_bounds__(256) void kfq_end_kernel(const uint8_t *__restrict__ t, uint64_t n, int final_chunk, unsigned long long *__restrict__ ctl) {
    const uint32_t tid = threadIdx.x;
    // the final call's text ends there; a call that is not the last sees the first line end behind it
    uint64_t n_eff = kt_last_outside(t, n, [](uint8_t c) { return c == '\n' || c == '\r'; });
    if (!final_chunk) {
        while (n_eff < n && t[n_eff] == '\r') ++n_eff;
        n_eff = min(n_eff + 1, n);
    }
    if (tid < KFQ_CTL_WORDS) ctl[tid] = tid == KFQ_N_EFF ? n_eff : tid == KFQ_FIRST_BAD ? ~0ull : 0ull;
}

__global__ __launch_bounds__(256) void kfq_count_kernel(const uint8_t *__restrict__ t, uint64_t n, uint32_t skew, const unsigned long long *__restrict__ ctl,
                                                        uint32_t *__restrict__ tile_nl) {
    __shared__ uint32_t wsum[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t v = (uint32_t)__popc(kfq_line_ends(t, n, ctl[KFQ_N_EFF], (int64_t)((uint64_t)blockIdx.x * KFQ_TILE + 16u * tid) - skew));
    const uint32_t sum = kb_block_sum(v, wsum);
    if (tid == 0) tile_nl[blockIdx.x] = sum;
}

// One workgroup of 256; thread i owns the tiles [i * per, (i + 1) * per).  cap_rec: the records the caller's buffers admit;
// r_cap: the records the scratch admits (<= cap_rec; a well-formed text has no more, see kdf_fastqfeed.hip).
__global__ __launch_bounds__(256) void kfq_scan_kernel(uint32_t *__restrict__ tile_nl, uint64_t nt, int final_chunk, uint64_t cap_rec, uint64_t r_cap,
                                                       unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t ws[17];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (nt + 255) / 256, b = min(nt, tid * per), e = min(nt, b + per);
    uint32_t sum = 0;
    for (uint64_t i = b; i < e; ++i) sum += tile_nl[i];
    uint32_t total;
    uint32_t run = kb_block_exscan(sum, ws, &total);                   // (a chunk has at most 2^31 bytes)
    for (uint64_t i = b; i < e; ++i) { const uint32_t c = tile_nl[i]; tile_nl[i] = run; run += c; }
    if (tid == 0) {
        const uint64_t n_eff = ctl[KFQ_N_EFF];
        const uint64_t lines = final_chunk ? (n_eff ? (uint64_t)total + 1 : 0) : total;      // (the text's end closes the last line)
        const uint64_t n_rec = final_chunk ? (lines + 3) / 4 : lines / 4;
        ctl[KFQ_NL] = total; ctl[KFQ_LINES] = lines; ctl[KFQ_N_REC] = n_rec;
        ctl[KFQ_N_CHK] = min(n_rec, r_cap);
        ctl[KFQ_ROOM] = n_rec > cap_rec;
    }
}

__global__ __launch_bounds__(256) void kfq_lines_kernel(const uint8_t *__restrict__ t, uint64_t n, uint32_t skew, int final_chunk,
                                                        const unsigned long long *__restrict__ ctl, const uint32_t *__restrict__ tile_nl,
                                                        uint32_t *__restrict__ nl) {
    __shared__ uint32_t ws[17];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_eff = ctl[KFQ_N_EFF], keep = 4 * ctl[KFQ_N_CHK];
    const int64_t s0 = (int64_t)((uint64_t)blockIdx.x * KFQ_TILE + 16u * tid) - skew;
    uint32_t m = kfq_line_ends(t, n, n_eff, s0);
    uint64_t idx = (uint64_t)tile_nl[blockIdx.x] + kb_block_exscan((uint32_t)__popc(m), ws, nullptr);
    for (; m && idx < keep; m &= m - 1, ++idx) nl[idx] = (uint32_t)(s0 + (uint32_t)(__ffs(m) - 1));
    if (blockIdx.x == 0 && tid == 0 && final_chunk && n_eff && ctl[KFQ_NL] < keep) nl[ctl[KFQ_NL]] = (uint32_t)n_eff;
}

// the line [s, e) without the '\r' directly in front of its end
__device__ __forceinline__ uint32_t kfq_strip(const uint8_t *__restrict__ t, uint32_t s, uint32_t e) {
    while (e > s && t[e - 1] == '\r') --e;
    return e;
}

__global__ __launch_bounds__(KFQ_REC_BLOCK) void kfq_records_kernel(const uint8_t *__restrict__ t, int final_chunk, unsigned long long *__restrict__ ctl,
                                                                    const uint32_t *__restrict__ nl, unsigned long long *__restrict__ off,
                                                                    unsigned long long *__restrict__ bsum) {
    __shared__ uint32_t wsum[KFQ_REC_BLOCK / 64];
    const uint64_t n_chk = ctl[KFQ_N_CHK], lines = ctl[KFQ_LINES], r = (uint64_t)blockIdx.x * KFQ_REC_BLOCK + threadIdx.x;
    if ((uint64_t)blockIdx.x * KFQ_REC_BLOCK >= n_chk) return;
    uint32_t positions = 0;
    if (r < n_chk) {
        const uint32_t have = final_chunk && lines - 4 * r < 4 ? (uint32_t)(lines - 4 * r) : 4u;       // lines of the record: 1 .. 4
        const uint32_t s0 = r ? nl[4 * r - 1] + 1 : 0, e0 = nl[4 * r];
        uint32_t rule = (s0 < e0 && t[s0] == '@') ? 0u : KDF_FQ_BAD_HEADER, len = 0;
        if (have >= 2) {
            const uint32_t s1 = e0 + 1, e1 = nl[4 * r + 1];
            len = kfq_strip(t, s1, e1) - s1;
            if (have >= 3) {
                const uint32_t s2 = e1 + 1, e2 = nl[4 * r + 2];
                if (!rule && !(s2 < e2 && t[s2] == '+')) rule = KDF_FQ_BAD_PLUS;
                if (have == 4) {
                    const uint32_t s3 = e2 + 1;
                    if (!rule && kfq_strip(t, s3, nl[4 * r + 3]) - s3 != len) rule = KDF_FQ_LENGTH;
                }
            }
        }
        if (!rule && have < 4 && !(have == 3 && len == 0)) rule = KDF_FQ_TRUNCATED;      // (three lines and no bases: the quality line is empty)
        if (rule) atomicMin(&ctl[KFQ_FIRST_BAD], (unsigned long long)s0 << 3 | rule);
        positions = len + 1;
        off[r] = positions;
    }
    const uint32_t sum = kb_block_sum(positions, wsum);                // (a 32-bit sum: the text of a call has fewer than 2^31 bytes, so a block's positions cannot wrap it)
    if (threadIdx.x == 0) bsum[blockIdx.x] = sum;
}

// One workgroup of 256 behind the record pass (the feeder) or behind kfx_len_kernel (EXTRACT, below): scans the block sums
// and decides the verdict.  The format comes first (among the records the capacities admit); then, for the extract, the
// caller's record count; then the room, cap: the bases (the feeder) or output bytes (the extract) the caller's buffers
// admit.  nothing: a call that is not the last and has no complete record writes nothing.
template <bool EXTRACT>
__global__ __launch_bounds__(256) void kfq_total_kernel(uint64_t n, int final_chunk, uint64_t n_reads, uint64_t cap, const uint32_t *__restrict__ nl,
                                                        unsigned long long *__restrict__ bsum, unsigned long long *__restrict__ ctl) {
    __shared__ unsigned long long ws[4];
    const uint64_t n_rec = ctl[KFQ_N_REC], n_chk = ctl[KFQ_N_CHK], room = ctl[KFQ_ROOM], bad = ctl[KFQ_FIRST_BAD];
    const unsigned long long total = kb_sums_exscan(bsum, (n_chk + KFQ_REC_BLOCK - 1) / KFQ_REC_BLOCK, ws);
    if (threadIdx.x) return;
    const uint64_t size = EXTRACT ? total & 0xFFFFFFFFull : total;    // EXTRACT: kept << 32 | bytes
    uint64_t verdict = KFQ_OK;
    if (bad != ~0ull) verdict = KFQ_ERR_FORMAT | bad << 8;
    else if (EXTRACT && (n_rec != n_reads || n_chk < n_rec)) verdict = KFX_ERR_COUNT;      // (n_chk < n_rec without room or a bad record cannot be: a guard,
    else if ((!EXTRACT && (room || n_chk < n_rec)) || size > cap) verdict = KFQ_ERR_ROOM;  // here and below)
    else if (!final_chunk && n_rec == 0) verdict = KFQ_NOTHING;
    ctl[KFQ_RES + 0] = size; ctl[KFQ_RES + 1] = EXTRACT ? total >> 32 | n_rec << 32 : n_rec;
    ctl[KFQ_RES + 2] = final_chunk ? n : (n_rec && verdict == KFQ_OK ? (uint64_t)nl[4 * n_rec - 1] + 1 : 0);
    ctl[KFQ_RES + 3] = verdict;
}

// owner[w] = r for the slots w0 <= w < w1 that record r owns (index words of 64 positions: the feeder; output tiles: the
// extract), by a workgroup of KFQ_REC_BLOCK records.  A record of up to KFQ_SELF_WORDS slots marks them itself, a longer
// one is handed to the whole block.  mine: the thread has a record to mark.  REQUIRES blockDim.x == KFQ_REC_BLOCK and a
// block-uniform call that every thread reaches (barriers inside); the LDS is the function's own: one call per kernel.
__device__ __forceinline__ void kfq_mark_owner(bool mine, uint32_t r, uint64_t w0, uint64_t w1, uint32_t *__restrict__ owner) {
    __shared__ uint32_t n_long, long_rec[KFQ_REC_BLOCK];
    __shared__ unsigned long long long_w0[KFQ_REC_BLOCK], long_w1[KFQ_REC_BLOCK];
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    if (mine) {
        if (w1 - w0 <= KFQ_SELF_WORDS) {
            for (uint64_t w = w0; w < w1; ++w) owner[w] = r;
        } else {
            const uint32_t i = atomicAdd(&n_long, 1u);
            long_rec[i] = r; long_w0[i] = w0; long_w1[i] = w1;
        }
    }
    __syncthreads();
    for (uint32_t i = 0; i < n_long; ++i)
        for (uint64_t w = long_w0[i] + threadIdx.x; w < long_w1[i]; w += KFQ_REC_BLOCK) owner[w] = long_rec[i];
}

__global__ __launch_bounds__(KFQ_REC_BLOCK) void kfq_offsets_kernel(const unsigned long long *__restrict__ ctl, const unsigned long long *__restrict__ bsum,
                                                                    unsigned long long *__restrict__ off, uint32_t *__restrict__ word_rec,
                                                                    int64_t *__restrict__ offsets) {
    __shared__ uint32_t ws[17];
    if (ctl[KFQ_RES + 3] != KFQ_OK) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t n_rec = ctl[KFQ_RES + 1], n_bases = ctl[KFQ_RES + 0], r0 = (uint64_t)blockIdx.x * KFQ_REC_BLOCK, r = r0 + tid;
    if (blockIdx.x == 0 && tid == 0) {
        off[n_rec] = n_bases;
        if (offsets) offsets[n_rec] = (int64_t)n_bases;
    }
    if (r0 >= n_rec) return;
    const uint32_t positions = r < n_rec ? (uint32_t)off[r] : 0u;
    const uint64_t o = bsum[blockIdx.x] + kb_block_exscan(positions, ws, nullptr);
    if (r < n_rec) {
        off[r] = o;
        if (offsets) offsets[r] = (int64_t)o;
    }
    // the words whose first position is the record's
    kfq_mark_owner(r < n_rec, (uint32_t)r, (o + 63) / 64, (o + positions + 63) / 64, word_rec);
}

// bit i of x -> bit 2 i
__device__ __forceinline__ uint64_t kfq_spread(uint64_t x) {
    x = (x | x << 16) & 0x0000FFFF0000FFFFull;
    x = (x | x << 8) & 0x00FF00FF00FF00FFull;
    x = (x | x << 4) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | x << 2) & 0x3333333333333333ull;
    x = (x | x << 1) & 0x5555555555555555ull;
    return x;
}

// A workgroup of 4 waves; wave w of the grid owns the positions [64 w, 64 w + 64): mask word w, packed words 2 w and 2 w + 1.
template <bool QUAL>
__global__ __launch_bounds__(256) void kfq_pack_kernel(const uint8_t *__restrict__ t, uint32_t min_qual, const unsigned long long *__restrict__ ctl,
                                                       const uint32_t *__restrict__ nl, const unsigned long long *__restrict__ off,
                                                       const uint32_t *__restrict__ word_rec, uint64_t *__restrict__ packed, uint64_t *__restrict__ invalid) {
    if (ctl[KFQ_RES + 3] != KFQ_OK) return;
    const uint64_t n_bases = ctl[KFQ_RES + 0], n_rec = ctl[KFQ_RES + 1], words = (n_bases + 63) / 64;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= words + 2) return;                                        // (wave-uniform)
    uint32_t code = 4;
    if (w < words) {
        const uint64_t base = 64 * w, p = base + lane, r0 = word_rec[w];
        // lane j: the start of record r0 + 1 + j; those inside the wave's positions mark where records begin
        const uint64_t next = r0 + 1 + lane <= n_rec ? off[r0 + 1 + lane] : ~0ull;
        unsigned long long starts = next - base < 64 ? 1ull << (next - base) : 0ull;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) starts |= __shfl_xor(starts, o);
        const uint32_t ahead = (uint32_t)__popcll(starts & (~0ull >> (63 - lane)));      // records that begin in (base, p]
        const uint64_t first = off[r0];
        const uint64_t prev_start = __shfl((unsigned long long)next, ahead ? (int)ahead - 1 : 0), end = __shfl((unsigned long long)next, (int)ahead);
        const uint64_t start = ahead ? prev_start : first, rec = r0 + ahead;
        if (p < n_bases && p + 1 < end) {                              // (p + 1 == end: the separator)
            const uint32_t j = (uint32_t)(p - start);
            code = kdf_base_code(t[nl[4 * rec] + 1 + j]);
            if (QUAL && t[nl[4 * rec + 2] + 1 + j] < min_qual) code = 4;
        }
    }
    const unsigned long long inv = __ballot(code > 3), lo = __ballot(code & 1u), hi = __ballot((code >> 1) & 1u);      // (4: bits 0)
    if (lane < 2) packed[2 * w + lane] = kfq_spread((lo >> (32 * lane)) & 0xFFFFFFFFull) | kfq_spread((hi >> (32 * lane)) & 0xFFFFFFFFull) << 1;
    else if (lane == 2) invalid[w] = inv;
}

// ---- kdf_fq_extract: the kept records back out as text -------------------------------------------------------------
// A record's value in the scans: kept << 32 | bytes.  An output has at most 2^31 + 2 bytes and a call fewer than 2^29
// records, so the two halves never carry into each other and one 64-bit sum scans both.

// Behind kfq_records_kernel, which has checked record r; off and bsum are written again with the extract's values.  A
// record's text is [s0, end): through the '\n' of line 3.  The last record of a final call ends at n_eff, where only '\r' and
// '\n' follow: it goes on through the first '\n' when there is one, else a '\n' is supplied; a record of three lines is
// given its quality line, one more '\n'.  keep is read below the caller's n_reads only (a wrong n_reads is refused later).
__global__ __launch_bounds__(KFQ_REC_BLOCK) void kfx_len_kernel(const uint8_t *__restrict__ t, uint64_t n, int final_chunk, const uint8_t *__restrict__ keep,
                                                                uint64_t n_reads, unsigned long long *__restrict__ ctl, const uint32_t *__restrict__ nl,
                                                                unsigned long long *__restrict__ off, unsigned long long *__restrict__ bsum) {
    __shared__ unsigned long long wsum[KFQ_REC_BLOCK / 64];
    const uint64_t n_chk = ctl[KFQ_N_CHK], n_rec = ctl[KFQ_N_REC], lines = ctl[KFQ_LINES], r = (uint64_t)blockIdx.x * KFQ_REC_BLOCK + threadIdx.x;
    if ((uint64_t)blockIdx.x * KFQ_REC_BLOCK >= n_chk) return;
    unsigned long long v = 0;
    if (r < n_chk) {
        const uint64_t s0 = r ? (uint64_t)nl[4 * r - 1] + 1 : 0;
        uint64_t end, supplied = 0;
        if (final_chunk && r + 1 == n_rec) {
            const uint64_t n_eff = ctl[KFQ_N_EFF];
            uint64_t p = n_eff;
            while (p < n && t[p] == '\r') ++p;
            if (p < n) end = p + 1;                                    // (behind n_eff lie only '\r' and '\n': t[p] is a '\n')
            else { end = n_eff; supplied = 1; }
            if (lines - 4 * r == 3) ++supplied;
            ctl[KFX_LAST_END] = end;
        } else {
            end = (uint64_t)nl[4 * r + 3] + 1;
        }
        if (r < n_reads && keep[r]) v = 1ull << 32 | (end - s0 + supplied);
        off[r] = v;
    }
    const unsigned long long sum = kb_block_sum(v, wsum);
    if (threadIdx.x == 0) bsum[blockIdx.x] = sum;
}

// oskew: the output's address mod 16.  Output tile T holds the output offsets [KFQ_TILE T - oskew, KFQ_TILE (T + 1) - oskew).
__global__ __launch_bounds__(KFQ_REC_BLOCK) void kfx_offsets_kernel(const unsigned long long *__restrict__ ctl, const unsigned long long *__restrict__ bsum,
                                                                    uint32_t oskew, unsigned long long *__restrict__ off, uint32_t *__restrict__ tile_rec,
                                                                    int64_t *__restrict__ offsets) {
    __shared__ uint32_t ws[17];
    if (ctl[KFQ_RES + 3] != KFQ_OK) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t total = ctl[KFQ_RES + 0], n_kept = ctl[KFQ_RES + 1] & 0xFFFFFFFFull, n_rec = ctl[KFQ_RES + 1] >> 32;
    const uint64_t r0 = (uint64_t)blockIdx.x * KFQ_REC_BLOCK, r = r0 + tid;
    if (blockIdx.x == 0 && tid == 0) {
        off[n_rec] = total;
        if (offsets) offsets[n_kept] = (int64_t)total;
        if (oskew) tile_rec[0] = 0;                                    // (its first byte is output byte 0; without a skew the record at 0 writes it)
    }
    if (r0 >= n_rec) return;
    const unsigned long long v = r < n_rec ? off[r] : 0ull;
    const uint32_t len = (uint32_t)v, kept = (uint32_t)(v >> 32);     // (kept: 0 at and past n_rec)
    const unsigned long long before = bsum[blockIdx.x];
    const uint64_t o = (before & 0xFFFFFFFFull) + kb_block_exscan(len, ws, nullptr);
    const uint64_t rank = (before >> 32) + kb_block_exscan(kept, ws, nullptr);
    if (r < n_rec) off[r] = o;
    if (kept && offsets) offsets[rank] = (int64_t)o;
    // the tiles whose first byte is a kept record's
    kfq_mark_owner(kept, (uint32_t)r, (o + oskew + KFQ_TILE - 1) / KFQ_TILE, (o + len + oskew + KFQ_TILE - 1) / KFQ_TILE, tile_rec);
}

// the last record of [lo, hi] whose offset is <= b (off[lo] <= b).  The offsets do not fall, a dropped record shares its
// successor's, and a kept record takes 6 bytes or more: the record found is the kept one that byte b lies in.
__device__ __forceinline__ uint64_t kfx_find(const unsigned long long *__restrict__ off, uint64_t lo, uint64_t hi, uint64_t b) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the 16 bytes at src, at any alignment, from aligned 16-byte loads: the granule src lies in and, unless src is aligned,
// the next.  Each holds a byte of [src, src + 16), so neither load leaves the pages of the text.
__device__ __forceinline__ uint4 kfx_load16(const uint8_t *src) {
    const uint32_t a = (uint32_t)((uintptr_t)src & 15u);
    const uint4 *p = reinterpret_cast<const uint4 *>(src - a);
    const uint4 v0 = p[0];
    if (a == 0) return v0;
    const uint4 v1 = p[1];
    uint64_t q0 = v0.x | (uint64_t)v0.y << 32, q1 = v0.z | (uint64_t)v0.w << 32, q2 = v1.x | (uint64_t)v1.y << 32;
    const uint64_t q3 = v1.z | (uint64_t)v1.w << 32;
    uint32_t sh = 8 * a;
    if (sh >= 64) { q0 = q1; q1 = q2; q2 = q3; sh -= 64; }
    if (sh) { q0 = q0 >> sh | q1 << (64 - sh); q1 = q1 >> sh | q2 << (64 - sh); }
    return make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
}

// A workgroup takes the output tiles blockIdx.x, blockIdx.x + gridDim.x ... below the output's end: the grid is sized by
// the capacity, the work by the bytes kept.
__global__ __launch_bounds__(256) void kfx_copy_kernel(const uint8_t *__restrict__ t, int final_chunk, uint32_t oskew, const unsigned long long *__restrict__ ctl,
                                                       const uint32_t *__restrict__ nl, const unsigned long long *__restrict__ off,
                                                       const uint32_t *__restrict__ tile_rec, uint8_t *__restrict__ out) {
    if (ctl[KFQ_RES + 3] != KFQ_OK) return;
    const uint64_t total = ctl[KFQ_RES + 0], n_rec = ctl[KFQ_RES + 1] >> 32, last_end = ctl[KFX_LAST_END];
    if (total == 0) return;
    const uint64_t n_tiles = (total + oskew + KFQ_TILE - 1) / KFQ_TILE;
    for (uint64_t T = blockIdx.x; T < n_tiles; T += gridDim.x) {
        const int64_t b0 = (int64_t)(T * KFQ_TILE + 16u * threadIdx.x) - (int64_t)oskew;      // the output offset of the granule's first byte
        if (b0 >= (int64_t)total || b0 + 16 <= 0) continue;
        const uint64_t hi = T + 1 < n_tiles ? tile_rec[T + 1] : n_rec - 1;
        uint64_t r = kfx_find(off, tile_rec[T], hi, b0 > 0 ? (uint64_t)b0 : 0);
        uint64_t o = off[r], next = off[r + 1], s0 = r ? (uint64_t)nl[4 * r - 1] + 1 : 0;
        uint64_t text = (final_chunk && r + 1 == n_rec ? last_end : (uint64_t)nl[4 * r + 3] + 1) - s0;      // bytes of the record that are the text's
        if (b0 >= 0 && (uint64_t)b0 + 16 <= total && (uint64_t)b0 + 16 - o <= text) {
            *reinterpret_cast<uint4 *>(out + b0) = kfx_load16(t + s0 + ((uint64_t)b0 - o));
            continue;
        }
        for (int i = 0; i < 16; ++i) {
            const int64_t bb = b0 + i;
            if (bb < 0) continue;
            if (bb >= (int64_t)total) break;
            if ((uint64_t)bb >= next) {
                r = kfx_find(off, r + 1, hi, (uint64_t)bb);
                o = off[r]; next = off[r + 1]; s0 = (uint64_t)nl[4 * r - 1] + 1;
                text = (final_chunk && r + 1 == n_rec ? last_end : (uint64_t)nl[4 * r + 3] + 1) - s0;
            }
            const uint64_t j = (uint64_t)bb - o;
            out[bb] = j < text ? t[s0 + j] : (uint8_t)'\n';
        }
    }
}

