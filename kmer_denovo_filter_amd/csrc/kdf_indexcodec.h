// kdf_indexcodec.h -- the record codec of the index files ({ref}.k{k}.jf, proband_unique.jf, the merged chunks): keys and
// counts in HBM -> record bytes in HBM (ix_encode_kernel) and back (ix_decode_kernel), and the GF(2) hash position of
// Jellyfish's binary/sorted order (ix_positions_kernel).  The key layout follows the call's k, not the engine's
// (include/kdf.h, "index record codec").  A record is kb = ceil(2k / 8) little-endian key bytes and the count's bytes.
//
// ENCODE is output-centric like kf_format_kernel (kdf_kmerfasta.h): a workgroup owns 4 KiB of the body, a lane 16
// consecutive bytes.  Records have one length R = kb + 4 (5 .. 55), so the record of a byte is
// one multiply-high by ceil(2^64 / R) and one correction.  The keys and counts of the at most 4096 / R + 2 records a
// tile touches are staged in LDS first -- coalesced, or gathered through perm -- and a lane then walks its 16 bytes
// over the staged words and stores them at once.
//
// DECODE is record-centric: a workgroup takes 256 records, stages the aligned 16-byte words that enclose their bytes
// in LDS (so the record area may lie at any alignment and no load leaves the enclosing 16 bytes), and a lane puts one
// record together from 32-bit LDS words, two of them funnel-shifted into each 4 bytes of the record.  Rows of long keys
// go back through LDS so that they leave in whole lines.  The first record whose key has a bit at or above 2k is the
// minimum of one atomic per workgroup, so the report does not depend on the scheduling.
//
// POSITIONS: the position is linear over GF(2) in the key's bits, so it is the XOR of one table entry per key byte:
// table b, entry t = XOR of the columns of the set bits of t at key bits 8b .. 8b + 7.  A workgroup builds the at most
// 16 tables of 256 words in LDS (32 KiB), entry t from entry t & (t - 1) and one column, in nine rounds by the number
// of set bits, and then strides over the keys.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define IX_TILE_BYTES 4096                 // body bytes per encode workgroup: 256 lanes x 16
#define IX_DEC_RECORDS 256                 // records per decode workgroup: one per lane
#define IX_DEC_PAD 48                      // LDS beyond the records' bytes: the 15 bytes in front, and the reads past the last record

// Kernel argument of ix_encode_kernel.
struct IxEncPlan {
    int words, kb;                         // words per key (1, 2 or W of the rows); key bytes of a record
    uint32_t rec, key_rows;                // R = kb + 4; records a workgroup stages: IX_TILE_BYTES / R + 2
    uint64_t magic, n;                     // ceil(2^64 / R); records
};

// FORM 0: lo[n] (k <= 32); 1: lo[n], hi[n] (k 33 .. 63); 2: rows of p.words words in lo.  Grid: ceil(byte_count / 4096);
// dynamic LDS: key_rows x (8 words + 4) bytes.  Writes out[0 .. byte_count) = bytes byte_first .. of the body and nothing
// else; `aligned`: out is 16-byte aligned.  A perm value >= n (a broken precondition) gives a record of zeros, no access.
template <int FORM>
__global__ __launch_bounds__(256) void ix_encode_kernel(const IxEncPlan p, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                        const uint32_t *__restrict__ counts, const uint32_t *__restrict__ perm,
                                                        uint64_t byte_first, uint64_t byte_count, uint8_t *__restrict__ out, int aligned) {
    extern __shared__ uint64_t ix_keys[];                            // [key_rows][W], then uint32 counts[key_rows]
    __shared__ uint64_t first_rec;
    const int W = FORM == 2 ? p.words : FORM + 1;
    const uint32_t R = p.rec, kb = (uint32_t)p.kb;
    uint32_t *const ix_cnt = reinterpret_cast<uint32_t *>(ix_keys + (size_t)p.key_rows * W);
    const uint64_t tile_off = (uint64_t)blockIdx.x * IX_TILE_BYTES, lane_off = tile_off + threadIdx.x * 16u;
    const bool live = lane_off < byte_count;                         // (the tile's first lane always is)
    // the record of the lane's first byte (a lane past the window: of the tile's)
    const uint64_t g = byte_first + (live ? lane_off : tile_off);
    uint64_t e = __umul64hi(g, p.magic);                             // g < 2^63: the quotient or one more
    if (e * R > g) --e;
    uint32_t off = (uint32_t)(g - e * R);

    if (threadIdx.x == 0) first_rec = e;
    __syncthreads();
    const uint64_t e0 = first_rec;
    const uint32_t rows = (uint32_t)min((uint64_t)p.key_rows, p.n - e0);
    auto source = [&](uint32_t i) -> uint64_t { return perm ? (uint64_t)perm[e0 + i] : e0 + i; };
    if constexpr (FORM == 1) {
        for (uint32_t i = threadIdx.x; i < rows; i += 256) {
            const uint64_t s = source(i);
            const bool ok = s < p.n;
            ix_keys[2 * i] = ok ? lo[s] : 0; ix_keys[2 * i + 1] = ok ? hi[s] : 0;
        }
    } else if (!perm) {
        const uint64_t *src = lo + e0 * (uint64_t)W;
        for (uint32_t i = threadIdx.x; i < rows * (uint32_t)W; i += 256) ix_keys[i] = src[i];
    } else {
        for (uint32_t i = threadIdx.x; i < rows * (uint32_t)W; i += 256) {
            const uint32_t r = i / (uint32_t)W, j = i - r * (uint32_t)W;
            const uint64_t s = source(r);
            ix_keys[i] = s < p.n ? lo[s * (uint64_t)W + j] : 0;
        }
    }
    for (uint32_t i = threadIdx.x; i < rows; i += 256) {
        const uint64_t s = source(i);
        ix_cnt[i] = counts && s < p.n ? counts[s] : 0;
    }
    __syncthreads();
    if (!live) return;

    uint32_t row = (uint32_t)(e - e0);                               // (past the staged rows only in bytes past the body's end)
    uint32_t cnt = row < rows ? ix_cnt[row] : 0;
    uint32_t w[4] = {0, 0, 0, 0};
    uint64_t cw = 0;
    int cwi = -1;                                                    // the key word in cw
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        uint32_t ch;
        if (off < kb) {
            const int wi = (int)(off >> 3);
            if (wi != cwi) { cw = row < rows ? ix_keys[row * W + wi] : 0; cwi = wi; }
            ch = (uint32_t)(cw >> (8 * (off & 7))) & 0xFFu;
        } else {
            ch = (cnt >> (8 * (off - kb))) & 0xFFu;
        }
        w[i >> 2] |= ch << (8 * (i & 3));
        if (++off == R) {
            off = 0; ++row; cwi = -1;
            cnt = row < rows ? ix_cnt[row] : 0;
        }
    }
    const uint64_t rem = byte_count - lane_off;
    if (rem >= 16 && aligned) {
        *reinterpret_cast<uint4 *>(out + lane_off) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if ((uint64_t)i < rem) out[lane_off + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

// bytes o .. o + 3 of the LDS image, little-endian, from the two 32-bit words that hold them
__device__ __forceinline__ uint32_t ix_get32(const uint32_t *b32, uint32_t o) {
    return __funnelshift_r(b32[o >> 2], b32[(o >> 2) + 1], (o & 3u) * 8u);
}

// the little-endian value of bytes o .. o + len - 1 (len 1 .. 8)
__device__ __forceinline__ uint64_t ix_get(const uint32_t *b32, uint32_t o, int len) {
    uint64_t v = ix_get32(b32, o);
    if (len > 4) v |= (uint64_t)ix_get32(b32, o + 4) << 32;
    return len < 8 ? v & ((1ull << (8 * len)) - 1) : v;
}

// bytes needed in LDS by a decode workgroup of KW-word keys and records of rd bytes
static inline size_t ix_decode_lds(int KW, uint32_t rd) {
    const size_t image = (size_t)IX_DEC_RECORDS * rd + IX_DEC_PAD, rows = KW > 2 ? (size_t)IX_DEC_RECORDS * KW * 8 : 0;
    return ((image > rows ? image : rows) + 15) / 16 * 16;
}

// KW 1: k <= 32 -> lo (and zeros to hi when given); 2: k 33 .. 63 -> lo, hi; 3 .. 7: odd k 65 .. 201 -> rows of KW words in
// lo.  Grid: ceil(n / 256); dynamic LDS: ix_decode_lds.  bytes: n records of kb + cb bytes at any alignment; loads are
// whole aligned 16-byte words from the one that holds the first byte to the one that holds the last.  counts may be NULL.
template <int KW>
__global__ __launch_bounds__(256) void ix_decode_kernel(const uint8_t *__restrict__ bytes, uint64_t n, int k, int kb, int cb,
                                                        uint64_t *__restrict__ lo, uint64_t *__restrict__ hi, uint32_t *__restrict__ counts,
                                                        unsigned long long *__restrict__ first_bad) {
    extern __shared__ __align__(16) uint8_t ix_buf[];
    __shared__ unsigned long long wave_bad[4];
    const uint32_t rd = (uint32_t)(kb + cb);
    const uint64_t r0 = (uint64_t)blockIdx.x * IX_DEC_RECORDS;
    const uint32_t nrec = (uint32_t)min((uint64_t)IX_DEC_RECORDS, n - r0);
    const uint8_t *first = bytes + r0 * rd;
    const uint32_t shift = (uint32_t)((uintptr_t)first & 15);
    const uint4 *src = reinterpret_cast<const uint4 *>(first - shift);
    const uint32_t nvec = (shift + nrec * rd + 15) / 16;
    for (uint32_t c = threadIdx.x; c < nvec; c += 256) reinterpret_cast<uint4 *>(ix_buf)[c] = src[c];
    __syncthreads();

    const uint32_t *b32 = reinterpret_cast<const uint32_t *>(ix_buf);
    const bool have = threadIdx.x < nrec;
    const uint32_t s = shift + threadIdx.x * rd;
    uint64_t key[KW];
    uint32_t cnt = 0;
    bool bad = false;
    if (have) {
#pragma unroll
        for (int j = 0; j < KW; ++j) {
            const int len = kb - 8 * j;
            key[j] = len > 0 ? ix_get(b32, s + 8 * j, len < 8 ? len : 8) : 0;
        }
        uint64_t c64 = ix_get(b32, s + kb, cb < 8 ? cb : 8);
        if (cb > 8 && ix_get(b32, s + kb + 8, cb - 8)) c64 = ~0ull;   // a byte past the eighth is set
        cnt = c64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c64;
        const int tb = 2 * k - 64 * (KW - 1);                        // bits of the top word
        bad = tb < 64 && (key[KW - 1] >> tb) != 0;
    } else {
#pragma unroll
        for (int j = 0; j < KW; ++j) key[j] = 0;
    }
    const uint64_t r = r0 + threadIdx.x;
    if constexpr (KW == 1) {
        if (have) { lo[r] = key[0]; if (hi) hi[r] = 0; }
    } else if constexpr (KW == 2) {
        if (have) { lo[r] = key[0]; hi[r] = key[1]; }
    } else {
        __syncthreads();                                             // (every lane has read its record: the image may go)
        uint64_t *rows = reinterpret_cast<uint64_t *>(ix_buf);
#pragma unroll
        for (int j = 0; j < KW; ++j) rows[threadIdx.x * KW + j] = key[j];
        __syncthreads();
        uint64_t *dst = lo + r0 * KW;
        for (uint32_t i = threadIdx.x; i < nrec * KW; i += 256) dst[i] = rows[i];
    }
    if (have && counts) counts[r] = cnt;

    unsigned long long b = bad ? (unsigned long long)r : ~0ull;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_xor(b, o); b = y < b ? y : b; }
    if ((threadIdx.x & 63) == 0) wave_bad[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < 4; ++j) b = wave_bad[j] < b ? wave_bad[j] : b;
        if (b != ~0ull) atomicMin(first_bad, b);
    }
}

// Kernel argument of ix_positions_kernel: bit[b] = the matrix column of key bit b (columns[2k - 1 - b]) ANDed with
// size - 1, zero from bit 2k on.
struct IxColumns { uint64_t bit[128]; };

// FORM 0: lo[n] (k <= 32); 1: lo[n], hi[n] (k 33 .. 63).  Any grid (the lanes stride over the keys); dynamic LDS: kb x 2 KiB.
template <int FORM>
__global__ __launch_bounds__(256) void ix_positions_kernel(const IxColumns cols, int kb, const uint64_t *__restrict__ lo,
                                                           const uint64_t *__restrict__ hi, uint64_t n, uint64_t *__restrict__ pos) {
    extern __shared__ uint64_t ix_tab[];                             // [kb][256]
    const uint32_t t = threadIdx.x;
    const int bits = __popc(t);
    for (int round = 0; round <= 8; ++round) {                       // entry t of every table, once entry t & (t - 1) is there
        if (bits == round)
            for (int b = 0; b < kb; ++b)
                ix_tab[b * 256 + t] = t ? ix_tab[b * 256 + (t & (t - 1))] ^ cols.bit[8 * b + __ffs(t) - 1] : 0;
        __syncthreads();
    }
    const int nlo = kb < 8 ? kb : 8;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + t; i < n; i += (uint64_t)gridDim.x * 256) {
        uint64_t v = lo[i], x = 0;
        for (int b = 0; b < nlo; ++b, v >>= 8) x ^= ix_tab[b * 256 + (uint32_t)(v & 0xFF)];
        if constexpr (FORM == 1) {
            v = hi[i];
            for (int b = 8; b < kb; ++b, v >>= 8) x ^= ix_tab[b * 256 + (uint32_t)(v & 0xFF)];
        }
        pos[i] = x;
    }
}
