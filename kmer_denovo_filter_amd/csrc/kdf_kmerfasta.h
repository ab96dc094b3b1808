// kdf_kmerfasta.h -- the text codec of the k-mer FASTA files the discovery stages hand on (`>{i}\n{KMER}\n`), and of the
// (n, k) ASCII matrix of keys.to_ascii: keys in HBM -> text in HBM (kf_format_kernel) and back (kf_count_kernel,
// kf_parse_kernel).  The key layout follows the call's k, not the engine's (include/kdf.h, "k-mer FASTA codec").
//
// FORMAT is output-centric: a lane owns 16 consecutive bytes of the text and stores them at once.  The text is a
// sequence of at most 20 DIGIT CLASSES: class c holds the records whose index has d0 + c decimal digits, all of one
// length (digits + k + 3), so the record of a byte is
//     class  = the last c with cls_byte[c] <= byte            (a walk over <= 20 kernel arguments)
//     record = cls_rec[c] + (byte - cls_byte[c]) / length     (one multiply-high by ceil(2^64 / length), one correction)
// and the lane then walks its 16 bytes carrying (record, offset in the record, digits of the index).  A workgroup's 4 KiB
// of text touch at most 4096 / (shortest record) + 2 consecutive records; their keys are staged in LDS with coalesced
// loads first, so a key word is read from HBM once per workgroup whatever the record boundaries do to the lanes.
//
// PARSE runs over 4 KiB tiles of the text held in LDS with one byte before and k + 2 bytes behind:
//   1. kf_count_kernel  the sequence-line starts of a tile (a byte whose predecessor is '\n', that is not '>' and does
//                       not start an empty line) -> block sums; the offset behind the last '\n' -> one atomic maximum
//   2. kh_scan_kernel   exclusive scan of the block sums (kdf_hits.h)
//   3. kf_parse_kernel  the same tiles again, a workgroup scan of the per-lane counts, then every lane takes the lines
//                       that start in its 16 bytes: terminator at + k ('\n', "\r\n"), k bases, canonical key, row stored
//                       at the line's rank -- file order whatever the scheduling.  The first bad line is an atomic
//                       minimum of (offset, rule), so the report does not depend on the scheduling either.
// A chunk that is not the file's last ends in a line without '\n': pass 1 counts its start like any other (it is the
// last one, so no rank moves), pass 3 recognises it by its offset (>= the maximum of pass 1), stores nothing, checks
// nothing and raises a flag that takes it off the count.
#pragma once
#include "kdf_tilewalk.h"
#include "kdf_scan.h"
#include "kdf_text.h"

#define KF_TILE_BYTES 4096                 // text bytes per workgroup: 256 lanes x 16
#define KF_MAX_CLASSES 20
#define KF_HALO 208                        // bytes behind a parse tile: k + 2 <= 203 (the bases, '\r', '\n'), in 16s
#define KF_PRE 16                          // a tile's LDS copy starts at byte 16: byte 15 is the text's byte before the tile

// ---- format ---------------------------------------------------------------------------------------------------------
// Kernel argument of kf_format_kernel, built on the host (kf_plan, kdf_kmerfasta.hip).  KDF_TEXT_ROWS: one class of
// records of k bytes.
struct KfPlan {
    int k, words;                          // words per key: 1, 2 ((lo, hi) arrays) or W of the rows
    int ncls, d0;                          // classes; decimal digits of first_index (class c: d0 + c digits)
    uint32_t key_rows;                     // keys a workgroup stages: KF_TILE_BYTES / shortest record + 2
    uint64_t n, first_index;
    uint64_t cls_byte[KF_MAX_CLASSES + 1]; // text offset of class c's first record; [ncls]: the whole text
    uint64_t cls_rec[KF_MAX_CLASSES];      // ... and that record's number, 0 .. n - 1
    uint64_t cls_magic[KF_MAX_CLASSES];    // ceil(2^64 / record length); 0: length 1
};

// FORM 0: lo[n] (k <= 32); 1: lo[n], hi[n] (k 33 .. 63); 2: rows of p.words words in lo.  Grid: ceil(byte_count / 4096).
// Writes out[0 .. byte_count) = bytes byte_first .. of the text and nothing else; `aligned`: out is 16-byte aligned.
template <int FORM, bool FASTA>
__global__ __launch_bounds__(256) void kf_format_kernel(const KfPlan p, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                                        uint64_t byte_first, uint64_t byte_count, uint8_t *__restrict__ out, int aligned) {
    extern __shared__ uint64_t kf_keys[];                            // [rows][W]
    __shared__ uint64_t first_rec;
    const int k = p.k, W = FORM == 2 ? p.words : FORM + 1;
    const uint64_t tile_off = (uint64_t)blockIdx.x * KF_TILE_BYTES, lane_off = tile_off + threadIdx.x * 16u;
    const bool live = lane_off < byte_count;                         // (the tile's first lane always is)
    // the record of the lane's first byte (a lane past the window: of the tile's)
    const uint64_t g = byte_first + (live ? lane_off : tile_off);
    int c = 0;
    for (int j = 1; j < p.ncls; ++j) c += g >= p.cls_byte[j];
    int d = FASTA ? p.d0 + c : 0;
    uint32_t len = FASTA ? (uint32_t)(d + k + 3) : (uint32_t)k;
    const uint64_t x = g - p.cls_byte[c], magic = p.cls_magic[c];
    uint64_t q = magic ? __umul64hi(x, magic) : x;                   // x < 2^63: the quotient or one more
    if (magic && q * len > x) --q;
    uint32_t off = (uint32_t)(x - q * len);
    uint64_t e = p.cls_rec[c] + q;

    if (threadIdx.x == 0) first_rec = e;
    __syncthreads();
    const uint64_t e0 = first_rec;
    const uint32_t rows = (uint32_t)min((uint64_t)p.key_rows, p.n - e0);
    if constexpr (FORM == 1) {
        for (uint32_t i = threadIdx.x; i < rows; i += 256) { kf_keys[2 * i] = lo[e0 + i]; kf_keys[2 * i + 1] = hi[e0 + i]; }
    } else {
        const uint64_t *src = lo + e0 * (uint64_t)W;
        for (uint32_t i = threadIdx.x; i < rows * (uint32_t)W; i += 256) kf_keys[i] = src[i];
    }
    __syncthreads();
    if (!live) return;

    uint64_t idx = p.first_index + e, p10 = 1, dig_lo = 0;
    uint32_t dig_hi = 0;                                             // decimal digits of idx, 4 bits each, units first
    for (int j = 0; j < d; ++j) p10 *= 10;                           // d <= 19: the first index of the next class
    auto digits = [&]() {
        uint64_t v = idx;
        dig_lo = 0; dig_hi = 0;
        for (int j = 0; j < d; ++j) {
            const uint64_t t = v / 10, r = v - t * 10;
            if (j < 16) dig_lo |= r << (4 * j); else dig_hi |= (uint32_t)r << (4 * (j - 16));
            v = t;
        }
    };
    if (FASTA && off <= (uint32_t)d) digits();
    uint32_t w[4] = {0, 0, 0, 0};
    uint64_t cw = 0;
    int cwi = -1;                                                    // the key word in cw
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int b = FASTA ? (int)off - d - 2 : (int)off;           // base of the k-mer, -1 and k: the two '\n'
        uint32_t ch;
        if (FASTA && off == 0) ch = '>';
        else if (FASTA && off <= (uint32_t)d) {
            const int r = d - (int)off;
            ch = '0' + (r < 16 ? (uint32_t)(dig_lo >> (4 * r)) & 15u : (dig_hi >> (4 * (r - 16))) & 15u);
        } else if (FASTA && (b < 0 || b == k)) ch = '\n';
        else {
            const int sh = 2 * (k - 1 - b), wi = sh >> 6;
            if (wi != cwi) {
                const uint64_t row = e - e0;                         // (past the staged rows only in bytes past the text's end)
                cw = row < rows ? kf_keys[row * W + wi] : 0;
                cwi = wi;
            }
            ch = (0x54474341u >> (8 * ((uint32_t)(cw >> (sh & 63)) & 3u))) & 0xFFu;
        }
        w[i >> 2] |= ch << (8 * (i & 3));
        if (++off == len) {
            off = 0; ++e; ++idx; cwi = -1;
            if (FASTA) {
                if (idx == p10) { ++d; ++len; p10 *= 10; }
                digits();
            }
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

// ---- parse ----------------------------------------------------------------------------------------------------------
// The text as the rule reads it: its n bytes, one '\n' behind them when the last chunk lacks it (`supply`), zeros beyond.
struct KfText { const uint8_t *t; uint64_t n; int supply, aligned; };

__device__ __forceinline__ KfText kf_text(const uint8_t *t, uint64_t n, int final_chunk) {
    return KfText{t, n, final_chunk && t[n - 1] != '\n', ((uintptr_t)t & 15) == 0};
}

// buf[KF_PRE + j] = byte t0 + j of the text, j = -1 .. KF_TILE_BYTES + HALO - 1 (HALO in 16s); before byte 0 lies a '\n'
template <int HALO>
__device__ __forceinline__ void kf_load_tile(const KfText &x, uint64_t t0, uint8_t *buf) {
    for (uint32_t c = threadIdx.x; c < (KF_TILE_BYTES + HALO) / 16; c += 256) {
        const uint64_t p = t0 + 16 * c;
        *reinterpret_cast<uint4 *>(buf + KF_PRE + 16 * c) = kt_load_granule(x.t, (int64_t)p, 0, (int64_t)x.n, x.aligned, 0u);
        if (x.supply && x.n - p < 16) buf[KF_PRE + 16 * c + (uint32_t)(x.n - p)] = '\n';      // (x.n < p wraps: no byte of this granule)
    }
    if (threadIdx.x == 0) buf[KF_PRE - 1] = t0 ? x.t[t0 - 1] : '\n';
    __syncthreads();
}

// bit i: a sequence line starts at the lane's byte i (text offset s0 + i, buf index j0 + i)
__device__ __forceinline__ uint32_t kf_lane_starts(const uint8_t *buf, uint32_t j0, uint64_t s0, uint64_t n) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint8_t c = buf[j0 + i];
        const bool seq = buf[j0 + i - 1] == '\n' && c != '>' && c != '\n' && !(c == '\r' && buf[j0 + i + 1] == '\n');
        m |= (uint32_t)(seq && s0 + i < n) << i;
    }
    return m;
}

// ctl, behind the block sums' total: [0] the first bad line, offset * 2 + rule (0 length, 1 base), ~0: none; [1] the
// offset behind the last '\n'; [2] the chunk's unfinished last line was counted as a sequence line
__global__ void kf_ctl_init_kernel(unsigned long long *ctl) { ctl[0] = ~0ull; ctl[1] = 0; ctl[2] = 0; }

__global__ __launch_bounds__(256) void kf_count_kernel(const uint8_t *__restrict__ t, uint64_t n, int final_chunk,
                                                       unsigned long long *__restrict__ block_sums, unsigned long long *__restrict__ ctl) {
    __shared__ __align__(16) uint8_t buf[KF_PRE + KF_TILE_BYTES + 16];
    __shared__ uint32_t ws[17];
    __shared__ unsigned long long nl[4];
    const KfText x = kf_text(t, n, final_chunk);
    const uint64_t t0 = (uint64_t)blockIdx.x * KF_TILE_BYTES, s0 = t0 + threadIdx.x * 16u;
    kf_load_tile<16>(x, t0, buf);
    const uint32_t j0 = KF_PRE + threadIdx.x * 16u;
    uint32_t total;
    kb_block_exscan((uint32_t)__popc(kf_lane_starts(buf, j0, s0, n)), ws, &total);
    unsigned long long last = 0;                                      // behind the lane's last '\n'
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (buf[j0 + i] == '\n' && s0 + i < n) last = s0 + i + 1;
    last = kb_block_max(last, nl);
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x] = total;
        if (last) atomicMax(&ctl[1], last);
    }
}

// KW 1: k <= 32 -> lo; 2: k 33 .. 63 -> lo, hi; 3 .. 7: odd k 65 .. 201 -> rows of KW words in lo.  Rows rank < cap only.
template <int KW>
__global__ __launch_bounds__(256) void kf_parse_kernel(const uint8_t *__restrict__ t, uint64_t n, int final_chunk, int k, int canonical,
                                                       const unsigned long long *__restrict__ block_off, unsigned long long *__restrict__ ctl,
                                                       uint64_t *__restrict__ lo, uint64_t *__restrict__ hi, uint64_t cap) {
    __shared__ __align__(16) uint8_t buf[KF_PRE + KF_TILE_BYTES + KF_HALO];
    __shared__ uint32_t ws[17];
    const KfText x = kf_text(t, n, final_chunk);
    const uint64_t t0 = (uint64_t)blockIdx.x * KF_TILE_BYTES, s0 = t0 + threadIdx.x * 16u;
    kf_load_tile<KF_HALO>(x, t0, buf);
    const uint64_t whole = final_chunk ? n : ctl[1];                  // lines that start below it have their '\n'
    const uint32_t j0 = KF_PRE + threadIdx.x * 16u;
    uint32_t starts = kf_lane_starts(buf, j0, s0, n);
    uint64_t rank = block_off[blockIdx.x] + kb_block_exscan((uint32_t)__popc(starts), ws, nullptr);
    for (; starts; starts &= starts - 1, ++rank) {
        const int i = __ffs(starts) - 1;
        const uint64_t s = s0 + i;
        const uint8_t *line = buf + j0 + i;
        if (s >= whole) { ctl[2] = 1; continue; }                     // the unfinished last line: the next chunk's
        uint64_t e0 = 0, e1 = 0;                                      // KW <= 2: base j at bits 2j (kdf_canon_*'s window form)
        KdfRoll<(KW > 2 ? KW : 1)> roll;
#pragma unroll
        for (int j = 0; j < (KW > 2 ? KW : 1); ++j) { roll.f[j] = 0; roll.r[j] = 0; }
        roll.run = 0;
        const int tb = 2 * k - 64 * (KW - 1);
        bool bad_len = false, bad_base = false;
        for (int b = 0; b < k; ++b) {
            const uint8_t c = line[b];
            if (c == '\n') { bad_len = true; break; }
            uint32_t code = kdf_base_code(c);
            if (code > 3) { bad_base = true; code = 0; }
            if constexpr (KW > 2) roll.push(code, false, tb);
            else if (KW == 2 && b >= 32) e1 |= (uint64_t)code << (2 * b - 64);
            else e0 |= (uint64_t)code << (2 * b);
        }
        if (!bad_len) {                                               // k bytes without '\n': the line ends here, after one '\r' at most
            const uint8_t c = line[k];
            bad_len = c == '\n' ? line[k - 1] == '\r' : !(c == '\r' && line[k + 1] == '\n');
        }
        if (bad_len || bad_base) { atomicMin(&ctl[0], (unsigned long long)s * 2 + (bad_len ? 0 : 1)); continue; }
        if (rank >= cap) continue;
        if constexpr (KW == 1) {
            lo[rank] = canonical ? kdf_canon_narrow(e0, k, k >= 32 ? ~0ull : (1ull << (2 * k)) - 1) : kdf_rev2(e0) >> (64 - 2 * k);
        } else if constexpr (KW == 2) {
            uint64_t klo, khi;
            if (canonical) kdf_canon_wide(e0, e1, k, klo, khi);
            else {                                                    // the forward half of kdf_canon_wide
                const uint64_t f1 = kdf_rev2(e0), f0 = kdf_rev2(e1);
                const int sh = 128 - 2 * k;
                klo = (f0 >> sh) | (f1 << (64 - sh)); khi = f1 >> sh;
            }
            lo[rank] = klo; hi[rank] = khi;
        } else {
            uint64_t key[KW];
            if (canonical) roll.canon(key);
            else {
#pragma unroll
                for (int j = 0; j < KW; ++j) key[j] = roll.f[j];
            }
#pragma unroll
            for (int j = 0; j < KW; ++j) lo[rank * KW + j] = key[j];
        }
    }
}
