// kdf_fastafeed.h -- the device FASTA feeder (include/kdf.h, "device FASTA feeder"): the raw text of a (multi-)FASTA in
// HBM -> the packed 2-bit stream, its invalid mask and the record offsets, by the per-byte rule of the header.  A
// stream compaction over tiles of KDF_FASTA_TILE_BYTES = 256 lanes x 16 bytes:
//   1. kfa_count_kernel  a tile's summary.  What a byte emits depends on the first byte of its line and on whether a
//                        header has been seen, and both may lie before the tile, so the tile counts three ways:
//                        A  bytes before its first line start (emitted iff the carried-in line is no header line and a
//                           record is open), B  bytes of sequence lines before its first header start (iff a record is
//                           open), C  everything behind its first header start (always; the separators of the later
//                           header starts included).  Plus the header starts, whether the first one owes a separator (S),
//                           whether the tile has a line start and whether the last one starts a header.
//   2. kfa_scan_kernel   one workgroup: resolves the carried line state (the nearest tile to the left with a line start)
//                        and record state (any header start to the left, or the incoming state) of every tile, turns
//                        the summaries into counts, scans them, and writes the totals, `consumed` and the outgoing
//                        state.  It also refuses: a stream beyond cap_bases / cap_reads, no progress.
//   3. kfa_zero_kernel   zeroes the kdf_stream_words(n_bases) words (the write pass ORs its edge words)
//   4. kfa_write_kernel  classifies again with the carried state known, scans the lanes' counts on DPP, ORs codes and
//                        invalid bits into LDS at (first position mod 64) + rank -- so LDS words ARE output words --
//                        and stores them coalesced: a word the tile owns whole with a plain store, the two partial
//                        words at its edges with a vector atomic OR.  Record offsets go to their rank.
//   5. kfa_tail_kernel   the carry (the last c positions of the previous stream, a bit-unaligned copy, ORed in), the
//                        closing separator, the mask ones from n_bases to the end of its words, offsets [0] and [n_reads].
// 3 .. 5 read the scan's verdict from the control words and do nothing after a refusal, so the host synchronises once.
// A '\r' is dropped iff only '\r' lie between it and the next '\n' or the text's end: inside a lane a backward walk,
// across lanes the nearest lane to the right with another byte (a ballot), across tiles a walk in global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kdf.h"
#include "kdf_scan.h"
#include "kdf_text.h"

#define KFA_TILE KDF_FASTA_TILE_BYTES
static_assert(KFA_TILE == 256 * 16, "a tile is 256 lanes of 16 bytes");
#define KFA_PW ((KFA_TILE + 64) / 32)          // packed / mask words of a tile's LDS image: its positions behind up to 63 of the
#define KFA_MW ((KFA_TILE + 64) / 64 + 1)      // word they start in
// control words: [0] n_bases [1] n_reads [2] consumed [3] outgoing flags | KFA_ERR_* << 8 | closing separator << 16
#define KFA_CTL_WORDS 4
enum { KFA_ERR_ROOM = 1, KFA_ERR_STUCK = 2 };
// a tile's summary
#define KFA_F 13                               // bits of a count field (<= 4096)
#define KFA_SUM_SEP (1ull << 52)               // its first header start owes a separator if a record is open
#define KFA_SUM_LS (1ull << 53)                // it has a line start ...
#define KFA_SUM_LHDR (1ull << 54)              // ... and the last one starts a header
// a tile's carried-in state, in the top bits of its first record rank
#define KFA_IN_HDR (1ull << 62)
#define KFA_IN_REC (1ull << 63)

struct KfaText { const uint8_t *t; uint64_t n; uint32_t flags; int aligned; };

// only '\r' between byte p and the next '\n' or the text's end
__device__ __forceinline__ uint32_t kfa_walk(const KfaText &x, uint64_t p) {
    while (p < x.n && x.t[p] == '\r') ++p;
    return p >= x.n || x.t[p] == '\n';
}

// What a lane knows of its 16 bytes, one bit per byte.  lh / ir: the line state (1: a header line) and the record state
// (1: a header has been seen) in front of the lane's first byte; 2: not known inside the tile.
struct KfaLane {
    uint32_t w[4];
    uint32_t ls, hs, cand;                     // line starts, header starts, bytes that are a position on a sequence line in a record
    uint32_t lh, ir;
    uint32_t tile_ls, tile_lhdr;               // thread 0 only: the tile has a line start, its last one starts a header
};

// LDS of the classification: per wave, [0] another byte than '\r' [1] the first such is '\n' [2] a line start [3] the
// last one starts a header [4] a header start
struct KfaShared { uint32_t wv[4][5]; };

__device__ __forceinline__ void kfa_classify(const KfaText &x, uint64_t t0, KfaShared &sh, KfaLane &L) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t s0 = t0 + 16u * tid;
    const uint4 v = kt_load_granule(x.t, (int64_t)s0, 0, (int64_t)x.n, x.aligned, 0u);
    L.w[0] = v.x; L.w[1] = v.y; L.w[2] = v.z; L.w[3] = v.w;
    uint32_t prev = __shfl_up(L.w[3] >> 24, 1);                       // the byte in front of the lane
    if (lane == 0) prev = s0 == 0 ? ((x.flags & KDF_FA_MID_LINE) ? 0u : '\n') : (s0 <= x.n ? x.t[s0 - 1] : 0u);
    uint32_t live = 0, nl = 0, cr = 0, gt = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t c = (L.w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        live |= (uint32_t)(s0 + i < x.n) << i;
        nl |= (uint32_t)(c == '\n') << i;
        cr |= (uint32_t)(c == '\r') << i;
        gt |= (uint32_t)(c == '>') << i;
    }
    nl &= live; cr &= live;
    L.ls = ((nl << 1) | (uint32_t)(prev == '\n')) & live;
    L.hs = L.ls & gt;
    const uint32_t other = live & ~cr;                                 // not '\r'
    const bool has_other = other != 0, first_nl = has_other && ((nl >> (__ffs(other) - 1)) & 1u);
    const bool has_ls = L.ls != 0, last_hdr = has_ls && ((L.hs >> (31 - __clz(L.ls))) & 1u);
    const uint64_t b_other = __ballot(has_other), b_nl = __ballot(first_nl);
    const uint64_t b_ls = __ballot(has_ls), b_lhdr = __ballot(last_hdr), b_hs = __ballot(L.hs != 0);
    if (lane == 0) {
        sh.wv[wave][0] = b_other != 0; sh.wv[wave][1] = b_other ? (uint32_t)(b_nl >> (__ffsll((unsigned long long)b_other) - 1)) & 1u : 0u;
        sh.wv[wave][2] = b_ls != 0;    sh.wv[wave][3] = b_ls ? (uint32_t)(b_lhdr >> (63 - __clzll((long long)b_ls))) & 1u : 0u;
        sh.wv[wave][4] = b_hs != 0;
    }
    __syncthreads();
    // the '\r' behind the lane's last other byte: dropped iff the next other byte of the text is '\n' (or there is none)
    uint32_t drop = 2;
    const uint64_t right = lane == 63 ? 0 : b_other & (~0ull << (lane + 1)), left = (1ull << lane) - 1;
    if (right) drop = (uint32_t)(b_nl >> (__ffsll((unsigned long long)right) - 1)) & 1u;
    for (uint32_t j = wave + 1; j < 4 && drop == 2; ++j)
        if (sh.wv[j][0]) drop = sh.wv[j][1];
    if (drop == 2) drop = cr > other ? kfa_walk(x, t0 + KFA_TILE) : 0u;   // (cr > other: the lane ends in '\r')
    uint32_t dropped = 0;
#pragma unroll
    for (int i = 15; i >= 0; --i) {
        if ((other >> i) & 1u) drop = (nl >> i) & 1u;
        else dropped |= (drop & (cr >> i) & 1u) << i;
    }
    L.cand = live & ~nl & ~dropped;
    L.lh = (b_ls & left) ? (uint32_t)(b_lhdr >> (63 - __clzll((long long)(b_ls & left)))) & 1u : 2u;
    L.ir = (b_hs & left) ? 1u : 2u;
    for (int j = (int)wave - 1; j >= 0 && L.lh == 2; --j)
        if (sh.wv[j][2]) L.lh = sh.wv[j][3];
    for (int j = (int)wave - 1; j >= 0 && L.ir == 2; --j)
        if (sh.wv[j][4]) L.ir = 1;
    L.tile_ls = 0; L.tile_lhdr = 0;
    if (tid == 0)
        for (int j = 3; j >= 0 && !L.tile_ls; --j)
            if (sh.wv[j][2]) { L.tile_ls = 1; L.tile_lhdr = sh.wv[j][3]; }
}

// The lane's bytes by what decides whether they emit a position: mc always, ma iff the carried-in line is no header line
// and a record is open, mb iff a record is open, ms (a header start's separator) iff a record is open.  With lh and ir
// known (0 / 1) only mc is filled.
__device__ __forceinline__ void kfa_emit_masks(const KfaLane &L, uint32_t &ma, uint32_t &mb, uint32_t &mc, uint32_t &ms) {
    uint32_t lh = L.lh, ir = L.ir;
    ma = mb = mc = ms = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t bit = 1u << i;
        if (L.ls & bit) lh = (L.hs >> i) & 1u;
        if (L.hs & bit) {
            if (ir == 1) mc |= bit; else if (ir == 2) ms |= bit;
            ir = 1;
        } else if (L.cand & bit) {
            if (lh == 2) ma |= bit;
            else if (lh == 0) { if (ir == 1) mc |= bit; else if (ir == 2) mb |= bit; }
        }
    }
}

__global__ __launch_bounds__(256) void kfa_count_kernel(const uint8_t *__restrict__ t, uint64_t n, uint32_t flags, int aligned,
                                                        unsigned long long *__restrict__ sums) {
    __shared__ KfaShared sh;
    __shared__ unsigned long long wsum[4];
    const KfaText x{t, n, flags, aligned};
    KfaLane L;
    kfa_classify(x, (uint64_t)blockIdx.x * KFA_TILE, sh, L);
    uint32_t ma, mb, mc, ms;
    kfa_emit_masks(L, ma, mb, mc, ms);
    unsigned long long v = (unsigned long long)__popc(ma) | (unsigned long long)__popc(mb) << KFA_F | (unsigned long long)__popc(mc) << (2 * KFA_F) |
                           (unsigned long long)__popc(L.hs) << (3 * KFA_F) | (ms ? KFA_SUM_SEP : 0ull);
    v = kb_block_sum(v, wsum);
    if (threadIdx.x == 0) sums[blockIdx.x] = v + (L.tile_ls ? KFA_SUM_LS : 0ull) + (L.tile_lhdr ? KFA_SUM_LHDR : 0ull);
}

// positions a tile emits, given its carried-in states
__device__ __forceinline__ uint32_t kfa_tile_positions(unsigned long long s, bool in_hdr, bool in_rec) {
    const uint32_t a = (uint32_t)s & ((1u << KFA_F) - 1), b = (uint32_t)(s >> KFA_F) & ((1u << KFA_F) - 1), c = (uint32_t)(s >> (2 * KFA_F)) & ((1u << KFA_F) - 1);
    return c + (in_rec ? b + ((s & KFA_SUM_SEP) ? 1u : 0u) + (in_hdr ? 0u : a) : 0u);
}
__device__ __forceinline__ uint32_t kfa_tile_records(unsigned long long s) { return (uint32_t)(s >> (3 * KFA_F)) & ((1u << KFA_F) - 1); }

// One workgroup of 256; thread i owns the tiles [i * per, (i + 1) * per).  c: the carry's positions; cap_reads: ~0 when no
// offsets are asked for.  tile_pos[t]: the stream position of tile t's first; tile_rec[t]: the rank of its first header
// start | KFA_IN_HDR | KFA_IN_REC.
__global__ __launch_bounds__(256) void kfa_scan_kernel(const unsigned long long *__restrict__ sums, uint64_t nt, const uint8_t *__restrict__ t, uint64_t n,
                                                       int final_chunk, uint32_t flags, uint64_t c, uint64_t cap_bases, uint64_t cap_reads,
                                                       unsigned long long *__restrict__ tile_pos, unsigned long long *__restrict__ tile_rec,
                                                       unsigned long long *__restrict__ ctl) {
    __shared__ uint32_t ws[17];
    __shared__ uint32_t line_of[256];                                  // 0: the thread's tiles have no line start; 1 / 2: the last one starts a sequence / header line
    __shared__ uint32_t end_hdr;
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (nt + 255) / 256, b = min(nt, tid * per), e = min(nt, b + per);
    if (tid == 0) end_hdr = (flags & KDF_FA_IN_HEADER) != 0;           // (published by the barriers of the scans below)
    // consumed: everything (the last chunk), else everything in front of the trailing run of '\r'
    const uint64_t m = final_chunk ? n : kt_last_outside(t, n, [](uint8_t c) { return c == '\r'; });
    uint32_t my_line = 0, my_hs = 0;
    for (uint64_t i = b; i < e; ++i) {
        const unsigned long long s = sums[i];
        if (s & KFA_SUM_LS) my_line = (s & KFA_SUM_LHDR) ? 2 : 1;
        my_hs |= kfa_tile_records(s) != 0;
    }
    line_of[tid] = my_line;
    uint32_t any;
    const uint32_t hs_before = kb_block_exscan(my_hs, ws, &any);      // (its barriers publish line_of)
    bool in_rec = (flags & KDF_FA_IN_RECORD) || hs_before, in_hdr = (flags & KDF_FA_IN_HEADER) != 0;
    for (int j = (int)tid - 1; j >= 0; --j)
        if (line_of[j]) { in_hdr = line_of[j] == 2; break; }
    const bool in_rec0 = in_rec, in_hdr0 = in_hdr;
    uint32_t pos = 0, rec = 0;
    for (uint64_t i = b; i < e; ++i) {
        const unsigned long long s = sums[i];
        pos += kfa_tile_positions(s, in_hdr, in_rec);
        rec += kfa_tile_records(s);
        in_rec |= kfa_tile_records(s) != 0;
        if (s & KFA_SUM_LS) in_hdr = (s & KFA_SUM_LHDR) != 0;
    }
    if (e == nt && b < e) end_hdr = in_hdr;                            // the thread of the last tile
    uint32_t n_pos, n_rec;
    uint64_t p = c + kb_block_exscan(pos, ws, &n_pos);
    uint64_t r = ((flags & KDF_FA_IN_RECORD) ? 1 : 0) + kb_block_exscan(rec, ws, &n_rec);
    in_rec = in_rec0; in_hdr = in_hdr0;
    for (uint64_t i = b; i < e; ++i) {
        const unsigned long long s = sums[i];
        tile_pos[i] = p;
        tile_rec[i] = r | (in_hdr ? KFA_IN_HDR : 0ull) | (in_rec ? KFA_IN_REC : 0ull);
        p += kfa_tile_positions(s, in_hdr, in_rec);
        r += kfa_tile_records(s);
        in_rec |= kfa_tile_records(s) != 0;
        if (s & KFA_SUM_LS) in_hdr = (s & KFA_SUM_LHDR) != 0;
    }
    if (tid == 0) {
        const bool open = (flags & KDF_FA_IN_RECORD) || n_rec;
        const uint64_t closing = final_chunk && open ? 1 : 0;
        const uint64_t n_bases = c + n_pos + closing, n_reads = ((flags & KDF_FA_IN_RECORD) ? 1 : 0) + (uint64_t)n_rec;
        uint32_t out = 0, err = 0;
        if (!final_chunk) {
            const bool mid = m ? t[m - 1] != '\n' : (flags & KDF_FA_MID_LINE) != 0;
            out = (open ? KDF_FA_IN_RECORD : 0u) | (mid ? KDF_FA_MID_LINE : 0u) | (mid && end_hdr ? KDF_FA_IN_HEADER : 0u);
        }
        if (n_bases > cap_bases || n_reads > cap_reads) err = KFA_ERR_ROOM;
        else if (n && !final_chunk && !m) err = KFA_ERR_STUCK;
        ctl[0] = n_bases; ctl[1] = n_reads; ctl[2] = m;
        ctl[3] = out | err << 8 | (uint32_t)closing << 16;
    }
}

__device__ __forceinline__ bool kfa_refused(const unsigned long long *ctl) { return ((ctl[3] >> 8) & 0xFFu) != 0; }

__global__ __launch_bounds__(256) void kfa_zero_kernel(const unsigned long long *__restrict__ ctl, uint64_t *__restrict__ packed, uint64_t *__restrict__ invalid) {
    if (kfa_refused(ctl)) return;
    const uint64_t T = (ctl[0] + 63) / 64, pw = 2 * T + 4, mw = T + 2;      // kdf_stream_words(n_bases)
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < pw; i += (uint64_t)gridDim.x * 256) {
        packed[i] = 0;
        if (i < mw) invalid[i] = 0;
    }
}

__global__ __launch_bounds__(256) void kfa_write_kernel(const uint8_t *__restrict__ t, uint64_t n, uint32_t flags, int aligned,
                                                        const unsigned long long *__restrict__ tile_pos, const unsigned long long *__restrict__ tile_rec,
                                                        const unsigned long long *__restrict__ ctl, uint64_t *__restrict__ packed,
                                                        uint64_t *__restrict__ invalid, int64_t *__restrict__ offsets) {
    __shared__ KfaShared sh;
    __shared__ uint32_t ws[17];
    __shared__ unsigned long long lp[KFA_PW], lm[KFA_MW];
    if (kfa_refused(ctl)) return;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < KFA_PW; i += 256) lp[i] = 0;
    if (tid < KFA_MW) lm[tid] = 0;
    const KfaText x{t, n, flags, aligned};
    KfaLane L;
    kfa_classify(x, (uint64_t)blockIdx.x * KFA_TILE, sh, L);           // (its barrier publishes the zeroes)
    const unsigned long long tr = tile_rec[blockIdx.x];
    const uint64_t g0 = tile_pos[blockIdx.x], r0 = tr & ~(KFA_IN_HDR | KFA_IN_REC);
    if (L.lh == 2) L.lh = (tr & KFA_IN_HDR) ? 1 : 0;
    if (L.ir == 2) L.ir = (tr & KFA_IN_REC) ? 1 : 0;
    uint32_t ma, mb, emit, ms;
    kfa_emit_masks(L, ma, mb, emit, ms);
    const uint32_t cnt = (uint32_t)__popc(emit), nhs = (uint32_t)__popc(L.hs);
    uint32_t total;
    const uint32_t ex = kb_block_exscan(cnt | nhs << 16, ws, &total);  // (a tile emits <= 4096 positions and has <= 2049 header starts)
    const uint32_t lpos = ex & 0xFFFFu, tot = total & 0xFFFFu, first = (uint32_t)(g0 & 63);
    if (cnt) {
        uint64_t codes = 0, inv = 0;
        uint32_t j = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (!((emit >> i) & 1u)) continue;
            const uint32_t code = kdf_base_code((L.w[i >> 2] >> (8 * (i & 3))) & 0xFFu);   // ('>': a separator is an invalid position)
            codes |= (uint64_t)(code & 3u) << (2 * j);
            inv |= (uint64_t)(code > 3) << j;
            ++j;
        }
        const uint32_t q = first + lpos, ps = (2 * q) & 63, qs = q & 63;
        atomicOr(&lp[(2 * q) >> 6], (unsigned long long)(codes << ps));
        if (ps + 2 * cnt > 64) atomicOr(&lp[((2 * q) >> 6) + 1], (unsigned long long)(codes >> (64 - ps)));
        atomicOr(&lm[q >> 6], (unsigned long long)(inv << qs));
        if (qs + cnt > 64) atomicOr(&lm[(q >> 6) + 1], (unsigned long long)(inv >> (64 - qs)));
    }
    if (offsets && nhs) {                                              // a record starts behind the separator its '>' emits
        uint64_t rank = r0 + (ex >> 16);
        for (uint32_t hs = L.hs; hs; hs &= hs - 1, ++rank) {
            const uint32_t bit = hs & (0u - hs);
            offsets[rank] = (int64_t)(g0 + lpos + (uint32_t)__popc(emit & (bit - 1)) + ((emit & bit) ? 1u : 0u));
        }
    }
    __syncthreads();
    if (!tot) return;
    // LDS word j is output word (g0 / 64) * 2 + j (packed: positions base + 32 j ..) or g0 / 64 + j (mask)
    const uint64_t base = g0 - first, end = g0 + tot;
    const uint32_t npw = (first + tot + 31) / 32, nmw = (first + tot + 63) / 64;
    for (uint32_t j = tid; j < npw; j += 256) {
        const uint64_t p0 = base + 32ull * j;
        const unsigned long long v = lp[j];
        uint64_t *dst = packed + (base >> 5) + j;
        if (p0 >= g0 && p0 + 32 <= end) *dst = v;
        else if (v) atomicOr((unsigned long long *)dst, v);
    }
    for (uint32_t j = tid; j < nmw; j += 256) {
        const uint64_t p0 = base + 64ull * j;
        const unsigned long long v = lm[j];
        uint64_t *dst = invalid + (base >> 6) + j;
        if (p0 >= g0 && p0 + 64 <= end) *dst = v;
        else if (v) atomicOr((unsigned long long *)dst, v);
    }
}

// nbits bits of src from bit sb on -> ORed into dst from bit 0 on (src has a word behind the last one read: the padding
// words of kdf_stream_words)
__device__ __forceinline__ void kfa_copy_bits(uint64_t *dst, const uint64_t *src, uint64_t sb, uint64_t nbits) {
    const uint32_t s = (uint32_t)(sb & 63);
    for (uint64_t j = threadIdx.x; j * 64 < nbits; j += 256) {
        const uint64_t sw = (sb >> 6) + j, rem = nbits - j * 64;
        unsigned long long v = src[sw] >> s;
        if (s) v |= (unsigned long long)src[sw + 1] << (64 - s);
        if (rem < 64) v &= (1ull << rem) - 1;
        if (v) atomicOr((unsigned long long *)dst + j, v);
    }
}

// one workgroup, behind the write pass
__global__ __launch_bounds__(256) void kfa_tail_kernel(const unsigned long long *__restrict__ ctl, const uint64_t *__restrict__ prev_packed,
                                                       const uint64_t *__restrict__ prev_invalid, uint64_t prev_n, uint64_t c,
                                                       uint64_t *__restrict__ packed, uint64_t *__restrict__ invalid, int64_t *__restrict__ offsets) {
    if (kfa_refused(ctl)) return;
    const uint64_t n_bases = ctl[0], n_reads = ctl[1], closing = (ctl[3] >> 16) & 1u;
    if (c) {
        kfa_copy_bits(packed, prev_packed, 2 * (prev_n - c), 2 * c);
        kfa_copy_bits(invalid, prev_invalid, prev_n - c, c);
    }
    const uint64_t from = n_bases - closing, mw = (n_bases + 63) / 64 + 2;      // invalid from here to the end of the mask words
    if (threadIdx.x == 0 && (from & 63)) atomicOr((unsigned long long *)invalid + (from >> 6), ~0ull << (from & 63));
    for (uint64_t i = (from + 63) / 64 + threadIdx.x; i < mw; i += 256) invalid[i] = ~0ull;
    if (offsets && threadIdx.x == 0) { offsets[0] = 0; offsets[n_reads] = (int64_t)n_bases; }
}
