// kdf_depth.h -- the count profile along a read stream: per-window counts (kdf_window_counts*, `jellyfish query -s`)
// and their per-read summary (kdf_read_depth*).  One kernel template for every key width W = 1 .. 7 words; it only
// READS the table.
//
// Layout: LANE PER WINDOW.  The scan kernels give a thread a tile of 64 window starts because they keep one bit per
// window; a count per window from that layout would be a 256-byte-strided store per lane.  Here a wave owns
// KD_WAVE_TILES consecutive tiles and lane l takes window l of each of them, so
//   - the 64 counts of a tile leave as ONE 256-byte store of the wave, and its validity word as one ballot,
//   - the NB home-slot loads of NB consecutive tiles are issued back to back before any is resolved (the scan's eight
//     loads in flight per lane, turned by 90 degrees),
//   - everything that concerns reads is wave-uniform: which read a tile's windows belong to is decided on the
//     validity ballot with scalar loads of the offsets, and no lane carries per-read state.
// A lane cuts its window straight out of the packed stream (W + 1 word loads, two distinct addresses per wave: they
// coalesce to two requests) and tests its own k mask bits; positions at or past n_bases are invalid whatever the
// buffers hold because a window is valid only if p + k <= n_bases, and every load is clamped to the
// kdf_stream_words(n_bases) words of its buffer.
//
// Per-read reduction (DEPTH).  The wave accumulates the read it is in: windows / present / low as popcounts of
// ballots (scalar), sum / min / max in lane-private registers.  When the read changes, and at the end of the wave's
// tiles, the lane values are reduced across the wave and lanes 0..5 each send one 64-bit atomic to the row (add,
// add, add, max of ~min, max, add).  A 150-base read is flushed about once per tile it touches; a contig of any
// length once per wave (4096 positions), so long sequences do not pile atomics onto one row.  Rows are zeroed by the
// call and column `min` is turned back (and set to 0 for reads without windows) by kd_rows_fix_kernel.  All integer:
// the result does not depend on scheduling.
#pragma once
#include "kdf_device.h"
#include "kdf_long.h"

#define KD_WAVE_TILES 64                  // tiles per wave: 4096 stream positions
// (KD_ROW_WORDS = 6 -- windows, present, low, min, max, sum -- is in kdf_device.h: a spool's replay strides by it)

template <int W> struct KdCfg { static constexpr int NB = W <= 3 ? 8 : 4; };      // tiles resolved together (long keys: registers)

// no invalid position in [p, p + k) and the window ends inside the stream; mw = mask words of the stream buffer
template <int W>
__device__ __forceinline__ bool kd_window_valid(const uint64_t *__restrict__ invalid, uint64_t mw, uint64_t p, int k, uint64_t n_bases) {
    if (p + (uint64_t)k > n_bases) return false;
    constexpr int NCH = (W + 1) / 2;                                 // 64-position chunks of a window: k <= 32 W
    const uint64_t q = p >> 6;
    const int lo = (int)(p & 63);
    uint64_t bad = 0, m = q < mw ? invalid[q] : ~0ull;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int left = k - 64 * j;                                 // positions of the window from chunk j on
        if (left <= 0) break;
        const uint64_t m1 = q + j + 1 < mw ? invalid[q + j + 1] : ~0ull;
        const uint64_t chunk = kdf_funnel(m, m1, lo);                // mask bits of window positions [64 j, 64 j + 64)
        bad |= left >= 64 ? chunk : (chunk & ((1ull << left) - 1));
        m = m1;
    }
    return bad == 0;
}

// canonical key of the k-base window at stream position p: W words, word 0 least significant (kdf_canon_narrow /
// kdf_canon_wide / KdfRoll::canon give the same words); pw = packed words of the stream buffer
template <int W>
__device__ __forceinline__ void kd_window_key(const uint64_t *__restrict__ packed, uint64_t pw, uint64_t p, int k, uint64_t (&key)[W]) {
    const uint64_t q = p >> 5;
    const int sh = (int)(p & 31) * 2;
    const int tb = 2 * k - 64 * (W - 1);                            // bits of the top word, 2 .. 64
    const uint64_t tmask = tb >= 64 ? ~0ull : ((1ull << tb) - 1);
    uint64_t e[W], g[W];                                            // e: base j of the window in bits 2j
    uint64_t x = q < pw ? packed[q] : 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const uint64_t x1 = q + j + 1 < pw ? packed[q + j + 1] : 0;
        e[j] = kdf_funnel(x, x1, sh);
        x = x1;
    }
    e[W - 1] &= tmask;
    // forward code: the 2-bit groups of the whole value reversed, shifted down to 2k bits
#pragma unroll
    for (int j = 0; j < W; ++j) g[j] = kdf_rev2(e[W - 1 - j]);
    const int s = 64 - tb;                                          // 0 .. 62
    uint64_t f[W];
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] = j == W - 1 ? g[j] >> s : kdf_funnel(g[j], g[j + 1], s);
    bool lt = false, decided = false;                               // canonical = the smaller of the two, compared from the top word down
#pragma unroll
    for (int j = W - 1; j >= 0; --j) {
        const uint64_t r = j == W - 1 ? (~e[j] & tmask) : ~e[j];    // reverse complement
        if (!decided && f[j] != r) { lt = f[j] < r; decided = true; }
        key[j] = r;
    }
#pragma unroll
    for (int j = 0; j < W; ++j) key[j] = lt ? f[j] : key[j];
}

template <int W>
__device__ __forceinline__ uint64_t kd_hash(const uint64_t (&key)[W]) {
    if constexpr (W == 1) return kdf_hash(key[0], 0);
    else if constexpr (W == 2) return kdf_hash(key[0], key[1]);
    else return kdf_long_hash<W>(key);
}
// the word of a slot that tells it is empty: lo (narrow), hi (wide), the top word (long)
template <int W>
__device__ __forceinline__ const uint64_t *kd_occ_word(const KdfTable &t, uint64_t slot) {
    if constexpr (W == 1) return t.lo + slot;
    else if constexpr (W == 2) return t.hi + slot;
    else return kdf_long_word<W>(t, W - 1, slot);
}
template <int W>
__device__ __forceinline__ uint32_t kd_count_of(const KdfTable &t, uint64_t h, const uint64_t (&key)[W]) {
    uint64_t s;
    if constexpr (W == 1) s = kdf_find_narrow(t, h);
    else if constexpr (W == 2) s = kdf_find_wide(t, h, key[1]);
    else s = kdf_find_long<W>(t, h, key);
    return s == ~0ull ? 0u : t.cnt[s];
}

// DEPTH = false: counts_out[p] for every p < n_bases, valid_out[tile] (may be NULL).
// DEPTH = true:  rows[r * 6 ..] += the windows of read r (offs[n_reads + 1]); n_reads >= 1.
// Grid: one wave per KD_WAVE_TILES tiles, 4 waves per workgroup.
template <int W, bool DEPTH>
__global__ __launch_bounds__(256) void kdf_depth_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_bases, int k, KdfTable t,
    uint32_t *__restrict__ counts_out, unsigned long long *__restrict__ valid_out,
    const int64_t *__restrict__ offs, int64_t n_reads, uint32_t low_max, unsigned long long *__restrict__ rows)
{
    constexpr int NB = KdCfg<W>::NB;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (uint64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const KdfStreamGeom g = kdf_stream_geom(n_bases);
    const uint64_t T = g.tiles, pw = g.packed_words, mw = g.mask_words;
    const uint64_t tile_begin = wave * KD_WAVE_TILES;
    const uint64_t tile_end = tile_begin + KD_WAVE_TILES < T ? tile_begin + KD_WAVE_TILES : T;
    if (tile_begin >= tile_end) return;

    // ---- DEPTH: the read the wave is in (wave-uniform) and what it has gathered for it
    int64_t r = 0, beg = 0, end = 0, off0 = 0, offN = 0;
    bool have = false;
    uint32_t a_windows = 0, a_present = 0, a_low = 0;               // uniform
    uint64_t a_sum = 0; uint32_t a_min = 0xFFFFFFFFu, a_max = 0;    // per lane
    if constexpr (DEPTH) { off0 = offs[0]; offN = offs[n_reads]; }
    auto flush = [&]() {
        if (a_windows == 0) return;
        uint64_t sm = a_sum; uint32_t mn = a_min, mx = a_max;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sm += __shfl_xor(sm, o);
            const uint32_t mn2 = __shfl_xor(mn, o), mx2 = __shfl_xor(mx, o);
            mn = mn2 < mn ? mn2 : mn; mx = mx2 > mx ? mx2 : mx;
        }
        if (lane < KD_ROW_WORDS) {
            unsigned long long *cell = rows + (uint64_t)r * KD_ROW_WORDS + lane;       // 0 <= r < n_reads
            const unsigned long long v = lane == 0 ? a_windows : lane == 1 ? a_present : lane == 2 ? a_low
                                       : lane == 3 ? ~(unsigned long long)mn : lane == 4 ? mx : sm;
            if (lane == 3 || lane == 4) atomicMax(cell, v); else atomicAdd(cell, v);
        }
        a_windows = a_present = a_low = 0; a_sum = 0; a_min = 0xFFFFFFFFu; a_max = 0;
    };
    // the read that holds position p, off0 <= p < offN: r with offs[r] <= p < offs[r + 1].  A few steps forward from the
    // current read (the next window nearly always lies in the next read), else a binary search.  Whatever the offsets
    // hold, 0 <= r < n_reads.
    auto locate = [&](int64_t p) {
        int64_t a = offs[r] <= p ? r : 0;
        for (int s = 0; s < 4 && a + 1 < n_reads && offs[a + 1] <= p; ++s) ++a;
        if (a + 1 < n_reads && offs[a + 1] <= p) {
            int64_t lo = a + 1, hi = n_reads - 1;
            while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (offs[mid] <= p) lo = mid; else hi = mid - 1; }
            a = lo;
        }
        r = a;
    };

    for (uint64_t tb0 = tile_begin; tb0 < tile_end; tb0 += NB) {
        uint64_t key[NB][W], h[NB], pre[NB];
        bool ok[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const uint64_t p = (tb0 + u) * KDF_TILE + lane;
            ok[u] = tb0 + u < tile_end && kd_window_valid<W>(invalid, mw, p, k, n_bases);
            h[u] = 0;
            if (ok[u]) { kd_window_key<W>(packed, pw, p, k, key[u]); h[u] = kd_hash<W>(key[u]); }
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) pre[u] = ok[u] ? *kd_occ_word<W>(t, kdf_home(t, h[u])) : KDF_EMPTY;
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const uint64_t tile = tb0 + u;
            if (tile >= tile_end) break;                             // (wave-uniform)
            uint32_t c = 0;
            if (ok[u] && pre[u] != KDF_EMPTY) c = kd_count_of<W>(t, h[u], key[u]);
            const unsigned long long vb = __ballot(ok[u]);
            if constexpr (!DEPTH) {
                const uint64_t p = tile * KDF_TILE + lane;
                if (p < n_bases) counts_out[p] = c;
                if (valid_out && lane == 0) valid_out[tile] = vb;
            } else {
                const unsigned long long pres = __ballot(ok[u] && c != 0), lowm = __ballot(ok[u] && c <= low_max);
                const int64_t tp = (int64_t)(tile * KDF_TILE);
                unsigned long long rem = vb;
                while (rem) {                                        // one turn per read that has windows in this tile
                    const int fb = __builtin_ctzll(rem);
                    const int64_t p = tp + fb;
                    if (!(have && p >= beg && p < end)) {
                        flush();
                        have = false;
                        if (p >= offN) break;                        // past the last read: so is the rest of the tile
                        if (p < off0) { const int64_t d = off0 - tp; rem &= d >= 64 ? 0ull : ~0ull << d; continue; }    // before the first read (d > fb)
                        locate(p);
                        beg = offs[r]; end = offs[r + 1];
                        if (!(p >= beg && p < end)) { rem &= rem - 1; continue; }     // (offsets that break the precondition)
                        have = true;
                    }
                    const int64_t d = end - tp;                      // > fb
                    const unsigned long long seg = rem & (d >= 64 ? ~0ull : ((1ull << d) - 1));
                    a_windows += (uint32_t)__popcll(seg); a_present += (uint32_t)__popcll(seg & pres); a_low += (uint32_t)__popcll(seg & lowm);
                    if ((seg >> lane) & 1) { a_sum += c; a_min = c < a_min ? c : a_min; a_max = c > a_max ? c : a_max; }
                    rem &= ~seg;
                }
            }
        }
    }
    if constexpr (DEPTH) flush();
}

// column `min` was gathered as max(~count) over rows zeroed by the call: turn it back; 0 for a read without windows
__global__ __launch_bounds__(256) void kd_rows_fix_kernel(unsigned long long *__restrict__ rows, int64_t n_reads) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    unsigned long long *row = rows + (uint64_t)i * KD_ROW_WORDS;
    row[3] = row[0] ? ~row[3] : 0ull;
}
