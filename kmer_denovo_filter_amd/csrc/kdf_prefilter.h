// kdf_prefilter.h -- the counting sieve of the two-pass count (include/kdf.h, "two-pass counting").
//
// Pass 1 (TALLY) walks the read stream tile by tile (kdf_tilewalk.h) and bumps one saturating cell per valid
// window; pass 2 (GATE) walks the stream the count is about to take and writes, per tile of 64 window starts, one
// 64-bit "admitted" word (bit i: window i is valid and its cell reads >= min_count) which the count kernels AND into
// their validity bitmap.  The sieve is immutable between kdf_prefilter_arm and kdf_prefilter_drop, so the gate may run
// whenever the windows are formed: per call on the direct path, at partition time for the pending stream.
//
// Cells.  2^s cells, 16 <= s <= 38; cell(key) = h >> (64 - s), h the key's 64-bit stored form / hash (kdf_mix64(key),
// kdf_hash(lo, hi), kdf_long_hash(words)): the TOP bits, so a table bucket owns a contiguous range of cells.
// A cell is one nibble: HALF A BYTE per cell, sixteen cells per 64-bit word, cell c in bits [4 (c & 15), +4) of word
// c >> 4.  Bits 0..2 of the nibble are three planes A, B, C; bit 3 is unused.  A sighting sets the lowest plane that is
// not yet set, with a ladder of RETURNING atomic ORs: OR in A; if A was already set OR in B; if B was already set OR in
// C.  Whatever the order and the concurrency of the sightings, after n of them min(n, 3) planes are set: the first
// OR to reach a plane sets it, every other one moves on.  value(cell) = number of planes set = min(sightings, 3).
// No compare-and-swap loop, and no lane ever waits for another lane.  The word is LOADED first and the atomics are
// skipped when the cell already reads 3: in a 15-30x sample that is most windows, and it keeps a homopolymer key
// with 10^6 sightings from hammering one word (a stale read only costs atomics that change nothing).
#pragma once
#include "kdf_device.h"
#include "kdf_long.h"

#define KDF_PF_MIN_LOG2 16
#define KDF_PF_MAX_LOG2 38

// (struct KdfPrefilter -- words, log2_cells, min_count -- is in kdf_device.h: the engine holds one by value)

__device__ __forceinline__ void kdf_pf_locate(const KdfPrefilter &pf, uint64_t h, uint64_t &word, uint32_t &sh) {
    const uint64_t cell = h >> (64 - pf.log2_cells);
    word = cell >> 4;
    sh = (uint32_t)(cell & 15) * 4;
}

// one sighting of the cell at (w, sh); `cur`: the word as loaded before
__device__ __forceinline__ void kdf_pf_bump(unsigned long long *w, uint32_t sh, uint64_t cur) {
    if (((cur >> sh) & 7) == 7) return;                               // saturated: nothing left to set
    unsigned long long old = atomicOr(w, 1ull << sh);
    if (!((old >> sh) & 1)) return;                                   // this sighting set plane A
    old = atomicOr(w, 2ull << sh);
    if (!((old >> sh) & 2)) return;                                   // ... plane B
    if (!((old >> sh) & 4)) atomicOr(w, 4ull << sh);                  // ... plane C (or it is set already)
}

__device__ __forceinline__ bool kdf_pf_admits(const KdfPrefilter &pf, uint64_t cur, uint32_t sh) {
    return (uint32_t)__popc((uint32_t)(cur >> sh) & 7u) >= pf.min_count;
}

// k <= 63.  One thread = one tile of 64 window starts (kdf_walk_tile, kdf_tilewalk.h); windows are taken 8 at a time so
// that 8 sieve words are in flight per lane.  GATE = false: tally (windows: sharded counter of tallied windows).
// GATE = true: admit[tile] is written.
template <int KW, bool GATE>
__global__ __launch_bounds__(256) void kdf_pf_stream_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_bases, int k,
    KdfPrefilter pf, unsigned long long *__restrict__ windows, uint64_t *__restrict__ admit)
{
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nwin = 0;
    if (tile < n_tiles) {
        uint64_t adm = 0;
        nwin = kdf_walk_tile<KW>(packed, invalid, tile, n_bases, k, ~0ull,
            [&](int b, const uint64_t (&klo)[8], const uint64_t (&khi)[8], uint32_t vb) __attribute__((always_inline)) {
                uint64_t word[8], cur[8]; uint32_t sh[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) kdf_pf_locate(pf, kdf_hash(klo[u], khi[u]), word[u], sh[u]);
#pragma unroll
                for (int u = 0; u < 8; ++u) cur[u] = ((vb >> u) & 1) ? pf.words[word[u]] : 0ull;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (!((vb >> u) & 1)) continue;
                    if constexpr (GATE) { if (kdf_pf_admits(pf, cur[u], sh[u])) adm |= 1ull << (b + u); }
                    else kdf_pf_bump(&pf.words[word[u]], sh[u], cur[u]);
                }
            });
        if constexpr (GATE) admit[tile] = adm;
    }
    if constexpr (!GATE) kdf_shard_add(windows, nwin);
}

// long keys (odd k 65..201), 4 sieve words in flight per lane.  The kernel keeps a reader of its own, the loop of
// kdf_walk_tile_long (kdf_tilewalk.h): over the walker the k = 101 tally of 10 M x 150 bp reads measured 24.10 ms
// against 22.99 ms (profiles/tile_walk_bench.txt, second table).
template <int W, bool GATE>
__global__ __launch_bounds__(256) void kdf_pf_long_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_bases, int k,
    KdfPrefilter pf, unsigned long long *__restrict__ windows, uint64_t *__restrict__ admit)
{
    constexpr int NB = 4;
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = tile < n_tiles;
    const KdfStreamGeom g = kdf_stream_geom(n_bases);
    const uint64_t pw = g.packed_words, mw = g.mask_words;
    const int tb = 2 * k - 64 * (W - 1);
    uint32_t nwin = 0;
    uint64_t adm = 0;
    KdfRoll<W> st;
#pragma unroll
    for (int j = 0; j < W; ++j) { st.f[j] = 0; st.r[j] = 0; }
    st.run = 0;
    const uint64_t p0 = tile * KDF_TILE;
    uint64_t curw = 0, curm = ~0ull;
    int o = 0;
    auto push = [&]() {
        if ((o & 31) == 0) { const uint64_t q = 2 * tile + (o >> 5); curw = (active && q < pw) ? packed[q] : 0; }
        if ((o & 63) == 0) { const uint64_t q = tile + (o >> 6); curm = (active && q < mw) ? invalid[q] : ~0ull; }
        const bool inv = (curm & 1) || p0 + (uint64_t)o >= n_bases;
        st.push((uint32_t)(curw & 3), inv, tb);
        curw >>= 2; curm >>= 1; ++o;
    };
    for (int i = 0; i < k - 1; ++i) push();
    for (int b = 0; b < KDF_TILE; b += NB) {
        uint64_t word[NB], cur[NB]; uint32_t sh[NB];
        bool ok[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            uint64_t key[W];
            push();                                                // base o - 1 = b + u + k - 1 closes window b + u
            st.canon(key);
            ok[u] = active && st.run >= k;
            if (ok[u]) ++nwin;
            kdf_pf_locate(pf, kdf_long_hash<W>(key), word[u], sh[u]);
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) cur[u] = ok[u] ? pf.words[word[u]] : 0ull;
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            if (!ok[u]) continue;
            if constexpr (GATE) { if (kdf_pf_admits(pf, cur[u], sh[u])) adm |= 1ull << (b + u); }
            else kdf_pf_bump(&pf.words[word[u]], sh[u], cur[u]);
        }
    }
    if constexpr (GATE) { if (active) admit[tile] = adm; }
    else kdf_shard_add(windows, nwin);
}

// cells by value: out3 += {cells reading >= 1, >= 2, 3} (the planes are nested: B is only set after A, C after B)
__global__ __launch_bounds__(256) void kdf_pf_fill_kernel(const unsigned long long *__restrict__ words, uint64_t n_words,
                                                         unsigned long long *__restrict__ out3)
{
    unsigned long long a = 0, b = 0, c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long w = words[i];
        a += __popcll(w & 0x1111111111111111ull); b += __popcll(w & 0x2222222222222222ull); c += __popcll(w & 0x4444444444444444ull);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o); b += __shfl_down(b, o); c += __shfl_down(c, o); }
    if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(&out3[0], a);
        if (b) atomicAdd(&out3[1], b);
        if (c) atomicAdd(&out3[2], c);
    }
}

// ---- merge of sieves (include/kdf.h, "two-pass counting": several ranks) -----------------------------------------------------
// A cell is min(sightings, 3), so the saturating sum of the ranks' cells is the cell one engine would have tallied over
// all of their reads.  SWAR on whole words, sixteen cells at a time: the value of a nibble is the number of its planes
// A, B, C that are set (what kdf_pf_admits reads; bit 3 is ignored, a non-thermometer code such as 0b101 reads as 2),
// values are summed with a clamp at 3 after every segment (3 + 3 = 6 still fits a nibble), and the result is written
// as the code the tally writes: 0 / 1 / 3 / 7, bit 3 clear -- whatever a segment holds, no other code reaches the sieve.
#define KDF_PF_MAX_SEGS 64

struct KdfPfSegs {                        // the segments of one merge call (device pointers), by value
    const unsigned long long *seg[KDF_PF_MAX_SEGS];
    uint32_t nseg;
};

// two words at an address that is only known to be a multiple of 8 (a segment need not start where a sieve word pair does)
typedef unsigned long long kdf_pf_w2 __attribute__((ext_vector_type(2), aligned(8)));

__device__ __forceinline__ uint64_t kdf_pf_values(uint64_t w) {           // per nibble: planes set, 0..3
    const uint64_t M1 = 0x1111111111111111ull;
    return (w & M1) + ((w >> 1) & M1) + ((w >> 2) & M1);
}

__device__ __forceinline__ uint64_t kdf_pf_sat_add(uint64_t acc, uint64_t v) {   // per nibble: min(acc + v, 3), both <= 3
    const uint64_t s = acc + v;                                                  // <= 6: no carry into the next nibble
    const uint64_t g = (s >> 2) & 0x1111111111111111ull;                         // 4, 5, 6 have bit 2 set
    return (s | g | (g << 1)) & 0x3333333333333333ull;
}

__device__ __forceinline__ uint64_t kdf_pf_encode(uint64_t v) {           // per nibble: 0 / 1 / 2 / 3 -> 0 / 1 / 3 / 7
    const uint64_t M1 = 0x1111111111111111ull;
    const uint64_t b0 = v & M1, b1 = (v >> 1) & M1;
    return (b0 | b1) | (b1 << 1) | ((b0 & b1) << 2);
}

template <bool REPLACE>
__device__ __forceinline__ void kdf_pf_merge_word(unsigned long long *__restrict__ own, const KdfPfSegs &sg, uint64_t i) {
    uint64_t acc = REPLACE ? 0ull : kdf_pf_values(own[i]);
    for (uint32_t s = 0; s < sg.nseg; ++s) acc = kdf_pf_sat_add(acc, kdf_pf_values(sg.seg[s][i]));
    own[i] = kdf_pf_encode(acc);
}

// own: the engine's slice (own[i] is sieve word first_word + i), seg[s][i] the same word of segment s.  `head` (0 / 1)
// words come before the first sieve word pair, `n_pairs` pairs of 16 aligned bytes follow (one pair per lane per
// load, grid-stride), and what is left (0 / 1 word) is the tail.  No atomics, no LDS: (nseg + 1) reads and 1 write per word
// (nseg reads with REPLACE).  nseg and the pointers are uniform: scalar loads from the kernel arguments.
template <bool REPLACE>
__global__ __launch_bounds__(256) void kdf_pf_merge_kernel(unsigned long long *__restrict__ own, KdfPfSegs sg,
                                                          uint64_t n_words, uint32_t head, uint64_t n_pairs)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0 && head) kdf_pf_merge_word<REPLACE>(own, sg, 0);
    if (t == 1 && head + 2 * n_pairs < n_words) kdf_pf_merge_word<REPLACE>(own, sg, n_words - 1);
    const uint64_t M1 = 0x1111111111111111ull;
    for (uint64_t p = t; p < n_pairs; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = head + 2 * p;
        uint64_t a0 = 0, a1 = 0;
        if constexpr (!REPLACE) {
            const kdf_pf_w2 o = *(const kdf_pf_w2 *)(own + i);
            a0 = kdf_pf_values(o.x); a1 = kdf_pf_values(o.y);
        }
        uint32_t s = 0;
        for (; s + 4 <= sg.nseg; s += 4) {                         // four 16-byte loads in flight, one clamp: 3 + 4 x 3 = 15 fits a nibble
            kdf_pf_w2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *(const kdf_pf_w2 *)(sg.seg[s + u] + i);
#pragma unroll
            for (int u = 0; u < 4; ++u) { a0 += kdf_pf_values(v[u].x); a1 += kdf_pf_values(v[u].y); }
            const uint64_t g0 = ((a0 >> 2) | (a0 >> 3)) & M1, g1 = ((a1 >> 2) | (a1 >> 3)) & M1;   // >= 4: bit 2 or bit 3
            a0 = (a0 | g0 | (g0 << 1)) & 0x3333333333333333ull;
            a1 = (a1 | g1 | (g1 << 1)) & 0x3333333333333333ull;
        }
        for (; s < sg.nseg; ++s) {
            const kdf_pf_w2 v = *(const kdf_pf_w2 *)(sg.seg[s] + i);
            a0 = kdf_pf_sat_add(a0, kdf_pf_values(v.x)); a1 = kdf_pf_sat_add(a1, kdf_pf_values(v.y));
        }
        kdf_pf_w2 r;
        r.x = kdf_pf_encode(a0); r.y = kdf_pf_encode(a1);
        *(kdf_pf_w2 *)(own + i) = r;
    }
}
