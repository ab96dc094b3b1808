// kdf_tilewalk.h -- the tile walkers of the thread-per-tile stream kernels: count / count --if / scan / gated count
// (kdf_engine.hip, kdf_long.h), the two-pass sieve's tally and gate (kdf_prefilter.h) and the distinct sketch
// (kdf_sketch.h).  One thread = one tile of KDF_TILE = 64 window starts.  A walker reads the tile, forms the canonical
// keys of its windows and hands them to the kernel a batch at a time; the kernel keeps only what differs: locate ->
// load -> resolve for its table, sieve cell or sketch register.
//
// THE END-OF-STREAM RULE of these kernels (include/kdf.h, "Read streams"): a position at or
// past n_bases is invalid whatever the buffers hold there, and no load goes past the kdf_stream_words(n_bases) words
// of the stream (kdf_stream_geom).  For k <= 63 it lives in kdf_walk_tile and nowhere else.  For long keys it lives in
// kdf_walk_tile_long and in ONE kernel that keeps a copy of its loop, kdf_pf_long_kernel (kdf_prefilter.h), whose
// tally measured 5 % slower over the walker.  `packed` / `invalid` / `n_bases` may describe a PIECE of a longer
// stream: the stream that starts at one of its tiles and ends where the whole stream ends.
//
// The loads of a batch belong in the kernel's per-batch body, all issued before the first is used, and only for the
// batch's valid windows.
#pragma once
#include "kdf_device.h"

// ---- k <= 63 (KW = 1, 2): closed-form windows (kdf_device.h, "Window extraction") -------------------------------
// body(b, klo[8], khi[8], vb): the canonical keys of windows b .. b + 7 (khi = 0 for KW == 1) and their validity, bit u
// of vb for window b + u.  Batches without a valid window are skipped, a tile without one loads no packed word.
// `admit`: ANDed into the validity bitmap (the gate's word of the tile; ~0: no gate).  Returns the number of valid
// windows of the tile.  For tile < ceil(n_bases / 64) only.  The body is reached by every lane that reached the batch,
// whatever its own vb: a wave-cooperative probe (kdf_add_wide) may be called from it with todo = that lane's bit.
template <int KW, typename Body>
__device__ __forceinline__ uint32_t kdf_walk_tile(const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid,
                                                  uint64_t tile, uint64_t n_bases, int k, uint64_t admit, Body &&body) {
    uint64_t m0 = invalid[tile], m1 = invalid[tile + 1];
    kdf_mask_past_end(n_bases - tile * KDF_TILE, m0, m1);
    const uint64_t valid = kdf_valid_windows(m0, m1, k) & admit;
    if (valid) {
        constexpr int NW = KW == 1 ? 3 : 4;
        uint64_t w[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = packed[tile * 2 + i];
        const uint64_t kmask = (k >= 32) ? ~0ull : ((1ull << (2 * k)) - 1);
#pragma unroll
        for (int b = 0; b < KDF_TILE; b += 8) {
            const uint32_t vb = (uint32_t)(valid >> b) & 0xFFu;
            if (vb == 0) continue;
            uint64_t klo[8], khi[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if constexpr (KW == 1) { klo[u] = kdf_window_narrow(w, b + u, k, kmask); khi[u] = 0; }
                else kdf_window_wide(w, b + u, k, klo[u], khi[u]);
            }
            body(b, klo, khi, vb);
        }
    }
    return (uint32_t)__popcll(valid);
}

// ---- odd k 65..201 (W = 3..7 words per key, kdf_long.h): rolling registers ----------------------------------------
// The thread rolls a forward and a reverse-complement register of W words base by base over the 64 + k - 1 bases of
// its tile and keeps validity as the run length of valid bases since the last invalid position (kdf_valid_windows
// assumes k <= 64).
template <int W>
struct KdfRoll {
    uint64_t f[W], r[W];
    int run;
    __device__ __forceinline__ void push(uint32_t b, bool inv, int tb) {
        // forward: (f << 2) | b over W words, top word masked to tb bits
#pragma unroll
        for (int j = W - 1; j >= 1; --j) f[j] = (f[j] << 2) | (f[j - 1] >> 62);
        f[0] = (f[0] << 2) | b;
        f[W - 1] &= (1ull << tb) - 1;
        // reverse complement: (r >> 2) | ((3 - b) << (2k - 2))
#pragma unroll
        for (int j = 0; j < W - 1; ++j) r[j] = (r[j] >> 2) | (r[j + 1] << 62);
        r[W - 1] = (r[W - 1] >> 2) | ((uint64_t)(3u - b) << (tb - 2));
        run = inv ? 0 : run + 1;
    }
    // canonical = numeric minimum (odd k: never a tie)
    __device__ __forceinline__ void canon(uint64_t (&w)[W]) const {
        bool lt = false, decided = false;
#pragma unroll
        for (int j = W - 1; j >= 0; --j) {
            if (!decided && f[j] != r[j]) { lt = f[j] < r[j]; decided = true; }
        }
#pragma unroll
        for (int j = 0; j < W; ++j) w[j] = lt ? f[j] : r[j];
    }
};

// Two bodies.  each(u, key[W], ok) is called as window b + u of a batch is formed, u = 0 .. NB - 1: the kernel hashes the
// key there and keeps what it needs of it (a slot, a cell), so that the keys of a batch need not all stay in registers;
// ok: the window is valid (and admitted: bit b + u of `admit`; ~0: no gate).  batch(b) follows the NB calls.  Returns
// the number of ok windows of the tile.  EVERY lane of the wave walks all 64 / NB batches, an inactive one (tile at or
// past the launch's n_tiles) with every window invalid and no load, so that a wave-cooperative probe loop in batch()
// (kdf_add_long) stays wave-uniform: no early return before the walk.
template <int W, int NB, typename Each, typename Batch>
__device__ __forceinline__ uint32_t kdf_walk_tile_long(const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid,
                                                       uint64_t tile, bool active, uint64_t n_bases, int k, uint64_t admit,
                                                       Each &&each, Batch &&batch) {
    const KdfStreamGeom g = kdf_stream_geom(n_bases);
    const int tb = 2 * k - 64 * (W - 1);                          // bits of the top word, 2 .. 62
    KdfRoll<W> st;
#pragma unroll
    for (int j = 0; j < W; ++j) { st.f[j] = 0; st.r[j] = 0; }
    st.run = 0;
    const uint64_t p0 = tile * KDF_TILE;
    uint64_t cur = 0, curm = ~0ull;
    int o = 0;                                                    // bases pushed so far (local offset)
    auto push = [&]() {
        if ((o & 31) == 0) { const uint64_t q = 2 * tile + (o >> 5); cur = (active && q < g.packed_words) ? packed[q] : 0; }
        if ((o & 63) == 0) { const uint64_t q = tile + (o >> 6); curm = (active && q < g.mask_words) ? invalid[q] : ~0ull; }
        const bool inv = (curm & 1) || p0 + (uint64_t)o >= n_bases;
        st.push((uint32_t)(cur & 3), inv, tb);
        cur >>= 2; curm >>= 1; ++o;
    };
    for (int i = 0; i < k - 1; ++i) push();
    uint32_t nwin = 0;
    for (int b = 0; b < KDF_TILE; b += NB) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            uint64_t key[W];
            push();                                                // base o - 1 = b + u + k - 1 closes window b + u
            st.canon(key);
            const bool ok = active && st.run >= k && ((admit >> (b + u)) & 1);
            if (ok) ++nwin;
            each(u, key, ok);
        }
        batch(b);
    }
    return nwin;
}
