// kdf_sketch.h -- the distinct k-mer sketch (include/kdf.h, "distinct k-mer sketch"): a HyperLogLog over the canonical
// k-mers of read streams, so that tables, key slices and owner tables are sized from the reads before any key is stored.
//
// A pure STREAM kernel: it walks the read stream exactly like the prefilter's tally (kdf_prefilter.h) -- the direct
// window extraction for k <= 63, the rolling registers of kdf_long.h for long keys -- and touches no table.  Per valid
// window: the key's 64-bit stored form h, the finaliser g (below), register j = top p bits of g, rank r = 1 + leading
// zeros of the bits behind them; reg[j] = max(reg[j], r).
//
// Registers on the device are 32-bit cells (atomicMax), 2^p of them: 256 KB at p = 16, resident in the L2 of every XCD.
// After the first few thousand windows almost no window raises its register, so the cell is LOADED first and the atomic
// is issued only when the rank is larger (a stale read costs an atomic that changes nothing, never a lost maximum):
// without that every register is one contended atomic address, and a homopolymer key with 10^6 sightings would hammer
// one cell.  The exported form is one byte per register (kdf_sk_pack_kernel).
#pragma once
#include "kdf_device.h"
#include "kdf_long.h"
#include "kdf_prefilter.h"     // kdf_pf_add_windows: the wave-reduced sharded window counter

#include <math.h>

#define KDF_SK_MIN_LOG2 10
#define KDF_SK_MAX_LOG2 18
#define KDF_SK_DEFAULT_LOG2 16

// The finaliser.  kdf_mix64 ends in a multiply, so bit i of h depends on key bits 0..i only (after the one fold of the
// high half): the top bits, which address the table, see every key bit, the low bits do not -- and the rank is read
// from the bits BELOW the index.  Two further xorshift-multiply rounds and a closing xorshift (the finaliser of
// splitmix64, Steele / Lea / Flood 2014; a bijection) bring every input bit to every output bit.
__host__ __device__ __forceinline__ uint64_t kdf_sketch_fin(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// k <= 32 and long keys: g = fin(h).  33 <= k <= 63: the stored form is the PAIR (h, hi), and g takes both words, so
// that two keys whose (lo ^ rotl(hi, 37)) agree are still two keys to the sketch.
#define KDF_SK_HI_MUL 0xD6E8FEB86659FD93ull
__host__ __device__ __forceinline__ uint64_t kdf_sketch_g(uint64_t h) { return kdf_sketch_fin(h); }
__host__ __device__ __forceinline__ uint64_t kdf_sketch_g_wide(uint64_t h, uint64_t hi) { return kdf_sketch_fin(h + hi * KDF_SK_HI_MUL); }

struct KdfSketch {
    uint32_t *cells;       // 2^p cells, cell j = register j (0 .. 65 - p)
    uint32_t p;
};

__device__ __forceinline__ void kdf_sk_locate(uint32_t p, uint64_t g, uint32_t &j, uint32_t &r) {
    j = (uint32_t)(g >> (64 - p));                                        // < 2^p
    r = 1u + (uint32_t)__clzll((long long)((g << p) | (1ull << (p - 1))));   // the guard bit: 1 <= r <= 65 - p
}

// k <= 63.  One thread = one tile of 64 window starts, the stream read as kdf_pf_stream_kernel reads it (positions at or
// past n_bases invalid); windows are taken 8 at a time so that 8 cell loads are in flight per lane.
template <int KW>
__global__ __launch_bounds__(256) void kdf_sk_stream_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_bases, int k,
    KdfSketch sk, unsigned long long *__restrict__ windows)
{
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nwin = 0;
    if (tile < n_tiles) {
        uint64_t m0 = invalid[tile], m1 = invalid[tile + 1];
        kdf_mask_past_end(n_bases - tile * KDF_TILE, m0, m1);          // (tile < ceil(n_bases / 64): the host's n_tiles)
        const uint64_t valid = kdf_valid_windows(m0, m1, k);
        nwin = __popcll(valid);
        if (valid) {
            constexpr int NW = KW == 1 ? 3 : 4;
            uint64_t w[NW];
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = packed[tile * 2 + i];
            const uint64_t kmask = (k >= 32) ? ~0ull : ((1ull << (2 * k)) - 1);
#pragma unroll
            for (int b = 0; b < KDF_TILE; b += 8) {
                if (((valid >> b) & 0xFF) == 0) continue;
                uint32_t j[8], r[8], cur[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    uint64_t klo, khi = 0, g;
                    if constexpr (KW == 1) { klo = kdf_window_narrow((const uint64_t (&)[3])w, b + u, k, kmask); g = kdf_sketch_g(kdf_mix64(klo)); }
                    else { kdf_window_wide((const uint64_t (&)[4])w, b + u, k, klo, khi); g = kdf_sketch_g_wide(kdf_hash(klo, khi), khi); }
                    kdf_sk_locate(sk.p, g, j[u], r[u]);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) cur[u] = ((valid >> (b + u)) & 1) ? sk.cells[j[u]] : 0xFFFFFFFFu;
#pragma unroll
                for (int u = 0; u < 8; ++u) if (r[u] > cur[u]) atomicMax(&sk.cells[j[u]], r[u]);
            }
        }
    }
    kdf_pf_add_windows(windows, nwin);
}

// long keys (odd k 65..201): the rolling registers and clamped loads of kdf_pf_long_kernel
template <int W>
__global__ __launch_bounds__(256) void kdf_sk_long_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_bases, int k,
    KdfSketch sk, unsigned long long *__restrict__ windows)
{
    constexpr int NB = 4;
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = tile < n_tiles;
    const uint64_t T = (n_bases + KDF_TILE - 1) / KDF_TILE;
    const uint64_t pw = 2 * T + 4, mw = T + 2;                   // kdf_stream_words(n_bases)
    const int tb = 2 * k - 64 * (W - 1);
    uint32_t nwin = 0;
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
        uint32_t j[NB], r[NB], cur[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            uint64_t key[W];
            push();                                                // base o - 1 = b + u + k - 1 closes window b + u
            st.canon(key);
            const bool ok = active && st.run >= k;
            if (ok) ++nwin;
            kdf_sk_locate(sk.p, kdf_sketch_g(kdf_long_hash<W>(key)), j[u], r[u]);
            if (!ok) r[u] = 0;                                     // (rank 0 raises nothing)
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) cur[u] = r[u] ? sk.cells[j[u]] : 0xFFFFFFFFu;
#pragma unroll
        for (int u = 0; u < NB; ++u) if (r[u] > cur[u]) atomicMax(&sk.cells[j[u]], r[u]);
    }
    kdf_pf_add_windows(windows, nwin);
}

// cells -> one byte per register (the exported form)
__global__ __launch_bounds__(256) void kdf_sk_pack_kernel(const uint32_t *__restrict__ cells, uint32_t m, uint8_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = (uint8_t)cells[i];
}

// reg = max(own, given); the bytes were range-checked on the host
__global__ __launch_bounds__(256) void kdf_sk_merge_kernel(uint32_t *__restrict__ cells, uint32_t m, const uint8_t *__restrict__ in) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) { const uint32_t v = in[i]; if (v > cells[i]) cells[i] = v; }
}

// The estimate, on the host in double, the registers summed in index order (reproducible).  Returns false when a
// register is above 65 - p.
static inline bool kdf_sk_estimate_host(const uint8_t *regs, uint32_t p, double *out) {
    const uint64_t m = 1ull << p;
    double sum = 0.0;
    uint64_t zeros = 0;
    for (uint64_t i = 0; i < m; ++i) {
        if (regs[i] > 65 - p) return false;
        sum += ldexp(1.0, -(int)regs[i]);
        zeros += regs[i] == 0;
    }
    const double dm = (double)m, alpha = 0.7213 / (1.0 + 1.079 / dm);
    double e = alpha * dm * dm / sum;
    if (e <= 2.5 * dm && zeros > 0) e = dm * log(dm / (double)zeros);   // linear counting
    *out = e;
    return true;
}
