// kdf_sketch.h -- the distinct k-mer sketch (include/kdf.h, "distinct k-mer sketch"): a HyperLogLog over the canonical
// k-mers of read streams, so that tables, key slices and owner tables are sized from the reads before any key is stored.
//
// A pure STREAM kernel: it walks the read stream tile by tile (kdf_tilewalk.h) and touches no table.  Per valid
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

// (struct KdfSketch -- cells, p -- is in kdf_device.h: the engine holds one by value)

__device__ __forceinline__ void kdf_sk_locate(uint32_t p, uint64_t g, uint32_t &j, uint32_t &r) {
    j = (uint32_t)(g >> (64 - p));                                        // < 2^p
    r = 1u + (uint32_t)__clzll((long long)((g << p) | (1ull << (p - 1))));   // the guard bit: 1 <= r <= 65 - p
}

// k <= 63.  One thread = one tile of 64 window starts (kdf_walk_tile, kdf_tilewalk.h); windows are taken 8 at a time so
// that 8 cell loads are in flight per lane.
template <int KW>
__global__ __launch_bounds__(256) void kdf_sk_stream_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_bases, int k,
    KdfSketch sk, unsigned long long *__restrict__ windows)
{
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nwin = 0;
    if (tile < n_tiles) {
        nwin = kdf_walk_tile<KW>(packed, invalid, tile, n_bases, k, ~0ull,
            [&](int, const uint64_t (&klo)[8], const uint64_t (&khi)[8], uint32_t vb) __attribute__((always_inline)) {
                uint32_t j[8], r[8], cur[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint64_t h = kdf_hash(klo[u], khi[u]);
                    kdf_sk_locate(sk.p, KW == 1 ? kdf_sketch_g(h) : kdf_sketch_g_wide(h, khi[u]), j[u], r[u]);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) cur[u] = ((vb >> u) & 1) ? sk.cells[j[u]] : 0xFFFFFFFFu;   // (invalid: nothing is above it)
#pragma unroll
                for (int u = 0; u < 8; ++u) if (r[u] > cur[u]) atomicMax(&sk.cells[j[u]], r[u]);
            });
    }
    kdf_shard_add(windows, nwin);
}

// long keys (odd k 65..201): kdf_walk_tile_long, 4 cell loads in flight per lane
template <int W>
__global__ __launch_bounds__(256) void kdf_sk_long_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_bases, int k,
    KdfSketch sk, unsigned long long *__restrict__ windows)
{
    constexpr int NB = 4;
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t j[NB], r[NB], cur[NB];
    const uint32_t nwin = kdf_walk_tile_long<W, NB>(packed, invalid, tile, tile < n_tiles, n_bases, k, ~0ull,
        [&](int u, const uint64_t (&key)[W], bool ok) __attribute__((always_inline)) {
            kdf_sk_locate(sk.p, kdf_sketch_g(kdf_long_hash<W>(key)), j[u], r[u]);
            if (!ok) r[u] = 0;                                     // (rank 0 raises nothing)
        },
        [&](int) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < NB; ++u) cur[u] = r[u] ? sk.cells[j[u]] : 0xFFFFFFFFu;
#pragma unroll
            for (int u = 0; u < NB; ++u) if (r[u] > cur[u]) atomicMax(&sk.cells[j[u]], r[u]);
        });
    kdf_shard_add(windows, nwin);
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
