// kdf_long_sieve.h -- long keys (odd k 65..201) through the membership sieve: count --if and the Module-3 scan of a
// stream in which almost every window MISSES the table.  Opt-in: option "long_sieve".
// Included by kdf_engine.hip behind KdfSieve / kdf_sieve_bits: the sieve is the one of k <= 63 (two bits inside one
// 64-bit word per key, chosen by the stored form h), so sieve_prepare sizes it whatever the key width.
//
// Survivors probe the table IN PLACE, from the registers that hold the keys of the batch: no LDS queue.  A long key is
// W words, so a queue entry would be up to 60 B; in place the scan keeps its one uint64 store per tile (no atomics, no
// zeroed bitmap, no 2^32-position limit) and the LDS holds nothing but the sieve.  The price is divergence: a wave waits
// for the lanes of a batch that have a survivor.
#pragma once
#include "kdf_long.h"

// the sieve over the keys a long table holds now: a slot's lo is the stored form h already
template <int W>
__global__ __launch_bounds__(256) void kdf_long_sieve_from_table_kernel(KdfTable t, uint64_t *__restrict__ words, uint64_t wmask) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1ull << t.log2cap)) return;
    if (*kdf_long_word<W>(t, W - 1, i) == KDF_EMPTY) return;
    uint64_t w, b;
    kdf_sieve_bits(t.lo[i], wmask, w, b);
    atomicOr((unsigned long long *)&words[w], (unsigned long long)b);
}

#define KDF_LSV_THREADS 256               // sieve read from L2
#define KDF_LSV_LDS_THREADS 512           // sieve copied into LDS: 2 waves per SIMD each, so one or two workgroups per CU by the
                                          // instantiation's registers (3 or 4-5 waves per SIMD; two 64 KB sieves fit the LDS)

// One thread = one tile at a time (kdf_walk_tile_long).  each(): the hash and, for a valid window only, the request for
// its sieve word -- NB of them in flight.  batch(): the two bits; the survivors' home-slot top words, all requested
// before the first probe; then kdf_add_long (count --if: reached by the whole wave, todo = survivor) or kdf_find_long
// and cnt != 0 (SCAN).
// IN_LDS: the sieve (sv.wmask + 1 <= KDF_SV_LDS_WORDS words of dynamic LDS) is copied once per workgroup, so the grid is
// what a device holds at once and every thread walks `rounds` tiles, a grid apart (the host's ceil(n_tiles / threads
// of the grid): wave-uniform).  The L2 form is launched one tile per thread like the direct kernel and ignores
// `rounds`: the loop's scalar registers made its W = 7 instantiations spill.
template <int W, bool IN_LDS, bool SCAN>
__global__ __launch_bounds__(IN_LDS ? KDF_LSV_LDS_THREADS : KDF_LSV_THREADS) void kdf_long_sieve_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_bases, int k,
    KdfTable t, KdfCtl *ctl, KdfSieve sv, uint32_t rounds, uint64_t *__restrict__ hit_bits)
{
    constexpr int NB = KdfLongCfg<W>::NB;
    extern __shared__ __attribute__((aligned(16))) uint64_t kdf_lsv[];
    if constexpr (IN_LDS) {
        for (uint32_t i = threadIdx.x; i <= (uint32_t)sv.wmask; i += blockDim.x) kdf_lsv[i] = sv.words[i];
        __syncthreads();
    }
    const uint64_t *const svw = IN_LDS ? kdf_lsv : sv.words;
    const uint32_t wmask = (uint32_t)sv.wmask;                     // (a sieve has fewer than 2^32 words)
    uint32_t claimed = 0, nwin = 0, full = 0;
    uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nr = IN_LDS ? rounds : 1u;
    for (uint32_t r = 0; r < nr; ++r, tile += (uint64_t)gridDim.x * blockDim.x) {
        const bool active = tile < n_tiles;
        uint64_t hits = 0;
        uint64_t key[NB][W], h[NB], sw[NB];
        uint32_t okm = 0;                                          // bit u: window u of the batch is valid (NB lane masks would spill SGPRs)
        nwin += kdf_walk_tile_long<W, NB>(packed, invalid, tile, active, n_bases, k, ~0ull,
            [&](int u, const uint64_t (&kw)[W], bool okw) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < W; ++j) key[u][j] = kw[j];
                h[u] = kdf_long_hash<W>(kw);
                okm = (u ? okm : 0u) | (okw ? 1u << u : 0u);
                sw[u] = 0;                                         // (an invalid window asks for nothing)
                if (okw) sw[u] = svw[(uint32_t)(h[u] >> 12) & wmask];
            },
            [&](int b) __attribute__((always_inline)) {
                uint64_t slot[NB], pre[NB];
                uint32_t surv = 0;
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    surv |= ((okm >> u) & (uint32_t)(sw[u] >> (h[u] & 63)) & (uint32_t)(sw[u] >> ((h[u] >> 6) & 63)) & 1u) << u;
                    slot[u] = kdf_home(t, h[u]);
                    pre[u] = ((surv >> u) & 1) ? *kdf_long_word<W>(t, W - 1, slot[u]) : KDF_EMPTY;
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    if constexpr (SCAN) {
                        if (((surv >> u) & 1) && pre[u] != KDF_EMPTY) {
                            const uint64_t s = kdf_find_long<W>(t, h[u], key[u]);
                            if (s != ~0ull && t.cnt[s] != 0) hits |= 1ull << (b + u);
                        }
                    } else {
                        full |= kdf_add_long<W, false>(t, (surv >> u) & 1, h[u], key[u], 1u, slot[u], pre[u], true, claimed) ? 0u : 1u;
                    }
                }
            });
        if (SCAN && active) hit_bits[tile] = hits;
    }
    if (full) atomicOr(&ctl->error, 1u);
    if constexpr (!SCAN) kdf_shard_add(ctl->windows, nwin);        // (exactly what the direct kernel adds; a scan counts nothing)
}
