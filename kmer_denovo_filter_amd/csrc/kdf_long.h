// kdf_long.h -- long keys: odd k from 65 to 201, W = ceil(2k/64) = 3..7 64-bit words per key.
// Everything is templated on W; kdf_engine.hip instantiates W = 3 .. 7.
//
// Key words.  Word 0 holds the least significant 64 bits of the Jellyfish value (2 bits per base, A=0 C=1 G=2 T=3,
// leftmost base most significant); word W-1, the TOP word, holds 2k - 64 (W - 1) <= 62 bits for odd k, so the
// all-ones KDF_EMPTY and the KDF_PENDING bit stay free exactly as for wide keys.
//
// Table.  Open addressing, structure of arrays:
//   t.lo[cap]             stored form h = kdf_mix64(w0 ^ kdf_long_fold(w1 .. w_{W-1}))
//   t.hi[(j - 1) cap + s] key word j = 1 .. W-1 of slot s (the top word last)
//   t.cnt[cap]            saturating uint32 count
// Home slot, bucket and key_parts slice come from h, as for narrow and wide keys; w0 comes back on export as
// kdf_unmix64(h) ^ kdf_long_fold(...).  The fold multiplies: a plain XOR of rotated words would let keys that differ
// only in their upper words (w0 shared, or everything but the top word shared) collide into one home slot.
#pragma once
#include "kdf_device.h"
#include "kdf_tilewalk.h"

#define KDF_LONG_MIN_K 65
#define KDF_LONG_MAX_K 201

__host__ __device__ __forceinline__ uint64_t kdf_long_fold_step(uint64_t f, uint64_t w) {
    return kdf_mix64(f ^ w) + 0x632BE59BD9B4E019ull;          // (the constant keeps an all-zero upper part from folding to 0)
}
template <int W>
__host__ __device__ __forceinline__ uint64_t kdf_long_fold(const uint64_t (&w)[W]) {
    uint64_t f = 0;
#pragma unroll
    for (int j = W - 1; j >= 1; --j) f = kdf_long_fold_step(f, w[j]);
    return f;
}
template <int W>
__host__ __device__ __forceinline__ uint64_t kdf_long_hash(const uint64_t (&w)[W]) {
    return kdf_mix64(w[0] ^ kdf_long_fold<W>(w));
}

// word j (1 .. W-1) of slot s
template <int W>
__device__ __forceinline__ uint64_t *kdf_long_word(const KdfTable &t, int j, uint64_t s) {
    return t.hi + ((uint64_t)(j - 1) << t.log2cap) + s;
}

// ---- claim protocol: the wide keys' (kdf_device.h), generalised to W words -------------------------------------
// 1. CAS the top word EMPTY -> top | PENDING; 2. publish h and the middle words with returning atomics (complete at
// memory before the final store issues); 3. store the final top word.  A prober that matches a PENDING top word
// returns KDF_BLOCKED and is retried by the caller's wave-uniform loop (kdf_add_long): no lane ever waits inside a
// divergent loop.  A match needs the top word, h and every middle word to be equal.  Two random keys never share h, so
// the middle-word compares (here and in kdf_find_long) are reachable only with keys written under one h
// (tests/long_truth.py, used by tests/test_gpu_long_table_truth.py).
//
// `pre`: the top word of the home slot loaded earlier by the caller (KDF_EMPTY-safe: a claimed top word never
// changes, and a stale EMPTY is corrected by the CAS); have_pre = false loads it here.
template <int W, bool INSERT>
__device__ __forceinline__ int kdf_try_add_long(const KdfTable &t, uint64_t h, const uint64_t (&w)[W], uint32_t add,
                                                uint64_t slot, uint64_t pre, bool have_pre, uint32_t &claimed) {
    const uint64_t bmask = (1ull << t.bucket_bits) - 1;
    const uint64_t base = slot & ~bmask;
    const uint64_t ktop = w[W - 1];
    for (uint64_t i = 0;;) {
        uint64_t *ptop = kdf_long_word<W>(t, W - 1, slot);
        uint64_t ctop = (i == 0 && have_pre) ? pre : (INSERT ? kdf_ld(ptop) : *ptop);
        if (ctop == KDF_EMPTY) {
            if (!INSERT) return KDF_OK_ADD;
            const uint64_t old = atomicCAS((unsigned long long *)ptop, KDF_EMPTY, ktop | KDF_PENDING);
            if (old == KDF_EMPTY) {
                uint64_t prev = atomicExch((unsigned long long *)&t.lo[slot], h);
#pragma unroll
                for (int j = 1; j < W - 1; ++j) prev ^= atomicExch((unsigned long long *)kdf_long_word<W>(t, j, slot), w[j]);
                asm volatile("s_waitcnt vmcnt(0)" :: "v"(prev) : "memory");
                __hip_atomic_store(ptop, ktop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                claimed++;
                if (add) kdf_sat_add(&t.cnt[slot], add);
                return KDF_OK_ADD;
            }
            ctop = old;
        }
        if ((ctop & ~KDF_PENDING) == ktop) {
            if (ctop & KDF_PENDING) return KDF_BLOCKED;          // h / middle words not published yet: retry later
            bool eq = (INSERT ? kdf_ld(&t.lo[slot]) : t.lo[slot]) == h;
#pragma unroll
            for (int j = 1; j < W - 1; ++j) {
                const uint64_t *pw = kdf_long_word<W>(t, j, slot);
                eq = eq && (INSERT ? kdf_ld(pw) : *pw) == w[j];
            }
            if (eq) { if (add) kdf_sat_add(&t.cnt[slot], add); return KDF_OK_ADD; }
        }
        if (++i > bmask) return KDF_FULL;
        slot = base | ((slot + 1) & bmask);
    }
}

// Reached by the lanes of a wave together; `todo` tells which of them have a key.
template <int W, bool INSERT>
__device__ __forceinline__ bool kdf_add_long(const KdfTable &t, bool todo, uint64_t h, const uint64_t (&w)[W], uint32_t add,
                                             uint64_t slot, uint64_t pre, bool have_pre, uint32_t &claimed) {
    bool ok = true;
    while (__any(todo)) {
        if (todo) {
            const int r = kdf_try_add_long<W, INSERT>(t, h, w, add, slot, pre, have_pre, claimed);
            if (r != KDF_BLOCKED) { todo = false; ok = (r == KDF_OK_ADD); }
            have_pre = false;                                   // a retry reloads the top word
        }
        __builtin_amdgcn_wave_barrier();
    }
    return ok;
}

// slot of the key or ~0 when absent (read-only table)
template <int W>
__device__ __forceinline__ uint64_t kdf_find_long(const KdfTable &t, uint64_t h, const uint64_t (&w)[W]) {
    const uint64_t bmask = (1ull << t.bucket_bits) - 1;
    uint64_t slot = kdf_home(t, h);
    const uint64_t base = slot & ~bmask;
    for (uint64_t i = 0; i <= bmask; ++i) {
        const uint64_t ctop = *kdf_long_word<W>(t, W - 1, slot);
        if (ctop == KDF_EMPTY) return ~0ull;
        if (ctop == w[W - 1] && t.lo[slot] == h) {
            bool eq = true;
#pragma unroll
            for (int j = 1; j < W - 1; ++j) eq = eq && *kdf_long_word<W>(t, j, slot) == w[j];
            if (eq) return slot;
        }
        slot = base | ((slot + 1) & bmask);
    }
    return ~0ull;
}

// ---- read stream -> canonical long keys -----------------------------------------------------------------------------
// One thread = one tile of 64 window starts, walked by kdf_walk_tile_long (kdf_tilewalk.h), so the hit bitmap of
// MODE_SCAN is still one uint64 store per tile.  Windows are resolved NB at a time: the NB top-word loads of their
// home slots are issued back to back before any of them is used.
template <int W> struct KdfLongCfg { static constexpr int NB = W == 3 ? 8 : 4; };   // (W = 4 at 8: SGPR spills in MODE_SCAN)

template <int W, int MODE>
__global__ __launch_bounds__(256) void kdf_long_stream_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid,
    uint64_t n_tiles, uint64_t n_bases, int k, KdfTable t, KdfCtl *ctl,
    uint64_t *__restrict__ hit_bits)
{
    constexpr int NB = KdfLongCfg<W>::NB;
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = tile < n_tiles;
    uint32_t claimed = 0, dropped = 0;
    bool full = false;
    uint64_t hits = 0;
    const bool sliced = MODE == MODE_INSERT && t.key_parts > 1;
    constexpr bool INS = MODE == MODE_INSERT || MODE == MODE_GATED;       // keys are inserted (MODE_GATED: behind a prefilter,
    uint64_t adm = ~0ull;                                                 // hit_bits[tile] = the tile's admitted windows)
    if constexpr (MODE == MODE_GATED) adm = active ? hit_bits[tile] : 0ull;
    uint64_t key[NB][W], h[NB], slot[NB];
    bool ok[NB];
    const uint32_t nwin = kdf_walk_tile_long<W, NB>(packed, invalid, tile, active, n_bases, k, adm,
        [&](int u, const uint64_t (&kw)[W], bool okw) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < W; ++j) key[u][j] = kw[j];
            h[u] = kdf_long_hash<W>(kw);
            slot[u] = kdf_home(t, h[u]);
            ok[u] = okw;
            if (sliced && okw && kdf_slice(h[u], t.key_parts) != t.key_part) { ok[u] = false; ++dropped; }
        },
        [&](int b) __attribute__((always_inline)) {
            uint64_t pre[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const uint64_t *ptop = kdf_long_word<W>(t, W - 1, slot[u]);
                pre[u] = ok[u] ? (INS ? kdf_ld(ptop) : *ptop) : KDF_EMPTY;
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                if constexpr (MODE == MODE_SCAN) {
                    if (ok[u] && pre[u] != KDF_EMPTY) {
                        const uint64_t s = kdf_find_long<W>(t, h[u], key[u]);
                        if (s != ~0ull && t.cnt[s] != 0) hits |= 1ull << (b + u);
                    }
                } else {
                    if (!kdf_add_long<W, INS>(t, ok[u], h[u], key[u], 1u, slot[u], pre[u], true, claimed)) full = true;
                }
            }
        });
    if (MODE == MODE_SCAN && active) hit_bits[tile] = hits;
    if (full) atomicOr(&ctl->error, 1u);
    kdf_shard_add(ctl->distinct, claimed);
    if constexpr (MODE != MODE_SCAN) kdf_shard_add(ctl->windows, nwin - dropped);   // (a scan counts nothing)
}

// ---- key kernels --------------------------------------------------------------------------------------------------
// Word j of key i is src[i * rs + j * ws]: row-major caller keys (rs = W, ws = 1) or the SoA slots of a table that is
// being rehashed (rs = 1, ws = old capacity; `stored`: word 0 is then the stored form h, not w0).
template <int W>
__device__ __forceinline__ void kdf_long_read_key(const uint64_t *w0p, const uint64_t *upp, uint64_t rs, uint64_t ws,
                                                  uint64_t i, uint64_t (&w)[W]) {
    w[0] = w0p[i * rs];
#pragma unroll
    for (int j = 1; j < W; ++j) w[j] = upp[i * rs + (uint64_t)(j - 1) * ws];
}

// thread per key: insert with an explicit add (add_pairs: add = counts[i]; filter load: add = NULL; rehash: add = count).
// A caller key whose top word has a bit at or above tb = 2k - 64 (W - 1) is no k-mer (and bits 62 / 63 could collide
// with EMPTY / PENDING): it is left out and raises error bit 4.
template <int W>
__global__ __launch_bounds__(256) void kdf_long_insert_kernel(
    const uint64_t *__restrict__ w0p, const uint64_t *__restrict__ upp, uint64_t rs, uint64_t ws,
    const uint32_t *__restrict__ add, uint64_t n, KdfTable t, KdfCtl *ctl, int stored, int tb)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t claimed = 0;
    bool full = false;
    {
        uint64_t w[W];
#pragma unroll
        for (int j = 0; j < W; ++j) w[j] = KDF_EMPTY;
        if (i < n) kdf_long_read_key<W>(w0p, upp, rs, ws, i, w);
        const bool bad = i < n && !stored && (w[W - 1] >> tb) != 0;
        if (bad) atomicOr(&ctl->error, 4u);
        w[W - 1] &= ~KDF_PENDING;                                     // (EMPTY stays "absent" below)
        const bool todo = i < n && !bad && (!stored || w[W - 1] != (KDF_EMPTY & ~KDF_PENDING));
        const uint32_t a = (todo && add) ? add[i] : 0u;
        const uint64_t h = stored ? w[0] : kdf_long_hash<W>(w);
        const uint64_t slot = kdf_home(t, h);
        if (!kdf_add_long<W, true>(t, todo, h, w, a, slot, 0, false, claimed)) full = true;
    }
    if (full) atomicOr(&ctl->error, 1u);
    kdf_shard_add(ctl->distinct, claimed);
}

template <int W>
__global__ __launch_bounds__(256) void kdf_long_query_kernel(const uint64_t *__restrict__ keys, uint64_t n, KdfTable t,
                                                            uint32_t *__restrict__ out, int tb)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t w[W];
    kdf_long_read_key<W>(keys, keys + 1, W, 1, i, w);
    // a top word with a bit at or above tb = 2k - 64 (W - 1) is no k-mer: absent (and never matches a PENDING slot)
    const uint64_t s = (w[W - 1] >> tb) ? ~0ull : kdf_find_long<W>(t, kdf_long_hash<W>(w), w);
    out[i] = (s == ~0ull) ? 0u : t.cnt[s];
}

// dump -L: count (WRITE = false: into ctl->tally) or append (cursor) the entries with cnt >= min_count, keys rebuilt
// row-major.  A wave owns KDF_EXPORT_ROWS x 64 consecutive slots and reserves its output range with one atomic.
template <int W, bool WRITE>
__global__ __launch_bounds__(256) void kdf_long_export_kernel(
    KdfTable t, uint32_t min_count, KdfCtl *ctl, uint64_t *__restrict__ okeys, uint32_t *__restrict__ ocnt, uint64_t out_cap)
{
    const uint64_t cap = 1ull << t.log2cap;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t first = wave * (KDF_EXPORT_ROWS * 64);
    if (first >= cap) return;
    const uint64_t *top = t.hi + ((uint64_t)(W - 2) << t.log2cap);
    uint32_t mine = 0;
    for (int r = 0; r < KDF_EXPORT_ROWS; ++r) {
        const uint64_t i = first + (uint64_t)r * 64 + lane;
        if (i < cap) mine += (min_count >= 1 ? t.cnt[i] >= min_count : top[i] != KDF_EMPTY) ? 1u : 0u;
    }
    uint32_t tot = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    if (tot == 0) return;
    if (!WRITE) {
        if (lane == 0) atomicAdd(&ctl->tally[(uint32_t)(wave % KDF_SHARDS) * 16], (unsigned long long)tot);
        return;
    }
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&ctl->cursor, (unsigned long long)tot);
    base = __shfl(base, 0);
    for (int r = 0; r < KDF_EXPORT_ROWS; ++r) {
        const uint64_t i = first + (uint64_t)r * 64 + lane;
        bool keep = false;
        uint32_t c = 0;
        if (i < cap) {
            c = t.cnt[i];
            keep = top[i] != KDF_EMPTY && c >= min_count;
        }
        const unsigned long long bb = __ballot(keep);
        if (keep) {
            const uint64_t pos = base + __popcll(bb & ((1ull << lane) - 1));
            if (pos < out_cap) {
                uint64_t w[W];
                w[0] = 0;
#pragma unroll
                for (int j = 1; j < W; ++j) w[j] = *kdf_long_word<W>(t, j, i);
                w[0] = kdf_unmix64(t.lo[i]) ^ kdf_long_fold<W>(w);   // w0 back from the stored form
#pragma unroll
                for (int j = 0; j < W; ++j) okeys[pos * W + j] = w[j];
                if (ocnt) ocnt[pos] = c;
            }
        }
        base += __popcll(bb);
    }
}
