// kdf_engine.hip -- libkdf.so, the core unit: the table, the direct kernels, the sieve, the host side of the binned
// pipeline and the merge, the long-key paths, the table join, the counting sieve, the sketch, the device BAM feeder, and the engine's C
// ABI of include/kdf.h (create and destroy, count, count --if, query, export, profile, options and stats).  The
// per-read consumers live in kdf_engine_reads.hip, the read spool in kdf_spool.hip; kdf_engine_priv.h is what they
// share.  See DESIGN.md for the data layout and the roofline of each kernel.  No CPU fallback exists in this library:
// every entry point either runs on the GPU or returns an error.
#include <hip/hip_runtime.h>
#include <zlib.h>
#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "kdf_engine_priv.h"
#include "kdf_tilewalk.h"
#include "kdf_binned.h"
#include "kdf_merge.h"
#include "kdf_histo.h"
// long keys (odd k 65..201): table layout, claim protocol and kernels
#include "kdf_long.h"
// ... across ranks: the dump grouped by owner rank, set_counts
#include "kdf_long_merge.h"
// table join: one table's entries by their count in another table
#include "kdf_join.h"
// the counting sieve of the two-pass count: tally, gate and fill kernels
#include "kdf_prefilter.h"
#include "kdf_sketch.h"
#include "kdf_bamdev.h"

// sorted export lives in kdf_sort.hip (rocPRIM radix sort)
int kdf_sort_pairs_device(uint64_t *d_lo, uint64_t *d_hi, uint32_t *d_cnt, uint64_t n,
                          hipStream_t stream, std::string &err);
int kdf_sort_rows_device(uint64_t *d_keys, int words, uint32_t *d_cnt, uint64_t n, hipStream_t stream, std::string &err);

// ===========================================================================
// kernels
// ===========================================================================

// One thread = one tile of 64 window starts (kdf_walk_tile, kdf_tilewalk.h).  Windows are processed in batches
// of 8: the 8 home-slot key loads are issued back to back before any of them is
// resolved, so a wave keeps 8 x 64 random HBM reads in flight.
template <int KW, int MODE>
__global__ __launch_bounds__(256) void kdf_stream_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid,
    uint64_t n_tiles, uint64_t n_bases, int k, KdfTable t, KdfCtl *ctl,
    uint64_t *__restrict__ hit_bits)
{
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t claimed = 0, nwin = 0;
    bool full = false;
    if (tile < n_tiles) {
        const bool sliced = MODE == MODE_INSERT && t.key_parts > 1;       // count only this key-space slice (KdfTable::key_parts)
        uint64_t hits = 0;
        uint32_t dropped = 0;
        nwin = kdf_walk_tile<KW>(packed, invalid, tile, n_bases, k, MODE == MODE_GATED ? hit_bits[tile] : ~0ull,
            [&](int b, uint64_t (&klo)[8], const uint64_t (&khi)[8], uint32_t vb) __attribute__((always_inline)) {
                uint64_t slot[8], cur[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint64_t hsh = kdf_hash(klo[u], khi[u]);
                    klo[u] = hsh;                                  // from here on the key is its stored form (kdf_device.h)
                    slot[u] = kdf_home(t, hsh);
                    if (sliced && ((vb >> u) & 1) && kdf_slice(hsh, t.key_parts) != t.key_part) { vb &= ~(1u << u); ++dropped; }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bool ok = (vb >> u) & 1;
                    if constexpr (KW == 1) cur[u] = ok ? t.lo[slot[u]] : 0;
                    else cur[u] = 0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bool ok = (vb >> u) & 1;
                    if constexpr (MODE == MODE_SCAN) {
                        if (!ok) continue;
                        uint64_t s = KW == 1 ? kdf_find_narrow(t, klo[u]) : kdf_find_wide(t, klo[u], khi[u]);
                        if (s != ~0ull && t.cnt[s] != 0) hits |= 1ull << (b + u);
                    } else if constexpr (KW == 1) {
                        if (!ok) continue;
                        if (!kdf_add_narrow<MODE != MODE_FILTERED>(t, klo[u], 1u, slot[u], cur[u], claimed)) full = true;
                    } else {
                        // every lane that reached this batch calls in; idle lanes pass todo = false
                        if (!kdf_add_wide<MODE != MODE_FILTERED>(t, ok, klo[u], khi[u], 1u, slot[u], claimed)) full = true;
                    }
                }
            });
        nwin -= dropped;
        if constexpr (MODE == MODE_SCAN) hit_bits[tile] = hits;
    }
    if (full) atomicOr(&ctl->error, 1u);
    kdf_shard_add(ctl->distinct, claimed);
    if constexpr (MODE != MODE_SCAN) kdf_shard_add(ctl->windows, nwin);   // (a scan counts nothing: kdf_stats' windows are the count calls')
}

// thread per key: insert with an explicit add (filter load: add = 0; rehash: add = count).
// stored != 0: klo[] already holds stored forms (the slots of a table that is being rehashed), else keys.
template <int KW>
__global__ __launch_bounds__(256) void kdf_insert_keys_kernel(
    const uint64_t *__restrict__ klo, const uint64_t *__restrict__ khi,
    const uint32_t *__restrict__ add, uint64_t n, KdfTable t, KdfCtl *ctl, int skip_empty, int stored)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t claimed = 0;
    bool full = false;
    {
        const uint64_t lo = i < n ? klo[i] : KDF_EMPTY, hi = (KW == 2 && i < n) ? khi[i] : (KW == 2 ? KDF_EMPTY : 0);
        const bool present = KW == 1 ? (lo != KDF_EMPTY) : (hi != KDF_EMPTY);
        const bool todo = i < n && (present || !skip_empty);
        const uint32_t a = (todo && add) ? add[i] : 0u;
        const uint64_t h = stored ? lo : kdf_hash(lo, (KW == 2 ? hi & ~KDF_PENDING : 0));
        const uint64_t slot = kdf_home(t, h);
        if constexpr (KW == 1) {
            if (todo && !kdf_add_narrow<true>(t, h, a, slot, t.lo[slot], claimed)) full = true;
        } else {
            if (!kdf_add_wide<true>(t, todo, h, hi & ~KDF_PENDING, a, slot, claimed)) full = true;
        }
    }
    if (full) atomicOr(&ctl->error, 1u);
    kdf_shard_add(ctl->distinct, claimed);
}

template <int KW>
__global__ __launch_bounds__(256) void kdf_query_kernel(
    const uint64_t *__restrict__ klo, const uint64_t *__restrict__ khi, uint64_t n,
    KdfTable t, uint32_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = KW == 1 ? kdf_find_narrow(t, kdf_hash(klo[i], 0)) : kdf_find_wide(t, kdf_hash(klo[i], khi[i]), khi[i]);
    out[i] = (s == ~0ull) ? 0u : t.cnt[s];
}

// thread per key: the count of a STORED key becomes counts[i] (the merged counts of a sharded count --if go back into
// every rank's table); a key that is not stored raises the error flag
template <int KW>
__global__ __launch_bounds__(256) void kdf_set_counts_kernel(
    const uint64_t *__restrict__ klo, const uint64_t *__restrict__ khi, const uint32_t *__restrict__ counts, uint64_t n,
    KdfTable t, KdfCtl *ctl)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = KW == 1 ? kdf_find_narrow(t, kdf_hash(klo[i], 0)) : kdf_find_wide(t, kdf_hash(klo[i], khi[i]), khi[i]);
    if (s == ~0ull) atomicOr(&ctl->error, 2u);
    else t.cnt[s] = counts[i];
}

// dump -L: count / append entries with cnt >= min_count.  Each wave owns a
// chunk of EXPORT_ROWS x 64 consecutive slots: it counts its matches, reserves
// its output range with ONE atomic, then re-reads the (cache-resident) chunk and
// writes.  One same-address atomic per 2048 slots instead of one per 64.
// (KDF_EXPORT_ROWS = 32: kdf_device.h, the dumps of long keys use it too)
template <int KW, bool WRITE>
__global__ __launch_bounds__(256) void kdf_export_kernel(
    KdfTable t, uint32_t min_count, KdfCtl *ctl, uint64_t *__restrict__ olo,
    uint64_t *__restrict__ ohi, uint32_t *__restrict__ ocnt, uint64_t out_cap)
{
    const uint64_t cap = 1ull << t.log2cap;
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t first = wave * (KDF_EXPORT_ROWS * 64);
    if (first >= cap) return;
    uint32_t mine = 0;
    if (!WRITE && min_count >= 1 && first + KDF_EXPORT_ROWS * 64 <= cap) {
        // count > 0 implies the slot is occupied: stream the counts array only, 16 B per lane
        const uint4 *c4 = (const uint4 *)(t.cnt + first);
#pragma unroll
        for (int r = 0; r < KDF_EXPORT_ROWS / 4; ++r) {
            const uint4 v = c4[r * 64 + lane];
            mine += (v.x >= min_count) + (v.y >= min_count) + (v.z >= min_count) + (v.w >= min_count);
        }
    } else
#pragma unroll 4
    for (int r = 0; r < KDF_EXPORT_ROWS; ++r) {
        const uint64_t i = first + (uint64_t)r * 64 + lane;
        if (i < cap) {
            if (min_count >= 1) {          // count > 0 implies the slot is occupied: counts array only
                mine += t.cnt[i] >= min_count ? 1u : 0u;
            } else {
                const bool occ = KW == 1 ? (t.lo[i] != KDF_EMPTY) : (t.hi[i] != KDF_EMPTY);
                mine += occ ? 1u : 0u;
            }
        }
    }
    uint32_t tot = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    if (tot == 0) return;
    if (!WRITE) {      // counting pass: no positions needed, spread the adds over 64 lines
        if (lane == 0) atomicAdd(&ctl->tally[(uint32_t)(wave % KDF_SHARDS) * 16], (unsigned long long)tot);
        return;
    }
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&ctl->cursor, (unsigned long long)tot);
    base = __shfl(base, 0);
    for (int r = 0; r < KDF_EXPORT_ROWS; ++r) {
        const uint64_t i = first + (uint64_t)r * 64 + lane;
        bool keep = false; uint64_t lo = 0, hi = 0; uint32_t c = 0;
        if (i < cap) {
            lo = t.lo[i];
            if (KW == 2) hi = t.hi[i];
            const bool occ = KW == 1 ? (lo != KDF_EMPTY) : (hi != KDF_EMPTY);
            c = t.cnt[i];
            keep = occ && c >= min_count;
        }
        const unsigned long long b = __ballot(keep);
        if (keep) {
            const uint64_t pos = base + __popcll(b & ((1ull << lane) - 1));
            if (pos < out_cap) {
                olo[pos] = kdf_key_lo(lo, hi);                       // the key back from its stored form
                if (KW == 2 && ohi) ohi[pos] = hi;
                if (ocnt) ocnt[pos] = c;
            }
        }
        base += __popcll(b);
    }
}

// dump -L into device buffers, narrow keys, min_count >= 1: ONE read of the table.  A wave takes 16 rows of 64 slots;
// all 32 loads (keys + counts) are issued before anything is used, the kept entries are counted with ballots, the
// wave reserves its output range with one atomic and writes.  (The two-phase kernel above reads the counts twice and
// runs at half the memory rate; it stays for wide keys, min_count = 0 and the owner-grouped dump.)
#define KDF_EXPORT1_ROWS 16
#define KDF_EXPORT1_THREADS 1024
template <int KW>
__global__ __launch_bounds__(KDF_EXPORT1_THREADS) void kdf_export1_kernel(KdfTable t, uint32_t min_count, KdfCtl *ctl, uint64_t *__restrict__ olo,
                                                                         uint64_t *__restrict__ ohi, uint32_t *__restrict__ ocnt, uint64_t out_cap)
{
    // one atomic per WORKGROUP (16 K slots): a same-address returning atomic per wave was what bounded the dump
    __shared__ uint32_t wtot[KDF_EXPORT1_THREADS / 64];
    __shared__ unsigned long long wg_base;
    constexpr int ROWS = KW == 1 ? KDF_EXPORT1_ROWS : KDF_EXPORT1_ROWS / 2;     // wide keys: 5 registers per slot
    const uint64_t cap = 1ull << t.log2cap;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * (KDF_EXPORT1_THREADS / 64) + wv;
    const uint64_t first = wave * (ROWS * 64);
    uint64_t lo[ROWS], hi[KW == 2 ? ROWS : 1]; uint32_t c[ROWS];
    unsigned long long kb[ROWS]; uint32_t tot = 0;
    if (KW == 1 && min_count >= 1) {
        // a count > 0 implies an occupied slot: read the counts first and the keys only where they are kept (a `dump -L 3`
        // keeps a fifth of the slots: the memory system fetches the key sectors that hold at least one kept slot)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) { const uint64_t i = first + (uint64_t)r * 64 + lane; c[r] = i < cap ? t.cnt[i] : 0u; }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const uint64_t i = first + (uint64_t)r * 64 + lane;
            const bool keep = c[r] >= min_count;
            lo[r] = keep ? t.lo[i] : KDF_EMPTY;
            kb[r] = __ballot(keep); tot += (uint32_t)__popcll(kb[r]);
        }
    } else {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint64_t i = first + (uint64_t)r * 64 + lane;
        const bool in = i < cap;
        c[r] = in ? t.cnt[i] : 0u;
        lo[r] = in ? t.lo[i] : KDF_EMPTY;
        if constexpr (KW == 2) hi[r] = in ? t.hi[i] : KDF_EMPTY;
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const bool occ = KW == 1 ? (lo[r] != KDF_EMPTY) : (hi[r] != KDF_EMPTY);
        kb[r] = __ballot(c[r] >= min_count && occ); tot += (uint32_t)__popcll(kb[r]);
    }
    }
    if (lane == 0) wtot[wv] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int i = 0; i < KDF_EXPORT1_THREADS / 64; ++i) { const uint32_t v = wtot[i]; wtot[i] = acc; acc += v; }
        wg_base = acc ? atomicAdd(&ctl->cursor, (unsigned long long)acc) : 0ull;
    }
    __syncthreads();
    unsigned long long base = wg_base + wtot[wv];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        if ((kb[r] >> lane) & 1) {
            const uint64_t pos = base + __popcll(kb[r] & ((1ull << lane) - 1));
            if (pos < out_cap) { olo[pos] = kdf_key_lo(lo[r], KW == 2 ? hi[r] : 0); if (KW == 2 && ohi) ohi[pos] = hi[r]; if (ocnt) ocnt[pos] = c[r]; }
        }
        base += __popcll(kb[r]);
    }
}

// ---------------------------------------------------------------------------
// count --if through a membership sieve.  In the parent-filter / VCF stages almost every window MISSES the filter
// (discovery/pipeline.py:377-443: a whole parent's reads against the child's candidate k-mers), so partitioning
// every window (binned path) or probing the hash table for every window (direct path) is wasted work.  The filter
// keys are folded into a blocked Bloom filter (two bits inside ONE 64-bit word per key; 16-32 bits per key, so it
// lives in L2 / the Infinity Cache); a window costs its canonical k-mer, one hash and ONE word load, and only the
// survivors (hits + a 0.4-1.4 % false-positive share) probe the table -- densely, 64 at a time from a wave-private
// LDS queue (ballot + mbcnt, no atomics, no barrier), so the rare slow path runs with every lane busy.
struct KdfSieve { const uint64_t *words; uint64_t wmask; };

__device__ __forceinline__ void kdf_sieve_bits(uint64_t hsh, uint64_t wmask, uint64_t &word, uint64_t &bits) {
    word = (hsh >> 12) & wmask;
    bits = (1ull << (hsh & 63)) | (1ull << ((hsh >> 6) & 63));
}

template <int KW>
__global__ __launch_bounds__(256) void kdf_sieve_build_kernel(const uint64_t *__restrict__ klo, const uint64_t *__restrict__ khi, uint64_t n,
                                                             uint64_t *__restrict__ words, uint64_t wmask) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t w, b;
    kdf_sieve_bits(kdf_hash(klo[i], KW == 2 ? khi[i] : 0), wmask, w, b);
    atomicOr((unsigned long long *)&words[w], (unsigned long long)b);
}

// the sieve over the keys the (hash-layout) table holds NOW: an index that was loaded with kdf_add_pairs or counted has
// none (kdf_load_filter builds one from the key list)
template <int KW>
__global__ __launch_bounds__(256) void kdf_sieve_from_table_kernel(KdfTable t, uint64_t *__restrict__ words, uint64_t wmask) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1ull << t.log2cap)) return;
    const uint64_t lo = t.lo[i], hi = KW == 2 ? t.hi[i] : 0;
    if ((KW == 1 ? lo : hi) == KDF_EMPTY) return;
    uint64_t w, b;
    kdf_sieve_bits(lo, wmask, w, b);                                // the slot holds the hash
    atomicOr((unsigned long long *)&words[w], (unsigned long long)b);
}

#define KDF_SV_WQ 128                     // queue entries per wave (drained 64 at a time)
#define KDF_SV_LDS_WORDS 8192             // a sieve of up to 64 KB is copied into LDS by every (persistent) workgroup:
                                          // filters of up to 64 K keys (VCF mode, Module 3) then cost no L2 request per window
// SCAN: the Module-3 probe (kdf_scan_reads_dev) through the same sieve: a survivor that is stored with count > 0 sets its
// window's bit in hit_bits (zeroed by the host first); nothing is counted.
template <int KW, bool IN_LDS = false, bool SCAN = false>
__global__ __launch_bounds__(KB_THREADS) void kdf_sieve_count_kernel(
    const uint64_t *__restrict__ packed, const uint64_t *__restrict__ invalid, uint64_t n_tiles, uint64_t n_bases, int k,
    KdfTable t, KdfCtl *ctl, KdfSieve sv, uint32_t slabs_per_wg, unsigned long long *__restrict__ hit_bits = nullptr)
{
    constexpr int WPT = KbCfg<KW>::WPT, TPT = 64 / WPT;
    constexpr uint32_t TILES_PER_SLAB = KB_THREADS / TPT;
    __shared__ uint64_t qlo[(KB_THREADS / 64) * KDF_SV_WQ];
    __shared__ uint64_t qhi[KW == 2 ? (KB_THREADS / 64) * KDF_SV_WQ : 1];
    __shared__ uint64_t lsv[IN_LDS ? KDF_SV_LDS_WORDS : 1];
    __shared__ uint32_t qpos[SCAN ? (KB_THREADS / 64) * KDF_SV_WQ : 1];       // SCAN: stream position of the queued window (< 2^32: host-checked)
    uint32_t *wqpos = qpos + (SCAN ? (threadIdx.x >> 6) * KDF_SV_WQ : 0);
    if constexpr (IN_LDS) {
        for (uint32_t i = threadIdx.x; i <= (uint32_t)sv.wmask; i += KB_THREADS) lsv[i] = sv.words[i];
        __syncthreads();
    }
    const uint64_t *const svw = IN_LDS ? lsv : sv.words;
    uint64_t *wqlo = qlo + (threadIdx.x >> 6) * KDF_SV_WQ, *wqhi = qhi + (KW == 2 ? (threadIdx.x >> 6) * KDF_SV_WQ : 0);
    const int lane = threadIdx.x & 63;
    uint32_t wq_n = 0, nwin = 0, claimed = 0;
    bool full = false;
    // probe the table for 64 queued keys (or the rest): every lane has a key
    auto drain = [&](uint32_t from, uint32_t cnt) {
        const bool todo = (uint32_t)lane < cnt;
        const uint64_t klo = todo ? wqlo[from + lane] : 0, khi = (KW == 2 && todo) ? wqhi[from + lane] : 0;
        if constexpr (SCAN) {
            if (todo) {
                const uint64_t sl = KW == 1 ? kdf_find_narrow(t, klo) : kdf_find_wide(t, klo, khi);
                if (sl != ~0ull && t.cnt[sl] != 0) { const uint32_t p = wqpos[from + lane]; atomicOr(&hit_bits[p >> 6], 1ull << (p & 63)); }
            }
        } else {
            const uint64_t slot = kdf_home(t, klo);              // the queue holds stored forms
            if constexpr (KW == 1) { if (todo && !kdf_add_narrow<false>(t, klo, 1u, slot, t.lo[slot], claimed)) full = true; }
            else { if (!kdf_add_wide<false>(t, todo, klo, khi, 1u, slot, claimed)) full = true; }
        }
    };
    const uint64_t slab0 = (uint64_t)blockIdx.x * slabs_per_wg;
    for (uint32_t sl = 0; sl < slabs_per_wg; ++sl) {
        if ((slab0 + sl) * TILES_PER_SLAB >= n_tiles) break;
        const uint64_t tile = (slab0 + sl) * TILES_PER_SLAB + threadIdx.x / TPT;
        KbWindows<KW> win;
        win.load(packed, invalid, tile, n_tiles, n_bases, threadIdx.x % TPT, k);
        nwin += __popc(win.valid);
        // eight sieve words in flight per lane; only the word and 12 hash bits are kept per window (the key of a
        // survivor is taken again from the registers that hold the stream), so eight waves fit a SIMD
        constexpr int HB = WPT < 8 ? WPT : 8;
#pragma unroll
        for (int u0 = 0; u0 < WPT; u0 += HB) {
            uint64_t w[HB]; uint32_t hb[HB];
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                uint64_t hsh, hi; win.stored(u0 + u, hsh, hi);
                hb[u] = (uint32_t)hsh & 0xFFFu;
                // only VALID windows ask for their sieve word: the kernel runs at the L2's request rate, and
                // 22 % of the window slots of 150 bp reads are invalid (N, read ends) -- 420 M of 2 031 M requests per parent
                w[u] = 0;
                if ((win.valid >> (u0 + u)) & 1) w[u] = svw[(hsh >> 12) & sv.wmask];
            }
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                const bool ok = ((win.valid >> (u0 + u)) & 1) && (((w[u] >> (hb[u] & 63)) & (w[u] >> (hb[u] >> 6)) & 1ull) != 0);
                const unsigned long long mk = __ballot(ok);
                if (mk) {
                    const uint32_t at = wq_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
                    if (ok) {
                        uint64_t lo, hi; win.stored(u0 + u, lo, hi); wqlo[at] = lo; if constexpr (KW == 2) wqhi[at] = hi;
                        if constexpr (SCAN) wqpos[at] = (uint32_t)(tile * 64 + (threadIdx.x % TPT) * WPT + u0 + u);
                    }
                    wq_n += (uint32_t)__popcll(mk);
                    if (wq_n >= 64) { wq_n -= 64; drain(wq_n, 64); }        // (wave-uniform)
                }
            }
        }
    }
    if (wq_n) drain(0, wq_n);
    if (full) atomicOr(&ctl->error, 1u);
    if constexpr (!SCAN) kdf_shard_add(ctl->windows, nwin);
}

// long keys through the same sieve (option "long_sieve")
#include "kdf_long_sieve.h"
// k <= 63 behind kernel A through a sieve laid out bin-major (option "sieve_bins")
#include "kdf_binsieve.h"

__global__ void kdf_ctl_reduce_kernel(KdfCtl *ctl, unsigned long long *out3) {
    // out3 = {distinct, windows, error}; single wave
    unsigned long long d = ctl->distinct[threadIdx.x * 16], w = ctl->windows[threadIdx.x * 16], y = ctl->tally[threadIdx.x * 16];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { d += __shfl_down(d, o); w += __shfl_down(w, o); y += __shfl_down(y, o); }
    if (threadIdx.x == 0) { out3[0] = d; out3[1] = w; out3[2] = ctl->error; out3[3] = ctl->cursor + y; }
}

// ===========================================================================
// engine
// ===========================================================================

thread_local std::string g_err;

int fail(kdf_engine *h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (h) h->err = buf; else g_err = buf;
    return code;
}

// slots needed so that n keys sit at load <= 0.5 (narrow: 8192-slot buckets,
// wide: 4096-slot buckets = what one workgroup can hold in LDS)
static uint32_t cap_log2_for(uint64_t n_keys) {
    uint32_t l = log2ceil(std::max<uint64_t>(n_keys, 1) * 2);
    return std::max<uint32_t>(l, 10);
}

// bucket bits of a table of 2^log2cap slots: 48 / 40 KB of LDS per bucket; tables of 2^big_bucket_log2cap slots and more:
// twice that (kdf_binned.h: KB_C_CT_BIG)
static uint32_t bucket_bits_for(const kdf_engine *h, uint32_t log2cap) {
    return std::min<uint32_t>(log2cap, KB_BB_SMALL(h->kw) + (log2cap >= h->opt_big_bucket_log2cap ? 1u : 0u));
}

// A table of 2^log2cap slots that is not the engine's yet: its arrays and the view of them.  It frees itself unless
// table_adopt takes it.
struct NewTable { TableMem mem; KdfTable t{}; };

static int table_alloc(kdf_engine *h, uint32_t log2cap, NewTable &nt, bool clear = true) {
    const uint64_t cap = 1ull << log2cap;
    KdfTable &t = nt.t;
    t = KdfTable{};
    hipError_t e = nt.mem.lo.alloc(cap * 8);
    if (e == hipSuccess && h->kw >= 2) e = nt.mem.hi.alloc(cap * 8 * (h->kw - 1));   // long keys: words 1 .. W-1
    if (e == hipSuccess) e = nt.mem.cnt.alloc(cap * 4);
    if (e != hipSuccess) {
        nt.mem = TableMem{};
        return fail(h, e == hipErrorOutOfMemory ? KDF_ERR_NOMEM : KDF_ERR_HIP,
                    "a table of 2^%u slots (%.1f GB) does not fit the device (%s): count the sample in key-space "
                    "slices (option key_parts / key_part; KDF_KEY_PARTS for the child count)",
                    log2cap, (double)cap * (8.0 * h->kw + 4.0) / 1e9, hipGetErrorString(e));
    }
    t.lo = nt.mem.lo.as<uint64_t>(); t.hi = nt.mem.hi.as<uint64_t>(); t.cnt = nt.mem.cnt.as<uint32_t>();
    t.log2cap = log2cap;
    t.bucket_bits = bucket_bits_for(h, log2cap);
    t.hshift = h->opt_hash_shift;
    if (!clear) return KDF_OK;                       // the caller keeps the engine's deferred-clear flag set
    HIPCHK(h, hipMemsetAsync(t.lo, 0xFF, cap * 8, h->stream));
    if (h->kw >= 2) HIPCHK(h, hipMemsetAsync(t.hi, 0xFF, cap * 8 * (h->kw - 1), h->stream));
    HIPCHK(h, hipMemsetAsync(t.cnt, 0, cap * 4, h->stream));
    return KDF_OK;
}
// nt becomes the engine's table; the old one is freed (the caller has drained the stream that may still read it)
static void table_adopt(kdf_engine *h, NewTable &nt) {
    h->t_mem = std::move(nt.mem);
    h->t = nt.t; h->t.key_parts = h->opt_key_parts; h->t.key_part = h->opt_key_part;
    h->cap = 1ull << h->t.log2cap;
}

// kdf_clear defers the 12 B/slot memset: a binned insert into an empty table
// rewrites every bucket anyway.  Everything else calls this first.
int materialize(kdf_engine *h) {
    if (!h->lazy_empty) return KDF_OK;
    HIPCHK(h, hipMemsetAsync(h->t.lo, 0xFF, h->cap * 8, h->stream));
    if (h->kw >= 2) HIPCHK(h, hipMemsetAsync(h->t.hi, 0xFF, h->cap * 8 * (h->kw - 1), h->stream));
    HIPCHK(h, hipMemsetAsync(h->t.cnt, 0, h->cap * 4, h->stream));
    h->lazy_empty = false;
    return KDF_OK;
}

// Room for `bytes` in one of the engine's buffers whose readers all run on the engine's stream (staging, binned scratch,
// merge scratch, hit reduction): slack(bytes) are allocated (the site's rule), the stream is drained before a free.
// what: the buffer's name in the message of a failed allocation (NULL: the plain HIP error text).
int eng_reserve(kdf_engine *h, DevBuf &b, size_t bytes, size_t (*slack)(size_t), const char *what) {
    const size_t want = slack(bytes);
    const hipError_t e = dev_reserve(b, bytes, want, [&] { (void)hipStreamSynchronize(h->stream); return hipSuccess; });
    if (e == hipSuccess) return KDF_OK;
    const int code = e == hipErrorOutOfMemory ? KDF_ERR_NOMEM : KDF_ERR_HIP;
    if (!what) return fail(h, code, "hipMalloc of %zu bytes of device scratch failed: %s", want, hipGetErrorString(e));
    return fail(h, code, "the %s of the hit reduction (%.2f GB) does not fit the device (%s)", what, (double)want / 1e9, hipGetErrorString(e));
}

// read distinct / windows / error from the control block (synchronises)
static int ctl_sync(kdf_engine *h, bool *table_full, uint64_t *cursor = nullptr) {
    hipLaunchKernelGGL(kdf_ctl_reduce_kernel, dim3(1), dim3(64), 0, h->stream, h->ctl, h->d_out4);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->h_out4, h->d_out4, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->distinct = h->h_out4[0];
    h->windows = h->h_out4[1];
    if (table_full) *table_full = h->h_out4[2] != 0;
    if (cursor) *cursor = h->h_out4[3];
    return KDF_OK;
}

static int ctl_reset(kdf_engine *h, bool keep_windows) {
    if (keep_windows) {
        HIPCHK(h, hipMemsetAsync(h->ctl->distinct, 0, sizeof(h->ctl->distinct), h->stream));
        HIPCHK(h, hipMemsetAsync(h->ctl->tally, 0, sizeof(h->ctl->tally) + 16, h->stream));
    } else {
        HIPCHK(h, hipMemsetAsync(h->ctl, 0, sizeof(KdfCtl), h->stream));
    }
    return KDF_OK;
}

// the sieve no longer describes the table (keys joined it, it was cleared, a new filter, other sizing options)
static void bin_sieve_drop(kdf_engine *h) { h->bsv.valid = false; h->bsv.unfit = false; }
static void sieve_drop(kdf_engine *h) { h->sieve.valid = false; h->sieve.unfit = false; bin_sieve_drop(h); }

// Insert-or-add n keys into table t, adding add[i] (NULL: 0).  Caller keys (stored = false) are the (lo, hi) arrays of
// k <= 63 or the row-major W-word rows at lo of long keys; stored = true: lo / hi are the arrays of the live table,
// which is being rehashed into t.  (A launch holds fewer than 2^32 threads: it goes in pieces of 2^30 keys.)
static void insert_keys(kdf_engine *h, const KdfTable &t, const uint64_t *lo, const uint64_t *hi, const uint32_t *add,
                        uint64_t n, bool stored) {
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        for (uint64_t off = 0; off < n; off += 1ull << 30) {
            const uint64_t m = std::min<uint64_t>(1ull << 30, n - off);
            const unsigned blocks = (unsigned)((m + 255) / 256);
            const uint32_t *a = add ? add + off : nullptr;
            if constexpr (W <= 2) {
                hipLaunchKernelGGL(kdf_insert_keys_kernel<W>, dim3(blocks), dim3(256), 0, h->stream, lo + off,
                                   W == 2 ? hi + off : nullptr, a, m, t, h->ctl, (int)stored, (int)stored);
            } else {
                // word j of key i: src[i * rs + j * ws] (kdf_long_read_key)
                const uint64_t rs = stored ? 1 : W, ws = stored ? h->cap : 1;
                const uint64_t *up = stored ? hi : lo + 1;
                hipLaunchKernelGGL(kdf_long_insert_kernel<W>, dim3(blocks), dim3(256), 0, h->stream, lo + off * rs, up + off * rs,
                                   rs, ws, a, m, t, h->ctl, (int)stored, long_top_bits(h));
            }
        }
        return 0;
    });
}

// rehash the live table into one with 2^new_log2 slots
static int table_rehash(kdf_engine *h, uint32_t new_log2) {
    // (the window counter lives on the device between synchronisations: pending partition passes have added to it)
    { int rc0 = ctl_sync(h, nullptr); if (rc0) return rc0; }
    if (h->lazy_empty || h->distinct == 0) {              // nothing to carry over: a new table (a lazily cleared one stays so)
        NewTable nt0;
        int rc0 = table_alloc(h, new_log2, nt0, !h->lazy_empty);
        if (rc0) return rc0;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        table_adopt(h, nt0);
        return KDF_OK;
    }
    NewTable nt;
    int rc = table_alloc(h, new_log2, nt);
    if (rc) return rc;
    const uint64_t windows = h->windows;
    rc = ctl_reset(h, false);
    if (rc) return rc;
    insert_keys(h, nt.t, h->t.lo, h->t.hi, h->t.cnt, h->cap, true);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, KDF_ERR_HIP, "rehash launch failed: %s", hipGetErrorString(e));
    bool full = false;
    rc = ctl_sync(h, &full);
    if (rc) return rc;
    if (full) return fail(h, KDF_ERR_TABLE_FULL, "rehash: bucket overflow at 2^%u slots", new_log2);
    table_adopt(h, nt);
    // restore the window counter (host-side accumulation)
    h->windows = windows;
    HIPCHK(h, hipMemcpyAsync(&h->ctl->windows[0], &h->windows, 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return KDF_OK;
}

// The one launcher of the thread-per-tile stream kernels (kdf_tilewalk.h).  A launch holds fewer than 2^32 threads, so
// the stream goes in pieces of at most 2^30 tiles; a piece is a stream of its own that starts at tile t0 and ends where
// the whole stream ends.  launch(W, blocks, packed, invalid, n_tiles, n_bases, per_tile) starts the kernel of the
// engine's key width W on one piece; per_tile: the hit / admit words of the stream, one per tile (may be NULL).
// n_tiles may be fewer than the tiles of n_bases: the stream then goes on behind what is walked (direct_insert).
template <typename F>
static void launch_tiles(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_tiles, uint64_t n_bases,
                         uint64_t *per_tile, F &&launch) {
    by_words(h, [&](auto Wc) {
        for (uint64_t t0 = 0; t0 < n_tiles; t0 += 1ull << 30) {
            const uint64_t m = std::min<uint64_t>(1ull << 30, n_tiles - t0);
            launch(Wc, (unsigned)((m + 255) / 256), d_packed + 2 * t0, d_invalid + t0, m, n_bases - t0 * KDF_TILE,
                   per_tile ? per_tile + t0 : nullptr);
        }
        return 0;
    });
}

template <int MODE>
static void launch_stream(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_tiles, uint64_t n_bases,
                          uint64_t *d_hits) {
    EvSpan span(h->timer[T_STREAM], h->prof, h->stream, n_tiles);
    launch_tiles(h, d_packed, d_invalid, n_tiles, n_bases, d_hits,
                 [&](auto Wc, unsigned blocks, const uint64_t *p, const uint64_t *m, uint64_t nt, uint64_t nb, uint64_t *hits) {
        constexpr int W = decltype(Wc)::value;
        if constexpr (W <= 2)
            hipLaunchKernelGGL((kdf_stream_kernel<W, MODE>), dim3(blocks), dim3(256), 0, h->stream,
                               p, m, nt, nb, h->k, h->t, h->ctl, hits);
        else
            hipLaunchKernelGGL((kdf_long_stream_kernel<W, MODE>), dim3(blocks), dim3(256), 0, h->stream,
                               p, m, nt, nb, h->k, h->t, h->ctl, hits);
    });
    span.stop();
}

// fold the finished stage records of the binned path into the running totals (synchronises on them)
static void stage_collect(kdf_engine *h) {
    for (auto &ev : h->prof_stage_ev) {
        if (ev.size() == 4) {                                     // a partition pass: A0, A1, B
            (void)hipEventSynchronize(ev[3]);
            bool ok = true; float ms[3];
            for (int i = 0; i < 3; ++i) ok = ok && hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) == hipSuccess;
            if (ok) { for (int i = 0; i < 3; ++i) h->prof_stage_ms[i] += ms[i]; h->prof_stage_passes++; }
        } else if (ev.size() == 2) {                              // a flush: kernel C over the pending passes
            (void)hipEventSynchronize(ev[1]);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) h->prof_stage_ms[3] += ms;
        }
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    h->prof_stage_ev.clear();
}

// ---------------------------------------------------------------------------
// binned path (kdf_binned.h): partition passes into the entry ring, deferred kernel C

// the partition geometry for a table: coarse / fine bits; sub_bits = what the bucket kernel resolves itself
static KbPlan kb_make_plan(const kdf_engine *h, const KdfTable &t) {
    KbPlan p{};
    p.log2cap = t.log2cap; p.bucket_bits = t.bucket_bits;
    const uint32_t nb_bits = t.log2cap - t.bucket_bits;
    // 8 + 8 bits while that resolves the table; then the FINE radix widens first (8 + 9: the piece sort gathers 512-byte
    // runs instead of 256-byte ones and ranks into 512 bins; the bucket kernel pays with twice the runs of half the
    // length -- measured at bench size, 9 + 8 / 8 + 9 / 10 + 7: piece sort 4.74 / 4.21 / 5.88 ms, bucket kernel 4.40 / 4.79 / 4.20,
    // pass 12.35 / 12.16 / 13.60), then the coarse one (9 + 9, 10 + 9)
    p.c2 = std::min<uint32_t>(KB_F_BITS, nb_bits);
    p.c1 = std::min<uint32_t>(8, nb_bits - p.c2);
    if (p.c1 + p.c2 < nb_bits) p.c2 = std::min<uint32_t>(9, nb_bits - p.c1);               // fine runs halve: still >= 240 B
    if (p.c1 + p.c2 < nb_bits) p.c1 = std::min<uint32_t>(KB_C1_MAX, nb_bits - p.c2);      // coarse runs halve
    // (beyond 2^19 buckets kernel C reads every run once per sub-bucket: 10 fine bits -- 16-entry runs -- measured worse,
    // 9.65 against 8.86 ms per 10 M reads into 2^32 slots)
    if (const char *ev = getenv("KDF_C1")) {                       // (experiments: another split of the same bits)
        const uint32_t c1 = (uint32_t)atoi(ev);
        if (c1 <= KB_C1_MAX && c1 <= nb_bits && nb_bits - c1 <= KB_F_BITS_MAX) { p.c1 = c1; p.c2 = nb_bits - c1; }
    }
    p.sub_bits = nb_bits - p.c1 - p.c2;
    p.off_stride = (1u << p.c2) + 1;
    // Slabs per group: a piece (bin x group) is ~0.93 CHUNK entries.  Windows per stream position: what this engine has
    // seen so far (150 bp reads at k = 31: 0.78), 1 before its first flush; a pass that turns out denser only gets some
    // pairs of two pieces (kb_piecesort_more_kernel).
    const uint64_t chunk = h->kw == 1 ? KbCfg<1>::CHUNK : KbCfg<2>::CHUNK, slab = h->kw == 1 ? KbCfg<1>::SLAB : KbCfg<2>::SLAB;
    double dens = 1.0;
    if (h->dens_positions >= (1u << 20)) dens = std::min(1.0, std::max(0.05, 1.03 * (double)h->dens_windows / (double)h->dens_positions));
    // (0.98 of a piece's capacity, on a density taken 3 % high: pieces come out 95 % full -- 6 sigma below 16 K entries on
    // uniform input; measured 0.93 / 0.97 / 1.0 / 1.03: pass 12.48 / 12.29 / 12.25 / 13.12 ms, the last with overflow pieces)
    static const double fill = [] { const char *e = getenv("KDF_PIECE_FILL"); const double v = e ? atof(e) : 0.0; return v > 0.1 && v <= 1.2 ? v : 0.98; }();
    p.group = (uint32_t)std::min<double>(KB_G_MAX, std::max<double>(1.0, fill * (double)chunk * (double)((uint64_t)1 << p.c1) / ((double)slab * dens)));
    return p;
}

// Every instantiation of kernel C per key width, written once: f(MODE, VAR, BIG, DUMP, LAZY) -- integral constants, the
// template arguments of kb_bucket_kernel<KW, ..> -- is called for each in turn until it returns non-zero, which is returned
// (0: f took them all).  Insert, count --if and the fused dump, each plain (VAR 1) and skewed (VAR 2); the dump-only flush;
// all with small and with big buckets.  The order is the one the code object has always held them in (another order moves
// every kernel behind them).  The attribute setter walks them all, the launcher picks the one that matches: a variant that
// is launched has its LDS limit raised.
template <typename F>
static int kb_c_variants(F &&f) {
    using ins = std::integral_constant<int, KB_MODE_INSERT>; using flt = std::integral_constant<int, KB_MODE_FILTERED>;
    using no = std::false_type; using yes = std::true_type;
    int rc = 0;
    auto one = [&](auto mode, auto var, auto big, auto dump, auto lazy) { return (rc = f(mode, var, big, dump, lazy)) != 0; };
    auto each = [&](auto var) {
        return one(ins{}, var, no{}, no{}, no{}) || one(flt{}, var, no{}, no{}, no{}) || one(ins{}, var, yes{}, no{}, no{}) || one(flt{}, var, yes{}, no{}, no{}) ||
               one(ins{}, var, no{}, yes{}, no{}) || one(ins{}, var, yes{}, yes{}, no{});
    };
    const std::integral_constant<int, 1> v1{};
    (void)(each(v1) || each(std::integral_constant<int, 2>{}) || one(ins{}, v1, no{}, yes{}, yes{}) || one(ins{}, v1, yes{}, yes{}, yes{}));
    return rc;
}

template <int KW>
static int kb_set_lds_attrs(kdf_engine *h, size_t a, size_t b, size_t c, size_t hv) {
    HIPCHK(h, hipFuncSetAttribute((const void *)(kb_slabsort_kernel<KW, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a));
    HIPCHK(h, hipFuncSetAttribute((const void *)(kb_slabsort_kernel<KW, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a));
    HIPCHK(h, hipFuncSetAttribute((const void *)(kb_slabsort_gated_kernel<KW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a));
    HIPCHK(h, hipFuncSetAttribute((const void *)kb_piecesort_kernel<KW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b));
    HIPCHK(h, hipFuncSetAttribute((const void *)kb_piecesort_more_kernel<KW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b));
    HIPCHK(h, hipFuncSetAttribute((const void *)kb_piecesort_pipe_kernel<KW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b));
    const size_t cbig = KB_C_LDS(KW, KB_BB_SMALL(KW) + 1);
    if (const int rc = kb_c_variants([&](auto M, auto V, auto B, auto D, auto L) -> int {
            constexpr bool BIG = decltype(B)::value;
            HIPCHK(h, hipFuncSetAttribute((const void *)(kb_bucket_kernel<KW, decltype(M)::value, decltype(V)::value, BIG, decltype(D)::value, decltype(L)::value>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BIG ? cbig : c)));
            return KDF_OK;
        })) return rc;
    HIPCHK(h, hipFuncSetAttribute((const void *)kb_heavy_slice_kernel<KW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hv));
    HIPCHK(h, hipFuncSetAttribute((const void *)kb_heavy_combine_kernel<KW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hv));
    HIPCHK(h, hipFuncSetAttribute((const void *)kb_heavy_filtered_kernel<KW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hv));
    return KDF_OK;
}

// dynamic LDS of kernel A and of the piece sort
template <int KW> static constexpr size_t kb_lds_a() { return (size_t)(KbCfg<KW>::SLAB + 64) * 8 * KW + (size_t)(2 * ((1 << KB_C1_MAX) + 96)) * 4; }
template <int KW> static constexpr size_t kb_lds_b() { return (size_t)KbCfg<KW>::CHUNK * 8 * KW + (size_t)(2 * KB_F + 32) * 4 + (size_t)KB_G_MAX * 12 + 32; }
// the LDS limits of the binned path's kernels, raised once per engine and key width
template <int KW>
static int kb_ensure_attrs(kdf_engine *h) {
    if (h->kb.attrs_set[KW]) return KDF_OK;
    const size_t lds_c = KB_C_LDS(KW, KB_BB_SMALL(KW));
    if (const int rc = kb_set_lds_attrs<KW>(h, kb_lds_a<KW>(), kb_lds_b<KW>(), lds_c, ((size_t)(8 * KW + 4) << (KB_BB_SMALL(KW) + 1)) + KB_RI_LDS_BYTES)) return rc;
    h->kb.attrs_set[KW] = true;
    return KDF_OK;
}

// the small device arrays of the binned path, allocated once per engine; fills the pointers of `s` from the engine's buffers
static int kb_scratch(kdf_engine *h, KbScratch &s) {
    KbState &kb = h->kb;
    if (!kb.small) {
        HIPCHK(h, kb.small.alloc((16 + 64) * 8));
        HIPCHK(h, hipMemsetAsync(kb.small.p, 0, (16 + 64) * 8, h->stream));
    }
    if (!kb.totals_host) HIPCHK(h, kb.totals_host.alloc(16 * 8));
    if (!kb.pass) HIPCHK(h, kb.pass.alloc(sizeof(KbPass) * KB_MAX_PASS));
    const size_t hv_pairs = (size_t)KB_HV_MAX * KB_HV_SLICES << (KB_BB_SMALL(h->kw) + 1);   // (room for the buckets of big tables)
    const size_t hv_pair_bytes = 8 * (size_t)h->kw + 4;
    if (!kb.heavy) {                                              // heavy buckets of skewed flushes (kb_heavy_slice_kernel): ~200 MB, once
        HIPCHK(h, kb.heavy.alloc(hv_pairs * hv_pair_bytes + (4 + 3 * KB_HV_MAX) * 4));
        HIPCHK(h, hipMemsetAsync(kb.heavy.as<char>() + hv_pairs * hv_pair_bytes, 0, (4 + 3 * KB_HV_MAX) * 4, h->stream));
    }
    s = KbScratch{};
    s.totals = kb.small.as<unsigned long long>(); s.trash = (uint64_t *)(s.totals + 16);
    s.pass = kb.pass.as<KbPass>();
    if (kb.heavy) {
        s.hv_key = kb.heavy.as<uint64_t>();
        s.hv_khi = h->kw == 2 ? s.hv_key + hv_pairs : nullptr;
        s.hv_cnt = (uint32_t *)(s.hv_key + hv_pairs * h->kw);
        s.hv_ctr = s.hv_cnt + hv_pairs; s.hv_bucket = s.hv_ctr + 4; s.hv_n = s.hv_bucket + KB_HV_MAX; s.hv_failed = s.hv_n + KB_HV_MAX;
    }
    s.ent = h->kb.ent.as<uint64_t>(); s.tmp = h->kb.tmp.as<uint64_t>();
    s.chunk_off = h->kb.chunk_off.as<uint32_t>(); s.failed = h->kb.failed.as<uint32_t>();
    s.off = h->kb.off_rows.as<uint16_t>();
    // row tables of the ring: row_ent u64 | row_len u32, ring_rows of each
    s.row_ent = h->kb.row_tables.as<unsigned long long>();
    s.row_len = (uint32_t *)(s.row_ent + h->kb.ring.cap_rows);
    return KDF_OK;
}

// the ring is empty again: nothing pending, the flush-wide counters zeroed
static int kb_ring_reset(kdf_engine *h) {
    h->kb.ring.reset();
    if (h->kb.small) HIPCHK(h, hipMemsetAsync(h->kb.small.p, 0, 16 * 8, h->stream));
    return KDF_OK;
}

static int kb_flush_ring(kdf_engine *h, KbDump *dump = nullptr);

// Room for a pass of need_e entries (upper bound: its stream positions) in need_r pieces.  A full ring is applied to the
// table first; a ring that was too small for the pending passes plus this one grows (doubling, up to the budget) while
// it is empty.
static int kb_ring_make_room(kdf_engine *h, uint64_t need_e, uint64_t need_r, uint32_t off_stride) {
    int rc;
    const uint64_t rows_cap = std::min<uint64_t>(h->kb.ring.cap_rows, h->kb.chunk_off.bytes / ((uint64_t)off_stride * 4));
    bool forced = false;
    if (h->kb.ring.n_pass >= KB_MAX_PASS || h->kb.ring.used_entries + need_e > h->kb.ring.cap_entries || h->kb.ring.used_rows + need_r > rows_cap) {
        forced = !h->kb.ring.empty();
        if (forced && (rc = kb_flush_ring(h))) return rc;
    }
    const uint64_t esz = 8ull * h->kw;
    const uint64_t budget = h->opt_defer_max_bytes ? h->opt_defer_max_bytes : h->dev_total_bytes / 5 * 2;
    uint64_t want_e = h->kb.ring.cap_entries;
    // (at least 128 / 256 MB: small batches never force a flush; with deferral on, room for one more pass like this one)
    if (need_e > want_e) want_e = std::max<uint64_t>(h->opt_defer ? std::max<uint64_t>(need_e, std::min<uint64_t>(2 * need_e, budget / esz)) : need_e, 1ull << 24);
    if (forced && h->opt_defer && h->kb.ring.cap_entries * esz < budget)
        want_e = std::max<uint64_t>(want_e, std::min<uint64_t>(2 * h->kb.ring.cap_entries, std::max<uint64_t>(budget / esz, need_e)));
    // pieces: in proportion to the entries (passes of one sample look alike), and never fewer than this pass needs
    const uint64_t want_r = std::max<uint64_t>(need_r, (uint64_t)((double)need_r * ((double)want_e / (double)need_e))) + 4096;
    if (want_e > h->kb.ring.cap_entries || need_r > rows_cap) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if ((rc = eng_reserve(h, h->kb.ent, want_e * esz, slack_page))) return rc;
        if ((rc = eng_reserve(h, h->kb.chunk_off, want_r * (uint64_t)off_stride * 4, slack_page))) return rc;
        if ((rc = eng_reserve(h, h->kb.row_tables, want_r * 12, slack_page))) return rc;
        h->kb.ring.cap_entries = std::max(h->kb.ring.cap_entries, want_e); h->kb.ring.cap_rows = std::max(h->kb.ring.cap_rows, want_r);
        // (a buffer only ever grows: the row tables are laid out for ring_rows rows)
        if (h->kb.row_tables.bytes < h->kb.ring.cap_rows * 12) return fail(h, KDF_ERR_STATE, "entry ring: row tables out of step");
    }
    return KDF_OK;
}

// ONE partition pass (A, P, B) of a device-resident stream of at most opt_binned_max_positions positions into the ring
template <int KW>
static int kb_partition(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases, uint64_t n_end, bool filtered,
                        const uint64_t *admit) {
    constexpr int WPT = KbCfg<KW>::WPT, TPT = 64 / WPT, CHUNK = KbCfg<KW>::CHUNK, SLAB = KbCfg<KW>::SLAB;
    constexpr uint32_t TILES_PER_SLAB = KB_A_THREADS / TPT;
    const uint64_t n_tiles = (n_bases + KDF_TILE - 1) / KDF_TILE;
    if (n_tiles == 0) return KDF_OK;
    int rc;
    // pending passes must share their geometry, key slice and mode (kdf_set_option / a mode change flush first)
    if (!h->kb.ring.empty() && h->kb.ring.filtered != filtered && (rc = kb_flush_ring(h))) return rc;
    KbPlan plan = h->kb.ring.empty() ? kb_make_plan(h, h->t) : h->kb.ring.plan;
    if (h->kb.ring.empty()) { plan.key_parts = filtered ? 0 : h->t.key_parts; plan.key_part = h->t.key_part; }
    const int nbins = 1 << plan.c1;
    const uint64_t n_slabs = (n_tiles + TILES_PER_SLAB - 1) / TILES_PER_SLAB;
    const uint64_t n_groups = (n_slabs + plan.group - 1) / plan.group;
    const uint64_t n_entries_max = n_tiles * KDF_TILE;
    const uint64_t n_rows_max = n_groups * nbins + n_entries_max / CHUNK + 1;
    if (n_rows_max >= (1ull << 32) || n_slabs >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "binned pass: too many positions for one pass");
    if ((rc = kb_ring_make_room(h, n_entries_max, n_rows_max, plan.off_stride))) return rc;
    if (h->kb.ring.empty()) { h->kb.ring.plan = plan; h->kb.ring.filtered = filtered; }
    plan.dbg = h->opt_debug_flags;
    plan.n_slabs = (uint32_t)n_slabs; plan.n_groups = (uint32_t)n_groups;
    const int nb1 = 1 << KB_C1_MAX;
    const size_t lds_a = kb_lds_a<KW>(), lds_b = kb_lds_b<KW>();
    if ((rc = kb_ensure_attrs<KW>(h))) return rc;
    // the pass's own buffers: slab-sorted entries, offset rows, planning arrays (reused by the next pass: stream order)
    if ((rc = eng_reserve(h, h->kb.tmp, n_slabs * (uint64_t)SLAB * 8 * KW, slack_16th))) return rc;
    if ((rc = eng_reserve(h, h->kb.off_rows, n_slabs * (uint64_t)(nbins + 1) * 2 + 64, slack_16th))) return rc;
    const uint64_t n_pairs = n_groups * nbins;
    const uint64_t ovf_cap = n_entries_max / CHUNK + 1;       // pieces beyond the first of their pair: sum (np - 1) <= entries / CHUNK
    if ((rc = eng_reserve(h, h->kb.pass_plan, n_pairs * 16 + (size_t)nb1 * 12 + (2 * ovf_cap + 2) * 4 + 64, slack_16th))) return rc;
    KbScratch s;
    if ((rc = kb_scratch(h, s))) return rc;
    s.gpre_ent = h->kb.pass_plan.as<unsigned long long>();
    s.bin_ent = s.gpre_ent + n_pairs;
    s.gn = (uint32_t *)(s.bin_ent + nb1); s.gpre_row = s.gn + n_pairs; s.bin_rows = s.gpre_row + n_pairs; s.ovf = s.bin_rows + nb1;
    s.ovf_cap = (uint32_t)ovf_cap;

    StageStamps st(h->prof, h->stream);
    EvSpan span(h->timer[T_STREAM], h->prof, h->stream, n_tiles);
    st.stamp();                                                  // start of A

    const uint32_t pass_idx = h->kb.ring.n_pass;
    const bool sliced = plan.key_parts > 1;
    // A: a workgroup takes a few consecutive slabs (the next slab's words are prefetched under the current one)
    const uint32_t slabs_per_wg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(8, n_slabs / ((uint64_t)h->n_cu * 8)));
    const unsigned grid_a = (unsigned)((n_slabs + slabs_per_wg - 1) / slabs_per_wg);
    // (admit: the windows an armed prefilter lets through, one word per tile of this pass -- never together with a key slice)
    if (admit) hipLaunchKernelGGL((kb_slabsort_gated_kernel<KW>), dim3(grid_a), dim3(KB_A_THREADS), lds_a, h->stream, d_packed, d_invalid, n_tiles, n_end, h->k, plan, s, slabs_per_wg, admit);
    else if (sliced) hipLaunchKernelGGL((kb_slabsort_kernel<KW, true>), dim3(grid_a), dim3(KB_A_THREADS), lds_a, h->stream, d_packed, d_invalid, n_tiles, n_end, h->k, plan, s, slabs_per_wg);
    else hipLaunchKernelGGL((kb_slabsort_kernel<KW, false>), dim3(grid_a), dim3(KB_A_THREADS), lds_a, h->stream, d_packed, d_invalid, n_tiles, n_end, h->k, plan, s, slabs_per_wg);
    st.stamp();                                                // end of A
    hipLaunchKernelGGL(kb_groupsum_kernel, dim3((unsigned)n_groups, (unsigned)((nbins + 63) / 64)), dim3(256), 0, h->stream, plan, s);
    hipLaunchKernelGGL(kb_binscan_kernel<CHUNK>, dim3((unsigned)nbins), dim3(256), 0, h->stream, plan, s);
    hipLaunchKernelGGL(kb_binfirst_kernel, dim3(1), dim3(KB_THREADS), 0, h->stream, plan, s, pass_idx, (unsigned long long)h->kb.ring.used_entries,
                       (unsigned long long)h->kb.ring.used_rows, h->ctl);
    HIPCHK(h, hipGetLastError());
    st.stamp();                                                // end of the planning kernels
    // No host round trip: the pass's share of the ring is sized for one entry per position; B's first launch has one
    // workgroup per (group, bin) pair, its second walks the (usually empty) list of further pieces.
    // (debug flag 64: the one-piece-per-workgroup kernel of round 3's first half, for same-box comparisons)
    if (plan.dbg & 64) hipLaunchKernelGGL(kb_piecesort_kernel<KW>, dim3((unsigned)((n_pairs + 7) / 8 * 8)), dim3(KB_THREADS), lds_b, h->stream, plan, s, pass_idx);
    else hipLaunchKernelGGL(kb_piecesort_pipe_kernel<KW>, dim3((unsigned)std::max(8, h->n_cu / 8 * 8)), dim3(KB_THREADS), lds_b, h->stream, plan, s, pass_idx);
    hipLaunchKernelGGL(kb_piecesort_more_kernel<KW>, dim3((unsigned)std::min<uint64_t>(ovf_cap, (uint64_t)h->n_cu)), dim3(KB_THREADS), lds_b, h->stream, plan, s, pass_idx);
    st.stamp();                                                // end of B
    HIPCHK(h, hipGetLastError());
    span.stop();
    st.commit(h->prof_stage_ev);
    h->kb.ring.n_pass++;
    h->kb.ring.used_entries += n_entries_max; h->kb.ring.used_rows += n_rows_max;
    h->kb.ring.positions += n_entries_max;
    h->stat_binned_passes++;
    h->last_path = 1;
    return KDF_OK;
}

// tally (admit == NULL) or gate (admit[tile] written) over a device-resident stream
static void pf_launch(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases, uint64_t *admit) {
    launch_tiles(h, d_packed, d_invalid, kdf_stream_geom(n_bases).tiles, n_bases, admit,
                 [&](auto Wc, unsigned blocks, const uint64_t *p, const uint64_t *m, uint64_t nt, uint64_t nb, uint64_t *adm) {
        constexpr int W = decltype(Wc)::value;
#define PF_LAUNCH(KRN, G) hipLaunchKernelGGL((KRN<W, G>), dim3(blocks), dim3(256), 0, h->stream, p, m, nt, nb, h->k, h->pf.view, h->pf.ctr.as<unsigned long long>(), adm)
        if constexpr (W <= 2) { if (adm) PF_LAUNCH(kdf_pf_stream_kernel, true); else PF_LAUNCH(kdf_pf_stream_kernel, false); }
        else { if (adm) PF_LAUNCH(kdf_pf_long_kernel, true); else PF_LAUNCH(kdf_pf_long_kernel, false); }
#undef PF_LAUNCH
    });
}

// Armed: *admit = one word per tile of the stream, bit i = window i is valid and its cell reads >= min_count (stream
// order: the buffer is reused by the next gated stream).  Not armed: *admit = NULL, the count is not gated.
static int pf_gate(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases, const uint64_t **admit) {
    *admit = nullptr;
    if (h->pf.state != PF_ARMED || n_bases == 0) return KDF_OK;
    const uint64_t n_tiles = (n_bases + KDF_TILE - 1) / KDF_TILE;
    if (const int rc = eng_reserve(h, h->pf.admit, n_tiles * 8)) return rc;
    pf_launch(h, d_packed, d_invalid, n_bases, h->pf.admit.as<uint64_t>());
    HIPCHK(h, hipGetLastError());
    *admit = h->pf.admit.as<uint64_t>();
    return KDF_OK;
}

// partition a stream of any length: passes of at most opt_binned_max_positions
// positions, each starting on a tile boundary (windows that start in a pass may read on
// into the next tiles: the stream is one buffer)
static int kb_partition_stream(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases, bool filtered) {
    const uint64_t step = h->opt_binned_max_positions;
    const uint64_t *admit = nullptr;                      // armed prefilter: the gate runs once over the whole stream
    if (!filtered) { int rcg = pf_gate(h, d_packed, d_invalid, n_bases, &admit); if (rcg) return rcg; }
    for (uint64_t off = 0; off < n_bases; off += step) {
        const uint64_t len = std::min<uint64_t>(step, n_bases - off);
        const uint64_t *p = d_packed + off / 32, *m = d_invalid + off / 64;
        int rc = by_width(h, [&](auto KWc) { return kb_partition<decltype(KWc)::value>(h, p, m, len, n_bases - off, filtered, admit ? admit + off / 64 : nullptr); });
        if (rc) return rc;
    }
    return KDF_OK;
}

// ---- the flush: kernel C over every pending pass, the ring applied to the table and emptied -- in steps ------------------
// What a flush decides before it launches anything (kb_flush_choose)
struct KbChoice {
    bool redo;                    // passes a dump-only flush has applied (n_dumped) are applied AGAIN, dump-only or not: the table is
                                  // still empty, so the result is what the first application would have left
    bool skewed;                  // VAR 2 of kernel C ...
    bool heavy;                   // ... with the heavy-bucket kernels behind it, if the buckets are whole at the launch (sub_bits 0)
    bool grow_first;              // the table doubles before the launch
    bool dump_only;               // the dump and the counters are written, the table is not, and the passes stay in the ring
    uint64_t distinct_before;     // keys of the table the flush adds to
    double est;                   // ... and of the table afterwards, at the last flush's rate of new keys
};
// ... and what its steps hand on to each other
struct KbFlush {
    KbScratch s{};
    bool filtered = false;        // count --if passes
    uint64_t n_entries = 0;       // entries of the pending passes
    KbChoice c{};
    KbPlan plan{};                // the partition's geometry on the table as it is at the launch; dump_min: the dump kernel C writes
    uint64_t nb_table = 0;        // table buckets = workgroups of kernel C
    int nonempty = 1;             // 0: kernel C rewrites every bucket (this IS the clear)
};

// A table that grew since the partition has more buckets than the partition made: kernel C resolves the extra bits itself
static uint32_t kb_sub_bits_now(const kdf_engine *h) { return (h->t.log2cap - h->t.bucket_bits) - h->kb.ring.plan.c1 - h->kb.ring.plan.c2; }

// what the pending passes hold (entries, skew) and what the table holds now; the density accounting
static int kb_flush_totals(kdf_engine *h, KbFlush &f) {
    int rc;
    if ((rc = kb_scratch(h, f.s))) return rc;
    f.filtered = h->kb.ring.filtered;
    HIPCHK(h, hipMemcpyAsync(h->kb.totals_host.p, f.s.totals, 16 * 8, hipMemcpyDeviceToHost, h->stream));
    if ((rc = ctl_sync(h, nullptr))) return rc;
    f.n_entries = h->kb.total(0);
    h->dens_windows += f.n_entries - h->kb.ring.acct_entries; h->dens_positions += h->kb.ring.positions - h->kb.ring.acct_positions;
    h->kb.ring.acct_entries = f.n_entries; h->kb.ring.acct_positions = h->kb.ring.positions;
    return KDF_OK;
}

// Which flush this is: reads the engine and the totals, changes nothing.  dump_only_ok (a dump is waiting and would be this
// flush's only reader): the dump-only flush is allowed.
static KbChoice kb_flush_choose(const kdf_engine *h, const KbFlush &f, const KbDump *dump, bool dump_only_ok) {
    KbChoice c{};
    // passes a dump-only flush has applied: kernel C counts their keys again, so the counter restarts at 0 (the table is
    // empty) -- just before the launch (kb_flush_launch), after everything that can still fail or return
    c.redo = h->kb.ring.n_dumped > 0;
    c.skewed = h->kb.total(7) != 0 || (h->opt_debug_flags & 4096);          // (debug flag 4096 forces VAR 2: fuzzing)
    c.heavy = c.skewed && f.s.hv_ctr;
    c.distinct_before = c.redo ? 0 : h->distinct;
    // Grow BEFORE the flush when the last flush's rate of new keys says the pending entries will not fit: growing now
    // rehashes the smaller table, and kernel C resolves the extra bucket bits itself (sub_bits) -- no failed buckets, no
    // replay through the global-atomic path.  (First flush of a table: the caller's capacity hint is trusted.)
    c.est = (double)c.distinct_before + h->grow_ratio * (double)f.n_entries;
    c.grow_first = !f.filtered && h->grow_ratio > 0.0 && c.est > 0.6 * (double)h->cap && h->t.log2cap < 40;
    // the dump-only flush: everything that gates the fused dump, an empty table, passes no flush has seen, and nothing that
    // would send a bucket another way (skew: the heavy-bucket split; a table about to grow).  Counts of one key slice
    // (key_parts) and counts behind a prefilter keep the ordinary flush: their dumps are followed by reads of the table.
    // A table that grew since the partition (kb_sub_bits_now): a per-key test the dump-only instantiation leaves out: such
    // a table takes the ordinary flush.
    c.dump_only = dump_only_ok && h->opt_lazy_table && dump && dump->min_count && !f.filtered && h->lazy_empty && !c.skewed && !c.grow_first &&
                  kb_sub_bits_now(h) == 0 && h->kb.ring.undumped_passes() && h->kb.ring.plan.key_parts <= 1 && h->pf.state == PF_OFF &&
                  !(h->opt_debug_flags & 2048);
    return c;
}

// grow-first: the table doubles until est keys sit at load <= 0.6; a step that fails ends the growth, not the flush
static int kb_grow_first(kdf_engine *h, double est) {
    int rc;
    while (est > 0.6 * (double)h->cap && h->t.log2cap < 40) {
        if (h->lazy_empty) {                                  // nothing to carry over: a new table, still to be cleared
            NewTable nt;
            if ((rc = table_alloc(h, h->t.log2cap + 1, nt, false))) break;       // (no room: kernel C will tell what really overflows)
            HIPCHK(h, hipStreamSynchronize(h->stream));
            table_adopt(h, nt);
        } else if ((rc = table_rehash(h, h->t.log2cap + 1))) { (void)hipGetLastError(); h->err.clear(); break; }
    }
    return KDF_OK;
}

// the plan of kernel C on the table as it is now, the dump it writes and the bitmap of failed buckets
static int kb_flush_prepare(kdf_engine *h, KbFlush &f, const KbDump *dump) {
    int rc;
    if (f.filtered && (rc = materialize(h))) return rc;
    f.plan = h->kb.ring.plan;
    f.plan.n_pass = h->kb.ring.n_pass; f.plan.dbg = h->opt_debug_flags;
    f.plan.log2cap = h->t.log2cap; f.plan.bucket_bits = h->t.bucket_bits;
    // a dump is waiting for this flush: kernel C writes it out of the buckets it holds
    if (dump && !f.filtered && dump->min_count) {
        f.plan.dump_min = dump->min_count;
        f.s.dump_lo = dump->lo; f.s.dump_hi = dump->hi; f.s.dump_cnt = dump->cnt; f.s.dump_cap = dump->cap;
        HIPCHK(h, hipMemsetAsync(h->ctl->tally, 0, sizeof(h->ctl->tally) + 8, h->stream));   // tally[] + cursor: ctl_sync reports their sum (a kdf_count_ge before this leaves its tally behind)
    }
    f.plan.sub_bits = kb_sub_bits_now(h);             // a table that grew since the partition (just now, perhaps): more sub-buckets
    f.nb_table = 1ull << (f.plan.c1 + f.plan.c2 + f.plan.sub_bits);
    const size_t failed_bytes = (size_t)((f.nb_table + 31) / 32) * 4;
    if ((rc = eng_reserve(h, h->kb.failed, failed_bytes, slack_16th))) return rc;
    f.s.failed = h->kb.failed.as<uint32_t>();
    HIPCHK(h, hipMemsetAsync(f.s.failed, 0, failed_bytes, h->stream));
    f.nonempty = h->lazy_empty ? 0 : 1;
    return KDF_OK;
}

// kernel C -- the one of kb_c_variants this flush chose -- and, for a skewed flush, the heavy-bucket kernels
static int kb_flush_launch(kdf_engine *h, const KbFlush &f) {
    const KbPlan &plan = f.plan;
    const KbScratch &s = f.s;
    StageStamps st(h->prof, h->stream);
    EvSpan span(h->timer[T_STREAM], h->prof, h->stream, 0);      // (tag 0: its positions were counted with the partition passes)
    st.stamp();
    const bool heavy = f.c.heavy && plan.sub_bits == 0;
    if (heavy) {
        HIPCHK(h, hipMemsetAsync(s.hv_ctr, 0, (4 + 3 * KB_HV_MAX) * 4, h->stream));
    }
    if (f.c.redo) {
        HIPCHK(h, hipMemsetAsync(h->ctl->distinct, 0, sizeof(h->ctl->distinct), h->stream));
        h->distinct = 0;
        if (!f.c.dump_only) h->stat_materialisations++;
    }
    const int mode = f.filtered ? KB_MODE_FILTERED : KB_MODE_INSERT, var = f.c.skewed ? 2 : 1;
    const bool dumps = plan.dump_min != 0, dump_only = f.c.dump_only;
    const int launched = by_width(h, [&](auto KWc) {
        constexpr int KW = decltype(KWc)::value;
        const size_t lds_c = KB_C_LDS(KW, plan.bucket_bits);
        const bool big = plan.bucket_bits > KB_BB_SMALL(KW);
        return kb_c_variants([&](auto M, auto V, auto B, auto D, auto L) -> int {
            constexpr bool BIG = decltype(B)::value;
            if (decltype(M)::value != mode || decltype(V)::value != var || BIG != big || decltype(D)::value != dumps || decltype(L)::value != dump_only) return 0;
            hipLaunchKernelGGL((kb_bucket_kernel<KW, decltype(M)::value, decltype(V)::value, BIG, decltype(D)::value, decltype(L)::value>),
                               dim3((unsigned)f.nb_table), dim3(KB_C_CTB(KW, BIG)), lds_c, h->stream, plan, s, h->t, h->ctl, f.nonempty);
            return 1;
        });
    });
    if (!launched) return fail(h, KDF_ERR_STATE, "binned flush: no kernel C instantiation for mode %d, variant %d", mode, var);
    if (heavy) {
        // the buckets the skewed instantiation left aside
        const size_t lds_h = ((size_t)(8 * h->kw + 4) << plan.bucket_bits) + KB_RI_LDS_BYTES;
        by_width(h, [&](auto KWc) {
            constexpr int KW = decltype(KWc)::value;
            if (f.filtered) {                                      // the keys stay put: the slices add to the counts in HBM
                hipLaunchKernelGGL(kb_heavy_filtered_kernel<KW>, dim3(KB_HV_SLICES, KB_HV_MAX), dim3(256), lds_h, h->stream, plan, s, h->t);
            } else {
                hipLaunchKernelGGL(kb_heavy_slice_kernel<KW>, dim3(KB_HV_SLICES, KB_HV_MAX), dim3(256), lds_h, h->stream, plan, s);
                hipLaunchKernelGGL(kb_heavy_combine_kernel<KW>, dim3(KB_HV_MAX), dim3(256), lds_h, h->stream, plan, s, h->t, h->ctl, f.nonempty);
            }
            return 0;
        });
    }
    HIPCHK(h, hipGetLastError());
    st.stamp(); st.commit(h->prof_stage_ev);
    span.stop();
    return KDF_OK;
}

// A dump-only attempt is over (cursor: the keys it dumped).  It stands -- *again stays false -- or is undone for a second,
// ordinary attempt with the same request.
static int kb_settle_dump_only(kdf_engine *h, const KbFlush &f, KbDump *dump, uint64_t cursor, bool *again) {
    // whole (no bucket failed) and the table need not grow for what comes next: the dump is the caller's, the passes stay
    if (h->kb.total(2) == 0 && h->distinct * 10 <= h->cap * 7) {
        dump->done = true; dump->n = cursor; h->stat_fused_dumps++; h->stat_flushes++; h->stat_dump_only++;
        if (f.n_entries >= 100000) h->grow_ratio = (double)(h->distinct - f.c.distinct_before) / (double)f.n_entries;
        h->kb.ring.n_dumped = h->kb.ring.n_pass; h->kb.ring.dumped_positions = h->kb.ring.positions;
        return KDF_OK;
    }
    // otherwise: what the parent path does, from the start -- the ordinary flush of the same passes into the empty table
    // (it dumps too, replays the failed buckets, grows the table); nothing of this attempt is counted.  Undone here is
    // EVERYTHING kernel C<.., LAZY> accumulates into (the list at "what a bucket leaves behind" in kdf_binned.h):
    // totals[2] and ctl->distinct below; s.failed, ctl->tally / cursor and the dump buffers are reset or rewritten by the
    // second attempt.  Under kdf_profile the discarded launch stays in the C stage slot as a second C.
    HIPCHK(h, hipMemsetAsync(f.s.totals + 2, 0, 8, h->stream));
    HIPCHK(h, hipMemsetAsync(h->ctl->distinct, 0, sizeof(h->ctl->distinct), h->stream));
    h->distinct = 0;
    *again = true;
    return KDF_OK;
}

// The buckets kernel C flagged as failed go through the global-atomic kernel: INS (the kernel's) inserts their keys --
// into a table grown to 2^grow_log2 slots first (0: the table stays) -- or, count --if, only probes for them.  who: the
// message's subject.  *ring_kept: the one failure that leaves the ring as it is (the launch itself).
template <bool INS>
static int kb_replay(kdf_engine *h, const KbFlush &f, uint32_t grow_log2, const char *who, bool *ring_kept) {
    int rc;
    if (grow_log2 && (rc = table_rehash(h, grow_log2))) return rc;
    by_width(h, [&](auto KWc) {
        hipLaunchKernelGGL((kb_replay_kernel<decltype(KWc)::value, INS>), dim3((unsigned)f.nb_table), dim3(256), 0, h->stream, f.plan, f.s, h->t, h->ctl);
        return 0;
    });
    *ring_kept = true;
    HIPCHK(h, hipGetLastError());
    *ring_kept = false;
    bool full = false;
    if ((rc = ctl_sync(h, &full))) return rc;
    if (full) return fail(h, KDF_ERR_TABLE_FULL, "%s: bucket overflow during replay (capacity 2^%u)", who, h->t.log2cap);
    return KDF_OK;
}

// keep the load <= 0.7 for what comes next (a 2048-slot bucket then holds
// 1434 +- 38 keys: overflow, which is handled anyway, stays a rare event)
static int kb_load_rule(kdf_engine *h) {
    int rc;
    while (h->distinct * 10 > h->cap * 7)
        if ((rc = table_rehash(h, h->t.log2cap + 1))) return rc;
    return KDF_OK;
}

// An ordinary flush is over: the fused dump, the failed buckets, the ring emptied, the load rule
static int kb_settle(kdf_engine *h, const KbFlush &f, KbDump *dump, uint64_t cursor) {
    int rc;
    // the fused dump is whole only if every bucket went through kernel C's write-back (none failed, none was left to the
    // heavy-bucket kernels); otherwise the caller dumps from the table as usual
    if (f.plan.dump_min && h->kb.total(2) == 0 && h->kb.total(4) == 0) { dump->done = true; dump->n = cursor; h->stat_fused_dumps++; }
    if (h->kb.ring.undumped_passes()) h->stat_flushes++;         // (only retained passes: their dump-only flush was counted)
    h->lazy_empty = false;
    h->stat_heavy_buckets += h->kb.total(4);
    const uint64_t n_failed = h->kb.total(2);
    if (n_failed) {
        h->stat_replayed_buckets += n_failed;
        bool ring_kept = false;
        if (f.filtered) {
            // count --if: kernel C left these buckets as they were in HBM (a stored wide key whose hash word is the empty
            // marker; a full bucket probed for an absent key).  Their entries go through the direct filtered probe: the
            // keys stay put, the table does not grow, absent keys count nothing.
            rc = kb_replay<false>(h, f, 0, "binned count --if", &ring_kept);
        } else {
            // some buckets overflowed: they are untouched in HBM.  Grow the table so
            // that even if every entry of the failed buckets were new the load stays
            // <= 0.5, then replay exactly those buckets through the global-atomic path.
            const uint64_t worst = h->distinct + std::min<uint64_t>(f.n_entries, n_failed * ((f.n_entries / std::max<uint64_t>(f.nb_table, 1)) * 4 + 4096));
            rc = kb_replay<true>(h, f, std::max<uint32_t>(h->t.log2cap + 1, cap_log2_for(worst)), "binned count", &ring_kept);
        }
        if (rc) {                                              // the one error exit behind the launch that empties the ring
            if (!ring_kept) (void)kb_ring_reset(h);
            return rc;
        }
    }
    if (!f.filtered && f.n_entries >= 100000) h->grow_ratio = (double)(h->distinct - f.c.distinct_before) / (double)f.n_entries;
    if ((rc = kb_ring_reset(h))) return rc;
    return f.filtered ? KDF_OK : kb_load_rule(h);
}

// one attempt at the flush; *again: it was a dump-only attempt that has to be redone the ordinary way
static int kb_flush_attempt(kdf_engine *h, KbDump *dump, bool dump_only_ok, bool *again) {
    int rc;
    KbFlush f;
    if ((rc = kb_flush_totals(h, f))) return rc;
    f.c = kb_flush_choose(h, f, dump, dump_only_ok);
    if (f.c.grow_first && (rc = kb_grow_first(h, f.c.est))) return rc;
    if ((rc = kb_flush_prepare(h, f, dump))) return rc;
    if (f.plan.dbg & 2048) return kb_ring_reset(h);               // (ablation: the partition passes are timed alone, what they wrote is dropped)
    if ((rc = kb_flush_launch(h, f))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->kb.totals_host.p, f.s.totals, 16 * 8, hipMemcpyDeviceToHost, h->stream));
    bool full = false;
    uint64_t cursor = 0;
    if ((rc = ctl_sync(h, &full, &cursor))) return rc;
    return f.c.dump_only ? kb_settle_dump_only(h, f, dump, cursor, again) : kb_settle(h, f, dump, cursor);
}

// Kernel C over every pending pass.  dump: a dump is waiting for this flush (the caller's last before it) -- kernel C
// writes it, and the dump-only flush is allowed; its fallback is a second, ordinary attempt with the same request.
static int kb_flush_ring(kdf_engine *h, KbDump *dump) {
    if (h->kb.ring.empty()) return KDF_OK;
    bool again = false;
    int rc = kb_flush_attempt(h, dump, dump != nullptr, &again);
    if (!rc && again) rc = kb_flush_attempt(h, dump, false, &again);
    return rc;
}

// can the binned pipeline work on this engine's table at all?
static bool kb_eligible(const kdf_engine *h) {
    if (is_long(h)) return false;                              // long keys: the direct kernels only (kdf_long.h)
    if (h->opt_hash_shift) return false;                       // an owner table: the bins assume home = top hash bits
    if (h->t.log2cap <= h->t.bucket_bits) return false;        // a single bucket: nothing to partition
    return h->opt_force_path != 1;
}

// Is a flush of n_bases pending positions worth the binned pipeline?  Kernel C reads and rewrites EVERY bucket of the
// table (0.5 ms per GB), whatever the pending passes hold; the direct kernels cost 0.056 ms per million positions whatever
// the table.  Crossover (scratch/bigtable_probe.py): ~14 M positions per GB of table.  table_empty: the table is only
// logically empty (the engine's lazy_empty, or false to ask what an engine with a live table would do).
static bool use_binned(const kdf_engine *h, uint64_t n_bases, bool filtered, bool table_empty) {
    if (!kb_eligible(h)) return false;
    if (h->opt_force_path == 2) return true;
    if (n_bases < h->opt_binned_min_positions) return false;
    if (filtered && h->t.log2cap < h->opt_binned_filtered_min_log2cap) return false;
    if (filtered && h->opt_defer) return true;                 // (more batches will follow before the counts are read: the rewrite is shared)
    // (a table that was only `clear`ed: the binned flush is also its clear, the direct path pays a memset first --
    // 0.2 ms per GB -- which moves the crossover to ~8.6 M positions per GB)
    const uint64_t table_bytes = h->cap * (uint64_t)(8 * h->kw + 4);
    const uint64_t per = table_empty ? h->opt_binned_bytes_per_position * 5 / 3 : h->opt_binned_bytes_per_position;
    return n_bases * per >= table_bytes;
}

// insert-mode count through the global-atomic kernels.  The stream is walked in
// chunks sized so that even if every position were a new key the table stays
// at load <= 0.8; the table doubles when fewer than cap/8 positions fit.
static int direct_insert(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases) {
    const uint64_t n_tiles = (n_bases + KDF_TILE - 1) / KDF_TILE;
    { int rc0 = materialize(h); if (rc0) return rc0; }
    const uint64_t *admit = nullptr;                      // armed prefilter: the gate runs once over the whole stream
    { int rcg = pf_gate(h, d_packed, d_invalid, n_bases, &admit); if (rcg) return rcg; }
    h->last_path = 0;
    uint64_t tile = 0;
    while (tile < n_tiles) {
        uint64_t room = (h->cap / 10) * 8 > h->distinct ? (h->cap / 10) * 8 - h->distinct : 0;
        if (room < h->cap / 8) {
            int rc = table_rehash(h, h->t.log2cap + 1);
            if (rc) return rc;
            continue;
        }
        uint64_t chunk = std::min<uint64_t>(n_tiles - tile, std::max<uint64_t>(room / KDF_TILE, 1));
        // the chunk is a stream of its own that starts at tile `tile` and ends where the whole stream ends
        const uint64_t *p = d_packed + 2 * tile, *m = d_invalid + tile;
        const uint64_t nb = n_bases - tile * KDF_TILE;
        if (admit) launch_stream<MODE_GATED>(h, p, m, chunk, nb, const_cast<uint64_t *>(admit) + tile);
        else launch_stream<MODE_INSERT>(h, p, m, chunk, nb, nullptr);
        HIPCHK(h, hipGetLastError());
        bool full = false;
        int rc = ctl_sync(h, &full);
        if (rc) return rc;
        if (full) return fail(h, KDF_ERR_TABLE_FULL, "count: bucket overflow (capacity 2^%u, %llu distinct)",
                              h->t.log2cap, (unsigned long long)h->distinct);
        tile += chunk;
    }
    return KDF_OK;
}

// L1: append a batch to the pending stream (tile aligned; the copy forces the mask bits past n_bases to "invalid").
// A batch that fills its last tile keeps the all-invalid padding tile behind it: the next batch starts one tile later,
// or a window of this batch's last k - 1 positions would run on into the next batch's first bases.
static int l1_append(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases) {
    const uint64_t n_tiles = n_bases / KDF_TILE + 1;
    if (h->kb.l1.tiles + n_tiles > h->kb.l1.cap_tiles) {
        // grow (the pending stream moves): up to the size at which it is partitioned anyway
        const uint64_t target = std::max<uint64_t>((h->opt_l1_positions + h->opt_l1_direct_positions) / KDF_TILE + 1, h->kb.l1.tiles + n_tiles);
        const uint64_t cap = std::min<uint64_t>(target, std::max<uint64_t>({2 * h->kb.l1.cap_tiles, 4 * (h->kb.l1.tiles + n_tiles), (uint64_t)1 << 18}));
        DevBuf np, nm;                                             // (an error below frees them; the stream stays where it is)
        HIPCHK(h, np.alloc((cap * 2 + 4) * 8));
        hipError_t e = nm.alloc((cap + 2) * 8);
        if (e != hipSuccess) return fail(h, KDF_ERR_NOMEM, "pending stream: %s", hipGetErrorString(e));
        if (h->kb.l1.tiles) {
            HIPCHK(h, hipMemcpyAsync(np.p, h->kb.l1.packed.p, (h->kb.l1.tiles * 2 + 4) * 8, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(nm.p, h->kb.l1.mask.p, (h->kb.l1.tiles + 2) * 8, hipMemcpyDeviceToDevice, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->kb.l1.packed = std::move(np); h->kb.l1.mask = std::move(nm); h->kb.l1.cap_tiles = cap;
    }
    const unsigned blocks = (unsigned)((2 * n_tiles + 4 + 255) / 256);               // (covers the kernel's ceil(n_bases / 64) tiles + padding)
    hipLaunchKernelGGL(kb_append_kernel, dim3(blocks), dim3(256), 0, h->stream, h->kb.l1.packed.as<uint64_t>() + 2 * h->kb.l1.tiles,
                       h->kb.l1.mask.as<uint64_t>() + h->kb.l1.tiles, d_packed, d_invalid, n_bases);
    HIPCHK(h, hipGetLastError());
    h->kb.l1.tiles += n_tiles;
    return KDF_OK;
}

// everything pending (the concatenated small batches, the partitioned passes) goes into the table.  dump: a request the
// LAST flush may serve (earlier ones see counts that are not final)
int pending_flush(kdf_engine *h, KbDump *dump) {
    int rc;
    if (h->kb.l1.tiles && h->kb.ring.n_dumped && !h->kb.ring.undumped_passes()) {
        // small batches behind passes that only a dump-only flush has applied: without lazy_table the ring would be empty
        // and the table live here.  Choose as that engine would; a batch it sends through the direct kernels gets the
        // table first (same last_count_path / binned_passes, and no second rewrite of the table for a few reads)
        if (!use_binned(h, h->kb.l1.positions(), false, false) && (rc = kb_flush_ring(h))) return rc;
    }
    if (h->kb.l1.tiles) {
        const bool binned = h->kb.ring.empty() ? use_binned(h, h->kb.l1.positions(), false, h->lazy_empty) : kb_eligible(h);
        const uint64_t n = h->kb.l1.take();
        if (binned) rc = kb_partition_stream(h, h->kb.l1.packed.as<uint64_t>(), h->kb.l1.mask.as<uint64_t>(), n, false);
        else rc = direct_insert(h, h->kb.l1.packed.as<uint64_t>(), h->kb.l1.mask.as<uint64_t>(), n);
        if (rc) return rc;
    }
    return kb_flush_ring(h, dump);
}
// ... or is forgotten (kdf_clear)
static int pending_drop(kdf_engine *h) {
    h->kb.l1.tiles = 0;
    return kb_ring_reset(h);
}

#define PF_TALLYING_MSG "insert-mode count while the prefilter is tallying: such a count would be neither gated nor known to be meant " \
                       "ungated -- kdf_prefilter_arm (gated counts) or kdf_prefilter_drop (plain counts) first"

// insert-mode count over a device-resident stream
static int count_insert_dev(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases) {
    if (h->filter_mode) return fail(h, KDF_ERR_STATE, "kdf_count_reads: a filter is loaded; call kdf_clear first");
    if (h->pf.state == PF_TALLYING) return fail(h, KDF_ERR_STATE, "%s", PF_TALLYING_MSG);
    sieve_drop(h);                                   // new keys join the table: a sieve built from it earlier (scan) is stale
    h->t.key_parts = h->opt_key_parts; h->t.key_part = h->opt_key_part;       // (tables are re-created by reserve / rehash: set per call)
    if (n_bases == 0) return KDF_OK;
    int rc;
    if (h->opt_force_path == 2 && kb_eligible(h)) rc = kb_partition_stream(h, d_packed, d_invalid, n_bases, false);
    else if (!kb_eligible(h) || h->opt_force_path == 1) {
        if ((rc = pending_flush(h))) return rc;
        rc = direct_insert(h, d_packed, d_invalid, n_bases);
    } else if (n_bases >= h->opt_l1_direct_positions) rc = kb_partition_stream(h, d_packed, d_invalid, n_bases, false);   // big enough by itself
    else {
        rc = l1_append(h, d_packed, d_invalid, n_bases);
        if (!rc && h->kb.l1.positions() >= h->opt_l1_positions) rc = kb_partition_stream(h, h->kb.l1.packed.as<uint64_t>(), h->kb.l1.mask.as<uint64_t>(), h->kb.l1.take(), false);
    }
    if (rc) return rc;
    if (!h->opt_defer) return pending_flush(h);
    return KDF_OK;
}

// kdf_sieve_count_kernel: persistent workgroups over slabs of 1024 x WPT positions.  hits: the scan's hit bits (zeroed by
// the caller), or NULL for a count --if; in_lds: every workgroup copies the sieve into LDS first
static void launch_sieve(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_tiles, uint64_t n_bases,
                         unsigned long long *hits, bool in_lds) {
    by_width(h, [&](auto KWc) {
        constexpr int KW = decltype(KWc)::value;
        const uint64_t tiles_per_slab = KB_THREADS / (64 / KbCfg<KW>::WPT);
        const uint64_t n_slabs = (n_tiles + tiles_per_slab - 1) / tiles_per_slab;
        const uint32_t n_wg = (uint32_t)std::min<uint64_t>(n_slabs, (uint64_t)h->n_cu * 8);
        const uint32_t spw = (uint32_t)((n_slabs + n_wg - 1) / n_wg);
        const unsigned grid = (unsigned)((n_slabs + spw - 1) / spw);
        KdfSieve sv{h->sieve.buf.as<uint64_t>(), h->sieve.words - 1};
        h->last_sieve_in_lds = in_lds;
#define SV_LAUNCH(L, S) hipLaunchKernelGGL((kdf_sieve_count_kernel<KW, L, S>), dim3(grid), dim3(KB_THREADS), 0, h->stream, \
                                           d_packed, d_invalid, n_tiles, n_bases, h->k, h->t, h->ctl, sv, spw, hits)
        if (hits) { if (in_lds) SV_LAUNCH(true, true); else SV_LAUNCH(false, true); }
        else { if (in_lds) SV_LAUNCH(true, false); else SV_LAUNCH(false, false); }
#undef SV_LAUNCH
        return 0;
    });
}

// Size, allocate and zero the membership sieve for n keys (sieve_valid says whether there is one).  Every window costs
// one random 8-byte read of it, i.e. one L2 request: measured on the parent-filter workload (1.49 G windows, 1.9 M keys)
// 8.3 ms with a 2 MB sieve, 9.1 ms with 4 MB, 16 ms with 8 MB, 24 ms with 16 MB -- it must sit in the 4 MB L2 of every XCD
// beside the streamed reads.  So: the most bits per key out of 32 / 16 / 8 that keep it within 2 MB, 8 bits per key beyond
// that, and no sieve (the binned path) once even that passes 16 MB.  Up to 64 K keys it is shrunk to the 64 KB that the
// kernel copies into LDS (no L2 request per window at all: ~700 Gk-mer/s for the filters of VCF mode and Module 3).
static int sieve_prepare(kdf_engine *h, uint64_t n) {
    h->sieve.valid = false;
    uint64_t bpk = h->opt_sieve_bits ? (uint64_t)h->opt_sieve_bits : 32;
    if (!h->opt_sieve_bits) {
        while (bpk > 8 && n * bpk > (16ull << 20)) bpk >>= 1;
        if (n * 8 <= (uint64_t)KDF_SV_LDS_WORDS * 64) while (bpk > 8 && n * bpk > (uint64_t)KDF_SV_LDS_WORDS * 64) bpk >>= 1;
    }
    if (!(h->opt_sieve_bits || n * bpk <= (128ull << 20))) return KDF_OK;
    const uint64_t bits = n * bpk;
    const uint64_t words = std::max<uint64_t>(1024, 1ull << log2ceil((bits + 63) / 64));
    if (const int rc = eng_reserve(h, h->sieve.buf, words * 8, slack_exact)) return rc;
    h->sieve.words = words;
    HIPCHK(h, hipMemsetAsync(h->sieve.buf.p, 0, words * 8, h->stream));
    h->sieve.valid = true;
    return KDF_OK;
}

// long engines, option "long_sieve": the sieve over the keys the table holds now (kdf_long_sieve_from_table_kernel)
// unless there is one; sieve_valid tells whether the keys fit one (sieve_prepare)
static int long_sieve_ensure(kdf_engine *h) {
    if (h->sieve.valid || h->sieve.unfit) return KDF_OK;          // (unfit: the direct kernels, without a host round trip per call)
    int rc;
    if ((rc = ctl_sync(h, nullptr))) return rc;
    if ((rc = sieve_prepare(h, h->distinct))) return rc;
    if (!h->sieve.valid) { h->sieve.unfit = true; return KDF_OK; }
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        if constexpr (W > 2)
            hipLaunchKernelGGL(kdf_long_sieve_from_table_kernel<W>, dim3((unsigned)((h->cap + 255) / 256)), dim3(256), 0, h->stream,
                               h->t, h->sieve.buf.as<uint64_t>(), h->sieve.words - 1);
        return 0;
    });
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

// kdf_long_sieve_kernel over a whole stream of any length.  hits: the scan's hit words, one store per tile, or NULL for a
// count --if.  in_lds: every workgroup copies the sieve into LDS first, so the grid is what the device holds at once and
// every thread walks `rounds` tiles; otherwise one tile per thread, in the pieces of launch_tiles.  How many workgroups
// of 512 a CU holds depends on the instantiation (a workgroup is 2 waves per SIMD: one workgroup where the kernel has
// 3 waves per SIMD -- count --if at W = 3, 6, 7 -- two at 4 or 5, and the sieve's LDS bytes permitting), so the
// runtime is asked.  debug_flags 8192 (tests): a grid of two workgroups, so that small streams take several rounds.
static void launch_long_sieve(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_tiles, uint64_t n_bases,
                              uint64_t *hits, bool in_lds) {
    EvSpan span(h->timer[T_STREAM], h->prof, h->stream, n_tiles);
    KdfSieve sv{h->sieve.buf.as<uint64_t>(), h->sieve.words - 1};
    h->last_sieve_in_lds = in_lds;
    h->last_sieve_rounds = 1;
#define LSV_LAUNCH(L, S, grid, threads, lds, p, m, nt, nb, rounds, hw) \
    hipLaunchKernelGGL((kdf_long_sieve_kernel<W, L, S>), dim3(grid), dim3(threads), lds, h->stream, p, m, nt, nb, h->k, h->t, h->ctl, sv, rounds, hw)
    if (in_lds) {
        const size_t lds = (size_t)h->sieve.words * 8;
        by_words(h, [&](auto Wc) {
            constexpr int W = decltype(Wc)::value;
            if constexpr (W > 2) {
                int per_cu = 0;
                const hipError_t eo = hits ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kdf_long_sieve_kernel<W, true, true>, KDF_LSV_LDS_THREADS, lds)
                                           : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kdf_long_sieve_kernel<W, true, false>, KDF_LSV_LDS_THREADS, lds);
                if (eo != hipSuccess) { (void)hipGetLastError(); per_cu = 1; }
                uint64_t max_wg = (uint64_t)h->n_cu * (uint64_t)std::min(std::max(per_cu, 1), 4);
                if (h->opt_debug_flags & 8192) max_wg = 2;
                const unsigned grid = (unsigned)std::min<uint64_t>((n_tiles + KDF_LSV_LDS_THREADS - 1) / KDF_LSV_LDS_THREADS, max_wg);
                const uint64_t per_round = (uint64_t)grid * KDF_LSV_LDS_THREADS;
                const uint32_t rounds = (uint32_t)((n_tiles + per_round - 1) / per_round);
                h->last_sieve_rounds = rounds;
                if (hits) LSV_LAUNCH(true, true, grid, KDF_LSV_LDS_THREADS, lds, d_packed, d_invalid, n_tiles, n_bases, rounds, hits);
                else LSV_LAUNCH(true, false, grid, KDF_LSV_LDS_THREADS, lds, d_packed, d_invalid, n_tiles, n_bases, rounds, hits);
            }
            return 0;
        });
    } else {
        static_assert(KDF_LSV_THREADS == 256, "launch_tiles counts workgroups of 256");
        launch_tiles(h, d_packed, d_invalid, n_tiles, n_bases, hits,
                     [&](auto Wc, unsigned blocks, const uint64_t *p, const uint64_t *m, uint64_t nt, uint64_t nb, uint64_t *hw) {
            constexpr int W = decltype(Wc)::value;
            if constexpr (W > 2) {
                if (hits) LSV_LAUNCH(false, true, blocks, KDF_LSV_THREADS, 0, p, m, nt, nb, 1u, hw);
                else LSV_LAUNCH(false, false, blocks, KDF_LSV_THREADS, 0, p, m, nt, nb, 1u, hw);
            }
        });
    }
#undef LSV_LAUNCH
    span.stop();
}

// ---- count --if through the bin-major sieve (kdf_binsieve.h, option "sieve_bins") ---------------------------------------
// The sieve over the keys the table holds now, unless there is one; bsv_valid tells whether the sizing rule took them
// (as long_sieve_ensure does for the other sieve: one host round trip per build, none per call).
static int bin_sieve_ensure(kdf_engine *h) {
    if (h->bsv.valid || h->bsv.unfit) return KDF_OK;
    int rc;
    if ((rc = ctl_sync(h, nullptr))) return rc;
    uint32_t c1 = 0, sw = 0, bpk = 0;
    if (kdf_bs_geometry(h->distinct, h->kw, h->opt_sieve_bits, h->opt_sieve_bins, &c1, &sw, &bpk)) { h->bsv.unfit = true; return KDF_OK; }
    const uint64_t words = (uint64_t)sw << c1;
    if ((rc = eng_reserve(h, h->bsv.buf, words * 8, slack_exact))) return rc;
    h->bsv.c1 = c1; h->bsv.slice_words = sw;
    HIPCHK(h, hipMemsetAsync(h->bsv.buf.p, 0, words * 8, h->stream));
    KbPlan plan{};
    plan.c1 = c1;
    by_width(h, [&](auto KWc) {
        hipLaunchKernelGGL(kdf_bs_from_table_kernel<decltype(KWc)::value>, dim3((unsigned)((h->cap + 255) / 256)), dim3(256), 0, h->stream,
                           h->t, plan, h->bsv.buf.as<uint64_t>(), sw);
        return 0;
    });
    HIPCHK(h, hipGetLastError());
    h->bsv.valid = true;
    return KDF_OK;
}

// ONE pass of at most opt_binned_max_positions positions: kernel A as kb_partition launches it (coarse bits only), the
// offset rows transposed bin-major, one workgroup of the bin kernel per (bin, share of the slabs).  Eager: no ring.
template <int KW>
static int bin_sieve_pass(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases, uint64_t n_end) {
    constexpr int WPT = KbCfg<KW>::WPT, TPT = 64 / WPT, SLAB = KbCfg<KW>::SLAB;
    constexpr uint32_t TILES_PER_SLAB = KB_A_THREADS / TPT;
    const uint64_t n_tiles = (n_bases + KDF_TILE - 1) / KDF_TILE;
    if (n_tiles == 0) return KDF_OK;
    int rc;
    KbPlan plan{};
    plan.c1 = h->bsv.c1; plan.c2 = 0; plan.key_parts = 0;
    plan.log2cap = h->t.log2cap; plan.bucket_bits = h->t.bucket_bits; plan.off_stride = 2; plan.group = 1;
    const uint32_t nbins = 1u << plan.c1;
    const uint64_t n_slabs = (n_tiles + TILES_PER_SLAB - 1) / TILES_PER_SLAB;
    if (n_slabs >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "bin sieve pass: too many positions for one pass");
    plan.n_slabs = (uint32_t)n_slabs; plan.n_groups = (uint32_t)n_slabs;
    if ((rc = kb_ensure_attrs<KW>(h))) return rc;
    const size_t lds_bin = (size_t)h->bsv.slice_words * 8 + KDF_BS_LDS_OTHER(KW);
    if (!h->bsv.attr_set[KW]) {
        HIPCHK(h, hipFuncSetAttribute((const void *)kdf_bin_sieve_kernel<KW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)((size_t)kdf_bs_cap_words() * 8 + KDF_BS_LDS_OTHER(KW))));
        h->bsv.attr_set[KW] = true;
    }
    if ((rc = eng_reserve(h, h->kb.tmp, n_slabs * (uint64_t)SLAB * 8 * KW, slack_16th))) return rc;
    if ((rc = eng_reserve(h, h->kb.off_rows, n_slabs * (uint64_t)(nbins + 1) * 2 + 64, slack_16th))) return rc;
    if ((rc = eng_reserve(h, h->kb.bin_runs, n_slabs * (uint64_t)nbins * 4, slack_16th))) return rc;
    KbScratch s;
    if ((rc = kb_scratch(h, s))) return rc;
    uint32_t *runs = h->kb.bin_runs.as<uint32_t>();

    StageStamps st(h->prof, h->stream);
    EvSpan span(h->timer[T_STREAM], h->prof, h->stream, n_tiles);
    st.stamp();                                                  // start of A
    const uint32_t slabs_per_wg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(8, n_slabs / ((uint64_t)h->n_cu * 8)));
    const unsigned grid_a = (unsigned)((n_slabs + slabs_per_wg - 1) / slabs_per_wg);
    hipLaunchKernelGGL((kb_slabsort_kernel<KW, false>), dim3(grid_a), dim3(KB_A_THREADS), kb_lds_a<KW>(), h->stream, d_packed, d_invalid, n_tiles, n_end, h->k, plan, s, slabs_per_wg);
    st.stamp();                                                  // end of A
    hipLaunchKernelGGL(kdf_bs_transpose_kernel, dim3((unsigned)((n_slabs + 63) / 64), (nbins + 63) / 64), dim3(256), 0, h->stream,
                       (const uint16_t *)s.off, runs, (uint32_t)n_slabs, nbins);
    st.stamp();                                                  // end of the transposer
    // about four workgroups per CU over all bins, and no share of less than one round of slabs
    const uint64_t want = std::max<uint64_t>(1, ((uint64_t)h->n_cu * 4 + nbins - 1) / nbins);
    const uint64_t shares0 = std::min<uint64_t>(want, (n_slabs + KDF_BS_THREADS - 1) / KDF_BS_THREADS);
    const uint32_t slabs_per_share = (uint32_t)((n_slabs + shares0 - 1) / shares0);
    const uint32_t shares = (uint32_t)((n_slabs + slabs_per_share - 1) / slabs_per_share);
    hipLaunchKernelGGL(kdf_bin_sieve_kernel<KW>, dim3(nbins * shares), dim3(KDF_BS_THREADS), lds_bin, h->stream,
                       (const uint64_t *)s.tmp, (const uint32_t *)runs, h->bsv.buf.as<const uint64_t>(), h->bsv.slice_words, (uint32_t)n_slabs,
                       shares, slabs_per_share, h->t, h->ctl);
    st.stamp();                                                  // end of the bin kernel
    HIPCHK(h, hipGetLastError());
    span.stop();
    st.commit(h->prof_stage_ev);                                 // (kdf_profile_stages: A, transposer, bin kernel in the partition's three slots)
    h->stat_bin_sieve_passes++;
    return KDF_OK;
}

// the whole stream, in passes that start on tile boundaries (as kb_partition_stream cuts them)
static int count_bin_sieve(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases) {
    int rc;
    if ((rc = kb_flush_ring(h))) return rc;                       // (binned --if passes pending from earlier batches)
    const uint64_t step = h->opt_binned_max_positions;
    for (uint64_t off = 0; off < n_bases; off += step) {
        const uint64_t len = std::min<uint64_t>(step, n_bases - off);
        const uint64_t *p = d_packed + off / 32, *m = d_invalid + off / 64;
        if ((rc = by_width(h, [&](auto KWc) { return bin_sieve_pass<decltype(KWc)::value>(h, p, m, len, n_bases - off); }))) return rc;
    }
    h->last_path = 5;
    h->last_sieve_bins = h->bsv.c1; h->last_sieve_slice_words = h->bsv.slice_words;
    return KDF_OK;
}

static int count_filtered_dev(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases) {
    if (!h->filter_mode) return fail(h, KDF_ERR_STATE, "kdf_count_reads_filtered: no filter loaded (kdf_load_filter)");
    const uint64_t n_tiles = (n_bases + KDF_TILE - 1) / KDF_TILE;
    if (n_tiles == 0) return KDF_OK;
    { int rc0 = materialize(h); if (rc0) return rc0; }
    if (h->opt_sieve_bins && h->opt_force_path == 0 && !h->opt_hash_shift && !is_long(h)) {
        int rc = bin_sieve_ensure(h);                              // (the option was set, or keys were added, after the filter was loaded)
        if (rc) return rc;
        if (h->bsv.valid) return count_bin_sieve(h, d_packed, d_invalid, n_bases);
    }
    if (is_long(h)) {
        if (h->opt_long_sieve && h->opt_force_path != 1) {
            int rc = long_sieve_ensure(h);                         // (the option was set, or keys were added, after the filter was loaded)
            if (rc) return rc;
            if (h->sieve.valid) {
                launch_long_sieve(h, d_packed, d_invalid, n_tiles, n_bases, nullptr, h->sieve.words <= KDF_SV_LDS_WORDS && !(h->opt_debug_flags & 2048));
                HIPCHK(h, hipGetLastError());
                h->last_path = 3;
                return KDF_OK;
            }
        }
    } else if (h->sieve.valid && (h->opt_force_path == 0 || h->opt_force_path == 4)) {
        EvSpan span(h->timer[T_STREAM], h->prof, h->stream, n_tiles);
        launch_sieve(h, d_packed, d_invalid, n_tiles, n_bases, nullptr, h->sieve.words <= KDF_SV_LDS_WORDS && !(h->opt_debug_flags & 2048));
        span.stop();
        HIPCHK(h, hipGetLastError());
        h->last_path = 3;
        return KDF_OK;
    }
    if (h->opt_force_path == 4) return fail(h, KDF_ERR_STATE, "force_path 4 (sieve): no sieve for this filter (it would not fit the caches, or keys were added after kdf_load_filter)");
    if (use_binned(h, n_bases, true, h->lazy_empty)) {
        int rc = kb_partition_stream(h, d_packed, d_invalid, n_bases, true);
        if (!rc && !h->opt_defer) rc = kb_flush_ring(h);
        return rc;
    }
    { int rc0 = kb_flush_ring(h); if (rc0) return rc0; }           // (binned --if passes pending from earlier batches)
    h->last_path = 0;
    launch_stream<MODE_FILTERED>(h, d_packed, d_invalid, n_tiles, n_bases, nullptr);
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

__global__ void kdf_mask_tail_kernel(uint64_t *word, uint64_t bits) { *word |= bits; }

// copy n_bases > 0 positions into device buffers of kdf_stream_words(n_bases) words, on stream s.  The caller's arrays
// hold ceil(n/32) packed / ceil(n/64) mask words: the rest is padded with 0 / 0xFF, and the bits past n_bases in the
// last mask word must read "invalid" too.
static int upload_padded(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases,
                         uint64_t *d_packed, uint64_t *d_invalid, hipStream_t s) {
    uint64_t pw, mw;
    kdf_stream_words(n_bases, &pw, &mw);
    const uint64_t pw_in = (n_bases + 31) / 32, mw_in = (n_bases + 63) / 64;
    if (pw > pw_in) HIPCHK(h, hipMemsetAsync(d_packed + pw_in, 0, (pw - pw_in) * 8, s));
    if (mw > mw_in) HIPCHK(h, hipMemsetAsync(d_invalid + mw_in, 0xFF, (mw - mw_in) * 8, s));
    HIPCHK(h, hipMemcpyAsync(d_packed, packed, pw_in * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(d_invalid, invalid, mw_in * 8, hipMemcpyHostToDevice, s));
    if (n_bases % 64) hipLaunchKernelGGL(kdf_mask_tail_kernel, dim3(1), dim3(1), 0, s, d_invalid + (mw_in - 1), ~0ull << (n_bases % 64));
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

// ---- the staging frame of a host form (kdf_engine_priv.h) ----
int HostCall::commit() {
    if (h->arena_user) return fail(h, KDF_ERR_STATE, "%s: the staging arena is still held by %s", fn, h->arena_user);
    const int rc = eng_reserve(h, h->arena, lay.total);
    if (rc) return rc;
    h->arena_user = fn; open = true;
    for (int i = 0; i < lay.n; ++i) {
        if (!item[i].src || !lay.size[i]) continue;
        if (item[i].n_bases) {                                     // a stream: both halves, padded
            const int rcs = upload_padded(h, (const uint64_t *)item[i].src, (const uint64_t *)item[i + 1].src, item[i].n_bases, dev<uint64_t>(i), dev<uint64_t>(i + 1), h->stream);
            if (rcs) return rcs;
            ++i;
            continue;
        }
        const hipError_t e = hipMemcpyAsync(dev(i), item[i].src, lay.size[i], hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) return fail(h, KDF_ERR_HIP, "%s: copy of %zu bytes to the device failed: %s", fn, lay.size[i], hipGetErrorString(e));
    }
    return KDF_OK;
}
int HostCall::fetch(int i, size_t bytes) {
    if (bytes && item[i].dst) HIPCHK(h, hipMemcpyAsync(item[i].dst, dev(i), bytes, hipMemcpyDeviceToHost, h->stream));
    return KDF_OK;
}
int HostCall::finish() {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return KDF_OK;
}

static int src_dev(kdf_engine *h, const char *fn, const void *d_packed, const void *d_invalid, uint64_t n_bases, StreamSrc &src) {
    if (n_bases && (!d_packed || !d_invalid)) return fail(h, KDF_ERR_INVALID, "%s: NULL stream", fn);
    HIPCHK(h, hipSetDevice(h->device));
    src = StreamSrc{(const uint64_t *)d_packed, (const uint64_t *)d_invalid, n_bases, -1};
    return KDF_OK;
}

// host arrays, staged on the engine's stream in the caller's frame, which stays open while the consumer is launched;
// n_bases == 0: an empty source, nothing is asked or touched
static int src_host(HostCall &c, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases, StreamSrc &src) {
    kdf_engine *h = c.h;
    src = StreamSrc{};
    if (n_bases == 0) return KDF_OK;
    if (!packed || !invalid) return fail(h, KDF_ERR_INVALID, "%s: NULL stream", c.fn);
    HIPCHK(h, hipSetDevice(h->device));
    const int s = c.stream(packed, invalid, n_bases);
    const int rc = c.commit();
    if (!rc) src = StreamSrc{c.dev<uint64_t>(s), c.dev<uint64_t>(s + 1), n_bases, -1};
    return rc;
}

// behind the consumer's last launch: the slot's next upload waits for this reader
void src_release(kdf_engine *h, const StreamSrc &src) {
    if (src.slot >= 0) (void)hipEventRecord(h->up.slot[src.slot].use_done, h->stream);
}

// ---------------------------------------------------------------------------
// two-pass counting (kdf_prefilter.h)

static int pf_tally_dev(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases) {
    if (n_bases == 0) return KDF_OK;
    EvSpan span(h->timer[T_PF], h->prof, h->stream);
    pf_launch(h, d_packed, d_invalid, n_bases, nullptr);
    span.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

// merge `nseg` device segments of n_words words into sieve words [first_word, first_word + n_words): one launch
static int pf_merge_dev(kdf_engine *h, uint64_t first_word, uint64_t n_words, uint32_t nseg, const unsigned long long *const *d_segs, bool replace) {
    if (n_words == 0) return KDF_OK;
    KdfPfSegs sg{};
    for (uint32_t s = 0; s < nseg; ++s) sg.seg[s] = d_segs[s];
    sg.nseg = nseg;
    const uint32_t head = (uint32_t)(first_word & 1);             // the word before the first pair of 16 aligned bytes
    const uint64_t n_pairs = (n_words - head) / 2;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_pairs + 255) / 256, (uint64_t)h->n_cu * 8));
    EvSpan span(h->timer[T_PFM], h->prof, h->stream);
    if (replace) hipLaunchKernelGGL(kdf_pf_merge_kernel<true>, dim3(grid), dim3(256), 0, h->stream, h->pf.view.words + first_word, sg, n_words, head, n_pairs);
    else hipLaunchKernelGGL(kdf_pf_merge_kernel<false>, dim3(grid), dim3(256), 0, h->stream, h->pf.view.words + first_word, sg, n_words, head, n_pairs);
    span.stop();
    HIPCHK(h, hipGetLastError());
    h->pf.merged_words += n_words;
    return KDF_OK;
}

static void pf_free(kdf_engine *h) { h->pf = PfState{}; }

// ---------------------------------------------------------------------------
// distinct k-mer sketch (kdf_sketch.h)

static int sk_add_dev(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases) {
    if (n_bases == 0) return KDF_OK;
    EvSpan span(h->timer[T_SK], h->prof, h->stream);
    launch_tiles(h, d_packed, d_invalid, kdf_stream_geom(n_bases).tiles, n_bases, nullptr,
                 [&](auto Wc, unsigned blocks, const uint64_t *p, const uint64_t *m, uint64_t nt, uint64_t nb, uint64_t *) {
        constexpr int W = decltype(Wc)::value;
        if constexpr (W <= 2) hipLaunchKernelGGL((kdf_sk_stream_kernel<W>), dim3(blocks), dim3(256), 0, h->stream, p, m, nt, nb, h->k, h->sk.view, h->sk.ctr.as<unsigned long long>());
        else hipLaunchKernelGGL((kdf_sk_long_kernel<W>), dim3(blocks), dim3(256), 0, h->stream, p, m, nt, nb, h->k, h->sk.view, h->sk.ctr.as<unsigned long long>());
    });
    span.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

static void sk_free(kdf_engine *h) { h->sk = SkState{}; }

// the registers as bytes in `d_out` (device), in stream order
static int sk_pack(kdf_engine *h, uint8_t *d_out) {
    const uint32_t m = 1u << h->sk.view.p;
    hipLaunchKernelGGL(kdf_sk_pack_kernel, dim3((m + 255) / 256), dim3(256), 0, h->stream, h->sk.view.cells, m, d_out);
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

#define SK_NEED_ON(h, fn) \
    do { if (!(h)->sk.on) return fail(h, KDF_ERR_STATE, "%s: no sketch is on (kdf_sketch_begin)", fn); } while (0)

#define PF_NEED_TALLYING(h, fn) \
    do { if ((h)->pf.state != PF_TALLYING) return fail(h, KDF_ERR_STATE, "%s: the prefilter is %s; reads are tallied between kdf_prefilter_begin and kdf_prefilter_arm", \
                                                       fn, (h)->pf.state == PF_ARMED ? "armed (its sieve is immutable)" : "off"); } while (0)

// n keys of a host form: the item of lo (or of the rows of long keys); the next one is hi (k 33..63, else empty)
static int keys_in(HostCall &c, const uint64_t *lo, const uint64_t *hi, uint64_t n) {
    const int i = c.in(lo, n * 8 * lo_words(c.h));
    c.in(hi, c.h->kw == 2 ? n * 8 : 0);
    return i;
}

// ===========================================================================
// C ABI
// ===========================================================================

extern "C" {

const char *kdf_last_error(const kdf_engine *h) { return h ? h->err.c_str() : g_err.c_str(); }

int kdf_create(int device, int k, uint64_t capacity_hint, kdf_engine **out) {
    if (!out) return fail(nullptr, KDF_ERR_INVALID, "kdf_create: out is NULL");
    *out = nullptr;
    if (k < 1 || k > KDF_LONG_MAX_K || (k > 63 && k % 2 == 0))
        return fail(nullptr, KDF_ERR_INVALID, "kdf_create: k=%d out of range (1..63, or odd 65..%d)", k, KDF_LONG_MAX_K);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, KDF_ERR_HIP, "kdf_create: no HIP device available (%s)", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, KDF_ERR_INVALID, "kdf_create: device %d of %d", device, ndev);
    kdf_engine *h = new kdf_engine();
    h->capacity_hint = capacity_hint;
    h->device = device; h->k = k; h->kw = k <= 32 ? 1 : k <= 63 ? 2 : (2 * k + 63) / 64;
    if (is_long(h)) { h->opt_fused_dump = 0; h->opt_lazy_table = 0; }
    else h->opt_long_sieve = 0;                      // (KDF_LONG_SIEVE is for long engines: k <= 63 takes its sieve anyway)
    if (is_long(h)) h->opt_sieve_bins = 0;           // (and KDF_SIEVE_BINS for k <= 63)
    auto bail = [&](int rc) { g_err = h->err; kdf_destroy(h); return rc; };
    if ((e = hipSetDevice(device)) != hipSuccess) { h->err = hipGetErrorString(e); return bail(KDF_ERR_HIP); }
    { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) h->n_cu = ncu; }
    { size_t f = 0, tt = 0; if (hipMemGetInfo(&f, &tt) == hipSuccess) h->dev_total_bytes = tt; else (void)hipGetLastError(); }
    if ((e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking)) != hipSuccess) { h->err = hipGetErrorString(e); return bail(KDF_ERR_HIP); }
    h->stream = h->own_stream;
    if ((e = h->ctl_mem.alloc(sizeof(KdfCtl))) != hipSuccess || (e = h->out4_mem.alloc(32)) != hipSuccess || (e = h->out4_pin.alloc(32)) != hipSuccess) {
        h->err = hipGetErrorString(e); return bail(KDF_ERR_NOMEM);
    }
    h->ctl = h->ctl_mem.as<KdfCtl>(); h->d_out4 = h->out4_mem.as<unsigned long long>(); h->h_out4 = h->out4_pin.as<unsigned long long>();
    int rc = ctl_reset(h, false);
    if (rc) return bail(rc);
    if (const char *ev = getenv("KDF_BIG_BUCKET_LOG2CAP")) { const int v = atoi(ev); if (v >= 10 && v <= 64) h->opt_big_bucket_log2cap = (uint32_t)v; }
    NewTable nt;
    rc = table_alloc(h, cap_log2_for(capacity_hint), nt);
    if (rc) return bail(rc);
    table_adopt(h, nt);
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) { h->err = hipGetErrorString(e); return bail(KDF_ERR_HIP); }
    *out = h;
    return KDF_OK;
}

// Every buffer of the engine frees itself with it (kdf_devbuf.h), after the streams that may still read it have drained
void kdf_destroy(kdf_engine *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->up.copy_stream) (void)hipStreamSynchronize(h->up.copy_stream);
    for (EvTimer &t : h->timer) t.collect();
    stage_collect(h);
    for (UpSlot &sl : h->up.slot)
        for (hipEvent_t ev : {sl.up_done, sl.use_done}) if (ev) (void)hipEventDestroy(ev);
    if (h->up.copy_stream) (void)hipStreamDestroy(h->up.copy_stream);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

int kdf_set_stream(kdf_engine *h, void *hip_stream) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    { int rcf = pending_flush(h); if (rcf) return rcf; }          // (pending passes were enqueued on the old stream)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return KDF_OK;
}

int kdf_synchronize(kdf_engine *h) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->up.copy_stream) HIPCHK(h, hipStreamSynchronize(h->up.copy_stream));      // uploads still in flight read host buffers
    return KDF_OK;
}

int kdf_clear(kdf_engine *h) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ctl_reset(h, false);
    if (rc) return rc;
    h->distinct = 0; h->windows = 0; h->filter_mode = false;
    h->lazy_empty = true; sieve_drop(h); h->zero_keys = false;
    h->grow_ratio = 0.0;
    if ((rc = pending_drop(h))) return rc;     // what was counted but not yet applied is dropped with the rest
    return KDF_OK;
}

int kdf_reserve(kdf_engine *h, uint64_t n_keys) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    HIPCHK(h, hipSetDevice(h->device));
    { int rcf = pending_flush(h); if (rcf) return rcf; }
    const uint32_t want = cap_log2_for(std::max(n_keys, h->distinct));
    if (want <= h->t.log2cap) return KDF_OK;
    int rc = ctl_sync(h, nullptr);
    if (rc) return rc;
    return table_rehash(h, want);
}

int kdf_stats(kdf_engine *h, uint64_t *capacity, uint64_t *distinct, uint64_t *windows) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    HIPCHK(h, hipSetDevice(h->device));
    // (passes a dump-only flush has applied: their keys and windows are in the counters already, the table is not needed)
    if (h->kb.l1.tiles || h->kb.ring.undumped_passes()) { int rcf = pending_flush(h); if (rcf) return rcf; }
    bool full = false;
    int rc = ctl_sync(h, &full);
    if (rc) return rc;
    if (capacity) *capacity = h->cap;
    if (distinct) *distinct = h->distinct;
    if (windows) *windows = h->windows;
    if (full) return fail(h, KDF_ERR_TABLE_FULL, "a bucket overflowed during an earlier call");
    return KDF_OK;
}

int kdf_flush(kdf_engine *h) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    HIPCHK(h, hipSetDevice(h->device));
    return pending_flush(h);
}

int kdf_count_reads_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    StreamSrc src;
    const int rc = src_dev(h, "kdf_count_reads_dev", d_packed, d_invalid, n_bases, src);
    return rc ? rc : count_insert_dev(h, src.packed, src.invalid, src.n_bases);
}

int kdf_count_reads(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    HostCall c(h, "kdf_count_reads");
    StreamSrc src;
    const int rc = src_host(c, packed, invalid, n_bases, src);
    return rc || !src.n_bases ? rc : count_insert_dev(h, src.packed, src.invalid, src.n_bases);
}

int kdf_host_alloc(uint64_t bytes, void **out) {
    if (!out) return fail(nullptr, KDF_ERR_INVALID, "kdf_host_alloc: NULL pointer");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 8, hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, KDF_ERR_NOMEM, "kdf_host_alloc: %s", hipGetErrorString(e)); }
    return KDF_OK;
}
int kdf_host_free(void *p) {
    if (p) (void)hipHostFree(p);
    return KDF_OK;
}

int kdf_upload_reads_async(kdf_engine *h, int slot, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (slot < 0 || slot > 1) return fail(h, KDF_ERR_INVALID, "kdf_upload_reads_async: slot must be 0 or 1");
    if (n_bases && (!packed || !invalid)) return fail(h, KDF_ERR_INVALID, "kdf_upload_reads_async: NULL stream");
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->up.copy_stream) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->up.copy_stream, hipStreamNonBlocking));
        for (int sl = 0; sl < 2; ++sl) {
            HIPCHK(h, hipEventCreateWithFlags(&h->up.slot[sl].up_done, hipEventDisableTiming));
            HIPCHK(h, hipEventCreateWithFlags(&h->up.slot[sl].use_done, hipEventDisableTiming));
        }
    }
    uint64_t pw, mw;
    kdf_stream_words(n_bases, &pw, &mw);
    auto both_streams = [&] {                                  // (the slot's last count may still read the old buffer)
        const hipError_t e = hipStreamSynchronize(h->stream);
        return e != hipSuccess ? e : hipStreamSynchronize(h->up.copy_stream);
    };
    UpSlot &up = h->up.slot[slot];
    HIPCHK(h, dev_reserve(up.packed, (size_t)pw * 8, slack_8th((size_t)pw * 8), both_streams));
    HIPCHK(h, dev_reserve(up.mask, (size_t)mw * 8, slack_8th((size_t)mw * 8), both_streams));
    h->up.slot[slot].valid = false;
    h->up.slot[slot].n_bases = n_bases;
    if (n_bases == 0) { h->up.slot[slot].valid = true; return KDF_OK; }
    hipStream_t cs = h->up.copy_stream;
    if (h->up.slot[slot].use_done) HIPCHK(h, hipStreamWaitEvent(cs, h->up.slot[slot].use_done, 0));   // the count that last read this slot
    int rc = upload_padded(h, packed, invalid, n_bases, up.packed.as<uint64_t>(), up.mask.as<uint64_t>(), cs);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->up.slot[slot].up_done, cs));
    h->up.slot[slot].valid = true;
    return KDF_OK;
}

int kdf_count_uploaded(kdf_engine *h, int slot, int filtered) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    StreamSrc src;
    // (a call refused for the engine's state keeps the slot's batch: a refused call changes nothing)
    int rc = src_slot(EngSink{h}, "kdf_count_uploaded", h, slot, true, true, src, [&](const StreamSrc &b) {
        if (!filtered && h->filter_mode) return fail(h, KDF_ERR_STATE, "kdf_count_uploaded: a filter is loaded; call kdf_clear first");
        if (filtered && !h->filter_mode) return fail(h, KDF_ERR_STATE, "kdf_count_uploaded: no filter loaded (kdf_load_filter)");
        if (filtered && b.n_bases && h->opt_force_path == 4 && !h->sieve.valid)      // (an empty batch asks nothing of the sieve: kdf_count_reads_filtered*)
            return fail(h, KDF_ERR_STATE, "kdf_count_uploaded: force_path 4 (sieve): no sieve for this filter (keys were added after kdf_load_filter)");
        if (!filtered && h->pf.state == PF_TALLYING) return fail(h, KDF_ERR_STATE, "%s", PF_TALLYING_MSG);
        return (int)KDF_OK;
    });
    if (rc || !src.n_bases) return rc;
    rc = filtered ? count_filtered_dev(h, src.packed, src.invalid, src.n_bases) : count_insert_dev(h, src.packed, src.invalid, src.n_bases);
    src_release(h, src);
    return rc;
}

__global__ void kdf_ctl_clear_error_bits_kernel(KdfCtl *ctl, unsigned int bits) { atomicAnd(&ctl->error, ~bits); }

// after an insert of caller keys and a ctl_sync: a long key with a top-word bit at or above 2k - 64 (W - 1) was refused
// (error bit 4).  Only that bit is cleared: a bucket overflow of the same launch (bit 1) stays raised and is reported too.
static int long_bad_keys(kdf_engine *h, const char *fn) {
    const unsigned int err = (unsigned int)h->h_out4[2];
    if (!(err & 4)) return KDF_OK;
    hipLaunchKernelGGL(kdf_ctl_clear_error_bits_kernel, dim3(1), dim3(1), 0, h->stream, h->ctl, 4u);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return fail(h, KDF_ERR_INVALID, "%s: a key's top word has bits at or above bit %d (no k-mer of k=%d); it was left out%s", fn,
                long_top_bits(h), h->k, (err & 1) ? "; a bucket also overflowed (KDF_ERR_TABLE_FULL)" : "");
}

// the table becomes exactly the n keys at d_lo / d_hi (device arrays; long keys: the rows at d_lo) with count 0
static int load_filter_core(kdf_engine *h, const uint64_t *d_lo, const uint64_t *d_hi, uint64_t n, const char *fn) {
    int rc;
    sieve_drop(h);
    if ((rc = pending_drop(h))) return rc;            // the table becomes the filter: whatever was pending goes with the old contents
    // size the table for n keys at load <= 0.5, then start from empty
    const uint32_t want = cap_log2_for(n);
    if (want != h->t.log2cap) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->t_mem = TableMem{}; h->t = KdfTable{};      // (freed first: the old and the new table need not fit side by side)
        NewTable nt;
        if ((rc = table_alloc(h, want, nt))) return rc;
        table_adopt(h, nt);
        if ((rc = ctl_reset(h, false))) return rc;
        h->distinct = 0; h->windows = 0; h->lazy_empty = false; h->filter_mode = false;
    } else if ((rc = kdf_clear(h))) return rc;
    if ((rc = materialize(h))) return rc;
    h->filter_mode = true; h->zero_keys = true;
    if (n) {
        insert_keys(h, h->t, d_lo, d_hi, nullptr, n, false);
        HIPCHK(h, hipGetLastError());
        bool full = false;
        if ((rc = ctl_sync(h, &full))) return rc;
        if ((rc = long_bad_keys(h, fn))) return rc;
        if (full) return fail(h, KDF_ERR_TABLE_FULL, "%s: bucket overflow", fn);
    }
    if (is_long(h)) return h->opt_long_sieve ? long_sieve_ensure(h) : KDF_OK;     // (long keys: from the table just loaded, and only when asked to)
    if ((rc = sieve_prepare(h, n)) != KDF_OK) return rc;
    if (h->sieve.valid && n) {
        by_width(h, [&](auto KWc) {
            hipLaunchKernelGGL(kdf_sieve_build_kernel<decltype(KWc)::value>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                               d_lo, d_hi, n, h->sieve.buf.as<uint64_t>(), h->sieve.words - 1);
            return 0;
        });
        HIPCHK(h, hipGetLastError());
    }
    return KDF_OK;
}

int kdf_load_filter(kdf_engine *h, const uint64_t *keys_lo, const uint64_t *keys_hi, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_REFUSE_LONG(h, "kdf_load_filter", "kdf_load_filter_w");
    if (n && (!keys_lo || (h->kw == 2 && !keys_hi))) return fail(h, KDF_ERR_INVALID, "kdf_load_filter: NULL keys");
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_load_filter");
    const int ik = keys_in(c, keys_lo, keys_hi, n);
    if (const int rc = c.commit()) return rc;
    return load_filter_core(h, c.dev<uint64_t>(ik), c.dev<uint64_t>(ik + 1), n, "kdf_load_filter");
}

int kdf_load_filter_dev(kdf_engine *h, const void *d_keys_lo, const void *d_keys_hi, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_REFUSE_LONG(h, "kdf_load_filter_dev", "kdf_load_filter_w_dev");
    if (n && (!d_keys_lo || (h->kw == 2 && !d_keys_hi))) return fail(h, KDF_ERR_INVALID, "kdf_load_filter_dev: NULL keys");
    HIPCHK(h, hipSetDevice(h->device));
    return load_filter_core(h, (const uint64_t *)d_keys_lo, (const uint64_t *)d_keys_hi, n, "kdf_load_filter");
}

int kdf_reset_counts(kdf_engine *h) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    HIPCHK(h, hipSetDevice(h->device));
    // filter mode: counts that were never applied need not be.  Insert mode: pending windows also bring KEYS, and the keys
    // stay -- what the table holds afterwards must not depend on whether a flush happened to come first.
    int rc = h->filter_mode ? pending_drop(h) : pending_flush(h);
    if (rc) return rc;
    if ((rc = materialize(h))) return rc;
    HIPCHK(h, hipMemsetAsync(h->t.cnt, 0, h->cap * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(h->ctl->windows, 0, sizeof(h->ctl->windows), h->stream));
    h->windows = 0; h->zero_keys = true;
    return KDF_OK;
}

// insert-or-add (key, count) pairs resident in HBM, in `nseg` segments (one per source rank of a merge); grows the
// table first so the pairs fit at load <= 0.5 even if all of them are new.  Hash-layout tables take segments of any
// order: km_bounds_kernel tests on the device whether every segment is grouped by table bucket (a dump made by
// kdf_export_parts_dev is) and the LDS bucket merge or the atomic insert runs accordingly -- no host decision.  Long keys
// (the rows at d_lo) take the atomic insert.
static int add_pairs_multi(kdf_engine *h, uint32_t nseg, const uint64_t *const *d_lo, const uint64_t *const *d_hi,
                           const uint32_t *const *d_cnt, const uint64_t *n, const char *fn) {
    uint64_t total = 0, nmax = 0;
    bool counts = true;
    for (uint32_t s = 0; s < nseg; ++s) { total += n[s]; nmax = std::max(nmax, n[s]); if (n[s] && !d_cnt[s]) counts = false; }
    if (total == 0) return KDF_OK;
    sieve_drop(h);                                   // keys may join the table that the sieve has not seen
    h->zero_keys = true;                             // ... with a count of 0 (NULL counts, a 0 in the array)
    int rc;
    if ((rc = pending_flush(h))) return rc;
    if ((rc = ctl_sync(h, nullptr))) return rc;
    const uint32_t want = cap_log2_for(h->distinct + total);
    if (want > h->t.log2cap && (rc = table_rehash(h, want))) return rc;
    const bool lds = !is_long(h) && counts && total >= h->opt_merge_min_pairs && nseg <= KM_MAX_SEGS && nmax < 0xFFFFFFFFull;
    if (!lds) {
        if ((rc = materialize(h))) return rc;
        for (uint32_t s = 0; s < nseg; ++s)
            if (n[s]) insert_keys(h, h->t, d_lo[s], d_hi[s], d_cnt[s], n[s], false);
        h->merge.last_path = 2;
    } else {
        KmSegs sg{};
        uint32_t m = 0;
        for (uint32_t s = 0; s < nseg; ++s) {
            if (!n[s]) continue;
            sg.lo[m] = d_lo[s]; sg.hi[m] = h->kw == 2 ? d_hi[s] : nullptr; sg.cnt[m] = d_cnt[s]; sg.n[m] = (uint32_t)n[s]; ++m;
        }
        sg.nseg = m;
        const uint32_t nb = (uint32_t)(h->cap >> h->t.bucket_bits);
        const size_t words = (size_t)m * nb * 2 + 16;
        if ((rc = eng_reserve(h, h->merge.scratch, words * 4, slack_exact))) return rc;
        uint32_t *first = h->merge.scratch.as<uint32_t>(), *last = first + (size_t)m * nb, *flag = last + (size_t)m * nb;
        HIPCHK(h, hipMemsetAsync(h->merge.scratch.p, 0, words * 4, h->stream));
        const dim3 pg((unsigned)((nmax + 255) / 256), m);
        const size_t lds_bytes = ((size_t)8 * h->kw + 4) << h->t.bucket_bits;
        const bool fresh = h->lazy_empty;            // the kernel writes every bucket: it IS the deferred clear
        if (lds_bytes > 65536 && !h->merge.attrs_set[h->kw]) {       // big buckets: past the default limit of dynamic LDS
            int rca = by_width(h, [&](auto KWc) {
                constexpr int KW = decltype(KWc)::value;
                HIPCHK(h, hipFuncSetAttribute((const void *)(km_merge_kernel<KW, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
                HIPCHK(h, hipFuncSetAttribute((const void *)(km_merge_kernel<KW, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
                return KDF_OK;
            });
            if (rca) return rca;
            h->merge.attrs_set[h->kw] = true;
        }
        by_width(h, [&](auto KWc) {
            constexpr int KW = decltype(KWc)::value;
            hipLaunchKernelGGL(km_bounds_kernel<KW>, pg, dim3(256), 0, h->stream, h->t, sg, nb, first, last, flag);
            if (fresh) hipLaunchKernelGGL((km_merge_kernel<KW, true>), dim3(nb), dim3(KM_MERGE_THREADS), lds_bytes, h->stream, h->t, sg, nb, first, last, flag, h->ctl);
            else hipLaunchKernelGGL((km_merge_kernel<KW, false>), dim3(nb), dim3(KM_MERGE_THREADS), lds_bytes, h->stream, h->t, sg, nb, first, last, flag, h->ctl);
            hipLaunchKernelGGL(km_insert_guarded_kernel<KW>, pg, dim3(256), 0, h->stream, h->t, sg, flag, h->ctl);
            return 0;
        });
        h->lazy_empty = false;
        h->merge.last_path = 1;
        HIPCHK(h, hipMemcpyAsync(&h->merge.flag_host, flag, 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipGetLastError());
    bool full = false;
    if ((rc = ctl_sync(h, &full))) return rc;
    if (h->merge.last_path == 1 && h->merge.flag_host) h->merge.last_path = 2;     // a segment was not grouped: the atomic kernel did the work
    if ((rc = long_bad_keys(h, fn))) return rc;
    if (full) return fail(h, KDF_ERR_TABLE_FULL, "%s: bucket overflow", fn);
    return KDF_OK;
}

static int add_pairs_dev(kdf_engine *h, const uint64_t *d_lo, const uint64_t *d_hi, const uint32_t *d_cnt, uint64_t n, const char *fn) {
    return add_pairs_multi(h, 1, &d_lo, &d_hi, &d_cnt, &n, fn);
}

int kdf_add_pairs_multi_dev(kdf_engine *h, uint32_t nseg, const void *const *d_keys_lo, const void *const *d_keys_hi,
                            const void *const *d_counts, const uint64_t *n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_REFUSE_LONG_MULTI(h, "kdf_add_pairs_multi_dev");
    if (nseg == 0) return KDF_OK;
    if (!d_keys_lo || !n || !d_counts) return fail(h, KDF_ERR_INVALID, "kdf_add_pairs_multi_dev: NULL pointer");
    if (h->kw == 2 && !d_keys_hi) return fail(h, KDF_ERR_INVALID, "kdf_add_pairs_multi_dev: wide keys need the hi words");
    std::vector<const uint64_t *> lo(nseg), hi(nseg, nullptr);
    std::vector<const uint32_t *> cnt(nseg);
    for (uint32_t s = 0; s < nseg; ++s) {
        lo[s] = (const uint64_t *)d_keys_lo[s]; cnt[s] = (const uint32_t *)d_counts[s];
        if (h->kw == 2) hi[s] = (const uint64_t *)d_keys_hi[s];
        if (n[s] && (!lo[s] || (h->kw == 2 && !hi[s]))) return fail(h, KDF_ERR_INVALID, "kdf_add_pairs_multi_dev: segment %u has NULL keys", s);
    }
    HIPCHK(h, hipSetDevice(h->device));
    return add_pairs_multi(h, nseg, lo.data(), hi.data(), cnt.data(), n, "kdf_add_pairs");
}

int kdf_add_pairs_dev(kdf_engine *h, const void *d_keys_lo, const void *d_keys_hi, const void *d_counts, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_REFUSE_LONG(h, "kdf_add_pairs_dev", "kdf_add_pairs_w_dev");
    if (n && (!d_keys_lo || (h->kw == 2 && !d_keys_hi))) return fail(h, KDF_ERR_INVALID, "kdf_add_pairs_dev: NULL keys");
    HIPCHK(h, hipSetDevice(h->device));
    return add_pairs_dev(h, (const uint64_t *)d_keys_lo, (const uint64_t *)d_keys_hi, (const uint32_t *)d_counts, n, "kdf_add_pairs");
}

int kdf_add_pairs(kdf_engine *h, const uint64_t *keys_lo, const uint64_t *keys_hi, const uint32_t *counts, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_REFUSE_LONG(h, "kdf_add_pairs", "kdf_add_pairs_w");
    if (n == 0) return KDF_OK;
    if (!keys_lo || (h->kw == 2 && !keys_hi)) return fail(h, KDF_ERR_INVALID, "kdf_add_pairs: NULL keys");
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_add_pairs");
    const int ik = keys_in(c, keys_lo, keys_hi, n), ic = c.in(counts, counts ? n * 4 : 0);
    if (const int rc = c.commit()) return rc;
    return add_pairs_dev(h, c.dev<uint64_t>(ik), c.dev<uint64_t>(ik + 1), c.dev<uint32_t>(ic), n, "kdf_add_pairs");
}

int kdf_set_counts_dev(kdf_engine *h, const void *d_keys_lo, const void *d_keys_hi, const void *d_counts, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_REFUSE_LONG_MULTI(h, "kdf_set_counts_dev");
    if (n == 0) return KDF_OK;
    if (!d_keys_lo || !d_counts || (h->kw == 2 && !d_keys_hi)) return fail(h, KDF_ERR_INVALID, "kdf_set_counts_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = pending_flush(h))) return rc;
    if ((rc = materialize(h))) return rc;
    h->zero_keys = true;
    by_width(h, [&](auto KWc) {
        constexpr int KW = decltype(KWc)::value;
        hipLaunchKernelGGL(kdf_set_counts_kernel<KW>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const uint64_t *)d_keys_lo,
                           KW == 2 ? (const uint64_t *)d_keys_hi : nullptr, (const uint32_t *)d_counts, n, h->t, h->ctl);
        return 0;
    });
    HIPCHK(h, hipGetLastError());
    bool bad = false;
    if ((rc = ctl_sync(h, &bad))) return rc;
    if (bad) {
        HIPCHK(h, hipMemsetAsync(&h->ctl->error, 0, 4, h->stream));
        return fail(h, KDF_ERR_INVALID, "kdf_set_counts_dev: a key is not stored in the table");
    }
    return KDF_OK;
}

int kdf_count_reads_filtered_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    StreamSrc src;
    const int rc = src_dev(h, "kdf_count_reads_filtered_dev", d_packed, d_invalid, n_bases, src);
    return rc ? rc : count_filtered_dev(h, src.packed, src.invalid, src.n_bases);
}

int kdf_count_reads_filtered(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (!h->filter_mode) return fail(h, KDF_ERR_STATE, "kdf_count_reads_filtered: no filter loaded (kdf_load_filter)");
    HostCall c(h, "kdf_count_reads_filtered");
    StreamSrc src;
    int rc = src_host(c, packed, invalid, n_bases, src);
    if (rc || !src.n_bases || (rc = count_filtered_dev(h, src.packed, src.invalid, src.n_bases))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));   // staging buffers are reused by the next call
    return KDF_OK;
}

// the counts of n keys (device: the (lo, hi) arrays of k <= 63, the rows at lo of long keys) into out (0: absent)
static int query_core(kdf_engine *h, const uint64_t *lo, const uint64_t *hi, uint64_t n, uint32_t *out) {
    { int rcf = pending_flush(h); if (rcf) return rcf; }
    { int rc0 = materialize(h); if (rc0) return rc0; }
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        for (uint64_t off = 0; off < n; off += 1ull << 30) {             // (a launch holds fewer than 2^32 threads)
            const uint64_t m = std::min<uint64_t>(1ull << 30, n - off);
            const unsigned blocks = (unsigned)((m + 255) / 256);
            if constexpr (W <= 2)
                hipLaunchKernelGGL(kdf_query_kernel<W>, dim3(blocks), dim3(256), 0, h->stream, lo + off, W == 2 ? hi + off : nullptr, m, h->t, out + off);
            else
                hipLaunchKernelGGL(kdf_long_query_kernel<W>, dim3(blocks), dim3(256), 0, h->stream, lo + off * W, m, h->t, out + off, long_top_bits(h));
        }
        return 0;
    });
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

int kdf_query_dev(kdf_engine *h, const void *d_keys_lo, const void *d_keys_hi, uint64_t n, void *d_counts_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_REFUSE_LONG(h, "kdf_query_dev", "kdf_query_w_dev");
    if (n == 0) return KDF_OK;
    if (!d_keys_lo || !d_counts_out || (h->kw == 2 && !d_keys_hi)) return fail(h, KDF_ERR_INVALID, "kdf_query_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    return query_core(h, (const uint64_t *)d_keys_lo, (const uint64_t *)d_keys_hi, n, (uint32_t *)d_counts_out);
}

int kdf_query(kdf_engine *h, const uint64_t *keys_lo, const uint64_t *keys_hi, uint64_t n, uint32_t *counts_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_REFUSE_LONG(h, "kdf_query", "kdf_query_w");
    if (n == 0) return KDF_OK;
    if (!keys_lo || !counts_out || (h->kw == 2 && !keys_hi)) return fail(h, KDF_ERR_INVALID, "kdf_query: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_query");
    const int ik = keys_in(c, keys_lo, keys_hi, n), io = c.out(counts_out, n * 4);
    int rc;
    if ((rc = c.commit()) || (rc = query_core(h, c.dev<uint64_t>(ik), c.dev<uint64_t>(ik + 1), n, c.dev<uint32_t>(io))) || (rc = c.fetch(io, n * 4))) return rc;
    return c.finish();
}

static int export_pass(kdf_engine *h, uint32_t min_count, bool write, uint64_t *olo, uint64_t *ohi,
                       uint32_t *ocnt, uint64_t out_cap, uint64_t *n_out) {
    // passes pending: the flush that applies them holds every bucket of the table in LDS once -- it writes the dump too
    // (kb_bucket_kernel, KbPlan::dump_min) unless a bucket took another way (overflow replay, heavy-bucket split)
    const bool fuse = write && min_count >= 1 && h->opt_fused_dump && !h->filter_mode && olo && (h->kw == 1 || ohi) && (h->kb.ring.undumped_passes() || h->kb.l1.tiles > 0);
    KbDump dump{min_count, olo, ohi, ocnt, out_cap};
    { int rcf = pending_flush(h, fuse ? &dump : nullptr); if (rcf) return rcf; }
    if (dump.done) { *n_out = dump.n; return KDF_OK; }
    { int rc0 = materialize(h); if (rc0) return rc0; }
    HIPCHK(h, hipMemsetAsync(h->ctl->tally, 0, sizeof(h->ctl->tally) + 8, h->stream));   // tally[] + cursor
    const uint64_t waves = (h->cap + KDF_EXPORT_ROWS * 64 - 1) / (KDF_EXPORT_ROWS * 64);
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        if constexpr (W > 2) {                                     // rows of W words into olo
            if (write) hipLaunchKernelGGL((kdf_long_export_kernel<W, true>), dim3(blocks), dim3(256), 0, h->stream, h->t, min_count, h->ctl, olo, ocnt, out_cap);
            else hipLaunchKernelGGL((kdf_long_export_kernel<W, false>), dim3(blocks), dim3(256), 0, h->stream, h->t, min_count, h->ctl, olo, ocnt, out_cap);
        } else if (write) {                                        // one read of the table (any min_count: occupancy is tested on the key)
            const unsigned rows = W == 1 ? KDF_EXPORT1_ROWS : KDF_EXPORT1_ROWS / 2;
            const uint64_t w1 = (h->cap + rows * 64 - 1) / (rows * 64);
            const unsigned wpb = KDF_EXPORT1_THREADS / 64;
            hipLaunchKernelGGL(kdf_export1_kernel<W>, dim3((unsigned)((w1 + wpb - 1) / wpb)), dim3(KDF_EXPORT1_THREADS), 0, h->stream, h->t, min_count, h->ctl, olo, ohi, ocnt, out_cap);
        } else {
            hipLaunchKernelGGL((kdf_export_kernel<W, false>), dim3(blocks), dim3(256), 0, h->stream, h->t, min_count, h->ctl, olo, ohi, ocnt, out_cap);
        }
        return 0;
    });
    HIPCHK(h, hipGetLastError());
    uint64_t cursor = 0;
    int rc = ctl_sync(h, nullptr, &cursor);
    if (rc) return rc;
    *n_out = cursor;
    return KDF_OK;
}

// The sender's half of the multi-GPU merge (kdf_merge.h): the table in hash order, one contiguous range per owner.
// packed: d_lo is the byte buffer of the packed layout, cap its size in bytes, part_bytes_out[parts + 1] the segment offsets.
static int export_parts(kdf_engine *h, uint32_t min_count, uint32_t parts, bool packed, void *d_lo, void *d_hi, void *d_cnt,
                        uint64_t cap, uint64_t *part_counts_out, uint64_t *part_bytes_out, uint64_t *n_out, const char *who) {
    if (parts < 1 || parts > KDF_SHARDS) return fail(h, KDF_ERR_INVALID, "%s: parts must be 1..%d", who, KDF_SHARDS);
    HIPCHK(h, hipSetDevice(h->device));
    { int rcf = pending_flush(h); if (rcf) return rcf; }
    { int rc0 = materialize(h); if (rc0) return rc0; }
    if (h->t.hshift) return fail(h, KDF_ERR_STATE, "%s: an owner table (hash_shift) is not dumped by owner again", who);
    if (h->t.log2cap < 28)                                  // an owner boundary (a 16-bit hash prefix) must be a block boundary
        return fail(h, KDF_ERR_STATE, "%s: table of 2^%u slots is too small for an owner-ordered dump (needs 2^28)", who, h->t.log2cap);
    const bool have_out = d_lo && (packed || h->kw == 1 || d_hi);
    const uint64_t nblk = h->cap / KM_BLOCK_SLOTS;
    // a big bucket is two dump blocks: its entries are dumped by the block they are homed in (kdf_merge.h, NH)
    const bool big = (1ull << h->t.bucket_bits) > KM_BLOCK_SLOTS;
    if (big && (h->kw != 1 || (1ull << h->t.bucket_bits) != 2 * KM_BLOCK_SLOTS))
        return fail(h, KDF_ERR_STATE, "%s: no owner-ordered dump for buckets of 2^%u slots", who, h->t.bucket_bits);
    // scratch: blk_off u64[nblk + 1] | part_first u64[S] | part_off u64[S + 1] | part_base u64[S + 1] | blk_cnt u32[nblk]
    const size_t off_words = nblk + 1 + KDF_SHARDS + 2 * (KDF_SHARDS + 1);
    int rc = eng_reserve(h, h->merge.scratch, off_words * 8 + nblk * 4, slack_exact);
    if (rc) return rc;
    unsigned long long *blk_off = h->merge.scratch.as<unsigned long long>();
    uint64_t *part_first = (uint64_t *)(blk_off + nblk + 1);
    unsigned long long *part_off = (unsigned long long *)(part_first + KDF_SHARDS);
    unsigned long long *part_base = part_off + KDF_SHARDS + 1;
    uint32_t *blk_cnt = (uint32_t *)(part_base + KDF_SHARDS + 1);
    std::vector<uint64_t> pf(KDF_SHARDS, 0);
    for (uint32_t p = 0; p < parts; ++p) {                  // first 16-bit hash prefix t with ((t * parts) >> 16) == p
        const uint64_t t16 = ((uint64_t)p * 65536 + parts - 1) / parts;
        pf[p] = (t16 << (h->t.log2cap - 16)) / KM_BLOCK_SLOTS;
    }
    HIPCHK(h, hipMemcpyAsync(part_first, pf.data(), KDF_SHARDS * 8, hipMemcpyHostToDevice, h->stream));
    std::vector<unsigned long long> po(2 * (KDF_SHARDS + 1), 0);
    const uint32_t esz = 8u * h->kw + 4u;
    auto dump = [&](auto KWc, auto NHc) {
        constexpr int KW = decltype(KWc)::value, NH = decltype(NHc)::value;
        hipLaunchKernelGGL((km_count_kernel<KW, NH>), dim3((unsigned)nblk), dim3(KM_THREADS), 0, h->stream, h->t, min_count, blk_cnt);
        hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(1024), 0, h->stream, blk_cnt, blk_off, nblk, part_first, parts, part_off);
        hipLaunchKernelGGL(km_packbase_kernel, dim3(1), dim3(64), 0, h->stream, part_off, parts, esz, part_base);
        if (have_out && packed)
            hipLaunchKernelGGL((km_write_kernel<KW, true, NH>), dim3((unsigned)nblk), dim3(KM_THREADS), 0, h->stream, h->t, min_count, blk_off,
                               (uint64_t *)d_lo, (uint64_t *)nullptr, (uint32_t *)nullptr, cap, part_off, part_base, parts);
        else if (have_out)
            hipLaunchKernelGGL((km_write_kernel<KW, false, NH>), dim3((unsigned)nblk), dim3(KM_THREADS), 0, h->stream, h->t, min_count, blk_off,
                               (uint64_t *)d_lo, h->kw == 2 ? (uint64_t *)d_hi : nullptr, (uint32_t *)d_cnt, cap, part_off, part_base, parts);
        return 0;
    };
    if (big) dump(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
    else by_width(h, [&](auto KWc) { return dump(KWc, std::integral_constant<int, 1>{}); });
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(po.data(), part_off, 2 * (KDF_SHARDS + 1) * 8, hipMemcpyDeviceToHost, h->stream));   // part_off | part_base
    HIPCHK(h, hipStreamSynchronize(h->stream));             // the one synchronisation of the dump (pf / po are pageable)
    const uint64_t n = po[parts];
    for (uint32_t p = 0; p < parts; ++p) part_counts_out[p] = po[p + 1] - po[p];
    if (part_bytes_out) for (uint32_t p = 0; p <= parts; ++p) part_bytes_out[p] = po[KDF_SHARDS + 1 + p];
    *n_out = n;
    if (n == 0) return KDF_OK;
    const uint64_t need = packed ? po[KDF_SHARDS + 1 + parts] : n;
    if (need > cap) return fail(h, KDF_ERR_INVALID, "%s: %llu %s, room for %llu", who, (unsigned long long)need, packed ? "bytes" : "entries", (unsigned long long)cap);
    if (!have_out) return fail(h, KDF_ERR_INVALID, "%s: NULL output", who);
    return KDF_OK;
}

int kdf_export_parts_dev(kdf_engine *h, uint32_t min_count, uint32_t parts, void *d_keys_lo_out, void *d_keys_hi_out,
                         void *d_counts_out, uint64_t cap, uint64_t *part_counts_out, uint64_t *n_out) {
    if (!h || !n_out || !part_counts_out) return fail(h, KDF_ERR_INVALID, "kdf_export_parts_dev: NULL pointer");
    KDF_REFUSE_LONG_MULTI(h, "kdf_export_parts_dev");
    return export_parts(h, min_count, parts, false, d_keys_lo_out, d_keys_hi_out, d_counts_out, cap, part_counts_out, nullptr, n_out,
                        "kdf_export_parts_dev");
}

int kdf_export_parts_packed_dev(kdf_engine *h, uint32_t min_count, uint32_t parts, void *d_buf, uint64_t cap_bytes,
                                uint64_t *part_counts_out, uint64_t *part_bytes_out, uint64_t *n_out) {
    if (!h || !n_out || !part_counts_out || !part_bytes_out) return fail(h, KDF_ERR_INVALID, "kdf_export_parts_packed_dev: NULL pointer");
    KDF_REFUSE_LONG_MULTI(h, "kdf_export_parts_packed_dev");
    return export_parts(h, min_count, parts, true, d_buf, nullptr, nullptr, cap_bytes, part_counts_out, part_bytes_out, n_out,
                        "kdf_export_parts_packed_dev");
}

int kdf_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes) {
    if (!free_bytes || !total_bytes) return fail(nullptr, KDF_ERR_INVALID, "kdf_device_memory: NULL pointer");
    size_t f = 0, t = 0;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMemGetInfo(&f, &t);
    if (e != hipSuccess) return fail(nullptr, KDF_ERR_HIP, "kdf_device_memory: %s", hipGetErrorString(e));
    *free_bytes = f; *total_bytes = t;
    return KDF_OK;
}

int kdf_count_ge(kdf_engine *h, uint32_t min_count, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_count_ge: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    return export_pass(h, min_count, false, nullptr, nullptr, nullptr, 0, n_out);
}

// `jellyfish histo` / `jellyfish stats` on the live table (kdf_histo.h): ONE pass over the count array fills the bins
// (device, high + 2 words) and {sum of counts, largest count} in d_out4[0..1]; h_out4[0..1] holds them on return.
static int histo_pass(kdf_engine *h, uint32_t high, unsigned long long *d_bins, const char *fn) {
    if (high > KH_MAX_HIGH) return fail(h, KDF_ERR_INVALID, "%s: high = %u is above the limit of %u", fn, high, KH_MAX_HIGH);
    { int rcf = pending_flush(h); if (rcf) return rcf; }
    { int rc0 = materialize(h); if (rc0) return rc0; }
    HIPCHK(h, hipMemsetAsync(d_bins, 0, ((size_t)high + 2) * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_out4, 0, 2 * sizeof(unsigned long long), h->stream));
    // the word that tells an empty slot from a key with count 0, read only when the table can hold such keys
    const uint64_t *occ = !h->zero_keys ? nullptr : h->kw == 1 ? h->t.lo : h->t.hi + ((uint64_t)(h->kw - 2) << h->t.log2cap);
    const uint64_t wgs = (h->cap / 4 + (uint64_t)KH_THREADS * KH_UNROLL - 1) / ((uint64_t)KH_THREADS * KH_UNROLL);
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(wgs, (uint64_t)h->n_cu * KH_WG_PER_CU));
    EvSpan span(h->timer[T_HISTO], h->prof, h->stream);
    hipLaunchKernelGGL(kdf_histo_kernel, dim3(grid), dim3(KH_THREADS), 0, h->stream, h->t.cnt, occ, h->cap, high, d_bins, h->d_out4);
    HIPCHK(h, hipGetLastError());                                    // (a launch that failed is not timed)
    span.stop();
    HIPCHK(h, hipMemcpyAsync(h->h_out4, h->d_out4, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return KDF_OK;
}

int kdf_histogram_dev(kdf_engine *h, uint32_t high, void *d_bins_out) {
    if (!h || !d_bins_out) return fail(h, KDF_ERR_INVALID, "kdf_histogram_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    return histo_pass(h, high, (unsigned long long *)d_bins_out, "kdf_histogram_dev");
}

int kdf_histogram(kdf_engine *h, uint32_t high, uint64_t *bins_out) {
    if (!h || !bins_out) return fail(h, KDF_ERR_INVALID, "kdf_histogram: NULL pointer");
    if (high > KH_MAX_HIGH) return fail(h, KDF_ERR_INVALID, "kdf_histogram: high = %u is above the limit of %u", high, KH_MAX_HIGH);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t bytes = ((size_t)high + 2) * 8;
    HostCall c(h, "kdf_histogram");
    const int ib = c.out(bins_out, bytes);
    int rc;
    if ((rc = c.commit()) || (rc = histo_pass(h, high, c.dev<unsigned long long>(ib), "kdf_histogram")) || (rc = c.fetch(ib, bytes))) return rc;
    return c.finish();
}

int kdf_count_stats(kdf_engine *h, uint64_t *unique, uint64_t *distinct, uint64_t *total, uint64_t *max_count) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    uint64_t bins[3] = {0, 0, 0};                      // count 0, count 1, above 1: the same kernel with high = 1
    int rc = kdf_histogram(h, 1, bins);
    if (rc) return rc;
    if (unique) *unique = bins[1];
    if (distinct) *distinct = bins[1] + bins[2];
    if (total) *total = h->h_out4[0];
    if (max_count) *max_count = h->h_out4[1];
    return KDF_OK;
}

// The entries with count >= min_count into device buffers (the (lo, hi) arrays of k <= 63 with hi NULL for k <= 32, the
// rows at lo of long keys), sorted if asked; sort_err: the entry point's code for a failed sort.  ONE pass over the table:
// entries are appended through the cursor, nothing is written past `cap`, and the cursor's final value is the number of
// entries the dump holds (kdf_count_ge gives it beforehand).
static int export_core(kdf_engine *h, uint32_t min_count, uint64_t *lo, uint64_t *hi, uint32_t *cnt, uint64_t cap, bool sorted,
                       uint64_t *n_out, const char *fn, int sort_err) {
    uint64_t n = 0;
    int rc = export_pass(h, min_count, true, lo, hi, cnt, cap, &n);
    if (rc) return rc;
    *n_out = n;
    if (n > cap) return fail(h, KDF_ERR_INVALID, "%s: %llu entries, room for %llu", fn, (unsigned long long)n, (unsigned long long)cap);
    if (sorted && n) {
        if (!cnt) return fail(h, KDF_ERR_INVALID, "%s: sorted export needs the counts array", fn);
        std::string serr;
        if (is_long(h) ? kdf_sort_rows_device(lo, h->kw, cnt, n, h->stream, serr) : kdf_sort_pairs_device(lo, hi, cnt, n, h->stream, serr))
            return fail(h, sort_err, "%s: sort failed: %s", fn, serr.c_str());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return KDF_OK;
}

// the host forms: a counting pass sizes the dump, which is staged, sorted and copied back
static int export_host(kdf_engine *h, uint32_t min_count, uint64_t *lo_out, uint64_t *hi_out, uint32_t *cnt_out, uint64_t cap,
                       uint64_t *n_out, const char *fn, int sort_err) {
    HIPCHK(h, hipSetDevice(h->device));
    uint64_t n = 0;
    int rc = export_pass(h, min_count, false, nullptr, nullptr, nullptr, 0, &n);
    if (rc) return rc;
    *n_out = n;
    if (n == 0) return KDF_OK;
    if (n > cap) return fail(h, KDF_ERR_INVALID, "%s: %llu entries, room for %llu", fn, (unsigned long long)n, (unsigned long long)cap);
    if (!lo_out || (h->kw == 2 && !hi_out)) return fail(h, KDF_ERR_INVALID, "%s: NULL key output", fn);
    HostCall c(h, fn);
    const size_t lo_bytes = n * 8 * lo_words(h), hi_bytes = h->kw == 2 ? n * 8 : 0;
    const int ilo = c.out(lo_out, lo_bytes), ihi = c.out(hi_out, hi_bytes), icnt = c.out(cnt_out, n * 4);    // (the sort needs the counts)
    if ((rc = c.commit())) return rc;
    uint64_t n2 = 0;
    if ((rc = export_core(h, min_count, c.dev<uint64_t>(ilo), c.dev<uint64_t>(ihi), c.dev<uint32_t>(icnt), n, true, &n2, fn, sort_err))) return rc;
    if (n2 != n) return fail(h, KDF_ERR_STATE, "%s: table changed between passes", fn);
    if (h->kw != 2 && hi_out) memset(hi_out, 0, n * 8);
    if ((rc = c.fetch(ilo, lo_bytes)) || (rc = c.fetch(ihi, hi_bytes)) || (rc = c.fetch(icnt, n * 4))) return rc;
    return c.finish();
}

int kdf_export_ge(kdf_engine *h, uint32_t min_count, uint64_t *keys_lo_out, uint64_t *keys_hi_out,
                  uint32_t *counts_out, uint64_t cap, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_export_ge: NULL pointer");
    KDF_REFUSE_LONG(h, "kdf_export_ge", "kdf_export_ge_w");
    return export_host(h, min_count, keys_lo_out, keys_hi_out, counts_out, cap, n_out, "kdf_export_ge", KDF_ERR_HIP);
}

int kdf_export_ge_dev(kdf_engine *h, uint32_t min_count, void *d_keys_lo_out, void *d_keys_hi_out,
                      void *d_counts_out, uint64_t cap, int sorted, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_export_ge_dev: NULL pointer");
    KDF_REFUSE_LONG(h, "kdf_export_ge_dev", "kdf_export_ge_w_dev");
    HIPCHK(h, hipSetDevice(h->device));
    if (cap && (!d_keys_lo_out || (h->kw == 2 && !d_keys_hi_out))) return fail(h, KDF_ERR_INVALID, "kdf_export_ge_dev: NULL key output");
    return export_core(h, min_count, (uint64_t *)d_keys_lo_out, h->kw == 2 ? (uint64_t *)d_keys_hi_out : nullptr, (uint32_t *)d_counts_out,
                       cap, sorted != 0, n_out, "kdf_export_ge_dev", KDF_ERR_HIP);
}

int kdf_scan_reads_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases, void *d_hit_bits) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n_bases == 0) return KDF_OK;
    if (!d_packed || !d_invalid || !d_hit_bits) return fail(h, KDF_ERR_INVALID, "kdf_scan_reads_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    { int rcf = pending_flush(h); if (rcf) return rcf; }
    { int rc0 = materialize(h); if (rc0) return rc0; }
    const uint64_t n_tiles = (n_bases + KDF_TILE - 1) / KDF_TILE;
    if (is_long(h) && h->opt_long_sieve && h->opt_force_path != 1) {
        // long keys (option "long_sieve"): survivors probe in place and the tile's hit word is stored whole -- any stream length
        int rc = long_sieve_ensure(h);
        if (rc) return rc;
        if (h->sieve.valid) {
            h->last_scan_path = 3;
            launch_long_sieve(h, (const uint64_t *)d_packed, (const uint64_t *)d_invalid, n_tiles, n_bases, (uint64_t *)d_hit_bits,
                              h->sieve.words <= KDF_SV_LDS_WORDS && !(h->opt_debug_flags & 2048));
            HIPCHK(h, hipGetLastError());
            return KDF_OK;
        }
    }
    if (!is_long(h) && h->opt_force_path != 1 && n_tiles * KDF_TILE < (1ull << 32)) {
        // through the membership sieve (section 3.5 of DESIGN.md): an index that was loaded with kdf_add_pairs has none yet
        int rc;
        if (!h->sieve.valid) {
            if ((rc = ctl_sync(h, nullptr))) return rc;
            if ((rc = sieve_prepare(h, h->distinct))) return rc;
            if (h->sieve.valid) {
                by_width(h, [&](auto KWc) {
                    hipLaunchKernelGGL(kdf_sieve_from_table_kernel<decltype(KWc)::value>, dim3((unsigned)((h->cap + 255) / 256)), dim3(256), 0,
                                       h->stream, h->t, h->sieve.buf.as<uint64_t>(), h->sieve.words - 1);
                    return 0;
                });
                HIPCHK(h, hipGetLastError());
            }
        }
        if (h->sieve.valid) {
            HIPCHK(h, hipMemsetAsync(d_hit_bits, 0, n_tiles * 8, h->stream));
            h->last_scan_path = 3;
            launch_sieve(h, (const uint64_t *)d_packed, (const uint64_t *)d_invalid, n_tiles, n_bases, (unsigned long long *)d_hit_bits,
                         h->sieve.words <= KDF_SV_LDS_WORDS);
            HIPCHK(h, hipGetLastError());
            return KDF_OK;
        }
    }
    h->last_scan_path = 0;
    launch_stream<MODE_SCAN>(h, (const uint64_t *)d_packed, (const uint64_t *)d_invalid, n_tiles, n_bases, (uint64_t *)d_hit_bits);
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

// host-side canonical key of the window at stream position p, used to count the DISTINCT hit k-mers of the few reads
// that carry hits: the smaller of the forward and reverse-complement codes, ceil(2k/64) words, word 0 least significant
// (kdf_canonical_w's rule), the unused words 0
static std::array<uint64_t, 7> host_window_key(const uint64_t *packed, uint64_t p, int k) {
    const int W = (2 * k + 63) / 64;
    uint64_t f[7] = {0}, r[7] = {0};
    for (int i = 0; i < k; ++i) {
        const uint64_t q = p + i;
        const uint64_t c = (packed[q >> 5] >> ((q & 31) * 2)) & 3;
        // forward: (f << 2) | c; reverse complement: base i lands at bits 2i of r
        for (int j = W - 1; j >= 1; --j) f[j] = (f[j] << 2) | (f[j - 1] >> 62);
        f[0] = (f[0] << 2) | c;
        r[i >> 5] |= (3 - c) << (2 * (i & 31));
    }
    bool lt = false;
    for (int j = W - 1; j >= 0; --j) if (f[j] != r[j]) { lt = f[j] < r[j]; break; }
    std::array<uint64_t, 7> key{};
    for (int j = 0; j < W; ++j) key[j] = lt ? f[j] : r[j];
    return key;
}

int kdf_scan_reads(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases,
                   const int64_t *read_offsets, int64_t n_reads, uint64_t *hit_bits, uint32_t *distinct_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (!hit_bits) return fail(h, KDF_ERR_INVALID, "kdf_scan_reads: hit_bits is NULL");
    uint64_t pw, mw;
    kdf_stream_words(n_bases, &pw, &mw);
    memset(hit_bits, 0, mw * 8);
    if (distinct_out && n_reads > 0) memset(distinct_out, 0, (size_t)n_reads * 4);
    if (n_bases == 0) return KDF_OK;
    if (!packed || !invalid) return fail(h, KDF_ERR_INVALID, "kdf_scan_reads: NULL stream");
    HIPCHK(h, hipSetDevice(h->device));
    const uint64_t n_tiles = (n_bases + KDF_TILE - 1) / KDF_TILE;
    {
        HostCall c(h, "kdf_scan_reads");
        const int is = c.stream(packed, invalid, n_bases), ib = c.out(hit_bits, mw * 8);
        int rc;
        if ((rc = c.commit()) || (rc = kdf_scan_reads_dev(h, c.dev(is), c.dev(is + 1), n_bases, c.dev(ib))) || (rc = c.fetch(ib, n_tiles * 8)) || (rc = c.finish())) return rc;
    }
    if (!read_offsets || !distinct_out) return KDF_OK;
    // distinct hit k-mers per read: only reads with hits are touched
    std::vector<std::array<uint64_t, 7>> keys;
    for (int64_t r = 0; r < n_reads; ++r) {
        const uint64_t b = (uint64_t)read_offsets[r], e = (uint64_t)read_offsets[r + 1];
        keys.clear();
        for (uint64_t wd = b >> 6; wd <= (e ? (e - 1) >> 6 : 0) && wd < n_tiles; ++wd) {
            uint64_t bits = hit_bits[wd];
            while (bits) {
                const int bit = __builtin_ctzll(bits);
                bits &= bits - 1;
                const uint64_t p = (wd << 6) + bit;
                if (p < b || p >= e) continue;
                keys.push_back(host_window_key(packed, p, h->k));
            }
        }
        if (keys.empty()) continue;
        std::sort(keys.begin(), keys.end());
        distinct_out[r] = (uint32_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
    }
    return KDF_OK;
}

// ---- long keys (odd k 65..201): W-word keys, row-major -----------------------------------------------------------
#define KDF_NEED_LONG(h, fn) \
    do { if (!is_long(h)) return fail(h, KDF_ERR_INVALID, "%s: takes engines for odd k 65..%d only (k=%d: use the (lo, hi) form)", fn, KDF_LONG_MAX_K, (h)->k); } while (0)

// ------------------------------------------------------------ two-pass counting ----

int kdf_prefilter_begin(kdf_engine *h, uint32_t min_count, uint32_t log2_cells) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (h->pf.state != PF_OFF)
        return fail(h, KDF_ERR_STATE, "kdf_prefilter_begin: a prefilter is already %s; kdf_prefilter_drop first", h->pf.state == PF_ARMED ? "armed" : "tallying");
    if (min_count != 2 && min_count != 3)
        return fail(h, KDF_ERR_INVALID, "kdf_prefilter_begin: min_count %u: must be 2 or 3 (1 is the plain count; a cell saturates at 3: for a dump "
                                        "with -L above 3 ask for 3 and dump with the larger bound)", min_count);
    if (log2_cells != 0 && (log2_cells < KDF_PF_MIN_LOG2 || log2_cells > KDF_PF_MAX_LOG2))
        return fail(h, KDF_ERR_INVALID, "kdf_prefilter_begin: log2_cells %u: must be %d..%d, or 0 for the engine's choice", log2_cells, KDF_PF_MIN_LOG2, KDF_PF_MAX_LOG2);
    if (h->opt_key_parts > 1) return fail(h, KDF_ERR_STATE, "kdf_prefilter_begin: key_parts = %u is set: a prefilter counts the whole key space in one table (set key_parts to 0 first)", h->opt_key_parts);
    if (h->opt_hash_shift) return fail(h, KDF_ERR_STATE, "kdf_prefilter_begin: hash_shift = %u is set: an owner table of the multi-GPU merge takes no prefilter (a rank sees only its shard of the reads)", h->opt_hash_shift);
    HIPCHK(h, hipSetDevice(h->device));
    { int rcf = pending_flush(h); if (rcf) return rcf; }
    if (log2_cells == 0) log2_cells = std::min<uint32_t>(KDF_PF_MAX_LOG2, std::max<uint32_t>(KDF_PF_MIN_LOG2, log2ceil(8 * std::max<uint64_t>(h->capacity_hint, 1))));
    const uint64_t bytes = 1ull << (log2_cells - 1);              // half a byte per cell
    hipError_t e = h->pf.words.alloc(bytes);
    if (e == hipSuccess) e = h->pf.ctr.alloc((KDF_SHARDS * 16 + 4) * 8);
    if (e != hipSuccess) {
        pf_free(h);
        return fail(h, e == hipErrorOutOfMemory ? KDF_ERR_NOMEM : KDF_ERR_HIP, "kdf_prefilter_begin: a sieve of 2^%u cells (%.1f GB) does not fit the device (%s)",
                    log2_cells, (double)bytes / 1e9, hipGetErrorString(e));
    }
    h->pf.view.words = h->pf.words.as<unsigned long long>(); h->pf.view.log2_cells = log2_cells; h->pf.view.min_count = min_count;
    HIPCHK(h, hipMemsetAsync(h->pf.words.p, 0, bytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->pf.ctr.p, 0, (KDF_SHARDS * 16 + 4) * 8, h->stream));
    h->pf.state = PF_TALLYING;
    h->pf.merged_words = 0;
    return KDF_OK;
}

int kdf_prefilter_add_reads_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    PF_NEED_TALLYING(h, "kdf_prefilter_add_reads_dev");
    StreamSrc src;
    const int rc = src_dev(h, "kdf_prefilter_add_reads_dev", d_packed, d_invalid, n_bases, src);
    return rc ? rc : pf_tally_dev(h, src.packed, src.invalid, src.n_bases);
}

int kdf_prefilter_add_reads(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    PF_NEED_TALLYING(h, "kdf_prefilter_add_reads");
    HostCall c(h, "kdf_prefilter_add_reads");
    StreamSrc src;
    const int rc = src_host(c, packed, invalid, n_bases, src);
    return rc ? rc : pf_tally_dev(h, src.packed, src.invalid, src.n_bases);
}

int kdf_prefilter_add_uploaded(kdf_engine *h, int slot) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    PF_NEED_TALLYING(h, "kdf_prefilter_add_uploaded");
    StreamSrc src;
    int rc = src_slot(EngSink{h}, "kdf_prefilter_add_uploaded", h, slot, true, true, src, NoRefusal{});
    if (rc || !src.n_bases) return rc;
    rc = pf_tally_dev(h, src.packed, src.invalid, src.n_bases);
    src_release(h, src);
    return rc;
}

int kdf_prefilter_arm(kdf_engine *h) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (h->pf.state != PF_TALLYING)
        return fail(h, KDF_ERR_STATE, "kdf_prefilter_arm: the prefilter is %s; only a tallying prefilter (kdf_prefilter_begin) is armed", h->pf.state == PF_ARMED ? "armed already" : "off");
    h->pf.state = PF_ARMED;
    return KDF_OK;
}

int kdf_prefilter_drop(kdf_engine *h) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (h->pf.state == PF_OFF) return fail(h, KDF_ERR_STATE, "kdf_prefilter_drop: no prefilter (kdf_prefilter_begin)");
    HIPCHK(h, hipSetDevice(h->device));
    { int rcf = pending_flush(h); if (rcf) return rcf; }           // what is pending was admitted under this sieve
    HIPCHK(h, hipStreamSynchronize(h->stream));
    pf_free(h);
    return KDF_OK;
}

int kdf_prefilter_fill(kdf_engine *h, uint64_t cells_by_value[4]) {
    if (!h || !cells_by_value) return fail(h, KDF_ERR_INVALID, "kdf_prefilter_fill: NULL pointer");
    if (h->pf.state == PF_OFF) return fail(h, KDF_ERR_STATE, "kdf_prefilter_fill: no prefilter (kdf_prefilter_begin)");
    HIPCHK(h, hipSetDevice(h->device));
    unsigned long long *out3 = h->pf.ctr.as<unsigned long long>() + KDF_SHARDS * 16;
    const uint64_t n_words = 1ull << (h->pf.view.log2_cells - 4);
    HIPCHK(h, hipMemsetAsync(out3, 0, 3 * 8, h->stream));
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_words + 1023) / 1024, (uint64_t)h->n_cu * 8));
    hipLaunchKernelGGL(kdf_pf_fill_kernel, dim3(grid), dim3(256), 0, h->stream, h->pf.view.words, n_words, out3);
    HIPCHK(h, hipGetLastError());
    unsigned long long ge[3] = {0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(ge, out3, sizeof ge, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    cells_by_value[0] = (1ull << h->pf.view.log2_cells) - ge[0];
    cells_by_value[1] = ge[0] - ge[1];
    cells_by_value[2] = ge[1] - ge[2];
    cells_by_value[3] = ge[2];
    return KDF_OK;
}

// ------------------------------------------------------ device BAM feeder (kdf_bamdev.h) ----

// Blocks the device decoder rejected (status[b] != 0, host copy): inflate each again with zlib and patch its bytes into
// d_out.  The block table (one copy) and the flagged payloads come back from the device: this path is rare (never taken
// for zlib-made files), and the caller owns no host copy of them.  Drains the stream, twice per patched block.
static int bd_fallback(kdf_engine *h, const char *fn, const uint8_t *d_comp, const kdf_bgzf_block *d_blocks, uint64_t n_blocks,
                       uint8_t *d_out, const uint32_t *status) {
    std::vector<uint8_t> comp, data;
    std::vector<kdf_bgzf_block> table;                                // fetched once, when the first flagged block is met
    for (uint64_t b = 0; b < n_blocks; ++b) {
        if (status[b] == KDF_INF_OK) continue;
        if (status[b] == KDF_INF_BOUNDS)
            return fail(h, KDF_ERR_INVALID, "%s: block table entry %llu does not fit the inflated buffer (or states more than 64 KB)", fn, (unsigned long long)b);
        if (table.empty()) {
            table.resize(n_blocks);
            HIPCHK(h, hipMemcpyAsync(table.data(), d_blocks, n_blocks * sizeof(kdf_bgzf_block), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        const kdf_bgzf_block blk = table[b];
        if (blk.isize == 0) continue;                                // (nothing to inflate, as the host reader's bgzf_inflate)
        comp.resize((size_t)blk.comp_len + 1); data.resize((size_t)blk.isize + 1);
        if (blk.comp_len) HIPCHK(h, hipMemcpyAsync(comp.data(), d_comp + blk.comp_off, blk.comp_len, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        z_stream zs; memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) return fail(h, KDF_ERR_NOMEM, "%s: inflateInit2 failed", fn);
        zs.next_in = comp.data(); zs.avail_in = blk.comp_len;
        zs.next_out = data.data(); zs.avail_out = blk.isize;
        const int zr = inflate(&zs, Z_FINISH);
        const bool ok = zr == Z_STREAM_END && zs.avail_out == 0;
        inflateEnd(&zs);
        if (!ok)
            return fail(h, KDF_ERR_IO, "%s: the BGZF block at file offset %llu does not inflate (device status %u, zlib %d)", fn,
                        (unsigned long long)blk.file_off, status[b], zr);
        HIPCHK(h, hipMemcpyAsync(d_out + blk.out_off, data.data(), blk.isize, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));                  // (data is reused by the next block)
        h->bd.stat_fallback++;
    }
    return KDF_OK;
}

static int bd_inflate_launch(kdf_engine *h, const void *d_comp, const void *d_blocks, uint64_t n_blocks, void *d_out, uint64_t out_cap, uint32_t *d_status) {
    if (!n_blocks) return KDF_OK;
    EvSpan span(h->timer[T_BD_INF], h->prof, h->stream);
    hipLaunchKernelGGL(kdf_bd_inflate_kernel, dim3((unsigned)((n_blocks + KDF_BD_WAVES - 1) / KDF_BD_WAVES)), dim3(64 * KDF_BD_WAVES), 0, h->stream,
                       (const uint8_t *)d_comp, (const kdf_bgzf_block *)d_blocks, n_blocks, (uint8_t *)d_out, out_cap, d_status);
    HIPCHK(h, hipGetLastError());
    span.stop();
    return KDF_OK;
}

int kdf_bgzf_inflate_dev(kdf_engine *h, const void *d_comp, const void *d_blocks, uint64_t n_blocks, void *d_out, uint64_t out_cap,
                         void *d_block_status) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n_blocks && (!d_comp || !d_blocks || !d_out)) return fail(h, KDF_ERR_INVALID, "kdf_bgzf_inflate_dev: NULL pointer");
    if (n_blocks > (1ull << 31)) return fail(h, KDF_ERR_INVALID, "kdf_bgzf_inflate_dev: %llu blocks in one call", (unsigned long long)n_blocks);
    if (!n_blocks) return KDF_OK;
    HIPCHK(h, hipSetDevice(h->device));
    uint32_t *d_status = (uint32_t *)d_block_status;
    if (!d_status) {
        const int rc = eng_reserve(h, h->bd.status, n_blocks * 4);
        if (rc) return rc;
        d_status = h->bd.status.as<uint32_t>();
    }
    { const int rc = bd_inflate_launch(h, d_comp, d_blocks, n_blocks, d_out, out_cap, d_status); if (rc) return rc; }
    std::vector<uint32_t> status(n_blocks);
    HIPCHK(h, hipMemcpyAsync(status.data(), d_status, n_blocks * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->bd.opt_host_inflate) for (uint32_t &st : status) if (st == KDF_INF_OK) st = KDF_INF_FORCED;
    return bd_fallback(h, "kdf_bgzf_inflate_dev", (const uint8_t *)d_comp, (const kdf_bgzf_block *)d_blocks, n_blocks, (uint8_t *)d_out, status.data());
}

int kdf_bamdev_decode_dev(kdf_engine *h, const void *d_comp, const void *d_blocks, uint64_t n_blocks, const void *d_subranges, uint64_t n_sub,
                          uint32_t flag_off, int collapse, void *d_packed, void *d_invalid, uint64_t cap_bases, void *d_offsets,
                          uint64_t cap_reads, uint64_t *n_bases, uint64_t *n_reads, uint32_t *sub_status) {
    const char *fn = "kdf_bamdev_decode_dev";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (!d_packed || !d_invalid || !d_offsets || !n_bases || !n_reads || (n_sub && (!d_subranges || !sub_status)) || (n_blocks && (!d_comp || !d_blocks)))
        return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    if (n_blocks > (1ull << 24) || n_sub > (1ull << 24))
        return fail(h, KDF_ERR_INVALID, "%s: %llu blocks / %llu sub-ranges in one batch", fn, (unsigned long long)n_blocks, (unsigned long long)n_sub);
    HIPCHK(h, hipSetDevice(h->device));
    *n_bases = *n_reads = 0;
    // scratch: [0] the inflated span (a BGZF block inflates to <= 64 KB) | [1] block status u32[nb] . sub status u32[ns] .
    // counts[ns] . bases[ns] . totals u64[4] | [2] per-read sequence offsets u64[cap_reads]
    const uint64_t out_cap = n_blocks * KDF_BGZF_MAX_ISIZE;
    const size_t o_sub = (size_t)((n_blocks * 4 + 15) & ~15ull), o_cnt = o_sub + (size_t)((n_sub * 4 + 15) & ~15ull);
    const size_t o_base = o_cnt + (size_t)n_sub * sizeof(KdfBdSubCount), o_tot = o_base + (size_t)n_sub * sizeof(KdfBdSubCount);
    int rc;
    if ((rc = eng_reserve(h, h->bd.inflated, (size_t)out_cap + 8))) return rc;
    if ((rc = eng_reserve(h, h->bd.status, o_tot + 32))) return rc;
    if ((rc = eng_reserve(h, h->bd.read_offs, (size_t)(cap_reads + 1) * 8))) return rc;
    uint8_t *d_out = h->bd.inflated.as<uint8_t>(), *small = h->bd.status.as<uint8_t>();
    uint32_t *d_bst = (uint32_t *)small, *d_sst = (uint32_t *)(small + o_sub);
    KdfBdSubCount *d_cnt = (KdfBdSubCount *)(small + o_cnt), *d_base = (KdfBdSubCount *)(small + o_base);
    uint64_t *d_tot = (uint64_t *)(small + o_tot), *d_src = h->bd.read_offs.as<uint64_t>();
    const kdf_bgzf_block *blocks = (const kdf_bgzf_block *)d_blocks;
    const kdf_bam_subrange *subs = (const kdf_bam_subrange *)d_subranges;
    std::vector<uint32_t> bst(n_blocks);
    uint64_t tot[4] = {0, 0, 0, 0};
    const unsigned walk_grid = (unsigned)((n_sub + 63) / 64);

    if ((rc = bd_inflate_launch(h, d_comp, d_blocks, n_blocks, d_out, out_cap, d_bst))) return rc;
    // count, scan, read the sizes back; a second turn only when a block had to be inflated on the host
    for (int turn = 0; turn < 2; ++turn) {
        EvSpan span(h->timer[T_BD_WALK], h->prof, h->stream, turn == 0);
        if (n_sub) {
            hipLaunchKernelGGL(kdf_bd_walk_kernel<false>, dim3(walk_grid), dim3(64), 0, h->stream, d_out, blocks, n_blocks, out_cap, subs, n_sub,
                               flag_off, collapse, d_cnt, d_sst, (const KdfBdSubCount *)nullptr, (int64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0);
            HIPCHK(h, hipGetLastError());
        }
        hipLaunchKernelGGL(kdf_bd_scan_kernel, dim3(1), dim3(1), 0, h->stream, d_cnt, d_sst, n_sub, d_base, d_tot, (int64_t *)d_offsets, cap_reads);
        HIPCHK(h, hipGetLastError());
        span.stop();
        if (turn == 0 && n_blocks) HIPCHK(h, hipMemcpyAsync(bst.data(), d_bst, n_blocks * 4, hipMemcpyDeviceToHost, h->stream));
        if (n_sub) HIPCHK(h, hipMemcpyAsync(sub_status, d_sst, n_sub * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        bool flagged = false;
        if (turn == 0 && h->bd.opt_host_inflate) for (uint32_t &st : bst) if (st == KDF_INF_OK) st = KDF_INF_FORCED;
        if (turn == 0) for (uint64_t b = 0; b < n_blocks; ++b) flagged |= bst[b] != KDF_INF_OK;
        if (!flagged) break;
        if ((rc = bd_fallback(h, fn, (const uint8_t *)d_comp, blocks, n_blocks, d_out, bst.data()))) return rc;
    }
    const uint64_t nr = tot[0], nbases = tot[1], first_bad = tot[2];
    if (first_bad < n_sub && sub_status[first_bad] == KDF_SUB_CORRUPT)
        return fail(h, KDF_ERR_IO, "%s: corrupt BAM record in sub-range %llu of the batch (field sizes, or a record cut off by the end of the file)", fn,
                    (unsigned long long)first_bad);
    if (nr > cap_reads || nbases > cap_bases)
        return fail(h, KDF_ERR_INVALID, "%s: the batch holds %llu reads / %llu stream positions, the buffers %llu / %llu", fn, (unsigned long long)nr,
                    (unsigned long long)nbases, (unsigned long long)cap_reads, (unsigned long long)cap_bases);
    if (first_bad) {
        EvSpan span(h->timer[T_BD_WALK], h->prof, h->stream, 0);
        hipLaunchKernelGGL(kdf_bd_walk_kernel<true>, dim3((unsigned)((first_bad + 63) / 64)), dim3(64), 0, h->stream, d_out, blocks, n_blocks, out_cap, subs,
                           first_bad, flag_off, collapse, (KdfBdSubCount *)nullptr, (uint32_t *)nullptr, (const KdfBdSubCount *)d_base, (int64_t *)d_offsets,
                           d_src, cap_reads);
        HIPCHK(h, hipGetLastError());
        span.stop();
    }
    {
        EvSpan span(h->timer[T_BD_PACK], h->prof, h->stream);
        const uint64_t n_words = kdf_stream_geom(nbases).mask_words;
        hipLaunchKernelGGL(kdf_bd_pack_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, h->stream, d_out, (const int64_t *)d_offsets,
                           d_src, nr, nbases, n_words, (uint64_t *)d_packed, (uint64_t *)d_invalid);
        HIPCHK(h, hipGetLastError());
        span.stop();
    }
    *n_reads = nr; *n_bases = nbases;
    return KDF_OK;
}

// ------------------------------------------------------ distinct k-mer sketch ----

int kdf_sketch_begin(kdf_engine *h, uint32_t log2_registers) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (h->sk.on) return fail(h, KDF_ERR_STATE, "kdf_sketch_begin: a sketch is already on (2^%u registers); kdf_sketch_drop first", h->sk.view.p);
    if (log2_registers == 0) log2_registers = KDF_SK_DEFAULT_LOG2;
    if (log2_registers < KDF_SK_MIN_LOG2 || log2_registers > KDF_SK_MAX_LOG2)
        return fail(h, KDF_ERR_INVALID, "kdf_sketch_begin: log2_registers %u: must be %d..%d, or 0 for %d", log2_registers, KDF_SK_MIN_LOG2, KDF_SK_MAX_LOG2, KDF_SK_DEFAULT_LOG2);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t m = (size_t)1 << log2_registers;
    hipError_t e = h->sk.cells.alloc(m * 4);
    if (e == hipSuccess) e = h->sk.bytes.alloc(m);
    if (e == hipSuccess) e = h->sk.ctr.alloc(KDF_SHARDS * 16 * 8);
    if (e != hipSuccess) {
        sk_free(h);
        return fail(h, e == hipErrorOutOfMemory ? KDF_ERR_NOMEM : KDF_ERR_HIP, "kdf_sketch_begin: 2^%u registers do not fit the device (%s)", log2_registers, hipGetErrorString(e));
    }
    h->sk.view.cells = h->sk.cells.as<uint32_t>(); h->sk.view.p = log2_registers;
    h->sk.on = true;
    HIPCHK(h, hipMemsetAsync(h->sk.cells.p, 0, m * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(h->sk.ctr.p, 0, KDF_SHARDS * 16 * 8, h->stream));
    return KDF_OK;
}

int kdf_sketch_add_reads_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    SK_NEED_ON(h, "kdf_sketch_add_reads_dev");
    StreamSrc src;
    const int rc = src_dev(h, "kdf_sketch_add_reads_dev", d_packed, d_invalid, n_bases, src);
    return rc ? rc : sk_add_dev(h, src.packed, src.invalid, src.n_bases);
}

int kdf_sketch_add_reads(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    SK_NEED_ON(h, "kdf_sketch_add_reads");
    HostCall c(h, "kdf_sketch_add_reads");
    StreamSrc src;
    const int rc = src_host(c, packed, invalid, n_bases, src);
    return rc ? rc : sk_add_dev(h, src.packed, src.invalid, src.n_bases);
}

int kdf_sketch_add_uploaded(kdf_engine *h, int slot) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    SK_NEED_ON(h, "kdf_sketch_add_uploaded");
    StreamSrc src;                                                 // the slot KEEPS its batch: the caller counts or tallies it next
    int rc = src_slot(EngSink{h}, "kdf_sketch_add_uploaded", h, slot, false, true, src, NoRefusal{});
    if (rc || !src.n_bases) return rc;
    rc = sk_add_dev(h, src.packed, src.invalid, src.n_bases);
    src_release(h, src);
    return rc;
}

int kdf_sketch_registers_dev(kdf_engine *h, void *d_regs_out) {
    if (!h || !d_regs_out) return fail(h, KDF_ERR_INVALID, "kdf_sketch_registers_dev: NULL pointer");
    SK_NEED_ON(h, "kdf_sketch_registers_dev");
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = sk_pack(h, (uint8_t *)d_regs_out); if (rc) return rc; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return KDF_OK;
}

int kdf_sketch_registers(kdf_engine *h, uint8_t *regs_out) {
    if (!h || !regs_out) return fail(h, KDF_ERR_INVALID, "kdf_sketch_registers: NULL pointer");
    SK_NEED_ON(h, "kdf_sketch_registers");
    HIPCHK(h, hipSetDevice(h->device));
    { int rc = sk_pack(h, h->sk.bytes.as<uint8_t>()); if (rc) return rc; }
    HIPCHK(h, hipMemcpyAsync(regs_out, h->sk.bytes.p, (size_t)1 << h->sk.view.p, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return KDF_OK;
}

int kdf_sketch_merge(kdf_engine *h, const uint8_t *regs) {
    if (!h || !regs) return fail(h, KDF_ERR_INVALID, "kdf_sketch_merge: NULL pointer");
    SK_NEED_ON(h, "kdf_sketch_merge");
    const uint32_t m = 1u << h->sk.view.p, top = 65 - h->sk.view.p;
    for (uint32_t i = 0; i < m; ++i)
        if (regs[i] > top) return fail(h, KDF_ERR_INVALID, "kdf_sketch_merge: register %u reads %u: a sketch of 2^%u registers holds ranks 0..%u", i, (unsigned)regs[i], h->sk.view.p, top);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->sk.bytes.p, regs, m, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(kdf_sk_merge_kernel, dim3((m + 255) / 256), dim3(256), 0, h->stream, h->sk.view.cells, m, h->sk.bytes.as<const uint8_t>());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));                    // (the caller's array is its own again)
    return KDF_OK;
}

int kdf_sketch_estimate_registers(const uint8_t *regs, uint32_t log2_registers, double *distinct_out) {
    if (!regs || !distinct_out) return fail(nullptr, KDF_ERR_INVALID, "kdf_sketch_estimate_registers: NULL pointer");
    if (log2_registers < KDF_SK_MIN_LOG2 || log2_registers > KDF_SK_MAX_LOG2)
        return fail(nullptr, KDF_ERR_INVALID, "kdf_sketch_estimate_registers: log2_registers %u: must be %d..%d", log2_registers, KDF_SK_MIN_LOG2, KDF_SK_MAX_LOG2);
    if (!kdf_sk_estimate_host(regs, log2_registers, distinct_out))
        return fail(nullptr, KDF_ERR_INVALID, "kdf_sketch_estimate_registers: a register is above %u, the largest rank of 2^%u registers", 65 - log2_registers, log2_registers);
    return KDF_OK;
}

int kdf_sketch_estimate(kdf_engine *h, double *distinct_out) {
    if (!h || !distinct_out) return fail(h, KDF_ERR_INVALID, "kdf_sketch_estimate: NULL pointer");
    SK_NEED_ON(h, "kdf_sketch_estimate");
    std::vector<uint8_t> regs((size_t)1 << h->sk.view.p);
    { int rc = kdf_sketch_registers(h, regs.data()); if (rc) return rc; }
    if (!kdf_sk_estimate_host(regs.data(), h->sk.view.p, distinct_out)) return fail(h, KDF_ERR_STATE, "kdf_sketch_estimate: a register is out of range");
    return KDF_OK;
}

int kdf_sketch_drop(kdf_engine *h) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    SK_NEED_ON(h, "kdf_sketch_drop");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    sk_free(h);
    return KDF_OK;
}

// [first_word, first_word + n_words) inside the sieve (the prefilter is not off)
#define PF_NEED_RANGE(h, fn) \
    do { const uint64_t total_ = 1ull << ((h)->pf.view.log2_cells - 4); \
         if (first_word > total_ || n_words > total_ - first_word) \
             return fail(h, KDF_ERR_INVALID, "%s: words [%llu, +%llu) reach past the sieve's %llu words (kdf_prefilter_words)", fn, \
                         (unsigned long long)first_word, (unsigned long long)n_words, (unsigned long long)total_); } while (0)

int kdf_prefilter_words(kdf_engine *h, uint64_t *n_words) {
    if (!h || !n_words) return fail(h, KDF_ERR_INVALID, "kdf_prefilter_words: NULL pointer");
    if (h->pf.state == PF_OFF) return fail(h, KDF_ERR_STATE, "kdf_prefilter_words: no prefilter (kdf_prefilter_begin)");
    *n_words = 1ull << (h->pf.view.log2_cells - 4);
    return KDF_OK;
}

int kdf_prefilter_export_dev(kdf_engine *h, uint64_t first_word, uint64_t n_words, void *d_words_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (h->pf.state == PF_OFF) return fail(h, KDF_ERR_STATE, "kdf_prefilter_export_dev: no prefilter (kdf_prefilter_begin)");
    PF_NEED_RANGE(h, "kdf_prefilter_export_dev");
    if (n_words == 0) return KDF_OK;
    if (!d_words_out) return fail(h, KDF_ERR_INVALID, "kdf_prefilter_export_dev: NULL output");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(d_words_out, h->pf.view.words + first_word, n_words * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return KDF_OK;
}

int kdf_prefilter_export(kdf_engine *h, uint64_t first_word, uint64_t n_words, uint64_t *words_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (h->pf.state == PF_OFF) return fail(h, KDF_ERR_STATE, "kdf_prefilter_export: no prefilter (kdf_prefilter_begin)");
    PF_NEED_RANGE(h, "kdf_prefilter_export");
    if (n_words == 0) return KDF_OK;
    if (!words_out) return fail(h, KDF_ERR_INVALID, "kdf_prefilter_export: NULL output");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(words_out, h->pf.view.words + first_word, n_words * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return KDF_OK;
}

// the checks both merge forms share (nothing is written when one fails)
static int pf_merge_check(kdf_engine *h, const char *fn, uint64_t first_word, uint64_t n_words, uint32_t nseg, const void *const *segs) {
    if (h->pf.state != PF_TALLYING)
        return fail(h, KDF_ERR_STATE, "%s: the prefilter is %s; sieves are merged between kdf_prefilter_begin and kdf_prefilter_arm", fn,
                    h->pf.state == PF_ARMED ? "armed (its sieve is immutable: partition-time gates rely on that)" : "off");
    PF_NEED_RANGE(h, fn);
    if (nseg == 0 || nseg > KDF_PF_MAX_SEGS) return fail(h, KDF_ERR_INVALID, "%s: nseg %u: must be 1..%d", fn, nseg, KDF_PF_MAX_SEGS);
    if (!segs) return fail(h, KDF_ERR_INVALID, "%s: NULL segment array", fn);
    for (uint32_t s = 0; s < nseg; ++s)
        if (!segs[s]) return fail(h, KDF_ERR_INVALID, "%s: segment %u is NULL", fn, s);
    return KDF_OK;
}

int kdf_prefilter_merge_dev(kdf_engine *h, uint64_t first_word, uint64_t n_words, uint32_t nseg, const void *const *d_segs, int replace) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    { int rc = pf_merge_check(h, "kdf_prefilter_merge_dev", first_word, n_words, nseg, d_segs); if (rc) return rc; }
    HIPCHK(h, hipSetDevice(h->device));
    return pf_merge_dev(h, first_word, n_words, nseg, (const unsigned long long *const *)d_segs, replace != 0);
}

int kdf_prefilter_merge(kdf_engine *h, uint64_t first_word, uint64_t n_words, uint32_t nseg, const uint64_t *const *segs, int replace) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    { int rc = pf_merge_check(h, "kdf_prefilter_merge", first_word, n_words, nseg, (const void *const *)segs); if (rc) return rc; }
    if (n_words == 0) return KDF_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // staged piece by piece (at most 256 MB of staging): segment s of a piece at s * piece words of the one item
    const uint64_t piece = std::max<uint64_t>(2, std::min<uint64_t>(n_words + (n_words & 1), ((1ull << 25) / nseg) & ~1ull));
    HostCall c(h, "kdf_prefilter_merge");
    const int ist = c.out(nullptr, (size_t)piece * nseg * 8);
    { int rc = c.commit(); if (rc) return rc; }
    unsigned long long *st = c.dev<unsigned long long>(ist);
    const unsigned long long *d[KDF_PF_MAX_SEGS];
    for (uint64_t w0 = 0; w0 < n_words; w0 += piece) {
        const uint64_t m = std::min<uint64_t>(piece, n_words - w0);
        for (uint32_t s = 0; s < nseg; ++s) {
            HIPCHK(h, hipMemcpyAsync(st + (size_t)s * piece, segs[s] + w0, m * 8, hipMemcpyHostToDevice, h->stream));
            d[s] = st + (size_t)s * piece;
        }
        int rc = pf_merge_dev(h, first_word + w0, m, nseg, d, replace != 0);
        if (rc) return rc;
    }
    return c.finish();                                           // (the caller's arrays are free again on return)
}

int kdf_key_words(int k) {
    if (k >= 1 && k <= 32) return 1;
    if (k >= 33 && k <= 63) return 2;
    if (k >= KDF_LONG_MIN_K && k <= KDF_LONG_MAX_K && k % 2 == 1) return (2 * k + 63) / 64;
    return 0;
}

int kdf_add_pairs_w_dev(kdf_engine *h, const void *d_keys, const void *d_counts, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_NEED_LONG(h, "kdf_add_pairs_w_dev");
    if (n && !d_keys) return fail(h, KDF_ERR_INVALID, "kdf_add_pairs_w_dev: NULL keys");
    HIPCHK(h, hipSetDevice(h->device));
    return add_pairs_dev(h, (const uint64_t *)d_keys, nullptr, (const uint32_t *)d_counts, n, "kdf_add_pairs_w");
}

int kdf_add_pairs_w(kdf_engine *h, const uint64_t *keys, const uint32_t *counts, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_NEED_LONG(h, "kdf_add_pairs_w");
    if (n == 0) return KDF_OK;
    if (!keys) return fail(h, KDF_ERR_INVALID, "kdf_add_pairs_w: NULL keys");
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_add_pairs_w");
    const int ik = keys_in(c, keys, nullptr, n), ic = c.in(counts, counts ? n * 4 : 0);
    if (const int rc = c.commit()) return rc;
    return add_pairs_dev(h, c.dev<uint64_t>(ik), nullptr, c.dev<uint32_t>(ic), n, "kdf_add_pairs_w");
}

int kdf_load_filter_w_dev(kdf_engine *h, const void *d_keys, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_NEED_LONG(h, "kdf_load_filter_w_dev");
    if (n && !d_keys) return fail(h, KDF_ERR_INVALID, "kdf_load_filter_w_dev: NULL keys");
    HIPCHK(h, hipSetDevice(h->device));
    return load_filter_core(h, (const uint64_t *)d_keys, nullptr, n, "kdf_load_filter_w");
}

int kdf_load_filter_w(kdf_engine *h, const uint64_t *keys, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_NEED_LONG(h, "kdf_load_filter_w");
    if (n && !keys) return fail(h, KDF_ERR_INVALID, "kdf_load_filter_w: NULL keys");
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_load_filter_w");
    const int ik = keys_in(c, keys, nullptr, n);
    if (const int rc = c.commit()) return rc;
    return load_filter_core(h, c.dev<uint64_t>(ik), nullptr, n, "kdf_load_filter_w");
}

int kdf_query_w_dev(kdf_engine *h, const void *d_keys, uint64_t n, void *d_counts_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_NEED_LONG(h, "kdf_query_w_dev");
    if (n == 0) return KDF_OK;
    if (!d_keys || !d_counts_out) return fail(h, KDF_ERR_INVALID, "kdf_query_w_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    return query_core(h, (const uint64_t *)d_keys, nullptr, n, (uint32_t *)d_counts_out);
}

int kdf_query_w(kdf_engine *h, const uint64_t *keys, uint64_t n, uint32_t *counts_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_NEED_LONG(h, "kdf_query_w");
    if (n == 0) return KDF_OK;
    if (!keys || !counts_out) return fail(h, KDF_ERR_INVALID, "kdf_query_w: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_query_w");
    const int ik = keys_in(c, keys, nullptr, n), io = c.out(counts_out, n * 4);
    int rc;
    if ((rc = c.commit()) || (rc = query_core(h, c.dev<uint64_t>(ik), nullptr, n, c.dev<uint32_t>(io))) || (rc = c.fetch(io, n * 4))) return rc;
    return c.finish();
}

int kdf_export_ge_w_dev(kdf_engine *h, uint32_t min_count, void *d_keys_out, void *d_counts_out, uint64_t cap,
                        int sorted, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_export_ge_w_dev: NULL pointer");
    KDF_NEED_LONG(h, "kdf_export_ge_w_dev");
    HIPCHK(h, hipSetDevice(h->device));
    if (cap && !d_keys_out) return fail(h, KDF_ERR_INVALID, "kdf_export_ge_w_dev: NULL key output");
    return export_core(h, min_count, (uint64_t *)d_keys_out, nullptr, (uint32_t *)d_counts_out, cap, sorted != 0, n_out,
                       "kdf_export_ge_w_dev", KDF_ERR_INVALID);
}

int kdf_export_ge_w(kdf_engine *h, uint32_t min_count, uint64_t *keys_out, uint32_t *counts_out, uint64_t cap,
                    uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_export_ge_w: NULL pointer");
    KDF_NEED_LONG(h, "kdf_export_ge_w");
    return export_host(h, min_count, keys_out, nullptr, counts_out, cap, n_out, "kdf_export_ge_w", KDF_ERR_INVALID);
}

// ---- table join (kdf_join.h) -------------------------------------------------------------------------
// the argument errors of every join entry point, before anything is launched
static int join_refuse(kdf_engine *h, kdf_engine *o, const KdfJoinArgs &a, const char *fn) {
    if (o == h) return fail(h, KDF_ERR_INVALID, "%s: other is the engine itself (a table is not joined with itself)", fn);
    if (a.min_count > a.max_count) return fail(h, KDF_ERR_INVALID, "%s: min_count %u > max_count %u", fn, a.min_count, a.max_count);
    if (!o) return KDF_OK;
    if (o->k != h->k) return fail(h, KDF_ERR_INVALID, "%s: the engines differ in k (%d and %d)", fn, h->k, o->k);
    if (o->device != h->device) return fail(h, KDF_ERR_INVALID, "%s: the engines are on different devices (%d and %d)", fn, h->device, o->device);
    if (a.other_min > a.other_max) return fail(h, KDF_ERR_INVALID, "%s: other_min %u > other_max %u", fn, a.other_min, a.other_max);
    return KDF_OK;
}

// ONE pass over h's table: the selected entries are counted (write = false) or appended through the cursor (keys: the lo
// array of k <= 63 or the rows of long keys); *n_out: how many the join holds.  Synchronises h's stream.
static int join_pass(kdf_engine *h, kdf_engine *o, const KdfJoinArgs &a, bool write, uint64_t *keys, uint64_t *hi, uint32_t *cnt,
                     uint32_t *ocnt, uint64_t out_cap, uint64_t *n_out, const char *fn) {
    int rc;
    if ((rc = pending_flush(h)) || (rc = materialize(h))) return rc;
    if (o) {                                                         // the same gate on the table that is probed
        if ((rc = pending_flush(o)) || (rc = materialize(o))) return fail(h, rc, "%s: other: %s", fn, o->err.c_str());
        HIPCHK(h, hipStreamSynchronize(o->stream));
    }
    HIPCHK(h, hipMemsetAsync(h->ctl->tally, 0, sizeof(h->ctl->tally) + 8, h->stream));   // tally[] + cursor
    const uint64_t per_wg = (uint64_t)KJ_THREADS * kj_rows(h->kw);
    const unsigned blocks = (unsigned)((h->cap + per_wg - 1) / per_wg);
    const KdfTable tb = o ? o->t : KdfTable{};
    EvSpan span(h->timer[T_JOIN], h->prof, h->stream);
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        if constexpr (W > 2) {
            if (write) hipLaunchKernelGGL((kdf_long_join_kernel<W, true>), dim3(blocks), dim3(KJ_THREADS), 0, h->stream, h->t, tb, a, h->ctl, keys, cnt, ocnt, out_cap);
            else hipLaunchKernelGGL((kdf_long_join_kernel<W, false>), dim3(blocks), dim3(KJ_THREADS), 0, h->stream, h->t, tb, a, h->ctl, keys, cnt, ocnt, out_cap);
        } else {
            if (write) hipLaunchKernelGGL((kdf_join_kernel<W, true>), dim3(blocks), dim3(KJ_THREADS), 0, h->stream, h->t, tb, a, h->ctl, keys, hi, cnt, ocnt, out_cap);
            else hipLaunchKernelGGL((kdf_join_kernel<W, false>), dim3(blocks), dim3(KJ_THREADS), 0, h->stream, h->t, tb, a, h->ctl, keys, hi, cnt, ocnt, out_cap);
        }
        return 0;
    });
    HIPCHK(h, hipGetLastError());                                    // (a launch that failed is not timed)
    span.stop();
    uint64_t cursor = 0;
    if ((rc = ctl_sync(h, nullptr, &cursor))) return rc;
    *n_out = cursor;
    return KDF_OK;
}

// the join into device buffers, sorted if asked: the keys are sorted with h's counts, other's counts are looked up
// again over the sorted keys
static int join_core(kdf_engine *h, kdf_engine *o, const KdfJoinArgs &a, uint64_t *keys, uint64_t *hi, uint32_t *cnt, uint32_t *ocnt,
                     uint64_t cap, bool sorted, uint64_t *n_out, const char *fn) {
    uint64_t n = 0;
    int rc = join_pass(h, o, a, true, keys, hi, cnt, sorted ? nullptr : ocnt, cap, &n, fn);
    if (rc) return rc;
    *n_out = n;
    if (n > cap) return fail(h, KDF_ERR_INVALID, "%s: %llu entries, room for %llu", fn, (unsigned long long)n, (unsigned long long)cap);
    if (sorted && n) {
        if (!cnt && !is_long(h)) {                                   // the pair sort carries a payload: a scratch one
            if ((rc = eng_reserve(h, h->merge.scratch, n * 4))) return rc;         // (nothing that fills merge.scratch runs inside a join)
            cnt = h->merge.scratch.as<uint32_t>();
            HIPCHK(h, hipMemsetAsync(cnt, 0, n * 4, h->stream));
        }
        std::string serr;
        if (is_long(h) ? kdf_sort_rows_device(keys, h->kw, cnt, n, h->stream, serr) : kdf_sort_pairs_device(keys, hi, cnt, n, h->stream, serr))
            return fail(h, KDF_ERR_HIP, "%s: sort failed: %s", fn, serr.c_str());
        if (ocnt && !o) HIPCHK(h, hipMemsetAsync(ocnt, 0, n * 4, h->stream));
        if (ocnt && o) {
            const KdfTable tb = o->t;
            by_words(h, [&](auto Wc) {
                constexpr int W = decltype(Wc)::value;
                for (uint64_t off = 0; off < n; off += 1ull << 30) {         // (a launch holds fewer than 2^32 threads)
                    const uint64_t m = std::min<uint64_t>(1ull << 30, n - off);
                    const unsigned blocks = (unsigned)((m + 255) / 256);
                    if constexpr (W <= 2)
                        hipLaunchKernelGGL(kdf_query_kernel<W>, dim3(blocks), dim3(256), 0, h->stream, keys + off, W == 2 ? hi + off : nullptr, m, tb, ocnt + off);
                    else
                        hipLaunchKernelGGL(kdf_long_query_kernel<W>, dim3(blocks), dim3(256), 0, h->stream, keys + off * W, m, tb, ocnt + off, long_top_bits(h));
                }
                return 0;
            });
            HIPCHK(h, hipGetLastError());
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return KDF_OK;
}

// the host forms: the join is staged, sorted and copied back.  A cap below the table's slot count sizes the staging
// buffers itself (the caller has counted: kdf_count_join) and the join is ONE pass; a cap that says nothing about the
// size of the answer (0, or the slot count and more) has a counting pass size them first
static int join_host(kdf_engine *h, kdf_engine *o, const KdfJoinArgs &a, uint64_t *keys_out, uint64_t *hi_out, uint32_t *cnt_out,
                     uint32_t *ocnt_out, uint64_t cap, uint64_t *n_out, const char *fn) {
    uint64_t n = 0, room = cap;
    int rc;
    if (cap == 0 || cap >= h->cap) {
        if ((rc = join_pass(h, o, a, false, nullptr, nullptr, nullptr, nullptr, 0, &n, fn))) return rc;
        *n_out = n;
        if (n == 0) return KDF_OK;
        if (n > cap) return fail(h, KDF_ERR_INVALID, "%s: %llu entries, room for %llu", fn, (unsigned long long)n, (unsigned long long)cap);
        room = n;
    }
    if (!keys_out || (h->kw == 2 && !hi_out)) return fail(h, KDF_ERR_INVALID, "%s: NULL key output", fn);
    HostCall c(h, fn);
    const int ik = c.out(keys_out, room * 8 * lo_words(h)), ihi = c.out(hi_out, h->kw == 2 ? room * 8 : 0);
    const int icnt = c.out(cnt_out, room * 4), iocnt = c.out(ocnt_out, room * 4);
    if ((rc = c.commit())) return rc;
    rc = join_core(h, o, a, c.dev<uint64_t>(ik), c.dev<uint64_t>(ihi), c.dev<uint32_t>(icnt), c.dev<uint32_t>(iocnt), room, true, &n, fn);
    *n_out = n;
    if (rc) return rc;                                               // (more than cap: *n_out says how many)
    if (n == 0) return KDF_OK;
    if (h->kw != 2 && hi_out) memset(hi_out, 0, n * 8);
    if ((rc = c.fetch(ik, n * 8 * lo_words(h))) || (rc = c.fetch(ihi, h->kw == 2 ? n * 8 : 0)) || (rc = c.fetch(icnt, n * 4)) || (rc = c.fetch(iocnt, n * 4))) return rc;
    return c.finish();
}

int kdf_count_join(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count, uint32_t other_min, uint32_t other_max,
                   uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_count_join: NULL pointer");
    const KdfJoinArgs a{min_count, max_count, other_min, other_max, other ? 1 : 0};
    int rc = join_refuse(h, other, a, "kdf_count_join");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return join_pass(h, other, a, false, nullptr, nullptr, nullptr, nullptr, 0, n_out, "kdf_count_join");
}

int kdf_export_join_dev(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count, uint32_t other_min, uint32_t other_max,
                        void *d_keys_lo_out, void *d_keys_hi_out, void *d_counts_out, void *d_other_counts_out, uint64_t cap, int sorted,
                        uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_export_join_dev: NULL pointer");
    KDF_REFUSE_LONG(h, "kdf_export_join_dev", "kdf_export_join_w_dev");
    const KdfJoinArgs a{min_count, max_count, other_min, other_max, other ? 1 : 0};
    int rc = join_refuse(h, other, a, "kdf_export_join_dev");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (cap && (!d_keys_lo_out || (h->kw == 2 && !d_keys_hi_out))) return fail(h, KDF_ERR_INVALID, "kdf_export_join_dev: NULL key output");
    return join_core(h, other, a, (uint64_t *)d_keys_lo_out, h->kw == 2 ? (uint64_t *)d_keys_hi_out : nullptr, (uint32_t *)d_counts_out,
                     (uint32_t *)d_other_counts_out, cap, sorted != 0, n_out, "kdf_export_join_dev");
}

int kdf_export_join(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count, uint32_t other_min, uint32_t other_max,
                    uint64_t *keys_lo_out, uint64_t *keys_hi_out, uint32_t *counts_out, uint32_t *other_counts_out, uint64_t cap,
                    uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_export_join: NULL pointer");
    KDF_REFUSE_LONG(h, "kdf_export_join", "kdf_export_join_w");
    const KdfJoinArgs a{min_count, max_count, other_min, other_max, other ? 1 : 0};
    int rc = join_refuse(h, other, a, "kdf_export_join");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return join_host(h, other, a, keys_lo_out, keys_hi_out, counts_out, other_counts_out, cap, n_out, "kdf_export_join");
}

int kdf_export_join_w_dev(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count, uint32_t other_min, uint32_t other_max,
                          void *d_keys_out, void *d_counts_out, void *d_other_counts_out, uint64_t cap, int sorted, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_export_join_w_dev: NULL pointer");
    KDF_NEED_LONG(h, "kdf_export_join_w_dev");
    const KdfJoinArgs a{min_count, max_count, other_min, other_max, other ? 1 : 0};
    int rc = join_refuse(h, other, a, "kdf_export_join_w_dev");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (cap && !d_keys_out) return fail(h, KDF_ERR_INVALID, "kdf_export_join_w_dev: NULL key output");
    return join_core(h, other, a, (uint64_t *)d_keys_out, nullptr, (uint32_t *)d_counts_out, (uint32_t *)d_other_counts_out, cap,
                     sorted != 0, n_out, "kdf_export_join_w_dev");
}

int kdf_export_join_w(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count, uint32_t other_min, uint32_t other_max,
                      uint64_t *keys_out, uint32_t *counts_out, uint32_t *other_counts_out, uint64_t cap, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_export_join_w: NULL pointer");
    KDF_NEED_LONG(h, "kdf_export_join_w");
    const KdfJoinArgs a{min_count, max_count, other_min, other_max, other ? 1 : 0};
    int rc = join_refuse(h, other, a, "kdf_export_join_w");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return join_host(h, other, a, keys_out, nullptr, counts_out, other_counts_out, cap, n_out, "kdf_export_join_w");
}

// The sender's half of the owner exchange for long keys (kdf_long_merge.h): two passes over the table and one
// synchronisation between them, where the segment offsets are made from the per-owner totals.
int kdf_export_parts_w_packed_dev(kdf_engine *h, uint32_t min_count, uint32_t parts, void *d_buf, uint64_t cap_bytes,
                                  uint64_t *n_out, uint64_t *part_counts, uint64_t *part_offsets) {
    const char *who = "kdf_export_parts_w_packed_dev";
    if (!h || !n_out || !part_counts || !part_offsets) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", who);
    KDF_NEED_LONG(h, who);
    if (parts < 1 || parts > KLM_MAX_PARTS) return fail(h, KDF_ERR_INVALID, "%s: parts must be 1..%d", who, KLM_MAX_PARTS);
    HIPCHK(h, hipSetDevice(h->device));
    { int rcf = pending_flush(h); if (rcf) return rcf; }
    { int rc0 = materialize(h); if (rc0) return rc0; }
    // scratch: part_cnt u64[64] | cursor u64[64] | part_base u64[64]
    int rc = eng_reserve(h, h->merge.scratch, 3 * KLM_MAX_PARTS * 8, slack_exact);
    if (rc) return rc;
    unsigned long long *part_cnt = h->merge.scratch.as<unsigned long long>(), *cursor = part_cnt + KLM_MAX_PARTS, *part_base = cursor + KLM_MAX_PARTS;
    HIPCHK(h, hipMemsetAsync(part_cnt, 0, 2 * KLM_MAX_PARTS * 8, h->stream));        // part_cnt | cursor
    const uint64_t waves = (h->cap + KDF_EXPORT_ROWS * 64 - 1) / (KDF_EXPORT_ROWS * 64);
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    const uint64_t *top = h->t.hi + ((uint64_t)(h->kw - 2) << h->t.log2cap);
    hipLaunchKernelGGL(kdf_long_parts_count_kernel, dim3(blocks), dim3(256), 0, h->stream, h->t, top, min_count, parts, part_cnt);
    HIPCHK(h, hipGetLastError());
    unsigned long long cnt[KLM_MAX_PARTS], base[KLM_MAX_PARTS];
    HIPCHK(h, hipMemcpyAsync(cnt, part_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const uint64_t esz = 8ull * h->kw + 4;
    uint64_t n = 0, off = 0;
    for (uint32_t p = 0; p < KLM_MAX_PARTS; ++p) {
        base[p] = off;
        if (p >= parts) continue;
        part_counts[p] = cnt[p];
        part_offsets[p] = off;
        n += cnt[p];
        off += (cnt[p] * esz + 7) & ~7ull;                     // every segment starts on 8 bytes
    }
    part_offsets[parts] = off;
    *n_out = n;
    if (n == 0) return KDF_OK;
    if (off > cap_bytes)                                        // (nothing was written: pass 2 has not run)
        return fail(h, KDF_ERR_INVALID, "%s: %llu bytes needed, room for %llu", who, (unsigned long long)off, (unsigned long long)cap_bytes);
    if (!d_buf) return fail(h, KDF_ERR_INVALID, "%s: NULL output", who);
    HIPCHK(h, hipMemcpyAsync(part_base, base, sizeof(base), hipMemcpyHostToDevice, h->stream));
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        if constexpr (W > 2)
            hipLaunchKernelGGL(kdf_long_parts_write_kernel<W>, dim3(blocks), dim3(256), 0, h->stream, h->t, min_count, parts,
                               (const unsigned long long *)part_cnt, (const unsigned long long *)part_base, cursor, (unsigned char *)d_buf);
        return 0;
    });
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));                 // (`base` is pageable; the dump is complete on return)
    return KDF_OK;
}

int kdf_set_counts_w_dev(kdf_engine *h, const void *d_keys, const void *d_counts, uint64_t n) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KDF_NEED_LONG(h, "kdf_set_counts_w_dev");
    if (n == 0) return KDF_OK;
    if (!d_keys || !d_counts) return fail(h, KDF_ERR_INVALID, "kdf_set_counts_w_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = pending_flush(h))) return rc;
    if ((rc = materialize(h))) return rc;
    h->zero_keys = true;
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        if constexpr (W > 2)
            for (uint64_t off = 0; off < n; off += 1ull << 30) {     // (a launch holds fewer than 2^32 threads)
                const uint64_t m = std::min<uint64_t>(1ull << 30, n - off);
                hipLaunchKernelGGL(kdf_long_set_counts_kernel<W>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream,
                                   (const uint64_t *)d_keys + off * W, (const uint32_t *)d_counts + off, m, h->t, h->ctl, long_top_bits(h));
            }
        return 0;
    });
    HIPCHK(h, hipGetLastError());
    bool bad = false;
    if ((rc = ctl_sync(h, &bad))) return rc;
    if (bad) {
        HIPCHK(h, hipMemsetAsync(&h->ctl->error, 0, 4, h->stream));
        return fail(h, KDF_ERR_INVALID, "kdf_set_counts_w_dev: a key is not stored in the table");
    }
    return KDF_OK;
}

int kdf_profile(kdf_engine *h, int enable) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    for (EvTimer &t : h->timer) t.reset();
    stage_collect(h);
    h->prof = enable != 0;
    for (double &m : h->prof_stage_ms) m = 0.0;
    h->prof_stage_passes = 0;
    return KDF_OK;
}

int kdf_profile_stages(kdf_engine *h, double *stage_ms4, uint64_t *passes) {
    if (!h || !stage_ms4) return fail(h, KDF_ERR_INVALID, "kdf_profile_stages: NULL pointer");
    stage_collect(h);
    for (int i = 0; i < 4; ++i) stage_ms4[i] = h->prof_stage_ms[i];
    if (passes) *passes = h->prof_stage_passes;
    return KDF_OK;
}

int kdf_profile_read(kdf_engine *h, double *kernel_ms, uint64_t *launches, uint64_t *positions) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    EvTimer &t = h->timer[T_STREAM];
    t.collect();
    if (kernel_ms) *kernel_ms = t.ms;
    if (launches) *launches = t.passes;
    if (positions) *positions = t.tag_sum * KDF_TILE;
    return KDF_OK;
}

int kdf_set_option(kdf_engine *h, const char *name, int64_t value) {
    if (!h || !name) return fail(h, KDF_ERR_INVALID, "kdf_set_option: NULL argument");
    const std::string n(name);
    // options change how the NEXT windows are counted: what is pending was counted under the old ones
    if (n != "debug_flags" && n != "defer_max_bytes") { HIPCHK(h, hipSetDevice(h->device)); int rcf = pending_flush(h); if (rcf) return rcf; }
    if (n == "key_parts" || n == "key_part") {
        const uint32_t parts = n == "key_parts" ? (uint32_t)value : h->opt_key_parts, part = n == "key_part" ? (uint32_t)value : h->opt_key_part;
        if (value < 0 || parts > 65536 || (n == "key_part" && part >= std::max<uint32_t>(parts, 1)))
            return fail(h, KDF_ERR_INVALID, "key_parts must be 0..65536 and key_part below it");
        if (parts > 1 && h->pf.state != PF_OFF)
            return fail(h, KDF_ERR_STATE, "key_parts = %u with a prefilter: a prefilter counts the whole key space in one table (kdf_prefilter_drop first)", parts);
        h->opt_key_parts = parts; h->opt_key_part = n == "key_parts" ? 0 : part;
    }
    else if (n == "binned_min_positions") h->opt_binned_min_positions = (uint64_t)value;
    else if (n == "binned_bytes_per_position") h->opt_binned_bytes_per_position = (uint64_t)value;
    else if (n == "binned_max_positions") {
        if (value < KDF_TILE || value > (1ll << 31)) return fail(h, KDF_ERR_INVALID, "binned_max_positions must be in [64, 2^31]");
        h->opt_binned_max_positions = (uint64_t)value / KDF_TILE * KDF_TILE;      // passes start on tile boundaries
    }
    else if (n == "binned_filtered_min_log2cap") h->opt_binned_filtered_min_log2cap = (uint32_t)value;
    else if (n == "big_bucket_log2cap") {
        if (value < 10 || value > 64) return fail(h, KDF_ERR_INVALID, "big_bucket_log2cap must be 10..64");
        h->opt_big_bucket_log2cap = (uint32_t)value;
        if (bucket_bits_for(h, h->t.log2cap) != h->t.bucket_bits) { int rc = table_rehash(h, h->t.log2cap); if (rc) return rc; }     // same slots, other buckets
    }
    else if (n == "force_path") {
        if (value != 0 && value != 1 && value != 2 && value != 4)
            return fail(h, KDF_ERR_INVALID, "force_path %lld: must be 0 (auto), 1 (direct), 2 (binned) or 4 (sieve, count --if only)", (long long)value);
        if (is_long(h) && (value == 2 || value == 4))
            return fail(h, KDF_ERR_INVALID, "force_path %lld: k=%d counts through the direct kernels only (no binned pipeline or sieve for k > 63)", (long long)value, h->k);
        h->opt_force_path = (int)value;
    }
    else if (n == "merge_min_pairs") h->opt_merge_min_pairs = (uint64_t)value;
    else if (n == "hash_shift") {
        if (value > 8) return fail(h, KDF_ERR_INVALID, "hash_shift must be 0..8");
        if (value != 0 && is_long(h)) return fail(h, KDF_ERR_INVALID, "hash_shift: not available for k > 63 (long keys count on one GPU)");
        if (value != 0 && h->pf.state != PF_OFF)
            return fail(h, KDF_ERR_STATE, "hash_shift = %lld with a prefilter: an owner table of the multi-GPU merge takes no prefilter (kdf_prefilter_drop first)", (long long)value);
        if ((uint32_t)value != h->opt_hash_shift) {
            int rc = ctl_sync(h, nullptr);
            if (rc) return rc;
            if (h->distinct) return fail(h, KDF_ERR_STATE, "hash_shift can only change on an empty table (kdf_clear first)");
        }
        h->opt_hash_shift = (uint32_t)value; h->t.hshift = (uint32_t)value;
    }
    else if (n == "defer") h->opt_defer = value != 0;
    else if (n == "defer_max_bytes") h->opt_defer_max_bytes = (uint64_t)value;
    else if (n == "bamdev_host_inflate") h->bd.opt_host_inflate = value != 0;
    else if (n == "fused_dump") {
        if (value != 0 && is_long(h)) return fail(h, KDF_ERR_INVALID, "fused_dump: not available for k > 63 (no binned pipeline for long keys)");
        h->opt_fused_dump = value != 0;
    }
    else if (n == "lazy_table") {
        if (value != 0 && is_long(h)) return fail(h, KDF_ERR_INVALID, "lazy_table: not available for k > 63 (no binned pipeline for long keys)");
        h->opt_lazy_table = value != 0;
    }
    else if (n == "l1_positions") h->opt_l1_positions = (uint64_t)std::max<int64_t>(value, KDF_TILE);
    else if (n == "l1_direct_positions") h->opt_l1_direct_positions = (uint64_t)std::max<int64_t>(value, 0);
    else if (n == "sieve_bits") { h->opt_sieve_bits = (int)value; h->sieve.unfit = false; bin_sieve_drop(h); }     // (other sizing: the keys may fit now)
    else if (n == "sieve_bins") {
        if (value != 0 && value != 1 && (value < KDF_BS_C1_MIN || value > KDF_BS_C1_MAX))
            return fail(h, KDF_ERR_INVALID, "sieve_bins %lld: must be 0 (off), 1 (coarse bits by the filter's size) or %d..%d coarse bits", (long long)value, KDF_BS_C1_MIN, KDF_BS_C1_MAX);
        if (value != 0 && is_long(h)) return fail(h, KDF_ERR_INVALID, "sieve_bins: not available for k > 63 (no binned pipeline for long keys)");
        if ((int)value != h->opt_sieve_bins) bin_sieve_drop(h);
        h->opt_sieve_bins = (int)value;
    }
    else if (n == "long_sieve") {
        if (!is_long(h)) return fail(h, KDF_ERR_INVALID, "long_sieve: k=%d always takes the sieve where it fits (the option is for k > 63)", h->k);
        if (value != 0 && value != 1) return fail(h, KDF_ERR_INVALID, "long_sieve %lld: must be 0 or 1", (long long)value);
        if (!value) sieve_drop(h);                    // off: the direct kernels from now on; on: built from the table by the next count --if or scan
        h->opt_long_sieve = (int)value;
    }
    else if (n == "debug_flags") h->opt_debug_flags = (uint32_t)value;
    else return fail(h, KDF_ERR_INVALID, "kdf_set_option: unknown option %s", name);
    return KDF_OK;
}

int kdf_get_stat(kdf_engine *h, const char *name, int64_t *value) {
    if (!h || !name || !value) return fail(h, KDF_ERR_INVALID, "kdf_get_stat: NULL argument");
    const std::string n(name);
    bool us = false;
    if (EvTimer *t = timer_of_stat(h->timer, TIMER_NAME, T_COUNT, n, &us)) *value = us ? t->us() : (t->collect(), (int64_t)t->passes);
    else if (n == "binned_passes") *value = (int64_t)h->stat_binned_passes;
    else if (n == "replayed_buckets") *value = (int64_t)h->stat_replayed_buckets;
    else if (n == "prefilter_state") *value = h->pf.state;
    else if (n == "prefilter_min_count") *value = h->pf.view.min_count;
    else if (n == "prefilter_log2_cells") *value = h->pf.view.log2_cells;
    else if (n == "prefilter_bytes") *value = h->pf.state == PF_OFF ? 0 : (int64_t)(1ull << (h->pf.view.log2_cells - 1));
    else if (n == "prefilter_windows") {
        *value = 0;
        if (h->pf.ctr) {                                              // the sharded device counter, summed here
            std::vector<unsigned long long> c(KDF_SHARDS * 16);
            HIPCHK(h, hipSetDevice(h->device));
            HIPCHK(h, hipMemcpyAsync(c.data(), h->pf.ctr.p, c.size() * 8, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (int i = 0; i < KDF_SHARDS; ++i) *value += (int64_t)c[i * 16];
        }
    }
    else if (n == "bamdev_fallback_blocks") *value = (int64_t)h->bd.stat_fallback;
    else if (n == "sketch_state") *value = h->sk.on ? 1 : 0;
    else if (n == "sketch_log2_registers") *value = h->sk.on ? (int64_t)h->sk.view.p : 0;
    else if (n == "sketch_windows") {
        *value = 0;
        if (h->sk.on) {                                               // the sharded device counter, summed here
            HIPCHK(h, hipSetDevice(h->device));
            std::vector<unsigned long long> c(KDF_SHARDS * 16);
            HIPCHK(h, hipMemcpyAsync(c.data(), h->sk.ctr.p, c.size() * 8, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            unsigned long long t = 0;
            for (int i = 0; i < KDF_SHARDS; ++i) t += c[(size_t)i * 16];
            *value = (int64_t)t;
        }
    }
    else if (n == "prefilter_merged_words") *value = h->pf.state == PF_OFF ? 0 : (int64_t)h->pf.merged_words;
    else if (n == "flushes") *value = (int64_t)h->stat_flushes;
    // (pending: not yet applied by any flush.  Passes a dump-only flush has applied are kept in the ring -- "retained_passes" --
    // until the table is asked for or cleared)
    else if (n == "pending_passes") *value = (int64_t)h->kb.ring.undumped_passes();
    else if (n == "pending_positions") *value = (int64_t)(h->kb.ring.undumped_positions() + h->kb.l1.positions());
    else if (n == "retained_passes") *value = (int64_t)h->kb.ring.n_dumped;
    else if (n == "dump_only_flushes") *value = (int64_t)h->stat_dump_only;
    else if (n == "materialisations") *value = (int64_t)h->stat_materialisations;
    else if (n == "lazy_table") *value = h->opt_lazy_table;
    else if (n == "ring_bytes") *value = (int64_t)(h->kb.ring.cap_entries * 8 * h->kw);
    else if (n == "defer") *value = h->opt_defer;
    else if (n == "last_count_path") *value = h->last_path;
    else if (n == "last_scan_path") *value = h->last_scan_path;
    else if (n == "sieve_bins") *value = h->opt_sieve_bins;
    else if (n == "last_sieve_bins") *value = h->last_sieve_bins;
    else if (n == "last_sieve_slice_words") *value = h->last_sieve_slice_words;
    else if (n == "bin_sieve_passes") *value = (int64_t)h->stat_bin_sieve_passes;
    else if (n == "last_sieve_in_lds") *value = h->last_sieve_in_lds;
    else if (n == "last_sieve_rounds") *value = h->last_sieve_rounds;
    else if (n == "long_sieve") *value = h->opt_long_sieve;
    else if (n == "last_merge_path") *value = h->merge.last_path;
    else if (n == "heavy_buckets") *value = (int64_t)h->stat_heavy_buckets;
    else if (n == "fused_dumps") *value = (int64_t)h->stat_fused_dumps;
    else if (n == "fused_dump") *value = h->opt_fused_dump;
    else if (n == "hash_shift") *value = h->opt_hash_shift;
    else if (n == "log2cap") *value = h->t.log2cap;
    else if (n == "bucket_bits") *value = h->t.bucket_bits;
    // the binned path's split of the bucket bits: of the pending passes, or what the next pass would be partitioned with
    else if (n == "c1") *value = (h->kb.ring.empty() ? kb_make_plan(h, h->t) : h->kb.ring.plan).c1;
    else if (n == "c2") *value = (h->kb.ring.empty() ? kb_make_plan(h, h->t) : h->kb.ring.plan).c2;
    else if (n.rfind("trash", 0) == 0 && n.size() > 5 && h->kb.small) {          // (variant builds with -DKB_TIMING: phase cycle sums)
        const int i = atoi(n.c_str() + 5);
        if (i < 0 || i >= 64) return fail(h, KDF_ERR_INVALID, "kdf_get_stat: trash0..trash63");
        unsigned long long v = 0;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(&v, h->kb.small.as<unsigned long long>() + 16 + i, 8, hipMemcpyDeviceToHost));
        *value = (int64_t)v;
    }
    else return fail(h, KDF_ERR_INVALID, "kdf_get_stat: unknown stat %s", name);
    return KDF_OK;
}

}  // extern "C"
