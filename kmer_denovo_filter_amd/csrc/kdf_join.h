// kdf_join.h -- table join: the entries of table A whose count lies in [min_count, max_count] and whose count in table B
// (0 when B does not hold the key, or holds it with count 0: kdf_query's answer) lies in [other_min, other_max].
// One pass over A's slots; nothing but the answer is written.  DESIGN.md 3.15.
//
// Every table of one k stores a key as the same h (kdf_device.h "STORED FORM", kdf_long.h), and kdf_find_narrow /
// kdf_find_wide / kdf_find_long take h: a slot of A probes B as it lies, with B's own geometry (capacity, buckets,
// hash_shift).  The key itself is rebuilt only for the entries that are written.
//
// A workgroup of KJ_THREADS / 64 waves owns KJ_THREADS x kj_rows(W) consecutive slots, a wave kj_rows(W) rows of 64 (8 for
// narrow keys, 4 for wide and long ones, whose rows keep two key words in registers: at 8 rows the long instantiations
// fell to 4-5 waves per SIMD and ran slower than with one probe in flight per lane).  A wave works in three phases of
// loads -- the counts; the key words of the slots whose count passes; the home slots of those keys in B -- and in each
// phase every row's load is requested before the first is looked at (the generated code has ONE s_waitcnt vmcnt(0) behind
// each phase's loads; empty asm statements keep the compiler from pulling a row's first use up to its load).  A probe
// into a table larger than the caches is a dependent HBM miss: what bounds the kernel is how many are in flight.  Only
// then the probe runs are walked.  The selected entries are counted with ballots; the workgroup reserves its output
// range with ONE atomic on ctl->cursor and writes with plain stores.  WRITE = false: the wave's total goes into
// ctl->tally[] and nothing else is written.  Both tables are only read.
#pragma once
#include "kdf_device.h"
#include "kdf_long.h"

#define KJ_THREADS 256
#ifndef KJ_ROWS_NARROW
#define KJ_ROWS_NARROW 8                // rows of 64 slots per wave, k <= 32
#endif
#ifndef KJ_ROWS_WIDE
#define KJ_ROWS_WIDE 4                  // ... wide and long keys: two key words per row in flight, and the registers for them
#endif
constexpr int kj_rows(int W) { return W == 1 ? KJ_ROWS_NARROW : KJ_ROWS_WIDE; }

struct KdfJoinArgs {
    uint32_t min_count, max_count;      // bounds on A's count, inclusive (max_count = UINT32_MAX: none)
    uint32_t other_min, other_max;      // bounds on B's count, inclusive; ignored without B
    int have_other;                     // 0: tb is not read
};

// out_keys: k <= 32 lo[]; wide lo[] and out_hi[] (may be NULL); long: rows of W words
template <int W, bool WRITE>
__device__ __forceinline__ void kdf_join_body(const KdfTable &ta, const KdfTable &tb, const KdfJoinArgs &a, KdfCtl *ctl,
                                              uint64_t *__restrict__ out_keys, uint64_t *__restrict__ out_hi,
                                              uint32_t *__restrict__ ocnt, uint32_t *__restrict__ oocnt, uint64_t out_cap)
{
    __shared__ uint32_t wtot[KJ_THREADS / 64];
    __shared__ unsigned long long wg_base;
    constexpr int KJ_ROWS = kj_rows(W);
    const uint64_t cap = 1ull << ta.log2cap;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * (KJ_THREADS / 64) + wv;
    const uint64_t first = wave * (KJ_ROWS * 64);
    // the word that tells an occupied slot: h for narrow keys, the top key word otherwise
    const uint64_t *atop = W == 1 ? ta.lo : ta.hi + ((uint64_t)(W - 2) << ta.log2cap);
    uint32_t c[KJ_ROWS], oc[KJ_ROWS];
    uint64_t h[KJ_ROWS], top[W >= 2 ? KJ_ROWS : 1], pre[KJ_ROWS];
    unsigned long long kb[KJ_ROWS];
    uint32_t in = 0, cand = 0, tot = 0; // bit r: row r of this lane passes A's bounds / is still in the join
#pragma unroll
    for (int r = 0; r < KJ_ROWS; ++r) { const uint64_t i = first + (uint64_t)r * 64 + lane; c[r] = i < cap ? ta.cnt[i] : 0u; }
#pragma unroll
    for (int r = 0; r < KJ_ROWS; ++r) {
        const uint64_t i = first + (uint64_t)r * 64 + lane;
        if (i < cap && c[r] >= a.min_count && c[r] <= a.max_count) in |= 1u << r;
    }
    // Every load of a phase is requested before the first of them is looked at.  The empty asm statements hold the
    // compiler to that: without them it moves each row's compare with KDF_EMPTY up to the row's load and waits there
    // (vmcnt(0) after every load: one request in flight per lane instead of KJ_ROWS).
#pragma unroll
    for (int r = 0; r < KJ_ROWS; ++r) {
        const uint64_t i = first + (uint64_t)r * 64 + lane;
        h[r] = KDF_EMPTY;
        if constexpr (W >= 2) top[r] = KDF_EMPTY;
        if ((in >> r) & 1) {
            h[r] = ta.lo[i];
            if constexpr (W >= 2) top[r] = atop[i];
        }
    }
#pragma unroll
    for (int r = 0; r < KJ_ROWS; ++r) {
        asm volatile("" : "+v"(h[r]));
        if constexpr (W >= 2) asm volatile("" : "+v"(top[r]));
    }
#pragma unroll
    for (int r = 0; r < KJ_ROWS; ++r)   // (min_count >= 1 implies an occupied slot; with 0 the key word tells)
        if (((in >> r) & 1) && (W == 1 ? h[r] : top[r]) != KDF_EMPTY) cand |= 1u << r;
    if (a.have_other) {
        const uint64_t *btop = W == 1 ? tb.lo : tb.hi + ((uint64_t)(W - 2) << tb.log2cap);
#pragma unroll
        for (int r = 0; r < KJ_ROWS; ++r) {
            pre[r] = KDF_EMPTY;
            if ((cand >> r) & 1) pre[r] = btop[kdf_home(tb, h[r])];
        }
#pragma unroll
        for (int r = 0; r < KJ_ROWS; ++r) asm volatile("" : "+v"(pre[r]));
#pragma unroll
        for (int r = 0; r < KJ_ROWS; ++r) {
            oc[r] = 0;
            if (((cand >> r) & 1) && pre[r] != KDF_EMPTY) {        // an empty home slot: absent, no walk
                uint64_t s;
                if constexpr (W == 1) s = kdf_find_narrow(tb, h[r]);
                else if constexpr (W == 2) s = kdf_find_wide(tb, h[r], top[r]);
                else {
                    const uint64_t i = first + (uint64_t)r * 64 + lane;
                    uint64_t w[W];
                    w[0] = 0;                                      // (kdf_find_long compares h, not w0)
#pragma unroll
                    for (int j = 1; j < W - 1; ++j) w[j] = *kdf_long_word<W>(ta, j, i);
                    w[W - 1] = top[r];
                    s = kdf_find_long<W>(tb, h[r], w);
                }
                if (s != ~0ull) oc[r] = tb.cnt[s];
            }
            if (oc[r] < a.other_min || oc[r] > a.other_max) cand &= ~(1u << r);
        }
    } else {
#pragma unroll
        for (int r = 0; r < KJ_ROWS; ++r) oc[r] = 0;
    }
#pragma unroll
    for (int r = 0; r < KJ_ROWS; ++r) { kb[r] = __ballot((cand >> r) & 1); tot += (uint32_t)__popcll(kb[r]); }
    if constexpr (!WRITE) {
        if (lane == 0 && tot) atomicAdd(&ctl->tally[(uint32_t)(wave % KDF_SHARDS) * 16], (unsigned long long)tot);
        return;
    }
    if (lane == 0) wtot[wv] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int i = 0; i < KJ_THREADS / 64; ++i) { const uint32_t v = wtot[i]; wtot[i] = acc; acc += v; }
        wg_base = acc ? atomicAdd(&ctl->cursor, (unsigned long long)acc) : 0ull;
    }
    __syncthreads();
    unsigned long long base = wg_base + wtot[wv];
#pragma unroll
    for (int r = 0; r < KJ_ROWS; ++r) {
        if ((kb[r] >> lane) & 1) {
            const uint64_t pos = base + __popcll(kb[r] & ((1ull << lane) - 1));
            if (pos < out_cap) {
                if constexpr (W <= 2) {
                    out_keys[pos] = kdf_key_lo(h[r], W == 2 ? top[r] : 0);            // the key back from its stored form
                    if (W == 2 && out_hi) out_hi[pos] = top[r];
                } else {
                    const uint64_t i = first + (uint64_t)r * 64 + lane;
                    uint64_t w[W];
                    w[0] = 0;
#pragma unroll
                    for (int j = 1; j < W - 1; ++j) w[j] = *kdf_long_word<W>(ta, j, i);
                    w[W - 1] = top[r];
                    w[0] = kdf_unmix64(h[r]) ^ kdf_long_fold<W>(w);
#pragma unroll
                    for (int j = 0; j < W; ++j) out_keys[pos * W + j] = w[j];
                }
                if (ocnt) ocnt[pos] = c[r];
                if (oocnt) oocnt[pos] = oc[r];
            }
        }
        base += __popcll(kb[r]);
    }
}

// k <= 63: KW = 1 narrow, 2 wide
template <int KW, bool WRITE>
__global__ __launch_bounds__(KJ_THREADS) void kdf_join_kernel(KdfTable ta, KdfTable tb, KdfJoinArgs a, KdfCtl *ctl, uint64_t *__restrict__ olo,
                                                             uint64_t *__restrict__ ohi, uint32_t *__restrict__ ocnt,
                                                             uint32_t *__restrict__ oocnt, uint64_t out_cap)
{
    kdf_join_body<KW, WRITE>(ta, tb, a, ctl, olo, ohi, ocnt, oocnt, out_cap);
}

// long keys: W = 3 .. 7, rows of W words
template <int W, bool WRITE>
__global__ __launch_bounds__(KJ_THREADS) void kdf_long_join_kernel(KdfTable ta, KdfTable tb, KdfJoinArgs a, KdfCtl *ctl, uint64_t *__restrict__ okeys,
                                                                  uint32_t *__restrict__ ocnt, uint32_t *__restrict__ oocnt, uint64_t out_cap)
{
    kdf_join_body<W, WRITE>(ta, tb, a, ctl, okeys, nullptr, ocnt, oocnt, out_cap);
}
