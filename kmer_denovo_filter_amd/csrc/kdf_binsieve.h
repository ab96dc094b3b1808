// kdf_binsieve.h -- count --if for large filters: a membership sieve laid out BIN-MAJOR behind kernel A (option "sieve_bins").
//
// The sieve of kdf_engine.hip answers a window with one random 8-byte read, so it must sit in the L2 of every XCD: up to
// 16 MB, ~16 M keys.  Here the stream is first slab-sorted by the top c1 hash bits (kb_slabsort_kernel, unchanged), and the
// sieve is cut into 2^c1 slices by the same bits:
//     word = kb_coarse(plan, h) * slice_words + ((h >> 12) & (slice_words - 1)),   bits = kdf_sieve_bits(h)
// (the bin bits are the top of h, the word bits start at bit 12, the two bit numbers are bits 0 .. 11: independent for every
// legal geometry).  A slice of up to 128 KB fits the LDS of one CU, so a workgroup that owns ONE bin copies its slice into
// LDS, streams that bin's runs out of A's output and tests every entry there; only the survivors probe the table.  Nothing
// is sorted a second time and the table is not rewritten.
//
// The part above `#if defined(__HIP__)` is plain C++: kdf_host.cpp compiles the sizing rule for kdf_bin_sieve_geometry.
#pragma once
#include <stdint.h>

#define KDF_BS_THREADS 512               // workgroup of the bin kernel: 8 waves
#define KDF_BS_WQ 128                    // survivor queue entries per wave (drained 64 at a time)
#define KDF_BS_C1_MIN 4
#define KDF_BS_C1_MAX 10                 // = KB_C1_MAX (kdf_binned.h)
#define KDF_BS_MIN_SLICE_WORDS 128u
#define KDF_BS_LDS_BYTES (160u * 1024u)  // one CU's LDS; a single workgroup may take all of it
// LDS of the bin kernel beside the slice: the waves' survivor queues (8 B x KW per entry), the run table of one round
// (KDF_BS_THREADS runs: source 8 B, first position 4 B, + 4 words of padding) and the block scan's 32 words
#define KDF_BS_LDS_OTHER(KW) ((KDF_BS_THREADS / 64u) * KDF_BS_WQ * 8u * (KW) + KDF_BS_THREADS * 8u + (KDF_BS_THREADS + 4u) * 4u + 32u * 4u)
// wide keys: 8 x 128 x 16 = 16 384 B of queues + 4 096 + 2 064 + 128 = 22 672 B; 163 840 - 22 672 = 141 168 B = 17 646 words
// -> the largest power of two is 2^14 words = 128 KB (narrow keys: 14 480 B beside it, the same cap).  With 1024 threads the
// wide queues alone are 32 KB: 2^14 words would not fit.
static inline uint32_t kdf_bs_cap_words() {
    uint32_t w = KDF_BS_MIN_SLICE_WORDS;
    while ((uint64_t)(2 * w) * 8 + KDF_BS_LDS_OTHER(2) <= KDF_BS_LDS_BYTES) w *= 2;
    return w;
}

// The sizing rule (the ONE place it lives: kdf_bin_sieve_geometry and the engine call it).  0: a geometry, 1: no bin-major
// sieve for this filter.  The sieve has pow2ceil(n_keys x bits / 64) words, cut into 2^c1 slices of at least 128 words; a
// slice must fit kdf_bs_cap_words().  Bits per key: sieve_bits as given, or (0) 8, and 4 when 8 does not fit even at
// c1 = 10; below 4 the two bits per key saturate the words: refused.  sieve_bins 1: the smallest c1 in 4 .. 10 that fits;
// 4 .. 10: that c1 or nothing.
static inline int kdf_bs_geometry(uint64_t n_keys, int key_words, int sieve_bits, int sieve_bins, uint32_t *c1, uint32_t *slice_words,
                                  uint32_t *bits_per_key) {
    if (key_words != 1 && key_words != 2) return 1;
    if (sieve_bits < 0 || sieve_bits > 64) return 1;
    if (sieve_bins != 1 && (sieve_bins < KDF_BS_C1_MIN || sieve_bins > KDF_BS_C1_MAX)) return 1;
    if (n_keys > (1ull << 40)) return 1;
    const uint32_t cap = kdf_bs_cap_words();
    auto slice = [&](uint32_t bpk, uint32_t c) -> uint64_t {
        const uint64_t need = (n_keys * bpk + 63) / 64;
        uint64_t words = 1;
        while (words < need) words <<= 1;
        const uint64_t s = words >> c;
        return s < KDF_BS_MIN_SLICE_WORDS ? KDF_BS_MIN_SLICE_WORDS : s;
    };
    uint32_t bpk = (uint32_t)sieve_bits;
    if (!bpk) bpk = slice(8, KDF_BS_C1_MAX) <= cap ? 8 : 4;
    uint32_t c = sieve_bins == 1 ? KDF_BS_C1_MIN : (uint32_t)sieve_bins;
    if (sieve_bins == 1) while (c < KDF_BS_C1_MAX && slice(bpk, c) > cap) ++c;
    if (slice(bpk, c) > cap) return 1;
    if (c1) *c1 = c;
    if (slice_words) *slice_words = (uint32_t)slice(bpk, c);
    if (bits_per_key) *bits_per_key = bpk;
    return 0;
}

#if defined(__HIP__)                        // the kernels: kdf_engine.hip, behind kdf_binned.h and kdf_sieve_bits

#define KDF_BS_EPT(KW) (16 / (KW))         // entries per thread and step of the bin kernel: 128 bytes in flight per lane

// the bin-major sieve over the keys the table holds now (a slot's lo is h), as kdf_sieve_from_table_kernel builds the other one
template <int KW>
__global__ __launch_bounds__(256) void kdf_bs_from_table_kernel(KdfTable t, KbPlan plan, uint64_t *__restrict__ words, uint32_t slice_words) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1ull << t.log2cap)) return;
    const uint64_t lo = t.lo[i], hi = KW == 2 ? t.hi[i] : 0;
    if ((KW == 1 ? lo : hi) == KDF_EMPTY) return;
    uint64_t w, b;
    kdf_sieve_bits(lo, slice_words - 1, w, b);
    atomicOr((unsigned long long *)&words[(uint64_t)kb_coarse(plan, lo) * slice_words + w], (unsigned long long)b);
}

// Kernel A's offset rows are [slab][nb + 1] u16: for one bin a 2 (nb + 1)-byte-strided gather.  This turns them, 64 slabs x 64
// bins per workgroup through LDS, into runs[bin][slab] = start | length << 16 (both <= 16 384), which the bin kernel reads
// coalesced.
__global__ __launch_bounds__(256) void kdf_bs_transpose_kernel(const uint16_t *__restrict__ off, uint32_t *__restrict__ runs, uint32_t n_slabs, uint32_t nb) {
    __shared__ uint32_t tile[64][65];
    const uint32_t slab0 = blockIdx.x * 64u, bin0 = blockIdx.y * 64u;
    const uint32_t ncol = min(64u, nb - bin0) + 1u;                 // offsets of this tile's bins and the one that ends the last
    for (uint32_t i = threadIdx.x; i < 64u * 65u; i += 256u) {
        const uint32_t r = i / 65u, c = i - r * 65u;
        if (slab0 + r < n_slabs && c < ncol) tile[r][c] = off[(uint64_t)(slab0 + r) * (nb + 1u) + bin0 + c];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 64u * 64u; i += 256u) {
        const uint32_t b = i >> 6, r = i & 63u;
        if (slab0 + r < n_slabs && b + 1u < ncol) {
            const uint32_t st = tile[r][b];
            runs[(uint64_t)(bin0 + b) * n_slabs + slab0 + r] = st | ((tile[r][b + 1] - st) << 16);
        }
    }
}

// One workgroup per (bin, share of the slabs); the grid has 2^c1 x shares workgroups.  The bin's slice lies in LDS; the share's
// slabs are taken KDF_BS_THREADS at a time: a block scan of their run lengths gives the round's run table, then the round's
// entries are indexed FLAT -- entry e of the round belongs to the run r with rpre[r] <= e < rpre[r + 1] and lies at
// tmp[rsrc[r] + e] -- so every lane has an entry whatever the run lengths (16 at c1 = 10, a whole slab when one bin takes
// everything).  A lane finds the run of its first entry by bisection and walks on from there (its entries are 64 apart).
// Survivors of the two-bit test go through a wave-private queue and probe the table 64 at a time, as in kdf_sieve_count_kernel.
template <int KW>
__global__ __launch_bounds__(KDF_BS_THREADS) void kdf_bin_sieve_kernel(
    const uint64_t *__restrict__ tmp, const uint32_t *__restrict__ runs, const uint64_t *__restrict__ sieve, uint32_t slice_words,
    uint32_t n_slabs, uint32_t shares, uint32_t slabs_per_share, KdfTable t, KdfCtl *ctl)
{
    constexpr uint32_t NT = KDF_BS_THREADS, EPT = KDF_BS_EPT(KW), SLAB = KbCfg<KW>::SLAB, QN = (NT / 64) * KDF_BS_WQ;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t *lsv = (uint64_t *)smem;                                   // [slice_words]
    uint64_t *qlo = lsv + slice_words;                                  // [QN]
    uint64_t *qhi = qlo + QN;                                           // [QN] (wide keys)
    unsigned long long *rsrc = (unsigned long long *)(qhi + (KW == 2 ? QN : 0));   // [NT] entry index in tmp of the run's first entry MINUS its position in the round
    uint32_t *rpre = (uint32_t *)(rsrc + NT);                           // [NT + 4] position of the run's first entry in the round; padded with the total
    uint32_t *wsum = rpre + NT + 4;                                     // [32]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // Workgroups are dealt to the 8 XCDs round robin by blockIdx and each XCD has its own L2: an XCD takes a contiguous eighth
    // of the bins, one share after the other, so the workgroups that run side by side on it hold NEIGHBOURING bins of the same
    // slabs -- a 16-entry run starts inside the cache line in which its neighbour's ends, and the second fetch of that line
    // then hits in the L2.  (Placement changes speed only.)
    const uint32_t nb8 = (gridDim.x / shares) >> 3, xcd = blockIdx.x & 7u, j = blockIdx.x >> 3;
    const uint32_t share = j / nb8, bin = xcd * nb8 + (j - share * nb8);
    {
        const ulonglong2 *src = (const ulonglong2 *)(sieve + (uint64_t)bin * slice_words);      // (slices are multiples of 1 KB)
        for (uint32_t i = tid; i < slice_words / 2; i += NT) ((ulonglong2 *)lsv)[i] = src[i];
        // (the first block scan's barriers come before the slice is read)
    }
    uint64_t *wqlo = qlo + wave * KDF_BS_WQ, *wqhi = qhi + (KW == 2 ? wave * KDF_BS_WQ : 0);
    uint32_t wq_n = 0, nwin = 0, claimed = 0;
    bool full = false;
    // probe the table for 64 queued keys (or the rest): every lane has a key
    auto drain = [&](uint32_t from, uint32_t cnt) {
        const bool todo = lane < cnt;
        const uint64_t klo = todo ? wqlo[from + lane] : 0, khi = (KW == 2 && todo) ? wqhi[from + lane] : 0;
        const uint64_t slot = kdf_home(t, klo);                       // the entries are stored forms
        if constexpr (KW == 1) { if (todo && !kdf_add_narrow<false>(t, klo, 1u, slot, t.lo[slot], claimed)) full = true; }
        else { if (!kdf_add_wide<false>(t, todo, klo, khi, 1u, slot, claimed)) full = true; }
    };
    const uint32_t s_begin = share * slabs_per_share, s_end = min(n_slabs, s_begin + slabs_per_share);
    const uint32_t *brow = runs + (uint64_t)bin * n_slabs;
    const uint32_t wmask = slice_words - 1;
    for (uint32_t s0 = s_begin; s0 < s_end; s0 += NT) {               // (uniform)
        uint32_t st = 0, len = 0;
        if (s0 + tid < s_end) { const uint32_t r = brow[s0 + tid]; st = r & 0xFFFFu; len = r >> 16; }
        uint32_t total;
        const uint32_t pre = kb_block_exscan(len, wsum, &total);      // (two barriers: every wave has left the last round's table)
        rsrc[tid] = (unsigned long long)(s0 + tid) * SLAB + st - pre;
        rpre[tid] = pre;                                              // (threads past the share's end: length 0, pre = total)
        if (tid < 4) rpre[NT + tid] = total;
        __syncthreads();
        if (tid == 0) nwin += total;
        // (Measured and dropped: two register sets, ping-pong, so that a step's loads are issued before the step before it is
        // tested -- 123 / 112 VGPRs, no spill, bin kernel 5.63 / 4.99 / 10.51 ms against 5.73 / 5.12 / 9.86 ms at c1 = 4 / 8 / 10,
        // k = 31, separate runs: the loads' latency is not what the kernel waits for.)
        for (uint32_t base = 0; base < total; base += NT * EPT) {     // (uniform)
            const uint32_t wbase = base + wave * (64 * EPT) + lane;  // this lane's first entry of the step
            uint32_t cr = 0, cnx = 0;                                 // current run and the position where the next one starts
            unsigned long long cs = 0;
            if (wbase < total) {
                // the last run that starts at or before wbase (rpre[0] = 0); runs behind it that start there too are empty
#pragma unroll
                for (uint32_t step = NT / 2; step > 0; step >>= 1) if (rpre[cr + step] <= wbase) cr += step;
                cnx = rpre[cr + 1]; cs = rsrc[cr];
            }
            uint64_t klo[EPT], khi[KW == 2 ? EPT : 1];
#pragma unroll
            for (uint32_t q = 0; q < EPT; ++q) {
                const uint32_t e = wbase + 64 * q;
                klo[q] = 0; if constexpr (KW == 2) khi[q] = 0;
                if (e < total) {
                    if (e >= cnx) {
                        do { ++cr; cnx = rpre[cr + 1]; } while (e >= cnx);      // (rpre[NT] = total > e: stops at the last run)
                        cs = rsrc[cr];
                    }
                    if constexpr (KW == 2) { const KbEnt2 v = ((const KbEnt2 *)tmp)[cs + e]; klo[q] = v.lo; khi[q] = v.hi; }
                    else klo[q] = tmp[cs + e];
                }
            }
#pragma unroll
            for (uint32_t q = 0; q < EPT; ++q) {
                const uint64_t h = klo[q];
                const uint64_t w = lsv[(uint32_t)(h >> 12) & wmask];
                const bool ok = (wbase + 64 * q < total) && (((w >> (h & 63)) & (w >> ((h >> 6) & 63)) & 1ull) != 0);
                const unsigned long long mk = __ballot(ok);
                if (mk) {
                    const uint32_t at = wq_n + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
                    if (ok) { wqlo[at] = h; if constexpr (KW == 2) wqhi[at] = khi[q]; }
                    wq_n += (uint32_t)__popcll(mk);
                    if (wq_n >= 64) { wq_n -= 64; drain(wq_n, 64); }        // (wave-uniform)
                }
            }
        }
    }
    if (wq_n) drain(0, wq_n);
    if (full) atomicOr(&ctl->error, 1u);
    kdf_shard_add(ctl->windows, nwin);                                // the entries are the stream's valid windows
}

#endif  // __HIP__
