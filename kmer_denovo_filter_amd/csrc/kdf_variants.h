// kdf_variants.h -- VCF mode on the device (kdf_variant_windows*, kdf_variant_evidence*): which windows of which reads
// span which variant, whether the read spells the ALT, and what the parents' table says about those windows.  The
// kernels only READ the stream, the alignment arrays, the variant arrays and (evidence) the table.
//
// Windows.  The unit of work is a CANDIDATE: a read and a variant whose position lies inside the read's reference
// interval.  Variants are sorted, so the candidates of a read are a range of the variant list.
//   1. kv_range_kernel    thread per read that is not skipped: one walk over its CIGAR for the reference bases it
//                         consumes, two binary searches of var_pos for the range; a read that has candidates walks its
//                         CIGAR once more and writes the per-operation prefix sums kc_prefix_kernel writes.
//   2. kv_offsets_kernel  exclusive scan of the range lengths (block sums through kh_scan_kernel): candidate c belongs
//                         to the read r with cand_off[r] <= c < cand_off[r + 1].
//   3. kv_count_kernel    lane per candidate: the anchor by binary search in the reference prefix sums, ONE pass over the
//                         at most k + span positions the candidate windows cover with the last bad position carried
//                         along (a window is an entry iff no bad position lies in it), then supports_alt for pairs.
//                         Writes the entry count and the flags of the candidate and the block sums of pairs and entries.
//   4. kv_write_kernel    lane per candidate, after kh_scan_kernel over both block sums: the same pass again, now
//                         writing.  Candidates are in (read, variant) order and a candidate's entries ascend, so the
//                         lists are ordered whatever the scheduling.
// Work: candidates x (k + span) plus the CIGAR operations of the reads that are not skipped; never a walk per window.
// Bounds, whatever the offsets hold: a read comes from kh_read_of over the scan (-1 or in [0, n_reads)), a variant from
// the range (inside [0, n_var)), operation, quality and ALT indices are clamped to their arrays, a stream position is
// touched only inside [max(offsets[r], 0), min(offsets[r + 1], n_bases)), and a write is issued only below its cap.
//
// Evidence.  kv_evidence_kernel, lane per entry: the table slot of the entry's key (kh_find), its count, and
//   - the pair's `windows` / `absent`: lanes of a wave in the same pair are neighbours (entries are grouped by pair) and
//     are summed on ballots, one atomic add per run, as kh_distinct_kernel does per read;
//   - the variant's distinct stored keys: (variant, tag, slot) goes into the open-addressing set kh_distinct_kernel uses;
//     the lane whose word was new adds the count to the variant's row (add, add, max of ~count, max).  Integer sums,
//     minima and maxima: the result does not depend on which lane wins a CAS.
#pragma once
#include "kdf_coverage.h"
#include "kdf_text.h"

#define KV_VAR_WORDS  8                   // n, sum, min, max, n_alt, sum_alt, min_alt, max_alt (uint64)
#define KV_PAIR_WORDS 2                   // windows, absent (uint32)

// exclusive prefix of v over the 256 threads of the workgroup and their total, 64-bit; ws: 4 words of LDS
__device__ __forceinline__ unsigned long long kv_block_excl(unsigned long long v, unsigned long long *ws, unsigned long long &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned long long y = __shfl_up(inc, o); if (lane >= o) inc += y; }
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    unsigned long long pre = 0;
    total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const unsigned long long s = ws[j]; pre += j < wv ? s : 0; total += s; }
    __syncthreads();
    return pre + inc - v;
}

// first i in [0, n) with a[i] >= x, n when there is none
__device__ __forceinline__ uint64_t kv_lower_bound(const int64_t *__restrict__ a, uint64_t n, int64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

__device__ __forceinline__ bool kv_takes_query(uint32_t op) { return kc_aligned(op) || op == 1 || op == 4; }
__device__ __forceinline__ bool kv_takes_ref(uint32_t op) { return kc_aligned(op) || op == 2 || op == 3; }

// cand_lo[r], cand_cnt[r]: the variants [lo, lo + cnt) lie in the reference interval of read r; block_sums[block] = sum
// of cnt over the block's reads; pre: the prefix sums of kc_prefix_kernel for the reads with cnt > 0
__global__ __launch_bounds__(256) void kv_range_kernel(
    int64_t n_reads, const int64_t *__restrict__ ref_start, const uint32_t *__restrict__ cigar, uint64_t n_cigar,
    const int64_t *__restrict__ cig_offs, const int64_t *__restrict__ var_pos, uint64_t n_var,
    unsigned long long *__restrict__ pre, uint64_t *__restrict__ cand_lo, unsigned long long *__restrict__ cand_cnt,
    unsigned long long *__restrict__ block_sums)
{
    __shared__ unsigned long long ws[4];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long cnt = 0, total;
    uint64_t lo = 0;
    if (r < n_reads) {
        const int64_t rs = ref_start[r];
        if (rs >= 0) {
            const int64_t cb = kc_clamp(cig_offs[r], 0, (int64_t)n_cigar), ce = kc_clamp(cig_offs[r + 1], cb, (int64_t)n_cigar);
            unsigned long long rc = 0;
            for (int64_t i = cb; i < ce; ++i) { const uint32_t w = cigar[i]; if (kv_takes_ref(w & 15u)) rc += w >> 4; }
            if (rc) {
                const unsigned long long room = 0x7FFFFFFFFFFFFFFFull - (unsigned long long)rs;
                const int64_t end = rs + (int64_t)(rc < room ? rc : room);
                lo = kv_lower_bound(var_pos, n_var, rs);
                const uint64_t hi = kv_lower_bound(var_pos, n_var, end);
                if (hi > lo) cnt = hi - lo;
            }
            if (cnt) {
                unsigned long long qc = 0;
                rc = 0;
                for (int64_t i = cb; i < ce; ++i) {
                    pre[2 * i] = qc;
                    pre[2 * i + 1] = rc;
                    const uint32_t w = cigar[i], op = w & 15u;
                    if (kv_takes_query(op)) qc += w >> 4;
                    if (kv_takes_ref(op)) rc += w >> 4;
                }
            }
        }
        cand_lo[r] = lo;
        cand_cnt[r] = cnt;
    }
    kv_block_excl(cnt, ws, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// cand[r] (the counts) -> the exclusive prefix sums, cand[n_reads] = the total; block_off: the scanned block sums
__global__ __launch_bounds__(256) void kv_offsets_kernel(int64_t n_reads, const unsigned long long *__restrict__ block_off,
                                                         unsigned long long *__restrict__ cand) {
    __shared__ unsigned long long ws[4];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long cnt = r < n_reads ? cand[r] : 0;
    unsigned long long total;
    const unsigned long long off = block_off[blockIdx.x] + kv_block_excl(cnt, ws, total);
    if (r < n_reads) cand[r] = off;
    if (r == n_reads - 1) cand[n_reads] = off + cnt;
}

struct KvArgs {
    const uint64_t *packed, *invalid; uint64_t n_bases; int k;
    const int64_t *offs; int64_t n_reads;
    const int64_t *ref_start; const uint32_t *cigar; uint64_t n_cigar; const int64_t *cig_offs;
    const uint8_t *qual; uint64_t n_qual; const int64_t *qual_offs; uint32_t min_baseq;    // qual == NULL: no quality rule
    const int64_t *var_pos; const uint32_t *var_span, *var_ref_len; uint64_t n_var;
    const uint8_t *alt; uint64_t n_alt; const int64_t *alt_offs;
    const unsigned long long *pre;              // prefix sums of the reads that have candidates
    const uint64_t *cand_lo; const unsigned long long *cand_off; uint64_t n_cand;
};

// What candidate c comes to.  Returns false when it has no read or variant to speak of.  Otherwise r, v and n_ent (the
// number of entries) are set; WRITE: the entries go to entry_pos / entry_pair [eo ..) below entry_cap, with pair index pi;
// !WRITE: flags is set for a pair (n_ent > 0).
template <bool WRITE>
__device__ __forceinline__ bool kv_candidate(const KvArgs &a, uint64_t c, int64_t &r, uint64_t &v, uint32_t &n_ent, uint8_t &flags,
                                             uint64_t *__restrict__ entry_pos, uint64_t *__restrict__ entry_pair, uint64_t eo,
                                             uint64_t entry_cap, uint64_t pi) {
    n_ent = 0; flags = 0;
    r = kh_read_of((const int64_t *)a.cand_off, a.n_reads, (int64_t)c);
    if (r < 0) return false;
    v = a.cand_lo[r] + (c - a.cand_off[r]);
    if (v >= a.n_var) return false;
    const int64_t span = a.var_span[v];
    const int64_t rs = a.ref_start[r];
    if (span == 0 || rs < 0) return true;
    const int64_t d = a.var_pos[v] - rs;
    if (d < 0) return true;
    const int64_t cb = kc_clamp(a.cig_offs[r], 0, (int64_t)a.n_cigar), ce = kc_clamp(a.cig_offs[r + 1], cb, (int64_t)a.n_cigar);
    if (ce == cb) return true;
    // the last operation whose reference prefix is <= d: the only one that can hold reference offset d
    auto op_of = [&](int64_t x) {
        int64_t lo = cb, hi = ce - 1;
        while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if ((int64_t)a.pre[2 * mid + 1] <= x) lo = mid; else hi = mid - 1; }
        return lo;
    };
    const int64_t j = op_of(d);
    const uint32_t w = a.cigar[j];
    const int64_t in = d - (int64_t)a.pre[2 * j + 1];
    if (!kc_aligned(w & 15u) || in < 0 || in >= (int64_t)(w >> 4)) return true;        // a D or N, or past the CIGAR: no anchor
    const int64_t at = (int64_t)a.pre[2 * j] + in;
    const int64_t b = a.offs[r], e = a.offs[r + 1];
    if (b < 0 || e <= b) return true;
    const int64_t lim = e < (int64_t)a.n_bases ? e : (int64_t)a.n_bases;               // end of the read's stream range
    const int64_t k = a.k;
    const int64_t s_first = at - k + 1 > 0 ? at - k + 1 : 0;
    int64_t s_last = at + span - 1;
    if (s_last > lim - b - k) s_last = lim - b - k;
    if (s_last < s_first) return true;
    // quality bytes of the read: query index x has one iff x < qn
    int64_t qo = 0, qn = 0;
    if (a.qual && a.min_baseq) {
        qo = kc_clamp(a.qual_offs[r], 0, (int64_t)a.n_qual);
        qn = kc_clamp(a.qual_offs[r + 1], qo, (int64_t)a.n_qual) - qo;
    }
    auto bad = [&](int64_t x) {                                      // query index x, b + x < lim
        const uint64_t q = (uint64_t)(b + x);
        if ((a.invalid[q >> 6] >> (q & 63)) & 1) return true;
        return x < qn && a.qual[qo + x] < a.min_baseq;
    };
    int64_t lastbad = s_first - 1;
    for (int64_t x = s_first; x < s_last + k; ++x) {
        if (bad(x)) lastbad = x;
        const int64_t s = x - k + 1;
        if (s >= s_first && lastbad < s) {
            if constexpr (WRITE) {
                const uint64_t o = eo + n_ent;
                if (o < entry_cap) { entry_pos[o] = (uint64_t)(b + s); entry_pair[o] = pi; }
            }
            ++n_ent;
        }
    }
    if constexpr (!WRITE) {
        if (n_ent == 0) return true;
        // supports_alt: the query bases from the anchor up to the first reference base at or past var_pos + ref_len
        const int64_t ao = kc_clamp(a.alt_offs[v], 0, (int64_t)a.n_alt), alen = kc_clamp(a.alt_offs[v + 1], ao, (int64_t)a.n_alt) - ao;
        if (alen == 0) return true;
        const int64_t ed = d + (int64_t)a.var_ref_len[v];
        const uint32_t wl = a.cigar[ce - 1];
        const int64_t qtot = (int64_t)a.pre[2 * (ce - 1)] + (kv_takes_query(wl & 15u) ? (int64_t)(wl >> 4) : 0);
        const int64_t rtot = (int64_t)a.pre[2 * (ce - 1) + 1] + (kv_takes_ref(wl & 15u) ? (int64_t)(wl >> 4) : 0);
        int64_t qe = qtot;
        if (ed < rtot) {
            const int64_t j2 = op_of(ed);
            qe = (int64_t)a.pre[2 * j2] + (kc_aligned(a.cigar[j2] & 15u) ? ed - (int64_t)a.pre[2 * j2 + 1] : 0);
        }
        if (qe - at != alen || b + qe > lim) return true;
        for (int64_t i = 0; i < alen; ++i) {
            const uint64_t q = (uint64_t)(b + at + i);
            if (bad(at + i) || ((a.packed[q >> 5] >> (2 * (q & 31))) & 3) != kdf_base_code(a.alt[ao + i])) return true;
        }
        flags = 1;
    }
    return true;
}

// ent_cnt[c], flags[c] of every candidate; sums_p / sums_e [block]: pairs / entries of the block's candidates
__global__ __launch_bounds__(256) void kv_count_kernel(KvArgs a, uint32_t *__restrict__ ent_cnt, uint8_t *__restrict__ cflags,
                                                       unsigned long long *__restrict__ sums_p, unsigned long long *__restrict__ sums_e) {
    __shared__ unsigned long long ws[4];
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t n_ent = 0;
    if (c < a.n_cand) {
        int64_t r; uint64_t v; uint8_t fl;
        kv_candidate<false>(a, c, r, v, n_ent, fl, nullptr, nullptr, 0, 0, 0);
        ent_cnt[c] = n_ent;
        cflags[c] = fl;
    }
    unsigned long long tp, te;
    kv_block_excl(n_ent != 0, ws, tp);
    kv_block_excl(n_ent, ws, te);
    if (threadIdx.x == 0) { sums_p[blockIdx.x] = tp; sums_e[blockIdx.x] = te; }
}

// the pair and the entries of every candidate that has entries, at the places the two scans give
__global__ __launch_bounds__(256) void kv_write_kernel(
    KvArgs a, const uint32_t *__restrict__ ent_cnt, const uint8_t *__restrict__ cflags, const unsigned long long *__restrict__ off_p,
    const unsigned long long *__restrict__ off_e, int64_t *__restrict__ pair_read, uint32_t *__restrict__ pair_var,
    uint8_t *__restrict__ pair_flags, uint64_t pair_cap, uint64_t *__restrict__ entry_pos, uint64_t *__restrict__ entry_pair, uint64_t entry_cap)
{
    __shared__ unsigned long long ws[4];
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t n = c < a.n_cand ? ent_cnt[c] : 0;
    unsigned long long tp, te;
    const uint64_t pi = off_p[blockIdx.x] + kv_block_excl(n != 0, ws, tp);
    const uint64_t eo = off_e[blockIdx.x] + kv_block_excl(n, ws, te);
    if (n == 0) return;
    int64_t r; uint64_t v; uint32_t n_ent; uint8_t fl;
    if (!kv_candidate<true>(a, c, r, v, n_ent, fl, entry_pos, entry_pair, eo, entry_cap, pi)) return;
    if (pi < pair_cap) { pair_read[pi] = r; pair_var[pi] = (uint32_t)v; pair_flags[pi] = cflags[c]; }
}

// ---- evidence ---------------------------------------------------------------------------------------------------------------

// pair_rows[pair] += (windows, absent); var_rows[variant] gathers its distinct stored keys (column min as max of ~count:
// kv_rows_fix_kernel).  set: 2^log2set words of KDF_EMPTY, 2^log2set >= 4 n_entries.  The host checked that
// (variant * 2 + tag) << log2cap | slot stays below 2^63 (so no word is KDF_EMPTY).
template <int W>
__global__ __launch_bounds__(256) void kv_evidence_kernel(
    KdfTable t, const uint64_t *__restrict__ keys, const uint64_t *__restrict__ entry_pair, uint64_t n_entries,
    const uint32_t *__restrict__ pair_var, const uint8_t *__restrict__ pair_flags, uint64_t n_pairs, uint64_t n_var,
    unsigned long long *__restrict__ set, uint32_t log2set, uint32_t *__restrict__ pair_rows, unsigned long long *__restrict__ var_rows)
{
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    long long pr = -1;
    bool absent = false;
    if (i < n_entries) {
        const uint64_t ep = entry_pair[i];
        const uint64_t v = ep < n_pairs ? pair_var[ep] : ~0ull;
        if (v < n_var) {
            pr = (long long)ep;
            uint64_t key[W];
            bool ones = true;
#pragma unroll
            for (int j = 0; j < W; ++j) { key[j] = keys[i * W + j]; ones = ones && key[j] == ~0ull; }
            uint64_t slot = ~0ull;
            if (!ones) slot = kh_find<W>(t, kd_hash<W>(key), key);    // (a row of all ones is a window past the stream: no key)
            const uint32_t cnt = slot == ~0ull ? 0u : t.cnt[slot];
            absent = cnt == 0;
            if (cnt) {
                const int tags = (pair_flags[ep] & 1) ? 2 : 1;
                const uint64_t smask = (1ull << log2set) - 1;
                for (int tag = 0; tag < tags; ++tag) {
                    const unsigned long long word = (((unsigned long long)v * 2 + tag) << t.log2cap) | slot;
                    uint64_t j = kdf_mix64(word) >> (64 - log2set);
                    bool isnew = false;
                    for (uint64_t n = 0; n <= smask; ++n) {          // (ends at an empty word: the set is at most half full)
                        const unsigned long long old = atomicCAS(&set[j], (unsigned long long)KDF_EMPTY, word);
                        if (old == KDF_EMPTY) { isnew = true; break; }
                        if (old == word) break;
                        j = (j + 1) & smask;
                    }
                    if (isnew) {
                        unsigned long long *row = var_rows + v * KV_VAR_WORDS + 4 * tag;
                        atomicAdd(row, 1ull);
                        atomicAdd(row + 1, (unsigned long long)cnt);
                        atomicMax(row + 2, ~(unsigned long long)cnt);
                        atomicMax(row + 3, (unsigned long long)cnt);
                    }
                }
            }
        }
    }
    // neighbours in the same pair: the first lane of each run adds the run's windows
    const long long prev = __shfl_up(pr, 1);
    const bool head = lane == 0 || prev != pr;
    const unsigned long long heads = __ballot(head), abs_ = __ballot(absent);
    if (head && pr >= 0) {
        const KdfWaveRun run = kdf_wave_run(heads, lane);
        const uint32_t na = (uint32_t)__popcll(abs_ & run.mask);
        atomicAdd(&pair_rows[(uint64_t)pr * KV_PAIR_WORDS], (uint32_t)run.len);
        if (na) atomicAdd(&pair_rows[(uint64_t)pr * KV_PAIR_WORDS + 1], na);
    }
}

// the two `min` columns were gathered as max(~count) over rows zeroed by the call: turn them back; 0 where n is 0
__global__ __launch_bounds__(256) void kv_rows_fix_kernel(unsigned long long *__restrict__ var_rows, uint64_t n_var) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_var) return;
    unsigned long long *row = var_rows + v * KV_VAR_WORDS;
    row[2] = row[0] ? ~row[2] : 0ull;
    row[6] = row[4] ? ~row[6] : 0ull;
}
