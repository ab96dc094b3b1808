// kdf_engine_reads.hip -- libkdf.so, the per-read consumers of a read stream: per-window counts and per-read depth
// (kdf_depth.h), per-read hits and the hit list of the scan (kdf_hits.h), hits in reference coordinates
// (kdf_coverage.h), VCF mode (kdf_variants.h) and the regions of informative reads (kdf_regions.h, which takes plain
// arrays).  They share kh_scan_kernel and the CIGAR prefix sums; the table is only read.  The engine itself is kdf_engine.hip, what this unit uses of it is declared in kdf_engine_priv.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <vector>

#include "kdf_engine_priv.h"
// per-window counts and per-read depth rows of a read stream
#include "kdf_depth.h"
#include "kdf_hits.h"
#include "kdf_coverage.h"
#include "kdf_variants.h"
#include "kdf_regions.h"
#include "kdf_sort.h"

// kh_scan_kernel for a caller in another unit (the spool's kdf_spool_select_reads): a kernel is compiled in one unit only
void kh_scan_launch(hipStream_t s, unsigned long long *sums, uint64_t n) { hipLaunchKernelGGL(kh_scan_kernel, dim3(1), dim3(256), 0, s, sums, n); }

// One launch of kdf_depth_kernel over the stream: the per-window form (rows == NULL) or the per-read form.  The table is
// only read; pending count work is applied first, as the scan does.
static int depth_pass(kdf_engine *h, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases, uint32_t *d_counts,
                      unsigned long long *d_valid, const int64_t *d_offs, int64_t n_reads, uint32_t low_max, unsigned long long *d_rows) {
    { int rcf = pending_flush(h); if (rcf) return rcf; }
    { int rc0 = materialize(h); if (rc0) return rc0; }
    const uint64_t n_tiles = (n_bases + KDF_TILE - 1) / KDF_TILE;
    const uint64_t waves = (n_tiles + KD_WAVE_TILES - 1) / KD_WAVE_TILES;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    EvSpan span(h->timer[T_DEPTH], h->prof, h->stream);
    if (d_rows) HIPCHK(h, hipMemsetAsync(d_rows, 0, (size_t)n_reads * KD_ROW_WORDS * 8, h->stream));
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        if (d_rows)
            hipLaunchKernelGGL((kdf_depth_kernel<W, true>), dim3(blocks), dim3(256), 0, h->stream, d_packed, d_invalid, n_bases, h->k, h->t,
                               (uint32_t *)nullptr, (unsigned long long *)nullptr, d_offs, n_reads, low_max, d_rows);
        else
            hipLaunchKernelGGL((kdf_depth_kernel<W, false>), dim3(blocks), dim3(256), 0, h->stream, d_packed, d_invalid, n_bases, h->k, h->t,
                               d_counts, d_valid, (const int64_t *)nullptr, (int64_t)0, 0u, (unsigned long long *)nullptr);
        return 0;
    });
    if (d_rows) hipLaunchKernelGGL(kd_rows_fix_kernel, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, h->stream, d_rows, n_reads);
    span.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

// Steps 1-2 of kdf_hits.h over the mask words of n_bases positions (n_bases >= 1): hits.block_sums then holds the exclusive
// prefix of every block of KH_BLOCK_WORDS words and, behind them, the number of set bits below n_bases.
static int hits_count(kdf_engine *h, const uint64_t *d_bits, uint64_t n_bases, uint64_t *n_blocks_out) {
    const uint64_t n_words = (n_bases + 63) / 64;
    const uint64_t n_blocks = (n_words + KH_BLOCK_WORDS - 1) / KH_BLOCK_WORDS;
    if (n_blocks >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "a hit mask of %llu positions is beyond the 2^47 a call takes", (unsigned long long)n_bases);
    int rc = eng_reserve(h, h->hits.block_sums, (n_blocks + 1) * 8, slack_8th, "block sums");
    if (rc) return rc;
    unsigned long long *sums = h->hits.block_sums.as<unsigned long long>();
    hipLaunchKernelGGL(kh_count_kernel, dim3((unsigned)n_blocks), dim3(256), 0, h->stream, d_bits, n_bases, sums);
    hipLaunchKernelGGL(kh_scan_kernel, dim3(1), dim3(256), 0, h->stream, sums, n_blocks);
    HIPCHK(h, hipGetLastError());
    *n_blocks_out = n_blocks;
    return KDF_OK;
}

// the total hits_count left, on the host (synchronises)
static int hits_total(kdf_engine *h, uint64_t n_blocks, uint64_t *n_hits) {
    HIPCHK(h, hipMemcpyAsync(h->h_out4, h->hits.block_sums.as<unsigned long long>() + n_blocks, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_hits = h->h_out4[0];
    return KDF_OK;
}

// d_kmer_cov / d_read_cov point at position `first`
static int coverage_list_core(kdf_engine *h, const char *fn, const uint32_t *d_kc, const uint32_t *d_rc, uint64_t first, uint64_t n,
                              uint32_t min_reads, void *d_pos_out, void *d_kmer_out, void *d_read_out, uint64_t cap, uint64_t *n_out) {
    const uint64_t n_blocks = (n + KC_BLOCK_ELEMS - 1) / KC_BLOCK_ELEMS;
    if (n_blocks >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "%s: a window of %llu positions is beyond the 2^41 a call takes", fn, (unsigned long long)n);
    int rc = eng_reserve(h, h->hits.block_sums, (n_blocks + 1) * 8, slack_8th, "block sums");
    if (rc) return rc;
    const uint32_t thr = std::max<uint32_t>(min_reads, 1);
    unsigned long long *sums = h->hits.block_sums.as<unsigned long long>();
    EvSpan p(h->timer[T_COV], h->prof, h->stream, 1);
    hipLaunchKernelGGL(kc_list_count_kernel, dim3((unsigned)n_blocks), dim3(256), 0, h->stream, d_rc, n, thr, sums);
    hipLaunchKernelGGL(kh_scan_kernel, dim3(1), dim3(256), 0, h->stream, sums, n_blocks);
    if (cap)
        hipLaunchKernelGGL(kc_list_write_kernel, dim3((unsigned)n_blocks), dim3(256), 0, h->stream, d_kc, d_rc, first, n, thr,
                           (const unsigned long long *)sums, (uint64_t *)d_pos_out, (uint32_t *)d_kmer_out, (uint32_t *)d_read_out, cap);
    p.stop();
    HIPCHK(h, hipGetLastError());
    uint64_t n_list = 0;
    if ((rc = hits_total(h, n_blocks, &n_list))) return rc;
    *n_out = n_list;
    if (n_list > cap)
        return fail(h, KDF_ERR_INVALID, "%s: the list holds %llu positions, the buffers %llu", fn, (unsigned long long)n_list, (unsigned long long)cap);
    return KDF_OK;
}

// offsets that start at 0, do not decrease and end at `total` (cigar_offsets, qual_offsets, alt_offsets)
static int check_offsets0(kdf_engine *h, const char *fn, const char *what, const int64_t *o, uint64_t n, uint64_t total) {
    if (!o) return fail(h, KDF_ERR_INVALID, "%s: %s is NULL", fn, what);
    if (o[0] != 0) return fail(h, KDF_ERR_INVALID, "%s: %s[0] = %lld, not 0", fn, what, (long long)o[0]);
    for (uint64_t i = 0; i < n; ++i)
        if (o[i + 1] < o[i])
            return fail(h, KDF_ERR_INVALID, "%s: %s decrease at %llu (%lld after %lld)", fn, what, (unsigned long long)i, (long long)o[i + 1], (long long)o[i]);
    if ((uint64_t)o[n] != total) return fail(h, KDF_ERR_INVALID, "%s: %s end at %lld, the array holds %llu", fn, what, (long long)o[n], (unsigned long long)total);
    return KDF_OK;
}

extern "C" {

// ------------------------------------------------ count profile of a read stream (kdf_depth.h) ----

int kdf_window_counts_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases, void *d_counts_out,
                          void *d_valid_bits_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n_bases == 0) return KDF_OK;
    if (!d_packed || !d_invalid || !d_counts_out) return fail(h, KDF_ERR_INVALID, "kdf_window_counts_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    return depth_pass(h, (const uint64_t *)d_packed, (const uint64_t *)d_invalid, n_bases, (uint32_t *)d_counts_out,
                      (unsigned long long *)d_valid_bits_out, nullptr, 0, 0, nullptr);
}

int kdf_window_counts(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases, uint32_t *counts_out,
                      uint64_t *valid_bits_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    uint64_t pw, mw;
    kdf_stream_words(n_bases, &pw, &mw);
    if (valid_bits_out) memset(valid_bits_out, 0, mw * 8);
    if (n_bases == 0) return KDF_OK;
    if (!packed || !invalid || !counts_out) return fail(h, KDF_ERR_INVALID, "kdf_window_counts: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t valid_bytes = valid_bits_out ? (n_bases + KDF_TILE - 1) / KDF_TILE * 8 : 0;
    HostCall c(h, "kdf_window_counts");
    const int is = c.stream(packed, invalid, n_bases), ic = c.out(counts_out, n_bases * 4), iv = c.out(valid_bits_out, valid_bytes);
    int rc;
    if ((rc = c.commit()) || (rc = kdf_window_counts_dev(h, c.dev(is), c.dev(is + 1), n_bases, c.dev(ic), c.dev(iv))) ||
        (rc = c.fetch(ic, n_bases * 4)) || (rc = c.fetch(iv, valid_bytes))) return rc;
    return c.finish();
}

int kdf_read_depth_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases, const void *d_read_offsets,
                       int64_t n_reads, uint32_t low_max, void *d_rows_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n_reads < 0) return fail(h, KDF_ERR_INVALID, "kdf_read_depth_dev: n_reads = %lld is negative", (long long)n_reads);
    if (n_reads == 0) return KDF_OK;
    if (!d_read_offsets || !d_rows_out) return fail(h, KDF_ERR_INVALID, "kdf_read_depth_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    if (n_bases == 0) {                                             // no window: every row is zero
        HIPCHK(h, hipMemsetAsync(d_rows_out, 0, (size_t)n_reads * KD_ROW_WORDS * 8, h->stream));
        return KDF_OK;
    }
    if (!d_packed || !d_invalid) return fail(h, KDF_ERR_INVALID, "kdf_read_depth_dev: NULL stream");
    return depth_pass(h, (const uint64_t *)d_packed, (const uint64_t *)d_invalid, n_bases, nullptr, nullptr,
                      (const int64_t *)d_read_offsets, n_reads, low_max, (unsigned long long *)d_rows_out);
}

int kdf_read_depth(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases, const int64_t *read_offsets,
                   int64_t n_reads, uint32_t low_max, uint64_t *rows_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n_reads > 0 && (!read_offsets || !rows_out)) return fail(h, KDF_ERR_INVALID, "kdf_read_depth: NULL pointer");
    if (const int rc = check_read_offsets(EngSink{h}, "kdf_read_depth", read_offsets, n_reads)) return rc;
    if (n_reads == 0) return KDF_OK;
    const size_t row_bytes = (size_t)n_reads * KD_ROW_WORDS * 8;
    if (n_bases == 0) { memset(rows_out, 0, row_bytes); return KDF_OK; }
    if (!packed || !invalid) return fail(h, KDF_ERR_INVALID, "kdf_read_depth: NULL stream");
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_read_depth");
    const int is = c.stream(packed, invalid, n_bases), io = c.in(read_offsets, (size_t)(n_reads + 1) * 8), ir = c.out(rows_out, row_bytes);
    int rc;
    if ((rc = c.commit()) || (rc = kdf_read_depth_dev(h, c.dev(is), c.dev(is + 1), n_bases, c.dev(io), n_reads, low_max, c.dev(ir))) ||
        (rc = c.fetch(ir, row_bytes))) return rc;
    return c.finish();
}

// ------------------------------------------------ per-read hits of the scan (kdf_hits.h) ----

int kdf_read_hits_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases, const void *d_read_offsets,
                      int64_t n_reads, void *d_hit_bits, void *d_rows_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n_reads < 0) return fail(h, KDF_ERR_INVALID, "kdf_read_hits_dev: n_reads = %lld is negative", (long long)n_reads);
    if (n_reads > 0 && (!d_read_offsets || !d_rows_out)) return fail(h, KDF_ERR_INVALID, "kdf_read_hits_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t row_bytes = (size_t)n_reads * KH_ROW_WORDS * 4;
    if (n_bases == 0) {                                             // no window: every row is zero, no hit word is written
        if (n_reads) HIPCHK(h, hipMemsetAsync(d_rows_out, 0, row_bytes, h->stream));
        return KDF_OK;
    }
    if (!d_packed || !d_invalid) return fail(h, KDF_ERR_INVALID, "kdf_read_hits_dev: NULL stream");
    int rc;
    uint64_t *bits = (uint64_t *)d_hit_bits;
    if (!bits) {
        if ((rc = eng_reserve(h, h->hits.mask, (n_bases + 63) / 64 * 8, slack_8th, "hit mask"))) return rc;
        bits = h->hits.mask.as<uint64_t>();
    }
    if ((rc = kdf_scan_reads_dev(h, d_packed, d_invalid, n_bases, bits))) return rc;     // (applies pending count work)
    if (n_reads == 0) return KDF_OK;
    // a (read, slot) pair must fit 63 bits: bit 63 keeps every pair apart from the set's empty word
    if (log2ceil((uint64_t)n_reads) + h->t.log2cap > 63)
        return fail(h, KDF_ERR_INVALID, "kdf_read_hits_dev: %lld reads against a table of 2^%u slots: read index and slot index must fit 63 bits "
                    "together (at most 2^%u reads per call for this table)", (long long)n_reads, h->t.log2cap, 63 - h->t.log2cap);
    uint64_t n_blocks = 0, n_hits = 0;
    EvSpan p1(h->timer[T_HITS], h->prof, h->stream, 1);           // (opens the call: counted as its pass)
    HIPCHK(h, hipMemsetAsync(d_rows_out, 0, row_bytes, h->stream));
    if ((rc = hits_count(h, bits, n_bases, &n_blocks))) return rc;
    p1.stop();
    if ((rc = hits_total(h, n_blocks, &n_hits))) return rc;
    if (n_hits == 0) return KDF_OK;
    uint32_t log2set = log2ceil(2 * n_hits);
    if ((rc = eng_reserve(h, h->hits.positions, n_hits * 8, slack_8th, "hit list"))) return rc;
    if ((rc = eng_reserve(h, h->hits.pair_set, (size_t)8 << log2set, slack_8th, "set of (read, k-mer) pairs"))) return rc;
    uint64_t *pos = h->hits.positions.as<uint64_t>();
    unsigned long long *set = h->hits.pair_set.as<unsigned long long>();
    const int64_t *offs = (const int64_t *)d_read_offsets;
    EvSpan p2(h->timer[T_HITS], h->prof, h->stream, 0);           // (the same call's second group: time only)
    HIPCHK(h, hipMemsetAsync(set, 0xFF, (size_t)8 << log2set, h->stream));
    hipLaunchKernelGGL(kh_write_kernel, dim3((unsigned)n_blocks), dim3(256), 0, h->stream, bits, n_bases, h->hits.block_sums.as<const unsigned long long>(),
                       pos, (int64_t *)nullptr, (const int64_t *)nullptr, (int64_t)0, n_hits);
    hipLaunchKernelGGL(kh_hits_kernel, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, h->stream, pos, n_hits, offs, n_reads,
                       (uint32_t *)d_rows_out);
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        hipLaunchKernelGGL(kh_distinct_kernel<W>, dim3((unsigned)((n_hits + 255) / 256)), dim3(256), 0, h->stream, (const uint64_t *)d_packed, n_bases,
                           h->k, h->t, pos, n_hits, offs, n_reads, set, log2set, (uint32_t *)d_rows_out);
        return 0;
    });
    p2.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

int kdf_read_hits(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases, const int64_t *read_offsets,
                  int64_t n_reads, uint64_t *hit_bits, uint32_t *rows_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    int rc = check_read_offsets(EngSink{h}, "kdf_read_hits", read_offsets, n_reads);       // (before any device work)
    if (rc) return rc;
    if (n_reads > 0 && !rows_out) return fail(h, KDF_ERR_INVALID, "kdf_read_hits: rows_out is NULL");
    uint64_t pw, mw;
    kdf_stream_words(n_bases, &pw, &mw);
    const size_t row_bytes = (size_t)n_reads * KH_ROW_WORDS * 4;
    if (hit_bits) memset(hit_bits, 0, mw * 8);
    if (n_bases == 0) { if (n_reads) memset(rows_out, 0, row_bytes); return KDF_OK; }
    if (!packed || !invalid) return fail(h, KDF_ERR_INVALID, "kdf_read_hits: NULL stream");
    if (n_reads == 0 && !hit_bits) return KDF_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_read_hits");
    const int is = c.stream(packed, invalid, n_bases), io = c.in(read_offsets, n_reads ? (size_t)(n_reads + 1) * 8 : 0), ir = c.out(rows_out, row_bytes);
    if ((rc = c.commit()) || (rc = kdf_read_hits_dev(h, c.dev(is), c.dev(is + 1), n_bases, c.dev(io), n_reads, nullptr, c.dev(ir))) ||
        (rc = c.fetch(ir, row_bytes))) return rc;
    // the mask is the _dev form's own buffer (it was given none), not staging
    if (hit_bits) HIPCHK(h, hipMemcpyAsync(hit_bits, h->hits.mask.p, (n_bases + 63) / 64 * 8, hipMemcpyDeviceToHost, h->stream));
    return c.finish();
}

int kdf_hit_list_dev(kdf_engine *h, const void *d_hit_bits, uint64_t n_bases, const void *d_read_offsets, int64_t n_reads,
                     void *d_positions_out, void *d_reads_out, uint64_t cap, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_hit_list_dev: NULL pointer");
    *n_out = 0;
    if (n_reads < 0) return fail(h, KDF_ERR_INVALID, "kdf_hit_list_dev: n_reads = %lld is negative", (long long)n_reads);
    if (d_reads_out && !d_read_offsets) return fail(h, KDF_ERR_INVALID, "kdf_hit_list_dev: reads_out needs read_offsets");
    if (n_bases == 0) return KDF_OK;
    if (!d_hit_bits || (cap && !d_positions_out)) return fail(h, KDF_ERR_INVALID, "kdf_hit_list_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    uint64_t n_blocks = 0, n_hits = 0;
    int rc;
    EvSpan p(h->timer[T_HITS], h->prof, h->stream, 1);
    if ((rc = hits_count(h, (const uint64_t *)d_hit_bits, n_bases, &n_blocks))) return rc;
    if (cap)
        hipLaunchKernelGGL(kh_write_kernel, dim3((unsigned)n_blocks), dim3(256), 0, h->stream, (const uint64_t *)d_hit_bits, n_bases,
                           h->hits.block_sums.as<const unsigned long long>(), (uint64_t *)d_positions_out, (int64_t *)d_reads_out,
                           (const int64_t *)d_read_offsets, n_reads, cap);
    p.stop();
    HIPCHK(h, hipGetLastError());
    if ((rc = hits_total(h, n_blocks, &n_hits))) return rc;
    *n_out = n_hits;
    if (n_hits > cap)
        return fail(h, KDF_ERR_INVALID, "kdf_hit_list_dev: the mask holds %llu hits, the buffers %llu", (unsigned long long)n_hits, (unsigned long long)cap);
    return KDF_OK;
}

int kdf_hit_list(kdf_engine *h, const uint64_t *hit_bits, uint64_t n_bases, const int64_t *read_offsets, int64_t n_reads,
                 uint64_t *positions_out, int64_t *reads_out, uint64_t cap, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_hit_list: NULL pointer");
    *n_out = 0;
    if (reads_out && !read_offsets) return fail(h, KDF_ERR_INVALID, "kdf_hit_list: reads_out needs read_offsets");
    int rc = check_read_offsets(EngSink{h}, "kdf_hit_list", read_offsets, read_offsets ? n_reads : (n_reads < 0 ? n_reads : 0));
    if (rc) return rc;
    if (n_bases == 0) return KDF_OK;
    if (!hit_bits || (cap && !positions_out)) return fail(h, KDF_ERR_INVALID, "kdf_hit_list: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_hit_list");
    const int ib = c.in(hit_bits, (n_bases + 63) / 64 * 8), io = c.in(read_offsets, reads_out ? (size_t)(n_reads + 1) * 8 : 0);
    const int ip = c.out(positions_out, cap * 8), ir = c.out(reads_out, reads_out ? cap * 8 : 0);
    if ((rc = c.commit())) return rc;
    const int rcl = kdf_hit_list_dev(h, c.dev(ib), n_bases, c.dev(io), reads_out ? n_reads : 0, c.dev(ip), c.dev(ir), cap, n_out);
    if (rcl && !(rcl == KDF_ERR_INVALID && *n_out > cap)) return rcl;
    const uint64_t n = std::min<uint64_t>(*n_out, cap);
    if (n && ((rc = c.fetch(ip, n * 8)) || (rc = c.fetch(ir, n * 8)) || (rc = c.finish()))) return rc;
    return rcl;
}

// ------------------------------------------------ hits in reference coordinates (kdf_coverage.h) ----

int kdf_hit_coverage_dev(kdf_engine *h, const void *d_hit_bits, uint64_t n_bases, const void *d_read_offsets, int64_t n_reads,
                         const void *d_ref_start, const void *d_cigar, uint64_t n_cigar, const void *d_cigar_offsets,
                         void *d_kmer_cov, void *d_read_cov, uint64_t span) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n_reads < 0) return fail(h, KDF_ERR_INVALID, "kdf_hit_coverage_dev: n_reads = %lld is negative", (long long)n_reads);
    if (n_reads == 0 || n_bases == 0) return KDF_OK;
    if (!d_hit_bits || !d_read_offsets || !d_ref_start || !d_cigar_offsets || (n_cigar && !d_cigar) || (span && (!d_kmer_cov || !d_read_cov)))
        return fail(h, KDF_ERR_INVALID, "kdf_hit_coverage_dev: NULL pointer");
    // a hit is a set bit p with p + k <= n_bases: the list is cut from the first n_bases - k + 1 bits; without an
    // operation or an accumulator word nothing can be added
    if (n_bases < (uint64_t)h->k || n_cigar == 0 || span == 0) return KDF_OK;
    const uint64_t n_starts = n_bases - (uint64_t)h->k + 1;
    HIPCHK(h, hipSetDevice(h->device));
    uint64_t n_blocks = 0, n_hits = 0;
    int rc;
    EvSpan p1(h->timer[T_COV], h->prof, h->stream, 1);            // (opens the call: counted as its pass)
    if ((rc = hits_count(h, (const uint64_t *)d_hit_bits, n_starts, &n_blocks))) return rc;
    p1.stop();
    if ((rc = hits_total(h, n_blocks, &n_hits))) return rc;
    if (n_hits == 0) return KDF_OK;
    if ((rc = eng_reserve(h, h->hits.positions, n_hits * 8, slack_8th, "hit list"))) return rc;
    if ((rc = eng_reserve(h, h->cov.cigar_pre, (size_t)n_cigar * 16, slack_8th, "CIGAR prefix sums"))) return rc;
    uint64_t *pos = h->hits.positions.as<uint64_t>();
    unsigned long long *pre = h->cov.cigar_pre.as<unsigned long long>();
    const int64_t *offs = (const int64_t *)d_read_offsets, *rs = (const int64_t *)d_ref_start, *co = (const int64_t *)d_cigar_offsets;
    const uint32_t *cig = (const uint32_t *)d_cigar;
    EvSpan p2(h->timer[T_COV], h->prof, h->stream, 0);            // (the same call's second group: time only)
    hipLaunchKernelGGL(kh_write_kernel, dim3((unsigned)n_blocks), dim3(256), 0, h->stream, (const uint64_t *)d_hit_bits, n_starts,
                       h->hits.block_sums.as<const unsigned long long>(), pos, (int64_t *)nullptr, (const int64_t *)nullptr, (int64_t)0, n_hits);
    hipLaunchKernelGGL(kc_prefix_kernel, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, h->stream, pos, n_hits, offs, n_reads, rs,
                       cig, n_cigar, co, pre);
    hipLaunchKernelGGL(kc_accum_kernel, dim3((unsigned)((n_hits + 255) / 256)), dim3(256), 0, h->stream, pos, n_hits, h->k, offs, n_reads, rs,
                       cig, n_cigar, co, (const unsigned long long *)pre, (uint32_t *)d_kmer_cov, (uint32_t *)d_read_cov, span);
    p2.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

int kdf_hit_coverage(kdf_engine *h, const uint64_t *hit_bits, uint64_t n_bases, const int64_t *read_offsets, int64_t n_reads,
                     const int64_t *ref_start, const uint32_t *cigar, uint64_t n_cigar, const int64_t *cigar_offsets,
                     uint32_t *kmer_cov, uint32_t *read_cov, uint64_t span) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    int rc = check_read_offsets(EngSink{h}, "kdf_hit_coverage", read_offsets, n_reads);  // (before any device work)
    if (rc) return rc;
    if (n_reads > 0) {
        if (!cigar_offsets || !ref_start) return fail(h, KDF_ERR_INVALID, "kdf_hit_coverage: NULL pointer");
        if (cigar_offsets[0] != 0) return fail(h, KDF_ERR_INVALID, "kdf_hit_coverage: cigar_offsets[0] = %lld, not 0", (long long)cigar_offsets[0]);
        for (int64_t r = 0; r < n_reads; ++r)
            if (cigar_offsets[r + 1] < cigar_offsets[r])
                return fail(h, KDF_ERR_INVALID, "kdf_hit_coverage: cigar_offsets decrease at read %lld (%lld after %lld)", (long long)r,
                            (long long)cigar_offsets[r + 1], (long long)cigar_offsets[r]);
        if ((uint64_t)cigar_offsets[n_reads] != n_cigar)
            return fail(h, KDF_ERR_INVALID, "kdf_hit_coverage: cigar_offsets end at %lld, n_cigar is %llu", (long long)cigar_offsets[n_reads],
                        (unsigned long long)n_cigar);
    }
    if (n_reads == 0 || n_bases == 0 || n_cigar == 0 || span == 0) return KDF_OK;
    if (!hit_bits || !cigar || !kmer_cov || !read_cov) return fail(h, KDF_ERR_INVALID, "kdf_hit_coverage: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, "kdf_hit_coverage");
    const size_t offs_bytes = (size_t)(n_reads + 1) * 8, cov_bytes = (size_t)span * 4;
    const int ib = c.in(hit_bits, (n_bases + 63) / 64 * 8), io = c.in(read_offsets, offs_bytes), irs = c.in(ref_start, (size_t)n_reads * 8);
    const int ic = c.in(cigar, (size_t)n_cigar * 4), ico = c.in(cigar_offsets, offs_bytes);
    const int ik = c.inout(kmer_cov, cov_bytes), ir = c.inout(read_cov, cov_bytes);          // the accumulators
    if ((rc = c.commit()) || (rc = kdf_hit_coverage_dev(h, c.dev(ib), n_bases, c.dev(io), n_reads, c.dev(irs), c.dev(ic), n_cigar, c.dev(ico),
                                                        c.dev(ik), c.dev(ir), span)) ||
        (rc = c.fetch(ik, cov_bytes)) || (rc = c.fetch(ir, cov_bytes))) return rc;
    return c.finish();
}

int kdf_coverage_list_dev(kdf_engine *h, const void *d_kmer_cov, const void *d_read_cov, uint64_t first, uint64_t n, uint32_t min_reads,
                          void *d_pos_out, void *d_kmer_out, void *d_read_out, uint64_t cap, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_coverage_list_dev: NULL pointer");
    *n_out = 0;
    if (n == 0) return KDF_OK;
    if (!d_read_cov || (cap && !d_pos_out) || (d_kmer_out && !d_kmer_cov)) return fail(h, KDF_ERR_INVALID, "kdf_coverage_list_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    return coverage_list_core(h, "kdf_coverage_list_dev", d_kmer_cov ? (const uint32_t *)d_kmer_cov + first : nullptr,
                              (const uint32_t *)d_read_cov + first, first, n, min_reads, d_pos_out, d_kmer_out, d_read_out, cap, n_out);
}

int kdf_coverage_list(kdf_engine *h, const uint32_t *kmer_cov, const uint32_t *read_cov, uint64_t first, uint64_t n, uint32_t min_reads,
                      uint64_t *pos_out, uint32_t *kmer_out, uint32_t *read_out, uint64_t cap, uint64_t *n_out) {
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "kdf_coverage_list: NULL pointer");
    *n_out = 0;
    if (n == 0) return KDF_OK;
    if (!read_cov || (cap && !pos_out) || (kmer_out && !kmer_cov)) return fail(h, KDF_ERR_INVALID, "kdf_coverage_list: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    // the window alone is staged
    HostCall c(h, "kdf_coverage_list");
    const int irc = c.in(read_cov + first, (size_t)n * 4), ikc = c.in(kmer_out ? kmer_cov + first : nullptr, kmer_out ? (size_t)n * 4 : 0);
    const int ip = c.out(pos_out, cap * 8), iko = c.out(kmer_out, kmer_out ? cap * 4 : 0), iro = c.out(read_out, read_out ? cap * 4 : 0);
    if ((rc = c.commit())) return rc;
    const int rcl = coverage_list_core(h, "kdf_coverage_list", c.dev<uint32_t>(ikc), c.dev<uint32_t>(irc), first, n, min_reads, c.dev(ip), c.dev(iko),
                                       c.dev(iro), cap, n_out);
    if (rcl && !(rcl == KDF_ERR_INVALID && *n_out > cap)) return rcl;
    const uint64_t m = std::min<uint64_t>(*n_out, cap);
    if (m && ((rc = c.fetch(ip, m * 8)) || (rc = c.fetch(iko, m * 4)) || (rc = c.fetch(iro, m * 4)) || (rc = c.finish()))) return rc;
    return rcl;
}

int kdf_hit_keys_dev(kdf_engine *h, const void *d_packed, uint64_t n_bases, const void *d_positions, uint64_t n, void *d_keys_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n == 0) return KDF_OK;
    if (!d_positions || !d_keys_out || (n_bases && !d_packed)) return fail(h, KDF_ERR_INVALID, "kdf_hit_keys_dev: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        hipLaunchKernelGGL(kc_keys_kernel<W>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const uint64_t *)d_packed, n_bases, h->k,
                           (const uint64_t *)d_positions, n, (uint64_t *)d_keys_out);
        return 0;
    });
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

int kdf_hit_keys(kdf_engine *h, const uint64_t *packed, uint64_t n_bases, const uint64_t *positions, uint64_t n, uint64_t *keys_out) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n == 0) return KDF_OK;
    if (!positions || !keys_out || (n_bases && !packed)) return fail(h, KDF_ERR_INVALID, "kdf_hit_keys: NULL pointer");
    HIPCHK(h, hipSetDevice(h->device));
    uint64_t pw, mw;
    kdf_stream_words(n_bases, &pw, &mw);
    const uint64_t pw_in = (n_bases + 31) / 32;
    const size_t key_bytes = (size_t)n * 8 * (size_t)h->kw;
    HostCall c(h, "kdf_hit_keys");
    const int is = c.out(nullptr, pw * 8), ip = c.in(positions, (size_t)n * 8), ik = c.out(keys_out, key_bytes);      // is: the packed words alone, zero-padded below
    int rc;
    if ((rc = c.commit())) return rc;
    HIPCHK(h, hipMemsetAsync(c.dev(is), 0, pw * 8, h->stream));
    if (pw_in) HIPCHK(h, hipMemcpyAsync(c.dev(is), packed, pw_in * 8, hipMemcpyHostToDevice, h->stream));
    if ((rc = kdf_hit_keys_dev(h, c.dev(is), n_bases, c.dev(ip), n, c.dev(ik))) || (rc = c.fetch(ik, key_bytes))) return rc;
    return c.finish();
}

// ------------------------------------------------ VCF mode on the device (kdf_variants.h) ----

int kdf_variant_windows_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases, const void *d_read_offsets,
                            int64_t n_reads, const void *d_ref_start, const void *d_cigar, uint64_t n_cigar, const void *d_cigar_offsets,
                            const void *d_qual, uint64_t n_qual, const void *d_qual_offsets, uint32_t min_baseq, const void *d_var_pos,
                            const void *d_var_span, const void *d_var_ref_len, uint64_t n_var, const void *d_alt, uint64_t n_alt,
                            const void *d_alt_offsets, void *d_pair_read, void *d_pair_var, void *d_pair_flags, uint64_t pair_cap,
                            void *d_entry_pos, void *d_entry_pair, uint64_t entry_cap, uint64_t *n_pairs_out, uint64_t *n_entries_out) {
    if (!h || !n_pairs_out || !n_entries_out) return fail(h, KDF_ERR_INVALID, "kdf_variant_windows_dev: NULL pointer");
    *n_pairs_out = *n_entries_out = 0;
    if (n_reads < 0) return fail(h, KDF_ERR_INVALID, "kdf_variant_windows_dev: n_reads = %lld is negative", (long long)n_reads);
    if (n_reads == 0 || n_var == 0 || n_bases == 0) return KDF_OK;
    if (!d_packed || !d_invalid || !d_read_offsets || !d_ref_start || !d_cigar_offsets || (n_cigar && !d_cigar) || !d_var_pos || !d_var_span ||
        !d_var_ref_len || !d_alt_offsets || (n_alt && !d_alt) || (d_qual && !d_qual_offsets) ||
        (pair_cap && (!d_pair_read || !d_pair_var || !d_pair_flags)) || (entry_cap && (!d_entry_pos || !d_entry_pair)))
        return fail(h, KDF_ERR_INVALID, "kdf_variant_windows_dev: NULL pointer");
    if (n_var >= (1ull << 32)) return fail(h, KDF_ERR_INVALID, "kdf_variant_windows_dev: %llu variants: pair_var holds 32 bits", (unsigned long long)n_var);
    if (n_bases < (uint64_t)h->k || n_cigar == 0) return KDF_OK;     // no window, or no aligned base
    HIPCHK(h, hipSetDevice(h->device));
    const uint64_t nbr = ((uint64_t)n_reads + 255) / 256;
    if (nbr >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "kdf_variant_windows_dev: %lld reads are beyond the 2^39 a call takes", (long long)n_reads);
    int rc;
    if ((rc = eng_reserve(h, h->hits.block_sums, (nbr + 1) * 8, slack_8th, "block sums"))) return rc;
    if ((rc = eng_reserve(h, h->var.cigar_pre, (size_t)n_cigar * 16, slack_8th, "CIGAR prefix sums"))) return rc;
    if ((rc = eng_reserve(h, h->var.ranges, (size_t)(2 * (uint64_t)n_reads + 1) * 8, slack_8th, "candidate ranges"))) return rc;
    unsigned long long *sums = h->hits.block_sums.as<unsigned long long>();
    uint64_t *cand_lo = h->var.ranges.as<uint64_t>();
    unsigned long long *cand_off = h->var.ranges.as<unsigned long long>() + n_reads;
    KvArgs a{};
    a.packed = (const uint64_t *)d_packed; a.invalid = (const uint64_t *)d_invalid; a.n_bases = n_bases; a.k = h->k;
    a.offs = (const int64_t *)d_read_offsets; a.n_reads = n_reads; a.ref_start = (const int64_t *)d_ref_start;
    a.cigar = (const uint32_t *)d_cigar; a.n_cigar = n_cigar; a.cig_offs = (const int64_t *)d_cigar_offsets;
    a.qual = min_baseq ? (const uint8_t *)d_qual : nullptr; a.n_qual = n_qual; a.qual_offs = (const int64_t *)d_qual_offsets; a.min_baseq = min_baseq;
    a.var_pos = (const int64_t *)d_var_pos; a.var_span = (const uint32_t *)d_var_span; a.var_ref_len = (const uint32_t *)d_var_ref_len; a.n_var = n_var;
    a.alt = (const uint8_t *)d_alt; a.n_alt = n_alt; a.alt_offs = (const int64_t *)d_alt_offsets;
    a.pre = h->var.cigar_pre.as<const unsigned long long>(); a.cand_lo = cand_lo; a.cand_off = cand_off;
    EvSpan p1(h->timer[T_VAR], h->prof, h->stream, 1);            // (opens the call: counted as its pass)
    hipLaunchKernelGGL(kv_range_kernel, dim3((unsigned)nbr), dim3(256), 0, h->stream, n_reads, a.ref_start, a.cigar, n_cigar, a.cig_offs, a.var_pos,
                       n_var, h->var.cigar_pre.as<unsigned long long>(), cand_lo, cand_off, sums);
    hipLaunchKernelGGL(kh_scan_kernel, dim3(1), dim3(256), 0, h->stream, sums, nbr);
    hipLaunchKernelGGL(kv_offsets_kernel, dim3((unsigned)nbr), dim3(256), 0, h->stream, n_reads, (const unsigned long long *)sums, cand_off);
    p1.stop();
    HIPCHK(h, hipGetLastError());
    uint64_t n_cand = 0;
    if ((rc = hits_total(h, nbr, &n_cand))) return rc;               // (first synchronisation: sizes the per-candidate scratch)
    if (n_cand == 0) return KDF_OK;
    const uint64_t nbc = (n_cand + 255) / 256;
    if (nbc >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "kdf_variant_windows_dev: %llu (read, variant) candidates are beyond the 2^39 a call takes", (unsigned long long)n_cand);
    if ((rc = eng_reserve(h, h->hits.block_sums, 2 * (nbc + 1) * 8, slack_8th, "block sums"))) return rc;
    if ((rc = eng_reserve(h, h->var.cand_counts, (size_t)n_cand * 5, slack_8th, "candidate counts"))) return rc;
    sums = h->hits.block_sums.as<unsigned long long>();
    unsigned long long *sums_p = sums, *sums_e = sums + nbc + 1;
    uint32_t *ent_cnt = h->var.cand_counts.as<uint32_t>();
    uint8_t *cflags = (uint8_t *)(ent_cnt + n_cand);
    a.n_cand = n_cand;
    EvSpan p2(h->timer[T_VAR], h->prof, h->stream, 0);            // (the same call's later groups: time only)
    hipLaunchKernelGGL(kv_count_kernel, dim3((unsigned)nbc), dim3(256), 0, h->stream, a, ent_cnt, cflags, sums_p, sums_e);
    hipLaunchKernelGGL(kh_scan_kernel, dim3(1), dim3(256), 0, h->stream, sums_p, nbc);
    hipLaunchKernelGGL(kh_scan_kernel, dim3(1), dim3(256), 0, h->stream, sums_e, nbc);
    p2.stop();
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->h_out4, sums_p + nbc, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->h_out4 + 1, sums_e + nbc, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                      // (second synchronisation: the two counts)
    const uint64_t n_pairs = h->h_out4[0], n_entries = h->h_out4[1];
    *n_pairs_out = n_pairs;
    *n_entries_out = n_entries;
    if (pair_cap == 0 && entry_cap == 0) {
        if (!d_pair_read && !d_pair_var && !d_pair_flags && !d_entry_pos && !d_entry_pair) return KDF_OK;       // a sizing call
    } else if (n_pairs) {
        EvSpan p3(h->timer[T_VAR], h->prof, h->stream, 0);
        hipLaunchKernelGGL(kv_write_kernel, dim3((unsigned)nbc), dim3(256), 0, h->stream, a, (const uint32_t *)ent_cnt, (const uint8_t *)cflags,
                           (const unsigned long long *)sums_p, (const unsigned long long *)sums_e, (int64_t *)d_pair_read, (uint32_t *)d_pair_var,
                           (uint8_t *)d_pair_flags, pair_cap, (uint64_t *)d_entry_pos, (uint64_t *)d_entry_pair, entry_cap);
        p3.stop();
        HIPCHK(h, hipGetLastError());
    }
    if (n_pairs > pair_cap || n_entries > entry_cap)
        return fail(h, KDF_ERR_INVALID, "kdf_variant_windows_dev: %llu pairs and %llu entries, the buffers hold %llu and %llu", (unsigned long long)n_pairs,
                    (unsigned long long)n_entries, (unsigned long long)pair_cap, (unsigned long long)entry_cap);
    return KDF_OK;
}

int kdf_variant_windows(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases, const int64_t *read_offsets,
                        int64_t n_reads, const int64_t *ref_start, const uint32_t *cigar, uint64_t n_cigar, const int64_t *cigar_offsets,
                        const uint8_t *qual, uint64_t n_qual, const int64_t *qual_offsets, uint32_t min_baseq, const int64_t *var_pos,
                        const uint32_t *var_span, const uint32_t *var_ref_len, uint64_t n_var, const uint8_t *alt, uint64_t n_alt,
                        const int64_t *alt_offsets, int64_t *pair_read, uint32_t *pair_var, uint8_t *pair_flags, uint64_t pair_cap,
                        uint64_t *entry_pos, uint64_t *entry_pair, uint64_t entry_cap, uint64_t *n_pairs_out, uint64_t *n_entries_out) {
    static const char *const fn = "kdf_variant_windows";
    if (!h || !n_pairs_out || !n_entries_out) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    *n_pairs_out = *n_entries_out = 0;
    int rc = check_read_offsets(EngSink{h}, fn, read_offsets, n_reads);                  // (before any device work)
    if (rc) return rc;
    if (n_reads > 0) {
        if (!ref_start) return fail(h, KDF_ERR_INVALID, "%s: ref_start is NULL", fn);
        if ((rc = check_offsets0(h, fn, "cigar_offsets", cigar_offsets, (uint64_t)n_reads, n_cigar))) return rc;
        if (qual && (rc = check_offsets0(h, fn, "qual_offsets", qual_offsets, (uint64_t)n_reads, n_qual))) return rc;
    }
    if (n_var > 0) {
        if (!var_pos || !var_span || !var_ref_len) return fail(h, KDF_ERR_INVALID, "%s: NULL variant array", fn);
        for (uint64_t v = 1; v < n_var; ++v)
            if (var_pos[v] < var_pos[v - 1])
                return fail(h, KDF_ERR_INVALID, "%s: var_pos decreases at variant %llu (%lld after %lld)", fn, (unsigned long long)v, (long long)var_pos[v], (long long)var_pos[v - 1]);
        if ((rc = check_offsets0(h, fn, "alt_offsets", alt_offsets, n_var, n_alt))) return rc;
    }
    if (n_reads == 0 || n_var == 0 || n_bases == 0 || n_cigar == 0) return KDF_OK;
    if (!packed || !invalid || !cigar || (n_alt && !alt) || (pair_cap && (!pair_read || !pair_var || !pair_flags)) || (entry_cap && (!entry_pos || !entry_pair)))
        return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    HIPCHK(h, hipSetDevice(h->device));
    const bool q = qual && min_baseq;
    const size_t offs_bytes = (size_t)(n_reads + 1) * 8;
    HostCall c(h, fn);
    const int is = c.stream(packed, invalid, n_bases), io = c.in(read_offsets, offs_bytes), irs = c.in(ref_start, (size_t)n_reads * 8);
    const int ic = c.in(cigar, (size_t)n_cigar * 4), ico = c.in(cigar_offsets, offs_bytes);
    const int iq = c.in(qual, q ? (size_t)n_qual : 0), iqo = c.in(qual_offsets, q ? offs_bytes : 0);
    const int ivp = c.in(var_pos, (size_t)n_var * 8), ivs = c.in(var_span, (size_t)n_var * 4), ivr = c.in(var_ref_len, (size_t)n_var * 4);
    const int ia = c.in(alt, (size_t)n_alt), iao = c.in(alt_offsets, (size_t)(n_var + 1) * 8);
    const int opr = c.out(pair_read, (size_t)pair_cap * 8), opv = c.out(pair_var, (size_t)pair_cap * 4), opf = c.out(pair_flags, (size_t)pair_cap);
    const int oep = c.out(entry_pos, (size_t)entry_cap * 8), oer = c.out(entry_pair, (size_t)entry_cap * 8);
    if ((rc = c.commit())) return rc;
    const int rcl = kdf_variant_windows_dev(h, c.dev(is), c.dev(is + 1), n_bases, c.dev(io), n_reads, c.dev(irs), c.dev(ic), n_cigar, c.dev(ico), c.dev(iq),
                                            q ? n_qual : 0, c.dev(iqo), min_baseq, c.dev(ivp), c.dev(ivs), c.dev(ivr), n_var, c.dev(ia), n_alt, c.dev(iao),
                                            c.dev(opr), c.dev(opv), c.dev(opf), pair_cap, c.dev(oep), c.dev(oer), entry_cap, n_pairs_out, n_entries_out);
    if (rcl && !(rcl == KDF_ERR_INVALID && (*n_pairs_out > pair_cap || *n_entries_out > entry_cap))) return rcl;
    const uint64_t np = std::min<uint64_t>(*n_pairs_out, pair_cap), ne = std::min<uint64_t>(*n_entries_out, entry_cap);
    if ((rc = c.fetch(opr, np * 8)) || (rc = c.fetch(opv, np * 4)) || (rc = c.fetch(opf, np)) || (rc = c.fetch(oep, ne * 8)) || (rc = c.fetch(oer, ne * 8)) ||
        (rc = c.finish())) return rc;
    return rcl;
}

int kdf_variant_evidence_dev(kdf_engine *h, const void *d_keys, const void *d_entry_pair, uint64_t n_entries, const void *d_pair_var,
                             const void *d_pair_flags, uint64_t n_pairs, uint64_t n_var, void *d_pair_rows, void *d_var_rows) {
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if ((n_pairs && !d_pair_rows) || (n_var && !d_var_rows)) return fail(h, KDF_ERR_INVALID, "kdf_variant_evidence_dev: NULL pointer");
    const bool work = n_entries && n_pairs && n_var;
    if (work && (!d_keys || !d_entry_pair || !d_pair_var || !d_pair_flags)) return fail(h, KDF_ERR_INVALID, "kdf_variant_evidence_dev: NULL pointer");
    // (variant, tag, slot) must fit 63 bits: bit 63 keeps every word apart from the set's empty word.  Refused before
    // anything is written, and once more below when pending work has grown the table
    if (n_var >= (1ull << 62) || log2ceil(n_var) + 1 + h->t.log2cap > 63)
        return fail(h, KDF_ERR_INVALID, "kdf_variant_evidence_dev: %llu variants against a table of 2^%u slots: variant index, tag and slot index must "
                    "fit 63 bits together", (unsigned long long)n_var, h->t.log2cap);
    if ((n_entries + 255) / 256 >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "kdf_variant_evidence_dev: %llu entries are beyond the 2^39 a call takes", (unsigned long long)n_entries);
    HIPCHK(h, hipSetDevice(h->device));
    if (work) {
        { int rcf = pending_flush(h); if (rcf) return rcf; }
        { int rc0 = materialize(h); if (rc0) return rc0; }
        if (log2ceil(n_var) + 1 + h->t.log2cap > 63)
            return fail(h, KDF_ERR_INVALID, "kdf_variant_evidence_dev: %llu variants against a table of 2^%u slots: variant index, tag and slot index "
                        "must fit 63 bits together", (unsigned long long)n_var, h->t.log2cap);
    }
    if (n_pairs) HIPCHK(h, hipMemsetAsync(d_pair_rows, 0, (size_t)n_pairs * KV_PAIR_WORDS * 4, h->stream));
    if (n_var) HIPCHK(h, hipMemsetAsync(d_var_rows, 0, (size_t)n_var * KV_VAR_WORDS * 8, h->stream));
    if (!work) return KDF_OK;
    const uint32_t log2set = log2ceil(4 * n_entries);              // two words per entry at most, load <= 0.5
    int rc;
    if ((rc = eng_reserve(h, h->hits.pair_set, (size_t)8 << log2set, slack_8th, "set of (variant, k-mer) pairs"))) return rc;
    unsigned long long *set = h->hits.pair_set.as<unsigned long long>();
    EvSpan p(h->timer[T_VAR], h->prof, h->stream, 1);
    HIPCHK(h, hipMemsetAsync(set, 0xFF, (size_t)8 << log2set, h->stream));
    by_words(h, [&](auto Wc) {
        constexpr int W = decltype(Wc)::value;
        hipLaunchKernelGGL(kv_evidence_kernel<W>, dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, h->stream, h->t, (const uint64_t *)d_keys,
                           (const uint64_t *)d_entry_pair, n_entries, (const uint32_t *)d_pair_var, (const uint8_t *)d_pair_flags, n_pairs, n_var, set,
                           log2set, (uint32_t *)d_pair_rows, (unsigned long long *)d_var_rows);
        return 0;
    });
    hipLaunchKernelGGL(kv_rows_fix_kernel, dim3((unsigned)((n_var + 255) / 256)), dim3(256), 0, h->stream, (unsigned long long *)d_var_rows, n_var);
    p.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

int kdf_variant_evidence(kdf_engine *h, const uint64_t *keys, const uint64_t *entry_pair, uint64_t n_entries, const uint32_t *pair_var,
                         const uint8_t *pair_flags, uint64_t n_pairs, uint64_t n_var, uint32_t *pair_rows, uint64_t *var_rows) {
    static const char *const fn = "kdf_variant_evidence";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if ((n_pairs && (!pair_rows || !pair_var || !pair_flags)) || (n_var && !var_rows) || (n_entries && (!keys || !entry_pair)))
        return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t pair_bytes = (size_t)n_pairs * KV_PAIR_WORDS * 4, var_bytes = (size_t)n_var * KV_VAR_WORDS * 8;
    HostCall c(h, fn);
    const int ik = c.in(keys, (size_t)n_entries * 8 * (size_t)h->kw), iep = c.in(entry_pair, (size_t)n_entries * 8);
    const int ipv = c.in(pair_var, (size_t)n_pairs * 4), ipf = c.in(pair_flags, (size_t)n_pairs);
    const int opr = c.out(pair_rows, pair_bytes), ovr = c.out(var_rows, var_bytes);
    int rc;
    if ((rc = c.commit()) || (rc = kdf_variant_evidence_dev(h, c.dev(ik), c.dev(iep), n_entries, c.dev(ipv), c.dev(ipf), n_pairs, n_var, c.dev(opr), c.dev(ovr))) ||
        (rc = c.fetch(opr, pair_bytes)) || (rc = c.fetch(ovr, var_bytes))) return rc;
    return c.finish();
}

// ------------------------------------------------ regions of informative reads (kdf_regions.h) ----

int kdf_cluster_intervals_dev(kdf_engine *h, const void *d_chrom, const void *d_start, const void *d_end, int64_t n, int64_t merge_distance,
                              void *d_region_of, void *d_regions_out, uint64_t cap, uint64_t *n_out) {
    static const char *const fn = "kdf_cluster_intervals_dev";
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    *n_out = 0;
    if (n < 0 || (uint64_t)n >= (1ull << 32)) return fail(h, KDF_ERR_INVALID, "%s: n = %lld outside 0 .. 2^32 - 1", fn, (long long)n);
    if (merge_distance < 0 || merge_distance >= (1ll << 62)) return fail(h, KDF_ERR_INVALID, "%s: merge_distance = %lld outside 0 .. 2^62 - 1", fn, (long long)merge_distance);
    if (n == 0) return KDF_OK;
    if (!d_chrom || !d_start || !d_end || !d_region_of || (cap && !d_regions_out)) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    HIPCHK(h, hipSetDevice(h->device));
    const uint64_t un = (uint64_t)n, nb = (un + KR_BLOCK - 1) / KR_BLOCK;
    // scratch: the chrom word of the sort, then the block maxima, then one flag per entry
    StageLayout lay;
    const int ik = lay.add(un * 8), ia = lay.add(nb * sizeof(KrMax)), ifl = lay.add(un);
    int rc;
    if ((rc = eng_reserve(h, h->reg.scratch, lay.total, slack_8th, "interval scratch"))) return rc;
    if ((rc = eng_reserve(h, h->reg.perm, un * 4, slack_8th, "interval order"))) return rc;
    if ((rc = eng_reserve(h, h->hits.block_sums, (nb + 1) * 8, slack_8th, "block sums"))) return rc;
    uint64_t *ckey = (uint64_t *)lay.at(h->reg.scratch.p, ik);
    KrMax *agg = (KrMax *)lay.at(h->reg.scratch.p, ia);
    uint8_t *flags = (uint8_t *)lay.at(h->reg.scratch.p, ifl);
    uint32_t *perm = h->reg.perm.as<uint32_t>();
    unsigned long long *sums = h->hits.block_sums.as<unsigned long long>();
    const int64_t *chrom = (const int64_t *)d_chrom, *start = (const int64_t *)d_start, *end = (const int64_t *)d_end;
    const unsigned blocks = (unsigned)nb;
    EvSpan p1(h->timer[T_REG], h->prof, h->stream, 1);            // (opens the call: counted as its pass)
    hipLaunchKernelGGL(kr_chrom_key_kernel, dim3(blocks), dim3(256), 0, h->stream, chrom, un, ckey);
    HIPCHK(h, hipGetLastError());
    {
        const KdfSortPass passes[2] = {{(const uint64_t *)d_start, 1, 0, 62}, {ckey, 1, 0, 32}};
        std::string serr;
        if (kdf_sort_perm_device(passes, 2, un, perm, h->stream, serr)) return fail(h, KDF_ERR_HIP, "%s: sort failed: %s", fn, serr.c_str());
    }
    hipLaunchKernelGGL(kr_max_block_kernel, dim3(blocks), dim3(256), 0, h->stream, chrom, end, (const uint32_t *)perm, un, agg);
    hipLaunchKernelGGL(kr_max_scan_kernel, dim3(1), dim3(256), 0, h->stream, agg, nb);
    hipLaunchKernelGGL(kr_flag_kernel, dim3(blocks), dim3(256), 0, h->stream, chrom, start, end, (const uint32_t *)perm, un, (uint64_t)merge_distance,
                       (const KrMax *)agg, flags, sums);
    hipLaunchKernelGGL(kh_scan_kernel, dim3(1), dim3(256), 0, h->stream, sums, nb);
    p1.stop();
    HIPCHK(h, hipGetLastError());
    uint64_t n_regions = 0;
    if ((rc = hits_total(h, nb, &n_regions))) return rc;             // (synchronises: the caller learns the number of regions)
    *n_out = n_regions;
    const uint64_t rows = std::min<uint64_t>(n_regions, cap);
    EvSpan p2(h->timer[T_REG], h->prof, h->stream, 0);            // (the same call's second group: time only)
    if (rows) HIPCHK(h, hipMemsetAsync(d_regions_out, 0, rows * 32, h->stream));
    hipLaunchKernelGGL(kr_regions_kernel, dim3(blocks), dim3(256), 0, h->stream, chrom, start, end, (const uint32_t *)perm, (const uint8_t *)flags, un,
                       (const unsigned long long *)sums, (int64_t *)d_region_of, (unsigned long long *)d_regions_out, rows);
    p2.stop();
    HIPCHK(h, hipGetLastError());
    if (n_regions > cap)
        return fail(h, KDF_ERR_INVALID, "%s: %llu regions, the buffer holds %llu", fn, (unsigned long long)n_regions, (unsigned long long)cap);
    return KDF_OK;
}

int kdf_cluster_intervals(kdf_engine *h, const int64_t *chrom, const int64_t *start, const int64_t *end, int64_t n, int64_t merge_distance,
                          int64_t *region_of, int64_t *regions_out, uint64_t cap, uint64_t *n_out) {
    static const char *const fn = "kdf_cluster_intervals";
    if (!h || !n_out) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    *n_out = 0;
    if (n < 0 || (uint64_t)n >= (1ull << 32)) return fail(h, KDF_ERR_INVALID, "%s: n = %lld outside 0 .. 2^32 - 1", fn, (long long)n);
    if (merge_distance < 0 || merge_distance >= (1ll << 62)) return fail(h, KDF_ERR_INVALID, "%s: merge_distance = %lld outside 0 .. 2^62 - 1", fn, (long long)merge_distance);
    if (n == 0) return KDF_OK;
    if (!chrom || !start || !end || !region_of || (cap && !regions_out)) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    for (int64_t i = 0; i < n; ++i) {                                 // (before any device work; skipped intervals are not looked at)
        if (chrom[i] < 0) continue;
        if (chrom[i] >= (1ll << 31)) return fail(h, KDF_ERR_INVALID, "%s: chrom[%lld] = %lld is not below 2^31", fn, (long long)i, (long long)chrom[i]);
        if (start[i] < 0 || end[i] < start[i] || end[i] >= (1ll << 62))
            return fail(h, KDF_ERR_INVALID, "%s: interval %lld = [%lld, %lld) breaks 0 <= start <= end < 2^62", fn, (long long)i, (long long)start[i], (long long)end[i]);
    }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t col = (size_t)n * 8;
    HostCall c(h, fn);
    const int ic = c.in(chrom, col), is = c.in(start, col), ie = c.in(end, col), iro = c.out(region_of, col), irg = c.out(regions_out, (size_t)cap * 32);
    int rc;
    if ((rc = c.commit())) return rc;
    const int rcl = kdf_cluster_intervals_dev(h, c.dev(ic), c.dev(is), c.dev(ie), n, merge_distance, c.dev(iro), c.dev(irg), cap, n_out);
    if (rcl && !(rcl == KDF_ERR_INVALID && *n_out > cap)) return rcl;
    if ((rc = c.fetch(iro, col)) || (rc = c.fetch(irg, (size_t)std::min<uint64_t>(*n_out, cap) * 32)) || (rc = c.finish())) return rc;
    return rcl;
}

int kdf_group_distinct_dev(kdf_engine *h, const void *d_group, const void *d_keys, int words, uint64_t n, int64_t n_groups, void *d_counts_out) {
    static const char *const fn = "kdf_group_distinct_dev";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n >= (1ull << 32)) return fail(h, KDF_ERR_INVALID, "%s: %llu entries are beyond the 2^32 - 1 a call takes", fn, (unsigned long long)n);
    if (words < 1 || words > 8) return fail(h, KDF_ERR_INVALID, "%s: words = %d outside 1 .. 8", fn, words);
    if (n_groups < 0) return fail(h, KDF_ERR_INVALID, "%s: n_groups = %lld is negative", fn, (long long)n_groups);
    if (n_groups == 0) return KDF_OK;
    if (!d_counts_out || (n && (!d_group || !d_keys))) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemsetAsync(d_counts_out, 0, (size_t)n_groups * 8, h->stream));
    if (n == 0) return KDF_OK;
    int rc;
    if ((rc = eng_reserve(h, h->reg.scratch, n * 8, slack_8th, "group words"))) return rc;
    if ((rc = eng_reserve(h, h->reg.perm, n * 4, slack_8th, "row order"))) return rc;
    uint64_t *gkey = h->reg.scratch.as<uint64_t>();
    uint32_t *perm = h->reg.perm.as<uint32_t>();
    const uint64_t *keys = (const uint64_t *)d_keys;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    EvSpan p(h->timer[T_REG], h->prof, h->stream, 1);
    hipLaunchKernelGGL(kr_group_key_kernel, dim3(blocks), dim3(256), 0, h->stream, (const int64_t *)d_group, keys, words, n, (uint64_t)n_groups, gkey);
    HIPCHK(h, hipGetLastError());
    {
        // the group word on top: its values are 0 .. n_groups (n_groups: ignored), so it costs the radix passes of their bits
        KdfSortPass passes[9];
        for (int j = 0; j < words; ++j) passes[j] = KdfSortPass{keys + j, (uint64_t)words, 0, 64};
        passes[words] = KdfSortPass{gkey, 1, 0, (int)std::max<uint32_t>(1, log2ceil((uint64_t)n_groups + 1))};
        std::string serr;
        if (kdf_sort_perm_device(passes, words + 1, n, perm, h->stream, serr)) return fail(h, KDF_ERR_HIP, "%s: sort failed: %s", fn, serr.c_str());
    }
    hipLaunchKernelGGL(kr_distinct_kernel, dim3(blocks), dim3(256), 0, h->stream, (const uint64_t *)gkey, keys, words, (const uint32_t *)perm, n,
                       (uint64_t)n_groups, (unsigned long long *)d_counts_out);
    p.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

int kdf_group_distinct(kdf_engine *h, const int64_t *group, const uint64_t *keys, int words, uint64_t n, int64_t n_groups, uint64_t *counts_out) {
    static const char *const fn = "kdf_group_distinct";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (n >= (1ull << 32)) return fail(h, KDF_ERR_INVALID, "%s: %llu entries are beyond the 2^32 - 1 a call takes", fn, (unsigned long long)n);
    if (words < 1 || words > 8) return fail(h, KDF_ERR_INVALID, "%s: words = %d outside 1 .. 8", fn, words);
    if (n_groups < 0) return fail(h, KDF_ERR_INVALID, "%s: n_groups = %lld is negative", fn, (long long)n_groups);
    if (n_groups == 0) return KDF_OK;
    if (!counts_out || (n && (!group || !keys))) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    const size_t count_bytes = (size_t)n_groups * 8;
    if (n == 0) { memset(counts_out, 0, count_bytes); return KDF_OK; }
    HIPCHK(h, hipSetDevice(h->device));
    HostCall c(h, fn);
    const int ig = c.in(group, (size_t)n * 8), ik = c.in(keys, (size_t)n * 8 * (size_t)words), io = c.out(counts_out, count_bytes);
    int rc;
    if ((rc = c.commit()) || (rc = kdf_group_distinct_dev(h, c.dev(ig), c.dev(ik), words, n, n_groups, c.dev(io))) || (rc = c.fetch(io, count_bytes))) return rc;
    return c.finish();
}

}  // extern "C"
