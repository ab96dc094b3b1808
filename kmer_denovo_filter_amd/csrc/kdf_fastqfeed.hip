// kdf_fastqfeed.hip -- libkdf.so, the device FASTQ feeder (kdf_fastqfeed.h): kdf_fastq_pack, and kdf_fq_extract on the
// same line index, each one function with a `mem` argument: host arrays are staged through the engine's staging frame,
// device arrays are used in place.
// The table is not touched and nothing is flushed; what this unit uses of the engine is declared in kdf_engine_priv.h.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "kdf_engine_priv.h"
#include "kdf_fastqfeed.h"

static const char *const fq_rule_text[5] = {"", "line 0 does not begin with '@'", "line 2 does not begin with '+'",
                                            "the sequence and quality lines differ in length", "the last record has fewer than four lines"};

// The scratch of one call: the arrays of passes (1)-(5) for r_cap records, and `tail_bytes` behind them (the feeder's word
// index, the extract's tile index).
static int fq_scratch(kdf_engine *h, const void *d_text, uint64_t n_bytes, uint64_t r_cap, uint64_t tail_bytes, KfqScratchView &v, uint64_t &nt,
                      uint64_t &rec_blocks) {
    const uint32_t skew = (uint32_t)((uintptr_t)d_text & 15);          // the tiles are laid over 16-byte granules of the memory
    nt = n_bytes ? (n_bytes + skew + KFQ_TILE - 1) / KFQ_TILE : 0;
    rec_blocks = std::max<uint64_t>((r_cap + KFQ_REC_BLOCK - 1) / KFQ_REC_BLOCK, 1);
    auto up16 = [](uint64_t b) { return (b + 15) / 16 * 16; };
    const uint64_t b_ctl = up16(KFQ_CTL_WORDS * 8), b_tile = up16(nt * 4), b_nl = up16(4 * r_cap * 4), b_off = up16((r_cap + 1) * 8),
                   b_bsum = up16(rec_blocks * 8), b_word = up16(tail_bytes);
    int rc;                                                            // (the entry points have set the device)
    if ((rc = eng_reserve(h, h->fq.scratch, b_ctl + b_tile + b_nl + b_off + b_bsum + b_word, slack_8th, "FASTQ feeder scratch"))) return rc;
    char *base = h->fq.scratch.as<char>();
    v.ctl = (unsigned long long *)base;
    v.tile_nl = (uint32_t *)(base + b_ctl);
    v.nl = (uint32_t *)(base + b_ctl + b_tile);
    v.off = (unsigned long long *)(base + b_ctl + b_tile + b_nl);
    v.bsum = (unsigned long long *)(base + b_ctl + b_tile + b_nl + b_off);
    v.word_rec = v.tile_rec = (uint32_t *)(base + b_ctl + b_tile + b_nl + b_off + b_bsum);
    return KDF_OK;
}

// Passes (1)-(5) on the engine's stream: the end of the text, the line ends per tile, their scan, the line offsets and the
// per-record rule check.  Both entry points read the records off what this leaves in the scratch.
static void fq_records(kdf_engine *h, const KfqScratchView &v, const uint8_t *t, uint64_t n_bytes, int final_chunk, uint64_t cap_rec, uint64_t r_cap,
                       uint64_t nt, uint64_t rec_blocks) {
    const uint32_t skew = (uint32_t)((uintptr_t)t & 15);
    const dim3 wg(256);
    hipLaunchKernelGGL(kfq_end_kernel, dim3(1), wg, 0, h->stream, t, n_bytes, final_chunk, v.ctl);
    if (nt) hipLaunchKernelGGL(kfq_count_kernel, dim3((unsigned)nt), wg, 0, h->stream, t, n_bytes, skew, (const unsigned long long *)v.ctl, v.tile_nl);
    hipLaunchKernelGGL(kfq_scan_kernel, dim3(1), wg, 0, h->stream, v.tile_nl, nt, final_chunk, cap_rec, r_cap, v.ctl);
    if (nt) hipLaunchKernelGGL(kfq_lines_kernel, dim3((unsigned)nt), wg, 0, h->stream, t, n_bytes, skew, final_chunk, (const unsigned long long *)v.ctl,
                               (const uint32_t *)v.tile_nl, v.nl);
    hipLaunchKernelGGL(kfq_records_kernel, dim3((unsigned)rec_blocks), dim3(KFQ_REC_BLOCK), 0, h->stream, t, final_chunk, v.ctl, (const uint32_t *)v.nl, v.off, v.bsum);
}

// Launches the passes and queues the copy of the four result words to h->h_out4; the caller synchronises.  Every array
// argument is a device pointer.
static int fq_core(kdf_engine *h, const void *d_text, uint64_t n_bytes, int final_chunk, uint32_t min_qual, void *d_packed, void *d_invalid,
                   uint64_t cap_bases, void *d_offsets, uint64_t cap_reads) {
    // The records the buffers admit, and those the scratch is sized for: a record that breaks no rule takes 6 bytes or more
    // unless it is the last, so among the first n_bytes / 6 + 1 records of a text that has more, one is bad -- and that is
    // what the call reports.
    const uint64_t cap_rec = d_offsets ? std::min(cap_bases, cap_reads) : cap_bases;
    const uint64_t r_cap = std::min(cap_rec, n_bytes / 6 + 1), pos_cap = std::min(cap_bases, n_bytes / 2);
    const uint64_t pack_blocks = ((pos_cap + 63) / 64 + 2 + 3) / 4;
    KfqScratchView v;
    uint64_t nt, rec_blocks;
    int rc;
    if ((rc = fq_scratch(h, d_text, n_bytes, r_cap, ((pos_cap + 63) / 64 + 1) * 4, v, nt, rec_blocks))) return rc;
    const uint8_t *t = (const uint8_t *)d_text;
    const dim3 wg(256);
    EvSpan span(h->timer[T_FQ], h->prof, h->stream, 1);
    fq_records(h, v, t, n_bytes, final_chunk, cap_rec, r_cap, nt, rec_blocks);
    hipLaunchKernelGGL((kfq_total_kernel<false>), dim3(1), wg, 0, h->stream, n_bytes, final_chunk, (uint64_t)0, cap_bases, (const uint32_t *)v.nl, v.bsum, v.ctl);
    hipLaunchKernelGGL(kfq_offsets_kernel, dim3((unsigned)rec_blocks), dim3(KFQ_REC_BLOCK), 0, h->stream, (const unsigned long long *)v.ctl,
                       (const unsigned long long *)v.bsum, v.off, v.word_rec, (int64_t *)d_offsets);
    if (min_qual)
        hipLaunchKernelGGL((kfq_pack_kernel<true>), dim3((unsigned)pack_blocks), wg, 0, h->stream, t, min_qual, (const unsigned long long *)v.ctl, (const uint32_t *)v.nl,
                           (const unsigned long long *)v.off, (const uint32_t *)v.word_rec, (uint64_t *)d_packed, (uint64_t *)d_invalid);
    else
        hipLaunchKernelGGL((kfq_pack_kernel<false>), dim3((unsigned)pack_blocks), wg, 0, h->stream, t, min_qual, (const unsigned long long *)v.ctl, (const uint32_t *)v.nl,
                           (const unsigned long long *)v.off, (const uint32_t *)v.word_rec, (uint64_t *)d_packed, (uint64_t *)d_invalid);
    span.stop();
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->h_out4, v.ctl + KFQ_RES, 4 * 8, hipMemcpyDeviceToHost, h->stream));
    return KDF_OK;
}

// kdf_fq_extract: passes (1)-(5), then the kept lengths, their scan and the copy.  Queues the copy of the four result
// words to h->h_out4; the caller synchronises.  cap_out: what the output admits, at most n_bytes + 2 (no output needs more).
static int fx_core(kdf_engine *h, const void *d_text, uint64_t n_bytes, int final_chunk, const void *d_keep, uint64_t n_reads, void *d_out, uint64_t cap_out,
                   void *d_out_offsets) {
    const uint64_t r_cap = n_bytes / 6 + 1;                            // every record is examined: a text of more has a bad one among these
    const uint32_t oskew = (uint32_t)((uintptr_t)d_out & 15);
    const uint64_t out_tiles = (cap_out + oskew + KFQ_TILE - 1) / KFQ_TILE;
    KfqScratchView v;
    uint64_t nt, rec_blocks;
    int rc;
    if ((rc = fq_scratch(h, d_text, n_bytes, r_cap, (out_tiles + 1) * 4, v, nt, rec_blocks))) return rc;
    const uint8_t *t = (const uint8_t *)d_text;
    const dim3 wg(256);
    const uint64_t copy_blocks = std::max<uint64_t>(std::min<uint64_t>(out_tiles, (uint64_t)h->n_cu * 8), 1);
    EvSpan span(h->timer[T_FX], h->prof, h->stream, 1);
    fq_records(h, v, t, n_bytes, final_chunk, ~0ull, r_cap, nt, rec_blocks);
    hipLaunchKernelGGL(kfx_len_kernel, dim3((unsigned)rec_blocks), dim3(KFQ_REC_BLOCK), 0, h->stream, t, n_bytes, final_chunk, (const uint8_t *)d_keep, n_reads, v.ctl,
                       (const uint32_t *)v.nl, v.off, v.bsum);
    hipLaunchKernelGGL((kfq_total_kernel<true>), dim3(1), wg, 0, h->stream, n_bytes, final_chunk, n_reads, cap_out, (const uint32_t *)v.nl, v.bsum, v.ctl);
    hipLaunchKernelGGL(kfx_offsets_kernel, dim3((unsigned)rec_blocks), dim3(KFQ_REC_BLOCK), 0, h->stream, (const unsigned long long *)v.ctl,
                       (const unsigned long long *)v.bsum, oskew, v.off, v.tile_rec, (int64_t *)d_out_offsets);
    hipLaunchKernelGGL(kfx_copy_kernel, dim3((unsigned)copy_blocks), wg, 0, h->stream, t, final_chunk, oskew, (const unsigned long long *)v.ctl, (const uint32_t *)v.nl,
                       (const unsigned long long *)v.off, (const uint32_t *)v.tile_rec, (uint8_t *)d_out);
    span.stop();
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->h_out4, v.ctl + KFQ_RES, 4 * 8, hipMemcpyDeviceToHost, h->stream));
    return KDF_OK;
}

extern "C" {

int kdf_fastq_pack(kdf_engine *h, int mem, const void *text, uint64_t n_bytes, int final_chunk, uint32_t min_qual, kdf_fastq_state *state,
                   void *packed, void *invalid, uint64_t cap_bases, void *offsets, uint64_t cap_reads,
                   uint64_t *n_bases, uint64_t *n_reads, uint64_t *consumed, uint64_t *bad_offset, uint32_t *bad_rule) {
    static const char *const fn = "kdf_fastq_pack";
    if (bad_offset) *bad_offset = ~0ull;
    if (bad_rule) *bad_rule = 0;
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "%s: NULL engine", fn);
    if (!state || !n_bases || !n_reads || !consumed) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    *n_bases = 0; *n_reads = 0; *consumed = 0;
    if (mem != KDF_MEM_HOST && mem != KDF_MEM_DEVICE) return fail(h, KDF_ERR_INVALID, "%s: mem = %d (0 host, 1 device)", fn, mem);
    if (min_qual > 255) return fail(h, KDF_ERR_INVALID, "%s: min_qual = %u is beyond a byte", fn, min_qual);
    if (n_bytes > (1ull << 31)) return fail(h, KDF_ERR_INVALID, "%s: a chunk of %llu bytes is beyond the 2^31 a call takes", fn, (unsigned long long)n_bytes);
    if (n_bytes == 0 && !final_chunk) return KDF_OK;
    if ((n_bytes && !text) || !packed || !invalid) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    if (!offsets) cap_reads = 0;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    uint64_t pw, mw;
    HostCall c(h, fn);
    int op = -1, om = -1, oo = -1;
    if (mem == KDF_MEM_DEVICE) {
        if ((rc = fq_core(h, text, n_bytes, final_chunk, min_qual, packed, invalid, cap_bases, offsets, cap_reads))) return rc;
    } else {
        kdf_stream_words(cap_bases, &pw, &mw);
        const int it = c.in(text, (size_t)n_bytes);
        op = c.out(packed, (size_t)pw * 8); om = c.out(invalid, (size_t)mw * 8); oo = c.out(offsets, offsets ? (size_t)(cap_reads + 1) * 8 : 0);
        if ((rc = c.commit()) || (rc = fq_core(h, c.dev(it), n_bytes, final_chunk, min_qual, c.dev(op), c.dev(om), cap_bases, c.dev(oo), cap_reads))) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));                       // (the caller learns the sizes and a possible error)
    const uint64_t nb = h->h_out4[0], nr = h->h_out4[1], m = h->h_out4[2], verdict = h->h_out4[3] & 0xFFu, bad = h->h_out4[3] >> 8;
    if (verdict == KFQ_ERR_ROOM)
        return fail(h, KDF_ERR_INVALID, "%s: the chunk holds %llu records (and packs to %llu positions if they are well formed), the buffers hold %llu and %llu", fn,
                    (unsigned long long)nr, (unsigned long long)nb, (unsigned long long)(offsets ? cap_reads : nr), (unsigned long long)cap_bases);
    if (verdict == KFQ_ERR_FORMAT) {
        const uint32_t rule = (uint32_t)(bad & 7u);
        if (bad_offset) *bad_offset = bad >> 3;
        if (bad_rule) *bad_rule = rule;
        return fail(h, KDF_ERR_IO, "%s: the record at offset %llu of the chunk (byte %llu of the text) is no FASTQ record: %s", fn, (unsigned long long)(bad >> 3),
                    (unsigned long long)(state->bytes + (bad >> 3)), fq_rule_text[rule <= 4 ? rule : 0]);
    }
    if (mem == KDF_MEM_HOST && verdict == KFQ_OK) {
        kdf_stream_words(nb, &pw, &mw);
        if ((rc = c.fetch(op, (size_t)pw * 8)) || (rc = c.fetch(om, (size_t)mw * 8)) || (rc = c.fetch(oo, offsets ? (size_t)(nr + 1) * 8 : 0)) || (rc = c.finish()))
            return rc;
    }
    state->records += nr; state->positions += nb; state->bytes += m;
    *n_bases = nb; *n_reads = nr; *consumed = m;
    return KDF_OK;
}

int kdf_fq_extract(kdf_engine *h, int mem, const void *text, uint64_t n_bytes, int final_chunk, const void *keep, uint64_t n_reads,
                      void *out, uint64_t cap_out, void *out_offsets, uint64_t *out_bytes, uint64_t *n_kept, uint64_t *consumed,
                      uint64_t *bad_offset, uint32_t *bad_rule) {
    static const char *const fn = "kdf_fq_extract";
    if (bad_offset) *bad_offset = ~0ull;
    if (bad_rule) *bad_rule = 0;
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "%s: NULL engine", fn);
    if (!out_bytes || !n_kept || !consumed) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    *out_bytes = 0; *n_kept = 0; *consumed = 0;
    if (mem != KDF_MEM_HOST && mem != KDF_MEM_DEVICE) return fail(h, KDF_ERR_INVALID, "%s: mem = %d (0 host, 1 device)", fn, mem);
    if (n_bytes > (1ull << 31)) return fail(h, KDF_ERR_INVALID, "%s: a chunk of %llu bytes is beyond the 2^31 a call takes", fn, (unsigned long long)n_bytes);
    if (n_reads && !keep) return fail(h, KDF_ERR_INVALID, "%s: NULL keep for %llu records", fn, (unsigned long long)n_reads);
    if (n_bytes == 0) {                                                // no records
        if (n_reads) return fail(h, KDF_ERR_INVALID, "%s: the chunk holds 0 records, keep has %llu flags", fn, (unsigned long long)n_reads);
        return KDF_OK;
    }
    if (!text || (!out && cap_out)) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    cap_out = std::min(cap_out, n_bytes + 2);                          // (no output needs more)
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    HostCall c(h, fn);
    int oo = -1, of = -1;
    if (mem == KDF_MEM_DEVICE) {
        if ((rc = fx_core(h, text, n_bytes, final_chunk, keep, n_reads, out, cap_out, out_offsets))) return rc;
    } else {
        const int it = c.in(text, (size_t)n_bytes), ik = c.in(keep, (size_t)n_reads);
        oo = c.out(out, (size_t)cap_out); of = c.out(out_offsets, out_offsets ? (size_t)(n_reads + 1) * 8 : 0);
        if ((rc = c.commit()) || (rc = fx_core(h, c.dev(it), n_bytes, final_chunk, c.dev(ik), n_reads, c.dev(oo), cap_out, c.dev(of)))) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));                       // (the caller learns the sizes and a possible error)
    const uint64_t ob = h->h_out4[0], nk = h->h_out4[1] & 0xFFFFFFFFull, nr = h->h_out4[1] >> 32, m = h->h_out4[2], verdict = h->h_out4[3] & 0xFFu,
                   bad = h->h_out4[3] >> 8;
    if (verdict == KFQ_ERR_FORMAT) {
        const uint32_t rule = (uint32_t)(bad & 7u);
        if (bad_offset) *bad_offset = bad >> 3;
        if (bad_rule) *bad_rule = rule;
        return fail(h, KDF_ERR_IO, "%s: the record at offset %llu of the chunk is no FASTQ record: %s", fn, (unsigned long long)(bad >> 3), fq_rule_text[rule <= 4 ? rule : 0]);
    }
    if (verdict == KFX_ERR_COUNT)
        return fail(h, KDF_ERR_INVALID, "%s: the chunk holds %llu records, keep has %llu flags", fn, (unsigned long long)nr, (unsigned long long)n_reads);
    if (verdict == KFQ_ERR_ROOM)
        return fail(h, KDF_ERR_INVALID, "%s: the %llu kept records take %llu bytes, the output holds %llu", fn, (unsigned long long)nk, (unsigned long long)ob,
                    (unsigned long long)cap_out);
    if (verdict == KFQ_NOTHING) return KDF_OK;
    if (mem == KDF_MEM_HOST && ((rc = c.fetch(oo, (size_t)ob)) || (rc = c.fetch(of, out_offsets ? (size_t)(nk + 1) * 8 : 0)) || (rc = c.finish()))) return rc;
    *out_bytes = ob; *n_kept = nk; *consumed = m;
    return KDF_OK;
}

}  // extern "C"
