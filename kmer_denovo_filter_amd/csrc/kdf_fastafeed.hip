// kdf_fastafeed.hip -- libkdf.so, the device FASTA feeder (kdf_fastafeed.h): kdf_fasta_pack_dev and its host form.
// The table is not touched and nothing is flushed; what this unit uses of the engine is declared in kdf_engine_priv.h.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "kdf_engine_priv.h"
#include "kdf_fastafeed.h"

// the positions of the previous stream a call copies in front of its slice
static uint64_t kfa_carry(const kdf_fasta_state *st, const void *prev_packed, const void *prev_invalid, uint64_t prev_n, uint32_t carry) {
    if (!carry || !prev_n || !prev_packed || !prev_invalid || !(st->flags & KDF_FA_IN_RECORD)) return 0;
    return std::min<uint64_t>(carry, prev_n);
}

extern "C" {

int kdf_fasta_pack_dev(kdf_engine *h, const void *d_text, uint64_t n_bytes, int final_chunk, kdf_fasta_state *state,
                       const void *d_prev_packed, const void *d_prev_invalid, uint64_t prev_n_bases, uint32_t carry,
                       void *d_packed, void *d_invalid, uint64_t cap_bases, void *d_offsets, uint64_t cap_reads,
                       uint64_t *n_bases, uint64_t *n_reads, uint64_t *consumed) {
    static const char *const fn = "kdf_fasta_pack_dev";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "%s: NULL engine", fn);
    if (!state || !n_bases || !n_reads || !consumed) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    *n_bases = 0; *n_reads = 0; *consumed = 0;
    if (state->flags & ~(KDF_FA_IN_RECORD | KDF_FA_MID_LINE | KDF_FA_IN_HEADER))
        return fail(h, KDF_ERR_INVALID, "%s: state flags %#x (zero the state before the first chunk)", fn, state->flags);
    if (n_bytes == 0 && !final_chunk) return KDF_OK;
    if ((n_bytes && !d_text) || !d_packed || !d_invalid) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    if ((d_prev_packed && d_prev_packed == d_packed) || (d_prev_invalid && d_prev_invalid == d_invalid))
        return fail(h, KDF_ERR_INVALID, "%s: the previous stream and the output are the same buffers", fn);
    if (n_bytes > (1ull << 31)) return fail(h, KDF_ERR_INVALID, "%s: a chunk of %llu bytes is beyond the 2^31 a call takes", fn, (unsigned long long)n_bytes);
    const uint32_t flags = (state->flags & KDF_FA_MID_LINE) ? state->flags : state->flags & KDF_FA_IN_RECORD;
    const uint64_t c = kfa_carry(state, d_prev_packed, d_prev_invalid, prev_n_bases, carry);
    const uint64_t nt = (n_bytes + KFA_TILE - 1) / KFA_TILE;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = eng_reserve(h, h->fa.scratch, (3 * nt + KFA_CTL_WORDS) * 8, slack_8th, "FASTA feeder scratch"))) return rc;
    unsigned long long *sums = h->fa.scratch.as<unsigned long long>(), *tile_pos = sums + nt, *tile_rec = tile_pos + nt, *ctl = tile_rec + nt;
    const uint8_t *t = (const uint8_t *)d_text;
    const int aligned = ((uintptr_t)d_text & 15) == 0;
    uint64_t pw_max, mw_max;
    kdf_stream_words(std::min(cap_bases, n_bytes + c + 1), &pw_max, &mw_max);
    EvSpan span(h->timer[T_FA], h->prof, h->stream, 1);
    if (nt) hipLaunchKernelGGL(kfa_count_kernel, dim3((unsigned)nt), dim3(256), 0, h->stream, t, n_bytes, flags, aligned, sums);
    hipLaunchKernelGGL(kfa_scan_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned long long *)sums, nt, t, n_bytes, final_chunk, flags, c,
                       cap_bases, d_offsets ? cap_reads : ~0ull, tile_pos, tile_rec, ctl);
    hipLaunchKernelGGL(kfa_zero_kernel, dim3((unsigned)std::min<uint64_t>((pw_max + 255) / 256, 4096)), dim3(256), 0, h->stream,
                       (const unsigned long long *)ctl, (uint64_t *)d_packed, (uint64_t *)d_invalid);
    if (nt) hipLaunchKernelGGL(kfa_write_kernel, dim3((unsigned)nt), dim3(256), 0, h->stream, t, n_bytes, flags, aligned, (const unsigned long long *)tile_pos,
                               (const unsigned long long *)tile_rec, (const unsigned long long *)ctl, (uint64_t *)d_packed, (uint64_t *)d_invalid, (int64_t *)d_offsets);
    hipLaunchKernelGGL(kfa_tail_kernel, dim3(1), dim3(256), 0, h->stream, (const unsigned long long *)ctl, (const uint64_t *)d_prev_packed,
                       (const uint64_t *)d_prev_invalid, prev_n_bases, c, (uint64_t *)d_packed, (uint64_t *)d_invalid, (int64_t *)d_offsets);
    span.stop();
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->h_out4, ctl, KFA_CTL_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                       // (the caller learns the sizes)
    const uint64_t nb = h->h_out4[0], nr = h->h_out4[1], m = h->h_out4[2], verdict = h->h_out4[3];
    const uint32_t err = (uint32_t)(verdict >> 8) & 0xFFu;
    if (err == KFA_ERR_ROOM)
        return fail(h, KDF_ERR_INVALID, "%s: the chunk packs to %llu positions in %llu records, the buffers hold %llu and %llu", fn, (unsigned long long)nb,
                    (unsigned long long)nr, (unsigned long long)cap_bases, (unsigned long long)(d_offsets ? cap_reads : nr));
    if (err == KFA_ERR_STUCK)
        return fail(h, KDF_ERR_INVALID, "%s: a chunk of %llu '\\r' that is not the last: nothing can be consumed", fn, (unsigned long long)n_bytes);
    const uint64_t piece = (state->flags & KDF_FA_IN_RECORD) ? 1 : 0;
    state->flags = (uint32_t)verdict & 0xFFu;
    state->records += nr - piece;
    state->positions += nb - c;
    *n_bases = nb; *n_reads = nr; *consumed = m;
    return KDF_OK;
}

int kdf_fasta_pack(kdf_engine *h, const uint8_t *text, uint64_t n_bytes, int final_chunk, kdf_fasta_state *state,
                   const uint64_t *prev_packed, const uint64_t *prev_invalid, uint64_t prev_n_bases, uint32_t carry,
                   uint64_t *packed, uint64_t *invalid, uint64_t cap_bases, int64_t *offsets, uint64_t cap_reads,
                   uint64_t *n_bases, uint64_t *n_reads, uint64_t *consumed) {
    static const char *const fn = "kdf_fasta_pack";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "%s: NULL engine", fn);
    if (!state || !n_bases || !n_reads || !consumed) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    *n_bases = 0; *n_reads = 0; *consumed = 0;
    if (n_bytes == 0 && !final_chunk) return KDF_OK;
    if ((n_bytes && !text) || !packed || !invalid) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    if ((prev_packed && prev_packed == packed) || (prev_invalid && prev_invalid == invalid))
        return fail(h, KDF_ERR_INVALID, "%s: the previous stream and the output are the same buffers", fn);
    HIPCHK(h, hipSetDevice(h->device));
    const bool prev = prev_packed && prev_invalid && prev_n_bases && carry;
    uint64_t pw, mw;
    kdf_stream_words(cap_bases, &pw, &mw);
    if (!offsets) cap_reads = 0;
    HostCall c(h, fn);
    const int it = c.in(text, (size_t)n_bytes);
    const int ip = prev ? c.stream(prev_packed, prev_invalid, prev_n_bases) : -1;
    const int op = c.out(packed, (size_t)pw * 8), om = c.out(invalid, (size_t)mw * 8), oo = c.out(offsets, offsets ? (size_t)(cap_reads + 1) * 8 : 0);
    int rc;
    if ((rc = c.commit()) ||
        (rc = kdf_fasta_pack_dev(h, c.dev(it), n_bytes, final_chunk, state, prev ? c.dev(ip) : nullptr, prev ? c.dev(ip + 1) : nullptr, prev_n_bases, carry,
                                 c.dev(op), c.dev(om), cap_bases, c.dev(oo), cap_reads, n_bases, n_reads, consumed)))
        return rc;
    kdf_stream_words(*n_bases, &pw, &mw);
    if ((rc = c.fetch(op, (size_t)pw * 8)) || (rc = c.fetch(om, (size_t)mw * 8)) || (rc = c.fetch(oo, offsets ? (size_t)(*n_reads + 1) * 8 : 0))) return rc;
    return c.finish();
}

}  // extern "C"
