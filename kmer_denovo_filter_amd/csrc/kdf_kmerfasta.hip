// kdf_kmerfasta.hip -- libkdf.so, the k-mer FASTA codec (kdf_kmerfasta.h): the closed form of the text's size, the
// format and parse entry points and their host forms.  The table is not touched; what this unit uses of the engine is
// declared in kdf_engine_priv.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>

#include "kdf_engine_priv.h"
#include "kdf_kmerfasta.h"

// words per key of the codec's key form for k: 1 (lo), 2 (lo, hi), W of the rows; 0: no form takes k
static int kf_words(int k) {
    if (k >= 1 && k <= 32) return 1;
    if (k >= 33 && k <= 63) return 2;
    if (k >= 65 && k <= 201 && (k & 1)) return (2 * k + 63) / 64;
    return 0;
}

template <typename F>
static int kf_by_words(int W, F &&f) {
    switch (W) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 7>{});
    }
}

// The digit classes of records first_index .. first_index + n - 1 and the text's size; false: bad k / layout, or the
// indices or the size pass 2^63.  Pure host arithmetic.
static bool kf_plan(int k, int layout, uint64_t first_index, uint64_t n, KfPlan &p, uint64_t &text_bytes) {
    static const uint64_t LIMIT = 1ull << 63;
    const int W = kf_words(k);
    if (!W || (layout != KDF_TEXT_FASTA && layout != KDF_TEXT_ROWS)) return false;
    p = KfPlan{};
    p.k = k; p.words = W; p.n = n; p.first_index = layout == KDF_TEXT_FASTA ? first_index : 0;
    auto magic = [](uint32_t len) { return len == 1 ? 0ull : ~0ull / len + 1; };   // ceil(2^64 / len): len = 2^j divides exactly, else floor + 1
    unsigned __int128 bytes = 0;
    uint32_t len_min = (uint32_t)k;
    if (layout == KDF_TEXT_ROWS) {
        if (n > LIMIT) return false;
        bytes = (unsigned __int128)n * (unsigned)k;
        if (n) { p.ncls = 1; p.cls_magic[0] = magic((uint32_t)k); }
    } else {
        if (first_index > LIMIT || n > LIMIT - first_index) return false;
        uint64_t p10 = 10;                                            // 10^d, d <= 19: the indices stay below 2^63 < 10^19
        int d = 1;
        while (first_index >= p10) { p10 *= 10; ++d; }
        p.d0 = d;
        len_min = (uint32_t)(d + k + 3);
        const uint64_t end = first_index + n;
        for (uint64_t cur = first_index; cur < end; ++d, p10 *= 10) {
            const uint64_t stop = std::min(end, p10);
            const uint32_t len = (uint32_t)(d + k + 3);
            p.cls_byte[p.ncls] = (uint64_t)bytes; p.cls_rec[p.ncls] = cur - first_index; p.cls_magic[p.ncls] = magic(len);
            ++p.ncls;
            bytes += (unsigned __int128)(stop - cur) * len;
            if (bytes > LIMIT) return false;
            cur = stop;
        }
    }
    if (bytes > LIMIT) return false;
    p.cls_byte[p.ncls] = text_bytes = (uint64_t)bytes;
    p.key_rows = KF_TILE_BYTES / len_min + 2;
    return true;
}

extern "C" {

uint64_t kdf_kmer_text_bytes(int k, int layout, uint64_t first_index, uint64_t n) {
    KfPlan p;
    uint64_t bytes = 0;
    return kf_plan(k, layout, first_index, n, p, bytes) ? bytes : 0;
}

int kdf_format_kmers_dev(kdf_engine *h, const void *d_lo, const void *d_hi, uint64_t n, int k, int layout, uint64_t first_index,
                         uint64_t byte_first, uint64_t byte_count, void *d_text_out) {
    static const char *const fn = "kdf_format_kmers_dev";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    KfPlan p;
    uint64_t text_bytes = 0;
    if (!kf_plan(k, layout, first_index, n, p, text_bytes))
        return fail(h, KDF_ERR_INVALID, "%s: k = %d (1 .. 63 or odd 65 .. 201), layout = %d (0 FASTA, 1 rows), or records %llu + %llu and their "
                    "text pass 2^63", fn, k, layout, (unsigned long long)first_index, (unsigned long long)n);
    if (byte_first % 16) return fail(h, KDF_ERR_INVALID, "%s: byte_first = %llu is no multiple of 16", fn, (unsigned long long)byte_first);
    if (byte_first > text_bytes || byte_count > text_bytes - byte_first)
        return fail(h, KDF_ERR_INVALID, "%s: window [%llu, +%llu) passes the text's %llu bytes", fn, (unsigned long long)byte_first,
                    (unsigned long long)byte_count, (unsigned long long)text_bytes);
    if (byte_count == 0 || n == 0) return KDF_OK;
    if (!d_lo || (p.words == 2 && !d_hi) || !d_text_out) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    const uint64_t blocks = (byte_count + KF_TILE_BYTES - 1) / KF_TILE_BYTES;
    if (blocks >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "%s: a window of %llu bytes is beyond the 2^43 a call takes", fn, (unsigned long long)byte_count);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t lds = (size_t)p.key_rows * (size_t)p.words * 8;      // <= 4098 keys of one word (rows of k = 1)
    const int aligned = ((uintptr_t)d_text_out & 15) == 0;
    const int form = p.words <= 2 ? p.words - 1 : 2;
    const uint64_t *lo = (const uint64_t *)d_lo, *hi = (const uint64_t *)d_hi;
    EvSpan span(h->timer[T_KF], h->prof, h->stream, 1);
#define KF_LAUNCH(FORM, FASTA) \
    hipLaunchKernelGGL((kf_format_kernel<FORM, FASTA>), dim3((unsigned)blocks), dim3(256), lds, h->stream, p, lo, hi, byte_first, byte_count, (uint8_t *)d_text_out, aligned)
    if (layout == KDF_TEXT_FASTA) { if (form == 0) KF_LAUNCH(0, true); else if (form == 1) KF_LAUNCH(1, true); else KF_LAUNCH(2, true); }
    else { if (form == 0) KF_LAUNCH(0, false); else if (form == 1) KF_LAUNCH(1, false); else KF_LAUNCH(2, false); }
#undef KF_LAUNCH
    span.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

int kdf_format_kmers(kdf_engine *h, const uint64_t *lo, const uint64_t *hi, uint64_t n, int k, int layout, uint64_t first_index,
                     uint64_t byte_first, uint64_t byte_count, uint8_t *text_out) {
    static const char *const fn = "kdf_format_kmers";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    const int W = kf_words(k);
    if (W && byte_count && n && (!lo || (W == 2 && !hi) || !text_out)) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    HIPCHK(h, hipSetDevice(h->device));
    const bool work = W && byte_count && n;                           // (the refusals are the device form's, with nothing staged)
    HostCall c(h, fn);
    const int il = c.in(lo, work ? (size_t)n * 8 * (W == 2 ? 1 : W) : 0), ih = c.in(hi, work && W == 2 ? (size_t)n * 8 : 0);
    const int io = c.out(text_out, work ? (size_t)byte_count : 0);
    int rc;
    if ((rc = c.commit()) || (rc = kdf_format_kmers_dev(h, c.dev(il), c.dev(ih), n, k, layout, first_index, byte_first, byte_count, c.dev(io))) ||
        (rc = c.fetch(io, work ? (size_t)byte_count : 0))) return rc;
    return c.finish();
}

int kdf_parse_kmer_fasta_dev(kdf_engine *h, const void *d_text, uint64_t n_bytes, int k, int canonical, int final_chunk, void *d_lo, void *d_hi,
                             uint64_t cap, uint64_t *n_out, uint64_t *consumed_out, uint64_t *bad_offset_out) {
    static const char *const fn = "kdf_parse_kmer_fasta_dev";
    if (!h || !n_out || !consumed_out) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    *n_out = 0; *consumed_out = 0;
    if (bad_offset_out) *bad_offset_out = ~0ull;
    const int W = kf_words(k);
    if (!W) return fail(h, KDF_ERR_INVALID, "%s: k = %d outside 1 .. 63 and odd 65 .. 201", fn, k);
    if (cap && (!d_lo || (W == 2 && !d_hi))) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    if (n_bytes == 0) return KDF_OK;
    if (!d_text) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    const uint64_t nb = (n_bytes + KF_TILE_BYTES - 1) / KF_TILE_BYTES;
    if (nb >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "%s: a chunk of %llu bytes is beyond the 2^43 a call takes", fn, (unsigned long long)n_bytes);
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = eng_reserve(h, h->kf.block_sums, (nb + 4) * 8, slack_8th, "block sums"))) return rc;
    unsigned long long *sums = h->kf.block_sums.as<unsigned long long>(), *ctl = sums + nb + 1;   // sums[nb]: the total; then ctl[3]
    const uint8_t *t = (const uint8_t *)d_text;
    EvSpan span(h->timer[T_KF], h->prof, h->stream, 1);
    hipLaunchKernelGGL(kf_ctl_init_kernel, dim3(1), dim3(1), 0, h->stream, ctl);
    hipLaunchKernelGGL(kf_count_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, t, n_bytes, final_chunk, sums, ctl);
    kh_scan_launch(h->stream, sums, nb);
    kf_by_words(W, [&](auto Wc) {
        constexpr int KW = decltype(Wc)::value;
        hipLaunchKernelGGL(kf_parse_kernel<KW>, dim3((unsigned)nb), dim3(256), 0, h->stream, t, n_bytes, final_chunk, k, canonical,
                           (const unsigned long long *)sums, ctl, (uint64_t *)d_lo, (uint64_t *)d_hi, cap);
        return 0;
    });
    span.stop();
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->h_out4, sums + nb, 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                       // (the caller learns the number of keys)
    const uint64_t total = h->h_out4[0], bad = h->h_out4[1], behind_nl = h->h_out4[2], tail = h->h_out4[3];
    *n_out = total - (tail ? 1 : 0);
    *consumed_out = final_chunk ? n_bytes : behind_nl;
    if (bad != ~0ull) {
        if (bad_offset_out) *bad_offset_out = bad >> 1;
        if (bad & 1) return fail(h, KDF_ERR_IO, "%s: non-ACGT base in the sequence line at byte %llu", fn, (unsigned long long)(bad >> 1));
        return fail(h, KDF_ERR_IO, "%s: sequence line of length != k=%d at byte %llu", fn, k, (unsigned long long)(bad >> 1));
    }
    if (*n_out > cap) return fail(h, KDF_ERR_INVALID, "%s: %llu keys, the buffer holds %llu", fn, (unsigned long long)*n_out, (unsigned long long)cap);
    return KDF_OK;
}

int kdf_parse_kmer_fasta(kdf_engine *h, const uint8_t *text, uint64_t n_bytes, int k, int canonical, int final_chunk, uint64_t *lo, uint64_t *hi,
                         uint64_t cap, uint64_t *n_out, uint64_t *consumed_out, uint64_t *bad_offset_out) {
    static const char *const fn = "kdf_parse_kmer_fasta";
    if (!h || !n_out || !consumed_out) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    *n_out = 0; *consumed_out = 0;
    if (bad_offset_out) *bad_offset_out = ~0ull;
    const int W = kf_words(k);
    if (!W) return fail(h, KDF_ERR_INVALID, "%s: k = %d outside 1 .. 63 and odd 65 .. 201", fn, k);
    if ((cap && (!lo || (W == 2 && !hi))) || (n_bytes && !text)) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    if (n_bytes == 0) return KDF_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t lo_row = 8 * (size_t)(W == 2 ? 1 : W);
    HostCall c(h, fn);
    const int it = c.in(text, (size_t)n_bytes), il = c.out(lo, (size_t)cap * lo_row), ih = c.out(hi, W == 2 ? (size_t)cap * 8 : 0);
    int rc;
    if ((rc = c.commit())) return rc;
    const int rcl = kdf_parse_kmer_fasta_dev(h, c.dev(it), n_bytes, k, canonical, final_chunk, c.dev(il), c.dev(ih), cap, n_out, consumed_out, bad_offset_out);
    if (rcl && !(rcl == KDF_ERR_INVALID && *n_out > cap)) return rcl;
    const size_t rows = (size_t)std::min<uint64_t>(*n_out, cap);
    if ((rc = c.fetch(il, rows * lo_row)) || (rc = c.fetch(ih, W == 2 ? rows * 8 : 0)) || (rc = c.finish())) return rc;
    return rcl;
}

}  // extern "C"
