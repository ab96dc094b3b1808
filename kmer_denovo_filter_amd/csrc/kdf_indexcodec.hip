// kdf_indexcodec.hip -- libkdf.so, the index record codec (kdf_indexcodec.h): the record size, encode, decode, the
// Jellyfish hash positions and the binary/sorted order.  Each entry point is one function with a `mem` argument: host
// arrays are staged through the engine's staging frame, device arrays are used in place.  The table is not touched;
// what this unit uses of the engine is declared in kdf_engine_priv.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>

#include "kdf_engine_priv.h"
#include "kdf_indexcodec.h"
#include "kdf_sort.h"

// words per key of the codec's key form for k: 1 (lo), 2 (lo, hi), W of the rows; 0: no form takes k
static int ix_words(int k) {
    if (k >= 1 && k <= 32) return 1;
    if (k >= 33 && k <= 63) return 2;
    if (k >= 65 && k <= 201 && (k & 1)) return (2 * k + 63) / 64;
    return 0;
}
static int ix_key_bytes(int k) { return (2 * k + 7) / 8; }
static bool ix_mem_ok(int mem) { return mem == KDF_MEM_HOST || mem == KDF_MEM_DEVICE; }

// ---- the device cores: every array argument is a device pointer ------------------------------------------------------

static int ix_encode_core(kdf_engine *h, const char *fn, const void *d_lo, const void *d_hi, const void *d_counts, const void *d_perm, uint64_t n,
                          int k, uint64_t byte_first, uint64_t byte_count, void *d_bytes) {
    const int W = ix_words(k);
    IxEncPlan p{};
    p.words = W; p.kb = ix_key_bytes(k); p.rec = (uint32_t)p.kb + 4; p.key_rows = IX_TILE_BYTES / p.rec + 2;
    p.magic = ~0ull / p.rec + 1;                                      // ceil(2^64 / R): R = 2^j (8, 16, 32) divides exactly, else floor + 1
    p.n = n;
    const uint64_t blocks = (byte_count + IX_TILE_BYTES - 1) / IX_TILE_BYTES;
    if (blocks >= (1ull << 31)) return fail(h, KDF_ERR_INVALID, "%s: a window of %llu bytes is beyond the 2^43 a call takes", fn, (unsigned long long)byte_count);
    const size_t lds = (size_t)p.key_rows * ((size_t)W * 8 + 4);      // <= 821 records of one word and a count (k <= 4)
    const int aligned = ((uintptr_t)d_bytes & 15) == 0;
    const int form = W <= 2 ? W - 1 : 2;
    const uint64_t *lo = (const uint64_t *)d_lo, *hi = (const uint64_t *)d_hi;
    EvSpan span(h->timer[T_IX], h->prof, h->stream, 1);
#define IX_LAUNCH(FORM) \
    hipLaunchKernelGGL((ix_encode_kernel<FORM>), dim3((unsigned)blocks), dim3(256), lds, h->stream, p, lo, hi, (const uint32_t *)d_counts, \
                       (const uint32_t *)d_perm, byte_first, byte_count, (uint8_t *)d_bytes, aligned)
    if (form == 0) IX_LAUNCH(0); else if (form == 1) IX_LAUNCH(1); else IX_LAUNCH(2);
#undef IX_LAUNCH
    span.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

// launches the decode and queues the copy of the first bad record's index to h->h_out4[0]; the caller synchronises
static int ix_decode_core(kdf_engine *h, const void *d_bytes, uint64_t n, int k, int counter_len, void *d_lo, void *d_hi, void *d_counts) {
    const int W = ix_words(k), kb = ix_key_bytes(k);
    int rc;
    if ((rc = eng_reserve(h, h->ix.ctl, 8, slack_8th, "first bad record"))) return rc;
    unsigned long long *first_bad = h->ix.ctl.as<unsigned long long>();
    HIPCHK(h, hipMemsetAsync(first_bad, 0xFF, 8, h->stream));
    const unsigned blocks = (unsigned)((n + IX_DEC_RECORDS - 1) / IX_DEC_RECORDS);
    EvSpan span(h->timer[T_IX], h->prof, h->stream, 1);
#define IX_LAUNCH(KW) \
    hipLaunchKernelGGL((ix_decode_kernel<KW>), dim3(blocks), dim3(256), ix_decode_lds(KW, (uint32_t)(kb + counter_len)), h->stream, (const uint8_t *)d_bytes, \
                       n, k, kb, counter_len, (uint64_t *)d_lo, (uint64_t *)d_hi, (uint32_t *)d_counts, first_bad)
    switch (W) {
    case 1: IX_LAUNCH(1); break;
    case 2: IX_LAUNCH(2); break;
    case 3: IX_LAUNCH(3); break;
    case 4: IX_LAUNCH(4); break;
    case 5: IX_LAUNCH(5); break;
    case 6: IX_LAUNCH(6); break;
    default: IX_LAUNCH(7); break;
    }
#undef IX_LAUNCH
    span.stop();
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->h_out4, first_bad, 8, hipMemcpyDeviceToHost, h->stream));
    return KDF_OK;
}

static int ix_positions_core(kdf_engine *h, const void *d_lo, const void *d_hi, uint64_t n, int k, const uint64_t *columns, uint64_t size, void *d_pos) {
    IxColumns cols{};
    for (int b = 0; b < 2 * k; ++b) cols.bit[b] = columns[2 * k - 1 - b] & (size - 1);
    const int kb = ix_key_bytes(k);
    const unsigned blocks = (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)std::max(h->n_cu, 1) * 4);
    EvSpan span(h->timer[T_IX], h->prof, h->stream, 1);
    if (k <= 32)
        hipLaunchKernelGGL((ix_positions_kernel<0>), dim3(blocks), dim3(256), (size_t)kb * 2048, h->stream, cols, kb, (const uint64_t *)d_lo,
                           (const uint64_t *)d_hi, n, (uint64_t *)d_pos);
    else
        hipLaunchKernelGGL((ix_positions_kernel<1>), dim3(blocks), dim3(256), (size_t)kb * 2048, h->stream, cols, kb, (const uint64_t *)d_lo,
                           (const uint64_t *)d_hi, n, (uint64_t *)d_pos);
    span.stop();
    HIPCHK(h, hipGetLastError());
    return KDF_OK;
}

// the refusals kdf_jf_positions and kdf_jf_order share; KDF_OK: k is 1 .. 63 and size a power of two
static int ix_jf_refuse(kdf_engine *h, const char *fn, int mem, int k, const uint64_t *columns, uint64_t size) {
    if (!ix_mem_ok(mem)) return fail(h, KDF_ERR_INVALID, "%s: mem = %d (0 host, 1 device)", fn, mem);
    if (k < 1 || k > 63) return fail(h, KDF_ERR_INVALID, "%s: k = %d outside 1 .. 63 (Jellyfish's binary/sorted order)", fn, k);
    if (!size || (size & (size - 1))) return fail(h, KDF_ERR_INVALID, "%s: size = %llu is no power of two", fn, (unsigned long long)size);
    if (!columns) return fail(h, KDF_ERR_INVALID, "%s: NULL columns", fn);
    return KDF_OK;
}

extern "C" {

uint64_t kdf_index_record_bytes(int k, int counter_len) {
    if (!ix_words(k) || counter_len < 1 || counter_len > 16) return 0;
    return (uint64_t)ix_key_bytes(k) + (uint64_t)counter_len;
}

int kdf_index_encode(kdf_engine *h, int mem, const void *lo, const void *hi, const void *counts, const void *perm, uint64_t n, int k,
                     uint64_t byte_first, uint64_t byte_count, void *bytes_out) {
    static const char *const fn = "kdf_index_encode";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (!ix_mem_ok(mem)) return fail(h, KDF_ERR_INVALID, "%s: mem = %d (0 host, 1 device)", fn, mem);
    const int W = ix_words(k);
    if (!W) return fail(h, KDF_ERR_INVALID, "%s: k = %d outside 1 .. 63 and odd 65 .. 201", fn, k);
    const uint64_t R = kdf_index_record_bytes(k, 4);
    if (n > ((1ull << 63) - 1) / R) return fail(h, KDF_ERR_INVALID, "%s: %llu records of %llu bytes pass 2^63", fn, (unsigned long long)n, (unsigned long long)R);
    if (perm && n >= (1ull << 32)) return fail(h, KDF_ERR_INVALID, "%s: %llu records are beyond the 2^32 - 1 a permutation takes", fn, (unsigned long long)n);
    if (byte_first % 16) return fail(h, KDF_ERR_INVALID, "%s: byte_first = %llu is no multiple of 16", fn, (unsigned long long)byte_first);
    const uint64_t body = n * R;
    if (byte_first > body || byte_count > body - byte_first)
        return fail(h, KDF_ERR_INVALID, "%s: window [%llu, +%llu) passes the body's %llu bytes", fn, (unsigned long long)byte_first,
                    (unsigned long long)byte_count, (unsigned long long)body);
    if (byte_count == 0 || n == 0) return KDF_OK;
    if (!lo || (W == 2 && !hi) || !bytes_out) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    HIPCHK(h, hipSetDevice(h->device));
    if (mem == KDF_MEM_DEVICE) return ix_encode_core(h, fn, lo, hi, counts, perm, n, k, byte_first, byte_count, bytes_out);
    HostCall c(h, fn);
    const int il = c.in(lo, (size_t)n * 8 * (W == 2 ? 1 : W)), ih = c.in(hi, W == 2 ? (size_t)n * 8 : 0);
    const int ic = c.in(counts, counts ? (size_t)n * 4 : 0), ip = c.in(perm, perm ? (size_t)n * 4 : 0);
    const int io = c.out(bytes_out, (size_t)byte_count);
    int rc;
    if ((rc = c.commit()) || (rc = ix_encode_core(h, fn, c.dev(il), c.dev(ih), c.dev(ic), c.dev(ip), n, k, byte_first, byte_count, c.dev(io))) ||
        (rc = c.fetch(io, (size_t)byte_count))) return rc;
    return c.finish();
}

int kdf_index_decode(kdf_engine *h, int mem, const void *bytes, uint64_t n, int k, int counter_len, void *lo, void *hi, void *counts,
                     uint64_t *bad_record_out) {
    static const char *const fn = "kdf_index_decode";
    if (bad_record_out) *bad_record_out = ~0ull;
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (!ix_mem_ok(mem)) return fail(h, KDF_ERR_INVALID, "%s: mem = %d (0 host, 1 device)", fn, mem);
    const int W = ix_words(k);
    const uint64_t rd = kdf_index_record_bytes(k, counter_len);
    if (!rd) return fail(h, KDF_ERR_INVALID, "%s: k = %d (1 .. 63 or odd 65 .. 201) or counter_len = %d (1 .. 16)", fn, k, counter_len);
    if (n >= (1ull << 31) * IX_DEC_RECORDS) return fail(h, KDF_ERR_INVALID, "%s: %llu records are beyond the 2^39 a call takes", fn, (unsigned long long)n);
    if (n == 0) return KDF_OK;
    if (!bytes || !lo || (W == 2 && !hi)) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if (mem == KDF_MEM_DEVICE) {
        if ((rc = ix_decode_core(h, bytes, n, k, counter_len, lo, hi, counts))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));                   // (the caller learns the bad record)
    } else {
        const size_t lo_row = 8 * (size_t)(W == 2 ? 1 : W);
        HostCall c(h, fn);
        const int ib = c.in(bytes, (size_t)(n * rd)), il = c.out(lo, (size_t)n * lo_row), ih = c.out(hi, hi && W <= 2 ? (size_t)n * 8 : 0);
        const int ic = c.out(counts, counts ? (size_t)n * 4 : 0);
        if ((rc = c.commit()) || (rc = ix_decode_core(h, c.dev(ib), n, k, counter_len, c.dev(il), c.dev(ih), c.dev(ic))) ||
            (rc = c.fetch(il, (size_t)n * lo_row)) || (rc = c.fetch(ih, hi && W <= 2 ? (size_t)n * 8 : 0)) || (rc = c.fetch(ic, counts ? (size_t)n * 4 : 0)) ||
            (rc = c.finish())) return rc;
    }
    const uint64_t bad = h->h_out4[0];
    if (bad != ~0ull) {
        if (bad_record_out) *bad_record_out = bad;
        return fail(h, KDF_ERR_IO, "%s: record %llu holds a key with a bit at or above 2k = %d", fn, (unsigned long long)bad, 2 * k);
    }
    return KDF_OK;
}

int kdf_jf_positions(kdf_engine *h, int mem, const void *lo, const void *hi, uint64_t n, int k, const uint64_t *columns, uint64_t size, void *pos_out) {
    static const char *const fn = "kdf_jf_positions";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (const int rc = ix_jf_refuse(h, fn, mem, k, columns, size)) return rc;
    if (n == 0) return KDF_OK;
    if (!lo || (k > 32 && !hi) || !pos_out) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    HIPCHK(h, hipSetDevice(h->device));
    if (mem == KDF_MEM_DEVICE) return ix_positions_core(h, lo, hi, n, k, columns, size, pos_out);
    HostCall c(h, fn);
    const int il = c.in(lo, (size_t)n * 8), ih = c.in(hi, k > 32 ? (size_t)n * 8 : 0), io = c.out(pos_out, (size_t)n * 8);
    int rc;
    if ((rc = c.commit()) || (rc = ix_positions_core(h, c.dev(il), c.dev(ih), n, k, columns, size, c.dev(io))) || (rc = c.fetch(io, (size_t)n * 8))) return rc;
    return c.finish();
}

int kdf_jf_order(kdf_engine *h, int mem, const void *lo, const void *hi, uint64_t n, int k, const uint64_t *columns, uint64_t size, void *perm_out) {
    static const char *const fn = "kdf_jf_order";
    if (!h) return fail(nullptr, KDF_ERR_INVALID, "NULL engine");
    if (const int rc = ix_jf_refuse(h, fn, mem, k, columns, size)) return rc;
    if (n >= (1ull << 32)) return fail(h, KDF_ERR_INVALID, "%s: %llu keys are beyond the 2^32 - 1 a call takes", fn, (unsigned long long)n);
    if (n == 0) return KDF_OK;
    if (!lo || (k > 32 && !hi) || !perm_out) return fail(h, KDF_ERR_INVALID, "%s: NULL pointer", fn);
    HIPCHK(h, hipSetDevice(h->device));
    // positions, then the library sort: the key words as the low passes, the position on top
    auto order = [&](const void *d_lo, const void *d_hi, void *d_perm) -> int {
        int rc;
        if ((rc = eng_reserve(h, h->ix.pos, n * 8, slack_8th, "hash positions"))) return rc;
        uint64_t *pos = h->ix.pos.as<uint64_t>();
        if ((rc = ix_positions_core(h, d_lo, d_hi, n, k, columns, size, pos))) return rc;
        KdfSortPass passes[3];
        int np = 0;
        passes[np++] = KdfSortPass{(const uint64_t *)d_lo, 1, 0, std::min(2 * k, 64)};
        if (k > 32) passes[np++] = KdfSortPass{(const uint64_t *)d_hi, 1, 0, 2 * k - 64};
        passes[np++] = KdfSortPass{pos, 1, 0, (int)std::max<uint32_t>(1, log2ceil(size))};
        std::string serr;
        EvSpan span(h->timer[T_IX], h->prof, h->stream, 0);
        if (kdf_sort_perm_device(passes, np, n, (uint32_t *)d_perm, h->stream, serr)) return fail(h, KDF_ERR_HIP, "%s: sort failed: %s", fn, serr.c_str());
        span.stop();
        return KDF_OK;
    };
    if (mem == KDF_MEM_DEVICE) {
        if (const int rc = order(lo, hi, perm_out)) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return KDF_OK;
    }
    HostCall c(h, fn);
    const int il = c.in(lo, (size_t)n * 8), ih = c.in(hi, k > 32 ? (size_t)n * 8 : 0), io = c.out(perm_out, (size_t)n * 4);
    int rc;
    if ((rc = c.commit()) || (rc = order(c.dev(il), c.dev(ih), c.dev(io))) || (rc = c.fetch(io, (size_t)n * 4))) return rc;
    return c.finish();
}

}  // extern "C"
