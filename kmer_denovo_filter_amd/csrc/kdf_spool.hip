// kdf_spool.hip -- libkdf.so, the read spool (kdf.h "read spool", kernels in kdf_spool.h): a sample's packed stream
// kept resident and replayed.  An object of its own: it drives the engine through the public C API and, of the
// engine's state (kdf_engine_priv.h), touches the device, the stream, the error text, the upload slots and sk.on only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "kdf_engine_priv.h"
#include "kdf_spool.h"

#define KS_STAGES 6
enum { KT_APPEND = 0, KT_OFFSETS, KT_COUNT };          // a spool's timers (option "profile"): stats "append_*", "offsets_*"
static const char *const KS_TIMER_NAME[KT_COUNT] = {"append", "offsets"};
struct KsSegment {
    uint64_t *packed = nullptr, *mask = nullptr;     // 2 cap_tiles + 4 / cap_tiles + 2 words: HBM, or pinned host memory
    uint64_t cap_tiles = 0, tiles = 0;               // room / used; the segment is a stream of tiles x 64 positions
    uint64_t bytes = 0;
    bool host = false;
    // a spool that keeps reads: offs[0 .. n_reads] in SEGMENT coordinates, in the segment's tier (room for offs_cap entries)
    int64_t *offs = nullptr;
    uint64_t offs_cap = 0, n_reads = 0, first_read = 0;
};
enum { KS_MODE_OPEN = 0, KS_MODE_STREAM = 1, KS_MODE_READS = 2 };   // decided by the first append since create / clear
struct kdf_spool {
    int device = 0;
    uint64_t hbm_budget = 0, host_budget = 0;
    uint64_t opt_segment_positions = 1ull << 30;
    std::vector<KsSegment> segs;
    uint64_t hbm_bytes = 0, host_bytes = 0, batches = 0, bases = 0, replays = 0;
    int mode = KS_MODE_OPEN;
    uint64_t reads = 0, offset_bytes = 0;
    uint64_t opt_offsets_chunk = 1ull << 16;         // entries: the unit an offsets array is sized and grown in
    bool overflowed = false;
    hipStream_t stream = nullptr;                    // kdf_spool_append (host sources) runs here
    hipEvent_t last = nullptr; bool have_last = false;   // behind the latest append, whatever stream it ran on
    DevBuf buf[KS_STAGES + 4];                       // every grow-only device buffer (released together), through the views below
    // 0/1 a host source's words, 2/3 a host-tier batch before its copy out, 4 a host source's offsets, 5 a host-tier
    // batch's offsets before their copy out; the last user is an append, and every append is behind `last`
    DevBuf *const stage = buf;
    // kdf_spool_append_uploaded_reads: the caller's offsets pass through pinned memory, so the copy is truly asynchronous
    // and the caller's array is its own again at once; pin_done is behind the copy that read it last
    // (one buffer per upload slot: the host never waits for the append it queued last)
    int64_t *pin_offs[2] = {nullptr, nullptr}; size_t pin_entries[2] = {0, 0};
    hipEvent_t pin_done[2] = {nullptr, nullptr}; bool have_pin_done[2] = {false, false};
    // replays of the per-read consumers: one host-tier segment's packed, mask and offsets words on the device (not
    // charged to the budget); rep_done is behind the consumer that read them last, whatever engine it ran on
    DevBuf *const rep = buf + KS_STAGES;
    hipEvent_t rep_done = nullptr; bool have_rep_done = false;
    // kdf_spool_select_reads: block sums (device) and the total (pinned)
    DevBuf *const sel_buf = buf + KS_STAGES + 3;
    unsigned long long *sel_total = nullptr;
    bool prof = false;
    EvTimer timer[KT_COUNT];                         // never reset: turning "profile" off keeps what was recorded
    std::string err;
};

static int ks_fail(kdf_spool *sp, int code, const char *fmt, ...) {
    char buf[768];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (sp) sp->err = buf; else g_err = buf;
    return code;
}

#define KSCHK(sp, call)                                                                 \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess)                                                           \
            return ks_fail(sp, e_ == hipErrorOutOfMemory ? KDF_ERR_NOMEM : KDF_ERR_HIP, \
                           "%s failed: %s", #call, hipGetErrorString(e_));              \
    } while (0)

struct KsSink {                                      // where the message of a refusal goes: this spool's error string
    kdf_spool *sp;
    template <typename... A> int operator()(int code, const char *fmt, A... a) const { return ks_fail(sp, code, fmt, a...); }
};

// Room for `bytes` in one of the spool's buffers (dev_reserve): `want` bytes are allocated, quiesce() waits for the old
// buffer's last reader (a failed wait is a KDF_ERR_HIP).  fmt words a failed allocation: (%zu bytes wanted, %s HIP's text).
template <typename Q>
static int ks_reserve(kdf_spool *sp, DevBuf &b, size_t bytes, size_t want, Q &&quiesce, const char *fmt) {
    hipError_t qe = hipSuccess;
    const hipError_t e = dev_reserve(b, bytes, want, [&] { return qe = quiesce(); });
    if (qe != hipSuccess) return ks_fail(sp, KDF_ERR_HIP, "read spool: waiting for a buffer's last reader failed: %s", hipGetErrorString(qe));
    return e == hipSuccess ? KDF_OK : ks_fail(sp, KDF_ERR_NOMEM, fmt, want, hipGetErrorString(e));
}

// staging: the buffer's last user is an append, and every append is behind sp->last
static int ks_stage_reserve(kdf_spool *sp, int i, size_t bytes) {
    return ks_reserve(sp, sp->stage[i], bytes, slack_8th(bytes), [&] { return sp->have_last ? hipEventSynchronize(sp->last) : hipSuccess; },
                      "read spool: %zu bytes of staging do not fit the device (%s)");
}

static void ks_free_all(kdf_spool *sp) {
    (void)hipSetDevice(sp->device);
    (void)hipDeviceSynchronize();                    // replays read the segments on their engines' streams
    for (EvTimer &t : sp->timer) t.collect();
    for (auto &s : sp->segs) {
        if (s.host) { if (s.packed) (void)hipHostFree(s.packed); if (s.mask) (void)hipHostFree(s.mask); if (s.offs) (void)hipHostFree(s.offs); }
        else { if (s.packed) (void)hipFree(s.packed); if (s.mask) (void)hipFree(s.mask); if (s.offs) (void)hipFree(s.offs); }
    }
    sp->segs.clear();
    for (DevBuf &b : sp->buf) b.release();
    for (int i = 0; i < 2; ++i) {
        if (sp->pin_offs[i]) (void)hipHostFree(sp->pin_offs[i]);
        sp->pin_offs[i] = nullptr; sp->pin_entries[i] = 0; sp->have_pin_done[i] = false;
    }
    sp->hbm_bytes = sp->host_bytes = sp->batches = sp->bases = sp->reads = sp->offset_bytes = 0;
    sp->mode = KS_MODE_OPEN;
    sp->overflowed = false; sp->have_last = false; sp->have_rep_done = false;
}

// The segment and tile at which a batch of n_tiles goes: the last segment while it has room, a new one otherwise (HBM
// within its budget, then pinned host memory within its, then KDF_ERR_NOMEM and the spool is marked overflowed).
// entries of an offsets array that must hold `need`: a new one (have == 0) is sized for the whole segment from the read
// density of the batch that opens it (at most one read per 32 positions is assumed), a grown one by at least an eighth;
// both in units of option "offsets_chunk"
static uint64_t ks_offsets_want(const kdf_spool *sp, uint64_t cap_tiles, uint64_t have, uint64_t need, uint64_t n_bases, uint64_t n_reads) {
    uint64_t want;
    if (!have) {
        const uint64_t cap_pos = cap_tiles * KDF_TILE;
        const double est = (double)cap_pos * (double)(n_reads + 1) / (double)std::max<uint64_t>(n_bases, 1) * 1.125;
        want = std::max<uint64_t>(need, (uint64_t)std::min<double>(est, (double)(cap_pos / 32)));
    } else want = std::max<uint64_t>(need, have + have / 8);
    const uint64_t chunk = sp->opt_offsets_chunk;
    return (want + chunk - 1) / chunk * chunk;
}

// keep_reads / keep_bases: the batch brings keep_reads > 0 reads, and a NEW segment must fit its tier's budget together with
// its first offsets array (so that array's allocation does not overflow a spool whose other tier has room)
static int spool_place(kdf_spool *sp, uint64_t n_tiles, KsSegment **seg_out, bool *fresh = nullptr, uint64_t keep_reads = 0, uint64_t keep_bases = 0) {
    if (fresh) *fresh = false;
    if (!sp->segs.empty() && sp->segs.back().tiles + n_tiles <= sp->segs.back().cap_tiles) { *seg_out = &sp->segs.back(); return KDF_OK; }
    KsSegment s;
    s.first_read = sp->reads;
    s.cap_tiles = std::max<uint64_t>(sp->opt_segment_positions / KDF_TILE, n_tiles);
    const uint64_t pb = (2 * s.cap_tiles + 4) * 8, mb = (s.cap_tiles + 2) * 8;
    s.bytes = pb + mb;
    const uint64_t ob = keep_reads ? ks_offsets_want(sp, s.cap_tiles, 0, keep_reads + 1, keep_bases, keep_reads) * 8 : 0;
    if (sp->hbm_bytes + s.bytes + ob <= sp->hbm_budget) {
        hipError_t e = hipMalloc((void **)&s.packed, pb);
        if (e == hipSuccess && (e = hipMalloc((void **)&s.mask, mb)) != hipSuccess) { (void)hipFree(s.packed); s.packed = nullptr; }
        if (e != hipSuccess) { (void)hipGetLastError(); s.packed = s.mask = nullptr; }      // an expected event: the next tier takes it
    }
    if (!s.packed && sp->host_bytes + s.bytes + ob <= sp->host_budget) {
        hipError_t e = hipHostMalloc((void **)&s.packed, pb, hipHostMallocDefault);
        if (e == hipSuccess && (e = hipHostMalloc((void **)&s.mask, mb, hipHostMallocDefault)) != hipSuccess) { (void)hipHostFree(s.packed); s.packed = nullptr; }
        if (e != hipSuccess) { (void)hipGetLastError(); s.packed = s.mask = nullptr; }
        else s.host = true;
    }
    if (!s.packed) {
        sp->overflowed = true;
        return ks_fail(sp, KDF_ERR_NOMEM, "read spool: a segment of %llu bytes (with its read offsets, if it keeps any) fits neither budget (HBM %llu of %llu bytes used, host %llu of %llu): "
                       "the spool is overflowed -- stream the source again, or kdf_spool_clear",
                       (unsigned long long)(s.bytes + ob), (unsigned long long)sp->hbm_bytes, (unsigned long long)sp->hbm_budget,
                       (unsigned long long)sp->host_bytes, (unsigned long long)sp->host_budget);
    }
    (s.host ? sp->host_bytes : sp->hbm_bytes) += s.bytes;
    sp->segs.push_back(s);
    *seg_out = &sp->segs.back();
    if (fresh) *fresh = true;
    return KDF_OK;
}

// Room for `need` entries in the segment's offsets array, in the segment's tier and within its budget; the entries
// stored so far move along.  A new array is sized for the whole segment from the read density of the batch that opens it
// (at most one read per 32 positions is assumed; more than that grows), in units of option "offsets_chunk", so that
// growing -- which waits for the device: replays may be reading the old array -- stays rare.
static int ks_offsets_reserve(kdf_spool *sp, KsSegment *seg, uint64_t need, uint64_t n_bases, uint64_t n_reads) {
    if (seg->offs_cap >= need) return KDF_OK;
    const uint64_t want = ks_offsets_want(sp, seg->cap_tiles, seg->offs_cap, need, n_bases, n_reads);
    const uint64_t add = (want - seg->offs_cap) * 8;
    uint64_t &used = seg->host ? sp->host_bytes : sp->hbm_bytes;
    const uint64_t budget = seg->host ? sp->host_budget : sp->hbm_budget;
    int64_t *fresh = nullptr;
    hipError_t e = hipErrorOutOfMemory;
    if (used + add <= budget) {
        e = seg->host ? hipHostMalloc((void **)&fresh, want * 8, hipHostMallocDefault) : hipMalloc((void **)&fresh, want * 8);
        if (e != hipSuccess) { (void)hipGetLastError(); fresh = nullptr; }
    }
    if (!fresh) {
        sp->overflowed = true;
        return ks_fail(sp, KDF_ERR_NOMEM, "read spool: %llu bytes of read offsets do not fit the %s budget (%llu of %llu bytes used): the spool is "
                       "overflowed -- stream the source again, or kdf_spool_clear", (unsigned long long)add, seg->host ? "host" : "HBM",
                       (unsigned long long)used, (unsigned long long)budget);
    }
    if (seg->offs) {
        e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(fresh, seg->offs, (seg->n_reads + 1) * 8, seg->host ? hipMemcpyHostToHost : hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            if (seg->host) (void)hipHostFree(fresh); else (void)hipFree(fresh);
            return ks_fail(sp, KDF_ERR_HIP, "read spool: moving a segment's read offsets failed: %s", hipGetErrorString(e));
        }
        if (seg->host) (void)hipHostFree(seg->offs); else (void)hipFree(seg->offs);
    }
    seg->offs = fresh; seg->offs_cap = want;
    used += add; seg->bytes += add; sp->offset_bytes += add;
    return KDF_OK;
}

// n_reads >= 0, offsets[0] == 0, no decrease, offsets[n_reads] == n_bases: what kdf_pack_reads and kdf_reader_next hand out
static int ks_check_offsets(kdf_spool *sp, const char *fn, const int64_t *offs, int64_t n_reads, uint64_t n_bases) {
    if (n_reads == 0 && n_bases) return ks_fail(sp, KDF_ERR_INVALID, "%s: %llu positions in no read (read_offsets[n_reads] must be n_bases)", fn, (unsigned long long)n_bases);
    if (n_reads > 0 && n_bases == 0) return ks_fail(sp, KDF_ERR_INVALID, "%s: %lld reads in a batch of no positions (a batch without positions has no place in a segment)", fn, (long long)n_reads);
    if (n_reads > 0 && offs && offs[0] != 0) return ks_fail(sp, KDF_ERR_INVALID, "%s: read_offsets[0] = %lld, not 0", fn, (long long)offs[0]);
    const int rc = check_read_offsets(KsSink{sp}, fn, offs, n_reads);                  // negative n_reads, NULL, a decrease
    if (rc || n_reads == 0) return rc;
    if ((uint64_t)offs[n_reads] != n_bases)
        return ks_fail(sp, KDF_ERR_INVALID, "%s: read_offsets[n_reads] = %lld, not n_bases = %llu (the last read must end where the batch ends)", fn,
                       (long long)offs[n_reads], (unsigned long long)n_bases);
    return KDF_OK;
}

// keep: this append brings read offsets.  The first append since create / clear decides what the spool keeps.
static int ks_check_append(kdf_spool *sp, const void *p, const void *m, uint64_t n_bases, const char *fn, bool keep = false) {
    if (sp->mode != KS_MODE_OPEN && (sp->mode == KS_MODE_READS) != keep)
        return ks_fail(sp, KDF_ERR_STATE, keep ? "%s: the spool keeps no read offsets (its first append brought none): kdf_spool_append* or kdf_spool_clear"
                                               : "%s: the spool keeps read offsets: kdf_spool_append*_reads or kdf_spool_clear", fn);
    if (n_bases > (1ull << 31)) return ks_fail(sp, KDF_ERR_INVALID, "%s: a batch of %llu positions (at most 2^31)", fn, (unsigned long long)n_bases);
    if (sp->overflowed) return ks_fail(sp, KDF_ERR_STATE, "%s: the spool is overflowed (kdf_spool_clear)", fn);
    if (n_bases && (!p || !m)) return ks_fail(sp, KDF_ERR_INVALID, "%s: NULL stream", fn);
    return KDF_OK;
}

// one batch from DEVICE buffers, on stream s (behind every earlier append).  keep: with its n_reads + 1 read offsets,
// either on the device (d_offs) or in host memory that stays valid until the copy queued here has run (h_offs).
static int spool_append_dev(kdf_spool *sp, hipStream_t s, const uint64_t *d_packed, const uint64_t *d_invalid, uint64_t n_bases,
                            bool keep = false, const int64_t *d_offs = nullptr, const int64_t *h_offs = nullptr, uint64_t n_reads = 0) {
    const uint64_t n_tiles = n_bases / KDF_TILE + 1;
    KsSegment *seg = nullptr;
    bool fresh = false;
    int rc = spool_place(sp, n_tiles, &seg, &fresh, keep ? n_reads : 0, n_bases);
    if (rc) return rc;
    if (keep && (rc = ks_offsets_reserve(sp, seg, seg->n_reads + n_reads + 1, n_bases, n_reads))) {
        if (fresh) {                                               // nothing of this batch stays behind
            if (seg->host) { (void)hipHostFree(seg->packed); (void)hipHostFree(seg->mask); sp->host_bytes -= seg->bytes; }
            else { (void)hipFree(seg->packed); (void)hipFree(seg->mask); sp->hbm_bytes -= seg->bytes; }
            sp->segs.pop_back();
        }
        return rc;
    }
    uint64_t *dp = seg->packed + 2 * seg->tiles, *dm = seg->mask + seg->tiles;
    int64_t *doffs = keep ? seg->offs + seg->n_reads : nullptr;
    if (seg->host) {
        if ((rc = ks_stage_reserve(sp, 2, (2 * n_tiles + 4) * 8)) || (rc = ks_stage_reserve(sp, 3, (n_tiles + 2) * 8)) ||
            (keep && (rc = ks_stage_reserve(sp, 5, (n_reads + 1) * 8)))) { sp->overflowed = true; return rc; }
        dp = (uint64_t *)sp->stage[2].p; dm = (uint64_t *)sp->stage[3].p;
        if (keep) doffs = (int64_t *)sp->stage[5].p;
    }
    if (keep && h_offs && (rc = ks_stage_reserve(sp, 4, (n_reads + 1) * 8))) return rc;
    if (sp->have_last) KSCHK(sp, hipStreamWaitEvent(s, sp->last, 0));
    if (keep && h_offs) {
        KSCHK(sp, hipMemcpyAsync(sp->stage[4].p, h_offs, (n_reads + 1) * 8, hipMemcpyHostToDevice, s));
        d_offs = (const int64_t *)sp->stage[4].p;
    }
    const unsigned blocks = (unsigned)std::min<uint64_t>((n_tiles + 2 + KS_THREADS - 1) / KS_THREADS, KS_MAX_BLOCKS);
    EvSpan span(sp->timer[KT_APPEND], sp->prof, s);
    hipLaunchKernelGGL(ks_append_kernel, dim3(blocks), dim3(KS_THREADS), 0, s, dp, dm, d_packed, d_invalid, n_bases, n_tiles,
                       (int)(((uintptr_t)d_packed & 15) == 0));
    KSCHK(sp, hipGetLastError());
    span.stop();
    if (keep) {
        // entries n_reads(seg) .. n_reads(seg) + n_reads: the first overwrites the last entry of the batch before (kdf.h: the gap)
        const unsigned oblocks = (unsigned)std::min<uint64_t>((n_reads + 1 + KS_THREADS - 1) / KS_THREADS, KS_MAX_BLOCKS);
        EvSpan ospan(sp->timer[KT_OFFSETS], sp->prof, s);
        hipLaunchKernelGGL(ks_offsets_kernel, dim3(oblocks), dim3(KS_THREADS), 0, s, doffs, d_offs, n_reads + 1, (int64_t)(seg->tiles * KDF_TILE));
        KSCHK(sp, hipGetLastError());
        ospan.stop();
    }
    if (seg->host) {
        KSCHK(sp, hipMemcpyAsync(seg->packed + 2 * seg->tiles, dp, (2 * n_tiles + 4) * 8, hipMemcpyDeviceToHost, s));
        KSCHK(sp, hipMemcpyAsync(seg->mask + seg->tiles, dm, (n_tiles + 2) * 8, hipMemcpyDeviceToHost, s));
        if (keep) KSCHK(sp, hipMemcpyAsync(seg->offs + seg->n_reads, doffs, (n_reads + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    KSCHK(sp, hipEventRecord(sp->last, s));
    sp->have_last = true;
    seg->tiles += n_tiles;
    ++sp->batches; sp->bases += n_bases;
    if (keep) { seg->n_reads += n_reads; sp->reads += n_reads; }
    sp->mode = keep ? KS_MODE_READS : KS_MODE_STREAM;
    return KDF_OK;
}

// a replay buffer's last reader ran on some engine's stream: the whole device is drained before a free
static int ks_rep_reserve(kdf_spool *sp, int i, size_t bytes) {
    return ks_reserve(sp, sp->rep[i], bytes, slack_8th(bytes), [] { return hipDeviceSynchronize(); },
                      "read spool: %zu bytes of staging for a host-tier segment do not fit the device (%s)");
}

// Every segment in order through kdf_read_hits_dev (depth false; 8 bytes a row) or kdf_read_depth_dev (48 bytes a row),
// rows of segment s at first_read(s).
static int spool_replay_reads(kdf_spool *sp, kdf_engine *h, const char *fn, bool depth, uint32_t low_max, void *d_rows_out) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    if (!h) return ks_fail(sp, KDF_ERR_INVALID, "%s: NULL engine", fn);
    if (h->device != sp->device) return ks_fail(sp, KDF_ERR_INVALID, "%s: the spool is on device %d, the engine on %d", fn, sp->device, h->device);
    if (sp->overflowed) return ks_fail(sp, KDF_ERR_STATE, "%s: the spool is overflowed: it does not hold the whole stream (kdf_spool_clear)", fn);
    if (sp->mode == KS_MODE_STREAM) return ks_fail(sp, KDF_ERR_STATE, "%s: the spool keeps no read offsets (fill it through kdf_spool_append*_reads)", fn);
    if (sp->reads == 0) return KDF_OK;
    if (!d_rows_out) return ks_fail(sp, KDF_ERR_INVALID, "%s: rows_out is NULL", fn);
    KSCHK(sp, hipSetDevice(sp->device));
    bool any_host = false;
    for (auto &s : sp->segs) any_host |= s.host && s.n_reads;
    if (sp->have_last) {
        KSCHK(sp, hipStreamWaitEvent(h->stream, sp->last, 0));
        if (any_host) KSCHK(sp, hipEventSynchronize(sp->last));    // (the copies below read host memory)
    }
    const size_t row_bytes = depth ? KD_ROW_WORDS * 8 : KH_ROW_WORDS * 4;
    for (size_t i = 0; i < sp->segs.size(); ++i) {
        const KsSegment &s = sp->segs[i];
        if (s.n_reads == 0) continue;
        const uint64_t n = s.tiles * KDF_TILE;
        const void *p = s.packed, *m = s.mask, *o = s.offs;
        if (s.host) {
            const size_t pb = (2 * s.tiles + 4) * 8, mb = (s.tiles + 2) * 8, ob = (s.n_reads + 1) * 8;
            int rc;
            if ((rc = ks_rep_reserve(sp, 0, pb)) || (rc = ks_rep_reserve(sp, 1, mb)) || (rc = ks_rep_reserve(sp, 2, ob))) return rc;
            if (sp->have_rep_done) KSCHK(sp, hipStreamWaitEvent(h->stream, sp->rep_done, 0));
            KSCHK(sp, hipMemcpyAsync(sp->rep[0].p, s.packed, pb, hipMemcpyHostToDevice, h->stream));
            KSCHK(sp, hipMemcpyAsync(sp->rep[1].p, s.mask, mb, hipMemcpyHostToDevice, h->stream));
            KSCHK(sp, hipMemcpyAsync(sp->rep[2].p, s.offs, ob, hipMemcpyHostToDevice, h->stream));
            p = sp->rep[0].p; m = sp->rep[1].p; o = sp->rep[2].p;
        }
        char *rows = (char *)d_rows_out + s.first_read * row_bytes;
        const int rc = depth ? kdf_read_depth_dev(h, p, m, n, o, (int64_t)s.n_reads, low_max, rows)
                             : kdf_read_hits_dev(h, p, m, n, o, (int64_t)s.n_reads, nullptr, rows);
        if (s.host) { KSCHK(sp, hipEventRecord(sp->rep_done, h->stream)); sp->have_rep_done = true; }
        if (rc) return ks_fail(sp, rc, "%s: segment %zu: %s", fn, i, h->err.c_str());
    }
    ++sp->replays;
    return KDF_OK;
}

// every segment in order into one stream entry point of the engine: mode 0 count, 1 count --if, 2 prefilter tally
// (kdf_spool_replay), 3 sketch (kdf_spool_sketch)
static int spool_walk(kdf_spool *sp, kdf_engine *h, int mode) {
    const char *fn = mode == 3 ? "kdf_spool_sketch" : "kdf_spool_replay";
    if (h->device != sp->device) return ks_fail(sp, KDF_ERR_INVALID, "%s: the spool is on device %d, the engine on %d", fn, sp->device, h->device);
    if (sp->overflowed) return ks_fail(sp, KDF_ERR_STATE, "%s: the spool is overflowed: it does not hold the whole stream (kdf_spool_clear)", fn);
    const size_t ns = sp->segs.size();
    size_t next_host = ns;                                         // the host-tier segment whose upload comes next
    for (size_t i = 0; i < ns; ++i) if (sp->segs[i].host) { next_host = i; break; }
    if (next_host < ns && (h->up.slot[0].valid || h->up.slot[1].valid))
        return ks_fail(sp, KDF_ERR_STATE, "%s: host-tier segments go through the engine's upload slots, and slot %d holds a batch "
                       "that was not counted", fn, h->up.slot[0].valid ? 0 : 1);
    KSCHK(sp, hipSetDevice(sp->device));
    if (sp->have_last) {
        KSCHK(sp, hipStreamWaitEvent(h->stream, sp->last, 0));
        if (next_host < ns) KSCHK(sp, hipEventSynchronize(sp->last));   // (the upload reads host memory on the engine's copy stream)
    }
    auto pass = [&](size_t i, int rc) {
        if (!rc) return KDF_OK;
        h->up.slot[0].valid = h->up.slot[1].valid = false;                   // (both were free on entry: what they hold is the spool's)
        return ks_fail(sp, rc, "%s: segment %zu: %s", fn, i, h->err.c_str());
    };
    auto upload = [&](size_t i, int slot) {
        const KsSegment &s = sp->segs[i];
        return kdf_upload_reads_async(h, slot, s.packed, s.mask, s.tiles * KDF_TILE);
    };
    int slot = 0, rc;
    if (next_host < ns && (rc = upload(next_host, slot))) return pass(next_host, rc);
    for (size_t i = 0; i < ns; ++i) {
        const KsSegment &s = sp->segs[i];
        const uint64_t n = s.tiles * KDF_TILE;
        if (!s.host) {
            rc = mode == 0 ? kdf_count_reads_dev(h, s.packed, s.mask, n) : mode == 1 ? kdf_count_reads_filtered_dev(h, s.packed, s.mask, n)
                 : mode == 2 ? kdf_prefilter_add_reads_dev(h, s.packed, s.mask, n) : kdf_sketch_add_reads_dev(h, s.packed, s.mask, n);
            if (rc) return pass(i, rc);
            continue;
        }
        size_t j = i + 1;
        while (j < ns && !sp->segs[j].host) ++j;
        if (j < ns && (rc = upload(j, slot ^ 1))) return pass(j, rc);   // its copy runs under this segment's count
        if (mode == 3) { rc = kdf_sketch_add_uploaded(h, slot); h->up.slot[slot].valid = false; }   // (the sketch leaves a batch in its slot: this one is the spool's)
        else rc = mode == 2 ? kdf_prefilter_add_uploaded(h, slot) : kdf_count_uploaded(h, slot, mode == 1);
        if (rc) return pass(i, rc);
        slot ^= 1;
    }
    if (mode != 3) ++sp->replays;
    return KDF_OK;
}

extern "C" {

int kdf_spool_create(int device, uint64_t hbm_budget_bytes, uint64_t host_budget_bytes, kdf_spool **out) {
    if (!out) return ks_fail(nullptr, KDF_ERR_INVALID, "kdf_spool_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return ks_fail(nullptr, KDF_ERR_HIP, "kdf_spool_create: no HIP device available (%s)", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return ks_fail(nullptr, KDF_ERR_INVALID, "kdf_spool_create: device %d of %d", device, ndev);
    if ((e = hipSetDevice(device)) != hipSuccess) return ks_fail(nullptr, KDF_ERR_HIP, "kdf_spool_create: %s", hipGetErrorString(e));
    kdf_spool *sp = new kdf_spool();
    sp->device = device; sp->hbm_budget = hbm_budget_bytes; sp->host_budget = host_budget_bytes;
    if ((e = hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sp->last, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sp->pin_done[0], hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sp->pin_done[1], hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sp->rep_done, hipEventDisableTiming)) != hipSuccess) {
        ks_fail(nullptr, KDF_ERR_HIP, "kdf_spool_create: %s", hipGetErrorString(e));
        kdf_spool_destroy(sp);
        return KDF_ERR_HIP;
    }
    *out = sp;
    return KDF_OK;
}

void kdf_spool_destroy(kdf_spool *sp) {
    if (!sp) return;
    ks_free_all(sp);
    if (sp->last) (void)hipEventDestroy(sp->last);
    for (int i = 0; i < 2; ++i) if (sp->pin_done[i]) (void)hipEventDestroy(sp->pin_done[i]);
    if (sp->rep_done) (void)hipEventDestroy(sp->rep_done);
    if (sp->sel_total) (void)hipHostFree(sp->sel_total);
    if (sp->stream) (void)hipStreamDestroy(sp->stream);
    delete sp;
}

const char *kdf_spool_error(const kdf_spool *sp) { return sp ? sp->err.c_str() : g_err.c_str(); }

int kdf_spool_clear(kdf_spool *sp) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    ks_free_all(sp);
    return KDF_OK;
}

int kdf_spool_set_option(kdf_spool *sp, const char *name, int64_t value) {
    if (!sp || !name) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_set_option: NULL argument");
    const std::string n(name);
    if (n == "segment_positions") {
        if (value < (1ll << 12) || value > (1ll << 31)) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_set_option: segment_positions must be 2^12 .. 2^31");
        sp->opt_segment_positions = (uint64_t)value;               // (segments already allocated keep their size)
    } else if (n == "offsets_chunk") {
        if (value < 1 || value > (1ll << 28)) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_set_option: offsets_chunk must be 1 .. 2^28 entries");
        sp->opt_offsets_chunk = (uint64_t)value;                   // (arrays already allocated keep their size)
    } else if (n == "profile") {
        if (!value) { (void)hipSetDevice(sp->device); for (EvTimer &t : sp->timer) t.collect(); }
        sp->prof = value != 0;
    } else return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_set_option: unknown option %s", name);
    return KDF_OK;
}

int kdf_spool_get_stat(kdf_spool *sp, const char *name, int64_t *value) {
    if (!sp || !name || !value) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_get_stat: NULL argument");
    const std::string n(name);
    bool us = false;
    if (EvTimer *t = timer_of_stat(sp->timer, KS_TIMER_NAME, KT_COUNT, n, &us)) {
        (void)hipSetDevice(sp->device);
        *value = us ? t->us() : (t->collect(), (int64_t)t->passes);
    }
    else if (n == "segments") *value = (int64_t)sp->segs.size();
    else if (n == "batches") *value = (int64_t)sp->batches;
    else if (n == "positions") { uint64_t t = 0; for (auto &s : sp->segs) t += s.tiles; *value = (int64_t)(t * KDF_TILE); }
    else if (n == "bases") *value = (int64_t)sp->bases;
    else if (n == "hbm_bytes") *value = (int64_t)sp->hbm_bytes;
    else if (n == "host_bytes") *value = (int64_t)sp->host_bytes;
    else if (n == "overflowed") *value = sp->overflowed ? 1 : 0;
    else if (n == "replays") *value = (int64_t)sp->replays;
    else if (n == "segment_positions") *value = (int64_t)sp->opt_segment_positions;
    else if (n == "offsets_chunk") *value = (int64_t)sp->opt_offsets_chunk;
    else if (n == "reads") *value = (int64_t)sp->reads;
    else if (n == "keeps_reads") *value = sp->mode == KS_MODE_READS ? 1 : 0;
    else if (n == "offset_bytes") *value = (int64_t)sp->offset_bytes;
    else return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_get_stat: unknown stat %s", name);
    return KDF_OK;
}

int kdf_spool_append_dev(kdf_spool *sp, void *hip_stream, const void *d_packed, const void *d_invalid, uint64_t n_bases) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    int rc = ks_check_append(sp, d_packed, d_invalid, n_bases, "kdf_spool_append_dev");
    if (rc || n_bases == 0) return rc;
    KSCHK(sp, hipSetDevice(sp->device));
    return spool_append_dev(sp, (hipStream_t)hip_stream, (const uint64_t *)d_packed, (const uint64_t *)d_invalid, n_bases);
}

int kdf_spool_append(kdf_spool *sp, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    int rc = ks_check_append(sp, packed, invalid, n_bases, "kdf_spool_append");
    if (rc || n_bases == 0) return rc;
    KSCHK(sp, hipSetDevice(sp->device));
    const uint64_t src_tiles = (n_bases + 63) / 64;                 // (the words the kernel loads, no more)
    if ((rc = ks_stage_reserve(sp, 0, 2 * src_tiles * 8)) || (rc = ks_stage_reserve(sp, 1, src_tiles * 8))) return rc;
    if (sp->have_last) KSCHK(sp, hipStreamWaitEvent(sp->stream, sp->last, 0));   // (the staging's last reader)
    KSCHK(sp, hipMemcpyAsync(sp->stage[0].p, packed, 2 * src_tiles * 8, hipMemcpyHostToDevice, sp->stream));
    KSCHK(sp, hipMemcpyAsync(sp->stage[1].p, invalid, src_tiles * 8, hipMemcpyHostToDevice, sp->stream));
    rc = spool_append_dev(sp, sp->stream, (const uint64_t *)sp->stage[0].p, (const uint64_t *)sp->stage[1].p, n_bases);
    KSCHK(sp, hipStreamSynchronize(sp->stream));                   // the caller's arrays are its own again
    return rc;
}

int kdf_spool_append_uploaded(kdf_spool *sp, kdf_engine *h, int slot) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    if (!h) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_append_uploaded: NULL engine");
    if (h->device != sp->device) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_append_uploaded: the spool is on device %d, the engine on %d", sp->device, h->device);
    StreamSrc src;                                                 // (the slot keeps its batch; the host does not wait for the copy)
    int rc = src_slot(KsSink{sp}, "kdf_spool_append_uploaded", h, slot, false, false, src, [&](const StreamSrc &b) {
        return ks_check_append(sp, b.packed, b.invalid, b.n_bases, "kdf_spool_append_uploaded");
    });
    if (rc || !src.n_bases) return rc;
    rc = spool_append_dev(sp, h->stream, src.packed, src.invalid, src.n_bases);
    src_release(h, src);                                           // (the slot's next upload waits for this reader as for a count)
    return rc;
}

// ---- appends that bring their read offsets ----

int kdf_spool_append_reads_dev(kdf_spool *sp, void *hip_stream, const void *d_packed, const void *d_invalid, uint64_t n_bases,
                               const void *d_read_offsets, int64_t n_reads) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    int rc = ks_check_append(sp, d_packed, d_invalid, n_bases, "kdf_spool_append_reads_dev", true);
    if (rc) return rc;
    if (n_reads < 0) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_append_reads_dev: n_reads = %lld is negative", (long long)n_reads);
    if (n_reads == 0) return n_bases ? ks_check_offsets(sp, "kdf_spool_append_reads_dev", nullptr, 0, n_bases) : KDF_OK;
    if (n_bases == 0) return ks_check_offsets(sp, "kdf_spool_append_reads_dev", nullptr, n_reads, 0);
    if (!d_read_offsets) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_append_reads_dev: read_offsets is NULL");
    KSCHK(sp, hipSetDevice(sp->device));
    return spool_append_dev(sp, (hipStream_t)hip_stream, (const uint64_t *)d_packed, (const uint64_t *)d_invalid, n_bases, true,
                            (const int64_t *)d_read_offsets, nullptr, (uint64_t)n_reads);
}

int kdf_spool_append_reads(kdf_spool *sp, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases, const int64_t *read_offsets,
                           int64_t n_reads) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    int rc = ks_check_append(sp, packed, invalid, n_bases, "kdf_spool_append_reads", true);
    if (rc || (rc = ks_check_offsets(sp, "kdf_spool_append_reads", read_offsets, n_reads, n_bases)) || n_reads == 0) return rc;
    KSCHK(sp, hipSetDevice(sp->device));
    const uint64_t src_tiles = (n_bases + 63) / 64;                 // (>= 1: a batch with reads has positions)
    if ((rc = ks_stage_reserve(sp, 0, 2 * src_tiles * 8)) || (rc = ks_stage_reserve(sp, 1, src_tiles * 8))) return rc;
    if (sp->have_last) KSCHK(sp, hipStreamWaitEvent(sp->stream, sp->last, 0));
    KSCHK(sp, hipMemcpyAsync(sp->stage[0].p, packed, 2 * src_tiles * 8, hipMemcpyHostToDevice, sp->stream));
    KSCHK(sp, hipMemcpyAsync(sp->stage[1].p, invalid, src_tiles * 8, hipMemcpyHostToDevice, sp->stream));
    rc = spool_append_dev(sp, sp->stream, (const uint64_t *)sp->stage[0].p, (const uint64_t *)sp->stage[1].p, n_bases, true, nullptr, read_offsets,
                          (uint64_t)n_reads);
    KSCHK(sp, hipStreamSynchronize(sp->stream));                   // the caller's arrays are its own again
    return rc;
}

int kdf_spool_append_uploaded_reads(kdf_spool *sp, kdf_engine *h, int slot, const int64_t *read_offsets, int64_t n_reads) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    if (!h) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_append_uploaded_reads: NULL engine");
    if (h->device != sp->device) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_append_uploaded_reads: the spool is on device %d, the engine on %d", sp->device, h->device);
    StreamSrc src;
    int rc = src_slot(KsSink{sp}, "kdf_spool_append_uploaded_reads", h, slot, false, false, src, [&](const StreamSrc &b) {
        const int rcb = ks_check_append(sp, b.packed, b.invalid, b.n_bases, "kdf_spool_append_uploaded_reads", true);
        return rcb ? rcb : ks_check_offsets(sp, "kdf_spool_append_uploaded_reads", read_offsets, n_reads, b.n_bases);
    });
    if (rc || n_reads == 0) return rc;
    // through pinned memory: the copy is queued behind the engine's work and the caller's array is not read after this returns
    const size_t entries = (size_t)n_reads + 1;
    if (sp->have_pin_done[slot]) KSCHK(sp, hipEventSynchronize(sp->pin_done[slot]));   // (the slot's append before this one)
    if (sp->pin_entries[slot] < entries) {
        if (sp->pin_offs[slot]) (void)hipHostFree(sp->pin_offs[slot]);
        sp->pin_offs[slot] = nullptr; sp->pin_entries[slot] = 0;
        const size_t want = entries + entries / 8 + 512;
        const hipError_t e = hipHostMalloc((void **)&sp->pin_offs[slot], want * 8, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); sp->pin_offs[slot] = nullptr; return ks_fail(sp, KDF_ERR_NOMEM, "read spool: %zu bytes of pinned staging: %s", want * 8, hipGetErrorString(e)); }
        sp->pin_entries[slot] = want;
    }
    memcpy(sp->pin_offs[slot], read_offsets, entries * 8);
    rc = spool_append_dev(sp, h->stream, src.packed, src.invalid, src.n_bases, true, nullptr, sp->pin_offs[slot], (uint64_t)n_reads);
    if (hipEventRecord(sp->pin_done[slot], h->stream) == hipSuccess) sp->have_pin_done[slot] = true;
    else { (void)hipGetLastError(); (void)hipStreamSynchronize(h->stream); sp->have_pin_done[slot] = false; }
    src_release(h, src);                                           // (the slot's next upload waits for this reader as for a count)
    return rc;
}

int kdf_spool_read_offsets(kdf_spool *sp, uint64_t seg, int64_t *out, uint64_t *first_read_out, uint64_t *n_reads_out) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    if (seg >= sp->segs.size()) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_read_offsets: segment %llu of %zu", (unsigned long long)seg, sp->segs.size());
    if (sp->mode != KS_MODE_READS) return ks_fail(sp, KDF_ERR_STATE, "kdf_spool_read_offsets: the spool keeps no read offsets (kdf_spool_append*_reads)");
    const KsSegment &s = sp->segs[seg];
    if (first_read_out) *first_read_out = s.first_read;
    if (n_reads_out) *n_reads_out = s.n_reads;
    if (!out) return KDF_OK;
    KSCHK(sp, hipSetDevice(sp->device));
    if (sp->have_last) KSCHK(sp, hipEventSynchronize(sp->last));
    KSCHK(sp, hipMemcpy(out, s.offs, (s.n_reads + 1) * 8, s.host ? hipMemcpyHostToHost : hipMemcpyDeviceToHost));
    return KDF_OK;
}

int kdf_spool_segment_dev(kdf_spool *sp, uint64_t seg, const void **d_packed, const void **d_invalid, uint64_t *n_positions,
                          const void **d_offsets, uint64_t *first_read, uint64_t *n_reads) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    if (seg >= sp->segs.size()) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_segment_dev: segment %llu of %zu", (unsigned long long)seg, sp->segs.size());
    const KsSegment &s = sp->segs[seg];
    if (s.host)
        return ks_fail(sp, KDF_ERR_STATE, "kdf_spool_segment_dev: segment %llu is in host memory, no device pointer exists (kdf_spool_read_segment "
                       "copies it out)", (unsigned long long)seg);
    KSCHK(sp, hipSetDevice(sp->device));
    if (sp->have_last) KSCHK(sp, hipEventSynchronize(sp->last));  // complete for every stream the caller may use
    if (d_packed) *d_packed = s.packed;
    if (d_invalid) *d_invalid = s.mask;
    if (n_positions) *n_positions = s.tiles * KDF_TILE;
    if (d_offsets) *d_offsets = sp->mode == KS_MODE_READS ? s.offs : nullptr;
    if (first_read) *first_read = s.first_read;
    if (n_reads) *n_reads = s.n_reads;
    return KDF_OK;
}

// ---- replays of the per-read consumers ----

int kdf_spool_read_hits(kdf_spool *sp, kdf_engine *h, void *d_rows_out) {
    return spool_replay_reads(sp, h, "kdf_spool_read_hits", false, 0, d_rows_out);
}

int kdf_spool_read_depth(kdf_spool *sp, kdf_engine *h, uint32_t low_max, void *d_rows_out) {
    return spool_replay_reads(sp, h, "kdf_spool_read_depth", true, low_max, d_rows_out);
}

int kdf_spool_select_reads(kdf_spool *sp, const void *d_hit_rows, uint32_t min_distinct, void *d_reads_out, uint64_t cap, uint64_t *n_out) {
    if (!sp || !n_out) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_select_reads: NULL pointer");
    *n_out = 0;
    if (sp->mode == KS_MODE_STREAM) return ks_fail(sp, KDF_ERR_STATE, "kdf_spool_select_reads: the spool keeps no read offsets (fill it through kdf_spool_append*_reads)");
    const uint64_t n_rows = sp->reads;
    if (n_rows == 0) return KDF_OK;
    if (!d_hit_rows || (cap && !d_reads_out)) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_select_reads: NULL pointer");
    const uint64_t n_blocks = (n_rows + KS_SELECT_ROWS - 1) / KS_SELECT_ROWS;
    if (n_blocks >= (1ull << 24))                                  // (a grid of 256-thread blocks stays below 2^32 threads)
        return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_select_reads: %llu rows are beyond the 2^34 a call takes", (unsigned long long)n_rows);
    KSCHK(sp, hipSetDevice(sp->device));
    if (!sp->sel_total) KSCHK(sp, hipHostMalloc((void **)&sp->sel_total, 8, hipHostMallocDefault));
    // (nothing to wait for before a free: every earlier use ended in a synchronise)
    if (const int rc = ks_reserve(sp, *sp->sel_buf, (n_blocks + 1) * 8, (n_blocks + 1) * 8 + n_blocks + 4096, [] { return hipSuccess; },
                                  "kdf_spool_select_reads: %zu bytes of block sums: %s")) return rc;
    unsigned long long *sums = (unsigned long long *)sp->sel_buf->p;
    const int rows16 = (int)(((uintptr_t)d_hit_rows & 15) == 0);
    hipLaunchKernelGGL(ks_select_count_kernel, dim3((unsigned)n_blocks), dim3(256), 0, sp->stream, (const uint64_t *)d_hit_rows, n_rows, min_distinct, rows16, sums);
    kh_scan_launch(sp->stream, sums, n_blocks);
    if (cap)
        hipLaunchKernelGGL(ks_select_write_kernel, dim3((unsigned)n_blocks), dim3(256), 0, sp->stream, (const uint64_t *)d_hit_rows, n_rows, min_distinct,
                           rows16, (const unsigned long long *)sums, (uint64_t *)d_reads_out, cap);
    KSCHK(sp, hipGetLastError());
    KSCHK(sp, hipMemcpyAsync(sp->sel_total, sums + n_blocks, 8, hipMemcpyDeviceToHost, sp->stream));
    KSCHK(sp, hipStreamSynchronize(sp->stream));
    *n_out = *sp->sel_total;
    if (*n_out > cap)
        return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_select_reads: %llu reads are selected, the buffer holds %llu", (unsigned long long)*n_out, (unsigned long long)cap);
    return KDF_OK;
}

int kdf_spool_read_segment(kdf_spool *sp, uint64_t seg, uint64_t *packed_out, uint64_t *invalid_out, uint64_t *n_positions_out) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    if (seg >= sp->segs.size()) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_read_segment: segment %llu of %zu", (unsigned long long)seg, sp->segs.size());
    const KsSegment &s = sp->segs[seg];
    if (n_positions_out) *n_positions_out = s.tiles * KDF_TILE;
    if (!packed_out && !invalid_out) return KDF_OK;
    KSCHK(sp, hipSetDevice(sp->device));
    if (sp->have_last) KSCHK(sp, hipEventSynchronize(sp->last));
    const hipMemcpyKind kind = s.host ? hipMemcpyHostToHost : hipMemcpyDeviceToHost;
    if (packed_out) KSCHK(sp, hipMemcpy(packed_out, s.packed, (2 * s.tiles + 4) * 8, kind));
    if (invalid_out) KSCHK(sp, hipMemcpy(invalid_out, s.mask, (s.tiles + 2) * 8, kind));
    return KDF_OK;
}

int kdf_spool_replay(kdf_spool *sp, kdf_engine *h, int mode) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    if (!h) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_replay: NULL engine");
    if (mode < 0 || mode > 2) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_replay: mode %d (0 count, 1 count --if, 2 prefilter tally)", mode);
    return spool_walk(sp, h, mode);
}

int kdf_spool_sketch(kdf_spool *sp, kdf_engine *h) {
    if (!sp) return ks_fail(nullptr, KDF_ERR_INVALID, "NULL spool");
    if (!h) return ks_fail(sp, KDF_ERR_INVALID, "kdf_spool_sketch: NULL engine");
    if (!h->sk.on) return ks_fail(sp, KDF_ERR_STATE, "kdf_spool_sketch: no sketch is on (kdf_sketch_begin)");
    return spool_walk(sp, h, 3);
}

}  // extern "C"
