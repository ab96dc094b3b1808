// kdf_engine_priv.h -- what the units of libkdf.so share of the engine (host only, no kernel): kdf_engine.hip (the
// core, which defines every function declared here unless noted), kdf_engine_reads.hip, kdf_kmerfasta.hip, kdf_fastafeed.hip, kdf_fastqfeed.hip, kdf_indexcodec.hip and kdf_spool.hip.  Nothing
// here is exported: include/kdf.h is the library's interface.
//
// One kernel, one unit: a __global__ function is compiled by exactly one unit (a non-template kernel in a header two
// units include would not link, a template instantiated by two would double its device code).  So this header pulls in
// no kernel header -- the structs of engine state that kernels take by value are in kdf_device.h -- and a kernel that a
// second unit needs gets a host launcher declared below (kh_scan_launch).
#pragma once
#include <cstddef>
#include <cstdint>

// Where the temporary device copies of ONE host-form call lie in the engine's staging arena: items side by side in
// registration order, each at a multiple of 256 bytes (what hipMalloc gave the separate buffers this replaces).  Plain
// C++, no HIP call: a host compiler includes this part of the header alone (tests/native/stage_layout_check.cpp).
struct StageLayout {
    enum : size_t { ALIGN = 256 };
    enum { MAX_ITEMS = 24 };                         // (the largest host form, kdf_variant_windows, registers 18)
    size_t off[MAX_ITEMS], size[MAX_ITEMS], total = 0;
    int n = 0;
    int add(size_t bytes) { off[n] = total; size[n] = bytes; total += (bytes + ALIGN - 1) / ALIGN * ALIGN; return n++; }
    // an item of 0 bytes is legal and has no address
    void *at(void *base, int i) const { return size[i] ? (char *)base + off[i] : nullptr; }
};

#if defined(__HIP__)                         // everything below needs the HIP runtime
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "kdf.h"
#include "kdf_device.h"
#include "kdf_hostutil.h"

struct KbPass;                            // kdf_binned.h (the core)

#define KDF_MERGE_MIN_PAIRS (1u << 16)
enum { PF_OFF = 0, PF_TALLYING = 1, PF_ARMED = 2 };      // stat "prefilter_state"
// the timers of kdf_profile (EvTimer); stats "<name>_us" / "<name>_passes", the stream timer through kdf_profile_read
enum { T_STREAM = 0, T_PF, T_PFM, T_DEPTH, T_HITS, T_SK, T_HISTO, T_COV, T_VAR, T_BD_INF, T_BD_WALK, T_BD_PACK, T_JOIN, T_REG, T_KF, T_FA, T_IX, T_FQ, T_FX, T_COUNT };
static const char *const TIMER_NAME[T_COUNT] = {nullptr, "prefilter", "prefilter_merge", "depth", "hits", "sketch", "histo", "coverage", "variants", "bamdev_inflate", "bamdev_walk", "bamdev_pack", "join", "regions", "kmerfasta", "fastafeed", "indexcodec", "fastqfeed", "fastqextract"};
// The entry ring: A0/A1/B append a partitioned pass per call; kernel C applies all pending passes at once when the
// table is needed or the ring is full (kb_flush_ring).  Reserved by upper bounds (one entry per stream position), so no
// host round trip sits between the stages.  Host only: what the kernels take of it is KbPlan (kdf_device.h).
struct KbRing {
    uint64_t cap_entries = 0, cap_rows = 0;          // capacity: entries (8 B x kw each), rows (pieces); kept over reset()
    uint64_t used_entries = 0, used_rows = 0;        // reserved by the pending passes
    uint32_t n_pass = 0;
    uint32_t n_dumped = 0;                           // pending passes a dump-only flush has applied: kept for the table, reported as flushed
    uint64_t positions = 0;                          // stream positions of the pending passes (upper bound of their entries)
    uint64_t dumped_positions = 0;                   // ... and of the first n_dumped of them
    uint64_t acct_entries = 0, acct_positions = 0;   // what of the pending passes dens_windows / dens_positions already hold
    KbPlan plan{};                                   // geometry (c1, c2, key slice) the pending passes were partitioned with
    bool filtered = false;                           // the pending passes are count --if passes
    bool empty() const { return n_pass == 0; }
    uint32_t undumped_passes() const { return n_pass - n_dumped; }                 // not yet applied by any flush
    uint64_t undumped_positions() const { return positions - dumped_positions; }
    // the only place the ring is emptied (kb_ring_reset: with the flush-wide device counters); plan / filtered are set by the next first pass
    void reset() { used_entries = used_rows = 0; n_pass = n_dumped = 0; positions = dumped_positions = 0; acct_entries = acct_positions = 0; }
};
// L1: small insert batches are concatenated (packed) in a pending stream first; the partition runs over ~2^30 positions
struct KbPendStream {
    DevBuf packed, mask;                             // uint64_t words: cap_tiles tiles of each (l1_append grows the pair together)
    uint64_t cap_tiles = 0, tiles = 0;
    uint64_t positions() const { return tiles * KDF_TILE; }
    uint64_t take() { const uint64_t n = positions(); tiles = 0; return n; }      // the stream is handed on (packed, mask: n positions) and empty again
};
// The request a dump hands to the LAST flush before it, and what came of it.  It lives on the dump's stack (export_pass):
// a flush that was not handed one cannot write a dump.
struct KbDump {
    uint32_t min_count = 0; uint64_t *lo = nullptr, *hi = nullptr; uint32_t *cnt = nullptr; uint64_t cap = 0;     // the request
    bool done = false; uint64_t n = 0;                                                                             // the result: written whole, n keys
};

// ---- the engine's state, by feature.  Every allocation is a DevBuf / PinBuf member (kdf_devbuf.h) named for what it holds:
// it is reserved where it is used (eng_reserve, dev_reserve, alloc) and freed when the engine goes (kdf_destroy drains the
// streams, then deletes the engine).  The structs kernels take by value (KdfTable, KbScratch, KdfPrefilter, KdfSketch) are
// views filled from these owners. ----
struct TableMem { DevBuf lo, hi, cnt; };             // the arrays of one table: keys (hi: words 1 .. W-1 of wide and long keys), counts
// binned (LDS-bucket) path (kdf_binned.h)
struct KbState {
    DevBuf ent, tmp;                                 // the ring's entries; the slab-sorted pass
    DevBuf chunk_off, failed, off_rows, pass_plan;   // the ring's offset rows, the bitmap of failed buckets; a pass's offset rows and planning arrays
    DevBuf row_tables, bin_runs;                     // row_ent u64 | row_len u32, ring.cap_rows of each; bin-major runs (bin sieve)
    DevBuf small, pass, heavy;                       // totals[16] then trash[64]; [KB_MAX_PASS] pass descriptors; heavy buckets of skewed flushes (kb_heavy_slice_kernel)
    PinBuf totals_host;                              // [16]
    uint64_t total(int i) const { return totals_host.as<unsigned long long>()[i]; }
    KbRing ring;                                     // the pending passes (above)
    KbPendStream l1;                                 // small insert batches waiting to be partitioned (above)
    bool attrs_set[4] = {false, false, false, false};   // hipFuncSetAttribute done (per key width)
};
// blocked Bloom filter over the filter keys (count --if, scan)
struct SieveState {
    DevBuf buf; uint64_t words = 0;                  // uint64_t words (grow-only); those of the sieve in use
    bool valid = false, unfit = false;               // unfit: long_sieve_ensure found the table's keys too many for a sieve: not asked again
                                                     // until the keys, the filter or the sizing options change (sieve_drop)
};
// count --if through the bin-major sieve (kdf_binsieve.h; option "sieve_bins" / env KDF_SIEVE_BINS: 0 off, 1 the sizing rule's
// coarse bits, 4 .. 10 exactly those): an allocation of its own, built from the table by the first eligible count --if
// (bin_sieve_ensure) and dropped with the other sieve (sieve_drop) and when sieve_bits / sieve_bins change
struct BinSieveState {
    DevBuf buf; uint32_t c1 = 0, slice_words = 0;    // uint64_t [2^c1][slice_words] (grow-only)
    bool valid = false, unfit = false;               // unfit: the sizing rule refused the table's keys (not asked again until a drop)
    bool attr_set[3] = {false, false, false};        // kdf_bin_sieve_kernel's LDS limit raised (per key width)
};
// two-pass counting (kdf_prefilter.h): off -> begin -> tallying -> arm -> armed -> drop -> off
struct PfState {
    int state = PF_OFF;
    KdfPrefilter view{};                             // the sieve (words), its size and the gate's threshold
    DevBuf words, ctr;                               // the counting sieve; sharded counter of tallied windows [KDF_SHARDS * 16], then 3 words of kdf_pf_fill_kernel
    DevBuf admit;                                    // the gate's output for the stream being counted, one word per tile (grow-only)
    uint64_t merged_words = 0;                       // words written by kdf_prefilter_merge* since kdf_prefilter_begin (stat "prefilter_merged_words")
};
// distinct k-mer sketch (kdf_sketch.h): independent of the table, the mode, the prefilter and the stream
struct SkState {
    bool on = false;
    KdfSketch view{};                                // the register cells and p
    DevBuf cells, bytes;                             // bytes: 2^p of them, the exported form on its way out / a merge's input
    DevBuf ctr;                                      // sharded counter of sketched windows [KDF_SHARDS * 16]
};
// double-buffered feeding (kdf_upload_reads_async / kdf_count_uploaded): two device staging slots filled on a copy
// stream of their own, so the H2D copy of batch i + 1 runs under the count of batch i
struct UpSlot {
    DevBuf packed, mask; uint64_t n_bases = 0; bool valid = false;
    hipEvent_t up_done = nullptr, use_done = nullptr;    // the copy into the slot; the consumer that last read it
};
struct UpState { UpSlot slot[2]; hipStream_t copy_stream = nullptr; };
// grow-only scratch kept between calls, per consumer
struct HitScratch { DevBuf mask, block_sums, positions, pair_set; };   // kdf_hits.h: hit mask (caller gave none), block sums, hit positions, the (read, slot) set
struct CovScratch { DevBuf cigar_pre; };                               // kdf_coverage.h: CIGAR prefix sums
struct VarScratch { DevBuf cigar_pre, ranges, cand_counts; };          // kdf_variants.h: CIGAR prefix sums, per-read ranges, per-candidate counts and flags
struct RegScratch { DevBuf scratch, perm; };                           // kdf_regions.h: the sort's top key word, block maxima and boundary flags; the permutation
struct KfScratch { DevBuf block_sums; };                               // kdf_kmerfasta.h: block sums of the record scan and its counters
struct FaScratch { DevBuf scratch; };                                  // kdf_fastafeed.h: tile summaries, tile offsets and the control words
struct IxScratch { DevBuf pos, ctl; };                                 // kdf_indexcodec.h: hash positions of kdf_jf_order; the first bad record of a decode
struct FqScratch { DevBuf scratch; };                                  // kdf_fastqfeed.h: control words, tile counts, line ends, record offsets, block sums, the word index (kdf_fq_extract: the output tiles' records)
struct BdState {                                                       // device BAM feeder (kdf_bamdev.h)
    DevBuf inflated, status, read_offs;              // inflated span; block / sub-range status, counts, bases and totals; per-read sequence offsets
    // 1: every block of a batch is inflated by zlib and patched in as if the device decoder had rejected it (option
    // "bamdev_host_inflate": tells a decoder fault from a file fault, and lets the tests walk the patch path, which no file zlib wrote takes)
    int opt_host_inflate = 0;
    uint64_t stat_fallback = 0;                      // blocks the device decoder rejected and zlib inflated (stat "bamdev_fallback_blocks")
};
struct MergeState {                                  // kdf_merge.h
    DevBuf scratch;                                  // block counts / offsets of the ordered dump, bucket ranges of a merge (sized exactly); the payload of a sorted join without counts
    uint32_t flag_host = 0; int last_path = 0;       // last_path: 0 none yet, 1 LDS bucket merge launched, 2 plain atomic insert
    bool attrs_set[3] = {false, false, false};       // km_merge_kernel's LDS limit raised (big buckets)
};

struct kdf_engine {
    int device = 0;
    int k = 0;
    int kw = 1;                   // key words: 1 narrow, 2 wide, 3..7 long (kdf_long.h)
    int n_cu = 256;               // compute units of the device (persistent-kernel grids)
    uint64_t dev_total_bytes = 0; // HBM of the device (sizes the entry ring's budget)
    TableMem t_mem;               // the live table's arrays ...
    KdfTable t{};                 // ... and the view of them that kernels take
    uint64_t cap = 0;
    DevBuf ctl_mem, out4_mem; PinBuf out4_pin;      // the control block, ctl readback scratch (device) and its pinned host mirror, seen through:
    KdfCtl *ctl = nullptr; unsigned long long *d_out4 = nullptr, *h_out4 = nullptr;
    hipStream_t own_stream = nullptr, stream = nullptr;      // stream: the one in use (kdf_set_stream), own_stream unless the caller gave one
    uint64_t distinct = 0;        // host mirror after the last sync
    uint64_t windows = 0;
    bool filter_mode = false;
    bool lazy_empty = false;      // logically empty, HBM slices not yet reset (see kdf_clear)
    bool zero_keys = false;       // the table may hold keys with count 0 (a filter, added pairs, reset / set counts): kdf_histo.h
    uint64_t capacity_hint = 0;   // kdf_create's: sizes the prefilter's sieve when the caller leaves that to the engine
    DevBuf arena;                                    // the staging of the host forms: laid out per call by a HostCall (below), touched by nothing else
    const char *arena_user = nullptr;                // the host form whose HostCall is open (commit() .. its destructor), else NULL
    // ---- the features' state (above) ----------------------------------------------------------------------------------
    KbState kb; SieveState sieve; BinSieveState bsv; PfState pf; SkState sk; UpState up;
    HitScratch hits; CovScratch cov; VarScratch var; RegScratch reg; KfScratch kf; FaScratch fa; IxScratch ix; FqScratch fq; BdState bd; MergeState merge;
    // ---- options, statistics and what the last call did ------------------------------------------------------------------
    uint64_t stat_flushes = 0;
    double grow_ratio = 0.0;                         // new distinct keys per counted window at the last flush (0: unknown)
    uint64_t dens_windows = 0, dens_positions = 0;   // valid windows / stream positions of every pass this engine has flushed: sizes the piece groups
    uint32_t opt_key_parts = 0, opt_key_part = 0;    // count only one slice of the key space (KdfTable::key_parts)
    uint64_t opt_binned_min_positions = 1ull << 22;  // fewer pending positions at flush time use the direct global-table kernels
    uint64_t opt_binned_bytes_per_position = 70;     // ... and so does a flush of fewer than table_bytes / 70 positions (use_binned)
    uint64_t opt_binned_max_positions = 1ull << 31;  // longer streams are partitioned in several passes
    uint32_t opt_binned_filtered_min_log2cap = 23;   // count --if goes binned from 2^23 slots (measured crossover)
    uint32_t opt_big_bucket_log2cap = 32;            // tables from 2^32 slots on have buckets of twice the slots (KDF_BIG_BUCKET_LOG2CAP / option big_bucket_log2cap)
    uint64_t opt_merge_min_pairs = KDF_MERGE_MIN_PAIRS;   // below this many pairs a merge goes straight to the atomic insert (tests lower it)
    uint32_t opt_hash_shift = 0;                     // KdfTable::hshift of the tables this engine creates (owner tables)
    int opt_force_path = 0;                          // 0 auto, 1 direct, 2 binned, 4 sieve only (count --if)
    int opt_defer = 1;                               // 1: kernel C is deferred over the pending passes; 0: every count call ends with a flush
    uint64_t opt_defer_max_bytes = 0;                // budget of the entry ring (0: 40 % of the device's memory)
    // 1 (the default): a dump (min_count >= 1, caller-sized device buffers) asked for while passes are pending is written by the
    // flush itself -- kernel C holds every bucket anyway (kb_bucket_kernel<.., DUMP>), and the dump's pass over the table is
    // saved.  Option "fused_dump" / env KDF_FUSED_DUMP=0 turn it off; long engines have no binned pipeline: 0
    int opt_fused_dump = [] { const char *e = getenv("KDF_FUSED_DUMP"); return e ? atoi(e) != 0 : 1; }();
    uint64_t stat_fused_dumps = 0;
    // 1 (the default): such a dump into a table that is still only logically empty (kdf_clear, nothing applied since) runs the
    // DUMP-ONLY flush -- kb_bucket_kernel<.., DUMP, LAZY> writes the dump and the ctl counters and leaves the table alone.  The
    // passes stay in the ring (KbRing: the first n_dumped of n_pass); whatever needs the table later applies them with the ordinary
    // flush, into the still empty table.  Option "lazy_table" / env KDF_LAZY_TABLE=0 turn it off.
    int opt_lazy_table = [] { const char *e = getenv("KDF_LAZY_TABLE"); return e ? atoi(e) != 0 : 1; }();
    uint64_t stat_dump_only = 0, stat_materialisations = 0;
    uint64_t opt_l1_positions = 1ull << 30;          // pending-stream size from which it is partitioned
    uint64_t opt_l1_direct_positions = 1ull << 28;   // batches from this size on are partitioned where they lie (no copy)
    uint64_t stat_heavy_buckets = 0;
    int opt_sieve_bits = 0;                          // sieve bits per filter key (0: 32 up to 2^20 keys, 16 beyond)
    // long engines take the sieve only when asked to (option "long_sieve" / env KDF_LONG_SIEVE=1; k <= 63: always): their
    // count --if and scan then go through kdf_long_sieve_kernel (kdf_long_sieve.h)
    int opt_long_sieve = [] { const char *e = getenv("KDF_LONG_SIEVE"); return e ? atoi(e) != 0 : 0; }();
    int last_sieve_in_lds = 0;                       // the last sieve kernel read the sieve from LDS (1) or from L2 (0)
    int last_path = 0;                               // count path of the last count call: 0 direct, 1 binned, 3 sieve, 5 bin-major sieve
    int last_scan_path = 0;                          // kernel of the last kdf_scan_reads_dev: 0 direct, 3 sieve
    int opt_sieve_bins = [] { const char *e = getenv("KDF_SIEVE_BINS"); const int v = e ? atoi(e) : 0; return v == 1 || (v >= 4 && v <= 10) ? v : 0; }();   // BinSieveState
    uint32_t last_sieve_bins = 0, last_sieve_slice_words = 0;
    uint64_t stat_bin_sieve_passes = 0;
    uint32_t last_sieve_rounds = 0;                  // tiles per thread of the last sieve kernel of a long engine (LDS form; L2 form: 1)
    uint32_t opt_debug_flags = 0;                    // experiments only (KbPlan::dbg)
    uint64_t stat_binned_passes = 0, stat_replayed_buckets = 0;
    // optional HIP-event timing (kdf_profile).  T_STREAM, the dominant kernels: a span's tag is its tiles, so passes are the
    // launches and tag_sum x 64 the positions (a flush is timed with tag 0: its positions were counted with the passes it
    // applies).  T_HITS: tag 1 for the span that opens a call, 0 for the second span of a call that finds hits.
    bool prof = false;
    EvTimer timer[T_COUNT];
    // binned path: events around each stage (A0 hist, A1 scatter, B finesort | C bucket)
    std::vector<std::vector<hipEvent_t>> prof_stage_ev;   // 4 events: a partition (A0, A1, B); 2 events: a flush (C)
    double prof_stage_ms[4] = {0, 0, 0, 0};
    uint64_t prof_stage_passes = 0;
    std::string err;
};

// ---- internal functions that more than one unit calls ----------------------------------------------------------------
#pragma GCC visibility push(hidden)
extern thread_local std::string g_err;    // the error text of calls without an engine or a spool
int fail(kdf_engine *h, int code, const char *fmt, ...);
// kdf_clear defers the table's memset: everything that reads or probes the table calls this first
int materialize(kdf_engine *h);
// everything pending (the concatenated small batches, the partitioned passes) goes into the table; dump: the LAST flush may write it
int pending_flush(kdf_engine *h, KbDump *dump = nullptr);
// room for `bytes` in one of the engine's buffers whose readers all run on the engine's stream
int eng_reserve(kdf_engine *h, DevBuf &b, size_t bytes, size_t (*slack)(size_t) = slack_8th, const char *what = nullptr);
// kdf_engine_reads.hip: kh_scan_kernel (kdf_hits.h) on stream s, for the spool's kdf_spool_select_reads
void kh_scan_launch(hipStream_t s, unsigned long long *sums, uint64_t n);
#pragma GCC visibility pop

// The staging of ONE host-form call, built on its stack: the form registers every host array it hands to its _dev form
// (in, stream) or gets back from it (out), commit() reserves the engine's arena once for all of them and copies the
// inputs to the device, dev() gives the _dev form its pointers, fetch() copies results back and finish() waits for them.
// All copies run on the engine's stream, in call order.  The arena belongs to the open frame: no code that a _dev entry
// point reaches touches it, and a second commit() before the first frame is gone is refused (KDF_ERR_STATE).
struct __attribute__((visibility("hidden"))) HostCall {
    kdf_engine *const h; const char *const fn;       // fn: the host form, for messages
    StageLayout lay;
    struct { const void *src; void *dst; uint64_t n_bases; } item[StageLayout::MAX_ITEMS];   // n_bases > 0: the packed half of a stream (the mask half follows)
    bool open = false;
    HostCall(kdf_engine *h_, const char *fn_) : h(h_), fn(fn_) {}
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;
    ~HostCall() { if (open) h->arena_user = nullptr; }
    int add(const void *src, void *dst, size_t bytes, uint64_t n_bases = 0) { const int i = lay.add(bytes); item[i] = {src, dst, n_bases}; return i; }
    int in(const void *src, size_t bytes) { return add(src, nullptr, bytes); }
    int out(void *dst, size_t bytes) { return add(nullptr, dst, bytes); }            // dst NULL: room only, the form copies by hand
    int inout(void *p, size_t bytes) { return add(p, p, bytes); }                    // an accumulator: copied in, fetched back
    // the padded stream of n_bases > 0 positions (upload_padded): the packed words' item, the mask words' is the next one
    int stream(const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases) {
        uint64_t pw, mw;
        kdf_stream_words(n_bases, &pw, &mw);
        const int i = add(packed, nullptr, pw * 8, n_bases);
        add(invalid, nullptr, mw * 8);
        return i;
    }
    template <typename T = void> T *dev(int i) const { return (T *)lay.at(h->arena.p, i); }
    int commit();
    int fetch(int i, size_t bytes);                  // the first `bytes` of output item i to its destination (it has none: nothing)
    int finish();                                    // the one synchronisation
};

#define HIPCHK(h, call)                                                                 \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(h, e_ == hipErrorOutOfMemory ? KDF_ERR_NOMEM : KDF_ERR_HIP,     \
                        "%s failed: %s", #call, hipGetErrorString(e_));                 \
    } while (0)

static inline uint32_t log2ceil(uint64_t x) { uint32_t l = 0; while ((1ull << l) < x) ++l; return l; }

// code for k <= 63 only (the binned pipeline, merge, sieve): W = 1 or 2
template <typename F>
static inline int by_width(kdf_engine *h, F &&f) { return h->kw == 1 ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 2>{}); }
// code for every key width: W = 1, 2 (kdf_device.h) or 3 .. 7 (long keys, kdf_long.h)
template <typename F>
static inline int by_words(kdf_engine *h, F &&f) {
    switch (h->kw) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 7>{});
    }
}
// long engines: W = 3 .. 7
static inline bool is_long(const kdf_engine *h) { return h->kw > 2; }
// bits of a long key's top word: 2k - 64 (W - 1), 2 .. 62 for odd k
static inline int long_top_bits(const kdf_engine *h) { return 2 * h->k - 64 * (h->kw - 1); }

// words per key of a host form's first key array: 1 for the (lo, hi) forms, W for the rows of the _w forms
static inline uint64_t lo_words(const kdf_engine *h) { return is_long(h) ? h->kw : 1; }

// The (lo, hi) key forms take k <= 63 engines only; a long engine names the W-word form to use instead.  The multi-GPU
// entry points are single-GPU-only for long keys.
#define KDF_REFUSE_LONG(h, fn, wfn) \
    do { if (is_long(h)) return fail(h, KDF_ERR_INVALID, "%s: k=%d takes %d-word keys: use %s", fn, (h)->k, (h)->kw, wfn); } while (0)
#define KDF_REFUSE_LONG_MULTI(h, fn) \
    do { if (is_long(h)) return fail(h, KDF_ERR_INVALID, "%s: not available for k > 63 (long keys count on one GPU)", fn); } while (0)

// ---------------------------------------------------------------------------
// Where a consumer's read stream comes from (count, count --if, prefilter tally, sketch, a spool's append): device
// pointers, host arrays or an upload slot.  Each maker holds its form's refusals, worded with the caller's name; an
// entry point is "refuse by state, make a source, run the _dev core, release".

struct StreamSrc { const uint64_t *packed = nullptr, *invalid = nullptr; uint64_t n_bases = 0; int slot = -1; };

// where the message of a refusal goes: this engine's error string (a spool has its own sink)
struct EngSink {
    kdf_engine *h;
    template <typename... A> int operator()(int code, const char *fmt, A... a) const { return fail(h, code, fmt, a...); }
};
struct NoRefusal { int operator()(const StreamSrc &) const { return KDF_OK; } };

#pragma GCC visibility push(hidden)
// behind the consumer's last launch: the slot's next upload waits for this reader
void src_release(kdf_engine *h, const StreamSrc &src);
#pragma GCC visibility pop

// The batch of upload slot `slot` (kdf_upload_reads_async), or KDF_ERR_STATE.  also_refuse(src) holds the refusals the
// caller tests AFTER the slot's: a refused call changes nothing, the slot keeps its batch.  consume: the slot is empty
// afterwards (count, tally), else it keeps the batch for the next consumer (sketch, spool).  The engine's stream waits for
// the copy; host_wait: so does the host -- the caller of a count, tally or sketch recycles its (pinned) source buffer as
// soon as the call returns, and the copy was issued a whole batch ago.  An empty batch (n_bases 0) needs no wait.
template <typename S, typename R>
static int src_slot(S &&sink, const char *fn, kdf_engine *h, int slot, bool consume, bool host_wait, StreamSrc &src, R &&also_refuse) {
    if (slot < 0 || slot > 1 || !h->up.slot[slot].valid) return sink(KDF_ERR_STATE, "%s: nothing was uploaded into slot %d", fn, slot);
    const UpSlot &up = h->up.slot[slot];
    src = StreamSrc{up.packed.as<const uint64_t>(), up.mask.as<const uint64_t>(), up.n_bases, slot};
    if (const int rc = also_refuse(src)) return rc;
    if (consume) h->up.slot[slot].valid = false;
    if (src.n_bases == 0) return KDF_OK;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, up.up_done, 0);
    if (e == hipSuccess && host_wait) e = hipEventSynchronize(up.up_done);
    if (e != hipSuccess) return sink(e == hipErrorOutOfMemory ? KDF_ERR_NOMEM : KDF_ERR_HIP, "%s: waiting for the copy into slot %d failed: %s", fn, slot, hipGetErrorString(e));
    return KDF_OK;
}
#endif  // __HIP__
