/*
 * kdf.h -- C ABI of the MI355X-native canonical k-mer count / filter / probe
 * engine (libkdf.so).  This is the drop-in boundary for the one hot path of
 * jlanej/kmer_denovo_filter; every entry point names the reference interface
 * it replaces (file:line relative to the reference repository root).
 *
 * The reference has no FFI: the path sits behind Python helper functions that
 * spawn `samtools fasta | jellyfish count [-C --if] ; jellyfish dump/query`.
 * A maintainer binds this header with ctypes (INTEGRATION.md shows the stub);
 * kmer_denovo_filter_amd/_native.py is that binding.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross the boundary.
 *   - every function returns 0 on success or a KDF_ERR_* code; the message is
 *     kdf_last_error(h) (or kdf_last_error(NULL) for create/IO failures).
 *     The Python mirror raises RuntimeError, matching the reference's
 *     RuntimeError("jellyfish ... failed: ...") convention
 *     (core/jellyfish_wrappers.py:239-242, discovery/pipeline.py:168-172).
 *   - the caller owns host buffers; the engine owns device memory.
 *   - one engine = one GPU = one table; a handle is not thread-safe.
 *   - keys are canonical k-mers in the Jellyfish encoding: 2 bits per base,
 *     A=0 C=1 G=2 T=3, leftmost base most significant, canonical = numeric min
 *     of the k-mer and its reverse complement (== kmer_utils.canonicalize,
 *     src/kmer_denovo_filter/kmer_utils.py:35-38).  k <= 32: one uint64 (lo);
 *     33 <= k <= 63: (lo, hi) pair.  `hi` arrays may be NULL when k <= 32.
 *   - long keys, odd k from 65 to 201 (utils.py:299-311 accepts any odd k up to
 *     201): W = ceil(2k/64) = 3..7 words per key, ROW-MAJOR (key i is words
 *     [i*W, i*W + W)), word 0 the least significant 64 bits.  Engines for such k
 *     take the `_w` entry points below; their (lo, hi) forms return
 *     KDF_ERR_INVALID and name the `_w` form.  The read-stream entry points
 *     (count / count --if / scan / window counts / read depth, host or device, the double-buffered upload)
 *     work unchanged for every k.  A long engine counts through the direct
 *     kernels (no binned pipeline or fused dump: force_path 2 / 4 and
 *     fused_dump 1 are KDF_ERR_INVALID; count --if and the scan go through the
 *     membership sieve only under option "long_sieve").  Across ranks a long engine has its own owner
 *     exchange (kdf_export_parts_w_packed_dev, kdf_set_counts_w_dev, "long keys" below); kdf_export_parts*,
 *     kdf_add_pairs_multi_dev, kdf_set_counts_dev and hash_shift stay KDF_ERR_INVALID.
 *
 * Read streams
 *   Reads are handed over as ONE 2-bit-packed base stream plus a 1-bit
 *   "invalid" mask.  Base i lives in bits 2*(i%32) of packed[i/32]; bit (i%64)
 *   of invalid[i/64] is set when position i is not A/C/G/T (N, IUPAC) or is the
 *   single separator position that kdf_pack_reads() inserts after every read,
 *   so that no window spans two records (Jellyfish: windows never span FASTA
 *   records).  A window [i, i+k) is counted iff none of its k positions is
 *   invalid.  This keeps the kernels free of per-read bookkeeping and load
 *   balanced for ragged reads.
 *
 *   What lies at and past n_bases (every entry point that takes a stream, host or device, every k, every path):
 *   1. a position >= n_bases is INVALID whatever the caller's buffers hold there -- the bits of the last mask word
 *      past n_bases % 64, the 2 padding mask words and 4 padding packed words that kdf_stream_words(n_bases) adds,
 *      the bases of the last packed words past n_bases.  A producer may pad with zeros or hand over a prefix of a
 *      longer stream (any n_bases, also one that cuts a read): no window reaches past n_bases.
 *   2. the device forms read at most the kdf_stream_words(n_bases) words of each buffer, so the buffers need be no
 *      longer than that; the host forms read ceil(n_bases / 32) packed and ceil(n_bases / 64) mask words.  The engine
 *      never writes to a caller's stream.
 *   3. kdf_scan_reads*: in hit words 0 .. ceil(n_bases / 64) - 1 every bit at a position > n_bases - k is 0.  The valid
 *      words of kdf_window_counts* follow the same rule, and kdf_window_counts* / kdf_read_depth* see no window there.
 *   4. kdf_stats' `windows` counts only windows that lie wholly below n_bases.
 */
#ifndef KDF_H
#define KDF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KDF_OK               0
#define KDF_ERR_INVALID      1   /* bad argument (k out of range, NULL pointer ...) */
#define KDF_ERR_HIP          2   /* HIP runtime error; message carries hipGetErrorString */
#define KDF_ERR_NOMEM        3   /* host or device allocation failed */
#define KDF_ERR_TABLE_FULL   4   /* a bucket overflowed: never silent, grow and redo */
#define KDF_ERR_IO           5   /* file open/read/format error (BAM/FASTA/.jf) */
#define KDF_ERR_STATE        6   /* call not valid in the engine's current mode */

typedef struct kdf_engine kdf_engine;
typedef struct kdf_reader kdf_reader;

/* ---------------------------------------------------------------- engine -- */

/* Create an engine on HIP device `device` for k-mers of length k (1..63, or odd 65..201) with
 * room for at least capacity_hint distinct keys before the first grow.
 * Replaces the process launch + `-m k -s SIZE` of `jellyfish count`
 * (core/jellyfish_wrappers.py:167-176,313-321; discovery/pipeline.py:114-122). */
int kdf_create(int device, int k, uint64_t capacity_hint, kdf_engine **out);
void kdf_destroy(kdf_engine *h);
const char *kdf_last_error(const kdf_engine *h);

/* Use an externally created hipStream_t (e.g. torch's current stream) for all
 * subsequent launches; NULL restores the engine's own stream.  Pending count work is applied and the old stream
 * synchronised first, so nothing of the engine's is left in flight on it; table, mode, options, upload slots and the
 * prefilter (tallying or armed) carry over unchanged. */
int kdf_set_stream(kdf_engine *h, void *hip_stream);
int kdf_synchronize(kdf_engine *h);

/* Empty the table (all keys and counts dropped): `windows` is 0, the engine is back in insert mode (a loaded filter is
 * gone), pending count work is dropped.  Options keep their values, and so do the upload slots and the prefilter:
 * cleared while TALLYING it goes on tallying with the tallies it has, cleared while armed it stays armed. */
int kdf_clear(kdf_engine *h);
/* Make room for at least n_keys distinct keys (rehashes the live entries).  Pending count work is applied first; the
 * contents, `windows` and the mode do not change, and a table never shrinks. */
int kdf_reserve(kdf_engine *h, uint64_t n_keys);
/* capacity in slots, distinct keys currently stored, valid windows processed
 * by the count calls since the last clear.  Any pointer may be NULL.  Answers from the counters of a dump-only
 * flush (option "lazy_table") without materialising the table. */
int kdf_stats(kdf_engine *h, uint64_t *capacity, uint64_t *distinct, uint64_t *windows);

/* Count calls in insert mode are DEFERRED: a call partitions its batch (or, for small batches, only appends it to a
 * pending stream) and returns; the table itself is updated when something reads it -- kdf_stats, kdf_query*,
 * kdf_count_ge, kdf_histogram*, kdf_count_stats, kdf_export_*, kdf_scan_*, kdf_read_hits*, kdf_window_counts*,
 * kdf_read_depth*, kdf_add_pairs*, kdf_reserve, kdf_set_option
 * -- or when the pending work fills its budget, so that a sample streamed in hundreds of batches pays the table rewrite of the binned pipeline
 * once per flush, not once per batch (`jellyfish count` over the whole `samtools fasta` pipe,
 * discovery/pipeline.py:106-172).  Such a call runs in stream order and does not synchronise.  A count that goes through
 * the direct kernels is not deferred -- option force_path 1, every long engine, an owner table (hash_shift), a table of a
 * single bucket -- and it SYNCHRONISES the engine's stream after every chunk it inserts: the host must learn the number
 * of distinct keys to grow the table before the next chunk.  kdf_flush applies everything pending now; errors of deferred work (a table that
 * cannot grow ...) surface there or in the call that triggered the flush.  kdf_clear drops pending work. */
int kdf_flush(kdf_engine *h);

/* Tuning knobs and counters (tests force either kernel path through these):
 *   options  "force_path" 0 auto / 1 direct global-table kernels / 2 binned LDS-bucket pipeline (every count call
 *            partitions its batch at once) / 4 count --if through the sieve only -- any other value is refused with
 *            KDF_ERR_INVALID and the option keeps its value; "binned_min_positions" (pending
 *            positions below which a flush uses the direct kernels); "key_parts" / "key_part" (count only
 *            the windows whose key lies in slice key_part of key_parts of the key space --
 *            ranges of the LOW 16 hash bits, so a slice spreads over the whole table -- so that
 *            a sample whose distinct k-mers exceed one table is counted slice by slice over
 *            the same stream; insert mode only; 0/1 = everything); "binned_max_positions" (positions per
 *            partition pass, <= 2^31: longer streams take several passes); "binned_filtered_min_log2cap";
 *            "sieve_bits" (bits per filter key; 0 = by size); "long_sieve" (k > 63 only, KDF_ERR_INVALID otherwise; 0 default,
 *            env KDF_LONG_SIEVE=0 / 1 sets the default; 1: kdf_count_reads_filtered* and kdf_scan_reads* of a long engine go through
 *            the membership sieve where the keys fit one, "last_count_path" / "last_scan_path" 3 -- the sieve is built by
 *            kdf_load_filter_w*, or from the table by the next count --if or scan when there is none, and dropped when keys
 *            join the table; force_path 1 keeps the direct kernels; 0 drops the sieve); "sieve_bins" (k <= 63; 0 default, env
 *            KDF_SIEVE_BINS sets the default; 1, or 4 .. 10 = exactly that many coarse bits; anything else, and any non-zero value
 *            on a k > 63 engine, is KDF_ERR_INVALID: kdf_count_reads_filtered* and every caller that ends there go through the
 *            BIN-MAJOR sieve -- the stream is slab-sorted by its top hash bits and one workgroup per bin tests the bin's entries
 *            against its slice of the sieve in LDS, "last_count_path" 5 -- under force_path 0, without hash_shift, when
 *            kdf_bin_sieve_geometry accepts the filter; otherwise the selection is what it is with 0, silently.  It wins over
 *            the other sieve; it is built from the table by the first such call and dropped where that one is, and when
 *            "sieve_bits" or "sieve_bins" change; the call is eager, pending binned passes are flushed first);
 *            "binned_bytes_per_position" (a flush goes
 *            binned only when pending positions x this >= table bytes: kernel C rewrites the whole table; default 70);
 *            "defer" (1 default; 0: every count call ends with a flush), "defer_max_bytes" (budget of the ring of
 *            partitioned entries, 0 = 40 % of the device's memory), "l1_positions" (size from which the pending
 *            stream of small batches is partitioned, default 2^30), "l1_direct_positions" (batches from this size on
 *            are partitioned where they lie, default 2^28); "fused_dump" (1 default, 0 for k > 63; 1: kdf_export_ge_dev with min_count >= 1
 *            called while partition passes are pending is written by the flush that applies them -- kernel C dumps every
 *            bucket it holds -- instead of by a pass over the table afterwards; falls back to that pass when a bucket
 *            overflowed or was split as heavy, same entries in another order; 0: always that pass; env KDF_FUSED_DUMP=0 / 1 sets the default);
 *            "lazy_table" (1 default, 0 for k > 63; 1: such a fused dump into a table that is still empty since kdf_clear writes the dump
 *            and the counters only -- the table is materialised, from the passes kept in the ring, by the first call that reads or
 *            changes it; 0: the flush writes the table as well; env KDF_LAZY_TABLE=0 / 1 sets the default);
 *            "hash_shift" (0..8: the home slot ignores that many top hash bits -- the table of an OWNER rank of the
 *            multi-GPU merge, see kdf_add_pairs_multi_dev; such an engine counts through the direct kernels only.  It
 *            changes on an empty table only, KDF_ERR_STATE otherwise: a table is empty after kdf_clear and after
 *            kdf_load_filter* of zero keys, and is not while it holds keys whose counts kdf_reset_counts zeroed);
 *            "merge_min_pairs" (below this many pairs kdf_add_pairs* skips the bucket merge);
 *            "big_bucket_log2cap" (default 32; KDF_BIG_BUCKET_LOG2CAP: tables of 2^that slots and more have buckets of
 *            twice the slots -- an internal layout: dumps, queries and index files do not depend on it; a live table
 *            is re-bucketed when the option changes its bucket size); "debug_flags" (experiments: 64 one piece per
 *            workgroup in the piece sort, 2048 partition without the bucket kernel, 4096 force the skew instantiation,
 *            8192 long_sieve's LDS form on a grid of two workgroups: small streams take several rounds).
 *            Environment, read when a partition is planned (experiments: DESIGN.md section 3.2 has what they measured):
 *            KDF_C1 (coarse bits of the partition), KDF_PIECE_FILL (how full the pieces are planned, default 0.98)
 *   stats    "binned_passes" (partition passes), "flushes" (kernel C launches), "pending_passes",
 *            "pending_positions", "ring_bytes", "replayed_buckets", "heavy_buckets" (buckets of skewed flushes that
 *            were shared by several workgroups), "log2cap", "bucket_bits", "c1" / "c2" (coarse / fine bits of the partition), "hash_shift", "defer", "fused_dump", "fused_dumps" (dumps written by a flush),
 *            "lazy_table", "dump_only_flushes" (flushes that wrote a dump and no table), "retained_passes" (passes such a flush applied,
 *            kept for the table: no longer "pending_passes"), "materialisations" (tables written later from retained passes),
 *            "last_count_path" (0 direct / 1 binned / 3 sieve / 5 bin-major sieve), "sieve_bins" (the option), "last_sieve_bins" /
 *            "last_sieve_slice_words" (coarse bits and words per bin of the last bin-major sieve call), "bin_sieve_passes" (its
 *            passes so far), "last_scan_path" (0 direct / 3 sieve), "last_sieve_in_lds" (the last
 *            sieve kernel, count --if or scan, read the sieve from LDS: 1, or from L2: 0), "last_sieve_rounds" (long engines: tiles per
 *            thread of that kernel, 1 for the L2 form), "long_sieve" (the option; 0 for k <= 63), "last_merge_path" (1 LDS bucket
 *            merge, 2 global atomics); "histo_us" / "histo_passes" (kdf_histo_kernel under kdf_profile);
 *            "join_us" / "join_passes" (the join kernels of kdf_count_join / kdf_export_join* under kdf_profile);
 *            "depth_us" / "depth_passes" (kdf_depth_kernel under kdf_profile: kdf_window_counts* / kdf_read_depth*);
 *            "hits_us" / "hits_passes" (the kh_* kernels of kdf_read_hits* / kdf_hit_list* under kdf_profile, the scan kernel
 *            not included; one pass per call); "coverage_us" / "coverage_passes" (the kc_* kernels of kdf_hit_coverage* /
 *            kdf_coverage_list* under kdf_profile); "variants_us" / "variants_passes" (the kv_* kernels of
 *            kdf_variant_windows* / kdf_variant_evidence* under kdf_profile); "trash0" .. "trash63" (phase cycle sums of -DKB_TIMING variant builds) */
int kdf_set_option(kdf_engine *h, const char *name, int64_t value);
/* Free / total HBM of a device (hipMemGetInfo): the child-count mirror sizes "key_parts" with it. */
int kdf_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);
int kdf_get_stat(kdf_engine *h, const char *name, int64_t *value);

/* Measurement hook (bench.py): when enabled, every launch of the dominant
 * stream kernel is bracketed by HIP events on the launch stream.
 * kdf_profile_read returns the summed kernel milliseconds, the number of
 * launches and the stream positions they covered since kdf_profile(h, 1). */
int kdf_profile(kdf_engine *h, int enable);
int kdf_profile_read(kdf_engine *h, double *kernel_ms, uint64_t *launches, uint64_t *positions);
/* Binned passes only: summed milliseconds of the four stages (A slab sort, the
 * planning kernels, B piece sort, C bucket kernel) and the number of passes. */
int kdf_profile_stages(kdf_engine *h, double *stage_ms4, uint64_t *passes);

/* ------------------------------------------------- count (insert) stage -- */

/* `jellyfish count -m k -C` over a read stream: every valid window's canonical
 * k-mer is inserted / incremented (saturating uint32, like Jellyfish's 4-byte
 * output counter).  Replaces the counting half of
 * _extract_child_kmers_discovery (discovery/pipeline.py:114-172) and of
 * _ensure_ref_jf (core/jellyfish_wrappers.py:313-326).  Host buffers. */
int kdf_count_reads(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid,
                    uint64_t n_bases);
/* Same with the stream already resident in HBM (device pointers to buffers of the kdf_stream_words(n_bases) sizes).
 * The words at and past n_bases may hold anything ("Read streams", points 1-2): the last k - 1 positions before
 * n_bases start no window, on every path (pending stream, direct, binned, key_parts, long keys), so a batch small
 * enough to wait in the pending stream and one that is partitioned where it lies give the same table.
 * Ordering: the deferred forms run in stream order and do not synchronise; whatever is deferred never reads the caller's
 * buffers after the call has returned in stream order (the pending stream is a copy, a batch partitioned where it lies is
 * partitioned by the call).  Through the direct kernels the call synchronises (see "Count calls ... are DEFERRED"). */
int kdf_count_reads_dev(kdf_engine *h, const void *d_packed, const void *d_invalid,
                        uint64_t n_bases);

/* Double-buffered feeding of a streamed sample (the `samtools fasta | jellyfish count` pipe,
 * core/jellyfish_wrappers.py:166-199, as two overlapping stages): kdf_upload_reads_async copies a host batch into
 * device staging slot 0 or 1 on a copy stream of the engine's own and returns at once when the host arrays are pinned
 * (kdf_host_alloc; pageable arrays work too, the copy is then synchronous); kdf_count_uploaded counts the batch a
 * slot holds (filtered != 0: count --if) on the engine's stream.  Upload batch i + 1, then count batch i: the copy
 * runs under the count.  The host arrays of a batch may be rewritten once kdf_count_uploaded for THAT batch returned.
 * A slot holds its batch until a count or a prefilter tally takes it: kdf_count_uploaded on a slot that holds none is
 * KDF_ERR_STATE, and a call refused for the engine's state (count with a filter loaded or while the prefilter is tallying,
 * count --if without a filter or under force_path 4 without a sieve) leaves the batch in the slot.  An empty batch
 * (n_bases = 0) asks nothing of the sieve, here as in kdf_count_reads_filtered*: it is KDF_OK under force_path 4 too.  kdf_clear,
 * kdf_load_filter* and kdf_set_stream do not touch the slots: a batch uploaded before kdf_set_stream is counted on the new
 * stream, after its copy.
 * Ordering: kdf_count_uploaded waits ON THE HOST for the slot's copy (that is what frees the batch's host arrays) and makes
 * the engine's stream wait for it; it does not synchronise the engine's stream unless the count itself does (direct
 * kernels, see "Count calls ... are DEFERRED").  A copy into a slot waits, on the copy stream, for the slot's last reader:
 * a count of the slot's NEXT batch therefore returns only when the count of the batch before has run. */
int kdf_host_alloc(uint64_t bytes, void **out);
int kdf_host_free(void *p);
int kdf_upload_reads_async(kdf_engine *h, int slot, const uint64_t *packed, const uint64_t *invalid,
                           uint64_t n_bases);
int kdf_count_uploaded(kdf_engine *h, int slot, int filtered);

/* Insert-or-add explicit (key, count) pairs: key i gains counts[i] (counts ==
 * NULL adds 0, i.e. plain insertion).  Loads an on-disk index into the table
 * (`jellyfish query` mmaps the .jf; discovery/pipeline.py:286-288) and merges
 * per-GPU partial counts after the owner-partitioned exchange (`jellyfish
 * merge`, core/jellyfish_wrappers.py:335-366).  A key that occurs twice in one call gains both counts; sums saturate at
 * 2^32 - 1.  Works in insert and in filter mode, is never gated by key_parts or an armed prefilter, and leaves `windows`
 * alone.  Keys added while a filter is loaded are filter keys like the others (kdf_count_reads_filtered* counts them on
 * every path); the filter's sieve does not know them, so option force_path 4 is KDF_ERR_STATE from then on, until
 * kdf_scan_reads* has rebuilt the sieve from the table or a filter is loaded again.
 * The _dev forms (kdf_add_pairs_multi_dev and the _w form too) read the caller's arrays in stream order and SYNCHRONISE
 * the engine's stream: the host learns the new number of distinct keys and whether a bucket overflowed. */
int kdf_add_pairs(kdf_engine *h, const uint64_t *keys_lo, const uint64_t *keys_hi,
                  const uint32_t *counts, uint64_t n);
int kdf_add_pairs_dev(kdf_engine *h, const void *d_keys_lo, const void *d_keys_hi,
                      const void *d_counts, uint64_t n);
/* The owner's half of the multi-GPU merge: `nseg` (<= 64 for the fast path) segments of pairs in HBM, one per source
 * rank, summed into the table in one call (d_keys_lo / d_keys_hi / d_counts / n are HOST arrays of nseg device
 * pointers / lengths; d_keys_hi may be NULL for k <= 32).  When every segment is grouped by this table's buckets in
 * ascending order -- what kdf_export_parts_dev writes -- each bucket is merged in LDS by one workgroup and written
 * once (the test runs on the device; any other order is merged through global atomics, same result).  An owner table
 * should be created with option "hash_shift" = floor(log2(world)): its home slots then ignore the hash bits that name
 * the owner, so the table is used over its whole length and the senders' order is its own. */
int kdf_add_pairs_multi_dev(kdf_engine *h, uint32_t nseg, const void *const *d_keys_lo,
                            const void *const *d_keys_hi, const void *const *d_counts, const uint64_t *n);

/* ------------------------------------------------- two-pass counting ---- */

/* Keep k-mers seen fewer than L times out of the table (`jellyfish bc` + `jellyfish count --bc`, made exact).  The
 * child count of the discovery chain is `jellyfish count` followed by `dump -L min_child_count`
 * (discovery/pipeline.py:114-226); in a sequenced sample most distinct k-mers are sequencing errors seen once, and
 * each of them costs a table slot only to be dropped by the dump.  With a prefilter the reads are streamed twice:
 *
 *   pass 1  kdf_prefilter_begin, kdf_prefilter_add_* over every batch (TALLY: no key is stored), kdf_prefilter_arm
 *   pass 2  the usual insert-mode count calls over the same batches: a window is counted iff its cell reads >= L
 *   then    dumps / queries as usual; kdf_prefilter_drop frees the sieve, counts are ungated again
 *
 * The sieve.  2^s cells, 16 <= s <= 38, HALF A BYTE each.  cell(key) = h >> (64 - s), the TOP s bits of the key's
 * 64-bit stored form h: kdf_mix64(key) = (key ^ (key >> 32)) * 0x9FB21C651E98DF25 for k <= 32,
 * kdf_mix64(lo ^ rotl(hi, 37)) for 33 <= k <= 63, and for long keys kdf_mix64(w0 ^ f) with f folded from the top word
 * down, f = 0; f = kdf_mix64(f ^ w_j) + 0x632BE59BD9B4E019 for j = W-1 .. 1 (all mod 2^64).  The value of a cell is
 * min(number of tallied windows whose key maps to it, 3), whatever the order or concurrency of the tally calls.
 *
 * Exactness.  Pass 1 only tallies and pass 2 counts every admitted window in full, so the table holds exactly
 * {(key, full count) : value(cell(key)) >= L}: every key with count >= L (its own sightings bring its cell to L), plus
 * those rarer keys that share a cell with enough other sightings.  `dump -L m` for every m >= L is therefore identical
 * to the plain count's.  kdf_stats' `windows` counts admitted windows only (as it does for key_parts).
 *
 * State machine, every violation an error that names the rule:
 *   - off -> begin -> tallying -> arm -> armed -> drop -> off.  begin flushes pending count work, allocates and zeroes
 *     the sieve (KDF_ERR_NOMEM when it does not fit).  min_count L must be 2 or 3 (KDF_ERR_INVALID: 1 is the plain
 *     count, above 3 the cell saturates -- for `-L 5` ask for 3 and dump with 5).  log2_cells 16..38, or 0: the engine
 *     takes ceil(log2(8 x capacity_hint of kdf_create)) clamped to that range.
 *   - kdf_prefilter_add_* and kdf_prefilter_arm only while tallying; begin while tallying or armed: KDF_ERR_STATE.
 *   - while TALLYING insert-mode count calls are KDF_ERR_STATE (such a count would be neither gated nor known to be
 *     meant ungated); while ARMED they are gated, on every path (direct, binned, pending stream, force_path, defer,
 *     fused_dump, growth of the table).  count --if, queries, dumps, histogram, scan, kdf_add_pairs*, kdf_load_filter*
 *     are never affected.
 *   - drop flushes pending count work first (it was admitted under the sieve).  kdf_clear empties the table and leaves
 *     the prefilter as it is; kdf_destroy frees it.
 *   - refused together (KDF_ERR_STATE, either order): key_parts > 1 and a prefilter; hash_shift != 0 and a prefilter.
 *   - every key width: k <= 32, 33..63, long engines (odd 65..201).
 * Several ranks (a sharded count: every rank streams its share of the reads).  A rank's own tallies under-count, but a
 * cell is min(sightings, 3), so the SATURATING SUM of the ranks' cells is exactly the cell one engine would have
 * tallied over the whole sample.  Every rank tallies its share into a sieve of the SAME log2_cells, the sieves are
 * merged (kdf_prefilter_export* / kdf_prefilter_merge* below) until every rank holds the merged sieve, every rank arms
 * and counts its share again: all ranks admit the same keys, and after the owner exchange of the local tables
 * (kdf_export_parts*, kdf_add_pairs_multi_dev) the owners hold exactly {(key, full count) : value(cell(key)) >= L} --
 * the contract above; `dump -L m`, m >= L, is identical to the plain sharded count's.  The owner tables themselves
 * never take a prefilter (hash_shift, refused above).  So far this has only run as several ranks on ONE GPU.
 * Stats (kdf_get_stat): "prefilter_state" (0 off / 1 tallying / 2 armed), "prefilter_min_count",
 * "prefilter_log2_cells", "prefilter_bytes", "prefilter_windows" (windows THIS engine tallied: a merge does not touch
 * it), "prefilter_merged_words" (words written by merges since begin), and under kdf_profile(h, 1) "prefilter_us" /
 * "prefilter_passes" (the tally kernel, HIP events), "prefilter_merge_us" / "prefilter_merge_passes" (the merge kernel). */
int kdf_prefilter_begin(kdf_engine *h, uint32_t min_count, uint32_t log2_cells);
/* Tally one batch of the read stream (host buffers / device buffers of the kdf_stream_words(n_bases) sizes / the batch
 * an upload slot holds, kdf_upload_reads_async).  The stream is read exactly as the count reads it ("Read streams":
 * positions at or past n_bases are invalid whatever the buffers hold).  The _dev and the uploaded form run in stream order
 * and do not synchronise the engine's stream (the uploaded form waits on the host for the slot's copy, as a count does). */
int kdf_prefilter_add_reads(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases);
int kdf_prefilter_add_reads_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases);
int kdf_prefilter_add_uploaded(kdf_engine *h, int slot);
int kdf_prefilter_arm(kdf_engine *h);
int kdf_prefilter_drop(kdf_engine *h);
/* cells_by_value[v] = number of cells that read v, v = 0 .. 3 (their sum is 2^log2_cells); tallying or armed. */
int kdf_prefilter_fill(kdf_engine *h, uint64_t cells_by_value[4]);
/* The sieve as words: sixteen cells per 64-bit word, cell c in bits [4 (c & 15), +4) of word c >> 4; bits 0..2 of a
 * nibble are a thermometer code (0 / 1 / 3 / 7 for the values 0..3), bit 3 is clear.  *n_words = 2^(log2_cells - 4).
 * Tallying or armed; off: KDF_ERR_STATE. */
int kdf_prefilter_words(kdf_engine *h, uint64_t *n_words);
/* Copy words [first_word, first_word + n_words) out, to device / host memory.  Read-only, tallying or armed (off:
 * KDF_ERR_STATE); runs in stream order after the pending tallies and merges and returns when the copy is complete.
 * A range past the sieve is KDF_ERR_INVALID; n_words == 0 is KDF_OK and copies nothing. */
int kdf_prefilter_export_dev(kdf_engine *h, uint64_t first_word, uint64_t n_words, void *d_words_out);
int kdf_prefilter_export(kdf_engine *h, uint64_t first_word, uint64_t n_words, uint64_t *words_out);
/* Saturating sum of `nseg` segments (n_words words each, word i of a segment belongs to sieve word first_word + i)
 * into the sieve: per cell new = min(own + sum of the segments' values, 3); with replace != 0 the engine's own value
 * is left out, new = min(sum, 3) -- how a rank takes over a slice another rank has merged.  The value of an incoming
 * nibble is popcount(bits 0..2), the rule the gate reads by: bit 3 is ignored and a non-thermometer code such as
 * 0b101 reads as 2; what is written is always 0 / 1 / 3 / 7, so garbage in a segment can never put a code into the
 * sieve that the tally does not produce.  One kernel launch for all segments; "prefilter_windows" is not changed.
 *   - only while TALLYING (KDF_ERR_STATE while armed -- the sieve is immutable between arm and drop, partition-time
 *     gates rely on that -- or off);
 *   - a range past the sieve, nseg == 0, nseg > 64, a NULL segment: KDF_ERR_INVALID, and nothing is written;
 *   - n_words == 0 is KDF_OK.
 * _dev: d_segs is a HOST array of nseg device pointers; the segments must be complete before the call and stay
 * untouched until kdf_synchronize (the kernel runs in stream order).  The host form stages the segments through the
 * engine and returns when the merge is complete. */
int kdf_prefilter_merge_dev(kdf_engine *h, uint64_t first_word, uint64_t n_words, uint32_t nseg,
                            const void *const *d_segs, int replace);
int kdf_prefilter_merge(kdf_engine *h, uint64_t first_word, uint64_t n_words, uint32_t nseg,
                        const uint64_t *const *segs, int replace);

/* ------------------------------------------------ count --if (filter) ---- */

/* Load the `--if` filter: the table becomes exactly these canonical keys with
 * count 0 (core/jellyfish_wrappers.py:173, discovery/pipeline.py:383).  Keys
 * must already be canonical (the reference's filter files are).  Whatever the table held is gone, pending count work
 * included; kdf_stats' `windows` reads 0; a key given twice is stored once; n = 0 loads the empty filter (filter mode, no
 * keys).  Options, the upload slots and the prefilter are not touched. */
int kdf_load_filter(kdf_engine *h, const uint64_t *keys_lo, const uint64_t *keys_hi,
                    uint64_t n);
/* The same with the keys already resident in HBM (device pointers): the hand-off between the discovery stages
 * (child candidates -> reference subtraction -> parent filter, discovery/pipeline.py:207-226,286-304,515-532)
 * without a host round trip.  Reads the keys in stream order and SYNCHRONISES the engine's stream (table size, bucket
 * overflow); the _w form does the same. */
int kdf_load_filter_dev(kdf_engine *h, const void *d_keys_lo, const void *d_keys_hi, uint64_t n);
/* Zero every count, keep the keys (and the filter mode): the same filter counted against the next parent
 * (discovery/pipeline.py:462-612 builds a fresh --if table per parent).  `windows` reads 0 and pending count --if work is
 * dropped (its counts would be zeroed anyway).  In insert mode pending count work is applied first, since it brings keys,
 * and then the same happens: the keys stay stored with count 0 -- they are in kdf_count_ge(h, 0) and in bin 0 of the
 * histogram, kdf_scan_reads* does not hit them, "hash_shift" still sees a table that holds keys -- and the next counts
 * add to them. */
int kdf_reset_counts(kdf_engine *h);
/* `jellyfish count -C --if`: only windows whose canonical k-mer is in the table
 * are counted; nothing is inserted.  Replaces _scan_parent_jellyfish
 * (core/jellyfish_wrappers.py:115-283) and _count_parent_jellyfish
 * (discovery/pipeline.py:322-459). */
int kdf_count_reads_filtered(kdf_engine *h, const uint64_t *packed,
                             const uint64_t *invalid, uint64_t n_bases);
/* (device form: buffers of the kdf_stream_words(n_bases) sizes whose words at and past n_bases may hold anything,
 * "Read streams" points 1-2 -- through the sieve, the binned pipeline and the direct kernel alike; nothing is inserted, so
 * the host has nothing to learn: stream order on every path, does not synchronise) */
int kdf_count_reads_filtered_dev(kdf_engine *h, const void *d_packed,
                                 const void *d_invalid, uint64_t n_bases);

/* ------------------------------------------------------- query / dump ---- */

/* `jellyfish query idx -s kmers.fa`: counts_out[i] = count of key i, 0 when
 * absent, INPUT ORDER (discovery/pipeline.py:286-304,515-532,565-583;
 * kmer_utils.py:152-183). */
int kdf_query(kdf_engine *h, const uint64_t *keys_lo, const uint64_t *keys_hi,
              uint64_t n, uint32_t *counts_out);
/* device-pointer form: d_counts_out can be a torch tensor that is then
 * all-reduced over RCCL (multi-GPU merge of per-rank filter counts).  Stream order on the engine's stream; does not
 * synchronise once pending count work is applied (the _w form too). */
int kdf_query_dev(kdf_engine *h, const void *d_keys_lo, const void *d_keys_hi,
                  uint64_t n, void *d_counts_out);

/* `jellyfish dump -c -L min_count`: number of entries with count >= min_count
 * (min_count = 0 returns every stored key, counts 0 included). */
int kdf_count_ge(kdf_engine *h, uint32_t min_count, uint64_t *n_out);
/* `jellyfish histo -h high`: bins_out[c], 0 <= c <= high, = number of STORED keys whose count is exactly c;
 * bins_out[high + 1] = number whose count is above `high` (high + 2 uint64 words in all; Jellyfish's default high is
 * 10000).  bins_out[0] counts the keys stored with count 0 -- a `count --if` filter key never seen, a pair added with
 * a NULL / zero count -- exactly as kdf_count_ge(h, 0) counts them; empty slots are in no bin.  So
 * sum(bins) == kdf_count_ge(h, 0) and sum(bins[m ..]) == kdf_count_ge(h, m) for every m <= high + 1.
 * ONE pass over the 4-byte count array, the same for every key width (the key words are read only for slots with
 * count 0, and only when the table can hold such keys); the table is not modified and a loaded filter's sieve stays
 * valid.  Works in insert and in filter mode, on owner tables (hash_shift), and with key_parts set (it then
 * describes the slice the table holds, like kdf_stats).  high <= 2^24 - 1 (KDF_ERR_INVALID above).
 * The reference has no call for it: the histogram is what a user reads --min-child-count and --parent-max-count
 * off.  The _dev form writes the bins to caller-owned HBM (e.g. a torch int64 tensor that is then all-reduced over
 * the owner ranks); both synchronise the engine's stream.  Under kdf_profile(h, 1) the kernel (kdf_histo_kernel) is
 * timed with HIP events: stats "histo_us" (summed microseconds) and "histo_passes". */
int kdf_histogram(kdf_engine *h, uint32_t high, uint64_t *bins_out);
int kdf_histogram_dev(kdf_engine *h, uint32_t high, void *d_bins_out);
/* `jellyfish stats`: unique = keys with count 1, distinct = keys with count >= 1, total = the sum of all counts
 * (counters saturate at 2^32 - 1 and are summed as stored), max_count = the largest stored count (0 for an empty
 * table).  Any pointer may be NULL.  The same single pass (the histogram kernel with high = 1). */
int kdf_count_stats(kdf_engine *h, uint64_t *unique, uint64_t *distinct, uint64_t *total, uint64_t *max_count);
/* ... and the entries themselves, ASCENDING key order (deterministic; the
 * reference does not rely on Jellyfish's hash order).  cap = room in the out
 * arrays; *n_out = entries written.  keys_hi_out / counts_out may be NULL.
 * (discovery/pipeline.py:207-226; core/jellyfish_wrappers.py:262-272) */
int kdf_export_ge(kdf_engine *h, uint32_t min_count, uint64_t *keys_lo_out,
                  uint64_t *keys_hi_out, uint32_t *counts_out, uint64_t cap,
                  uint64_t *n_out);

/* Device-to-device dump: the entries go to caller-owned HBM buffers (e.g. torch
 * tensors that are then exchanged over RCCL, or the next stage's filter); unsorted
 * unless sorted != 0.  ONE pass over the table: at most `cap` entries are written,
 * *n_out is the number the dump holds; KDF_ERR_INVALID when that exceeds cap
 * (kdf_count_ge sizes the buffers).  d_keys_hi_out may be NULL for k <= 32,
 * d_counts_out may be NULL when sorted == 0.  Synchronises the engine's stream.  With min_count >= 1, count passes
 * pending and a table still empty since kdf_clear, the dump is all that is written (option "lazy_table"): the table is
 * materialised by the next call that reads or changes it, kdf_clear drops it unwritten. */
int kdf_export_ge_dev(kdf_engine *h, uint32_t min_count, void *d_keys_lo_out,
                      void *d_keys_hi_out, void *d_counts_out, uint64_t cap,
                      int sorted, uint64_t *n_out);

/* Table join: the entries of h's table by their count in other's table -- reference subtraction (`dump -L 3` of the
 * child, kept where the reference holds nothing) and `dump -L min -U max` in one pass, without a key list in between.
 * An entry (key, c) of h is SELECTED iff
 *   - its slot is occupied,
 *   - min_count <= c <= max_count, and
 *   - when other != NULL: other_min <= oc <= other_max, where oc is the count kdf_query would return for the key in
 *     other: 0 when other does not hold the key, and 0 when it holds it with count 0 (the two are not told apart).
 * Every bound is inclusive; UINT32_MAX as an upper bound means none.  With other == NULL the other_* bounds are
 * ignored and every oc reads 0: that is `jellyfish dump -L min_count -U max_count`.
 *
 * kdf_count_join gives the number of selected entries, for every key width.  The export forms follow
 * kdf_export_ge_dev / kdf_export_ge_w_dev: ONE pass over h's table, at most `cap` entries written, *n_out = the number
 * the join holds, KDF_ERR_INVALID when that exceeds cap (*n_out is still set, nothing is written past cap); unsorted
 * unless sorted != 0, then ascending key order with both count columns following their keys (at most 2^32 entries for
 * k > 32).  d_keys_hi_out may be NULL for k <= 32; either counts pointer may be NULL.  The host forms write ascending
 * key order; with 0 < cap < the table's slot count (a cap from kdf_count_join) they stage cap entries and make one pass,
 * any other cap has a counting pass size the staging first.  The (lo, hi) forms refuse a long engine and name the _w form, the _w forms (rows of W words) refuse an
 * engine for k <= 63.
 *
 * KDF_ERR_INVALID before anything is launched: other == h, engines that differ in k or in device, min_count >
 * max_count, and with other != NULL other_min > other_max.
 *
 * Both engines pass the gate of every table reader first: pending count passes are applied and a table that is still
 * only logically empty is written (the dump-only flush of kdf_export_ge_dev is not used here).  other's stream is
 * synchronised before the kernel is queued on h's stream, and the call returns with h's stream synchronised.  Neither
 * table is modified: keys, counts, kdf_stats and a loaded filter's sieve stay valid.  Works with key_parts on either
 * side (a table holds the slice it holds), with hash_shift on either side (k <= 63), in insert and in filter mode, and
 * for any pair of capacities and bucket geometries.  Under kdf_profile(h, 1) the kernel (kdf_join_kernel /
 * kdf_long_join_kernel, csrc/kdf_join.h) is timed with HIP events: stats "join_us" and "join_passes". */
int kdf_count_join(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count,
                   uint32_t other_min, uint32_t other_max, uint64_t *n_out);
int kdf_export_join_dev(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count,
                        uint32_t other_min, uint32_t other_max, void *d_keys_lo_out, void *d_keys_hi_out,
                        void *d_counts_out, void *d_other_counts_out, uint64_t cap, int sorted, uint64_t *n_out);
int kdf_export_join(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count,
                    uint32_t other_min, uint32_t other_max, uint64_t *keys_lo_out, uint64_t *keys_hi_out,
                    uint32_t *counts_out, uint32_t *other_counts_out, uint64_t cap, uint64_t *n_out);
int kdf_export_join_w_dev(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count,
                          uint32_t other_min, uint32_t other_max, void *d_keys_out, void *d_counts_out,
                          void *d_other_counts_out, uint64_t cap, int sorted, uint64_t *n_out);
int kdf_export_join_w(kdf_engine *h, kdf_engine *other, uint32_t min_count, uint32_t max_count,
                      uint32_t other_min, uint32_t other_max, uint64_t *keys_out, uint32_t *counts_out,
                      uint32_t *other_counts_out, uint64_t cap, uint64_t *n_out);

/* The multi-GPU exchange of the full count stage (Jellyfish `merge`,
 * core/jellyfish_wrappers.py:335-366, done over xGMI): dump every (key, count >= min_count)
 * pair to DEVICE arrays grouped by owner rank, owner(key) = ((hash(key) >> 48) * parts) >> 16
 * with the table's own hash -- so the owners are contiguous slot ranges and no sort or
 * partition pass is needed.  part_counts_out[parts] (host) receives the pairs per owner;
 * part p occupies [sum(counts[0..p)), +counts[p]) of the outputs.  The whole dump is in HASH
 * ORDER (grouped by the top log2cap - 6 hash bits, ascending), which is bucket order in every
 * owner table of up to 64x this table's slots per owner: kdf_add_pairs_multi_dev merges it
 * bucket by bucket in LDS.  Order and owners follow each key's HASH, not the slot it lies in: on a table with big
 * buckets (8192 slots for k <= 32: from 2^32 slots on, or option "big_bucket_log2cap") a probe run can carry a key
 * out of the 4096 slots its hash names, even across an owner boundary that cuts its bucket (parts not a power of two
 * at 2^28 slots); it is still dumped under its own prefix and to its own owner.  One stream synchronisation.
 * parts <= 64; KDF_ERR_STATE when the table is smaller than 2^28 slots. */
int kdf_export_parts_dev(kdf_engine *h, uint32_t min_count, uint32_t parts, void *d_keys_lo_out,
                         void *d_keys_hi_out, void *d_counts_out, uint64_t cap,
                         uint64_t *part_counts_out, uint64_t *n_out);
/* The same dump written straight into the buffer the all-to-all sends: part p is ONE byte segment
 * [lo x n_p | hi x n_p (k > 32) | counts x n_p] starting at part_bytes_out[p] (multiples of 8; part_bytes_out[parts] =
 * total bytes; cap_bytes >= n * (12 or 20) + 8 * parts always suffices).  A receiver hands the segments it got to
 * kdf_add_pairs_multi_dev as they lie. */
int kdf_export_parts_packed_dev(kdf_engine *h, uint32_t min_count, uint32_t parts, void *d_buf, uint64_t cap_bytes,
                                uint64_t *part_counts_out, uint64_t *part_bytes_out, uint64_t *n_out);

/* The count of every listed key becomes counts[i] (device pointers; every key must be stored: KDF_ERR_INVALID
 * otherwise).  How the sum of the ranks' `count --if` tallies goes back into each rank's table after the all-reduce
 * (kmer_denovo_filter_amd/distributed.py; the reference's parent scan is one process, discovery/pipeline.py:377-443).
 * Reads keys and counts in stream order and SYNCHRONISES the engine's stream: the host learns whether a key was missing. */
int kdf_set_counts_dev(kdf_engine *h, const void *d_keys_lo, const void *d_keys_hi, const void *d_counts, uint64_t n);

/* ------------------------------------------------------ Module-3 scan ---- */

/* Probe every window of a read stream against the table: bit i of hit_bits is
 * set iff window i is valid and its canonical k-mer is stored with count > 0
 * (JellyfishKmerQuery: parts[1] != "0", kmer_utils.py:181).  hit_bits has
 * kdf_stream_words()' invalid-word count of uint64 words.
 * When read_offsets != NULL (n_reads+1 stream offsets of the read starts, as
 * kdf_pack_reads() returns them) distinct_out[r] = number of DISTINCT canonical
 * k-mers hit in read r (len(unique_in_read), core/bam_scanner.py:435-442).
 * Replaces the inner loop of _scan_contig_for_hits (core/bam_scanner.py:396-474)
 * and JellyfishKmerQuery.scan_read (kmer_utils.py:209-238).
 * The device form writes hit words 0 .. ceil(n_bases / 64) - 1; a bit at a position > n_bases - k is never set,
 * whatever the stream's words hold at and past n_bases ("Read streams" points 1-3).  Stat "last_scan_path": the
 * kernel the last scan ran through (0 direct, 3 sieve). */
int kdf_scan_reads(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid,
                   uint64_t n_bases, const int64_t *read_offsets, int64_t n_reads,
                   uint64_t *hit_bits, uint32_t *distinct_out);
int kdf_scan_reads_dev(kdf_engine *h, const void *d_packed, const void *d_invalid,
                       uint64_t n_bases, void *d_hit_bits);

/* ------------------------------------- per-read hits of the Module-3 scan ---- */

/* The scan and its per-read reduction without leaving the device: what Module 3 filters on
 * (len(unique_in_read) >= min_distinct_kmers_per_read, core/bam_scanner.py:435-442).  rows_out is n_reads x 2 uint32,
 * row-major: `hits` (valid windows of the read whose canonical key is stored with count > 0) and `distinct` (distinct
 * canonical keys among those windows).  A window belongs to a read by the rule of kdf_read_depth: window i belongs to
 * read r iff offsets[r] <= i < offsets[r + 1]; positions below offsets[0], at or past offsets[n_reads] or at or past
 * n_bases belong to no read, so a prefix of a longer stream is allowed.  hit_bits may be NULL; otherwise it receives
 * exactly what kdf_scan_reads* writes (the same words, the same tail rule: "Read streams" point 3; the device form
 * writes words 0 .. ceil(n_bases / 64) - 1, the host form zeroes all kdf_stream_words' mask words first).
 * Contract:
 *   - hits[r] equals column `present` of kdf_read_depth*, distinct[r] equals distinct_out[r] of kdf_scan_reads, and
 *     distinct <= hits.  A key stored with count 0 is no hit.
 *   - every key width (k <= 32, 33..63, long engines), insert and filter mode, owner tables (hash_shift); with
 *     key_parts set the hits are those of the slice the table holds.
 *   - the table is only read: pending count work is applied first and a loaded filter's sieve stays valid.  The bits
 *     come from the scan (the sieve, or the direct kernel under force_path 1); the result does not depend on which.
 *   - exact for a read of any length (a whole contig as one read), work linear in the number of hits: the hit mask is
 *     compacted to a position list and each hit puts the pair (read, table slot of its key) into a scratch set in HBM.
 *     The engine owns that scratch and keeps it between calls: 8 bytes per hit for the list, 16 to 32 for the set
 *     (KDF_ERR_NOMEM when it does not fit).  Read index and slot index must fit 63 bits together: n_reads <=
 *     2^(63 - log2cap), KDF_ERR_INVALID beyond (never hashed down inexactly).  hits[r] is reported modulo 2^32.
 *   - n_reads == 0 and n_bases == 0 are KDF_OK (n_bases == 0: rows zero, no hit word written).
 *   - host form: n_reads < 0, a negative offset and decreasing offsets are KDF_ERR_INVALID before any device work.
 *     Device form: the offsets are a precondition, but whatever they hold no write lands outside the n_reads rows.
 *   - all results are integer counts: bit-identical from run to run and between the host and device forms.
 *   - the device form SYNCHRONISES the engine's stream once (it learns the number of hits to size its scratch); the
 *     rows are complete in stream order when it returns. */
int kdf_read_hits_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases,
                      const void *d_read_offsets, int64_t n_reads, void *d_hit_bits, void *d_rows_out);
int kdf_read_hits(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases,
                  const int64_t *read_offsets, int64_t n_reads, uint64_t *hit_bits, uint32_t *rows_out);

/* The set bits of a hit mask (usually the one kdf_read_hits* just wrote) below n_bases as a list: positions_out[e] is
 * the position of the e-th set bit, ASCENDING, uint64.  When reads_out is non-NULL, reads_out[e] (int64) is the read
 * that holds the position by the rule above, or -1 for none; read_offsets may be NULL exactly when reads_out is NULL.
 * *n_out = number of set bits.  At most `cap` entries are written; when *n_out exceeds cap the call returns
 * KDF_ERR_INVALID with *n_out set (the convention of kdf_export_ge_dev).  The table is not touched (no flush).  Both
 * forms synchronise the engine's stream. */
int kdf_hit_list_dev(kdf_engine *h, const void *d_hit_bits, uint64_t n_bases, const void *d_read_offsets,
                     int64_t n_reads, void *d_positions_out, void *d_reads_out, uint64_t cap, uint64_t *n_out);
int kdf_hit_list(kdf_engine *h, const uint64_t *hit_bits, uint64_t n_bases, const int64_t *read_offsets,
                 int64_t n_reads, uint64_t *positions_out, int64_t *reads_out, uint64_t cap, uint64_t *n_out);

/* ---------------------------------------- hits in reference coordinates ---- */

/* Module 3's step from "which windows of a read hit" to "which reference positions carry the hit k-mers": the two
 * per-position sums behind .kmer_coverage.bedgraph and .read_coverage.bed (core/bam_scanner.py:97-117
 * _collect_kmer_ref_positions, summed over the informative reads, discovery/pipeline.py:840-860).  Inputs: a hit mask
 * (kdf_scan_reads* / kdf_read_hits*), the read offsets of the stream, per read a linear reference start and its CIGAR.
 * kmer_cov and read_cov are two arrays of `span` uint32 words that the CALLER owns and zeroes.
 *   Hits.   A hit is a set bit p of the mask with p + k <= n_bases (k: the engine's).  Bits at and past that, and
 *           whatever the words hold past n_bases, are ignored (the masking of kdf_hit_list*).  A hit belongs to read r
 *           by the rule of kdf_read_hits*: offsets[r] <= p < offsets[r + 1]; a hit that belongs to no read
 *           contributes nothing.
 *   Depth.  For a read r and a stream position q with offsets[r] <= q < offsets[r + 1], depth(r, q) is the number of
 *           hits p of read r with p <= q < p + k.  Hits of one read never add depth to a position of another read,
 *           however close the reads lie in the stream; a window that runs past its read's end is cut there.
 *   CIGAR.  cigar[cigar_offsets[r] .. cigar_offsets[r + 1]) are read r's operations in BAM encoding (len << 4 | op),
 *           exactly what kdf_reader_last_aux hands out.  Walk them with (qc, rc) = (0, 0).  For M, = and X (op 0, 7,
 *           8): query index c = q - offsets[r] is ALIGNED at reference offset d = rc + (c - qc) iff qc <= c < qc + len;
 *           then both counters advance by len.  I and S (1, 4) advance qc.  D and N (2, 3) advance rc.  H, P and the
 *           codes 9..15 advance nothing.  A query index that no aligned operation covers has no reference position:
 *           inserted and clipped bases, a read longer than its CIGAR consumes, an empty CIGAR.
 *   Sums.   A read with ref_start[r] < 0 is skipped entirely (unmapped, not selected, de-duplicated by the caller).
 *           Otherwise, for every aligned q of the read with depth(r, q) > 0 and g = ref_start[r] + d < span:
 *           kmer_cov[g] += depth(r, q) and read_cov[g] += 1.  A g >= span is dropped: not wrapped, nothing written.
 *           The call only ADDS, modulo 2^32, so several batches accumulate into one pair of arrays.  ref_start is a
 *           linear coordinate the caller defines: contig offset + leftmost reference base (kdf_reader_ref_length).
 *   - all sums are integer: bit-identical from run to run, between the host and device forms, and between one call and
 *     the same reads split over several calls.
 *   - work is linear in hits x k plus the CIGAR operations of the reads that hold hits; exact for a read of any length
 *     (a 20 kb read with hundreds of operations, a contig as one read): the operation of a query index is found by
 *     binary search in per-operation prefix sums, never by a walk per hit.  Scratch, owned by the engine and kept
 *     between calls: 8 bytes per hit, 16 per CIGAR operation (KDF_ERR_NOMEM when it does not fit).
 *   - the table is not touched (no flush), as for kdf_hit_list*; every key width is accepted, only k matters.
 *   - n_reads == 0 and n_bases == 0 are KDF_OK and add nothing.
 *   - device form: offsets, cigar_offsets and ref_start are preconditions, but whatever they hold no write lands
 *     outside the two span-word arrays and no CIGAR word outside [0, n_cigar) is read (indices are clamped).  The call
 *     synchronises the engine's stream once (it learns the number of hits to size its scratch); the sums are complete
 *     in stream order when it returns.  n_reads < 0 is KDF_ERR_INVALID.
 *   - host form: n_reads < 0, bad read offsets (negative, decreasing), cigar_offsets[0] != 0, decreasing
 *     cigar_offsets and a last cigar_offsets entry != n_cigar are KDF_ERR_INVALID before any device work; the arrays
 *     are then untouched.
 *   - under kdf_profile(h, 1) the kernels of kdf_hit_coverage* and kdf_coverage_list* are timed with HIP events:
 *     stats "coverage_us" / "coverage_passes" (one pass per call that launches). */
int kdf_hit_coverage_dev(kdf_engine *h, const void *d_hit_bits, uint64_t n_bases, const void *d_read_offsets,
                         int64_t n_reads, const void *d_ref_start, const void *d_cigar, uint64_t n_cigar,
                         const void *d_cigar_offsets, void *d_kmer_cov, void *d_read_cov, uint64_t span);
int kdf_hit_coverage(kdf_engine *h, const uint64_t *hit_bits, uint64_t n_bases, const int64_t *read_offsets,
                     int64_t n_reads, const int64_t *ref_start, const uint32_t *cigar, uint64_t n_cigar,
                     const int64_t *cigar_offsets, uint32_t *kmer_cov, uint32_t *read_cov, uint64_t span);

/* The covered positions as a list: the g in [first, first + n) with read_cov[g] >= max(min_reads, 1), ASCENDING (what
 * the bedGraph writer needs: no sort anywhere): pos_out[e] = g (uint64), kmer_out[e] = kmer_cov[g], read_out[e] =
 * read_cov[g] (uint32; either may be NULL, and kmer_cov may be NULL when kmer_out is).  first + n must not exceed the
 * arrays' length.  *n_out = number of such positions, always set; at most `cap` entries are written, and when *n_out
 * exceeds cap the call returns KDF_ERR_INVALID (the convention of kdf_hit_list_dev).  n == 0 is KDF_OK.  An
 * order-preserving compaction (count per block, scan, write).  Both forms synchronise the engine's stream. */
int kdf_coverage_list_dev(kdf_engine *h, const void *d_kmer_cov, const void *d_read_cov, uint64_t first, uint64_t n,
                          uint32_t min_reads, void *d_pos_out, void *d_kmer_out, void *d_read_out, uint64_t cap,
                          uint64_t *n_out);
int kdf_coverage_list(kdf_engine *h, const uint32_t *kmer_cov, const uint32_t *read_cov, uint64_t first, uint64_t n,
                      uint32_t min_reads, uint64_t *pos_out, uint32_t *kmer_out, uint32_t *read_out, uint64_t cap,
                      uint64_t *n_out);

/* The canonical keys of listed windows (unique_in_read, core/bam_scanner.py:435-442, without decoding a read to a
 * string): row e of keys_out, W = kdf_key_words(k) uint64 words, word 0 least significant, for every key width, is the
 * canonical key of window [positions[e], positions[e] + k) of the packed stream.  A position with p + k > n_bases gets
 * a row of all-ones words, which is never a canonical key.  Whether the window is VALID is the caller's business:
 * positions come from a hit list, and hits are valid windows.  The table is not touched.  The device form (packed of
 * the kdf_stream_words(n_bases) size, positions uint64[n], keys uint64[n x W]) runs in stream order and does not
 * synchronise; the host form reads ceil(n_bases / 32) packed words. */
int kdf_hit_keys_dev(kdf_engine *h, const void *d_packed, uint64_t n_bases, const void *d_positions, uint64_t n,
                     void *d_keys_out);
int kdf_hit_keys(kdf_engine *h, const uint64_t *packed, uint64_t n_bases, const uint64_t *positions, uint64_t n,
                 uint64_t *keys_out);

/* -------------------------------------------------- VCF mode on the device ---- */

/* VCF mode's step from "the reads over a candidate variant" to "the windows of each read that span it, and whether the
 * read spells the ALT": extract_variant_spanning_kmers and read_supports_alt (kmer_utils.py:1104-1172, :1037-1101) for
 * every (read, variant) at once, as positions in the stream instead of k-mer strings.  kdf_hit_keys* turns the
 * positions into keys: kdf_hit_keys_dev(d_packed, n_bases, d_entry_pos, n_entries, d_keys).
 *   Inputs.
 *     - a read stream (packed, invalid, n_bases) and read_offsets[n_reads + 1]: query index c of read r is stream
 *       position offsets[r] + c; the read's stream range is [offsets[r], min(offsets[r + 1], n_bases)).
 *     - ref_start[n_reads] (int64): the linear coordinate of the read's leftmost reference base (as for
 *       kdf_hit_coverage); a read with ref_start[r] < 0 is skipped entirely.
 *     - cigar[n_cigar] / cigar_offsets[n_reads + 1]: exactly what kdf_hit_coverage* takes.
 *     - base qualities, optional: qual[n_qual] (uint8, one byte per read base, no separators), qual_offsets[n_reads + 1]
 *       and min_baseq.  Query index c of read r has quality qual[qual_offsets[r] + c] when
 *       c < qual_offsets[r + 1] - qual_offsets[r], and otherwise has none: a read may be given an empty range, so the
 *       caller uploads qualities only for the reads that can matter.  qual == NULL or min_baseq == 0: no quality rule.
 *     - n_var variants (< 2^32), ASCENDING by var_pos (int64, the same linear coordinate; equal positions allowed), each
 *       with var_span (uint32: the number of read bases the variant occupies -- len(alt) for a literal ALT, 1 for a
 *       missing ALT, 0: the variant is skipped entirely, which is what the caller passes for a symbolic ALT),
 *       var_ref_len (uint32, len(ref)) and its ALT as ASCII bytes alt[alt_offsets[v] .. alt_offsets[v + 1]) of
 *       alt[n_alt].  Empty bytes, or any byte outside ACGTacgt, mean that the ALT never matches.
 *   Semantics, for every read r with ref_start[r] >= 0 and every variant v with var_span[v] > 0:
 *     Anchor.    Walk the CIGAR by the rules of kdf_hit_coverage (M, = and X align; I and S advance the query; D and N
 *                advance the reference; everything else advances nothing).  `at` is the query index that is aligned at
 *                reference offset var_pos[v] - ref_start[r].  When no query index is (the position lies in a D or N,
 *                before or behind the read's reference interval, or the CIGAR is empty) there is no pair.
 *     Bad.       Stream position q of the read's stream range is BAD when it is invalid ("Read streams" points 1-2: its
 *                mask bit is set -- N, IUPAC, the separator), or when the quality rule is on and its query index has a
 *                quality < min_baseq.
 *     Windows.   The candidate starts are the stream positions p = offsets[r] + s with
 *                max(0, at - k + 1) <= s <= at + var_span[v] - 1 and p + k <= min(offsets[r + 1], n_bases).  A candidate
 *                is an ENTRY iff none of its k positions is bad.
 *     Pair.      (r, v) is a PAIR iff it has at least one entry (`if not kmers: continue`, vcf/pipeline.py:619-726).
 *     supports_alt.  Let E = var_pos[v] + var_ref_len[v] - ref_start[r].  qe is the number of query bases the walk has
 *                consumed when it first stands on a reference offset >= E inside an M, =, X, D or N operation (inserted
 *                and clipped bases directly in front of that base are therefore consumed; inside an aligned operation
 *                qe counts the bases of the operation before that offset); when the walk never gets there, qe is the
 *                number of query bases the whole CIGAR consumes.  The pair supports the ALT iff len(alt) > 0,
 *                qe - at == len(alt), the query indices at .. qe - 1 all lie in the read's stream range, none of their
 *                stream positions is bad, and their bases spell the ALT, case-insensitively.
 *   Outputs (device form: caller-owned HBM; host form: host arrays, staged through the engine's scratch).
 *     - pairs, ascending by (read, variant index): pair_read (int64), pair_var (uint32), pair_flags (uint8, bit 0 =
 *       supports_alt, the other bits 0).
 *     - entries, ascending by (pair, position): entry_pos (uint64, the stream position of the window's start) and
 *       entry_pair (uint64, index into the pair list of this call).
 *     - *n_pairs_out and *n_entries_out are always set.  At most pair_cap pairs and entry_cap entries are written; when
 *       either count exceeds its cap the call returns KDF_ERR_INVALID (the convention of kdf_hit_list_dev).  With both
 *       caps 0 and every out pointer NULL the call is a SIZING call: KDF_OK with the two counts.
 *   - the table is not touched and nothing is flushed; every key width is accepted, only k matters.
 *   - n_reads == 0, n_var == 0 and n_bases == 0 are KDF_OK with both counts 0.
 *   - work is linear in (candidate pairs) x (k + span) plus the CIGAR operations of the reads that are not skipped,
 *     never a walk per window: a read finds its candidate variants by binary search of var_pos over [ref_start,
 *     ref_start + reference bases its CIGAR consumes), the anchor by binary search in per-operation prefix sums.
 *     Scratch, owned by the engine and kept between calls: 16 bytes per CIGAR operation and per read, 5 per candidate.
 *   - device form: offsets, cigar_offsets, qual_offsets, alt_offsets and the order of var_pos are preconditions, but
 *     whatever they hold no write lands outside the cap-sized outputs and no stream word, CIGAR word, quality byte or
 *     ALT byte is read outside its array (indices are clamped, as kdf_hit_coverage_dev does).  It SYNCHRONISES the
 *     engine's stream TWICE: once for the number of (read, variant) candidates, which sizes its scratch (a call without
 *     candidates returns after that one), once for the two counts; the lists are complete in stream order when it returns.
 *   - host form: n_reads < 0, bad read offsets (negative, decreasing), cigar_offsets / alt_offsets / qual_offsets (when
 *     qual is given) that do not start at 0, that decrease or that do not end at n_cigar / n_alt / n_qual, and a
 *     decreasing var_pos are KDF_ERR_INVALID before any device work.
 *   - all outputs are integers and positions: bit-identical from run to run, between the host and device forms, and
 *     between one call and the same reads split over several calls (concatenate, and re-base entry_pair by the pairs
 *     of the calls before).
 *   - under kdf_profile(h, 1) the kv_* kernels of these calls and of kdf_variant_evidence* are timed with HIP events:
 *     stats "variants_us" / "variants_passes" (one pass per call that launches). */
int kdf_variant_windows_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases,
                            const void *d_read_offsets, int64_t n_reads, const void *d_ref_start, const void *d_cigar,
                            uint64_t n_cigar, const void *d_cigar_offsets, const void *d_qual, uint64_t n_qual,
                            const void *d_qual_offsets, uint32_t min_baseq, const void *d_var_pos, const void *d_var_span,
                            const void *d_var_ref_len, uint64_t n_var, const void *d_alt, uint64_t n_alt,
                            const void *d_alt_offsets, void *d_pair_read, void *d_pair_var, void *d_pair_flags,
                            uint64_t pair_cap, void *d_entry_pos, void *d_entry_pair, uint64_t entry_cap,
                            uint64_t *n_pairs_out, uint64_t *n_entries_out);
int kdf_variant_windows(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases,
                        const int64_t *read_offsets, int64_t n_reads, const int64_t *ref_start, const uint32_t *cigar,
                        uint64_t n_cigar, const int64_t *cigar_offsets, const uint8_t *qual, uint64_t n_qual,
                        const int64_t *qual_offsets, uint32_t min_baseq, const int64_t *var_pos, const uint32_t *var_span,
                        const uint32_t *var_ref_len, uint64_t n_var, const uint8_t *alt, uint64_t n_alt,
                        const int64_t *alt_offsets, int64_t *pair_read, uint32_t *pair_var, uint8_t *pair_flags,
                        uint64_t pair_cap, uint64_t *entry_pos, uint64_t *entry_pair, uint64_t entry_cap,
                        uint64_t *n_pairs_out, uint64_t *n_entries_out);

/* VCF mode's annotation (annotate_variants, vcf/pipeline.py:1640-1724) against the table the engine holds -- the child's
 * keys loaded as a filter with both parents counted into it by `count --if`, so that a count is mother + father.
 * Inputs: keys (n_entries x W uint64 rows, as kdf_hit_keys* writes them; a row of all-ones words is no key and counts as
 * not stored), entry_pair[n_entries] (uint64), pair_var[n_pairs] (uint32), pair_flags[n_pairs] (uint8) and n_var.
 * Entries and pairs may come from many kdf_variant_windows* calls concatenated, in any order of variants.
 *   pair_rows  n_pairs x 2 uint32: `windows` (the entries of the pair) and `absent` (those whose key is not stored, or
 *              is stored with count 0).  A pair is informative iff absent > 0 (`not kmers.issubset(parent_set)`).
 *   var_rows   n_var x 8 uint64: n, sum, min, max and n_alt, sum_alt, min_alt, max_alt of the stored counts, taken over
 *              the DISTINCT keys with stored count > 0 among the variant's entries -- all its pairs for the first four,
 *              only the pairs with bit 0 of their flags set for the last four; min and max are 0 when n is 0
 *              (max_pkc / avg_pkc / min_pkc[_alt]; the caller forms the average as sum / n).
 *   - an entry whose entry_pair is >= n_pairs, and every entry of a pair whose pair_var is >= n_var, contributes nothing
 *     to either output; nothing is written outside the two outputs.  Both are written in full (rows without entries
 *     are zero); n_entries == 0 is KDF_OK.
 *   - distinctness is exact: a stored key and its slot are one-to-one, so the distinct keys of a variant are the
 *     distinct words (variant, tag, slot), tag 1 for the alt columns, in the engine's open-addressing scratch set (as
 *     kdf_read_hits*: 32 to 64 bytes per entry, KDF_ERR_NOMEM when it does not fit).  Variant index, tag and slot index
 *     must fit 63 bits together (the top bit keeps a word apart from the set's empty word): log2ceil(n_var) + 1 +
 *     log2cap <= 63, KDF_ERR_INVALID beyond, never hashed down.  All results are integer sums, minima and maxima.
 *   - the table is only read: pending count work is applied first and a loaded filter's sieve stays valid; every key
 *     width, insert and filter mode.
 *   - the device form runs in stream order and does not synchronise.  Timed into "variants_us" / "variants_passes". */
int kdf_variant_evidence_dev(kdf_engine *h, const void *d_keys, const void *d_entry_pair, uint64_t n_entries,
                             const void *d_pair_var, const void *d_pair_flags, uint64_t n_pairs, uint64_t n_var,
                             void *d_pair_rows, void *d_var_rows);
int kdf_variant_evidence(kdf_engine *h, const uint64_t *keys, const uint64_t *entry_pair, uint64_t n_entries,
                         const uint32_t *pair_var, const uint8_t *pair_flags, uint64_t n_pairs, uint64_t n_var,
                         uint32_t *pair_rows, uint64_t *var_rows);

/* ------------------------------------------- regions of informative reads ---- */

/* Module 3's step from "the informative reads and where they align" to the rows of discovery.bed: the intervals of the
 * reads clustered into regions (kdf_cluster_intervals*), and the number of distinct hit k-mers of every region
 * (kdf_group_distinct*, over the key rows kdf_hit_keys* wrote).  Both take plain arrays and stand on their own.
 *
 * Clustering.  chrom, start and end are int64[n], in ANY order.  chrom[i] is a rank the caller defines (the reference
 * sorts by contig NAME: the rank of the name among the sorted names); an interval with chrom[i] < 0 is skipped and gets
 * region_of[i] = -1 (the convention of ref_start < 0 in kdf_hit_coverage).
 *   Rule.   Order the remaining intervals by (chrom, start) ascending; the order of ties does not change the result.
 *           Let E_i be the maximum `end` over the EARLIER intervals of the same chrom.  Interval i opens a new region
 *           iff it is the first of its chrom or start_i > E_i + merge_distance; otherwise it joins the open region.
 *           Regions are numbered 0.. in that order.  Row g of regions_out (cap x 4 int64, row-major) is (chrom, start
 *           of the region's first interval, maximum end of its members, number of members); region_of[i] is i's region.
 *   - for end >= start and merge_distance >= 0 this is exactly the sweep of discovery/regions.py:_cluster_read_hits and
 *     of the reference (discovery/pipeline.py:1111-1144): the sweep keeps the open region's running end, and because the
 *     order is by start, that running end is the maximum end of EVERY earlier interval of the contig, not only of the
 *     region's own members (an earlier region ended below this region's first start, so its ends are below too): the
 *     prefix maximum within the contig.  It restarts at a contig change because the sweep never joins across contigs: a
 *     long interval at the end of one contig must not swallow the first intervals of the next, whose coordinates start
 *     over.
 *   - ranges: chrom < 2^31, 0 <= start <= end < 2^62, 0 <= merge_distance < 2^62, n < 2^32.  The host form returns
 *     KDF_ERR_INVALID before any device work when an input breaks them (the outputs are then untouched; a skipped
 *     interval's start and end are not looked at); for the
 *     device form n and merge_distance are checked and the arrays' contents are preconditions.
 *   - whatever the device arrays hold, no write lands outside region_of[0 .. n) and the first min(cap, *n_out) rows of
 *     regions_out.
 *   - *n_out is always set to the number of regions; when it exceeds cap the call returns KDF_ERR_INVALID with
 *     region_of complete and the first cap rows written (the convention of kdf_hit_list_dev).  regions_out may be NULL
 *     with cap == 0: a sizing call.  n == 0 is KDF_OK with *n_out = 0.
 *   - the table is not touched: no flush, any key width.  All outputs are integers, bit-identical between runs and
 *     between the two forms.
 *   - work: a library radix sort by start, then stably by chrom (skipped intervals behind the rest), then two block
 *     scans over the sorted order -- a prefix MAXIMUM of the pair (chrom, end), which restarts at a contig change by
 *     itself, and a prefix sum of the boundary flags -- and one pass that writes the rows with one atomic maximum and
 *     one atomic add per (wave, region).  Scratch: 13 bytes per interval owned by the engine and kept between calls,
 *     and the sort's own (24 bytes per interval and rocPRIM's), allocated and freed per call.
 *   - the device form synchronises the engine's stream (the sort, and the number of regions); both outputs are complete
 *     in stream order when it returns.
 *   - under kdf_profile(h, 1) the kernels of kdf_cluster_intervals* and kdf_group_distinct* (the sort included) are
 *     timed with HIP events: stats "regions_us" / "regions_passes" (one pass per call that launches). */
int kdf_cluster_intervals_dev(kdf_engine *h, const void *d_chrom, const void *d_start, const void *d_end, int64_t n,
                              int64_t merge_distance, void *d_region_of, void *d_regions_out, uint64_t cap,
                              uint64_t *n_out);
int kdf_cluster_intervals(kdf_engine *h, const int64_t *chrom, const int64_t *start, const int64_t *end, int64_t n,
                          int64_t merge_distance, int64_t *region_of, int64_t *regions_out, uint64_t cap,
                          uint64_t *n_out);

/* Distinct rows per group.  keys is n x words uint64, rows as kdf_hit_keys* writes them; words is 1..8 and independent
 * of the engine's own key width (W = 3..7 rows, one-word read-name ids).  group is int64[n].
 *   Rule.   counts_out[g] (uint64[n_groups], OVERWRITTEN) is the number of distinct rows among the entries e with
 *           group[e] == g.
 *   - entries with group[e] < 0 or >= n_groups are ignored, and so is a row of all-ones words: the "no key" row of
 *     kdf_hit_keys*, as in kdf_variant_evidence*.  The same row in two groups counts in both.
 *   - the result is exact: the entries are ordered by (group, row) with the library radix sort and a row is compared
 *     with its predecessor word by word, never a hash of a row in place of the row.  The counts are integer sums.
 *   - n == 0 writes zeros.  n_groups == 0 is KDF_OK and writes nothing.  n >= 2^32, words outside 1..8 and
 *     n_groups < 0 are KDF_ERR_INVALID.
 *   - the table is not touched.  Scratch: 12 bytes per entry owned by the engine, and the sort's own per call.
 *   - the device form synchronises the engine's stream (the sort); counts_out is complete in stream order when it
 *     returns.  Timed into "regions_us" / "regions_passes". */
int kdf_group_distinct_dev(kdf_engine *h, const void *d_group, const void *d_keys, int words, uint64_t n,
                           int64_t n_groups, void *d_counts_out);
int kdf_group_distinct(kdf_engine *h, const int64_t *group, const uint64_t *keys, int words, uint64_t n,
                       int64_t n_groups, uint64_t *counts_out);

/* ------------------------------------------------------ k-mer FASTA codec ---- */

/* The text of the k-mer files the discovery stages hand on (child_candidates.fa .. proband_unique.fa), made from keys
 * in device memory and read back into keys there.  The key form follows the call's k, not the engine's (as `words` of
 * kdf_group_distinct*): any engine on the device formats and parses any stage's set.
 *     k 1 .. 32        lo[n]
 *     k 33 .. 63       lo[n] and hi[n]
 *     odd k 65 .. 201  n x W uint64 rows (W = kdf_key_words(k)) in the lo position, hi NULL
 * Any other k is KDF_ERR_INVALID.  Bits as everywhere: base i of the k-mer at bits 2(k - 1 - i) of the value, word 0
 * least significant, A C G T = 0 1 2 3.  The table is not touched: no flush, any engine.
 *
 * Format.  layout KDF_TEXT_FASTA: record e is '>' + the decimal digits of first_index + e + '\n' + k upper-case bases
 * + '\n' (printf(">%llu\n%s\n")).  KDF_TEXT_ROWS: k bases per key and nothing else (first_index is ignored).
 *   - kdf_kmer_text_bytes is the size of the whole text, a pure host function (no engine, no GPU): records differ in
 *     length only by the digits of their index, so the text is at most 20 runs of equal records.  It returns 0 for a k
 *     or layout outside the above, and when first_index + n or the size passes 2^63 (n == 0 is 0 bytes as well).
 *   - a call writes bytes [byte_first, byte_first + byte_count) of the whole text to text_out[0 .. byte_count) and
 *     nothing else; the window may begin and end inside a record, a header or a digit string, so a text of any size
 *     goes through one bounded buffer.  byte_first % 16 != 0, a window that passes kdf_kmer_text_bytes and a (k, layout,
 *     first_index, n) for which that is 0 are KDF_ERR_INVALID, and nothing is written.  byte_count == 0 and n == 0 are
 *     KDF_OK.  A window takes fewer than 2^43 bytes.
 *   - work: one kernel.  A lane owns 16 consecutive output bytes, finds the record of its first byte from the table of
 *     the runs (kernel arguments) with one multiply-high in place of the division, walks its 16 bytes and stores them
 *     at once (byte stores: the window's last partial 16 bytes, and every byte when text_out is not 16-byte aligned).
 *     The keys of a workgroup's 4 KiB of text are staged in LDS with coalesced loads.
 *   - the device form runs in stream order on the engine's stream and does not synchronise.  The host form stages all
 *     n keys and the window through the engine's staging arena.
 *
 * Parse.  The rule of the reference's readers of these files: lines end at '\n' (with final_chunk a missing last '\n'
 * is supplied); one trailing '\r' is stripped; empty lines and lines whose first byte is '>' are skipped; every other
 * line must be exactly k bytes of ACGTacgt.  Its key is the forward value or, with canonical != 0, the numeric minimum
 * of the forward and the reverse-complement value.  Keys are written in file order.
 *   - without final_chunk only whole lines are consumed: *consumed_out is the offset behind the last '\n' (0 when the
 *     chunk holds none) and the caller hands the rest over again in front of the next chunk.  With final_chunk
 *     *consumed_out is n_bytes.
 *   - *n_out is always set.  When it exceeds cap the call returns KDF_ERR_INVALID with the first cap rows written (the
 *     convention of kdf_hit_list_dev); lo / hi may be NULL with cap == 0: a sizing call, which checks the lines as well.
 *   - a bad line returns KDF_ERR_IO: *bad_offset_out (may be NULL; ~0 when no line is bad) is the offset of the first
 *     byte of the first bad line of the chunk, and kdf_last_error names the rule that line broke -- its length, or,
 *     its length being k, a base.  Both are the same from run to run.  *n_out then counts the bad lines too.
 *   - whatever the text holds, nothing is written outside lo / hi[0 .. min(cap, *n_out)).
 *   - work: a pass that counts the sequence-line starts of 4 KiB tiles of the text (16-byte loads when the text is
 *     16-byte aligned), a scan of the tile counts, and a pass over the same tiles in which a lane checks and encodes the
 *     lines that start in its 16 bytes and stores their rows at their rank.  A chunk takes fewer than 2^43 bytes.
 *   - both forms synchronise the engine's stream: the caller learns *n_out.
 *
 * Under kdf_profile(h, 1) the kernels of both are timed with HIP events: stats "kmerfasta_us" / "kmerfasta_passes"
 * (one pass per call that launches). */
#define KDF_TEXT_FASTA 0
#define KDF_TEXT_ROWS  1
uint64_t kdf_kmer_text_bytes(int k, int layout, uint64_t first_index, uint64_t n);
int kdf_format_kmers_dev(kdf_engine *h, const void *d_lo, const void *d_hi, uint64_t n, int k, int layout,
                         uint64_t first_index, uint64_t byte_first, uint64_t byte_count, void *d_text_out);
int kdf_format_kmers(kdf_engine *h, const uint64_t *lo, const uint64_t *hi, uint64_t n, int k, int layout,
                     uint64_t first_index, uint64_t byte_first, uint64_t byte_count, uint8_t *text_out);
int kdf_parse_kmer_fasta_dev(kdf_engine *h, const void *d_text, uint64_t n_bytes, int k, int canonical, int final_chunk,
                             void *d_lo, void *d_hi, uint64_t cap, uint64_t *n_out, uint64_t *consumed_out,
                             uint64_t *bad_offset_out);
int kdf_parse_kmer_fasta(kdf_engine *h, const uint8_t *text, uint64_t n_bytes, int k, int canonical, int final_chunk,
                         uint64_t *lo, uint64_t *hi, uint64_t cap, uint64_t *n_out, uint64_t *consumed_out,
                         uint64_t *bad_offset_out);

/* ------------------------------------------------------ index record codec ---- */

/* The records of the index files the stages hand on ({ref}.k{k}.jf, proband_unique.jf, merged chunks: "kdf/sorted" and
 * Jellyfish's "binary/sorted"), made from keys and counts in device memory and read back into them there.  A record is
 * kb = ceil(2k / 8) little-endian key bytes followed by counter_len little-endian count bytes.  The key form follows the
 * call's k, not the engine's, as in the k-mer FASTA codec:
 *     k 1 .. 32        lo[n]
 *     k 33 .. 63       lo[n] and hi[n]
 *     odd k 65 .. 201  n x W uint64 rows (W = kdf_key_words(k)) in the lo position, hi NULL
 * Any other k is KDF_ERR_INVALID.  The table is not touched: no flush, any engine.
 *
 * Each entry point is ONE function with a `mem` argument in place of a host / device pair: with KDF_MEM_HOST the array
 * arguments are host pointers, staged through the engine's staging arena as the other host forms do (the call
 * synchronises); with KDF_MEM_DEVICE they are device pointers, used in place in stream order on the engine's stream.
 * Any other mem is KDF_ERR_INVALID.  `columns` and the scalar results are host memory with both.  With KDF_MEM_HOST an
 * encode call stages all n keys, counts and perm values whatever its window, so a caller that cuts a large body into
 * windows keeps its keys in device memory.
 *
 * kdf_index_record_bytes: kb + counter_len, a pure host function (no engine, no GPU); 0 for a k outside the above or a
 * counter_len outside 1 .. 16.
 *
 * Encode (4-byte counters: what this package writes).
 *   - record e of the body is the kb key bytes of key (perm ? perm[e] : e) and the 4 bytes of its count; with
 *     R = kb + 4 it begins at byte e * R.  perm is uint32[n] (values below n: a precondition), counts uint32[n]; a NULL
 *     counts writes count 0.
 *   - a call writes bytes [byte_first, byte_first + byte_count) of the body to bytes_out[0 .. byte_count) and nothing
 *     else; the window may begin and end inside a record, so a body of any size goes through one bounded buffer.
 *     bytes_out may have any alignment.
 *   - byte_first % 16 != 0, a window that passes n * R, n * R >= 2^63 and, with perm, n >= 2^32 are KDF_ERR_INVALID,
 *     and nothing is written.  byte_count == 0 and n == 0 are KDF_OK.  A window takes fewer than 2^43 bytes.
 *   - work: one kernel.  A lane owns 16 consecutive output bytes, finds the record of its first byte with one
 *     multiply-high in place of the division, walks its 16 bytes and stores them at once (byte stores: the window's
 *     last partial 16 bytes, and every byte when bytes_out is not 16-byte aligned).  The keys and counts of a
 *     workgroup's 4 KiB of body are staged in LDS, gathered through perm when given.
 *   - device memory: stream order, no synchronisation.
 *
 * Decode.
 *   - bytes holds n whole records of kb + counter_len bytes at any alignment.  The key is the kb bytes little-endian,
 *     zero-extended to the key form's words; the count is the first min(counter_len, 8) bytes little-endian, saturated
 *     at 2^32 - 1, and 2^32 - 1 as well when any byte past the eighth is non-zero (the rule of jf_io._decode).
 *   - hi may be NULL for k <= 32 (given, it is filled with zeros) and is ignored for k > 63; counts may be NULL.
 *   - a record whose key has a bit at or above 2k returns KDF_ERR_IO: *bad_record_out (may be NULL; ~0 when none) is
 *     the index of the first such record, the same from run to run.  The rows are still written as read.
 *   - loads touch only the aligned 16-byte words that enclose the first and the last byte of bytes; nothing is stored
 *     outside lo / hi / counts[0 .. n).  n == 0 is KDF_OK.  A call takes fewer than 2^39 records.
 *   - work: one kernel.  A workgroup stages the 16-byte words that enclose 256 records in LDS, a lane assembles one
 *     record's key words and count from there; rows of long keys leave through LDS in whole lines; the first bad record
 *     is one atomic minimum per workgroup.
 *   - the call synchronises the engine's stream with both memory kinds: the caller learns the bad record.
 *
 * Jellyfish's order (k <= 63 only; any other k is KDF_ERR_INVALID).  columns is a HOST array of 2k words with both
 * memory kinds (the header's matrix1.columns), size a power of two (else KDF_ERR_INVALID).
 *   - kdf_jf_positions: pos_out[i] (uint64) is the XOR of columns[j] over the set bits 2k - 1 - j of key i, ANDed with
 *     size - 1.  Work: one kernel; a workgroup builds one table of 256 words per key byte in LDS from the columns, a
 *     position is then the XOR of kb table reads.  Device memory: stream order, no synchronisation.
 *   - kdf_jf_order: perm_out (uint32[n]) is the permutation that puts the keys in ascending (position, key) order --
 *     the record order of a binary/sorted file; equal (position, key) pairs keep their input order.  The positions go
 *     to scratch the engine owns (8 bytes per key), the order is the library radix sort over the key words and the
 *     position.  n >= 2^32 is KDF_ERR_INVALID.  The call synchronises the engine's stream (the sort).
 *
 * Under kdf_profile(h, 1) the kernels of all four are timed with HIP events: stats "indexcodec_us" /
 * "indexcodec_passes" (one pass per timed span: a kernel, and the sort of kdf_jf_order). */
#define KDF_MEM_HOST   0
#define KDF_MEM_DEVICE 1
uint64_t kdf_index_record_bytes(int k, int counter_len);
int kdf_index_encode(kdf_engine *h, int mem, const void *lo, const void *hi, const void *counts, const void *perm,
                     uint64_t n, int k, uint64_t byte_first, uint64_t byte_count, void *bytes_out);
int kdf_index_decode(kdf_engine *h, int mem, const void *bytes, uint64_t n, int k, int counter_len,
                     void *lo, void *hi, void *counts, uint64_t *bad_record_out);
int kdf_jf_positions(kdf_engine *h, int mem, const void *lo, const void *hi, uint64_t n, int k,
                     const uint64_t *columns, uint64_t size, void *pos_out);
int kdf_jf_order(kdf_engine *h, int mem, const void *lo, const void *hi, uint64_t n, int k,
                 const uint64_t *columns, uint64_t size, void *perm_out);

/* ------------------------------------------- count profile of a stream ---- */

/* `jellyfish query idx -s reads.fa` over a whole read stream: counts_out[i], 0 <= i < n_bases, is the stored count of
 * the canonical k-mer of window [i, i + k) -- 0 when the key is not stored, when it is stored with count 0 (a
 * `count --if` filter key never seen) and when the window is not valid; a saturated counter reads 2^32 - 1 as stored.
 * JellyfishKmerQuery (kmer_utils.py:152-183) runs exactly this query and keeps one bit of it (parts[1] != "0");
 * kdf_scan_reads* is that bit: (counts_out[i] != 0) == bit i of its hit words, for every i, on every scan path.
 * valid_bits_out may be NULL; otherwise bit i % 64 of word i / 64 is set iff window i is valid ("Read streams"); it has
 * the size of a hit array (kdf_stream_words' mask words), words 0 .. ceil(n_bases / 64) - 1 are written and no bit at a
 * position > n_bases - k is set, whatever the buffers hold at and past n_bases.
 * The device form writes exactly n_bases counts and reads at most the kdf_stream_words(n_bases) words of each stream
 * buffer; n_bases == 0 is KDF_OK and writes nothing.  It does not synchronise (stream order, like kdf_scan_reads_dev).
 * Every key width, insert and filter mode, owner tables (hash_shift); with key_parts set the counts are those of the
 * slice the table holds (as kdf_histogram).  The table is only read: pending count work is applied first, a loaded
 * filter's sieve stays valid, an armed prefilter is not consulted, force_path does not matter.
 * Single GPU: an owner-partitioned table holds a share of the keys and cannot answer alone; a replicated table (the
 * parent-filter layout) can, with the reads sharded by the caller and no collective. */
int kdf_window_counts_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases,
                          void *d_counts_out, void *d_valid_bits_out);
int kdf_window_counts(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases,
                      uint32_t *counts_out, uint64_t *valid_bits_out);

/* The same lookups reduced per read where they are made (no per-position array): rows_out is n_reads x 6 uint64,
 * row-major: `windows` (valid windows of the read), `present` (of those, count > 0), `low` (of those, count <= low_max;
 * absent keys count as 0, so they are included), `min`, `max` (over the valid windows, absent = 0; both 0 when
 * `windows` is 0), `sum` (of the counts, 64-bit, counters summed as stored).  The read-level form of the discovery
 * chain's per-k-mer filter (child count >= min_child_count, parent count <= parent_max_count,
 * discovery/pipeline.py:207-226,515-612): how many windows of a read are absent or rare in a parent's table.
 * read_offsets are the n_reads + 1 stream offsets kdf_pack_reads / kdf_reader_next return: window i belongs to read r
 * iff offsets[r] <= i < offsets[r + 1] and the window is valid (a valid window never spans a separator).  Positions
 * below offsets[0], at or above offsets[n_reads] or at or above n_bases belong to no read: a prefix of a longer stream
 * is allowed.  All fields are integer sums, minima and maxima: the result is bit-identical from run to run and between
 * the host and device forms.
 * Host form: n_reads < 0, a negative offset or offsets that decrease are KDF_ERR_INVALID before any device work.
 * Device form: the offsets are a precondition, but whatever they hold no write lands outside the n_reads rows.
 * n_reads == 0 is KDF_OK.  Same widths, modes, tables and single-GPU note as kdf_window_counts; the device form runs in
 * stream order and does not synchronise either. */
int kdf_read_depth_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases,
                       const void *d_read_offsets, int64_t n_reads, uint32_t low_max, void *d_rows_out);
int kdf_read_depth(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases,
                   const int64_t *read_offsets, int64_t n_reads, uint32_t low_max, uint64_t *rows_out);

/* ------------------------------------------------------- host utilities -- */

/* Words a stream of n_bases needs (padding included): the packed array must
 * hold *packed_words uint64 (2 * ceil(n_bases / 64) + 4), the invalid / hit arrays *mask_words uint64
 * (ceil(n_bases / 64) + 2).  This is a SIZE: the kernels may read every one of those words, and none beyond; what the
 * words at and past n_bases hold does not matter ("Read streams" points 1-2). */
void kdf_stream_words(uint64_t n_bases, uint64_t *packed_words, uint64_t *mask_words);

/* The sizing rule of the bin-major sieve (option "sieve_bins"), a pure host function: for a filter of n_keys keys of
 * key_words (1: k <= 32, 2: k <= 63) words, under option values sieve_bits and sieve_bins (1, or 4 .. 10), the coarse bits
 * *c1, the 64-bit words per bin *slice_words (a power of two from 128 up to what one compute unit's LDS holds beside the
 * kernel's queues: 2^14) and the sieve bits per key *bits_per_key (sieve_bits as given; 0: 8, and 4 when 8 does not fit at
 * c1 = 10).  The sieve has 2^c1 x slice_words words >= n_keys x bits_per_key / 64, rounded up to a power of two.
 * sieve_bins 1 picks the smallest c1 in 4 .. 10 whose slice fits.  KDF_ERR_INVALID: no bin-major sieve for this filter
 * (it would need fewer than 4 bits per key or a larger slice than fits) or arguments out of range; the out pointers may
 * be NULL.  The engine sizes its sieve with this function. */
int kdf_bin_sieve_geometry(uint64_t n_keys, int key_words, int sieve_bits, int sieve_bins, uint32_t *c1, uint32_t *slice_words,
                           uint32_t *bits_per_key);

/* Pack ASCII records (A/C/G/T any case; everything else invalid) into a stream
 * with one separator after each record.  offsets[n_reads+1] delimit the records
 * in `ascii`.  stream_offsets_out[n_reads+1] (may be NULL) receives each
 * record's start in the stream (record r occupies [so[r], so[r]+len_r); the
 * last entry is n_bases).  Stream length = sum(len) + n_reads.
 * Restates what `samtools fasta` hands to Jellyfish (one FASTA record per read). */
int kdf_pack_reads(const char *ascii, const int64_t *offsets, int64_t n_reads,
                   uint64_t *packed_out, uint64_t *invalid_out,
                   int64_t *stream_offsets_out, uint64_t *n_bases_out);

/* Canonical key of one ASCII k-mer; returns KDF_ERR_INVALID on a non-ACGT byte
 * (kmer_utils.py:35-38). */
int kdf_canonical(const char *kmer, int k, uint64_t *lo, uint64_t *hi);

/* ------------------------------------------------- BAM / FASTA feeders ---- */

/* Streaming BAM reader with `samtools fasta -F flag_off` semantics
 * (core/jellyfish_wrappers.py:159-165, discovery/pipeline.py:106-112): records
 * with any flag_off bit are dropped; when collapse != 0 each run of consecutive
 * same-QNAME records yields at most one record per read part (READ1 / READ2 /
 * other), a record with qualities beating one without, first wins.
 * collapse = 0, flag_off = 0x500 gives Module 3's pysam iteration
 * (core/bam_scanner.py:405-409: skip SECONDARY and DUPLICATE, keep the rest). */
int kdf_bam_open(const char *path, uint32_t flag_off, int collapse, int threads,
                 kdf_reader **out);
/* The same reader over ONE RANGE of the file: the BGZF blocks that hold the records are cut at parts - 1 byte offsets
 * and the record stream at the first record boundary behind each cut -- the first QNAME-run boundary when runs are
 * collapsed, so no run is split: the parts 0 .. parts - 1 together yield exactly the records kdf_bam_open yields, each
 * once, whatever `parts` is, and a part only reads and inflates its own bytes.  This is how the read stream of one
 * sample is sharded over the GPUs of a node (reads are independent units) and over several reader
 * pipelines inside one process.  Record ordinals (kdf_reader_last_ordinals) count from the part's first record. */
int kdf_bam_open_range(const char *path, uint32_t flag_off, int collapse, int threads,
                       int part, int parts, kdf_reader **out);
/* Multi-record FASTA (reference genome, plain or gzip) as a reader: one stream
 * record per sequence, any case, non-ACGT invalid.  A sequence longer than a
 * batch is continued in the next batch k-1 bases back, so no window is lost or
 * counted twice.  Replaces Jellyfish's own FASTA parsing in _ensure_ref_jf
 * (core/jellyfish_wrappers.py:313-321). */
int kdf_fasta_open(const char *path, int k, kdf_reader **out);
/* Fill up to max_bases stream positions / max_reads records.  Returns the batch
 * through the out pointers; *n_reads_out = 0 at end of file.  packed_out /
 * invalid_out must hold kdf_stream_words(max_bases) words;
 * stream_offsets_out max_reads+1 entries.  A record longer than max_bases is an
 * error (KDF_ERR_INVALID). */
int kdf_reader_next(kdf_reader *r, uint64_t max_bases, int64_t max_reads,
                    uint64_t *packed_out, uint64_t *invalid_out,
                    int64_t *stream_offsets_out, int64_t *n_reads_out,
                    uint64_t *n_bases_out);
/* Per-record metadata of the LAST batch (BAM readers; arrays of n_reads):
 * flag, ref_id, pos, and the offsets of NUL-terminated names in name_buf. */
int kdf_reader_last_meta(kdf_reader *r, const uint16_t **flags, const int32_t **ref_ids,
                         const int32_t **positions, const char **name_buf,
                         const int64_t **name_offsets);
/* Alignment details for Module 3's post-processing of informative reads
 * (core/bam_scanner.py:97-117,284-337: CIGAR -> reference coordinates, SA tag,
 * soft clips).  Call kdf_reader_want_aux(r, 1) after kdf_bam_open; then, for the
 * last batch: cigar[cigar_offsets[i] .. cigar_offsets[i+1]) are record i's CIGAR
 * operations in BAM encoding (len << 4 | op), sa_offsets[i] is the offset of its
 * NUL-terminated SA:Z value in sa_buf or -1. */
int kdf_reader_want_aux(kdf_reader *r, int enable);
int kdf_reader_last_aux(kdf_reader *r, const uint32_t **cigar, const int64_t **cigar_offsets,
                        const char **sa_buf, const int64_t **sa_offsets);
/* Base qualities (qual[qual_offsets[i] .. qual_offsets[i+1]), 0xFF when the record
 * has none) and MAPQ of the last batch; needs kdf_reader_want_aux.  Used by the
 * VCF-mode producer (kmer_utils.py:1037-1172: --min-baseq, vcf/pipeline.py:673: --min-mapq). */
int kdf_reader_last_quals(kdf_reader *r, const uint8_t **qual, const int64_t **qual_offsets,
                          const uint8_t **mapq);
/* Record number in the file (0-based, counted before the flag filter) of every read
 * of the last batch: the handle kdf_bam_write_subset takes. */
int kdf_reader_last_ordinals(kdf_reader *r, const uint64_t **ordinals);
/* Reference sequence names of a BAM reader (header order = ref_id). */
int kdf_reader_ref_count(kdf_reader *r);
const char *kdf_reader_ref_name(kdf_reader *r, int i);
/* Reference length of sequence i of a BAM reader's header (l_ref), -1 for a bad index: the contig offsets of
 * kdf_hit_coverage's linear coordinate are their running sum. */
int kdf_reader_ref_length(kdf_reader *r, int i);
void kdf_reader_close(kdf_reader *r);
const char *kdf_reader_error(const kdf_reader *r);

/* ---------------------------------------------------- device BAM feeder ---- */

/* The feeder with the heavy part on the device: the host reads the COMPRESSED bytes of a BAM and
 * plans the batch (kdf_bamraw_*, host only, no GPU needed); the device inflates the BGZF blocks, walks the records
 * with the semantics of kdf_bam_open and writes the packed stream straight into HBM (kdf_bamdev_decode_dev).  It
 * serves the counting legs: sequence only -- no names, ordinals, CIGAR, qualities or SA.
 *
 * One BGZF block of a batch.  All fields come from the block's gzip header and trailer alone. */
typedef struct {
    uint64_t comp_off;   /* offset of the raw DEFLATE payload in the batch's compressed buffer */
    uint64_t out_off;    /* offset of the block's inflated bytes in the batch's inflated span (running sum of isize) */
    uint64_t file_off;   /* where the block starts in the file (error messages) */
    uint32_t comp_len;   /* payload bytes (header, extra field and trailer are not copied) */
    uint32_t isize;      /* inflated bytes (the trailer's ISIZE); 0: nothing to decode */
} kdf_bgzf_block;
/* One sub-range of a batch: the records a range reader (kdf_bam_open_range) over the same file cuts would yield.
 * start: offset in the inflated span of the sub-range's first record (KDF_SUB_NONE: the sub-range is empty).
 * stop: offset of its END ZONE, the first BGZF block at or after the next cut (KDF_SUB_NONE: the file's end).  The walk
 * runs from start; once a record STARTS at or after stop, only the QNAME run that straddles stop is finished (collapse
 * = 0: the walk ends at that record).  flags bit 0 (KDF_SUB_AT_EOF): the batch's inflated span ends where the file
 * ends, so running out of bytes is the end of the file and not a short tail. */
typedef struct { uint64_t start, stop, flags; } kdf_bam_subrange;
#define KDF_SUB_NONE   0xFFFFFFFFFFFFFFFFull
#define KDF_SUB_AT_EOF 1ull
/* sub_status of kdf_bamdev_decode_dev */
#define KDF_SUB_DONE       0
#define KDF_SUB_UNFINISHED 1   /* the batch's bytes ended before the stop record and the file has more: replay with a longer tail */
#define KDF_SUB_CORRUPT    2   /* block_size < 32, field sizes beyond block_size, negative l_seq, or a record cut off by the file's end */

/* The raw range planner.  Part `part` of `parts` of the file (the same cuts as kdf_bam_open_range) is cut again every
 * subrange_bytes of FILE (0: 1 MiB).  Opening reads the BAM header once; the start of each sub-range is located when a
 * batch first needs it, exactly as kdf_bam_open_range locates a part's start -- the only inflating the host does. */
typedef struct kdf_bamraw kdf_bamraw;
int kdf_bamraw_open(const char *path, uint32_t flag_off, int collapse, int part, int parts, uint64_t subrange_bytes,
                    kdf_bamraw **out);
/* Sub-ranges of the part (0 for a BAM without records). */
int kdf_bamraw_subranges(kdf_bamraw *r, uint64_t *n_subranges);
/* The next batch: a contiguous run of whole BGZF blocks, their payloads copied back to back into comp_buf (comp_cap
 * bytes; page-locked memory of kdf_host_alloc is meant, pageable works), with the block table (cap_blocks entries) and
 * the sub-range table (cap_subs entries).  It holds as many consecutive sub-ranges, from the cursor on, as fit with
 * `tail_blocks` further blocks behind the last sub-range's stop block (0: 2) -- the walk of a sub-range runs past
 * `stop` to its stop record; sub-ranges inside a batch need no tail, the next one's bytes follow.  *n_subs = 0: the
 * part is done.  *first_sub: index in the part of subs[0].  KDF_ERR_INVALID when not even one sub-range fits. */
int kdf_bamraw_next(kdf_bamraw *r, void *comp_buf, uint64_t comp_cap, uint32_t tail_blocks,
                    kdf_bgzf_block *blocks, uint64_t cap_blocks, kdf_bam_subrange *subs, uint64_t cap_subs,
                    uint64_t *n_blocks, uint64_t *n_subs, uint64_t *first_sub, uint64_t *comp_bytes,
                    uint64_t *inflated_bytes);
/* Move the cursor: the next batch starts with sub-range `sub` of the part (the replay of an unfinished sub-range). */
int kdf_bamraw_seek(kdf_bamraw *r, uint64_t sub);
void kdf_bamraw_close(kdf_bamraw *r);
const char *kdf_bamraw_error(const kdf_bamraw *r);

/* Inflate n_blocks BGZF blocks on the device, on the engine's stream: block b's payload d_comp[comp_off, + comp_len)
 * -> d_out[out_off, + isize).  Raw DEFLATE: stored, fixed and dynamic blocks, any number of them per BGZF block.  No
 * byte outside the payload is read and none outside [out_off, out_off + isize) is written, whatever the payload holds;
 * a table entry that does not fit d_out's out_cap bytes, or states more than 64 KB, is not decoded at all (status
 * KDF_INF_BOUNDS; the call returns KDF_ERR_INVALID).  A block the device decoder rejects (its KDF_INF_* status,
 * csrc/kdf_inflate.h; d_block_status, n_blocks uint32 on the device, may be NULL) does not fail the call: it is inflated
 * again with zlib on the host and its bytes are patched into d_out (stat "bamdev_fallback_blocks" counts them); only a
 * block zlib rejects too is KDF_ERR_IO, with its file offset in the message.  Synchronises.  No CRC is checked (the host
 * reader checks none).  The INPUT side of the table is trusted: the entry point does not know how large d_comp is, so
 * comp_off + comp_len of every entry must lie inside it (kdf_bamraw_next's tables do); inside a payload the decoder
 * never reads past comp_len.  Option "bamdev_host_inflate" = 1 sends EVERY block through that zlib path (tells a decoder
 * fault from a file fault; the tests reach the patch path with it: no block zlib wrote is rejected on the device).  It is
 * a diagnostic, not for timing: every patched block drains the stream twice. */
int kdf_bgzf_inflate_dev(kdf_engine *h, const void *d_comp, const void *d_blocks, uint64_t n_blocks,
                         void *d_out, uint64_t out_cap, void *d_block_status);
/* Decode one planned batch into a read stream in caller-owned device memory, in exactly the layout kdf_reader_next
 * produces: d_packed / d_invalid hold kdf_stream_words(cap_bases) words, d_offsets cap_reads + 1 int64.  Inflate, walk
 * (one walker per sub-range), scan, pack; one synchronisation, because the sizes are learnt on the way.  The stream
 * holds the sub-ranges' reads in sub-range order UP TO the first sub-range that is not KDF_SUB_DONE: *n_reads and
 * *n_bases count those, sub_status[n_sub] (host) says where and why it ended.  The caller replays from the first
 * KDF_SUB_UNFINISHED sub-range with a longer tail (kdf_bamraw_seek); nothing is lost or doubled.  KDF_SUB_CORRUPT
 * returns KDF_ERR_IO, a stream larger than cap_bases / cap_reads KDF_ERR_INVALID (nothing is written then).  Every
 * word below kdf_stream_words(*n_bases) is written: positions at and past *n_bases are invalid in the mask and zero in
 * the packed array.  The call returns with its last kernels (the walk's write pass and the pack) queued on the engine's
 * stream, and they read d_blocks, d_subranges and the engine's scratch: none of the inputs may be overwritten -- by a copy
 * on another stream, say -- before the stream has reached that point (an event recorded on it after the call orders that;
 * reads.stream_bam_device does so).  Stats: "bamdev_fallback_blocks", and under kdf_profile "bamdev_inflate_us", "bamdev_walk_us",
 * "bamdev_pack_us" with their "_passes". */
int kdf_bamdev_decode_dev(kdf_engine *h, const void *d_comp, const void *d_blocks, uint64_t n_blocks,
                          const void *d_subranges, uint64_t n_sub, uint32_t flag_off, int collapse,
                          void *d_packed, void *d_invalid, uint64_t cap_bases, void *d_offsets, uint64_t cap_reads,
                          uint64_t *n_bases, uint64_t *n_reads, uint32_t *sub_status);

/* -------------------------------------------------- device FASTA feeder ---- */

/* The FASTA leg with the parse on the device: the raw text of a (multi-)FASTA lies in HBM, kernels
 * write the packed stream, the invalid mask and the record offsets in the layout kdf_reader_next produces for a FASTA
 * file, and the host only moves bytes.  It serves the counting legs: sequence only, no record names.  The table is not
 * touched and nothing is flushed: any engine, of any k, packs any FASTA.
 *
 * THE RULE, per byte (this is the specification; it is what kdf_reader_next does for a FASTA file):
 *   - a line ends at '\n'; the file's end closes the last line.  All '\r' directly in front of the line's end are dropped.
 *   - a line whose first byte is '>' is a header line, at any length.  Everything before the first header line is skipped.
 *   - inside a record every remaining byte of a non-header line is ONE stream position: ACGTacgt valid with codes
 *     0 .. 3, every other byte (a blank, a tab, an interior '\r', IUPAC codes, '>' away from a line start) an invalid
 *     position with packed bits 0.
 *   - every record is followed by one separator position (invalid, bits 0), emitted at the next header line's '>' or, on
 *     the final chunk, at the end of the file.  A record without bases is a lone separator.
 * The host reader differs from the rule in one place only: it reads a line longer than its 65 535-byte gzgets buffer in
 * pieces, so a '\r' or '>' that falls exactly on a piece boundary is taken for a line end or a line start.  The rule
 * above, not that artefact, is what these entry points implement.
 *
 * CHUNKS.  The whole-file stream S is the concatenation of the records' positions and separators; a call emits the
 * slice of S that belongs to the bytes it consumes.  A call that is not the last consumes everything except a trailing
 * run of '\r' (whether those are dropped depends on the next byte): *consumed says how much was taken and the caller
 * hands the rest over again in front of the next chunk.  The final call consumes everything and emits the closing
 * separator; the state's flags are 0 afterwards.  `state` (zero it before the first chunk) carries the three flags and
 * the running totals of records (header lines) and of slice positions (carried positions are not counted again).  A
 * non-empty chunk that is not the last and of which nothing is consumed (only '\r') is KDF_ERR_INVALID.  Lines have no
 * length limit: an unwrapped chromosome on one line spans many chunks.  A chunk takes at most 2^31 bytes.
 *
 * CARRY.  With carry > 0, prev_n_bases > 0, both prev pointers given and the incoming state KDF_FA_IN_RECORD, the call
 * first copies the last c = min(carry, prev_n_bases) positions of the previous stream (bits and mask bits) to positions
 * [0, c) of the new one; the slice follows at position c.  The caller passes carry = k - 1: no window lies wholly inside
 * k - 1 positions, so the batches of a file, counted one after another, hold exactly the valid windows of S, each once
 * (copying across a separator is harmless for the same reason).  The prev buffers must not overlap the outputs: equal
 * pointers are KDF_ERR_INVALID.  carry = 0 or NULL prev: a plain slice.
 *
 * OUTPUTS.  d_packed / d_invalid hold kdf_stream_words(cap_bases) words.  Every word below kdf_stream_words(*n_bases) is
 * written -- positions at and past *n_bases are invalid in the mask and zero in the packed array, the guarantee of
 * kdf_bamdev_decode_dev -- and nothing outside those words.  cap_bases >= n_bytes + carry + 1 always suffices.
 * d_offsets may be NULL (cap_reads is ignored then); else it is int64[cap_reads + 1] and receives *n_reads + 1 entries:
 * record r of the call occupies [off[r], off[r + 1]), with its separator when it has one; if the call begins inside a
 * record, piece 0 starts at offset 0 and includes the carry; off[*n_reads] == *n_bases.  *n_reads is set without
 * offsets too.  A stream that needs more than cap_bases, or more than cap_reads records when offsets are asked for, is
 * KDF_ERR_INVALID: nothing is written and `state` is unchanged, as after every refusal.  n_bytes == 0 with final_chunk
 * closes an open record; n_bytes == 0 without it is KDF_OK, emits nothing and writes nothing.
 *
 * WORK.  On the engine's stream, over tiles of KDF_FASTA_TILE_BYTES of text: a pass that summarises each tile (16-byte
 * loads when the text is 16-byte aligned; any alignment works), one scan of the summaries, a pass over the same tiles
 * that compacts codes and mask bits in LDS and stores whole 64-bit words (the partial words at a tile's edges by
 * atomic OR into zeroed words), and a tail kernel for the carry and the words behind *n_bases.  The call synchronises
 * once, because it learns the sizes.  The host form stages text, previous stream and outputs through the engine's
 * staging arena.  Under kdf_profile(h, 1): stats "fastafeed_us" / "fastafeed_passes" (one pass per call that launches). */
typedef struct { uint32_t flags; uint32_t reserved; uint64_t records; uint64_t positions; } kdf_fasta_state;
#define KDF_FA_IN_RECORD 1u   /* a header line has been seen: sequence bytes emit positions */
#define KDF_FA_MID_LINE  2u   /* the chunk does not begin at a line start */
#define KDF_FA_IN_HEADER 4u   /* ... and that line is a header line */
#define KDF_FASTA_TILE_BYTES 4096   /* text bytes per workgroup of the passes (tests aim at its multiples) */
int kdf_fasta_pack_dev(kdf_engine *h, const void *d_text, uint64_t n_bytes, int final_chunk, kdf_fasta_state *state,
                       const void *d_prev_packed, const void *d_prev_invalid, uint64_t prev_n_bases, uint32_t carry,
                       void *d_packed, void *d_invalid, uint64_t cap_bases, void *d_offsets, uint64_t cap_reads,
                       uint64_t *n_bases, uint64_t *n_reads, uint64_t *consumed);
int kdf_fasta_pack(kdf_engine *h, const uint8_t *text, uint64_t n_bytes, int final_chunk, kdf_fasta_state *state,
                   const uint64_t *prev_packed, const uint64_t *prev_invalid, uint64_t prev_n_bases, uint32_t carry,
                   uint64_t *packed, uint64_t *invalid, uint64_t cap_bases, int64_t *offsets, uint64_t cap_reads,
                   uint64_t *n_bases, uint64_t *n_reads, uint64_t *consumed);

/* -------------------------------------------------- device FASTQ feeder ---- */

/* The FASTQ leg with the parse on the device: the raw text of a four-line FASTQ lies in HBM (or, with
 * KDF_MEM_HOST, in host memory and is staged), kernels write the packed stream, the invalid mask and the record offsets in
 * the layout kdf_reader_next and ReadStream.from_strings produce, and mask the bases whose quality is below min_qual.
 * Sequence and quality only, no read names.  The table is not touched and nothing is flushed: any engine, of any k, packs
 * any FASTQ.  ONE function with a `mem` argument, as the index record codec's.
 *
 * THE RULE, per byte (this is the specification):
 *   - LINES.  A line ends at '\n'.  All '\r' directly in front of a line's end are dropped.
 *   - RECORDS.  Lines are taken four at a time: line 0 must begin with '@' (the rest is ignored, at any length), line 1 is
 *     the sequence, line 2 must begin with '+' (the rest is ignored), line 3 is the quality.  Only four-line records are
 *     accepted: a sequence wrapped over several lines is an error by the rules below, never guessed at.
 *   - POSITIONS.  Every byte of the sequence line is ONE stream position: ACGTacgt valid with codes 0 .. 3, every other
 *     byte (N, IUPAC codes, a blank, an interior '\r') an invalid position with packed bits 0.  With min_qual > 0,
 *     position j is also invalid, with bits 0, when byte j of the quality line is below min_qual (an unsigned byte
 *     compare; `jellyfish count -Q` / --min-qual-char: the base becomes N).  min_qual == 0 never looks at quality values;
 *     min_qual > 255 is KDF_ERR_INVALID.
 *   - SEPARATOR.  Every record is followed by one separator position (invalid, bits 0); a record without bases is a lone
 *     separator.
 *   - SPANS.  Record r of the call occupies [off[r], off[r + 1]), its separator included; off[0] == 0 and
 *     off[*n_reads] == *n_bases.
 *   - A call that is NOT the last consumes whole records only: *consumed is the end of the last record whose four lines
 *     are all terminated by '\n', and only those records are examined and emitted.  The caller hands the rest over again
 *     in front of the next chunk; no window spans a call, so there is no carry.  Of the trailing bytes of its text that
 *     are only '\n' / '\r' such a call sees the first line end and leaves the rest: whether they are blank lines at the
 *     file's end (which the final call drops) or a blank line between records (an error) is for the call that sees what
 *     follows them.  A non-empty chunk without a complete record is KDF_OK with *consumed == 0, *n_reads == 0,
 *     *n_bases == 0 and writes nothing; so does n_bytes == 0.
 *   - The FINAL call first drops the trailing bytes that are only '\n' / '\r' behind the last byte that is neither; then
 *     the text's end closes the last line; then a last record of exactly three lines whose sequence line is empty gets an
 *     empty quality line.  Everything is consumed (*consumed == n_bytes).  An empty text is zero records.
 *   - FORMAT ERRORS return KDF_ERR_IO, and *bad_rule says which rule the record breaks:
 *       KDF_FQ_BAD_HEADER  line 0 does not begin with '@' (an empty line 0 -- a blank line between records -- included)
 *       KDF_FQ_BAD_PLUS    line 2 does not begin with '+'
 *       KDF_FQ_LENGTH      the sequence and quality lines differ in length after the '\r' rule
 *       KDF_FQ_TRUNCATED   on the final call the last record has fewer than four lines
 *     *bad_offset is the offset within this call's text of the first byte of the FIRST offending record: with several bad
 *     records the lowest, and *bad_rule the lowest-numbered rule that record breaks (a rule about a line the record does
 *     not have is not broken) -- the same from run to run.  Nothing usable is promised in the outputs, nothing is written,
 *     `state` is unchanged and *consumed is 0.  Without an error *bad_offset is ~0 and *bad_rule 0.
 *
 * OUTPUTS.  packed / invalid hold kdf_stream_words(cap_bases) words.  Every word below kdf_stream_words(*n_bases) is
 * written -- positions at and past *n_bases are invalid in the mask and zero in the packed array, the guarantee of the
 * FASTA feeder -- and nothing outside those words.  `offsets` may be NULL (cap_reads is ignored then); else it is
 * int64[cap_reads + 1] and receives *n_reads + 1 entries.  *n_reads is set without offsets too.  A stream that needs more
 * than cap_bases positions, or more than cap_reads records when offsets are asked for, is KDF_ERR_INVALID.  The format
 * comes first: only the first cap records are examined (cap: cap_bases, and cap_reads with offsets), a bad one among
 * them is KDF_ERR_IO, and more records than cap, or more positions than cap_bases, are KDF_ERR_INVALID after that.
 * Nothing is written and `state` is unchanged, as after every refusal.  A record of s bases takes at least 2 s + 6 bytes (2 s + 4 as the last
 * of a final call) and s + 1 positions, so *n_bases <= n_bytes / 2 and *n_reads <= n_bytes / 4:
 * cap_bases >= n_bytes / 2 and cap_reads >= n_bytes / 4 always suffice.  `state` (zeroed before the first chunk) carries
 * the running totals of records, positions and consumed bytes; the call reads nothing from it.  A chunk takes at most
 * 2^31 bytes.
 *
 * MEMORY.  KDF_MEM_DEVICE: text, packed, invalid and offsets are device pointers, used in place on the engine's stream.
 * KDF_MEM_HOST: they are host arrays, staged through the engine's staging arena as the other host forms do.  The scalar
 * results and `state` are host memory with both.  Any other mem is KDF_ERR_INVALID.  The call synchronises once, because
 * it learns the sizes and a possible error.
 *
 * WORK.  On the engine's stream: (1) one workgroup finds the end of the text in front of the trailing line ends;
 * (2) a pass over tiles of KDF_FASTQ_TILE_BYTES of text (aligned 16-byte loads at any alignment of the text: the tiles
 * are laid over the memory) counts line ends per tile; (3) one workgroup scans the counts and fixes the number of records; (4) a pass over
 * the same tiles writes the line ends' offsets into engine-owned scratch; (5) a thread per record checks the four rules,
 * takes an atomic minimum of (offset, rule) for the first bad record and writes the record's positions; (6) a scan of
 * those (block sums, one workgroup over them, a pass that adds them back) gives the offsets and, per 64 positions, the
 * record their first one lies in; (7) the pack kernel is output-driven: a wave owns 64 consecutive stream positions,
 * each lane finds its record from the offsets, loads its base byte and -- with min_qual -- its quality byte, one ballot
 * is the mask word and two more, interleaved, are the two packed words, so every output word is stored whole: no
 * atomics, no zeroing pass, reads of any length.  The last two passes read the verdict and do nothing after a
 * refusal.  The scratch is 16 bytes per record the capacities admit (at most n_bytes / 6 + 1) for the line ends
 * and 8 for the offsets.  Under kdf_profile(h, 1): stats "fastqfeed_us" / "fastqfeed_passes" (one pass per call that
 * launches). */
typedef struct { uint64_t records, positions, bytes; } kdf_fastq_state;
#define KDF_FQ_BAD_HEADER 1u
#define KDF_FQ_BAD_PLUS   2u
#define KDF_FQ_LENGTH     3u
#define KDF_FQ_TRUNCATED  4u
#define KDF_FASTQ_TILE_BYTES 4096   /* text bytes per workgroup of the line-end passes (tests aim at its multiples) */
int kdf_fastq_pack(kdf_engine *h, int mem, const void *text, uint64_t n_bytes, int final_chunk, uint32_t min_qual,
                   kdf_fastq_state *state, void *packed, void *invalid, uint64_t cap_bases,
                   void *offsets, uint64_t cap_reads,
                   uint64_t *n_bases, uint64_t *n_reads, uint64_t *consumed,
                   uint64_t *bad_offset, uint32_t *bad_rule);

/* --------------------------------------------------- FASTQ record extract ---- */

/* The records of a FASTQ chunk that the caller chose, back out as text: the raw text lies in HBM (or, with
 * KDF_MEM_HOST, in host memory and is staged), `keep` holds one flag per record, and a kernel writes the kept records one
 * behind the other, byte for byte.  It is the last step of "count, find the informative reads, hand only those on" for a
 * sample that starts from FASTQ: kdf_fastq_pack gives the stream and the record offsets of a chunk, kdf_read_hits_dev the
 * hits per record, and this call the text of the records that qualify, while the chunk is still in HBM.  The table is not
 * touched and nothing is flushed.  ONE function with a `mem` argument.  (Its name carries the prefix of the KDF_FQ_*
 * constants: the prefix kdf_fastq belongs to the feeder's one entry point.)
 *
 * RECORDS.  The records are delimited by THE RULE of kdf_fastq_pack (LINES, RECORDS, what a call that is not the last
 * consumes, what the final call drops and completes).  For the same (text, n_bytes, final_chunk) the records, *consumed,
 * the format errors (KDF_ERR_IO, *bad_offset, *bad_rule: the lowest record, its lowest rule) and their precedence are
 * those of kdf_fastq_pack with capacities that suffice.  The call is self-contained: it finds the lines itself and relies
 * on nothing that an earlier call left in the engine.  It neither takes nor changes a kdf_fastq_state.
 *
 * KEEP.  `keep` is uint8[n_reads]: a nonzero byte keeps record r of the call.  n_reads must be the number of records
 * the call holds -- what kdf_fastq_pack returns in *n_reads for the same arguments; any other value is KDF_ERR_INVALID and
 * nothing is written (the caller's flags and text have drifted apart).  A NULL keep with n_reads > 0 is KDF_ERR_INVALID.
 *
 * OUTPUT, per byte (this is the specification):
 *   - out[0 .. *out_bytes) is the concatenation, in record order, of the kept records.
 *   - A kept record is the bytes of the text from the first byte of its line 0 through the '\n' that ends its line 3,
 *     verbatim: the header's text, every '\r', the text behind '+' and the quality line are copied unchanged.
 *   - On the FINAL call the last record ends where the text ends in front of its trailing '\n' / '\r' bytes.  If a '\n'
 *     is among those trailing bytes, the record runs on, verbatim, through the first of them (so "IIII\r\n\n\n" gives
 *     "IIII\r\n").  If there is none -- the text's end closes the line -- the trailing '\r' are dropped and a '\n' is
 *     written behind the line.  A last record of three lines with an empty sequence, whose quality line the rule
 *     supplies, gets that line as "\n" behind its '+' line.  Trailing blank lines are dropped.  No other byte of the
 *     output is not a byte of the text.
 *   - Therefore *out_bytes <= *consumed + 2, and cap_out >= n_bytes + 2 always suffices.
 *   - `out_offsets` may be NULL; else it is int64[n_reads + 1] and receives *n_kept + 1 entries: the byte offset in `out`
 *     of each kept record, in order, and *out_bytes.
 *   - Nothing outside out[0 .. *out_bytes) and those entries is written.  `out` and `text` may lie at any byte alignment.
 *   - Needing more than cap_out bytes is KDF_ERR_INVALID -- after the format check and the check of n_reads -- and
 *     nothing is written.
 *   - A call that is not the last and holds no complete record is KDF_OK with *out_bytes == *n_kept == *consumed == 0 and
 *     writes nothing (n_reads must be 0); so does n_bytes == 0, final or not.  A final call of a text of only '\n' / '\r'
 *     holds no records either: *consumed == n_bytes.
 *   - After every refusal the three results are 0.  Without a format error *bad_offset is ~0 and *bad_rule 0.
 *   - A chunk takes at most 2^31 bytes.  Any mem other than KDF_MEM_HOST / KDF_MEM_DEVICE is KDF_ERR_INVALID.
 *
 * MEMORY.  KDF_MEM_DEVICE: text, keep, out and out_offsets are device pointers, used in place on the engine's stream.
 * KDF_MEM_HOST: they are host arrays, staged through the engine's staging arena.  The scalar results are host memory with
 * both.  The call synchronises once, because it learns the sizes and a possible error.
 *
 * WORK.  On the engine's stream: passes (1)-(5) of kdf_fastq_pack (the end of the text, line ends per tile, their scan,
 * the line offsets, the rule check per record) by the same kernels; (6) a thread per record writes (kept, bytes in the
 * output) -- 0 for a dropped record -- and the values are scanned as the feeder scans its positions (block sums, one
 * workgroup over them, a pass that adds them back), which gives every record its offset in the output, the caller's
 * offsets, and per tile of KDF_FASTQ_TILE_BYTES of OUTPUT the record its first byte lies in; (7) the copy kernel is
 * output-driven: the tiles are laid over the 16-byte granules of the memory `out` lies in, a workgroup owns a tile and a
 * lane a granule.  The lane finds its record by a binary search between the first records of its tile and of the next
 * (the offsets do not fall, a dropped record shares its successor's, a kept record has 6 bytes or more: the last record at
 * or below the byte is the kept one).  A granule inside one record's text is assembled from aligned 16-byte loads of the
 * unaligned source, shifted in registers, and stored whole; a granule that spans a record boundary, holds a supplied
 * '\n', or is the partial first or last granule of `out` is written byte by byte.  No atomics decide placement: the
 * output is the same from run to run.  The grid of (7) is bounded and its workgroups stride over the tiles below
 * *out_bytes, so the work is the records scanned plus the bytes kept.  Scratch: that of kdf_fastq_pack for
 * n_bytes / 6 + 1 records, and 4 bytes per output tile.  Under kdf_profile(h, 1): stats "fastqextract_us" /
 * "fastqextract_passes" (one pass per call that launches). */
int kdf_fq_extract(kdf_engine *h, int mem, const void *text, uint64_t n_bytes, int final_chunk,
                      const void *keep, uint64_t n_reads,
                      void *out, uint64_t cap_out, void *out_offsets,
                      uint64_t *out_bytes, uint64_t *n_kept, uint64_t *consumed,
                      uint64_t *bad_offset, uint32_t *bad_rule);

/* N4: the informative-reads BAM (discovery/pipeline.py:1979-2079 `_write_informative_reads_discovery`,
 * vcf/pipeline.py:1307-1357 `_write_informative_reads`: pysam write + `samtools sort` + `samtools index`).
 * Copies the records ordinals[0..n) (strictly ascending file record numbers, see
 * kdf_reader_last_ordinals) of src_bam to dst_bam byte for byte, appending
 * aux[aux_offsets[i] .. aux_offsets[i+1]) -- optional fields in BAM encoding, e.g.
 * "dkC\x01" or "DVZchr1:5:A:T\0" -- to record i (aux may be NULL).  With sort_and_index
 * the records are coordinate sorted (samtools order: tid unsigned, pos, strand; stable),
 * the header gets @HD SO:coordinate and dst_bam + ".bai" is written (SAM spec 5.2). */
int kdf_bam_write_subset(const char *src_bam, const char *dst_bam, const uint64_t *ordinals, uint64_t n,
                         const uint8_t *aux, const uint64_t *aux_offsets, int sort_and_index, int threads,
                         uint64_t *n_written);

/* ------------------------------------------- long keys (odd k 65..201) ---- */

/* Words per key of an engine for k: 1 (k <= 32), 2 (33..63), ceil(2k/64) for odd 65..201; 0 if no engine takes k. */
int kdf_key_words(int k);
/* Canonical key of one ASCII k-mer as ceil(2k/64) words, word 0 least significant (any k in 1..201;
 * KDF_ERR_INVALID on a non-ACGT byte).  kmer_utils.canonicalize + kmer_to_int, split into words. */
int kdf_canonical_w(const char *kmer, int k, uint64_t *words_out);
/* kdf_add_pairs / kdf_load_filter / kdf_query / kdf_export_ge (and their _dev forms) for long engines: `keys`
 * are n x W row-major words.  Same semantics as the (lo, hi) forms; KDF_ERR_INVALID on a k <= 63 engine.
 * kdf_export_ge_w writes ascending key order (lexicographic from the top word down); kdf_export_ge_w_dev
 * does when sorted != 0 (needs the counts array; at most 2^32 entries). */
int kdf_add_pairs_w(kdf_engine *h, const uint64_t *keys, const uint32_t *counts, uint64_t n);
int kdf_add_pairs_w_dev(kdf_engine *h, const void *d_keys, const void *d_counts, uint64_t n);
int kdf_load_filter_w(kdf_engine *h, const uint64_t *keys, uint64_t n);
int kdf_load_filter_w_dev(kdf_engine *h, const void *d_keys, uint64_t n);
int kdf_query_w(kdf_engine *h, const uint64_t *keys, uint64_t n, uint32_t *counts_out);
int kdf_query_w_dev(kdf_engine *h, const void *d_keys, uint64_t n, void *d_counts_out);
int kdf_export_ge_w(kdf_engine *h, uint32_t min_count, uint64_t *keys_out, uint32_t *counts_out,
                    uint64_t cap, uint64_t *n_out);
int kdf_export_ge_w_dev(kdf_engine *h, uint32_t min_count, void *d_keys_out, void *d_counts_out,
                        uint64_t cap, int sorted, uint64_t *n_out);

/* Long keys across ranks: the owner exchange for W-word keys (csrc/kdf_long_merge.h; distributed.py carries it, and
 * the mirrors use it only under KDF_LONG_RANKS=1).  The owner of a long key comes from bits 16..31 of its hash,
 *     h     = kdf_mix64(w0 ^ fold(w1 .. w_{W-1}))        (the stored form; kdf_long.h `kdf_long_hash`)
 *     owner = (((h >> 16) & 0xFFFF) * parts) >> 16,      parts = 1 .. 64
 * not from the top 16 bits as for k <= 63: the home slot takes the top log2cap bits and the key_parts slice the low
 * 16, so an owner's keys spread over the whole of an ordinary table -- an owner table needs no hash_shift (which long
 * engines keep refusing) and the rule is independent of the active key slice.  With log2cap > 32, more than any long
 * table fits in 288 GB, one or two owner bits would also be home bits; that costs probe locality, not correctness.
 *
 * kdf_export_parts_w_packed_dev dumps every entry with count >= min_count (0: every occupied slot, as
 * kdf_export_ge_w_dev) into d_buf (device, cap_bytes bytes) grouped by owner: part p is one byte segment
 *     [keys: n_p x W uint64, row-major | counts: n_p uint32]
 * at d_buf + part_offsets[p]; segments lie back to back, every start rounded up to 8 bytes, part_offsets[parts] is
 * the total; part_counts[parts] and part_offsets[parts + 1] are host arrays, *n_out the number of entries.  The
 * order inside a part is unspecified.  Any capacity, insert and filter mode, with a key_parts slice active or a
 * prefilter armed: it dumps what the table holds.  The sizes are known before anything is written: when cap_bytes is
 * too small the call returns KDF_ERR_INVALID, the message names the bytes needed (the outputs hold them too), and
 * d_buf is untouched.  KDF_ERR_INVALID on a k <= 63 engine and for parts outside 1..64.  Complete on return.
 * The owner adds each received segment with one kdf_add_pairs_w_dev call.
 *
 * kdf_set_counts_w_dev is kdf_set_counts_dev for n x W rows: the count of every listed stored key becomes
 * counts[i], in insert and in filter mode; a row that is not stored -- or whose top word has a bit at or above
 * 2k - 64 (W - 1), which is no k-mer, as in kdf_query_w_dev -- is not inserted and makes the call return
 * KDF_ERR_INVALID after the stored keys of the list were set. */
int kdf_export_parts_w_packed_dev(kdf_engine *h, uint32_t min_count, uint32_t parts, void *d_buf, uint64_t cap_bytes,
                                  uint64_t *n_out, uint64_t *part_counts, uint64_t *part_offsets);
int kdf_set_counts_w_dev(kdf_engine *h, const void *d_keys, const void *d_counts, uint64_t n);

/* -------------------------------------------------------- read spool ---- */

/* Keep a sample's packed read stream resident and replay it.  Every pass over a BAM goes through the host feeder, which
 * is many times slower than the count, and a sample counted in key-space slices ("key_parts") or
 * in two passes (kdf_prefilter_*) is read once per pass.  The packed stream is 3 bits per position: a spool keeps the
 * batches of the FIRST pass, and every later pass replays them into an engine at the device's rate.
 *
 * A spool is an object of its own, not part of an engine: one spool feeds any number of engines on its device (the
 * tally engine, the count engine, a fresh engine per slice), any number of times.  A handle is not thread-safe.
 *
 * Layout.  A spool is a list of SEGMENTS; a segment is one read stream in the layout of "Read streams" above: a packed
 * and a mask buffer of the kdf_stream_words(segment positions) sizes, handed to the `_dev` stream entry points as it lies.
 *   - a tile is 64 positions (one mask word, two packed words).  A batch of n_bases positions is appended at a tile
 *     boundary and occupies n_bases / 64 + 1 tiles: its mask bits at and past n_bases, up to the end of its last tile,
 *     are set and its packed bases there are zero.  A batch whose length is a multiple of 64 so keeps a whole
 *     all-invalid tile behind it (the engine's pending stream follows the same rule): no window runs from one batch into
 *     the next.
 *   - a segment of T tiles is a stream of 64 T positions: T mask and 2 T packed words, then the 2 (all ones) and 4 (zero)
 *     padding words of kdf_stream_words.
 *   - the bytes of a segment are a pure function of the appended (packed, invalid, n_bases) triples: whatever the
 *     sources held at and past n_bases does not reach the spool (the bases of invalid positions BELOW n_bases are kept
 *     as given).  An append reads at most the kdf_stream_words(n_bases) words of each source buffer.
 *   - a batch is never split: one that does not fit the room left in the last segment starts a new segment, one longer
 *     than option "segment_positions" gets a segment of its own size.  A batch of more than 2^31 positions is
 *     KDF_ERR_INVALID (before anything is allocated); n_bases == 0 is KDF_OK and stores nothing.
 * Tiers.  Segments are allocated one at a time, when a batch needs one: in HBM (hipMalloc) while "hbm_bytes" stays within
 * hbm_budget_bytes and the allocation succeeds, then in pinned host memory (hipHostMalloc) within host_budget_bytes,
 * and after that the append returns KDF_ERR_NOMEM and the spool is OVERFLOWED: further appends and every replay are
 * KDF_ERR_STATE (a replay would silently count a part of the sample), the segments stored stay readable
 * (kdf_spool_read_segment), kdf_spool_clear frees everything and resets the mark.  A host-tier batch is normalised by
 * the same kernel into a device staging buffer and copied out asynchronously; that staging (one batch) and the staging
 * of kdf_spool_append's host sources are the spool's own and are not charged to the HBM budget.
 * Ordering.  kdf_spool_append_dev runs on the stream it is given (the source must be complete in that stream's order);
 * kdf_spool_append_uploaded on the engine's stream, behind the slot's copy, and the slot KEEPS its batch: the caller
 * then counts or tallies it as before.  kdf_spool_append (host arrays) returns when the arrays may be reused.  Every
 * append is ordered behind the one before it, whatever streams they ran on, and the spool records an event behind each.
 * kdf_spool_replay makes the engine's stream wait for the last such event -- no host synchronisation of its own for the HBM
 * tier: the replay is as synchronous as the entry point it calls (a count through the direct kernels synchronises) --
 * and calls, for every segment in order, kdf_count_reads_dev (mode 0), kdf_count_reads_filtered_dev (mode 1) or
 * kdf_prefilter_add_reads_dev (mode 2).  Host-tier segments go through the engine's two upload slots
 * (kdf_upload_reads_async, then kdf_count_uploaded / kdf_prefilter_add_uploaded): the copy of the next host-tier segment
 * runs under the count of this one; the host waits once for the last append.  A slot that holds a caller's batch when a
 * replay needs the slots is KDF_ERR_STATE and nothing is replayed.  Every state rule of the target entry point applies
 * unchanged (count while tallying, count --if without a filter, ...): its error code is returned and its message is
 * passed on behind "segment i:"; such a refusal comes from the first segment, so nothing was replayed.  Spool and
 * engine must be on the same device (KDF_ERR_INVALID).  Every key width works, long engines included: the spool knows
 * nothing about k.
 * Contract.  After kdf_spool_replay the engine is in exactly the state it would be in had the appended batches been
 * given to the same entry point one by one: the same (key, count) set, the same `windows`, the same sieve words, the
 * same gating under "key_parts" and an armed prefilter.  A replay does not change the spool.  Segments must outlive the
 * work replayed from them: kdf_spool_clear and kdf_spool_destroy synchronise the device first.
 * Not kept: read names and alignment data (flags, positions, CIGAR); Module 3 reads the BAM with another flag filter
 * (0x500) than the count (0xD00), so its spool is one of its own ("Reads in a spool" below).
 * Options (kdf_spool_set_option): "segment_positions" (default 2^30, 2^12 .. 2^31; segments allocated later take it),
 * "offsets_chunk" (default 2^16 entries, 1 .. 2^28: the unit a segment's offsets array is sized and grown in), "profile"
 * (1: HIP events around every append kernel and every offsets kernel).  Stats (kdf_spool_get_stat): "segments", "batches",
 * "positions" (stream positions stored, padding included: 64 x tiles), "bases" (sum of the appended n_bases), "hbm_bytes",
 * "host_bytes" (segment bytes per tier, offsets arrays included), "overflowed", "replays", "segment_positions", "reads",
 * "keeps_reads", "offset_bytes" (bytes of the offsets arrays, both tiers), and under "profile" "append_us" /
 * "append_passes" and "offsets_us" / "offsets_passes".  Errors: kdf_spool_error(sp), or kdf_spool_error(NULL) for
 * kdf_spool_create. */
typedef struct kdf_spool kdf_spool;
int kdf_spool_create(int device, uint64_t hbm_budget_bytes, uint64_t host_budget_bytes, kdf_spool **out);
void kdf_spool_destroy(kdf_spool *sp);
const char *kdf_spool_error(const kdf_spool *sp);
int kdf_spool_set_option(kdf_spool *sp, const char *name, int64_t value);
int kdf_spool_get_stat(kdf_spool *sp, const char *name, int64_t *value);
int kdf_spool_append(kdf_spool *sp, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases);
int kdf_spool_append_dev(kdf_spool *sp, void *hip_stream, const void *d_packed, const void *d_invalid, uint64_t n_bases);
int kdf_spool_append_uploaded(kdf_spool *sp, kdf_engine *h, int slot);
int kdf_spool_replay(kdf_spool *sp, kdf_engine *h, int mode);
/* One segment to host arrays of the kdf_stream_words(*n_positions_out) sizes (tests, debugging); with both arrays NULL
 * only the size is returned.  Waits for the last append. */
int kdf_spool_read_segment(kdf_spool *sp, uint64_t seg, uint64_t *packed_out, uint64_t *invalid_out, uint64_t *n_positions_out);
int kdf_spool_clear(kdf_spool *sp);

/* Reads in a spool.  The per-read consumers -- kdf_scan_reads* with a hit list, kdf_read_hits*, kdf_read_depth* -- need the
 * read boundaries, and they are the calls a user repeats over the same reads against different tables (the child's reads
 * against either parent's table, or against one candidate k-mer set per threshold).  A spool filled through the
 * `_reads` appends keeps each batch's read offsets beside its segment and replays those consumers too.
 * Mode.  A spool either keeps reads or does not: the first append since create or clear decides ("keeps_reads").  The
 * other kind of append is KDF_ERR_STATE afterwards and stores nothing.  A spool never given offsets behaves exactly as
 * described above: nothing is allocated or launched for offsets.
 * Offsets.  read_offsets are the n_reads + 1 stream offsets kdf_pack_reads / kdf_reader_next hand out: offsets[0] == 0,
 * non-decreasing (a read of length 0 is allowed), offsets[n_reads] == n_bases.  The host forms (kdf_spool_append_reads,
 * kdf_spool_append_uploaded_reads) check this before any device work: a violation, or n_reads < 0, is KDF_ERR_INVALID
 * and no stat changes.  For kdf_spool_append_reads_dev it is a precondition; whatever the array holds, nothing is
 * written outside the n_reads + 1 entries the batch owns.  n_bases == 0 with n_reads == 0 is KDF_OK, stores nothing and
 * decides nothing; n_bases == 0 with n_reads > 0 is KDF_ERR_INVALID in every form (a batch without positions has no
 * place in a segment; empty reads are kept with a batch that has positions).
 * kdf_spool_append_uploaded_reads copies the offsets (into pinned memory, one buffer per upload slot) before it returns:
 * the caller's array is its own again at once.
 * Layout.  Every segment has an int64 array in its own tier with n_reads(segment) + 1 entries in SEGMENT coordinates: a
 * batch placed at tile t0 writes 64 t0 + offsets[i] for i = 0 .. n_reads (ks_offsets_kernel, on the stream of the batch's
 * append kernel; for the host tier through a staging buffer and the same asynchronous copy out).  The batch's last entry,
 * 64 t0 + n_bases, is overwritten by the first entry of the next batch in the segment, 64 t1 with t1 = t0 + n_bases / 64
 * + 1 (appends are ordered).  THE GAP: the last read of a batch so formally extends over the positions 64 t0 + n_bases ..
 * 64 t1 - 1 behind it.  Every one of them is invalid by the append kernel's rule and there is at least one, so no window
 * that starts in the gap or runs into it is valid, no hit bit lies in it, and -- because offsets[n_reads] == n_bases: no
 * position of the batch lies outside its reads -- the windows and hits of every read are exactly those it has in the
 * batch alone.  Without that rule positions behind the last read would silently join it.  A batch is never split, so a
 * read never spans segments.  Reads are numbered globally in append order; segment s owns reads first_read(s) ..
 * first_read(s) + n_reads(s) - 1.  The array is sized for the whole segment when its first batch arrives (from that
 * batch's reads per position) and grows in units of "offsets_chunk" when that was too little; its bytes are charged to
 * the tier's budget and reported in "hbm_bytes" / "host_bytes".  A new segment is placed in the first tier whose budget
 * holds the segment TOGETHER WITH that first offsets array, so the array never overflows a spool whose other tier had
 * room.  An array that grows later stays in its segment's tier: when the tier's budget does not hold the growth, the
 * spool overflows as for a segment that fits neither tier (KDF_ERR_NOMEM, "overflowed", nothing of the batch is stored).
 * Replays.  kdf_spool_read_hits / kdf_spool_read_depth make the engine's stream wait for the last append, walk the
 * segments in order and call kdf_read_hits_dev (d_hit_bits NULL) / kdf_read_depth_dev on each, with the segment's
 * stream, offsets and read count, writing into the caller's rows at first_read(s): n_reads x 2 uint32 / n_reads x 6
 * uint64 for "reads" reads, every row written exactly once.  The rows equal the concatenation, in append order, of what
 * the same entry point returns for each appended batch alone -- every key width, insert and filter mode, "key_parts".
 * A host-tier segment is first copied into a device staging buffer of the spool's own (one segment's packed, mask and
 * offsets words; grow-only; not charged to the HBM budget); copy and compute do not overlap.  Refusals: a spool that
 * keeps no reads and an overflowed spool are KDF_ERR_STATE, another device KDF_ERR_INVALID, an engine's refusal is
 * passed on behind "segment i:".  A spool with no reads is KDF_OK and writes nothing.  Synchronisation is the entry
 * point's: kdf_read_hits_dev synchronises the engine's stream once per segment; the rows are complete in the order of
 * the engine's stream.
 * kdf_spool_select_reads: the reads with distinct >= min_distinct among "reads" rows of kdf_spool_read_hits, as their
 * ASCENDING global indices (uint64) -- the device half of Module 3's selection at sample scale, where the rows are 8
 * bytes x 10^9 and the list is short.  An order-preserving compaction (ks_select_*: count, scan, write).  d_hit_rows
 * must be COMPLETE when the call is made (kdf_synchronize the engine that wrote them); the call runs on the spool's own
 * stream and synchronises it once.  At most 2^34 rows a call (KDF_ERR_INVALID beyond).  *n_out is always set; when it exceeds cap the call returns KDF_ERR_INVALID and at
 * most cap entries are written (the convention of kdf_hit_list_dev).  It depends on the rows alone: bit-identical from
 * run to run. */
int kdf_spool_append_reads(kdf_spool *sp, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases,
                           const int64_t *read_offsets, int64_t n_reads);
int kdf_spool_append_reads_dev(kdf_spool *sp, void *hip_stream, const void *d_packed, const void *d_invalid, uint64_t n_bases,
                               const void *d_read_offsets, int64_t n_reads);
int kdf_spool_append_uploaded_reads(kdf_spool *sp, kdf_engine *h, int slot, const int64_t *read_offsets, int64_t n_reads);
/* The twin of kdf_spool_read_segment: a segment's *n_reads_out + 1 offsets to a host array; out == NULL returns only
 * first_read and n_reads.  Waits for the last append.  KDF_ERR_STATE for a spool that keeps no reads. */
int kdf_spool_read_offsets(kdf_spool *sp, uint64_t seg, int64_t *out, uint64_t *first_read_out, uint64_t *n_reads_out);
/* The device pointers of an HBM-tier segment, to run any `_dev` entry point over it in place (kdf_scan_reads_dev,
 * kdf_hit_list_dev, kdf_window_counts_dev, ...): a stream of *n_positions positions and, for a spool that keeps reads,
 * its *n_reads + 1 offsets (*d_offsets is NULL otherwise).  Any out pointer may be NULL.  The call waits on the host
 * for the last append, so the buffers are complete for whatever stream reads them; they stay valid until the next
 * kdf_spool_clear / destroy, the offsets only until the next append (the array may move when it grows).  A host-tier
 * segment is KDF_ERR_STATE: kdf_spool_read_segment copies it out. */
int kdf_spool_segment_dev(kdf_spool *sp, uint64_t seg, const void **d_packed, const void **d_invalid, uint64_t *n_positions,
                          const void **d_offsets, uint64_t *first_read, uint64_t *n_reads);
int kdf_spool_read_hits(kdf_spool *sp, kdf_engine *h, void *d_rows_out);
int kdf_spool_read_depth(kdf_spool *sp, kdf_engine *h, uint32_t low_max, void *d_rows_out);
int kdf_spool_select_reads(kdf_spool *sp, const void *d_hit_rows, uint32_t min_distinct, void *d_reads_out, uint64_t cap,
                           uint64_t *n_out);

/* ------------------------------------------------- distinct k-mer sketch ---- */

/* How many distinct canonical k-mers does a read stream hold -- answered WITHOUT storing them, so that a table, the
 * number of key slices ("key_parts") and an owner table are sized from the reads before any key is inserted (SURVEY.md
 * section 8a row A13: "sizes from a distinct-count estimate").  A HyperLogLog sketch (Flajolet, Fusy, Gandouet, Meunier
 * 2007) of m = 2^p one-byte registers, owned by an engine because the engine knows k and the key kernels, and
 * independent of everything else the engine holds: it never flushes, reads or writes the table; it works in insert
 * mode, in filter mode and while a prefilter is tallying or armed; it survives kdf_clear, kdf_load_filter* and
 * kdf_set_stream; kdf_destroy frees it.  The kernel only walks the stream (kdf_sketch.h): a sketch pass rides on the
 * pass that fills a read spool, or replays one (kdf_spool_sketch).
 *
 * Contract (tests/sketch_model.py restates it in numpy from this text alone):
 *   - a window is sketched iff it is valid by "Read streams" points 1-2, on every path (host, device, uploaded, spool):
 *     positions at or past n_bases are invalid whatever the buffers hold.  "key_parts" and an armed prefilter are NOT
 *     consulted: the sketch describes the whole stream.
 *   - its key is the canonical key; h is the key's stored form as defined under "two-pass counting": kdf_mix64(key)
 *     for k <= 32, the pair (h, hi) with h = kdf_mix64(lo ^ rotl(hi, 37)) for 33 <= k <= 63, the folded
 *     h = kdf_mix64(w0 ^ f) for long keys.
 *   - x = h for k <= 32 and for long keys, x = h + hi * 0xD6E8FEB86659FD93 for 33 <= k <= 63 (both words of the stored
 *     pair, so two keys whose lo ^ rotl(hi, 37) agree stay two keys); g = fin(x), the finaliser of splitmix64:
 *         x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31      (mod 2^64)
 *     kdf_mix64 ends in a multiply: bit i of h depends on the key bits at and below i only, so its top bits (which
 *     address the table) see the whole key and the bits further down do not -- and the rank is read from the bits below
 *     the index.  The two further xorshift-multiply rounds bring every key bit to every bit of g.
 *   - register index j = g >> (64 - p); rank r = 1 + clz((g << p) | (1 << (p - 1))) (64-bit), so 1 <= r <= 65 - p;
 *     reg[j] = max over all sketched windows (0: no window yet).
 *   - because this is a max, the registers do not depend on batch order, batch boundaries, concurrency or path: they
 *     are bit-identical from run to run, between the host, device and uploaded forms, and between one engine over the
 *     whole sample and the merge of engines over its shards (reads are sharded, so no window is lost at a boundary).
 * Estimate (host, double, the registers summed in index order: reproducible): m = 2^p, alpha = 0.7213 / (1 + 1.079 / m),
 * E = alpha m^2 / sum_j 2^(-reg[j]); if E <= 2.5 m and V = #{j : reg[j] = 0} > 0 then E = m ln(m / V) (linear
 * counting).  The standard error is 1.04 / sqrt(m) (0.41 % at the default p = 16, 1.6 % at p = 12).  Between 2.5 m and
 * 5 m the classic estimator is biased by a few percent (no bias table is applied): a consumer that sizes memory adds its
 * own margin.  There is no large-range correction: g has 64 bits.
 * State: off -> kdf_sketch_begin -> on -> kdf_sketch_drop -> off.  begin: p = 10..18, 0 = 16 (else KDF_ERR_INVALID);
 * zeroes the registers; begin while a sketch is on is KDF_ERR_STATE.  Every other call without a sketch is
 * KDF_ERR_STATE.  The add calls take a stream exactly as the count takes it; n_bases == 0 is KDF_OK; they run in stream
 * order and do not synchronise, kdf_sketch_registers* and kdf_sketch_estimate do.  kdf_sketch_add_uploaded reads the
 * batch a slot holds (kdf_upload_reads_async) and the slot KEEPS it, as for kdf_spool_append_uploaded: the caller counts
 * or tallies it next; the call returns once the slot's copy is complete (the engine's stream is not synchronised), so a pass
 * that only sketches may rewrite the batch's host arrays then, as after kdf_count_uploaded.  kdf_sketch_registers writes the 2^p bytes to host memory, the _dev form to caller-owned HBM.
 * kdf_sketch_merge: reg = max(own, given) over 2^p host bytes (another engine's registers of the same p: another rank's
 * after an all-reduce(MAX), another shard's); a byte above 65 - p is KDF_ERR_INVALID and nothing is written; complete on
 * return.  kdf_sketch_estimate_registers is the estimate as a pure host function (no engine, no GPU): p = 10..18, a
 * byte above 65 - p is KDF_ERR_INVALID.
 * kdf_spool_sketch adds every segment of a spool in order: HBM-tier segments as they lie, host-tier segments through
 * the engine's two upload slots (they are free again afterwards), as kdf_spool_replay does, with the same refusals
 * (an overflowed spool and a slot that holds a caller's batch KDF_ERR_STATE, another device KDF_ERR_INVALID; no sketch
 * on: KDF_ERR_STATE).  The spool does not change ("replays" counts kdf_spool_replay only).
 * Stats (kdf_get_stat): "sketch_state" (0 / 1), "sketch_log2_registers", "sketch_windows" (windows THIS engine added
 * since begin: a merge does not change it), and under kdf_profile(h, 1) "sketch_us" / "sketch_passes" (the add
 * kernels, HIP events). */
int kdf_sketch_begin(kdf_engine *h, uint32_t log2_registers);
int kdf_sketch_add_reads(kdf_engine *h, const uint64_t *packed, const uint64_t *invalid, uint64_t n_bases);
int kdf_sketch_add_reads_dev(kdf_engine *h, const void *d_packed, const void *d_invalid, uint64_t n_bases);
int kdf_sketch_add_uploaded(kdf_engine *h, int slot);
int kdf_sketch_registers(kdf_engine *h, uint8_t *regs_out);
int kdf_sketch_registers_dev(kdf_engine *h, void *d_regs_out);
int kdf_sketch_merge(kdf_engine *h, const uint8_t *regs);
int kdf_sketch_estimate(kdf_engine *h, double *distinct_out);
int kdf_sketch_drop(kdf_engine *h);
int kdf_sketch_estimate_registers(const uint8_t *regs, uint32_t log2_registers, double *distinct_out);
int kdf_spool_sketch(kdf_spool *sp, kdf_engine *h);

#ifdef __cplusplus
}
#endif
#endif /* KDF_H */
