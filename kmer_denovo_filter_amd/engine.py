"""KmerEngine: Python face of one libkdf engine handle (one GPU, one table).

The methods map one-to-one onto the Jellyfish sub-commands the reference
shells out to ("External op" table):

    count(stream)            jellyfish count -m k -C            (insert mode)
    load_filter(keys)        --if filter.fa
    count_filtered(stream)   jellyfish count -m k -C --if ...
    export_ge(n)             jellyfish dump -c -L n             (ascending keys)
    histogram(high)          jellyfish histo -h high
    export_join(other, ...)  jellyfish dump -L a -U b, kept by the count in another table (ascending keys)
    count_stats()            jellyfish stats
    prefilter_*()            jellyfish bc + count --bc          (exact: two passes)
    sketch_*()               (no Jellyfish call) distinct k-mers of a stream, estimated without storing them
    query(keys)              jellyfish query idx -s kmers.fa    (input order)
    scan(stream)             JellyfishKmerQuery / Module-3 probe
    read_hits(stream)        ... and its per-read hits / distinct on the device
    hit_coverage(...)        ... and its hits in reference coordinates (k-mer / read coverage)
    cluster_intervals(...)   ... and its regions; group_distinct(...): the distinct k-mers of each
    format_kmers(keys)       the k-mer files between the stages, `>{i}\\n{KMER}\\n`, as text; parse_kmer_fasta(text): back

Long k-mers (odd k from 65 to 201) get a "long" engine (``engine.long``): its
keys are ``(n, key_words)`` C-contiguous uint64 arrays, word 0 the least
significant, passed and returned in the ``lo`` position with ``hi=None`` (so
``export_ge`` returns ``(keys, None, counts)``).  The read-stream methods are the
same for every k.  Across ranks a long engine has its own owner exchange:
``export_parts_w_packed_dev`` (the dump grouped by ``distributed.owner_of_w``),
``add_pairs_dev`` per received segment and ``set_counts_w_dev``; the (lo, hi)
owner-ordered dump, the multi-segment merge, ``set_counts_dev`` and ``hash_shift``
stay refused.  The mirrors take that path only under ``KDF_LONG_RANKS=1``; it has
run as several ranks on one GPU over gloo, never over RCCL.

No CPU fallback: constructing an engine without libkdf.so or without a GPU
raises.
"""
from __future__ import annotations

from ctypes import POINTER, byref, c_uint32, c_uint64, c_void_p
from typing import Optional, Tuple

import numpy as np

from . import _native
from .keys import key_words
from .reads import ReadStream, stream_words


def _vp(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


# layouts of KmerEngine.format_kmers (KDF_TEXT_FASTA, KDF_TEXT_ROWS)
TEXT_FASTA, TEXT_ROWS = 0, 1


class KmerFastaError(ValueError):
    """A line of k-mer FASTA text breaks the rule (``KmerEngine.parse_kmer_fasta``): ``offset`` is that of the first byte
    of the chunk's first bad line, ``rule`` is "length" or "base"."""

    def __init__(self, msg: str, offset: int):
        super().__init__(msg)
        self.offset = int(offset)
        self.rule = "base" if "non-ACGT" in msg else "length"


class IndexRecordError(ValueError):
    """A record of an index holds a key with a bit at or above 2k (``KmerEngine.index_decode``): ``record`` is the index
    of the first such record of the decoded block."""

    def __init__(self, msg: str, record: int):
        super().__init__(msg)
        self.record = int(record)


class KmerEngine:
    MAX_K = 63                # (lo, hi) keys
    LONG_MIN_K, LONG_MAX_K = 65, 201   # long engines: odd k only, (n, key_words) keys

    def __init__(self, k: int, capacity_hint: int = 1 << 20, device: int = 0):
        if key_words(k) == 0:
            raise ValueError(f"k={k} outside the engine's range 1..{self.MAX_K} or odd "
                             f"{self.LONG_MIN_K}..{self.LONG_MAX_K}")
        self._lib = _native.load()
        self.k = int(k)
        self.key_words = key_words(self.k)
        self.long = self.key_words > 2
        self.wide = self.k > 32
        self.device = int(device)
        h = c_void_p()
        rc = self._lib.kdf_create(self.device, self.k, int(capacity_hint), byref(h))
        _native.check(rc, None)
        self._h = h

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.kdf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        _native.check(rc, self._h)

    def set_stream(self, hip_stream: Optional[int]):
        """Launch on an external hipStream_t (e.g. ``torch.cuda.current_stream().cuda_stream``)."""
        self._ck(self._lib.kdf_set_stream(self._h, c_void_p(hip_stream) if hip_stream else None))

    def synchronize(self):
        self._ck(self._lib.kdf_synchronize(self._h))

    def flush(self):
        """Apply everything the count calls have deferred (pending stream, partitioned passes) to the table now."""
        self._ck(self._lib.kdf_flush(self._h))
        return self

    def clear(self):
        self._ck(self._lib.kdf_clear(self._h))

    def reserve(self, n_keys: int):
        self._ck(self._lib.kdf_reserve(self._h, int(n_keys)))

    def stats(self) -> Tuple[int, int, int]:
        """(capacity slots, distinct keys, valid windows counted since clear)."""
        c, d, w = c_uint64(0), c_uint64(0), c_uint64(0)
        self._ck(self._lib.kdf_stats(self._h, byref(c), byref(d), byref(w)))
        return c.value, d.value, w.value

    def set_option(self, name: str, value: int):
        self._ck(self._lib.kdf_set_option(self._h, name.encode(), int(value)))

    def get_stat(self, name: str) -> int:
        from ctypes import c_int64
        v = c_int64(0)
        self._ck(self._lib.kdf_get_stat(self._h, name.encode(), byref(v)))
        return v.value

    def profile(self, enable: bool = True):
        self._ck(self._lib.kdf_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        """(kernel ms, launches, stream positions) of the stream kernel since profile(True)."""
        import ctypes
        ms, n, p = ctypes.c_double(0), c_uint64(0), c_uint64(0)
        self._ck(self._lib.kdf_profile_read(self._h, byref(ms), byref(n), byref(p)))
        return ms.value, n.value, p.value

    def profile_stages(self):
        """([A0 hist+scans, A1 scatter, B finesort, C bucket] summed ms, binned passes)."""
        import ctypes
        ms = (ctypes.c_double * 4)()
        n = c_uint64(0)
        self._ck(self._lib.kdf_profile_stages(self._h, ms, byref(n)))
        return list(ms), n.value

    _PATHS = ("direct", "binned", "-", "sieve", "-", "bin_sieve")
    _STAGES = ["kb_slabsort_kernel", "kb_groupsum+kb_plan", "kb_piecesort_pipe_kernel", "kb_bucket_kernel"]

    def last_count_path(self) -> str:
        """Which pipeline the last count call took: direct / binned / sieve / bin_sieve (option sieve_bins)."""
        return self._PATHS[self.get_stat("last_count_path")]

    def profile_stage_names(self):
        return list(self._STAGES)

    def _rows(self, keys) -> np.ndarray:
        """Long engines: keys as an (n, key_words) C-contiguous uint64 array."""
        a = np.ascontiguousarray(keys, dtype=np.uint64)
        if a.ndim == 1 and a.size == 0:
            a = a.reshape(0, self.key_words)
        if a.ndim != 2 or a.shape[1] != self.key_words:
            raise ValueError(f"k={self.k}: keys must be an (n, {self.key_words}) uint64 array, got shape {a.shape}")
        return a

    # -- count / filter ----------------------------------------------------
    def count(self, stream: ReadStream):
        self._ck(self._lib.kdf_count_reads(self._h, _vp(stream.packed), _vp(stream.invalid), stream.n_bases))
        return self

    def upload_async(self, slot: int, stream: ReadStream):
        """Copy a host batch into device staging slot 0 / 1 on the engine's copy stream (asynchronous when the
        arrays are pinned, reads.PinnedBatches); count it later with count_uploaded(slot)."""
        self._ck(self._lib.kdf_upload_reads_async(self._h, int(slot), _vp(stream.packed), _vp(stream.invalid), stream.n_bases))
        return self

    def count_uploaded(self, slot: int, filtered: bool = False):
        self._ck(self._lib.kdf_count_uploaded(self._h, int(slot), 1 if filtered else 0))
        return self

    def count_dev(self, d_packed: int, d_invalid: int, n_bases: int):
        """Stream resident in HBM (raw device pointers to buffers of the stream_words(n_bases) sizes; positions at or
        past n_bases are invalid whatever those words hold, so zero padding or a prefix of a longer stream is fine).
        The engine launches on its own stream unless set_stream() was called:
        the buffers must be complete (synchronise the producer) before the call."""
        self._ck(self._lib.kdf_count_reads_dev(self._h, c_void_p(d_packed), c_void_p(d_invalid), int(n_bases)))
        return self

    def add_pairs(self, lo: np.ndarray, hi: Optional[np.ndarray] = None, counts: Optional[np.ndarray] = None):
        """Insert-or-add (key, count) pairs (index load / `jellyfish merge`)."""
        if self.long:
            keys = self._rows(lo)
            cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
            self._ck(self._lib.kdf_add_pairs_w(self._h, _vp(keys), _vp(cnt), len(keys)))
            return self
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        hi = np.ascontiguousarray(hi, dtype=np.uint64) if self.wide else None
        cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        self._ck(self._lib.kdf_add_pairs(self._h, _vp(lo), _vp(hi), _vp(cnt), len(lo)))
        return self

    def add_pairs_dev(self, d_lo: int, d_hi: Optional[int], d_counts: Optional[int], n: int):
        if self.long:          # d_lo: n x key_words row-major words
            self._ck(self._lib.kdf_add_pairs_w_dev(self._h, c_void_p(d_lo), c_void_p(d_counts) if d_counts else None, int(n)))
            return self
        self._ck(self._lib.kdf_add_pairs_dev(self._h, c_void_p(d_lo), c_void_p(d_hi) if d_hi else None,
                                             c_void_p(d_counts) if d_counts else None, int(n)))
        return self

    def set_counts_dev(self, d_lo: int, d_hi: Optional[int], d_counts: int, n: int):
        """The count of every listed (stored) key becomes d_counts[i] (``kdf_set_counts_dev``)."""
        self._ck(self._lib.kdf_set_counts_dev(self._h, c_void_p(d_lo), c_void_p(d_hi) if d_hi else None, c_void_p(d_counts), int(n)))
        return self

    def set_counts_w_dev(self, d_keys: int, d_counts: int, n: int):
        """Long engines: the count of every listed (stored) key row becomes d_counts[i] (``kdf_set_counts_w_dev``;
        ``d_keys``: n x key_words row-major words).  A row that is not stored raises, after the stored ones were set."""
        self._ck(self._lib.kdf_set_counts_w_dev(self._h, c_void_p(d_keys) if d_keys else None,
                                                c_void_p(d_counts) if d_counts else None, int(n)))
        return self

    def add_pairs_multi_dev(self, segments):
        """Sum several device-resident segments of (lo ptr, hi ptr or None, counts ptr, n) into the table in ONE call
        (the owner's half of the multi-GPU merge, ``kdf_add_pairs_multi_dev``)."""
        segs = [s for s in segments if s[3]]
        if not segs:
            return self
        m = len(segs)
        lo = (c_void_p * m)(*[s[0] for s in segs])
        hi = (c_void_p * m)(*[s[1] or None for s in segs])
        cnt = (c_void_p * m)(*[s[2] for s in segs])
        n = (c_uint64 * m)(*[int(s[3]) for s in segs])
        self._ck(self._lib.kdf_add_pairs_multi_dev(self._h, m, lo, hi if self.wide else None, cnt, n))
        return self

    def load_filter(self, lo: np.ndarray, hi: Optional[np.ndarray] = None):
        if self.long:
            keys = self._rows(lo)
            self._ck(self._lib.kdf_load_filter_w(self._h, _vp(keys), len(keys)))
            return self
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        if self.wide:
            if hi is None:
                raise ValueError("wide keys (k > 32) need the hi words")
            hi = np.ascontiguousarray(hi, dtype=np.uint64)
        else:
            hi = None
        self._ck(self._lib.kdf_load_filter(self._h, _vp(lo), _vp(hi), len(lo)))
        return self

    def load_filter_dev(self, d_lo: int, d_hi: Optional[int], n: int):
        """Filter keys already resident in HBM (raw device pointers)."""
        if self.long:
            self._ck(self._lib.kdf_load_filter_w_dev(self._h, c_void_p(d_lo), int(n)))
            return self
        self._ck(self._lib.kdf_load_filter_dev(self._h, c_void_p(d_lo), c_void_p(d_hi) if d_hi else None, int(n)))
        return self

    def reset_counts(self):
        """Zero every count, keep the keys (the same filter against the next parent)."""
        self._ck(self._lib.kdf_reset_counts(self._h))
        return self

    def count_filtered(self, stream: ReadStream):
        self._ck(self._lib.kdf_count_reads_filtered(self._h, _vp(stream.packed), _vp(stream.invalid),
                                                    stream.n_bases))
        return self

    def count_filtered_dev(self, d_packed: int, d_invalid: int, n_bases: int):
        self._ck(self._lib.kdf_count_reads_filtered_dev(self._h, c_void_p(d_packed), c_void_p(d_invalid),
                                                        int(n_bases)))
        return self

    # -- two-pass counting (kdf.h "two-pass counting") ----------------------
    def prefilter_begin(self, min_count: int = 3, log2_cells: int = 0):
        """Start pass 1: a counting sieve of 2^log2_cells cells (0: sized from the capacity hint).  Tally every batch
        with prefilter_add*, then prefilter_arm(); the insert-mode counts that follow only store keys whose cell
        reads >= min_count (2 or 3), with their full counts."""
        self._ck(self._lib.kdf_prefilter_begin(self._h, int(min_count), int(log2_cells)))
        return self

    def prefilter_add(self, stream: ReadStream):
        self._ck(self._lib.kdf_prefilter_add_reads(self._h, _vp(stream.packed), _vp(stream.invalid), stream.n_bases))
        return self

    def prefilter_add_dev(self, d_packed: int, d_invalid: int, n_bases: int):
        self._ck(self._lib.kdf_prefilter_add_reads_dev(self._h, c_void_p(d_packed), c_void_p(d_invalid), int(n_bases)))
        return self

    def prefilter_add_uploaded(self, slot: int):
        """Tally the batch upload_async() put into staging slot 0 / 1."""
        self._ck(self._lib.kdf_prefilter_add_uploaded(self._h, int(slot)))
        return self

    def prefilter_arm(self):
        self._ck(self._lib.kdf_prefilter_arm(self._h))
        return self

    def prefilter_drop(self):
        self._ck(self._lib.kdf_prefilter_drop(self._h))
        return self

    def prefilter_fill(self):
        """[cells reading 0, 1, 2, 3] of the sieve."""
        v = (c_uint64 * 4)()
        self._ck(self._lib.kdf_prefilter_fill(self._h, v))
        return [int(x) for x in v]

    def prefilter_words(self) -> int:
        """Number of 64-bit words of the sieve (sixteen cells each): 2^(log2_cells - 4)."""
        n = c_uint64(0)
        self._ck(self._lib.kdf_prefilter_words(self._h, byref(n)))
        return n.value

    def prefilter_export(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Words [first, first + n) of the sieve (n None: to its end) as a numpy uint64 array; tallying or armed."""
        if n is None:
            n = self.prefilter_words() - int(first)
        out = np.empty(max(int(n), 0), dtype=np.uint64)
        self._ck(self._lib.kdf_prefilter_export(self._h, int(first), int(n), _vp(out)))
        return out

    def prefilter_export_dev(self, d_out: int, first: int, n: int):
        """The same into HBM (raw device pointer to n words); complete on return."""
        self._ck(self._lib.kdf_prefilter_export_dev(self._h, int(first), int(n), c_void_p(d_out) if d_out else None))
        return self

    def prefilter_merge(self, segments, first: int = 0, replace: bool = False):
        """Saturating sum of the segments (uint64 arrays of one length: other engines' exports of the same words) into
        words [first, first + len) of the sieve; ``replace``: the sieve's own values are left out.  Only while tallying."""
        segs = [np.ascontiguousarray(s, dtype=np.uint64) for s in segments]
        n = len(segs[0]) if segs else 0
        if any(s.ndim != 1 or len(s) != n for s in segs):
            raise ValueError("prefilter_merge: the segments must be 1-d arrays of one length")
        if n == 0:                                                  # (an empty array need not have an address)
            segs = [np.zeros(1, dtype=np.uint64) for _ in segs]
        ptrs = (c_void_p * max(len(segs), 1))(*[s.ctypes.data for s in segs])
        self._ck(self._lib.kdf_prefilter_merge(self._h, int(first), n, len(segs), ptrs, 1 if replace else 0))
        return self

    def prefilter_merge_dev(self, d_segments, first: int, n: int, replace: bool = False):
        """The same with the segments in HBM (raw device pointers to n words each), ONE kernel launch for all of them;
        runs in stream order: synchronize() before the segments are reused."""
        segs = list(d_segments)
        ptrs = (c_void_p * max(len(segs), 1))(*[p or None for p in segs])
        self._ck(self._lib.kdf_prefilter_merge_dev(self._h, int(first), int(n), len(segs), ptrs, 1 if replace else 0))
        return self

    # -- distinct k-mer sketch (kdf.h "distinct k-mer sketch") ----------------
    def sketch_begin(self, log2_registers: int = 0):
        """Start a HyperLogLog sketch of 2^log2_registers registers (10..18; 0: 16) over the canonical k-mers of the
        streams given to sketch_add*.  Independent of the table, the mode and a prefilter; survives clear()."""
        self._ck(self._lib.kdf_sketch_begin(self._h, int(log2_registers)))
        return self

    def sketch_add(self, stream: ReadStream):
        self._ck(self._lib.kdf_sketch_add_reads(self._h, _vp(stream.packed), _vp(stream.invalid), stream.n_bases))
        return self

    def sketch_add_dev(self, d_packed: int, d_invalid: int, n_bases: int):
        """Stream resident in HBM (raw device pointers, as count_dev); stream order, does not synchronise."""
        self._ck(self._lib.kdf_sketch_add_reads_dev(self._h, c_void_p(d_packed), c_void_p(d_invalid), int(n_bases)))
        return self

    def sketch_add_uploaded(self, slot: int):
        """Sketch the batch upload_async() put into staging slot 0 / 1; the slot keeps it (count or tally it next)."""
        self._ck(self._lib.kdf_sketch_add_uploaded(self._h, int(slot)))
        return self

    def sketch_registers(self) -> np.ndarray:
        """The registers, uint8[2^log2_registers]."""
        out = np.zeros(1 << self.get_stat("sketch_log2_registers"), np.uint8)
        self._ck(self._lib.kdf_sketch_registers(self._h, _vp(out)))
        return out

    def sketch_registers_dev(self, d_out: int):
        """The same into caller-owned HBM (raw device pointer to 2^log2_registers bytes); complete on return."""
        self._ck(self._lib.kdf_sketch_registers_dev(self._h, c_void_p(d_out) if d_out else None))
        return self

    def sketch_merge(self, regs):
        """reg = max(own, regs): another engine's registers of the same size (another rank's, another shard's)."""
        regs = np.ascontiguousarray(regs, dtype=np.uint8)
        m = 1 << self.get_stat("sketch_log2_registers")
        if self.get_stat("sketch_state") and (regs.ndim != 1 or len(regs) != m):      # (no sketch: the engine says so)
            raise ValueError(f"sketch_merge: {regs.shape} registers for a sketch of {m}")
        self._ck(self._lib.kdf_sketch_merge(self._h, _vp(regs)))
        return self

    def sketch_estimate(self) -> float:
        """Estimated number of distinct canonical k-mers among the windows sketched (and merged) so far."""
        import ctypes
        v = ctypes.c_double(0.0)
        self._ck(self._lib.kdf_sketch_estimate(self._h, byref(v)))
        return v.value

    def sketch_drop(self):
        self._ck(self._lib.kdf_sketch_drop(self._h))
        return self

    # -- device BAM feeder (kdf.h "device BAM feeder") ---------------------------
    def bgzf_inflate_dev(self, d_comp: int, d_blocks: int, n_blocks: int, d_out: int, out_cap: int, d_status: Optional[int] = None):
        """Inflate ``n_blocks`` BGZF blocks on the device (raw device pointers: payload bytes, the block table of
        ``reads.BGZF_BLOCK_DTYPE``, the output of ``out_cap`` bytes, optionally uint32[n_blocks] for the decoder's
        statuses).  Blocks the device decoder rejects are inflated by zlib and patched in (stat
        ``bamdev_fallback_blocks``); one zlib rejects too raises KDF_ERR_IO.  Complete on return."""
        self._ck(self._lib.kdf_bgzf_inflate_dev(self._h, c_void_p(d_comp) if d_comp else None, c_void_p(d_blocks) if d_blocks else None,
                                                int(n_blocks), c_void_p(d_out) if d_out else None, int(out_cap),
                                                c_void_p(d_status) if d_status else None))
        return self

    def bamdev_decode_dev(self, d_comp: int, d_blocks: int, n_blocks: int, d_subs: int, n_sub: int, flag_off: int, collapse: bool,
                          d_packed: int, d_invalid: int, cap_bases: int, d_offsets: int, cap_reads: int):
        """One planned batch (``reads.bam_raw_reader``) -> the packed stream in caller-owned HBM, in the layout of
        the host readers.  -> (n_bases, n_reads, sub_status uint32[n_sub]); the stream holds the sub-ranges before the
        first whose status is not 0.  Synchronises once; the stream itself is complete in the engine's stream order."""
        nb, nr = c_uint64(0), c_uint64(0)
        status = np.zeros(max(int(n_sub), 1), np.uint32)
        self._ck(self._lib.kdf_bamdev_decode_dev(self._h, c_void_p(d_comp) if d_comp else None, c_void_p(d_blocks) if d_blocks else None,
                                                 int(n_blocks), c_void_p(d_subs) if d_subs else None, int(n_sub), int(flag_off),
                                                 1 if collapse else 0, c_void_p(d_packed), c_void_p(d_invalid), int(cap_bases),
                                                 c_void_p(d_offsets), int(cap_reads), byref(nb), byref(nr), _vp(status)))
        return nb.value, nr.value, status[:int(n_sub)]

    # -- device FASTA feeder -------------------------------------------------
    def fasta_pack_dev(self, d_text: Optional[int], n_bytes: int, final_chunk: bool, state: "_native.FastaState", d_packed: int,
                       d_invalid: int, cap_bases: int, d_offsets: Optional[int] = None, cap_reads: int = 0,
                       d_prev_packed: Optional[int] = None, d_prev_invalid: Optional[int] = None, prev_n_bases: int = 0,
                       carry: int = 0) -> Tuple[int, int, int]:
        """One chunk of raw FASTA text in HBM -> the slice of the file's packed stream that belongs to the bytes the call
        consumes, in caller-owned HBM (buffers of the ``stream_words(cap_bases)`` sizes; ``d_offsets``: int64[cap_reads +
        1] or None), behind the last ``min(carry, prev_n_bases)`` positions of the previous stream when the chunk begins
        inside a record (``carry = k - 1``).  ``state``: a ``FastaState``, zero before the first chunk, updated by the
        call.  -> (n_bases, n_reads, consumed): a chunk that is not the last leaves a trailing run of '\\r' to the
        caller.  Synchronises once; the table is not touched."""
        p = lambda x: c_void_p(x) if x else None
        nb, nr, used = c_uint64(0), c_uint64(0), c_uint64(0)
        self._ck(self._lib.kdf_fasta_pack_dev(self._h, p(d_text), int(n_bytes), int(bool(final_chunk)), byref(state), p(d_prev_packed),
                                              p(d_prev_invalid), int(prev_n_bases), int(carry), p(d_packed), p(d_invalid), int(cap_bases),
                                              p(d_offsets), int(cap_reads), byref(nb), byref(nr), byref(used)))
        return nb.value, nr.value, used.value

    def fasta_pack(self, text, final_chunk: bool, state: "_native.FastaState", prev: Optional[ReadStream] = None, carry: int = 0,
                   want_offsets: bool = True) -> Tuple[ReadStream, int]:
        """The same from host bytes to a host ``ReadStream`` (offsets: the call's records, piece 0 with the carry),
        staged through the engine.  -> (stream, consumed)."""
        raw = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        n = len(raw)
        cap_bases = n + int(carry) + 1
        cap_reads = n // 2 + 2
        pw, mw = stream_words(cap_bases)
        packed, invalid = np.zeros(pw, np.uint64), np.zeros(mw, np.uint64)
        offs = np.zeros(cap_reads + 1, np.int64) if want_offsets else None
        nb, nr, used = c_uint64(0), c_uint64(0), c_uint64(0)
        self._ck(self._lib.kdf_fasta_pack(self._h, _vp(raw) if n else None, n, int(bool(final_chunk)), byref(state),
                                          _vp(prev.packed) if prev is not None else None, _vp(prev.invalid) if prev is not None else None,
                                          prev.n_bases if prev is not None else 0, int(carry), _vp(packed), _vp(invalid), cap_bases,
                                          _vp(offs), cap_reads if want_offsets else 0, byref(nb), byref(nr), byref(used)))
        pw, mw = stream_words(nb.value)
        offsets = offs[:nr.value + 1].copy() if want_offsets else np.array([0, nb.value], np.int64)
        return ReadStream(packed[:pw].copy(), invalid[:mw].copy(), nb.value, offsets), used.value

    # -- device FASTQ feeder -------------------------------------------------
    def _fastq_packed(self, rc, nb, nr, used, bad, rule):
        """(n_bases, n_reads, consumed) of a kdf_fastq_pack call, or its error: a text that is no FASTQ raises
        ``FastqFormatError`` with the offset of the first bad record within the call's text and the rule it breaks."""
        if rc == _native.KDF_ERR_IO and rule.value:
            msg = self._lib.kdf_last_error(self._h)
            raise _native.FastqFormatError(rc, msg.decode(errors="replace") if msg else "bad record", bad.value, rule.value)
        self._ck(rc)
        return nb.value, nr.value, used.value

    def fastq_pack_dev(self, d_text: Optional[int], n_bytes: int, final_chunk: bool, state: "_native.FastqState", d_packed: int,
                       d_invalid: int, cap_bases: int, d_offsets: Optional[int] = None, cap_reads: int = 0,
                       min_qual: int = 0) -> Tuple[int, int, int]:
        """One chunk of raw four-line FASTQ text in HBM -> the packed stream of the whole records it holds, in
        caller-owned HBM (buffers of the ``stream_words(cap_bases)`` sizes, ``cap_bases >= n_bytes // 2`` always
        suffices; ``d_offsets``: int64[cap_reads + 1] or None).  A base whose quality byte is below ``min_qual`` (0: off)
        is an invalid position.  ``state``: a ``FastqState``, zero before the first chunk, updated by the call.
        -> (n_bases, n_reads, consumed): a chunk that is not the last leaves its incomplete last record to the caller.
        Synchronises once; the table is not touched."""
        p = lambda x: c_void_p(x) if x else None
        nb, nr, used, bad, rule = c_uint64(0), c_uint64(0), c_uint64(0), c_uint64(0), c_uint32(0)
        rc = self._lib.kdf_fastq_pack(self._h, _native.KDF_MEM_DEVICE, p(d_text), int(n_bytes), int(bool(final_chunk)), int(min_qual), byref(state),
                                      p(d_packed), p(d_invalid), int(cap_bases), p(d_offsets), int(cap_reads), byref(nb), byref(nr), byref(used),
                                      byref(bad), byref(rule))
        return self._fastq_packed(rc, nb, nr, used, bad, rule)

    def fastq_pack(self, text, final_chunk: bool, state: "_native.FastqState", min_qual: int = 0,
                   want_offsets: bool = True) -> Tuple[ReadStream, int]:
        """The same from host bytes to a host ``ReadStream`` (offsets: the call's records), staged through the engine.
        -> (stream, consumed)."""
        raw = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        n = len(raw)
        cap_bases, cap_reads = n // 2, n // 4
        pw, mw = stream_words(cap_bases)
        packed, invalid = np.zeros(pw, np.uint64), np.zeros(mw, np.uint64)
        offs = np.zeros(cap_reads + 1, np.int64) if want_offsets else None
        nb, nr, used, bad, rule = c_uint64(0), c_uint64(0), c_uint64(0), c_uint64(0), c_uint32(0)
        rc = self._lib.kdf_fastq_pack(self._h, _native.KDF_MEM_HOST, _vp(raw) if n else None, n, int(bool(final_chunk)), int(min_qual), byref(state),
                                      _vp(packed), _vp(invalid), cap_bases, _vp(offs), cap_reads if want_offsets else 0, byref(nb), byref(nr),
                                      byref(used), byref(bad), byref(rule))
        self._fastq_packed(rc, nb, nr, used, bad, rule)
        if not final_chunk and used.value == 0:                       # no complete record: nothing was written
            return ReadStream(np.zeros(stream_words(0)[0], np.uint64), np.full(stream_words(0)[1], ~np.uint64(0)), 0, np.zeros(1, np.int64)), 0
        pw, mw = stream_words(nb.value)
        offsets = offs[:nr.value + 1].copy() if want_offsets else np.array([0, nb.value], np.int64)
        return ReadStream(packed[:pw].copy(), invalid[:mw].copy(), nb.value, offsets), used.value

    # -- FASTQ record extract ------------------------------------------------
    def fastq_extract_dev(self, d_text: Optional[int], n_bytes: int, final_chunk: bool, d_keep: Optional[int], n_reads: int, d_out: Optional[int],
                          cap_out: int, d_out_offsets: Optional[int] = None) -> Tuple[int, int, int]:
        """The records of one chunk of raw FASTQ text in HBM whose flag in ``d_keep`` (uint8[n_reads], ``n_reads`` as
        ``fastq_pack_dev`` returned it for the same chunk) is nonzero, byte for byte and one behind the other, into
        caller-owned HBM of ``cap_out`` bytes (``n_bytes + 2`` always suffices; ``d_out_offsets``: int64[n_reads + 1] or
        None).  -> (out_bytes, n_kept, consumed).  A text that is no FASTQ raises ``FastqFormatError`` as ``fastq_pack_dev``
        does.  Synchronises once; the table is not touched."""
        p = lambda x: c_void_p(x) if x else None
        ob, nk, used, bad, rule = c_uint64(0), c_uint64(0), c_uint64(0), c_uint64(0), c_uint32(0)
        rc = self._lib.kdf_fq_extract(self._h, _native.KDF_MEM_DEVICE, p(d_text), int(n_bytes), int(bool(final_chunk)), p(d_keep), int(n_reads),
                                         p(d_out), int(cap_out), p(d_out_offsets), byref(ob), byref(nk), byref(used), byref(bad), byref(rule))
        return self._fastq_packed(rc, ob, nk, used, bad, rule)

    def fastq_extract(self, text, final_chunk: bool, keep, want_offsets: bool = False):
        """The same from host bytes and a host array of flags, staged through the engine.  -> (bytes, consumed), or
        (bytes, offsets int64[n_kept + 1], consumed) with ``want_offsets``."""
        raw = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        flags = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        n, nr = len(raw), len(flags)
        out = np.zeros(n + 2, np.uint8)
        offs = np.zeros(nr + 1, np.int64) if want_offsets else None
        ob, nk, used, bad, rule = c_uint64(0), c_uint64(0), c_uint64(0), c_uint64(0), c_uint32(0)
        rc = self._lib.kdf_fq_extract(self._h, _native.KDF_MEM_HOST, _vp(raw) if n else None, n, int(bool(final_chunk)), _vp(flags) if nr else None, nr,
                                         _vp(out), n + 2, _vp(offs), byref(ob), byref(nk), byref(used), byref(bad), byref(rule))
        self._fastq_packed(rc, ob, nk, used, bad, rule)
        data = out[:ob.value].tobytes()
        return (data, offs[:nk.value + 1].copy(), used.value) if want_offsets else (data, used.value)

    # -- query / dump ------------------------------------------------------
    def query(self, lo: np.ndarray, hi: Optional[np.ndarray] = None) -> np.ndarray:
        if self.long:
            keys = self._rows(lo)
            out = np.zeros(len(keys), dtype=np.uint32)
            self._ck(self._lib.kdf_query_w(self._h, _vp(keys), len(keys), _vp(out)))
            return out
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        hi = np.ascontiguousarray(hi, dtype=np.uint64) if (self.wide and hi is not None) else None
        if self.wide and hi is None:
            raise ValueError("wide keys (k > 32) need the hi words")
        out = np.zeros(len(lo), dtype=np.uint32)
        self._ck(self._lib.kdf_query(self._h, _vp(lo), _vp(hi), len(lo), _vp(out)))
        return out

    def query_dev(self, d_lo: int, d_hi: Optional[int], n: int, d_out: int):
        if self.long:
            self._ck(self._lib.kdf_query_w_dev(self._h, c_void_p(d_lo), int(n), c_void_p(d_out)))
            return
        self._ck(self._lib.kdf_query_dev(self._h, c_void_p(d_lo), c_void_p(d_hi) if d_hi else None, int(n),
                                         c_void_p(d_out)))

    def count_ge(self, min_count: int) -> int:
        n = c_uint64(0)
        self._ck(self._lib.kdf_count_ge(self._h, int(min_count), byref(n)))
        return n.value

    HISTO_MAX_HIGH = (1 << 24) - 1   # kdf_histogram's limit on `high`

    def histogram(self, high: int = 10000) -> np.ndarray:
        """`jellyfish histo -h high`: uint64[high + 2]; bins[c] = stored keys with count exactly c (bins[0]: keys
        stored with count 0, as count_ge(0) counts them), bins[high + 1] = keys with a count above ``high``."""
        if not 0 <= int(high) <= self.HISTO_MAX_HIGH:
            raise ValueError(f"high={high} outside 0..{self.HISTO_MAX_HIGH}")
        bins = np.zeros(int(high) + 2, np.uint64)
        self._ck(self._lib.kdf_histogram(self._h, int(high), _vp(bins)))
        return bins

    def histogram_dev(self, high: int, d_bins: int):
        """The same into caller-owned HBM: ``d_bins`` is a raw device pointer to high + 2 64-bit words."""
        if not 0 <= int(high) <= self.HISTO_MAX_HIGH:
            raise ValueError(f"high={high} outside 0..{self.HISTO_MAX_HIGH}")
        self._ck(self._lib.kdf_histogram_dev(self._h, int(high), c_void_p(d_bins)))
        return self

    def count_stats(self) -> dict:
        """`jellyfish stats`: {"unique": keys with count 1, "distinct": keys with count >= 1, "total": sum of all
        counts, "max_count": largest count (0 for an empty table)}."""
        u, d, t, m = c_uint64(0), c_uint64(0), c_uint64(0), c_uint64(0)
        self._ck(self._lib.kdf_count_stats(self._h, byref(u), byref(d), byref(t), byref(m)))
        return {"unique": u.value, "distinct": d.value, "total": t.value, "max_count": m.value}

    def export_ge(self, min_count: int = 0):
        """(lo, hi, counts) of entries with count >= min_count, ascending key order
        (long engines: (keys (n, key_words), None, counts))."""
        n = self.count_ge(min_count)
        if self.long:
            keys = np.zeros((n, self.key_words), np.uint64)
            cnt = np.zeros(n, np.uint32)
            got = c_uint64(0)
            self._ck(self._lib.kdf_export_ge_w(self._h, int(min_count), _vp(keys), _vp(cnt), n, byref(got)))
            if got.value != n:
                raise _native.KdfError(_native.KDF_ERR_STATE, "export size changed between passes")
            return keys, None, cnt
        lo = np.zeros(n, np.uint64)
        hi = np.zeros(n, np.uint64)
        cnt = np.zeros(n, np.uint32)
        got = c_uint64(0)
        self._ck(self._lib.kdf_export_ge(self._h, int(min_count), _vp(lo), _vp(hi), _vp(cnt), n, byref(got)))
        if got.value != n:
            raise _native.KdfError(_native.KDF_ERR_STATE, "export size changed between passes")
        return lo, hi, cnt

    def export_ge_dev(self, min_count: int, d_lo: int, d_hi: Optional[int], d_cnt: Optional[int], cap: int,
                      sorted_: bool = False) -> int:
        """Dump into caller-owned device buffers; returns the number of entries (long engines: d_lo holds
        cap x key_words row-major words, d_hi is ignored)."""
        n = c_uint64(0)
        if self.long:
            self._ck(self._lib.kdf_export_ge_w_dev(self._h, int(min_count), c_void_p(d_lo),
                                                   c_void_p(d_cnt) if d_cnt else None, int(cap),
                                                   1 if sorted_ else 0, byref(n)))
            return n.value
        self._ck(self._lib.kdf_export_ge_dev(self._h, int(min_count), c_void_p(d_lo),
                                             c_void_p(d_hi) if d_hi else None,
                                             c_void_p(d_cnt) if d_cnt else None, int(cap),
                                             1 if sorted_ else 0, byref(n)))
        return n.value

    # -- table join (kdf.h "Table join") -----------------------------------
    UNBOUNDED = 0xFFFFFFFF     # an upper bound of the join that bounds nothing

    def _join_args(self, other, min_count, max_count, other_min, other_max):
        if other is not None and not isinstance(other, KmerEngine):
            raise TypeError("other must be a KmerEngine or None")
        ub = lambda v: self.UNBOUNDED if v is None else int(v)      # noqa: E731
        return (self._h, other._h if other is not None else None, int(min_count), ub(max_count), int(other_min), ub(other_max))

    def count_join(self, other: Optional["KmerEngine"], min_count: int = 1, max_count: Optional[int] = None,
                   other_min: int = 0, other_max: Optional[int] = 0) -> int:
        """Number of stored keys with min_count <= count <= max_count whose count in ``other`` (0: absent there, or
        stored with count 0) lies in other_min..other_max; every bound inclusive, None as an upper bound: none.
        ``other=None``: the other bounds are ignored (``jellyfish dump -L min_count -U max_count``)."""
        n = c_uint64(0)
        self._ck(self._lib.kdf_count_join(*self._join_args(other, min_count, max_count, other_min, other_max), byref(n)))
        return n.value

    def export_join_dev(self, other: Optional["KmerEngine"], min_count: int, max_count: Optional[int], other_min: int,
                        other_max: Optional[int], d_lo: int, d_hi: Optional[int], d_cnt: Optional[int],
                        d_other_cnt: Optional[int], cap: int, sorted_: bool = False) -> int:
        """The join into caller-owned device buffers (the count_join selection; long engines: d_lo holds
        cap x key_words row-major words, d_hi is ignored); returns the number of entries.  More than ``cap`` raise."""
        n = c_uint64(0)
        args = self._join_args(other, min_count, max_count, other_min, other_max)
        p = lambda v: c_void_p(v) if v else None                    # noqa: E731
        if self.long:
            self._ck(self._lib.kdf_export_join_w_dev(*args, p(d_lo), p(d_cnt), p(d_other_cnt), int(cap), 1 if sorted_ else 0, byref(n)))
        else:
            self._ck(self._lib.kdf_export_join_dev(*args, p(d_lo), p(d_hi), p(d_cnt), p(d_other_cnt), int(cap), 1 if sorted_ else 0,
                                                   byref(n)))
        return n.value

    def export_join(self, other: Optional["KmerEngine"], min_count: int = 1, max_count: Optional[int] = None,
                    other_min: int = 0, other_max: Optional[int] = 0):
        """(keys, counts, other_counts) of the join, ascending key order; keys: (lo, hi) for k <= 63, (n, key_words)
        rows for long engines.  Two passes over the table: count_join sizes the arrays, the host form writes."""
        args = self._join_args(other, min_count, max_count, other_min, other_max)
        n = self.count_join(other, min_count, max_count, other_min, other_max)
        cnt, ocnt = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        got = c_uint64(0)
        if self.long:
            keys = np.zeros((n, self.key_words), np.uint64)
            self._ck(self._lib.kdf_export_join_w(*args, _vp(keys), _vp(cnt), _vp(ocnt), n, byref(got)))
        else:
            lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            self._ck(self._lib.kdf_export_join(*args, _vp(lo), _vp(hi), _vp(cnt), _vp(ocnt), n, byref(got)))
            keys = (lo, hi)
        if got.value != n:
            raise _native.KdfError(_native.KDF_ERR_STATE, "join size changed between passes")
        return keys, cnt, ocnt

    def export_parts_dev(self, min_count: int, parts: int, d_lo: int, d_hi: Optional[int], d_cnt: Optional[int],
                         cap: int):
        """Dump grouped by owner rank (distributed.owner_of) into caller-owned device
        buffers; returns (entries, per-owner counts)."""
        n = c_uint64(0)
        counts = (c_uint64 * int(parts))()
        self._ck(self._lib.kdf_export_parts_dev(self._h, int(min_count), int(parts), c_void_p(d_lo),
                                                c_void_p(d_hi) if d_hi else None,
                                                c_void_p(d_cnt) if d_cnt else None, int(cap), counts, byref(n)))
        return n.value, [int(x) for x in counts]

    def export_parts_packed_dev(self, min_count: int, parts: int, d_buf: int, cap_bytes: int):
        """The owner-ordered dump written into the packed all-to-all layout; returns (entries, per-owner counts,
        segment byte offsets [parts + 1])."""
        n = c_uint64(0)
        counts = (c_uint64 * int(parts))()
        offs = (c_uint64 * (int(parts) + 1))()
        self._ck(self._lib.kdf_export_parts_packed_dev(self._h, int(min_count), int(parts), c_void_p(d_buf), int(cap_bytes),
                                                       counts, offs, byref(n)))
        return n.value, [int(x) for x in counts], [int(x) for x in offs]

    def export_parts_w_packed_dev(self, min_count: int, parts: int, d_buf: Optional[int], cap_bytes: int):
        """Long engines: the dump grouped by owner rank (``distributed.owner_of_w``) in the packed all-to-all layout --
        per owner one byte segment ``[keys: n_p x key_words uint64 row-major | counts: n_p uint32]``, starts aligned
        to 8; returns (entries, per-owner counts, segment byte offsets [parts + 1]).  Any table size, insert or filter
        mode.  Too few ``cap_bytes`` raise (the message names the bytes needed) and nothing is written."""
        n = c_uint64(0)
        counts = (c_uint64 * max(int(parts), 1))()
        offs = (c_uint64 * (max(int(parts), 1) + 1))()
        self._ck(self._lib.kdf_export_parts_w_packed_dev(self._h, int(min_count), int(parts), c_void_p(d_buf) if d_buf else None,
                                                         int(cap_bytes), byref(n), counts, offs))
        return n.value, [int(x) for x in counts[:int(parts)]], [int(x) for x in offs[:int(parts) + 1]]

    # -- Module-3 scan -----------------------------------------------------
    def scan(self, stream: ReadStream, want_distinct: bool = True):
        """-> (hit_bits uint64[mask words], distinct uint32[n_reads] or None)."""
        _, mw = stream_words(stream.n_bases)
        hits = np.zeros(mw, np.uint64)
        distinct = np.zeros(stream.n_reads, np.uint32) if want_distinct else None
        offs = np.ascontiguousarray(stream.offsets, dtype=np.int64) if want_distinct else None
        self._ck(self._lib.kdf_scan_reads(self._h, _vp(stream.packed), _vp(stream.invalid), stream.n_bases,
                                          _vp(offs), stream.n_reads if want_distinct else 0,
                                          _vp(hits), _vp(distinct)))
        return hits, distinct

    def scan_dev(self, d_packed: int, d_invalid: int, n_bases: int, d_hits: int):
        self._ck(self._lib.kdf_scan_reads_dev(self._h, c_void_p(d_packed), c_void_p(d_invalid), int(n_bases),
                                              c_void_p(d_hits)))

    # -- per-read hits of the scan, on the device -----------------------------
    def read_hits(self, stream: ReadStream, want_bits: bool = False):
        """The scan reduced per read where it is made: uint32 (n_reads, 2), columns ``READ_HITS_COLUMNS`` -- windows of
        the read whose k-mer is stored with count > 0, and the distinct k-mers among them (what Module 3 filters on).
        ``hits`` equals column ``present`` of read_depth, ``distinct`` equals scan()'s.  ``want_bits``: -> (rows,
        hit_bits uint64[mask words]), the mask scan() returns."""
        rows = np.zeros((stream.n_reads, len(READ_HITS_COLUMNS)), np.uint32)
        bits = np.zeros(stream_words(stream.n_bases)[1], np.uint64) if want_bits else None
        offs = np.ascontiguousarray(stream.offsets, dtype=np.int64)
        self._ck(self._lib.kdf_read_hits(self._h, _vp(stream.packed), _vp(stream.invalid), stream.n_bases, _vp(offs),
                                         stream.n_reads, _vp(bits), _vp(rows)))
        return (rows, bits) if want_bits else rows

    def read_hits_dev(self, d_packed: int, d_invalid: int, n_bases: int, d_offsets: int, n_reads: int,
                      d_hit_bits: Optional[int], d_rows: int):
        """The same between device buffers: ``d_offsets`` int64[n_reads + 1], ``d_rows`` uint32[n_reads x 2],
        ``d_hit_bits`` uint64[ceil(n_bases / 64)] or None.  Synchronises the engine's stream once; the rows are complete
        in stream order."""
        self._ck(self._lib.kdf_read_hits_dev(self._h, c_void_p(d_packed), c_void_p(d_invalid), int(n_bases),
                                             c_void_p(d_offsets) if d_offsets else None, int(n_reads),
                                             c_void_p(d_hit_bits) if d_hit_bits else None, c_void_p(d_rows) if d_rows else None))

    def hit_list(self, hit_bits: np.ndarray, n_bases: int, offsets: Optional[np.ndarray] = None, cap: Optional[int] = None):
        """Positions of the set bits of a hit mask below ``n_bases``, ascending: uint64[n]; with ``offsets`` (int64
        [n_reads + 1]) -> (positions, reads int64[n]) where reads[e] is the read that holds positions[e] or -1.
        ``cap`` (default: as many as there are) bounds the output: more hits than that raise, like export_ge_dev."""
        bits = np.ascontiguousarray(hit_bits, dtype=np.uint64)
        if len(bits) * 64 < int(n_bases):
            raise ValueError(f"a mask of {len(bits)} words does not cover {n_bases} positions")
        if cap is None:
            cap = int(np.unpackbits(bits[:(int(n_bases) + 63) // 64].view(np.uint8), bitorder="little")[:int(n_bases)].sum())
        pos = np.zeros(int(cap), np.uint64)
        offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        reads = None if offs is None else np.zeros(int(cap), np.int64)
        n = c_uint64(0)
        self._ck(self._lib.kdf_hit_list(self._h, _vp(bits), int(n_bases), _vp(offs), 0 if offs is None else len(offs) - 1,
                                        _vp(pos), _vp(reads), int(cap), byref(n)))
        return pos[:n.value] if offs is None else (pos[:n.value], reads[:n.value])

    def _hit_list_dev(self, d_hit_bits, n_bases, d_offsets, n_reads, d_positions, d_reads, cap):
        n = c_uint64(0)
        rc = self._lib.kdf_hit_list_dev(self._h, c_void_p(d_hit_bits), int(n_bases), c_void_p(d_offsets) if d_offsets else None,
                                        int(n_reads), c_void_p(d_positions) if d_positions else None,
                                        c_void_p(d_reads) if d_reads else None, int(cap), byref(n))
        return rc, n.value

    def hit_list_dev(self, d_hit_bits: int, n_bases: int, d_offsets: Optional[int], n_reads: int, d_positions: int,
                     d_reads: Optional[int], cap: int) -> int:
        """The same between device buffers (``d_positions`` uint64[cap], ``d_reads`` int64[cap] or None); returns the
        number of hits and raises when it exceeds ``cap`` (at most ``cap`` entries are written).  Synchronises."""
        rc, n = self._hit_list_dev(d_hit_bits, n_bases, d_offsets, n_reads, d_positions, d_reads, cap)
        self._ck(rc)
        return n

    def scan_hits(self, stream: ReadStream):
        """-> (rows uint32 (n_reads, 2), positions int64[n] ascending): read_hits_dev + hit_list_dev over a stream
        uploaded once.  Only the rows and the compacted list come back to the host, never the mask."""
        import torch
        n, nr = int(stream.n_bases), int(stream.n_reads)
        if n == 0 or nr == 0:
            return np.zeros((nr, len(READ_HITS_COLUMNS)), np.uint32), np.zeros(0, np.int64)
        dev = torch.device("cuda", self.device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(np.int64)).to(dev)
        pw, mw = stream_words(n)
        if len(stream.packed) < pw or len(stream.invalid) < mw:
            raise ValueError(f"stream arrays are smaller than stream_words({n}) = ({pw}, {mw})")
        dp, dm = up(stream.packed[:pw], np.uint64), up(stream.invalid[:mw], np.uint64)
        do = up(stream.offsets, np.int64)
        dbits = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
        drows = torch.empty(nr, dtype=torch.int64, device=dev)               # one row = 2 x uint32
        torch.cuda.synchronize(dev)
        self.read_hits_dev(dp.data_ptr(), dm.data_ptr(), n, do.data_ptr(), nr, dbits.data_ptr(), drows.data_ptr())
        self.synchronize()
        rows = drows.cpu().numpy().view(np.uint32).reshape(nr, 2)
        cap = int(rows[:, 0].sum(dtype=np.int64))
        while True:
            dpos = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            rc, got = self._hit_list_dev(dbits.data_ptr(), n, None, 0, dpos.data_ptr(), None, cap)
            if got <= cap:
                self._ck(rc)
                break
            cap = got                                                     # (hits outside every read: not in the rows)
        return rows, dpos[:got].cpu().numpy()

    def scan_informative(self, stream: ReadStream, min_distinct: int = 1):
        """Module 3's selection on the device: -> (read_indices int64[m], distinct uint32[m], [hit offsets int64 of each
        of those reads, relative to the read's start]) for the reads with at least ``min_distinct`` distinct hit
        k-mers (``min_distinct`` <= 0: every read, as the reference keeps them)."""
        rows, pos = self.scan_hits(stream)
        offs = np.asarray(stream.offsets, dtype=np.int64)
        keep = np.flatnonzero(rows[:, 1] >= min_distinct) if min_distinct > 0 else np.arange(stream.n_reads)
        lo = np.searchsorted(pos, offs[keep], side="left")
        hi = np.searchsorted(pos, offs[keep + 1], side="left") if len(keep) else lo
        per_read = [pos[a:b] - s for a, b, s in zip(lo.tolist(), hi.tolist(), offs[keep].tolist())]
        return keep.astype(np.int64), rows[keep, 1].copy(), per_read

    # -- hits in reference coordinates ------------------------------------------
    def hit_coverage(self, hit_bits: np.ndarray, n_bases: int, offsets: np.ndarray, ref_start: np.ndarray,
                     cigar: np.ndarray, cigar_offsets: np.ndarray, kmer_cov: np.ndarray, read_cov: np.ndarray):
        """Add the hits of a mask to two per-position sums in reference coordinates (``include/kdf.h``, "hits in
        reference coordinates"): ``kmer_cov[g]`` gains the number of hit k-mers of a read that cover reference position
        g, ``read_cov[g]`` gains 1 per such read.  ``offsets`` int64[n_reads + 1], ``ref_start`` int64[n_reads] (the
        linear coordinate of each read's leftmost base, < 0: the read is skipped), ``cigar`` uint32 in BAM encoding with
        ``cigar_offsets`` int64[n_reads + 1] (``ReadStream.cigar`` / ``cigar_offsets``).  The two accumulators are
        C-contiguous uint32 arrays of one length, changed IN PLACE and only added to: batches accumulate."""
        bits = np.ascontiguousarray(hit_bits, dtype=np.uint64)
        if len(bits) * 64 < int(n_bases):
            raise ValueError(f"a mask of {len(bits)} words does not cover {n_bases} positions")
        for a in (kmer_cov, read_cov):
            if a.dtype != np.uint32 or not a.flags.c_contiguous or a.ndim != 1 or len(a) != len(kmer_cov):
                raise ValueError("kmer_cov and read_cov must be C-contiguous uint32 arrays of one length")
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        rs = np.ascontiguousarray(ref_start, dtype=np.int64)
        cg = np.ascontiguousarray(cigar, dtype=np.uint32)
        co = np.ascontiguousarray(cigar_offsets, dtype=np.int64)
        n_reads = len(offs) - 1
        if n_reads > 0 and (len(rs) != n_reads or len(co) != n_reads + 1):
            raise ValueError(f"{n_reads} reads, {len(rs)} ref_start and {len(co)} cigar_offsets entries")
        self._ck(self._lib.kdf_hit_coverage(self._h, _vp(bits), int(n_bases), _vp(offs), n_reads, _vp(rs), _vp(cg), len(cg),
                                            _vp(co), _vp(kmer_cov), _vp(read_cov), len(kmer_cov)))

    def hit_coverage_dev(self, d_hit_bits: int, n_bases: int, d_offsets: int, n_reads: int, d_ref_start: int, d_cigar: int,
                         n_cigar: int, d_cigar_offsets: int, d_kmer_cov: int, d_read_cov: int, span: int):
        """The same between device buffers: ``d_ref_start`` int64[n_reads], ``d_cigar`` uint32[n_cigar],
        ``d_cigar_offsets`` int64[n_reads + 1], ``d_kmer_cov`` / ``d_read_cov`` uint32[span].  Synchronises the engine's
        stream once; the sums are complete in stream order."""
        p = lambda x: c_void_p(x) if x else None
        self._ck(self._lib.kdf_hit_coverage_dev(self._h, p(d_hit_bits), int(n_bases), p(d_offsets), int(n_reads), p(d_ref_start),
                                                p(d_cigar), int(n_cigar), p(d_cigar_offsets), p(d_kmer_cov), p(d_read_cov),
                                                int(span)))

    def coverage_list(self, kmer_cov: np.ndarray, read_cov: np.ndarray, first: int = 0, n: Optional[int] = None,
                      min_reads: int = 1, cap: Optional[int] = None):
        """-> (positions uint64[m] ascending, kmer uint32[m], reads uint32[m]): the positions g of [first, first + n)
        with ``read_cov[g] >= max(min_reads, 1)`` and the two sums there.  ``cap`` (default: as many as there are)
        bounds the output: more entries than that raise, like hit_list."""
        kc = np.ascontiguousarray(kmer_cov, dtype=np.uint32)
        rc = np.ascontiguousarray(read_cov, dtype=np.uint32)
        n = len(rc) - int(first) if n is None else int(n)
        if first < 0 or n < 0 or int(first) + n > len(rc) or len(kc) != len(rc):
            raise ValueError(f"window [{first}, {first}+{n}) outside accumulators of {len(rc)} / {len(kc)} positions")
        if cap is None:
            cap = int((rc[first:first + n] >= max(int(min_reads), 1)).sum())
        pos, ko, ro = np.zeros(int(cap), np.uint64), np.zeros(int(cap), np.uint32), np.zeros(int(cap), np.uint32)
        m = c_uint64(0)
        self._ck(self._lib.kdf_coverage_list(self._h, _vp(kc), _vp(rc), int(first), n, int(min_reads), _vp(pos), _vp(ko),
                                             _vp(ro), int(cap), byref(m)))
        return pos[:m.value], ko[:m.value], ro[:m.value]

    def _coverage_list_dev(self, d_kmer_cov, d_read_cov, first, n, min_reads, d_pos, d_kmer, d_read, cap):
        m = c_uint64(0)
        p = lambda x: c_void_p(x) if x else None
        rc = self._lib.kdf_coverage_list_dev(self._h, p(d_kmer_cov), p(d_read_cov), int(first), int(n), int(min_reads),
                                             p(d_pos), p(d_kmer), p(d_read), int(cap), byref(m))
        return rc, m.value

    def coverage_list_dev(self, d_kmer_cov: Optional[int], d_read_cov: int, first: int, n: int, min_reads: int, d_pos: int,
                          d_kmer: Optional[int], d_read: Optional[int], cap: int) -> int:
        """The same between device buffers (``d_pos`` uint64[cap], ``d_kmer`` / ``d_read`` uint32[cap] or None);
        returns the number of entries and raises when it exceeds ``cap`` (at most ``cap`` are written).  Synchronises."""
        rc, m = self._coverage_list_dev(d_kmer_cov, d_read_cov, first, n, min_reads, d_pos, d_kmer, d_read, cap)
        self._ck(rc)
        return m

    def hit_keys(self, stream: ReadStream, positions: np.ndarray) -> np.ndarray:
        """uint64 (n, key_words): the canonical key of window [p, p + k) of the stream for every listed position, word
        0 least significant (k <= 32: column 0 is ``lo``; 33..63: ``lo``, ``hi``).  A window that ends past the stream
        gets a row of all-ones words.  Positions come from a hit list: whether a window is valid is not checked."""
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        keys = np.zeros((len(pos), self.key_words), np.uint64)
        self._ck(self._lib.kdf_hit_keys(self._h, _vp(stream.packed), int(stream.n_bases), _vp(pos), len(pos), _vp(keys)))
        return keys

    def hit_keys_dev(self, d_packed: int, n_bases: int, d_positions: int, n: int, d_keys: int):
        """The same between device buffers: ``d_positions`` uint64[n], ``d_keys`` uint64[n x key_words].  Stream order
        on the engine's stream; does not synchronise."""
        self._ck(self._lib.kdf_hit_keys_dev(self._h, c_void_p(d_packed) if d_packed else None, int(n_bases),
                                            c_void_p(d_positions) if d_positions else None, int(n),
                                            c_void_p(d_keys) if d_keys else None))

    # -- VCF mode on the device ------------------------------------------------
    def variant_windows(self, stream: ReadStream, ref_start: np.ndarray, cigar: np.ndarray, cigar_offsets: np.ndarray,
                        var_pos: np.ndarray, var_span: np.ndarray, var_ref_len: np.ndarray, alt: bytes,
                        alt_offsets: np.ndarray, qual: Optional[np.ndarray] = None, qual_offsets: Optional[np.ndarray] = None,
                        min_baseq: int = 0, pair_cap: Optional[int] = None, entry_cap: Optional[int] = None,
                        n_bases: Optional[int] = None):
        """Which windows of which reads span which variant (``include/kdf.h``, "VCF mode on the device").  ``ref_start``
        int64[n_reads] (< 0: the read is skipped), ``cigar`` / ``cigar_offsets`` as for :meth:`hit_coverage`; the
        variants ascend by ``var_pos`` int64, with ``var_span`` / ``var_ref_len`` uint32 and their ALT bytes
        ``alt[alt_offsets[v]:alt_offsets[v + 1]]``; ``qual`` uint8 with ``qual_offsets`` int64[n_reads + 1] and
        ``min_baseq`` switch the quality rule on.  -> (pair_read int64[p], pair_var uint32[p], pair_flags uint8[p],
        entry_pos uint64[e], entry_pair uint64[e]): pairs ascending by (read, variant), entries by (pair, position).
        Without caps the call sizes itself first; with caps, more pairs or entries than that raise.  ``n_bases``
        (default: the stream's) takes a prefix of the stream."""
        n = int(stream.n_bases if n_bases is None else n_bases)
        offs = np.ascontiguousarray(stream.offsets, dtype=np.int64)
        rs = np.ascontiguousarray(ref_start, dtype=np.int64)
        cg = np.ascontiguousarray(cigar, dtype=np.uint32)
        co = np.ascontiguousarray(cigar_offsets, dtype=np.int64)
        vp = np.ascontiguousarray(var_pos, dtype=np.int64)
        vs = np.ascontiguousarray(var_span, dtype=np.uint32)
        vr = np.ascontiguousarray(var_ref_len, dtype=np.uint32)
        al = np.frombuffer(bytes(alt), dtype=np.uint8)
        ao = np.ascontiguousarray(alt_offsets, dtype=np.int64)
        ql = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
        qo = None if qual is None else np.ascontiguousarray(qual_offsets, dtype=np.int64)
        n_reads, n_var = len(offs) - 1, len(vp)
        if n_reads > 0 and (len(rs) != n_reads or len(co) != n_reads + 1 or (qo is not None and len(qo) != n_reads + 1)):
            raise ValueError(f"{n_reads} reads, {len(rs)} ref_start, {len(co)} cigar_offsets entries")
        if len(vs) != n_var or len(vr) != n_var or len(ao) != n_var + 1:
            raise ValueError(f"{n_var} variants, {len(vs)} var_span, {len(vr)} var_ref_len, {len(ao)} alt_offsets entries")

        def call(pc, ec):
            out = (np.zeros(pc, np.int64), np.zeros(pc, np.uint32), np.zeros(pc, np.uint8), np.zeros(ec, np.uint64), np.zeros(ec, np.uint64))
            npairs, nent = c_uint64(0), c_uint64(0)
            o = [_vp(x) if len(x) else None for x in out]
            rc = self._lib.kdf_variant_windows(self._h, _vp(stream.packed), _vp(stream.invalid), n, _vp(offs), n_reads, _vp(rs), _vp(cg), len(cg),
                                               _vp(co), _vp(ql), 0 if ql is None else len(ql), _vp(qo), int(min_baseq), _vp(vp), _vp(vs), _vp(vr),
                                               n_var, _vp(al) if len(al) else None, len(al), _vp(ao), o[0], o[1], o[2], pc, o[3], o[4], ec,
                                               byref(npairs), byref(nent))
            return rc, npairs.value, nent.value, out
        if pair_cap is None or entry_cap is None:
            rc, pc, ec, _ = call(0, 0)
            self._ck(rc)
            pair_cap = pc if pair_cap is None else pair_cap
            entry_cap = ec if entry_cap is None else entry_cap
        rc, pc, ec, out = call(int(pair_cap), int(entry_cap))
        self._ck(rc)
        return out[0][:pc], out[1][:pc], out[2][:pc], out[3][:ec], out[4][:ec]

    def variant_windows_dev(self, d_packed: int, d_invalid: int, n_bases: int, d_offsets: int, n_reads: int, d_ref_start: int,
                            d_cigar: int, n_cigar: int, d_cigar_offsets: int, d_qual: Optional[int], n_qual: int,
                            d_qual_offsets: Optional[int], min_baseq: int, d_var_pos: int, d_var_span: int, d_var_ref_len: int,
                            n_var: int, d_alt: Optional[int], n_alt: int, d_alt_offsets: int, d_pair_read: Optional[int],
                            d_pair_var: Optional[int], d_pair_flags: Optional[int], pair_cap: int, d_entry_pos: Optional[int],
                            d_entry_pair: Optional[int], entry_cap: int, check: bool = True):
        """The same between device buffers: ``d_pair_read`` int64[pair_cap], ``d_pair_var`` uint32[pair_cap],
        ``d_pair_flags`` uint8[pair_cap], ``d_entry_pos`` / ``d_entry_pair`` uint64[entry_cap].  -> (n_pairs,
        n_entries); with both caps 0 and no output buffers it is a sizing call.  More pairs or entries than the caps
        raise (``check=False``: the counts are returned instead, at most the caps were written).  Synchronises the
        engine's stream twice."""
        p = lambda x: c_void_p(x) if x else None
        npairs, nent = c_uint64(0), c_uint64(0)
        rc = self._lib.kdf_variant_windows_dev(self._h, p(d_packed), p(d_invalid), int(n_bases), p(d_offsets), int(n_reads), p(d_ref_start),
                                               p(d_cigar), int(n_cigar), p(d_cigar_offsets), p(d_qual), int(n_qual), p(d_qual_offsets),
                                               int(min_baseq), p(d_var_pos), p(d_var_span), p(d_var_ref_len), int(n_var), p(d_alt), int(n_alt),
                                               p(d_alt_offsets), p(d_pair_read), p(d_pair_var), p(d_pair_flags), int(pair_cap), p(d_entry_pos),
                                               p(d_entry_pair), int(entry_cap), byref(npairs), byref(nent))
        if check or not (npairs.value > pair_cap or nent.value > entry_cap):
            self._ck(rc)
        return npairs.value, nent.value

    def variant_evidence(self, keys: np.ndarray, entry_pair: np.ndarray, pair_var: np.ndarray, pair_flags: np.ndarray, n_var: int):
        """Per-pair and per-variant evidence of listed windows against the table (``include/kdf.h``): ``keys`` uint64
        (n_entries, key_words) as :meth:`hit_keys` returns them, ``entry_pair`` uint64[n_entries], ``pair_var``
        uint32[n_pairs], ``pair_flags`` uint8[n_pairs].  -> (pair_rows uint32 (n_pairs, 2): windows, absent; var_rows
        uint64 (n_var, 8): n, sum, min, max and the same over the alt-supporting pairs, of the distinct stored keys
        with count > 0)."""
        ks = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, self.key_words)
        ep = np.ascontiguousarray(entry_pair, dtype=np.uint64)
        pv = np.ascontiguousarray(pair_var, dtype=np.uint32)
        pf = np.ascontiguousarray(pair_flags, dtype=np.uint8)
        if len(ks) != len(ep) or len(pv) != len(pf):
            raise ValueError(f"{len(ks)} key rows for {len(ep)} entries, {len(pv)} pair_var for {len(pf)} pair_flags")
        pair_rows = np.zeros((len(pv), 2), np.uint32)
        var_rows = np.zeros((int(n_var), 8), np.uint64)
        v = lambda a: _vp(a) if a.size else None
        self._ck(self._lib.kdf_variant_evidence(self._h, v(ks), v(ep), len(ep), v(pv), v(pf), len(pv), int(n_var), v(pair_rows), v(var_rows)))
        return pair_rows, var_rows

    def variant_evidence_dev(self, d_keys: int, d_entry_pair: int, n_entries: int, d_pair_var: int, d_pair_flags: int, n_pairs: int,
                             n_var: int, d_pair_rows: int, d_var_rows: int):
        """The same between device buffers: ``d_pair_rows`` uint32[n_pairs x 2], ``d_var_rows`` uint64[n_var x 8], both
        written in full.  Stream order on the engine's stream; does not synchronise."""
        p = lambda x: c_void_p(x) if x else None
        self._ck(self._lib.kdf_variant_evidence_dev(self._h, p(d_keys), p(d_entry_pair), int(n_entries), p(d_pair_var), p(d_pair_flags),
                                                    int(n_pairs), int(n_var), p(d_pair_rows), p(d_var_rows)))

    # -- regions of informative reads ------------------------------------------
    def _cluster_intervals(self, chrom, start, end, n, merge_distance, region_of, regions, cap):
        m = c_uint64(0)
        rc = self._lib.kdf_cluster_intervals(self._h, _vp(chrom), _vp(start), _vp(end), int(n), int(merge_distance),
                                             _vp(region_of), _vp(regions), int(cap), byref(m))
        return rc, m.value

    def cluster_intervals(self, chrom: np.ndarray, start: np.ndarray, end: np.ndarray, merge_distance: int):
        """Cluster intervals into regions (``include/kdf.h``, "regions of informative reads"): ``chrom`` (a rank the
        caller defines, < 0: the interval is skipped), ``start``, ``end`` int64[n] in any order.  An interval opens a
        region iff it is the first of its chrom in (chrom, start) order or starts more than ``merge_distance`` past the
        largest end of the earlier intervals of its chrom.  -> (region_of int64[n], -1 for skipped intervals; regions
        int64 (m, 4), columns ``REGION_COLUMNS``), regions numbered in (chrom, start) order."""
        c = np.ascontiguousarray(chrom, dtype=np.int64)
        s = np.ascontiguousarray(start, dtype=np.int64)
        e = np.ascontiguousarray(end, dtype=np.int64)
        if not (c.ndim == s.ndim == e.ndim == 1 and len(c) == len(s) == len(e)):
            raise ValueError(f"chrom, start and end must be 1-D arrays of one length, not {c.shape}, {s.shape}, {e.shape}")
        region_of = np.full(len(c), -1, np.int64)
        rc, m = self._cluster_intervals(c, s, e, len(c), merge_distance, region_of, None, 0)      # the sizing call
        if m == 0:
            self._ck(rc)
            return region_of, np.zeros((0, len(REGION_COLUMNS)), np.int64)
        regions = np.zeros((m, len(REGION_COLUMNS)), np.int64)
        rc, m = self._cluster_intervals(c, s, e, len(c), merge_distance, region_of, regions, m)
        self._ck(rc)
        return region_of, regions

    def _cluster_intervals_dev(self, d_chrom, d_start, d_end, n, merge_distance, d_region_of, d_regions, cap):
        m = c_uint64(0)
        p = lambda x: c_void_p(x) if x else None
        rc = self._lib.kdf_cluster_intervals_dev(self._h, p(d_chrom), p(d_start), p(d_end), int(n), int(merge_distance),
                                                 p(d_region_of), p(d_regions), int(cap), byref(m))
        return rc, m.value

    def cluster_intervals_dev(self, d_chrom: int, d_start: int, d_end: int, n: int, merge_distance: int, d_region_of: int,
                              d_regions: Optional[int], cap: int) -> int:
        """The same between device buffers (``d_chrom`` / ``d_start`` / ``d_end`` / ``d_region_of`` int64[n],
        ``d_regions`` int64[cap x 4] or None with ``cap`` 0 for a sizing call); returns the number of regions and raises
        when it exceeds ``cap`` (``d_region_of`` is complete then, at most ``cap`` rows are written).  Synchronises."""
        rc, m = self._cluster_intervals_dev(d_chrom, d_start, d_end, n, merge_distance, d_region_of, d_regions, cap)
        self._ck(rc)
        return m

    def group_distinct(self, group: np.ndarray, keys: np.ndarray, n_groups: int) -> np.ndarray:
        """uint64[n_groups]: the number of distinct rows of ``keys`` (uint64 (n, words), words 1..8, or 1-D for one
        word; rows as :meth:`hit_keys` returns them) among the entries with ``group[e] == g``.  Entries with a group
        outside [0, n_groups) and rows of all-ones words are ignored; the same row in two groups counts in both.  Exact."""
        g = np.ascontiguousarray(group, dtype=np.int64)
        ks = np.ascontiguousarray(keys, dtype=np.uint64)
        if ks.ndim == 1:
            ks = ks.reshape(-1, 1)
        if g.ndim != 1 or ks.ndim != 2 or len(ks) != len(g):
            raise ValueError(f"{g.shape} groups for key rows of shape {ks.shape}")
        counts = np.zeros(max(int(n_groups), 0), np.uint64)
        v = lambda a: _vp(a) if a.size else None
        self._ck(self._lib.kdf_group_distinct(self._h, v(g), v(ks), int(ks.shape[1]), len(g), int(n_groups), v(counts)))
        return counts

    def group_distinct_dev(self, d_group: int, d_keys: int, words: int, n: int, n_groups: int, d_counts: int):
        """The same between device buffers: ``d_group`` int64[n], ``d_keys`` uint64[n x words], ``d_counts``
        uint64[n_groups], overwritten.  Synchronises the engine's stream (the sort); the counts are complete in stream
        order."""
        p = lambda x: c_void_p(x) if x else None
        self._ck(self._lib.kdf_group_distinct_dev(self._h, p(d_group), p(d_keys), int(words), int(n), int(n_groups), p(d_counts)))

    # -- k-mer FASTA codec -----------------------------------------------------
    @staticmethod
    def kmer_text_bytes(k: int, layout: int = TEXT_FASTA, first_index: int = 0, n: int = 0) -> int:
        """Bytes of the text of ``n`` keys (``include/kdf.h``, "k-mer FASTA codec"): ``TEXT_FASTA`` records
        ``>{first_index + e}\\n{KMER}\\n`` or ``TEXT_ROWS`` k bases per key.  A pure host function of libkdf: no engine,
        no GPU.  0 for a k or layout the codec does not take and when the indices or the size pass 2^63."""
        return int(_native.load().kdf_kmer_text_bytes(int(k), int(layout), int(first_index), int(n)))

    def format_kmers(self, lo: np.ndarray, hi: Optional[np.ndarray], k: int, layout: int = TEXT_FASTA, first_index: int = 0,
                     byte_first: int = 0, byte_count: Optional[int] = None) -> np.ndarray:
        """uint8[byte_count]: bytes ``byte_first .. byte_first + byte_count`` (default: to the end) of the text of the
        keys, whose form follows ``k`` and not the engine's k: ``lo`` uint64[n] (k <= 32), ``lo`` and ``hi`` (k 33..63),
        (n, W) rows in ``lo`` and ``hi`` None (odd k 65..201).  ``byte_first`` must be a multiple of 16."""
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        hi = None if hi is None or not 33 <= int(k) <= 63 else np.ascontiguousarray(hi, dtype=np.uint64)
        n = len(lo)
        if byte_count is None:
            byte_count = max(self.kmer_text_bytes(k, layout, first_index, n) - int(byte_first), 0)
        out = np.empty(int(byte_count), np.uint8)
        v = lambda a: _vp(a) if a is not None and a.size else None
        self._ck(self._lib.kdf_format_kmers(self._h, v(lo), v(hi), n, int(k), int(layout), int(first_index), int(byte_first),
                                            int(byte_count), v(out)))
        return out

    def format_kmers_dev(self, d_lo: int, d_hi: Optional[int], n: int, k: int, layout: int, first_index: int, byte_first: int,
                         byte_count: int, d_text: int):
        """The same between device buffers (raw pointers): ``d_text`` takes ``byte_count`` bytes and nothing else.  Stream
        order on the engine's stream; does not synchronise."""
        p = lambda x: c_void_p(x) if x else None
        self._ck(self._lib.kdf_format_kmers_dev(self._h, p(d_lo), p(d_hi), int(n), int(k), int(layout), int(first_index),
                                                int(byte_first), int(byte_count), p(d_text)))

    def _parse_result(self, rc, n, consumed, bad):
        """(n keys, consumed bytes) of a parse call, or its error: a bad line raises ``KmerFastaError`` (a ValueError)."""
        if rc == _native.KDF_ERR_IO:
            msg = self._lib.kdf_last_error(self._h)
            raise KmerFastaError(msg.decode(errors="replace") if msg else "bad line", bad.value)
        self._ck(rc)
        return n.value, consumed.value

    def parse_kmer_fasta(self, text, k: int, canonical: bool = True, final_chunk: bool = True):
        """Sequence lines of a chunk of k-mer FASTA text (bytes or uint8 array) -> ``(lo, hi, consumed)``: the keys in
        file order in the form of ``k`` (hi None unless k is 33..63; long k: (n, W) rows) and the bytes consumed -- all of
        them with ``final_chunk``, else up to the last ``\\n``.  Lines: ``include/kdf.h``, "k-mer FASTA codec"; a bad
        line raises ``KmerFastaError`` with its offset."""
        t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
        W = key_words(k)
        if W == 0:
            raise ValueError(f"k={k} outside 1..{self.MAX_K} and odd {self.LONG_MIN_K}..{self.LONG_MAX_K}")
        n, consumed, bad = c_uint64(0), c_uint64(0), c_uint64(0)
        args = (self._h, _vp(t) if t.size else None, t.size, int(k), int(bool(canonical)), int(bool(final_chunk)))
        rc = self._lib.kdf_parse_kmer_fasta(*args, None, None, 0, byref(n), byref(consumed), byref(bad))       # the sizing call
        if rc == _native.KDF_ERR_INVALID and n.value > 0:
            rc = _native.KDF_OK
        m = self._parse_result(rc, n, consumed, bad)[0]
        lo = np.zeros((m, W) if W > 2 else m, np.uint64)
        hi = np.zeros(m, np.uint64) if W == 2 else None
        if m:
            rc = self._lib.kdf_parse_kmer_fasta(*args, _vp(lo), _vp(hi), m, byref(n), byref(consumed), byref(bad))
            self._parse_result(rc, n, consumed, bad)
        return lo, hi, consumed.value

    def parse_kmer_fasta_dev(self, d_text: int, n_bytes: int, k: int, canonical: bool, final_chunk: bool, d_lo: Optional[int],
                             d_hi: Optional[int], cap: int) -> Tuple[int, int]:
        """The same between device buffers: ``d_lo`` / ``d_hi`` hold ``cap`` rows (None with ``cap`` 0: a sizing call).
        -> (number of keys, bytes consumed); raises when the keys exceed ``cap`` (the first ``cap`` are written).
        Synchronises the engine's stream."""
        p = lambda x: c_void_p(x) if x else None
        n, consumed, bad = c_uint64(0), c_uint64(0), c_uint64(0)
        rc = self._lib.kdf_parse_kmer_fasta_dev(self._h, p(d_text), int(n_bytes), int(k), int(bool(canonical)), int(bool(final_chunk)),
                                                p(d_lo), p(d_hi), int(cap), byref(n), byref(consumed), byref(bad))
        if rc == _native.KDF_ERR_INVALID and cap == 0 and n.value > 0:      # a sizing call's answer
            rc = _native.KDF_OK
        return self._parse_result(rc, n, consumed, bad)

    # -- index record codec ---------------------------------------------------
    @staticmethod
    def index_record_bytes(k: int, counter_len: int = 4) -> int:
        """Bytes of one index record (``include/kdf.h``, "index record codec"): ceil(2k / 8) key bytes and
        ``counter_len`` count bytes.  A pure host function of libkdf: no engine, no GPU.  0 for a k the codec does not
        take or a ``counter_len`` outside 1..16."""
        return int(_native.load().kdf_index_record_bytes(int(k), int(counter_len)))

    def _index_key_form(self, lo, hi, k):
        """(lo, hi, n) as contiguous uint64 arrays in the form of ``k`` (hi None unless k is 33..63; long k: (n, W) rows)."""
        W = key_words(k)
        if W == 0:
            raise ValueError(f"k={k} outside 1..{self.MAX_K} and odd {self.LONG_MIN_K}..{self.LONG_MAX_K}")
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        if W > 2:
            lo = lo.reshape(-1, W)
        if W == 2:
            hi = np.zeros(len(lo), np.uint64) if hi is None else np.ascontiguousarray(hi, dtype=np.uint64)
            if len(hi) != len(lo):
                raise ValueError(f"{len(hi)} hi words for {len(lo)} lo words")
        else:
            hi = None
        return lo, hi, len(lo)

    def index_encode(self, lo: np.ndarray, hi: Optional[np.ndarray], counts: Optional[np.ndarray], k: int, perm: Optional[np.ndarray] = None,
                     byte_first: int = 0, byte_count: Optional[int] = None) -> np.ndarray:
        """uint8[byte_count]: bytes ``byte_first .. byte_first + byte_count`` (default: to the end) of the record body
        of an index of the keys -- record e = the key bytes of key ``perm[e]`` (``perm`` None: e), little-endian, and the
        4 little-endian bytes of its count (``counts`` None: 0).  The key form follows ``k``, not the engine's k: ``lo``
        uint64[n] (k <= 32), ``lo`` and ``hi`` (k 33..63), (n, W) rows in ``lo`` and ``hi`` None (odd k 65..201).
        ``byte_first`` must be a multiple of 16."""
        lo, hi, n = self._index_key_form(lo, hi, k)
        counts = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32)
        perm = None if perm is None else np.ascontiguousarray(perm, dtype=np.uint32)
        for name, a in (("counts", counts), ("perm", perm)):
            if a is not None and len(a) != n:
                raise ValueError(f"{len(a)} {name} for {n} keys")
        if byte_count is None:
            byte_count = max(n * self.index_record_bytes(k) - int(byte_first), 0)
        out = np.empty(int(byte_count), np.uint8)
        v = lambda a: _vp(a) if a is not None and a.size else None
        self._ck(self._lib.kdf_index_encode(self._h, _native.KDF_MEM_HOST, v(lo), v(hi), v(counts), v(perm), n, int(k), int(byte_first),
                                            int(byte_count), v(out)))
        return out

    def index_encode_dev(self, d_lo: int, d_hi: Optional[int], d_counts: Optional[int], d_perm: Optional[int], n: int, k: int,
                         byte_first: int, byte_count: int, d_bytes: int):
        """The same between device buffers (raw pointers; ``d_counts`` uint32[n], ``d_perm`` uint32[n] or None):
        ``d_bytes`` takes ``byte_count`` bytes at any alignment and nothing else.  Stream order on the engine's stream;
        does not synchronise."""
        p = lambda x: c_void_p(x) if x else None
        self._ck(self._lib.kdf_index_encode(self._h, _native.KDF_MEM_DEVICE, p(d_lo), p(d_hi), p(d_counts), p(d_perm), int(n), int(k),
                                            int(byte_first), int(byte_count), p(d_bytes)))

    def _index_decoded(self, rc, bad):
        """Nothing, or the error of a decode call: a record whose key has a bit at or above 2k raises ``IndexRecordError``."""
        if rc == _native.KDF_ERR_IO:
            msg = self._lib.kdf_last_error(self._h)
            raise IndexRecordError(msg.decode(errors="replace") if msg else "bad record", bad.value)
        self._ck(rc)

    def index_decode(self, data, k: int, counter_len: int = 4):
        """Record bytes (bytes or a uint8 array of whole records of ceil(2k / 8) + ``counter_len`` bytes) ->
        ``(lo, hi, counts)``: the keys in the form of ``k`` (hi None unless k is 33..63; long k: (n, W) rows) and the
        counts as uint32, saturated at 2^32 - 1 (the rule of ``jf_io._decode``).  A key with a bit at or above 2k raises
        ``IndexRecordError`` with the index of the first such record."""
        t = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        rd = self.index_record_bytes(k, counter_len)
        if rd == 0:
            raise ValueError(f"k={k} or counter_len={counter_len}: no index record of that shape")
        if t.size % rd:
            raise ValueError(f"{t.size} bytes are no whole records of {rd} bytes")
        n, W = t.size // rd, key_words(k)
        lo = np.zeros((n, W) if W > 2 else n, np.uint64)
        hi = np.zeros(n, np.uint64) if W == 2 else None
        counts = np.zeros(n, np.uint32)
        bad = c_uint64(0)
        v = lambda a: _vp(a) if a is not None and a.size else None
        rc = self._lib.kdf_index_decode(self._h, _native.KDF_MEM_HOST, v(t), n, int(k), int(counter_len), v(lo), v(hi), v(counts), byref(bad))
        self._index_decoded(rc, bad)
        return lo, hi, counts

    def index_decode_dev(self, d_bytes: int, n: int, k: int, counter_len: int, d_lo: int, d_hi: Optional[int], d_counts: Optional[int]):
        """The same between device buffers: ``d_bytes`` holds ``n`` records at any alignment, ``d_lo`` / ``d_hi`` /
        ``d_counts`` (uint32) take ``n`` rows (``d_hi`` may be None for k <= 32, ``d_counts`` may be None).  Synchronises
        the engine's stream; a bad record raises ``IndexRecordError`` after the rows were written as read."""
        p = lambda x: c_void_p(x) if x else None
        bad = c_uint64(0)
        rc = self._lib.kdf_index_decode(self._h, _native.KDF_MEM_DEVICE, p(d_bytes), int(n), int(k), int(counter_len), p(d_lo), p(d_hi),
                                        p(d_counts), byref(bad))
        self._index_decoded(rc, bad)

    @staticmethod
    def _jf_columns(columns, k):
        cols = np.ascontiguousarray([int(c) for c in columns], dtype=np.uint64)
        if len(cols) != 2 * int(k):
            raise ValueError(f"{len(cols)} matrix columns for key_len {2 * int(k)}")
        return cols

    def jf_positions(self, lo: np.ndarray, hi: Optional[np.ndarray], k: int, columns, size: int) -> np.ndarray:
        """uint64[n]: the hash position of every key under a Jellyfish header's ``matrix1.columns`` and ``size`` (a
        power of two): ``jf_io.jf_positions(columns, 2k, lo, hi) & (size - 1)``.  k <= 63."""
        lo, hi, n = self._index_key_form(lo, hi, k)
        cols = self._jf_columns(columns, k)
        pos = np.zeros(n, np.uint64)
        v = lambda a: _vp(a) if a is not None and a.size else None
        self._ck(self._lib.kdf_jf_positions(self._h, _native.KDF_MEM_HOST, v(lo), v(hi), n, int(k), cols.ctypes.data_as(POINTER(c_uint64)),
                                            int(size), v(pos)))
        return pos

    def jf_positions_dev(self, d_lo: int, d_hi: Optional[int], n: int, k: int, columns, size: int, d_pos: int):
        """The same between device buffers: ``d_pos`` takes ``n`` uint64 positions; ``columns`` stays a host sequence
        (it travels as kernel data).  Stream order on the engine's stream; does not synchronise."""
        p = lambda x: c_void_p(x) if x else None
        cols = self._jf_columns(columns, k)
        self._ck(self._lib.kdf_jf_positions(self._h, _native.KDF_MEM_DEVICE, p(d_lo), p(d_hi), int(n), int(k),
                                            cols.ctypes.data_as(POINTER(c_uint64)), int(size), p(d_pos)))

    def jf_order_dev(self, d_lo: int, d_hi: Optional[int], n: int, k: int, columns, size: int, d_perm: int):
        """The record order of a Jellyfish ``binary/sorted`` file: ``d_perm`` (uint32[n]) takes the permutation that
        puts the keys in ascending (hash position, key) order.  n < 2^32, k <= 63.  Synchronises the engine's stream."""
        p = lambda x: c_void_p(x) if x else None
        cols = self._jf_columns(columns, k)
        self._ck(self._lib.kdf_jf_order(self._h, _native.KDF_MEM_DEVICE, p(d_lo), p(d_hi), int(n), int(k),
                                        cols.ctypes.data_as(POINTER(c_uint64)), int(size), p(d_perm)))

    # -- count profile of a stream -------------------------------------------
    def window_counts(self, stream: ReadStream, want_valid: bool = False):
        """`jellyfish query -s reads.fa` over a whole stream: uint32[n_bases], the stored count of the canonical k-mer
        of every window start (0: absent, stored with count 0, or not a valid window).  ``want_valid``: -> (counts,
        valid_bits uint64[mask words]) with bit i set iff window i is valid.  Per read: slice with ``stream.offsets``."""
        counts = np.zeros(stream.n_bases, np.uint32)
        valid = np.zeros(stream_words(stream.n_bases)[1], np.uint64) if want_valid else None
        self._ck(self._lib.kdf_window_counts(self._h, _vp(stream.packed), _vp(stream.invalid), stream.n_bases,
                                             _vp(counts), _vp(valid)))
        return (counts, valid) if want_valid else counts

    def window_counts_dev(self, d_packed: int, d_invalid: int, n_bases: int, d_counts: int, d_valid: Optional[int] = None):
        """The same between device buffers (raw pointers): n_bases uint32 counts, and ceil(n_bases / 64) valid words
        when ``d_valid`` is given.  Stream order on the engine's stream; does not synchronise."""
        self._ck(self._lib.kdf_window_counts_dev(self._h, c_void_p(d_packed), c_void_p(d_invalid), int(n_bases),
                                                 c_void_p(d_counts), c_void_p(d_valid) if d_valid else None))

    def read_depth(self, stream: ReadStream, low_max: int = 0) -> np.ndarray:
        """Per-read summary of the window counts: uint64 (n_reads, 6), columns ``READ_DEPTH_COLUMNS`` -- valid
        windows, of those with count > 0, of those with count <= ``low_max`` (absent keys included), min, max and sum
        of the counts over the valid windows (absent = 0; min = max = 0 for a read without windows)."""
        if not 0 <= int(low_max) <= 0xFFFFFFFF:
            raise ValueError(f"low_max={low_max} outside 0..2^32 - 1")
        rows = np.zeros((stream.n_reads, len(READ_DEPTH_COLUMNS)), np.uint64)
        offs = np.ascontiguousarray(stream.offsets, dtype=np.int64)
        self._ck(self._lib.kdf_read_depth(self._h, _vp(stream.packed), _vp(stream.invalid), stream.n_bases, _vp(offs),
                                          stream.n_reads, int(low_max), _vp(rows)))
        return rows

    def read_depth_dev(self, d_packed: int, d_invalid: int, n_bases: int, d_offsets: int, n_reads: int, low_max: int,
                       d_rows: int):
        """The same between device buffers: ``d_offsets`` int64[n_reads + 1], ``d_rows`` uint64[n_reads x 6]."""
        self._ck(self._lib.kdf_read_depth_dev(self._h, c_void_p(d_packed), c_void_p(d_invalid), int(n_bases),
                                              c_void_p(d_offsets), int(n_reads), int(low_max), c_void_p(d_rows)))


# columns of KmerEngine.read_depth's rows
READ_DEPTH_COLUMNS = ("windows", "present", "low", "min", "max", "sum")
# columns of KmerEngine.read_hits' rows
READ_HITS_COLUMNS = ("hits", "distinct")
# columns of KmerEngine.cluster_intervals' regions
REGION_COLUMNS = ("chrom", "start", "end", "members")


def estimate_from_registers(regs) -> float:
    """The sketch's estimate from exported registers (uint8[2^p], p = 10..18) -- a pure host function of libkdf: no
    engine, no GPU."""
    import ctypes
    regs = np.ascontiguousarray(regs, dtype=np.uint8)
    m = len(regs)
    if regs.ndim != 1 or m < 2 or m & (m - 1):
        raise ValueError(f"estimate_from_registers: {regs.shape} is not 2^p registers")
    v = ctypes.c_double(0.0)
    _native.check(_native.load().kdf_sketch_estimate_registers(_vp(regs), m.bit_length() - 1, byref(v)), None)
    return v.value


def bin_sieve_geometry(n_keys: int, key_words: int, sieve_bits: int = 0, sieve_bins: int = 1) -> Tuple[int, int, int]:
    """(c1, slice_words, bits_per_key) of the bin-major sieve (option ``sieve_bins``) for a filter of ``n_keys`` keys of
    ``key_words`` (1: k <= 32, 2: k <= 63) words -- the engine's own sizing rule, a pure host function of libkdf: no
    engine, no GPU.  Raises KdfError (KDF_ERR_INVALID) when the rule gives this filter no bin-major sieve."""
    from ctypes import c_uint32
    c1, sw, bpk = c_uint32(0), c_uint32(0), c_uint32(0)
    rc = _native.load().kdf_bin_sieve_geometry(int(n_keys), int(key_words), int(sieve_bits), int(sieve_bins), byref(c1), byref(sw), byref(bpk))
    if rc != _native.KDF_OK:
        raise _native.KdfError(rc, f"no bin-major sieve for {n_keys} keys of {key_words} words (sieve_bits {sieve_bits}, sieve_bins {sieve_bins})")
    return c1.value, sw.value, bpk.value


def mirror_engine(k: int, *args, **kwargs) -> KmerEngine:
    """The engine the reference-interface mirrors (discovery chain, Module 3, the Jellyfish wrappers) count with.
    Long k-mers (odd 65..201) run in one process by default: under a process group of several ranks the mirrors shard
    through the multi-GPU exchange, and the (lo, hi) exchange takes k <= 63 only -- refused here, before any device
    call.  ``KDF_LONG_RANKS=1`` opts in to the owner exchange for W-word keys (distributed.owner_of_w,
    kdf_export_parts_w_packed_dev, kdf_set_counts_w_dev): the mirrors then shard long k as they shard k <= 63.  That
    path has run as several ranks on one GPU over gloo only; RCCL and real scaling are unmeasured."""
    if int(k) > KmerEngine.MAX_K:
        import os
        from . import dist_env
        world = dist_env.world_rank()[0]
        if world > 1 and os.environ.get("KDF_LONG_RANKS") != "1":
            raise ValueError(f"k={k}: long k-mers (odd {KmerEngine.LONG_MIN_K}..{KmerEngine.LONG_MAX_K}) run in one "
                             f"process; the multi-GPU mirrors ({world} ranks) take k <= {KmerEngine.MAX_K}")
    return KmerEngine(k, *args, **kwargs)


def hit_positions(hit_bits: np.ndarray, start: int, end: int) -> np.ndarray:
    """Window-start offsets (relative to ``start``) whose hit bit is set in [start, end)."""
    w0, w1 = start >> 6, (end + 63) >> 6
    bits = np.unpackbits(hit_bits[w0:w1].view(np.uint8), bitorder="little")
    lo = start - (w0 << 6)
    return np.nonzero(bits[lo:lo + (end - start)])[0]
