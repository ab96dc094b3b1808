"""Read streams: the 2-bit-packed base stream + invalid mask the engine consumes,
and the host feeders that produce them (ASCII reads, BAM, FASTA).

Replaces the ``samtools fasta -F 0xD00 | ...`` half of the reference's pipes
(core/jellyfish_wrappers.py:159-165, discovery/pipeline.py:106-112,369-375)
and pysam's read iteration in Module 3 (core/bam_scanner.py:405-414).
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_char_p, c_int32, c_int64, c_uint16, c_uint64, c_void_p, POINTER
from dataclasses import dataclass, field
from typing import Iterator, List, Optional, Sequence

import numpy as np

from . import _native, keys

# samtools fasta -F 0xD00: SECONDARY | DUPLICATE | SUPPLEMENTARY
FLAG_OFF_SAMTOOLS_FASTA = 0xD00
# Module 3 (bam_scanner.py:406-409): SECONDARY | DUPLICATE only
FLAG_OFF_MODULE3 = 0x500


def stream_words(n_bases: int):
    pw, mw = c_uint64(0), c_uint64(0)
    _native.load().kdf_stream_words(int(n_bases), byref(pw), byref(mw))
    return pw.value, mw.value


def _vp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(c_void_p)


@dataclass
class ReadStream:
    """One batch of reads as a packed stream (layout: include/kdf.h)."""
    packed: np.ndarray            # uint64, stream_words()[0] words (zero padded)
    invalid: np.ndarray           # uint64, stream_words()[1] words (tail = all ones)
    n_bases: int                  # stream positions, separators included
    offsets: np.ndarray           # int64[n_reads+1]: start of each read in the stream
    # per-read metadata (BAM feeders only)
    flags: Optional[np.ndarray] = None
    ref_ids: Optional[np.ndarray] = None
    positions: Optional[np.ndarray] = None
    name_buf: Optional[bytes] = None          # NUL-terminated names, back to back
    name_offsets: Optional[np.ndarray] = None
    ordinals: Optional[np.ndarray] = None     # uint64[n_reads]: record number in the BAM file (write_bam_subset)
    # alignment details (bam_reader(..., want_aux=True))
    cigar: Optional[np.ndarray] = None        # uint32, BAM encoding (len << 4 | op), all records back to back
    cigar_offsets: Optional[np.ndarray] = None  # int64[n_reads + 1]
    sa_buf: Optional[bytes] = None
    sa_offsets: Optional[np.ndarray] = None   # int64[n_reads], -1 = no SA tag
    quals: Optional[np.ndarray] = None        # uint8 base qualities, all records back to back
    qual_offsets: Optional[np.ndarray] = None  # int64[n_reads + 1]
    mapq: Optional[np.ndarray] = None         # uint8[n_reads]

    def qualities(self, i: int):
        """uint8 base qualities of record i, or None when the BAM stores none (0xFF)."""
        q = self.quals[int(self.qual_offsets[i]):int(self.qual_offsets[i + 1])]
        return None if (len(q) and q[0] == 0xFF) else q

    def cigartuples(self, i: int):
        """[(op, length), ...] of record i, as pysam's ``cigartuples``."""
        c = self.cigar[int(self.cigar_offsets[i]):int(self.cigar_offsets[i + 1])]
        return [(int(x) & 0xF, int(x) >> 4) for x in c]

    def sa_tag(self, i: int):
        o = int(self.sa_offsets[i])
        if o < 0:
            return None
        return self.sa_buf[o:self.sa_buf.index(b"\0", o)].decode()

    def name(self, i: int) -> str:
        o = int(self.name_offsets[i])
        return self.name_buf[o:self.name_buf.index(b"\0", o)].decode()

    @property
    def names(self) -> Optional[List[str]]:
        """All read names (decoded on demand: Module 3 only needs the few informative ones)."""
        if self.name_buf is None:
            return None
        return [x.decode() for x in self.name_buf.split(b"\0")[:self.n_reads]]

    @property
    def n_reads(self) -> int:
        return len(self.offsets) - 1

    def read_lengths(self) -> np.ndarray:
        """Bases per read (the separator after each read is not counted)."""
        return np.diff(self.offsets) - 1

    @staticmethod
    def empty() -> "ReadStream":
        pw, mw = stream_words(0)
        return ReadStream(np.zeros(pw, np.uint64), np.full(mw, ~np.uint64(0), np.uint64), 0,
                          np.zeros(1, np.int64))

    @staticmethod
    def from_ascii(buf: np.ndarray, offs: np.ndarray) -> "ReadStream":
        """ASCII records (uint8 buffer + int64 offsets[n+1]) -> stream."""
        lib = _native.load()
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        n_reads = len(offs) - 1
        total = int(offs[-1] - offs[0]) + n_reads if n_reads else 0
        pw, mw = stream_words(total)
        packed = np.zeros(pw, np.uint64)
        invalid = np.full(mw, ~np.uint64(0), np.uint64)
        so = np.zeros(n_reads + 1, np.int64)
        nb = c_uint64(0)
        rc = lib.kdf_pack_reads(_vp(buf), _vp(offs), n_reads, _vp(packed), _vp(invalid), _vp(so), byref(nb))
        _native.check(rc)
        # words the packer did not touch keep their padding defaults
        return ReadStream(packed, invalid, nb.value, so)

    @staticmethod
    def from_strings(reads: Sequence) -> "ReadStream":
        bs = [r if isinstance(r, (bytes, bytearray)) else r.encode() for r in reads]
        offs = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            offs[1:] = np.cumsum([len(b) for b in bs])
        buf = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, np.uint8)
        return ReadStream.from_ascii(buf, offs)


class _Reader:
    """Iterator over ReadStream batches from a native kdf_reader."""

    def __init__(self, handle, max_bases: int, max_reads: int, want_meta: bool, want_aux: bool = False,
                 is_bam: bool = False):
        self._h = handle
        self.max_bases = int(max_bases)
        self.max_reads = int(max_reads)
        self.want_meta = want_meta or want_aux
        self.want_aux = want_aux
        self.is_bam = is_bam
        self._lib = _native.load()
        if want_aux:
            _native.check_reader(self._lib.kdf_reader_want_aux(self._h, 1), self._h)

    def references(self) -> List[str]:
        n = self._lib.kdf_reader_ref_count(self._h)
        return [self._lib.kdf_reader_ref_name(self._h, i).decode() for i in range(max(n, 0))]

    def reference_lengths(self) -> List[int]:
        """Lengths of the header's reference sequences (BAM readers), in ``references()`` order."""
        n = self._lib.kdf_reader_ref_count(self._h)
        return [int(self._lib.kdf_reader_ref_length(self._h, i)) for i in range(max(n, 0))]

    def close(self):
        if self._h:
            self._lib.kdf_reader_close(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _next(self, packed, invalid, so):
        """One batch into the given arrays -> ReadStream (views of them), or None at end of file."""
        n_reads, nb = c_int64(0), c_uint64(0)
        rc = self._lib.kdf_reader_next(self._h, self.max_bases, self.max_reads, _vp(packed), _vp(invalid),
                                       _vp(so), byref(n_reads), byref(nb))
        _native.check_reader(rc, self._h)
        n = n_reads.value
        if n == 0:
            return None
        pw_used, mw_used = stream_words(nb.value)
        return ReadStream(packed[:pw_used], invalid[:mw_used], nb.value, so[:n + 1].copy())

    def next_into(self, packed: np.ndarray, invalid: np.ndarray):
        """Sequence-only batch into caller-owned arrays (e.g. pinned ones, PinnedBatches) of stream_words(max_bases)
        words; no per-record metadata.  None at end of file."""
        if not self._h:
            return None
        pw, mw = stream_words(self.max_bases)
        if len(packed) < pw or len(invalid) < mw:
            raise ValueError("batch arrays are smaller than stream_words(max_bases)")
        so = np.empty(self.max_reads + 1, np.int64)
        st = self._next(packed, invalid, so)
        if st is None:
            self.close()
        return st

    def __iter__(self) -> Iterator[ReadStream]:
        lib = self._lib
        pw, mw = stream_words(self.max_bases)
        while self._h:
            packed = np.empty(pw, np.uint64)           # the native reader initialises both arrays
            invalid = np.empty(mw, np.uint64)
            so = np.empty(self.max_reads + 1, np.int64)
            st = self._next(packed, invalid, so)
            if st is None:
                break
            n = st.n_reads
            if self.want_meta:
                f, r, p = POINTER(c_uint16)(), POINTER(c_int32)(), POINTER(c_int32)()
                nbuf, noff = c_char_p(), POINTER(c_int64)()
                lib.kdf_reader_last_meta(self._h, byref(f), byref(r), byref(p), byref(nbuf), byref(noff))
                st.flags = np.ctypeslib.as_array(f, (n,)).copy()
                st.ref_ids = np.ctypeslib.as_array(r, (n,)).copy()
                st.positions = np.ctypeslib.as_array(p, (n,)).copy()
                offs = np.ctypeslib.as_array(noff, (n,)).copy()
                base = ctypes.cast(nbuf, c_void_p).value
                last = int(offs[-1])
                end = last + len(ctypes.string_at(base + last)) + 1
                st.name_buf = ctypes.string_at(base, end)
                st.name_offsets = offs
                if self.is_bam:
                    od = POINTER(c_uint64)()
                    _native.check_reader(lib.kdf_reader_last_ordinals(self._h, byref(od)), self._h)
                    st.ordinals = np.ctypeslib.as_array(od, (n,)).copy()
            if self.want_aux:
                from ctypes import c_uint32
                cg, cgo = POINTER(c_uint32)(), POINTER(c_int64)()
                sab, sao = c_char_p(), POINTER(c_int64)()
                _native.check_reader(lib.kdf_reader_last_aux(self._h, byref(cg), byref(cgo), byref(sab), byref(sao)),
                                     self._h)
                st.cigar_offsets = np.ctypeslib.as_array(cgo, (n + 1,)).copy()
                ncg = int(st.cigar_offsets[-1])
                st.cigar = np.ctypeslib.as_array(cg, (ncg,)).copy() if ncg else np.zeros(0, np.uint32)
                st.sa_offsets = np.ctypeslib.as_array(sao, (n,)).copy()
                valid = st.sa_offsets[st.sa_offsets >= 0]
                if len(valid):
                    sbase = ctypes.cast(sab, c_void_p).value
                    last = int(valid.max())
                    st.sa_buf = ctypes.string_at(sbase, last + len(ctypes.string_at(sbase + last)) + 1)
                else:
                    st.sa_buf = b""
                from ctypes import c_uint8
                qb, qo, mq = POINTER(c_uint8)(), POINTER(c_int64)(), POINTER(c_uint8)()
                _native.check_reader(lib.kdf_reader_last_quals(self._h, byref(qb), byref(qo), byref(mq)), self._h)
                st.qual_offsets = np.ctypeslib.as_array(qo, (n + 1,)).copy()
                nq = int(st.qual_offsets[-1])
                st.quals = np.ctypeslib.as_array(qb, (nq,)).copy() if nq else np.zeros(0, np.uint8)
                st.mapq = np.ctypeslib.as_array(mq, (n,)).copy()
            yield st
        self.close()


class PinnedBatches:
    """A ring of page-locked host batches (packed + invalid words for ``max_bases`` stream positions each): the H2D copy
    of one is asynchronous, so it can run while the GPU counts the batch before it and the reader fills the next."""

    def __init__(self, n: int, max_bases: int):
        self._lib = _native.load()
        self._ptrs = []
        self.batches = []
        pw, mw = stream_words(max_bases)
        try:
            for _ in range(n):
                arrs = []
                for words in (pw, mw):
                    p = c_void_p()
                    _native.check(self._lib.kdf_host_alloc(words * 8, byref(p)), None)
                    self._ptrs.append(p)
                    arrs.append(np.ctypeslib.as_array(ctypes.cast(p, POINTER(c_uint64)), (words,)))
                self.batches.append(tuple(arrs))
        except Exception:
            self.close()
            raise

    def close(self):
        self.batches = []
        for p in self._ptrs:
            self._lib.kdf_host_free(p)
        self._ptrs = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


_pinned_cache = {}            # (ring, max_bases) -> PinnedBatches, kept for the life of the process: page-locking ~50 MB per
#                               batch costs more than counting it, and the child and both parents stream one after another


def _pinned_ring(ring: int, max_bases: int) -> PinnedBatches:
    key = (ring, max_bases)
    pb = _pinned_cache.get(key)
    if pb is None or not pb.batches:
        for old in list(_pinned_cache.values()):
            old.close()
        _pinned_cache.clear()
        pb = _pinned_cache[key] = PinnedBatches(ring, max_bases)
    return pb


def stream_batches_overlapped(engine, readers, filtered: bool, ring: int = 0, tally: bool = False, spool=None) -> int:
    """Count every batch of ``readers`` (one reader, or several readers of disjoint ranges of one file:
    ``bam_reader(part=, parts=)``) on ``engine`` as a three-stage pipeline: one reader thread PER READER decodes batches
    into pinned buffers (the native reader releases the GIL; inflate, chunking and parsing of the ranges run side by
    side), the copy stream uploads batch i + 1, the engine counts batch i.  Batches arrive in any order: counting does
    not care.  ``tally``: pass 1 of a two-pass count -- every batch goes to the engine's prefilter
    (``prefilter_add_uploaded``) instead of its table.  ``spool``: a ``spool.ReadSpool`` on the engine's device -- every
    batch is also appended to it from its upload slot, before it is counted or tallied, so that later passes replay the
    spool and not the file.  A spool that overflows stops taking batches (it reads ``stat("overflowed")``: the caller
    streams the file again for the later passes); the pass itself goes on.  A spool whose ``keep_reads`` attribute is set
    also gets every batch's read offsets (``ReadSpool.read_hits`` / ``read_depth`` / ``select_reads`` over it afterwards).
    Returns the number of reads."""
    return _stream_batches(engine, readers, filtered, ring, tally, spool, False)


def sketch_batches_overlapped(engine, readers, ring: int = 0, spool=None) -> int:
    """The same pipeline as a SIZING pass: every batch goes to the engine's distinct k-mer sketch
    (``sketch_add_uploaded``) and is neither counted nor tallied; a ``spool`` is filled as in
    ``stream_batches_overlapped``.  The sketch leaves a batch in its upload slot (``kdf_sketch_add_uploaded``), so the
    engine's two slots still hold the last two batches afterwards: the next ``upload_async`` overwrites them, and a replay
    of host-tier spool segments into THIS engine is refused until they are taken -- the sizing pass of the discovery chain
    uses an engine of its own and closes it.  Returns the number of reads."""
    return _stream_batches(engine, readers, False, ring, False, spool, True)


def _stream_batches(engine, readers, filtered, ring, tally, spool, sketch) -> int:
    import queue
    import threading
    if not isinstance(readers, (list, tuple)):
        readers = [readers]
    n_reads = 0
    ring = ring or len(readers) + 2
    pinned = _pinned_ring(ring, readers[0].max_bases)
    free, ready = queue.Queue(), queue.Queue()
    for i in range(ring):
        free.put(i)
    stop = threading.Event()

    def produce(reader):
        try:
            while not stop.is_set():
                i = free.get()
                if i is None:
                    free.put(None)                           # (pass the stop token on to the other producers)
                    break
                st = reader.next_into(*pinned.batches[i])
                if st is None:
                    free.put(i)                              # unused: back to the ring
                    break
                ready.put((i, st))
            ready.put(None)
        except BaseException as ex:  # noqa: BLE001 -- handed to the consumer
            ready.put(ex)

    threads = [threading.Thread(target=produce, args=(rd,), name="kdf-reader", daemon=True) for rd in readers]
    for th in threads:
        th.start()
    take_slot = engine.sketch_add_uploaded if sketch else engine.prefilter_add_uploaded if tally else (lambda slot: engine.count_uploaded(slot, filtered))
    spooling = [spool]
    keep_reads = bool(getattr(spool, "keep_reads", False))

    def take(slot, st):
        # the spool's copy runs on the engine's stream right before the count of the same slot (not at upload time: the
        # engine's stream would then wait for the copy of batch i + 1 before it counts batch i); the slot keeps the batch
        if spooling[0] is not None:
            try:
                if keep_reads:
                    spooling[0].append_uploaded(engine, slot, offsets=st.offsets)
                else:
                    spooling[0].append_uploaded(engine, slot)
            except _native.KdfError as ex:
                if ex.code != _native.KDF_ERR_NOMEM:
                    raise
                spooling[0] = None                               # overflowed: neither budget holds the next segment
        take_slot(slot)
    pending = None                                           # (slot, buffer) uploaded, not yet counted
    slot = 0
    live = len(threads)
    try:
        while live:
            item = ready.get()
            if item is None:
                live -= 1
                continue
            if isinstance(item, BaseException):
                raise item
            i, st = item
            engine.upload_async(slot, st)                    # returns at once: the buffer is pinned
            n_reads += st.n_reads
            if pending is not None:
                take(pending[0], pending[2])
                free.put(pending[1])                         # count_uploaded waited (on the HOST) for this buffer's copy
            pending = (slot, i, st)
            slot ^= 1
        if pending is not None:
            take(pending[0], pending[2])
            pending = None
    finally:
        stop.set()
        free.put(None)
        for th in threads:
            th.join()                                        # the native reader call always returns; never close a reader under it
        engine.synchronize()                                 # no copy may still read a pinned buffer the next caller will fill
    return n_reads


def bam_reader(path: str, flag_off: int = FLAG_OFF_SAMTOOLS_FASTA, collapse: bool = True,
               max_bases: int = 1 << 26, max_reads: int = 1 << 20, threads: int = 1,
               want_meta: bool = False, want_aux: bool = False, part: int = 0, parts: int = 1) -> _Reader:
    """``samtools fasta -F flag_off`` as an iterator of ReadStream batches.  ``part`` of ``parts``: one BGZF range of
    the file, cut on record (QNAME-run) boundaries -- the parts together are the whole file, each record once
    (``kdf_bam_open_range``: the shard of one rank, or of one reader pipeline inside a process)."""
    h = c_void_p()
    if parts > 1:
        rc = _native.load().kdf_bam_open_range(path.encode(), flag_off, 1 if collapse else 0, threads, int(part), int(parts), byref(h))
    else:
        rc = _native.load().kdf_bam_open(path.encode(), flag_off, 1 if collapse else 0, threads, byref(h))
    _native.check_reader(rc, None)
    return _Reader(h, max_bases, max_reads, want_meta, want_aux, is_bam=True)


# ---- the device BAM feeder (kdf.h "device BAM feeder") ------------------------------------------------------------------
# the two tables of a planned batch, as include/kdf.h lays them out
BGZF_BLOCK_DTYPE = np.dtype([("comp_off", "<u8"), ("out_off", "<u8"), ("file_off", "<u8"), ("comp_len", "<u4"), ("isize", "<u4")])
SUBRANGE_DTYPE = np.dtype([("start", "<u8"), ("stop", "<u8"), ("flags", "<u8")])
SUB_NONE = 0xFFFFFFFFFFFFFFFF
SUB_AT_EOF = 1
SUB_DONE, SUB_UNFINISHED, SUB_CORRUPT = 0, 1, 2


@dataclass
class RawBatch:
    """One planned batch of compressed BGZF blocks (``kdf_bamraw_next``)."""
    comp: np.ndarray              # uint8: the blocks' DEFLATE payloads back to back (a view of the caller's buffer)
    blocks: np.ndarray            # BGZF_BLOCK_DTYPE[n_blocks]
    subs: np.ndarray              # SUBRANGE_DTYPE[n_subs]
    first_sub: int                # index in the part of subs[0]
    inflated_bytes: int           # the batch's inflated span


class _RawReader:
    """The raw range planner of one part of a BAM (host only: it reads compressed bytes and inflates nothing but what
    locating a sub-range's start takes)."""

    def __init__(self, handle, comp_cap: int, tail_blocks: int, args):
        self._h = handle
        self._lib = _native.load()
        self.comp_cap = int(comp_cap)
        self.tail_blocks = int(tail_blocks)
        self.cap_blocks = self.comp_cap // 512 + 1024
        self.args = args                                       # (path, flag_off, collapse, part, parts, subrange_bytes): a replay opens its own planner
        n = c_uint64(0)
        _native.check_bamraw(self._lib.kdf_bamraw_subranges(self._h, byref(n)), self._h)
        self.n_subranges = n.value
        self.cap_subs = max(1, min(self.n_subranges, 1 << 16))

    def close(self):
        if self._h:
            self._lib.kdf_bamraw_close(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def seek(self, sub: int):
        _native.check_bamraw(self._lib.kdf_bamraw_seek(self._h, int(sub)), self._h)

    def next_into(self, comp_buf: np.ndarray, tail_blocks: Optional[int] = None, max_subs: Optional[int] = None):
        """The next batch into ``comp_buf`` (uint8, e.g. a page-locked array) -> RawBatch, or None when the part is done."""
        if not self._h:
            return None
        cap_subs = self.cap_subs if max_subs is None else max(1, min(int(max_subs), self.cap_subs))
        blocks = np.zeros(self.cap_blocks, BGZF_BLOCK_DTYPE)
        subs = np.zeros(cap_subs, SUBRANGE_DTYPE)
        nb, ns, first, cb, ib = c_uint64(0), c_uint64(0), c_uint64(0), c_uint64(0), c_uint64(0)
        rc = self._lib.kdf_bamraw_next(self._h, _vp(comp_buf), min(len(comp_buf), self.comp_cap),
                                       self.tail_blocks if tail_blocks is None else int(tail_blocks), _vp(blocks), len(blocks),
                                       _vp(subs), len(subs), byref(nb), byref(ns), byref(first), byref(cb), byref(ib))
        _native.check_bamraw(rc, self._h)
        if ns.value == 0:
            return None
        return RawBatch(comp_buf[:cb.value], blocks[:nb.value], subs[:ns.value], first.value, ib.value)

    def __iter__(self) -> Iterator[RawBatch]:
        while True:
            b = self.next_into(np.empty(self.comp_cap, np.uint8))
            if b is None:
                break
            yield b


def bam_raw_reader(path: str, flag_off: int = FLAG_OFF_SAMTOOLS_FASTA, collapse: bool = True, part: int = 0, parts: int = 1,
                   subrange_bytes: int = 1 << 20, comp_cap: int = 1 << 26, tail_blocks: int = 0) -> _RawReader:
    """The raw planner of part ``part`` of ``parts`` of a BAM (the cuts of ``bam_reader(part=, parts=)``), cut again
    every ``subrange_bytes`` of file: batches of at most ``comp_cap`` compressed bytes with their block and sub-range
    tables, for ``KmerEngine.bamdev_decode_dev``.  ``tail_blocks``: blocks kept behind a batch's last sub-range (0: 2)."""
    h = c_void_p()
    rc = _native.load().kdf_bamraw_open(path.encode(), flag_off, 1 if collapse else 0, int(part), int(parts), int(subrange_bytes), byref(h))
    _native.check_bamraw(rc, None)
    return _RawReader(h, comp_cap, tail_blocks, (path, flag_off, collapse, int(part), int(parts), int(subrange_bytes)))


class PinnedBytes:
    """A ring of page-locked byte buffers (the compressed batches of the device feeder)."""

    def __init__(self, n: int, nbytes: int):
        self._lib = _native.load()
        self._ptrs, self.buffers = [], []
        try:
            for _ in range(n):
                p = c_void_p()
                _native.check(self._lib.kdf_host_alloc(nbytes, byref(p)), None)
                self._ptrs.append(p)
                self.buffers.append(np.ctypeslib.as_array(ctypes.cast(p, POINTER(ctypes.c_uint8)), (nbytes,)))
        except Exception:
            self.close()
            raise

    def close(self):
        self.buffers = []
        for p in self._ptrs:
            self._lib.kdf_host_free(p)
        self._ptrs = []


_pinned_bytes_cache = {}      # (ring, nbytes) -> PinnedBytes, kept for the life of the process (as _pinned_cache: page-locking costs more than a batch)


def _pinned_bytes(ring: int, nbytes: int) -> PinnedBytes:
    key = (ring, nbytes)
    pb = _pinned_bytes_cache.get(key)
    if pb is None or not pb.buffers:
        for old in list(_pinned_bytes_cache.values()):
            old.close()
        _pinned_bytes_cache.clear()
        pb = _pinned_bytes_cache[key] = PinnedBytes(ring, nbytes)
    return pb


def decode_capacity(inflated_bytes: int):
    """(cap_bases, cap_reads) that hold whatever ``inflated_bytes`` of BAM records decode to: a record is >= 36 bytes and
    carries (l_seq + 1) / 2 sequence bytes, so positions <= 2 x bytes + one separator per record."""
    cap_reads = inflated_bytes // 36 + 1
    return 2 * inflated_bytes + cap_reads + 64, cap_reads


class _DeviceSlot:
    """Device buffers of one batch in flight (grow-only torch tensors on the feeder's stream)."""

    def __init__(self, torch, dev):
        self.torch, self.dev = torch, dev
        self.comp = self.blocks = self.subs = self.packed = self.invalid = self.offsets = None
        self.copied = None
        self.used = None                                       # recorded on the work stream behind the last kernels that read this slot
        self.grew = False

    def _room(self, name, n, dtype):
        t = getattr(self, name)
        if t is None or t.numel() < n:
            t = self.torch.empty(int(n + n // 8 + 64), dtype=dtype, device=self.dev)
            setattr(self, name, t)
            self.grew = True
        return t

    def upload(self, batch: RawBatch, copy_stream):
        torch = self.torch
        cap_bases, cap_reads = decode_capacity(batch.inflated_bytes)
        pw, mw = stream_words(cap_bases)
        self._room("packed", pw, torch.int64); self._room("invalid", mw, torch.int64); self._room("offsets", cap_reads + 1, torch.int64)
        views = (("comp", batch.comp, torch.uint8), ("blocks", batch.blocks.view(np.uint8), torch.uint8), ("subs", batch.subs.view(np.uint8), torch.uint8))
        for name, arr, dt in views:
            self._room(name, max(len(arr), 1), dt)
        if self.grew:                                                  # (memory the allocator hands out again may still be in use on this stream)
            torch.cuda.current_stream(self.dev).synchronize()
            self.grew = False
        with torch.cuda.stream(copy_stream):
            # the decode of the batch this slot held returns with its write pass and its pack still queued on the work
            # stream, and they read the slot's tables: the copies that overwrite them wait for those kernels
            if self.used is not None:
                copy_stream.wait_event(self.used)
            for name, arr, dt in views:
                if len(arr):
                    getattr(self, name)[:len(arr)].copy_(torch.from_numpy(arr), non_blocking=True)
            self.copied = torch.cuda.Event()
            self.copied.record(copy_stream)
        self.batch, self.cap_bases, self.cap_reads = batch, cap_bases, cap_reads


LAST_FEEDER = None            # what the last stream_bam_device call did: {"path", "batches", "fallback_blocks", "replays", ...}


def stream_bam_device(engine, path: str, parts_of_this_process, filtered: bool = False, tally: bool = False, sketch: bool = False,
                      spool=None, flag_off: int = FLAG_OFF_SAMTOOLS_FASTA, collapse: bool = True, subrange_bytes: int = 1 << 20,
                      comp_cap: int = 1 << 26, tail_blocks: int = 0, producers: int = 4) -> int:
    """Count (``filtered``: count --if; ``tally``: prefilter pass 1; ``sketch``: sizing pass) a BAM through the DEVICE
    feeder: producer threads plan batches of compressed BGZF blocks into page-locked buffers (``bam_raw_reader``), a copy
    stream uploads batch i + 1 while the engine inflates, walks and packs batch i on the device (``bamdev_decode_dev``)
    and takes the stream where it lies in HBM.  ``parts_of_this_process``: [(part, parts), ...] -- the shares of the file
    this process reads (a rank's contiguous parts).  ``spool``: as in ``stream_batches_overlapped``; it is filled from the
    device buffers (with the device read offsets when ``spool.keep_reads`` is set) before the batch is counted.  A
    sub-range whose walk ran off the batch's bytes is replayed with a longer tail; nothing is lost or doubled.  For the
    call's duration the engine runs on a stream of the feeder's; it is back on its own stream afterwards.  Returns the
    number of reads; ``LAST_FEEDER`` records batches, fallback blocks, replays and the planner's time."""
    global LAST_FEEDER
    import queue
    import threading
    import time
    import torch
    dev = torch.device("cuda", engine.device)
    readers = [bam_raw_reader(path, flag_off, collapse, p, n, subrange_bytes, comp_cap, tail_blocks) for p, n in parts_of_this_process]
    ring = min(len(readers), max(1, int(producers))) + 2
    pinned = _pinned_bytes(ring, comp_cap)
    free, ready = queue.Queue(), queue.Queue()
    for i in range(ring):
        free.put(i)
    todo = queue.Queue()
    for rd in readers:
        todo.put(rd)
    stop = threading.Event()
    plan_s = [0.0]
    lock = threading.Lock()

    def produce():
        try:
            while not stop.is_set():
                try:
                    rd = todo.get_nowait()
                except queue.Empty:
                    break
                while not stop.is_set():
                    i = free.get()
                    if i is None:
                        free.put(None)
                        return
                    t0 = time.perf_counter()
                    b = rd.next_into(pinned.buffers[i])
                    with lock:
                        plan_s[0] += time.perf_counter() - t0
                    if b is None:
                        free.put(i)
                        break
                    ready.put((rd, i, b))
            ready.put(None)
        except BaseException as ex:  # noqa: BLE001 -- handed to the consumer
            ready.put(ex)

    n_threads = min(len(readers), max(1, int(producers)))
    threads = [threading.Thread(target=produce, name="kdf-rawplan", daemon=True) for _ in range(n_threads)]
    work, copy_stream = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    engine.synchronize()
    engine.set_stream(work.cuda_stream)
    fallback0 = engine.get_stat("bamdev_fallback_blocks")
    info = {"path": "device", "batches": 0, "replays": 0, "h2d_bytes": 0, "subranges": sum(r.n_subranges for r in readers)}
    spooling = [spool]
    keep_reads = bool(getattr(spool, "keep_reads", False))
    n_reads = 0

    def consume(slot):
        """decode the slot's batch and hand the stream to the engine -> reads, index of the first sub-range not taken"""
        b = slot.batch
        nb, nr, status = engine.bamdev_decode_dev(slot.comp.data_ptr(), slot.blocks.data_ptr(), len(b.blocks), slot.subs.data_ptr(), len(b.subs),
                                                  flag_off, collapse, slot.packed.data_ptr(), slot.invalid.data_ptr(), slot.cap_bases,
                                                  slot.offsets.data_ptr(), slot.cap_reads)
        bad = np.flatnonzero(status != SUB_DONE)
        taken = int(bad[0]) if len(bad) else len(b.subs)
        if nb:
            dp, dm = slot.packed.data_ptr(), slot.invalid.data_ptr()
            if spooling[0] is not None:
                try:
                    if keep_reads:
                        spooling[0].append_dev(dp, dm, nb, work.cuda_stream, d_offsets=slot.offsets.data_ptr(), n_reads=nr)
                    else:
                        spooling[0].append_dev(dp, dm, nb, work.cuda_stream)
                except _native.KdfError as ex:
                    if ex.code != _native.KDF_ERR_NOMEM:
                        raise
                    spooling[0] = None                               # overflowed: the pass itself goes on
            if sketch:
                engine.sketch_add_dev(dp, dm, nb)
            elif tally:
                engine.prefilter_add_dev(dp, dm, nb)
            elif filtered:
                engine.count_filtered_dev(dp, dm, nb)
            else:
                engine.count_dev(dp, dm, nb)
        slot.used = torch.cuda.Event()
        slot.used.record(work)                                   # (behind the decode's last kernels and the consumer's)
        info["batches"] += 1
        return nr, taken

    def replay(rd, first, last):
        """sub-ranges [first, last) of rd's part, one at a time through a planner of their own, the tail doubled until the walk ends"""
        got = 0
        slot = _DeviceSlot(torch, dev)
        with bam_raw_reader(*rd.args, comp_cap=comp_cap) as rp, torch.cuda.stream(work):
            buf = np.empty(comp_cap, np.uint8)
            for sub in range(first, last):
                tail = max(rd.tail_blocks, 2) * 4
                while True:
                    rp.seek(sub)
                    b = rp.next_into(buf, tail_blocks=tail, max_subs=1)
                    slot.upload(b, copy_stream)
                    slot.copied.synchronize()
                    info["h2d_bytes"] += len(b.comp)
                    nr, taken = consume(slot)
                    engine.synchronize()                             # (the slot is reused at once)
                    info["replays"] += 1
                    if taken == 1:
                        got += nr
                        break
                    tail *= 4
        return got

    slots = [_DeviceSlot(torch, dev), _DeviceSlot(torch, dev)]
    try:
        for th in threads:
            th.start()
        live, cur, pending = len(threads), 0, None                   # pending: (slot, reader, pinned index) uploaded, not yet decoded
        with torch.cuda.stream(work):
            def finish(p):
                nonlocal n_reads
                slot, rd, i = p
                slot.copied.synchronize()
                free.put(i)                                          # the copy is done: the pinned buffer goes back to the producers
                nr, taken = consume(slot)
                n_reads += nr
                if taken < len(slot.batch.subs):
                    n_reads += replay(rd, slot.batch.first_sub + taken, slot.batch.first_sub + len(slot.batch.subs))
            while live:
                item = ready.get()
                if item is None:
                    live -= 1
                    continue
                if isinstance(item, BaseException):
                    raise item
                rd, i, b = item
                slots[cur].upload(b, copy_stream)                    # returns at once: the buffer is page-locked
                info["h2d_bytes"] += len(b.comp) + b.blocks.nbytes + b.subs.nbytes
                if pending is not None:
                    finish(pending)
                pending = (slots[cur], rd, i)
                cur ^= 1
            if pending is not None:
                finish(pending)
    finally:
        stop.set()
        free.put(None)
        for th in threads:
            if th.is_alive() or th.ident is not None:
                th.join()
        try:
            engine.synchronize()
        finally:
            engine.set_stream(None)
            copy_stream.synchronize()                                # no copy may still read a pinned buffer the next caller will fill
            for rd in readers:
                rd.close()
    info["fallback_blocks"] = engine.get_stat("bamdev_fallback_blocks") - fallback0
    info["plan_seconds"] = plan_s[0]
    info["reads"] = n_reads
    LAST_FEEDER = info
    return n_reads


LAST_FASTA_FEEDER = None      # what the last stream_fasta_device call did: {"path", "chunks", "bytes", "carries", "compressed", "records"}


class _FastaText:
    """The text of a FASTA file, chunk by chunk into caller buffers: a plain file is read in place, a gzip or BGZF file
    (found by its magic) is inflated with zlib, member after member."""

    def __init__(self, path: str):
        self.f = open(path, "rb", buffering=0)
        magic = self.f.read(2)
        self.f.seek(0)
        self.compressed = magic == b"\x1f\x8b"
        self._z, self._pending = None, b""

    def close(self):
        self.f.close()

    def readinto(self, buf: np.ndarray) -> int:
        """Fill ``buf`` (uint8) from its start -> bytes written; fewer than len(buf) only at the file's end."""
        if not self.compressed:
            view, n = memoryview(buf), 0
            while n < len(buf):
                got = self.f.readinto(view[n:])
                if not got:
                    break
                n += got
            return n
        import zlib
        n = 0
        while n < len(buf):
            if self._z is None:                                        # the next member, if the file has one
                if not self._pending:
                    self._pending = self.f.read(1 << 20)
                    if not self._pending:
                        break
                self._z = zlib.decompressobj(31)
            data = self._pending or self.f.read(1 << 20)
            if not data:
                raise OSError("compressed FASTA ends inside a gzip member")
            out = self._z.decompress(data, len(buf) - n)
            buf[n:n + len(out)] = np.frombuffer(out, np.uint8)
            n += len(out)
            if self._z.eof:
                self._pending, self._z = self._z.unused_data, None
            else:
                self._pending = self._z.unconsumed_tail              # (what the output limit kept it from taking)
        return n


def stream_fasta_device(engine, path: str, k: int, filtered: bool = False, tally: bool = False, sketch: bool = False, spool=None,
                        chunk_bytes: Optional[int] = None) -> int:
    """Count (``filtered``: count --if; ``tally``: prefilter pass 1; ``sketch``: sizing pass) a (multi-)FASTA through the
    DEVICE feeder: one reader thread fills two page-locked buffers with the file's text (``chunk_bytes`` each; default
    KDF_FASTA_FEED_MB MiB, 64), a copy stream uploads chunk i + 1 while the engine packs chunk i on the device
    (``fasta_pack_dev``) into one of two alternating stream buffers, behind the last k - 1 positions of the other, and
    takes the stream where it lies in HBM.  The batches hold every valid window of the file's stream exactly once.  A
    gzip or BGZF file is inflated on the host into the same buffers.  ``spool``: as in ``stream_bam_device``.  For the
    call's duration the engine runs on a stream of the feeder's.  Returns the number of records; ``LAST_FASTA_FEEDER``
    records chunks, bytes and carries."""
    global LAST_FASTA_FEEDER
    import os
    import queue
    import threading
    import torch
    if chunk_bytes is None:
        chunk_bytes = int(float(os.environ.get("KDF_FASTA_FEED_MB", "64")) * (1 << 20))
    src = _FastaText(path)
    if not src.compressed:                                       # a small file (proband_unique.fa) pins and allocates no more than it needs
        chunk_bytes = min(int(chunk_bytes), os.path.getsize(path) + 16)
    chunk_bytes = max(16, int(chunk_bytes) // 16 * 16)
    carry = max(int(k) - 1, 0)
    dev = torch.device("cuda", engine.device)
    pinned = _pinned_bytes(2, chunk_bytes)
    free, ready = queue.Queue(), queue.Queue()
    free.put(0)
    free.put(1)
    stop = threading.Event()

    def produce():
        try:
            while not stop.is_set():
                i = free.get()
                if i is None:
                    return
                n = src.readinto(pinned.buffers[i])
                if n == 0:
                    break
                ready.put((i, n))
            ready.put(None)
        except BaseException as ex:  # noqa: BLE001 -- handed to the consumer
            ready.put(ex)

    reader = threading.Thread(target=produce, name="kdf-fasta-text", daemon=True)
    work, copy_stream = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    engine.synchronize()
    engine.set_stream(work.cuda_stream)
    info = {"path": "device", "chunks": 0, "bytes": 0, "carries": 0, "compressed": src.compressed}
    state = _native.FastaState()
    spooling = [spool]
    keep_reads = bool(getattr(spool, "keep_reads", False))
    text = [torch.empty(chunk_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
    used = [None, None]                                          # recorded on the work stream behind the pack that read the text slot
    out = [None, None]                                           # (packed, invalid, offsets, cap_bases, cap_reads) of the alternating stream buffers
    prev = [None]                                                # (slot, n_bases) of the previous stream
    left = [0]                                                   # trailing '\r' of the previous chunk, handed over again

    def room(j, n_text):
        cap_bases, cap_reads = n_text + carry + 1, (n_text // 2 + 2 if keep_reads else 0)
        if out[j] is None or out[j][3] < cap_bases or out[j][4] < cap_reads:
            pw, mw = stream_words(cap_bases)
            torch.cuda.current_stream(dev).synchronize()          # (memory the allocator hands out again may still be in use on this stream)
            out[j] = (torch.empty(pw, dtype=torch.int64, device=dev), torch.empty(mw, dtype=torch.int64, device=dev),
                      torch.empty(cap_reads + 1, dtype=torch.int64, device=dev) if keep_reads else None, cap_bases, cap_reads)
        return out[j]

    def pack(t, n_text, final):
        """pack t[:n_text] into the stream buffer the previous stream does not lie in, hand it to the engine -> consumed"""
        j = 0 if prev[0] is None else prev[0][0] ^ 1
        packed, invalid, offs, cap_bases, cap_reads = room(j, n_text)
        pp = (out[prev[0][0]][0].data_ptr(), out[prev[0][0]][1].data_ptr(), prev[0][1]) if prev[0] is not None else (None, None, 0)
        in_record = bool(state.flags & _native.KDF_FA_IN_RECORD)
        nb, nr, consumed = engine.fasta_pack_dev(t.data_ptr() if n_text else None, n_text, final, state, packed.data_ptr(), invalid.data_ptr(),
                                                 cap_bases, offs.data_ptr() if offs is not None else None, cap_reads, pp[0], pp[1], pp[2], carry)
        if n_text == 0 and not final:
            return 0
        info["carries"] += 1 if (in_record and carry and pp[2]) else 0
        prev[0] = (j, nb)
        if nb:
            dp, dm = packed.data_ptr(), invalid.data_ptr()
            if spooling[0] is not None:
                try:
                    if keep_reads:
                        spooling[0].append_dev(dp, dm, nb, work.cuda_stream, d_offsets=offs.data_ptr(), n_reads=nr)
                    else:
                        spooling[0].append_dev(dp, dm, nb, work.cuda_stream)
                except _native.KdfError as ex:
                    if ex.code != _native.KDF_ERR_NOMEM:
                        raise
                    spooling[0] = None                               # overflowed: the pass itself goes on
            if sketch:
                engine.sketch_add_dev(dp, dm, nb)
            elif tally:
                engine.prefilter_add_dev(dp, dm, nb)
            elif filtered:
                engine.count_filtered_dev(dp, dm, nb)
            else:
                engine.count_dev(dp, dm, nb)
        return consumed

    def cr_run(n):
        return torch.full((n,), 13, dtype=torch.uint8, device=dev)

    try:
        reader.start()
        pending, cur = None, 0                                       # pending: (text slot, pinned index, bytes, copied event)
        with torch.cuda.stream(work):
            def finish(p):
                slot, i, n, copied = p
                copied.synchronize()
                free.put(i)                                          # the copy is done: the pinned buffer goes back to the reader
                work.wait_event(copied)
                t, n_text = text[slot], n
                if left[0]:                                          # the '\r' the last chunk left, in front of this one
                    t, n_text = torch.cat((cr_run(left[0]), text[slot][:n])), n + left[0]
                consumed = pack(t, n_text, False)
                left[0] = n_text - consumed
                used[slot] = torch.cuda.Event()
                used[slot].record(work)
                info["chunks"] += 1
                info["bytes"] += n
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                i, n = item
                with torch.cuda.stream(copy_stream):
                    if used[cur] is not None:
                        copy_stream.wait_event(used[cur])            # the pack that read this slot's last chunk
                    text[cur][:n].copy_(torch.from_numpy(pinned.buffers[i][:n]), non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(copy_stream)
                if pending is not None:
                    finish(pending)
                pending = (cur, i, n, copied)
                cur ^= 1
            if pending is not None:
                finish(pending)
            pack(cr_run(left[0]) if left[0] else text[0], left[0], True)     # the file's end: the closing separator
    finally:
        stop.set()
        free.put(None)
        if reader.ident is not None:
            reader.join()
        try:
            engine.synchronize()
        finally:
            engine.set_stream(None)
            copy_stream.synchronize()                                # no copy may still read a pinned buffer the next caller will fill
            src.close()
    info["records"] = int(state.records)
    info["positions"] = int(state.positions)
    LAST_FASTA_FEEDER = info
    return int(state.records)


LAST_FASTQ_FEEDER = None      # what the last stream_fastq_device call did: {"path", "files", "chunks", "bytes", "records", "positions", "compressed", "min_qual"}
FASTQ_SUFFIXES = (".fastq", ".fq", ".fastq.gz", ".fq.gz")


def is_fastq_path(path) -> bool:
    """The name says FASTQ: one path that ends in .fastq / .fq / .fastq.gz / .fq.gz, or a comma-separated list of such."""
    if path is None:
        return False
    parts = fastq_paths(path)
    return bool(parts) and all(p.lower().endswith(FASTQ_SUFFIXES) for p in parts)


def fastq_paths(paths) -> List[str]:
    """One path, a comma-separated list of paths or a sequence of paths -> the list of paths (R1, R2, ...)."""
    import os
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        return [p for p in os.fsdecode(os.fspath(paths)).split(",") if p]
    return [os.fsdecode(os.fspath(p)) for p in paths]


def refuse_fastq(path, what: str):
    """The paths that need an alignment name a FASTQ child and refuse it."""
    if is_fastq_path(path):
        raise ValueError(f"{what} needs aligned reads (a BAM): {path} is FASTQ, which only the alignment-free counting legs take")


def fastq_min_qual(value=None) -> int:
    """``KDF_FASTQ_MIN_QUAL`` (or ``value``) -> the byte below which a quality masks its base (`jellyfish count -Q`): a
    string of digits is that number (0 .. 255), any other single character is its code; unset, empty or 0: off."""
    import os
    v = os.environ.get("KDF_FASTQ_MIN_QUAL", "") if value is None else value
    if isinstance(v, int):
        q = v
    elif v == "":
        q = 0
    elif v.isdigit():
        q = int(v)
    elif len(v) == 1:
        q = ord(v)
    else:
        raise ValueError(f"KDF_FASTQ_MIN_QUAL={v!r}: one character or a number 0 .. 255")
    if not 0 <= q <= 255:
        raise ValueError(f"KDF_FASTQ_MIN_QUAL={v!r}: outside 0 .. 255")
    return q


def _walk_fastq_chunks(engine, files, chunk_bytes, what: str, consume):
    """The text of the FASTQ ``files``, one after the other, through HBM in chunks of whole records: the part that
    ``stream_fastq_device`` and ``informative_fastq`` share.  One reader thread fills two page-locked buffers with the text
    (``chunk_bytes`` each; default KDF_FASTQ_FEED_MB MiB, 64; a gzip or multi-member gzip file is inflated on the host), a
    copy stream uploads chunk i + 1 while the consumer works on chunk i, and the unconsumed tail of a chunk is copied in front
    of the next on the device.  ``consume(f, text, n_text, final, work) -> consumed`` is handed the index of the file, a view
    of the text in HBM, its length, whether this is the file's final call, and the stream it runs on (the current torch
    stream, and the engine's for the walk's duration); it returns what a ``fastq_*_dev`` call consumed.  A
    ``FastqFormatError`` it raises is raised again with the file's name and the offset within the file.
    -> {"files", "chunks", "bytes", "compressed"}."""
    import os
    import queue
    import threading
    import torch
    if chunk_bytes is None:
        chunk_bytes = int(float(os.environ.get("KDF_FASTQ_FEED_MB", "64")) * (1 << 20))
    srcs = [_FastaText(p) for p in files]                         # (the text of a file, plain or gzip: nothing of it is FASTA's)
    if not any(s.compressed for s in srcs):                       # small files pin and allocate no more than they need
        chunk_bytes = min(int(chunk_bytes), max(os.path.getsize(p) for p in files) + 16)
    chunk_bytes = max(16, int(chunk_bytes) // 16 * 16)
    dev = torch.device("cuda", engine.device)
    pinned = _pinned_bytes(2, chunk_bytes)
    free, ready = queue.Queue(), queue.Queue()
    free.put(0)
    free.put(1)
    stop = threading.Event()

    def produce():
        try:
            for f, src in enumerate(srcs):
                while not stop.is_set():
                    i = free.get()
                    if i is None:
                        return
                    n = src.readinto(pinned.buffers[i])
                    if n == 0:
                        free.put(i)
                        break
                    ready.put((f, i, n))
                ready.put((f, None, 0))                              # the file's end
            ready.put(None)
        except BaseException as ex:  # noqa: BLE001 -- handed to the consumer
            ready.put(ex)

    reader = threading.Thread(target=produce, name="kdf-fastq-text", daemon=True)
    work, copy_stream = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    engine.synchronize()
    engine.set_stream(work.cuda_stream)
    info = {"files": len(files), "chunks": 0, "bytes": 0, "compressed": any(s.compressed for s in srcs)}
    # a text slot: the chunk at [chunk_bytes, 2 chunk_bytes), and directly in front of it the tail the call on the OTHER
    # slot left (at most chunk_bytes): the copy stream writes the upper half only, the work stream the lower
    text = [torch.empty(2 * chunk_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
    used = [None, None]                                          # recorded on the work stream behind the last reader of the slot's chunk
    left = [0, 0]                                                # (text slot, bytes) of the unconsumed tail: it ends at the slot's chunk_bytes
    file_base = [0]                                              # bytes of the current file that earlier calls consumed
    cur_file = [0]

    def take(t, n_text, final):
        """hand t[:n_text] to the consumer -> consumed"""
        try:
            consumed = consume(cur_file[0], t, n_text, final, work)
        except _native.FastqFormatError as ex:
            raise _native.FastqFormatError(ex.code, f"{files[cur_file[0]]}: byte {file_base[0] + ex.offset}: {ex}", file_base[0] + ex.offset, ex.rule) from None
        file_base[0] += consumed
        return consumed

    try:
        reader.start()
        pending, cur = None, 0                                       # pending: (text slot, pinned index, bytes, copied event)
        with torch.cuda.stream(work):
            def finish(p):
                slot, i, n, copied = p
                copied.synchronize()
                free.put(i)                                          # the copy is done: the pinned buffer goes back to the reader
                work.wait_event(copied)
                start = chunk_bytes - left[1]                        # (the tail was put in front of this slot's chunk)
                n_text = left[1] + n
                consumed = take(text[slot][start:start + n_text], n_text, False)
                rest = n_text - consumed
                if rest > chunk_bytes:
                    raise ValueError(f"{what}: {files[cur_file[0]]}: {rest} bytes behind byte {file_base[0]} hold no complete FASTQ "
                                     f"record and a chunk is {chunk_bytes} bytes: raise KDF_FASTQ_FEED_MB (a chunk must hold the longest record)")
                if rest:                                             # in front of the other slot's chunk, where the next call reads
                    text[slot ^ 1][chunk_bytes - rest:chunk_bytes].copy_(text[slot][start + consumed:start + n_text])
                left[0], left[1] = slot ^ 1, rest
                used[slot] = torch.cuda.Event()
                used[slot].record(work)
                info["chunks"] += 1
                info["bytes"] += n

            def close_file():
                """the file's end: what the last call left is the final call's text"""
                slot, m = left
                if m:
                    take(text[slot][chunk_bytes - m:chunk_bytes], m, True)
                left[1] = 0
                file_base[0] = 0

            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                f, i, n = item
                cur_file[0] = f
                if i is None:                                        # the end of file f
                    if pending is not None:
                        finish(pending)
                        pending = None
                    close_file()
                    continue
                with torch.cuda.stream(copy_stream):
                    if used[cur] is not None:
                        copy_stream.wait_event(used[cur])            # the pack and the tail copy that read this slot's last chunk
                    text[cur][chunk_bytes:chunk_bytes + n].copy_(torch.from_numpy(pinned.buffers[i][:n]), non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(copy_stream)
                if pending is not None:
                    finish(pending)
                pending = (cur, i, n, copied)
                cur ^= 1
    finally:
        stop.set()
        free.put(None)
        if reader.ident is not None:
            reader.join()
        try:
            engine.synchronize()
        finally:
            engine.set_stream(None)
            copy_stream.synchronize()                                # no copy may still read a pinned buffer the next caller will fill
            for s in srcs:
                s.close()
    return info


def stream_fastq_device(engine, paths, filtered: bool = False, tally: bool = False, sketch: bool = False, spool=None, min_qual: int = 0,
                        chunk_bytes: Optional[int] = None) -> int:
    """Count (``filtered``: count --if; ``tally``: prefilter pass 1; ``sketch``: sizing pass) four-line FASTQ files through
    the DEVICE feeder.  ``paths``: one path or a sequence of paths (R1, R2, ...), streamed one after the other; a gzip or
    multi-member gzip file is inflated on the host.  One reader thread fills two page-locked buffers with the text
    (``chunk_bytes`` each; default KDF_FASTQ_FEED_MB MiB, 64), a copy stream uploads chunk i + 1 while the engine packs chunk
    i on the device (``fastq_pack_dev``) into one of two alternating stream buffers and takes the stream where it lies in
    HBM.  A call consumes whole records; the unconsumed tail of a chunk is copied in front of the next on the device
    (``_walk_fastq_chunks``).  ``min_qual`` > 0 masks the bases of a lower quality byte (`jellyfish count -Q`).  ``spool``: as in
    ``stream_bam_device``; with ``spool.keep_reads`` the records' offsets are kept.  For the call's duration the engine runs
    on a stream of the feeder's.  Returns the number of records; ``LAST_FASTQ_FEEDER`` records files, chunks, bytes, records
    and positions.  A text that is no FASTQ raises ``FastqFormatError`` with the offset within its file."""
    global LAST_FASTQ_FEEDER
    import torch
    files = fastq_paths(paths)
    if not files:
        raise ValueError("stream_fastq_device: no path")
    dev = torch.device("cuda", engine.device)
    state = _native.FastqState()
    spooling = [spool]
    keep_reads = bool(getattr(spool, "keep_reads", False))
    out = [None, None]                                           # (packed, invalid, offsets, cap_bases, cap_reads) of the alternating stream buffers
    turn = [0]

    def room(j, n_text):
        cap_bases, cap_reads = n_text // 2, (n_text // 4 if keep_reads else 0)
        if out[j] is None or out[j][3] < cap_bases or out[j][4] < cap_reads:
            pw, mw = stream_words(cap_bases)
            torch.cuda.current_stream(dev).synchronize()          # (memory the allocator hands out again may still be in use on this stream)
            out[j] = (torch.empty(pw, dtype=torch.int64, device=dev), torch.empty(mw, dtype=torch.int64, device=dev),
                      torch.empty(cap_reads + 1, dtype=torch.int64, device=dev) if keep_reads else None, cap_bases, cap_reads)
        return out[j]

    def pack(f, t, n_text, final, work):
        """pack t[:n_text] into the stream buffer the previous stream does not lie in, hand it to the engine -> consumed"""
        j = turn[0]
        turn[0] ^= 1
        packed, invalid, offs, cap_bases, cap_reads = room(j, n_text)
        nb, nr, consumed = engine.fastq_pack_dev(t.data_ptr() if n_text else None, n_text, final, state, packed.data_ptr(), invalid.data_ptr(),
                                                 cap_bases, offs.data_ptr() if offs is not None else None, cap_reads, min_qual)
        if nb:
            dp, dm = packed.data_ptr(), invalid.data_ptr()
            if spooling[0] is not None:
                try:
                    if keep_reads:
                        spooling[0].append_dev(dp, dm, nb, work.cuda_stream, d_offsets=offs.data_ptr(), n_reads=nr)
                    else:
                        spooling[0].append_dev(dp, dm, nb, work.cuda_stream)
                except _native.KdfError as ex:
                    if ex.code != _native.KDF_ERR_NOMEM:
                        raise
                    spooling[0] = None                               # overflowed: the pass itself goes on
            if sketch:
                engine.sketch_add_dev(dp, dm, nb)
            elif tally:
                engine.prefilter_add_dev(dp, dm, nb)
            elif filtered:
                engine.count_filtered_dev(dp, dm, nb)
            else:
                engine.count_dev(dp, dm, nb)
        return consumed

    walked = _walk_fastq_chunks(engine, files, chunk_bytes, "stream_fastq_device", pack)
    info = {"path": "device", "files": walked["files"], "chunks": walked["chunks"], "bytes": walked["bytes"], "compressed": walked["compressed"],
            "min_qual": int(min_qual), "records": int(state.records), "positions": int(state.positions)}
    LAST_FASTQ_FEEDER = info
    return int(state.records)


LAST_FASTQ_SUBSET = None      # what the last informative_fastq call did: {"files", "paired", "passes", "chunks", "bytes_read", "bytes_written", "records", "kept", "min_distinct", "min_qual", "compressed"}


def informative_fastq(engine, paths, out_paths, min_distinct: int = 1, paired: Optional[bool] = None, min_qual: int = 0,
                      chunk_bytes: Optional[int] = None):
    """The records of four-line FASTQ files that carry at least ``min_distinct`` distinct k-mers of the engine's table,
    written as FASTQ text, byte for byte: Module 3's read selection for a sample that starts from FASTQ, without an alignment
    and without a host pass over the text.  The caller has loaded the candidate k-mer set into ``engine`` (as for
    ``scan_bam_module3``: keys with a count > 0).  ``paths`` / ``out_paths``: one path per input and one output per input (a
    ``.gz`` output name is refused: compressing the small output is the caller's).

    Per chunk (``_walk_fastq_chunks``): ``fastq_pack_dev`` with the record offsets, ``read_hits_dev`` against the table,
    ``keep = distinct >= min_distinct`` as a torch op on the device (``min_distinct <= 0`` keeps every record), and
    ``fastq_extract_dev`` on the same chunk while its text is still in HBM; the kept bytes go through a page-locked buffer to
    ``write()``.  ``min_qual`` masks low-quality bases for the scan as in ``stream_fastq_device``; the text written is
    the file's.

    Unpaired (one file; several files with ``paired=False``; ``paired=None`` with other than two files): one pass, every
    file on its own.  Paired (``paired=True``, or ``None`` with exactly two files): pass 1 keeps one uint32 ``distinct`` per
    record per file on the device -- 4 bytes per record, about 3.6 GB for a 30x human pair of 2 x 450 M reads --, the two
    files must hold the same number of records (``ValueError`` naming both counts otherwise; names are not compared), a
    pair is kept when either mate qualifies, and pass 2 streams both files again and extracts with the flags of the records
    [records so far, + the chunk's), so the outputs stay in step: record i of R1 with record i of R2.  The flags are
    complete on the device before pass 2 starts (the call waits for them), and a file that changed between the passes is
    refused, not written wrongly.

    An output is opened at its first write, or at the end when nothing of its file was kept: unequal record counts of a
    pair leave no output behind, and an error later in the text leaves what was written before it.

    -> a list with one dict per file: ``records``, ``kept``, ``ordinals`` (int64, the ascending record numbers within the
    file of the records written) and ``distinct`` (uint32 of those records, a mate's own value).  ``LAST_FASTQ_SUBSET``
    records files, chunks, passes, bytes read and written.  A text that is no FASTQ raises ``FastqFormatError`` with the
    offset within its file.  For the call's duration the engine runs on a stream of the walker's."""
    global LAST_FASTQ_SUBSET
    import torch
    from . import dist_env
    files, outs = fastq_paths(paths), fastq_paths(out_paths)
    if not files:
        raise ValueError("informative_fastq: no path")
    if dist_env.world_rank()[0] > 1:
        raise ValueError(f"a FASTQ sample ({','.join(files)}) is not sharded over ranks: select its reads in one process")
    if len(outs) != len(files):
        raise ValueError(f"informative_fastq: {len(files)} inputs and {len(outs)} outputs: one output per input")
    for o in outs:
        if o.lower().endswith(".gz"):
            raise ValueError(f"informative_fastq: {o}: the output is written as plain text (compress the small output afterwards)")
    if paired and len(files) != 2:
        raise ValueError(f"informative_fastq: paired=True takes two files (R1, R2), not {len(files)}")
    pair = len(files) == 2 if paired is None else bool(paired)
    min_distinct = int(min_distinct)
    dev = torch.device("cuda", engine.device)
    state = _native.FastqState()
    buf = {}                                                     # the buffers of a chunk, grown when a chunk needs more
    n_files = len(files)
    records, kept, written = [0] * n_files, [0] * n_files, [0] * n_files
    scores = [[] for _ in files]                                 # per file: the uint32 `distinct` of every chunk, on the device
    chosen = [[] for _ in files]                                 # per file: (ordinals, distinct) of the kept records of every chunk, on the host
    sinks = [None] * n_files
    flags = [None]                                               # paired, pass 2: uint8 per record of a file
    done = [0] * n_files                                         # pass 2: records of the file that earlier calls held
    calls, turn = [[] for _ in files], [0] * n_files             # pass 1: the records of every call on a file; pass 2: the call it is at

    def room(n_text):
        cap_bases, cap_reads = n_text // 2, n_text // 4
        if not buf or buf["cap_bases"] < cap_bases:
            pw, mw = stream_words(cap_bases)
            torch.cuda.current_stream(dev).synchronize()          # (memory the allocator hands out again may still be in use on this stream)
            buf.update(packed=torch.empty(pw, dtype=torch.int64, device=dev), invalid=torch.empty(mw, dtype=torch.int64, device=dev),
                       offs=torch.empty(cap_reads + 1, dtype=torch.int64, device=dev), rows=torch.empty((cap_reads + 1, 2), dtype=torch.int32, device=dev),
                       cap_bases=cap_bases, cap_reads=cap_reads)
        return buf

    def out_room(n_text):
        if buf.get("cap_out", -1) < n_text + 2:
            torch.cuda.current_stream(dev).synchronize()
            buf.update(out=torch.empty(n_text + 2, dtype=torch.uint8, device=dev), host=torch.empty(n_text + 2, dtype=torch.uint8).pin_memory(),
                       cap_out=n_text + 2)
        return buf

    def score(t, n_text, final):
        """-> (records, consumed, uint32 `distinct` per record as an int32 tensor view on the device)"""
        b = room(n_text)
        nb, nr, consumed = engine.fastq_pack_dev(t.data_ptr() if n_text else None, n_text, final, state, b["packed"].data_ptr(), b["invalid"].data_ptr(),
                                                 b["cap_bases"], b["offs"].data_ptr(), b["cap_reads"], min_qual)
        if nr:
            engine.read_hits_dev(b["packed"].data_ptr(), b["invalid"].data_ptr(), nb, b["offs"].data_ptr(), nr, None, b["rows"].data_ptr())
        return nr, consumed, b["rows"][:nr, 1]

    def extract(f, t, n_text, final, keep, nr, distinct, first):
        """write the records of the chunk whose flag is set; note their ordinals and `distinct`"""
        b = out_room(n_text)
        ob, nk, consumed = engine.fastq_extract_dev(t.data_ptr() if n_text else None, n_text, final, keep.data_ptr() if nr else None, nr,
                                                    b["out"].data_ptr(), b["cap_out"])
        if nk:
            idx = torch.nonzero(keep, as_tuple=False).flatten()
            chosen[f].append(((idx + first).cpu().numpy().astype(np.int64), distinct[idx].cpu().numpy().view(np.uint32)))
            b["host"][:ob].copy_(b["out"][:ob], non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            if sinks[f] is None:                                     # opened at the first write: a refusal before it leaves no file behind
                sinks[f] = open(outs[f], "wb")
            sinks[f].write(memoryview(b["host"].numpy())[:ob])
        kept[f] += nk
        written[f] += ob
        return consumed

    def one_pass(f, t, n_text, final, work):
        nr, consumed, distinct = score(t, n_text, final)
        keep = (distinct >= min_distinct).to(torch.uint8) if min_distinct > 0 else torch.ones(nr, dtype=torch.uint8, device=dev)
        used = extract(f, t, n_text, final, keep, nr, distinct, records[f])
        assert used == consumed, "the feeder and the extract read the same records"
        records[f] += nr
        return consumed

    def pass_1(f, t, n_text, final, work):
        nr, consumed, distinct = score(t, n_text, final)
        if nr:
            scores[f].append(distinct.clone())
        calls[f].append(nr)
        records[f] += nr
        return consumed

    def pass_2(f, t, n_text, final, work):
        # The same file in the same chunks holds the same records per call as in pass 1.  Should the text have changed in
        # between, kdf_fq_extract refuses the call: its n_reads must be the records the chunk holds.
        changed = f"informative_fastq: {files[f]} does not hold the records it held in the first pass: the file changed between the two passes"
        if turn[f] >= len(calls[f]):
            raise ValueError(changed)
        nr = calls[f][turn[f]]
        turn[f] += 1
        try:
            used = extract(f, t, n_text, final, flags[0][done[f]:done[f] + nr], nr, own[f][done[f]:done[f] + nr], done[f])
        except _native.FastqFormatError:
            raise
        except _native.KdfError as ex:
            if ex.code != _native.KDF_ERR_INVALID:
                raise
            raise ValueError(f"{changed} ({ex})") from None
        done[f] += nr
        return used

    passes, chunks, bytes_read, compressed = 0, 0, 0, False
    try:
        if not pair:
            w = _walk_fastq_chunks(engine, files, chunk_bytes, "informative_fastq", one_pass)
            passes, chunks, bytes_read, compressed = 1, w["chunks"], w["bytes"], w["compressed"]
        else:
            w = _walk_fastq_chunks(engine, files, chunk_bytes, "informative_fastq", pass_1)
            if records[0] != records[1]:
                raise ValueError(f"informative_fastq: {files[0]} holds {records[0]} records and {files[1]} holds {records[1]}: a pair has the same number in both")
            own = [torch.cat(s) if s else torch.zeros(0, dtype=torch.int32, device=dev) for s in scores]
            either = torch.maximum(own[0], own[1]) >= min_distinct if min_distinct > 0 else torch.ones(records[0], dtype=torch.bool, device=dev)
            flags[0] = either.to(torch.uint8)
            # The scores and the flags are made on the caller's current stream; pass 2 reads them on the walker's own
            # stream, which nothing orders behind that one: they are complete before pass 2 starts.
            torch.cuda.current_stream(dev).synchronize()
            w2 = _walk_fastq_chunks(engine, files, chunk_bytes, "informative_fastq", pass_2)
            passes, chunks, bytes_read, compressed = 2, w["chunks"] + w2["chunks"], w["bytes"] + w2["bytes"], w["compressed"]
        for i, o in enumerate(outs):                                 # a file of which nothing was kept gets its empty output
            if sinks[i] is None:
                sinks[i] = open(o, "wb")
    finally:
        for s in sinks:
            if s is not None:
                s.close()
    result = []
    for f in range(n_files):
        ords = np.concatenate([c[0] for c in chosen[f]]) if chosen[f] else np.zeros(0, np.int64)
        dist = np.concatenate([c[1] for c in chosen[f]]) if chosen[f] else np.zeros(0, np.uint32)
        result.append({"records": records[f], "kept": kept[f], "ordinals": ords, "distinct": dist})
    LAST_FASTQ_SUBSET = {"files": n_files, "paired": pair, "passes": passes, "chunks": chunks, "bytes_read": bytes_read, "bytes_written": sum(written),
                         "records": sum(records), "kept": sum(kept), "min_distinct": min_distinct, "min_qual": int(min_qual), "compressed": compressed}
    return result


def write_bam_subset(src_bam: str, dst_bam: str, ordinals, aux_fields=None, sort_and_index: bool = True,
                     threads: int = 1) -> int:
    """Copy the records ``ordinals`` (ReadStream.ordinals values) of ``src_bam`` into
    ``dst_bam``; ``aux_fields[i]`` (bytes, BAM-encoded optional fields) is appended to
    record i.  With ``sort_and_index``: coordinate sorted + ``.bai`` (the reference's
    ``pysam.sort`` + ``pysam.index``).  Returns the number of records written."""
    order = np.argsort(np.asarray(ordinals, dtype=np.uint64), kind="stable")
    od = np.ascontiguousarray(np.asarray(ordinals, dtype=np.uint64)[order])
    aux = offs = None
    if aux_fields is not None:
        parts = [bytes(aux_fields[i]) for i in order.tolist()]
        offs = np.zeros(len(parts) + 1, np.uint64)
        if parts:
            offs[1:] = np.cumsum([len(x) for x in parts])
        aux = np.frombuffer(b"".join(parts), np.uint8) if int(offs[-1]) else np.zeros(1, np.uint8)
    nw = c_uint64(0)
    rc = _native.load().kdf_bam_write_subset(src_bam.encode(), dst_bam.encode(), _vp(od), len(od), _vp(aux), _vp(offs),
                                             1 if sort_and_index else 0, threads, byref(nw))
    _native.check_reader(rc, None)
    return nw.value


def fasta_reader(path: str, k: int, max_bases: int = 1 << 26, max_reads: int = 1 << 16,
                 want_meta: bool = False) -> _Reader:
    h = c_void_p()
    rc = _native.load().kdf_fasta_open(path.encode(), int(k), byref(h))
    _native.check_reader(rc, None)
    return _Reader(h, max_bases, max_reads, want_meta)


def kmers_to_keys(kmers: Sequence[str], k: int, canonical: bool = True):
    """K-mer strings -> (lo, hi) uint64 arrays of (canonical) keys; long k (> 64): ((n, W) rows, None)."""
    n = len(kmers)
    raw = np.frombuffer("".join(kmers).encode(), dtype=np.uint8)
    if raw.size != n * k:
        raise ValueError("k-mer of wrong length in input")
    codes = keys.encode(raw.reshape(n, k))
    if (codes > 3).any():
        raise ValueError("non-ACGT base in k-mer")
    return keys.to_pair(keys.from_codes(codes, canonical))


def keys_to_kmers(lo: np.ndarray, hi: Optional[np.ndarray], k: int) -> List[str]:
    flat = keys.to_ascii(keys.from_pair(lo, hi, k), k).tobytes().decode()
    return [flat[i * k:(i + 1) * k] for i in range(len(lo))]
