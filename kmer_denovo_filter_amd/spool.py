"""ReadSpool: Python face of one libkdf read spool (include/kdf.h "read spool").

A spool keeps the batches of a sample's packed read stream resident -- in HBM within ``hbm_budget`` bytes, then in pinned
host memory within ``host_budget`` -- so that every pass after the first (the count pass of a two-pass count, slices
1 .. P-1 of a ``key_parts`` count) is a replay at the device's rate and not another pass through the BAM feeder.  It is an
object of its own: one spool feeds any number of engines on its device.

    with ReadSpool(device, hbm_budget, host_budget) as sp:
        stream_batches_overlapped(engine, readers, filtered=False, tally=True, spool=sp)    # pass 1 also spools
        engine.prefilter_arm()
        sp.replay(engine, ReadSpool.COUNT)                                                  # pass 2 without the BAM

A spool filled with ``keep_reads=True`` (or with offsets) also keeps every batch's read offsets and replays the
per-read consumers -- the same reads against another table without another pass over the BAM:

    with ReadSpool(device, hbm_budget, host_budget) as sp:
        for n, infos in scan_bam_for_hits(bam, engine_a, spool=sp): ...                     # the scan also spools
        rows = sp.read_hits(engine_b)                                                       # (reads, 2): hits, distinct
        keep = sp.select_reads(engine_b, min_distinct=2)                                    # rows stay on the device
        write_bam_subset(bam, out, sp.ordinals[keep])

No CPU fallback: without libkdf.so or without a GPU the constructor raises.
"""
from __future__ import annotations

from ctypes import byref, c_int64, c_uint64, c_void_p
from typing import Optional

import numpy as np

from . import _native
from .reads import stream_words


def _vp(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


class ReadSpool:
    COUNT, COUNT_FILTERED, TALLY = 0, 1, 2           # replay modes

    def __init__(self, device: int = 0, hbm_budget: int = 0, host_budget: int = 0):
        self._lib = _native.load()
        self.device = int(device)
        h = c_void_p()
        _native.check_spool(self._lib.kdf_spool_create(self.device, int(hbm_budget), int(host_budget), byref(h)), None)
        self._h = h
        self._ordinals = []                          # one array per append that kept reads; None: an append brought none
        # True: ``append(stream)`` and the feeders that take ``spool=`` (reads.stream_batches_overlapped,
        # jellyfish_wrappers._stream_bam) hand every batch's read offsets on
        self.keep_reads = False

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.kdf_spool_destroy(self._h)
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
        _native.check_spool(rc, self._h)

    def clear(self):
        """Free every segment and reset the overflow mark (synchronises the device first)."""
        self._ck(self._lib.kdf_spool_clear(self._h))
        self._ordinals = []

    def set_option(self, name: str, value: int):
        self._ck(self._lib.kdf_spool_set_option(self._h, name.encode(), int(value)))

    def stat(self, name: str) -> int:
        v = c_int64(0)
        self._ck(self._lib.kdf_spool_get_stat(self._h, name.encode(), byref(v)))
        return v.value

    # -- append ------------------------------------------------------------
    def _note_ordinals(self, ordinals, n_reads):
        if n_reads == 0 or self._ordinals is None:
            return
        if ordinals is None:
            self._ordinals = None
            return
        o = np.array(ordinals, dtype=np.uint64)
        if len(o) != n_reads:
            raise ValueError(f"{len(o)} ordinals for {n_reads} reads")
        self._ordinals.append(o)

    def _check_ordinals(self, ordinals, n_reads):
        if ordinals is not None and len(ordinals) != n_reads:
            raise ValueError(f"{len(ordinals)} ordinals for {n_reads} reads")

    def append(self, stream_or_packed, invalid=None, n_bases=None, offsets=None, keep_reads: Optional[bool] = None, ordinals=None):
        """One batch from host arrays: a ReadStream, or (packed, invalid, n_bases) uint64 arrays of at least the
        stream_words(n_bases) sizes.  Returns when the arrays may be reused.  ``keep_reads`` (a ReadStream; default:
        the spool's ``keep_reads`` attribute) or
        ``offsets`` (int64[n_reads + 1], starting at 0 and ending at n_bases): the spool keeps the batch's read
        offsets too; the first append decides which kind a spool takes.  ``ordinals`` (default: the stream's, when it
        has them): one value per read, collected in ``self.ordinals``; the spool does not interpret them."""
        if keep_reads is None:
            keep_reads = self.keep_reads and (invalid is None or offsets is not None)
        if invalid is None:
            st = stream_or_packed
            packed, invalid, n_bases = st.packed, st.invalid, st.n_bases
            if keep_reads and offsets is None:
                offsets = st.offsets
                if ordinals is None:
                    ordinals = st.ordinals
        else:
            packed = stream_or_packed
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        invalid = np.ascontiguousarray(invalid, dtype=np.uint64)
        if offsets is None:
            if keep_reads:
                raise ValueError("keep_reads needs a ReadStream or offsets")
            self._ck(self._lib.kdf_spool_append(self._h, _vp(packed), _vp(invalid), int(n_bases)))
            return self
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        self._check_ordinals(ordinals, len(offs) - 1)
        self._ck(self._lib.kdf_spool_append_reads(self._h, _vp(packed), _vp(invalid), int(n_bases), _vp(offs), len(offs) - 1))
        self._note_ordinals(ordinals, len(offs) - 1)
        return self

    def append_dev(self, d_packed: int, d_invalid: int, n_bases: int, hip_stream: int = 0, d_offsets: Optional[int] = None,
                   n_reads: int = 0, ordinals=None):
        """One batch from device buffers (raw pointers), on ``hip_stream`` (0: the null stream); the buffers must be
        complete in that stream's order.  ``d_offsets``: int64[n_reads + 1] on the device -- the spool keeps them (they
        must start at 0, not decrease and end at n_bases: a precondition here, not checked)."""
        st = c_void_p(hip_stream) if hip_stream else None
        if d_offsets is None:
            self._ck(self._lib.kdf_spool_append_dev(self._h, st, c_void_p(d_packed), c_void_p(d_invalid), int(n_bases)))
            return self
        self._check_ordinals(ordinals, int(n_reads))
        self._ck(self._lib.kdf_spool_append_reads_dev(self._h, st, c_void_p(d_packed), c_void_p(d_invalid), int(n_bases),
                                                      c_void_p(d_offsets), int(n_reads)))
        self._note_ordinals(ordinals, int(n_reads))
        return self

    def append_uploaded(self, engine, slot: int, offsets=None, ordinals=None):
        """The batch upload slot ``slot`` of ``engine`` holds (engine.upload_async); the slot keeps it: count or tally
        it afterwards as usual.  ``offsets``: the batch's read offsets (host int64[n_reads + 1]), kept with it."""
        if offsets is None:
            self._ck(self._lib.kdf_spool_append_uploaded(self._h, engine._h, int(slot)))
            return self
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        self._check_ordinals(ordinals, len(offs) - 1)
        self._ck(self._lib.kdf_spool_append_uploaded_reads(self._h, engine._h, int(slot), _vp(offs), len(offs) - 1))
        self._note_ordinals(ordinals, len(offs) - 1)
        return self

    # -- replay / read back ------------------------------------------------
    def replay(self, engine, mode: int = 0):
        """Every segment, in order, into ``engine``: mode 0 count, 1 count --if, 2 prefilter tally.  The engine's own
        state rules apply; the spool is not changed."""
        self._ck(self._lib.kdf_spool_replay(self._h, engine._h, int(mode)))
        return self

    def sketch(self, engine):
        """Every segment, in order, into the distinct k-mer sketch of ``engine`` (engine.sketch_begin first); the spool
        and the engine's table, mode and upload slots are not changed."""
        self._ck(self._lib.kdf_spool_sketch(self._h, engine._h))
        return self

    def read_segment(self, seg: int):
        """(packed, invalid, n_positions) of one segment as host arrays of the stream_words(n_positions) sizes."""
        n = c_uint64(0)
        self._ck(self._lib.kdf_spool_read_segment(self._h, int(seg), None, None, byref(n)))
        pw, mw = stream_words(n.value)
        packed, invalid = np.empty(pw, np.uint64), np.empty(mw, np.uint64)
        self._ck(self._lib.kdf_spool_read_segment(self._h, int(seg), _vp(packed), _vp(invalid), byref(n)))
        return packed, invalid, n.value

    # -- reads -------------------------------------------------------------
    @property
    def n_reads(self) -> int:
        return self.stat("reads")

    @property
    def ordinals(self) -> Optional[np.ndarray]:
        """The ``ordinals`` of every append, concatenated in read order (uint64[n_reads]); None when an append that
        kept reads brought none."""
        if self._ordinals is None:
            return None
        return np.concatenate(self._ordinals) if self._ordinals else np.zeros(0, np.uint64)

    def read_offsets(self, seg: int):
        """(offsets int64[n_reads + 1] in segment coordinates, first_read, n_reads) of one segment."""
        first, n = c_uint64(0), c_uint64(0)
        self._ck(self._lib.kdf_spool_read_offsets(self._h, int(seg), None, byref(first), byref(n)))
        offs = np.empty(n.value + 1, np.int64)
        self._ck(self._lib.kdf_spool_read_offsets(self._h, int(seg), _vp(offs), byref(first), byref(n)))
        return offs, first.value, n.value

    def segment_dev(self, seg: int):
        """Device pointers of an HBM-tier segment: (d_packed, d_invalid, n_positions, d_offsets or None, first_read,
        n_reads), for the engine's ``_dev`` methods.  Waits for the last append; a host-tier segment raises."""
        dp, dm, do = c_void_p(), c_void_p(), c_void_p()
        n, first, nr = c_uint64(0), c_uint64(0), c_uint64(0)
        self._ck(self._lib.kdf_spool_segment_dev(self._h, int(seg), byref(dp), byref(dm), byref(n), byref(do), byref(first), byref(nr)))
        return dp.value, dm.value, n.value, do.value, first.value, nr.value

    def _rows_dev(self, words_per_read: int):
        """Result rows on the device.  Not zeroed -- the entry points write every row themselves -- and the device is
        synchronised before they are handed out: torch allocates on its own stream, the engine writes on another."""
        import torch
        dev = torch.device("cuda", self.device)
        rows = torch.empty(max(self.n_reads * words_per_read, 1), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        return rows

    def read_hits_dev(self, engine, d_rows: int):
        """``engine.read_hits`` of every spooled read into a device buffer of n_reads x 2 uint32, in append order."""
        self._ck(self._lib.kdf_spool_read_hits(self._h, engine._h, c_void_p(d_rows) if d_rows else None))

    def read_depth_dev(self, engine, low_max: int, d_rows: int):
        """``engine.read_depth`` of every spooled read into a device buffer of n_reads x 6 uint64."""
        self._ck(self._lib.kdf_spool_read_depth(self._h, engine._h, int(low_max), c_void_p(d_rows) if d_rows else None))

    def read_hits(self, engine) -> np.ndarray:
        """uint32 (n_reads, 2), columns ``engine.READ_HITS_COLUMNS``: what ``engine.read_hits`` returns for each
        appended batch, stacked in append order."""
        nr = self.n_reads
        rows = self._rows_dev(1)
        self.read_hits_dev(engine, rows.data_ptr())
        engine.synchronize()
        return rows[:nr].cpu().numpy().view(np.uint32).reshape(nr, 2)

    def read_depth(self, engine, low_max: int = 0) -> np.ndarray:
        """uint64 (n_reads, 6), columns ``engine.READ_DEPTH_COLUMNS``, as ``engine.read_depth`` batch by batch."""
        if not 0 <= int(low_max) <= 0xFFFFFFFF:
            raise ValueError(f"low_max={low_max} outside 0..2^32 - 1")
        nr = self.n_reads
        rows = self._rows_dev(6)
        self.read_depth_dev(engine, int(low_max), rows.data_ptr())
        engine.synchronize()
        return rows[:nr * 6].cpu().numpy().view(np.uint64).reshape(nr, 6)

    def select_reads_dev(self, d_hit_rows: int, min_distinct: int, d_reads: Optional[int], cap: int):
        """-> (rc, n): the raw call.  ``d_hit_rows`` must be complete (``engine.synchronize()``)."""
        n = c_uint64(0)
        rc = self._lib.kdf_spool_select_reads(self._h, c_void_p(d_hit_rows) if d_hit_rows else None, int(min_distinct),
                                              c_void_p(d_reads) if d_reads else None, int(cap), byref(n))
        return rc, n.value

    def select_reads(self, engine, min_distinct: int = 1) -> np.ndarray:
        """Ascending global indices (int64) of the spooled reads with at least ``min_distinct`` distinct hit k-mers in
        ``engine``'s table: Module 3's selection.  The per-read rows stay on the device; only the list comes back."""
        import torch
        if not 0 <= int(min_distinct) <= 0xFFFFFFFF:
            raise ValueError(f"min_distinct={min_distinct} outside 0..2^32 - 1")
        rows = self._rows_dev(1)
        self.read_hits_dev(engine, rows.data_ptr())
        engine.synchronize()
        rc, n = self.select_reads_dev(rows.data_ptr(), min_distinct, None, 0)         # the count alone
        if n == 0:
            self._ck(rc)
            return np.zeros(0, np.int64)
        out = torch.empty(n, dtype=torch.int64, device=rows.device)
        torch.cuda.synchronize(rows.device)
        rc, n = self.select_reads_dev(rows.data_ptr(), min_distinct, out.data_ptr(), n)
        self._ck(rc)
        return out[:n].cpu().numpy()
