"""ReadSpool: Python face of one libkdf read spool (include/kdf.h "read spool").

A spool keeps the batches of a sample's packed read stream resident -- in HBM within ``hbm_budget`` bytes, then in pinned
host memory within ``host_budget`` -- so that every pass after the first (the count pass of a two-pass count, slices
1 .. P-1 of a ``key_parts`` count) is a replay at the device's rate and not another pass through the BAM feeder.  It is an
object of its own: one spool feeds any number of engines on its device.

    with ReadSpool(device, hbm_budget, host_budget) as sp:
        stream_batches_overlapped(engine, readers, filtered=False, tally=True, spool=sp)    # pass 1 also spools
        engine.prefilter_arm()
        sp.replay(engine, ReadSpool.COUNT)                                                  # pass 2 without the BAM

No CPU fallback: without libkdf.so or without a GPU the constructor raises.
"""
from __future__ import annotations

from ctypes import byref, c_int64, c_uint64, c_void_p

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

    def set_option(self, name: str, value: int):
        self._ck(self._lib.kdf_spool_set_option(self._h, name.encode(), int(value)))

    def stat(self, name: str) -> int:
        v = c_int64(0)
        self._ck(self._lib.kdf_spool_get_stat(self._h, name.encode(), byref(v)))
        return v.value

    # -- append ------------------------------------------------------------
    def append(self, stream_or_packed, invalid=None, n_bases=None):
        """One batch from host arrays: a ReadStream, or (packed, invalid, n_bases) uint64 arrays of at least the
        stream_words(n_bases) sizes.  Returns when the arrays may be reused."""
        if invalid is None:
            packed, invalid, n_bases = stream_or_packed.packed, stream_or_packed.invalid, stream_or_packed.n_bases
        else:
            packed = stream_or_packed
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        invalid = np.ascontiguousarray(invalid, dtype=np.uint64)
        self._ck(self._lib.kdf_spool_append(self._h, _vp(packed), _vp(invalid), int(n_bases)))
        return self

    def append_dev(self, d_packed: int, d_invalid: int, n_bases: int, hip_stream: int = 0):
        """One batch from device buffers (raw pointers), on ``hip_stream`` (0: the null stream); the buffers must be
        complete in that stream's order."""
        self._ck(self._lib.kdf_spool_append_dev(self._h, c_void_p(hip_stream) if hip_stream else None,
                                                c_void_p(d_packed), c_void_p(d_invalid), int(n_bases)))
        return self

    def append_uploaded(self, engine, slot: int):
        """The batch upload slot ``slot`` of ``engine`` holds (engine.upload_async); the slot keeps it: count or tally
        it afterwards as usual."""
        self._ck(self._lib.kdf_spool_append_uploaded(self._h, engine._h, int(slot)))
        return self

    # -- replay / read back ------------------------------------------------
    def replay(self, engine, mode: int = 0):
        """Every segment, in order, into ``engine``: mode 0 count, 1 count --if, 2 prefilter tally.  The engine's own
        state rules apply; the spool is not changed."""
        self._ck(self._lib.kdf_spool_replay(self._h, engine._h, int(mode)))
        return self

    def read_segment(self, seg: int):
        """(packed, invalid, n_positions) of one segment as host arrays of the stream_words(n_positions) sizes."""
        n = c_uint64(0)
        self._ck(self._lib.kdf_spool_read_segment(self._h, int(seg), None, None, byref(n)))
        pw, mw = stream_words(n.value)
        packed, invalid = np.empty(pw, np.uint64), np.empty(mw, np.uint64)
        self._ck(self._lib.kdf_spool_read_segment(self._h, int(seg), _vp(packed), _vp(invalid), byref(n)))
        return packed, invalid, n.value
