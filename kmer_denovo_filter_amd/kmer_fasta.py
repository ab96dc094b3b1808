"""The reference's intermediate k-mer file format ``>{i}\\n{KMER}\\n``
(utils.py:150-170, core/bam_scanner.py:34-46; written inline at
discovery/pipeline.py:221-226,297-304,523-532,573-583), vectorised, plus a
binary sidecar so that stages running on the engine skip the text round trip.

The FASTA stays the contract (callers and users may read it); the sidecar
``<path>.kdfkeys.npz`` is only trusted when it records the FASTA's exact size and
mtime.

Long k-mers (odd k from 65 to 201) use the engine's long-key form: keys are
``(n, W)`` uint64 rows (W = ceil(2k/64), word 0 least significant) in the ``lo``
position and ``hi`` is None.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np

from . import keys

_CHUNK = 1 << 22


def _sidecar(path: str) -> str:
    return path + ".kdfkeys.npz"


def write_kmer_fasta(path: str, lo: np.ndarray, hi: Optional[np.ndarray], k: int,
                     sidecar: bool = True) -> int:
    """Write keys as ``>{i}\\n{KMER}\\n`` (i from 0).  Returns the number written.  Long k: ``lo`` = (n, W) rows."""
    words = keys.from_pair(lo, hi, k)
    n = len(words[0])
    with open(path, "wb") as fh:
        for a in range(0, n, _CHUNK):
            b = min(n, a + _CHUNK)
            seqs = keys.to_ascii([w[a:b] for w in words], k)
            idx = np.arange(a, b, dtype=np.int64)
            ndig = np.ones(b - a, dtype=np.int64)
            t = idx // 10
            while t.any():
                ndig += (t > 0)
                t //= 10
            for d in np.unique(ndig):
                sel = np.flatnonzero(ndig == d)          # contiguous run: indices are increasing
                m = len(sel)
                line = np.empty((m, 1 + d + 1 + k + 1), dtype=np.uint8)
                line[:, 0] = ord(">")
                v = idx[sel].copy()
                for j in range(d - 1, -1, -1):
                    line[:, 1 + j] = (v % 10) + ord("0")
                    v //= 10
                line[:, 1 + d] = 10
                line[:, 2 + d:2 + d + k] = seqs[sel]
                line[:, -1] = 10
                fh.write(line.tobytes())
    if sidecar:
        st = os.stat(path)
        lo, hi = keys.to_pair(words)
        hi = np.zeros(0, np.uint64) if hi is None else hi    # (long keys: unused; keeps the sidecar's fields)
        np.savez(_sidecar(path), lo=lo, hi=hi, k=np.int64(k), size=np.int64(st.st_size),
                 mtime_ns=np.int64(st.st_mtime_ns))
    return n


def read_kmer_fasta_keys(path: str, k: int, canonical: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """Sequence lines of a k-mer FASTA -> (lo, hi) keys, file order (long k: ((n, W) rows, None)).

    With ``canonical`` the keys are canonicalised, as Jellyfish does with an
    ``--if`` / ``query -s`` file under ``-C``.
    """
    sc = _sidecar(path)
    if os.path.exists(sc):
        try:
            z = np.load(sc)
            st = os.stat(path)
            if int(z["k"]) == k and int(z["size"]) == st.st_size and int(z["mtime_ns"]) == st.st_mtime_ns:
                return keys.to_pair(keys.from_pair(z["lo"], z["hi"], k))
        except Exception:  # noqa: BLE001  (stale or unreadable sidecar: fall back to the text)
            pass
    data = np.fromfile(path, dtype=np.uint8)
    if data.size and data[-1] != 10:
        data = np.append(data, np.uint8(10))
    nl = np.flatnonzero(data == 10)
    starts = np.zeros_like(nl)
    starts[1:] = nl[:-1] + 1
    lens = nl - starts
    # strip one trailing \r if present
    cr = (lens > 0) & (data[np.maximum(nl - 1, 0)] == 13)
    lens = lens - cr
    is_seq = (lens > 0) & (data[starts] != ord(">"))
    s, ln = starts[is_seq], lens[is_seq]
    if not (ln == k).all():
        raise ValueError(f"{path}: sequence line of length != k={k}")
    codes = keys.encode(data[s[:, None] + np.arange(k)[None, :]])
    if (codes > 3).any():
        raise ValueError(f"{path}: non-ACGT base in k-mer FASTA")
    return keys.to_pair(keys.from_codes(codes, canonical))


def remove_with_sidecar(path: str):
    for p in (path, _sidecar(path)):
        if os.path.exists(p):
            os.remove(p)


# ---- the same two on the device (KmerEngine.format_kmers_dev / parse_kmer_fasta_dev) ------------------------------------
# KDF_DEVICE_FASTA=1 sends the mirrors' writers and unregistered-path readers of these files here; the host functions
# above stay the default and the specification.  LAST_FASTA_CODEC: which codec the last such read or write took.
LAST_FASTA_CODEC: Optional[str] = None

_codec_engines = {}           # device -> a small KmerEngine kept for the codec (its table is never used)
_pinned = {}                  # window bytes -> reads.PinnedBytes of two buffers, kept for the life of the process


def device_fasta() -> bool:
    """The switch ``KDF_DEVICE_FASTA=1`` (default off)."""
    return os.environ.get("KDF_DEVICE_FASTA") == "1"


def codec_engine(device: int = 0):
    """The engine the device codec runs on when the caller names none: the codec takes any k on any engine, and an
    engine of its own leaves the counting engines' streams and pending work alone."""
    eng = _codec_engines.get(device)
    if eng is None or not getattr(eng, "_h", None):
        from .engine import KmerEngine
        eng = _codec_engines[device] = KmerEngine(31, 1 << 10, device)
    return eng


def store_kmer_set(path: str, k: int, dev=None, host=None, device: int = 0) -> int:
    """The mirrors' writer of a contract file, for a set held in HBM (``dev``: (lo, hi) tensors), on the host (``host``:
    (lo, hi) arrays) or both: ``write_kmer_fasta`` over the host arrays (taken from ``dev`` when not given), or under
    ``KDF_DEVICE_FASTA=1`` ``write_kmer_fasta_device`` over the device tensors (uploaded when not given).  The same
    file and sidecar either way.  Returns the number written."""
    global LAST_FASTA_CODEC
    from . import devkeys
    if device_fasta():
        if dev is None:
            dev = devkeys.from_host(host[0], host[1], keys.n_words(k) == 2, device)
        return write_kmer_fasta_device(path, dev[0], dev[1], k)
    lo, hi = host if host is not None else devkeys.to_host(*dev)
    n = write_kmer_fasta(path, lo, hi, k)
    LAST_FASTA_CODEC = "host"
    return n


def load_kmer_set(path: str, k: int, canonical: bool = True, device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The mirrors' reader of a k-mer FASTA whose set is not in HBM, for callers that want host arrays:
    ``read_kmer_fasta_keys``, or under ``KDF_DEVICE_FASTA=1`` the device reader's keys brought to the host (the same
    arrays)."""
    global LAST_FASTA_CODEC
    if device_fasta():
        from . import devkeys
        return devkeys.to_host(*read_kmer_fasta_keys_device(path, k, canonical, device=device))
    out = read_kmer_fasta_keys(path, k, canonical)
    LAST_FASTA_CODEC = "host"
    return out


def _window_bytes() -> int:
    """Bytes of one window of text in flight: ``KDF_FASTA_CHUNK_MB`` MiB (default 64, at least 1)."""
    try:
        mb = int(os.environ.get("KDF_FASTA_CHUNK_MB", "") or 64)
    except ValueError:
        mb = 64
    return max(1, mb) << 20


def _pinned_pair(nbytes: int):
    from .reads import PinnedBytes
    pb = _pinned.get(nbytes)
    if pb is None or not pb.buffers:
        for old in _pinned.values():
            old.close()
        _pinned.clear()
        pb = _pinned[nbytes] = PinnedBytes(2, nbytes)
    return pb.buffers


def write_kmer_fasta_device(path: str, dlo, dhi, k: int, engine=None, first_index: int = 0, sidecar: bool = True) -> int:
    """``write_kmer_fasta`` for keys in device memory (``devkeys`` form: int64 CUDA tensors, hi None unless k is 33..63,
    long k: (n, W) rows): the text is formatted on the device window by window (``KmerEngine.format_kmers_dev``) into one
    device buffer and copied to two page-locked buffers in turn, so that the copy of window i + 1 runs while ``write()``
    takes window i.  Records are numbered from ``first_index``.  The file is byte-identical to ``write_kmer_fasta``'s (for
    ``first_index`` 0) and so is the sidecar.  Returns the number written."""
    import torch
    from .engine import TEXT_FASTA
    global LAST_FASTA_CODEC
    n = int(dlo.shape[0])
    dev = dlo.device
    eng = engine if engine is not None else codec_engine(dev.index or 0)
    total = eng.kmer_text_bytes(k, TEXT_FASTA, first_index, n)
    if n and not total:
        raise ValueError(f"{path}: no k-mer text for k={k}, records {first_index} + {n}")
    win = _window_bytes()
    dlo = dlo.contiguous()
    dhi = dhi.contiguous() if dhi is not None and 33 <= int(k) <= 63 else None
    with open(path, "wb") as fh:
        if total:
            pinned = _pinned_pair(win)
            dbuf = torch.empty(min(win, total), dtype=torch.uint8, device=dev)
            stream = torch.cuda.Stream(dev)
            stream.wait_stream(torch.cuda.current_stream(dev))             # (the keys were written on the caller's stream)
            eng.set_stream(stream.cuda_stream)
            try:
                windows = [(a, min(win, total - a)) for a in range(0, total, win)]
                done = [None, None]

                def issue(i):
                    a, m = windows[i]
                    eng.format_kmers_dev(dlo.data_ptr(), dhi.data_ptr() if dhi is not None else None, n, k, TEXT_FASTA, first_index,
                                         a, m, dbuf.data_ptr())
                    with torch.cuda.stream(stream):
                        torch.from_numpy(pinned[i & 1][:m]).copy_(dbuf[:m], non_blocking=True)
                        done[i & 1] = torch.cuda.Event()
                        done[i & 1].record(stream)

                issue(0)
                for i, (a, m) in enumerate(windows):
                    done[i & 1].synchronize()
                    if i + 1 < len(windows):
                        issue(i + 1)                                       # (format and copy run while this window is written)
                    fh.write(memoryview(pinned[i & 1][:m]))
                stream.synchronize()
            finally:
                eng.set_stream(None)
    if sidecar:
        from . import devkeys
        st = os.stat(path)
        lo, hi = keys.to_pair(keys.from_pair(*devkeys.to_host(dlo, dhi), k))
        hi = np.zeros(0, np.uint64) if hi is None else hi
        np.savez(_sidecar(path), lo=lo, hi=hi, k=np.int64(k), size=np.int64(st.st_size), mtime_ns=np.int64(st.st_mtime_ns))
    LAST_FASTA_CODEC = "device"
    return n


def read_kmer_fasta_keys_device(path: str, k: int, canonical: bool = True, engine=None, device: int = 0):
    """``read_kmer_fasta_keys`` into device memory: -> (lo, hi) int64 CUDA tensors in ``devkeys`` form (hi None unless k
    is 33..63; long k: ((n, W) rows, None)).  A valid sidecar is honoured first; otherwise the file goes chunk by chunk
    through two page-locked buffers to ``KmerEngine.parse_kmer_fasta_dev``, the unfinished last line of a chunk in front
    of the next.  Raises ValueError with the host function's messages."""
    import torch
    from . import devkeys
    global LAST_FASTA_CODEC
    W = keys.n_words(k)
    sc = _sidecar(path)
    if os.path.exists(sc):
        try:
            z = np.load(sc)
            st = os.stat(path)
            if int(z["k"]) == k and int(z["size"]) == st.st_size and int(z["mtime_ns"]) == st.st_mtime_ns:
                LAST_FASTA_CODEC = "sidecar"
                return devkeys.from_host(*keys.to_pair(keys.from_pair(z["lo"], z["hi"], k)), wide=W == 2, device=device)
        except Exception:  # noqa: BLE001  (stale or unreadable sidecar: fall back to the text)
            pass
    dev = torch.device("cuda", device)
    eng = engine if engine is not None else codec_engine(device)
    win = _window_bytes()
    pinned = _pinned_pair(win)
    dtext = torch.empty(win, dtype=torch.uint8, device=dev)
    cap = win // (k + 1) + 1                                              # a sequence line takes k + 1 bytes at least
    parts = []
    have, which, in_header, eof = 0, 0, False, False                     # bytes of buf that wait; a header longer than a window is being skipped
    with open(path, "rb", buffering=0) as fh:
        while not eof:
            buf = pinned[which]
            while have < win:                                            # fill the window (short reads: pipes, network files)
                got = fh.readinto(memoryview(buf[have:]))
                if not got:
                    eof = True
                    break
                have += got
            if in_header:                                                # up to the header's '\n': nothing to parse
                nl = np.flatnonzero(buf[:have] == 10)
                if not len(nl):
                    have = 0
                    continue
                rest = have - int(nl[0]) - 1
                buf[:rest] = buf[int(nl[0]) + 1:have].copy()
                have, in_header = rest, False
                if not eof:
                    continue
            if have == 0:
                break
            dtext[:have].copy_(torch.from_numpy(buf[:have]), non_blocking=True)
            lo = torch.empty((cap, W) if W > 2 else cap, dtype=torch.int64, device=dev)
            hi = torch.empty(cap, dtype=torch.int64, device=dev) if W == 2 else None
            torch.cuda.current_stream(dev).synchronize()
            try:
                m, consumed = eng.parse_kmer_fasta_dev(dtext.data_ptr(), have, k, canonical, eof, lo.data_ptr(),
                                                       hi.data_ptr() if hi is not None else None, cap)
            except ValueError as e:                                      # (KmerFastaError: the first bad line's rule)
                if getattr(e, "rule", "") == "base":
                    raise ValueError(f"{path}: non-ACGT base in k-mer FASTA") from None
                raise ValueError(f"{path}: sequence line of length != k={k}") from None
            if m:
                parts.append((lo[:m], hi[:m] if hi is not None else None))
            if consumed == 0 and have == win and not eof:                # one line fills the window
                if buf[0] != ord(">"):
                    raise ValueError(f"{path}: sequence line of length != k={k}")
                have, in_header = 0, True
                continue
            nxt = pinned[which ^ 1]
            nxt[:have - consumed] = buf[consumed:have]
            have, which = have - consumed, which ^ 1
    LAST_FASTA_CODEC = "device"
    if not parts:
        empty = torch.empty((0, W) if W > 2 else 0, dtype=torch.int64, device=dev)
        return empty, (torch.empty(0, dtype=torch.int64, device=dev) if W == 2 else None)
    return devkeys.select(parts)
