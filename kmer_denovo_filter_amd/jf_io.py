"""On-disk k-mer indexes (the ``.jf`` files the reference passes between stages).

Reader: real Jellyfish ``binary/sorted`` files -- the format of ``--ref-jf`` /
``{ref}.k{k}.jf`` (core/jellyfish_wrappers.py:299-304) -- and this package's own
``kdf/sorted`` files.  Both share the container Jellyfish uses (SURVEY.md
section 0.5): 9 ASCII digits = byte length of the JSON header including its NUL
padding, the JSON header, then fixed records of ceil(key_len/8) key bytes (LE)
+ counter_len count bytes (LE).

Writers: ``kdf/sorted`` (records in ascending key order: ``write_index``, what
the mirrors write by default) and Jellyfish's own ``binary/sorted``
(``write_jellyfish_index``: records in the order of their hash position under the
header's GF(2) matrix -- position = XOR of ``matrix1.columns[i]`` over the set bits
``key_len - 1 - i`` of the key, ties in ascending key order).  That rule is pinned
by the reference's real Jellyfish file (tests/golden/giab/mini_ref.fa.k31.jf:
its 45 275 records are in exactly that order, and re-writing them from a shuffled
copy under its matrix gives the same bytes, tests/test_jf_helpers.py); that a real
``jellyfish query`` accepts a header generated HERE is unverified -- there is no
Jellyfish in this image.  ``KDF_JF_FORMAT=jellyfish``
makes the mirrors write ``{ref}.k{k}.jf`` that way.

Long k-mers (odd k from 65 to 201): records of ceil(2k/8) key bytes, and keys as
``(n, W)`` uint64 rows (W = ceil(2k/64), word 0 least significant) in the ``lo``
position with ``hi = None`` -- what a long KmerEngine takes and returns.  A real
Jellyfish ``binary/sorted`` file at k > 63 is read with the same byte layout
(little-endian key bytes, as at k <= 63); no such fixture exists, so that reading
is unpinned.  ``write_jellyfish_index`` refuses k > 63.

The record codec also runs on the device (``write_index_device``, ``write_jellyfish_index_device``,
``load_index_into_device``, ``read_index_device``, below): opt-in with ``KDF_DEVICE_INDEX=1``; the host functions stay
the default and the specification.
"""
from __future__ import annotations

import json
import os
from typing import Optional, Tuple

import numpy as np

from . import keys

KDF_FORMAT = "kdf/sorted"
JF_FORMAT = "binary/sorted"


def read_header(path: str) -> Tuple[dict, int]:
    with open(path, "rb") as fh:
        head = fh.read(9)
        if len(head) < 9 or not head.isdigit():
            raise ValueError(f"{path}: not a Jellyfish/kdf index (bad length prefix)")
        hlen = int(head)
        raw = fh.read(hlen)
    if len(raw) < hlen:
        raise ValueError(f"{path}: truncated index header")
    header = json.loads(raw.rstrip(b"\0").decode())
    return header, 9 + hlen


def _index_layout(path: str, expect_k: Optional[int]):
    header, off = read_header(path)
    fmt = header.get("format")
    if fmt not in (JF_FORMAT, KDF_FORMAT):
        raise ValueError(f"{path}: unsupported index format {fmt!r} (only {JF_FORMAT!r} and {KDF_FORMAT!r})")
    if fmt == JF_FORMAT and not header.get("canonical", False):
        raise ValueError(f"{path}: Jellyfish index was not built with -C (canonical)")
    key_len = int(header["key_len"])
    if key_len % 2:
        raise ValueError(f"{path}: odd key_len {key_len}")
    k = key_len // 2
    if expect_k is not None and k != expect_k:
        raise ValueError(f"{path}: index has k={k}, expected k={expect_k}")
    if k > 64 and not (k <= 201 and k % 2 == 1):
        raise ValueError(f"{path}: k={k} is beyond the engine's key width (1..63, odd 65..201)")
    kb, cb = (key_len + 7) // 8, int(header["counter_len"])
    rec = np.dtype([("k", "u1", (kb,)), ("c", "u1", (cb,))])
    n = (os.path.getsize(path) - off) // rec.itemsize
    return k, kb, cb, rec, off, n


def index_records(path: str) -> int:
    """Number of records of an index (from the file size; nothing is read)."""
    return _index_layout(path, None)[5]


def _decode(data, kb: int, cb: int):
    """One block of records -> (lo, hi or None, counts uint32).  Little-endian byte strings of any length up to 16 / 8
    bytes; the usual widths (8-byte keys, 4-byte counters) are plain views of one contiguous copy per field.  Keys of
    more than 16 bytes (long k-mers) come back as (n, W) uint64 rows in the lo position, hi = None."""
    n = len(data)
    lo, hi = keys.to_pair(keys.from_bytes(np.ascontiguousarray(data["k"])), zero_hi=False)
    craw = np.ascontiguousarray(data["c"])
    if cb == 4:
        counts = craw.view("<u4").reshape(n)
    else:
        cbytes = np.zeros((n, 8), dtype=np.uint8)
        cbytes[:, :min(cb, 8)] = craw[:, :8]
        c64 = cbytes.view("<u8").reshape(n)
        if cb > 8:
            c64 = np.where(craw[:, 8:].any(axis=1), np.uint64(0xFFFFFFFFFFFFFFFF), c64)
        counts = np.minimum(c64, np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return lo, hi, counts


def iter_index(path: str, expect_k: Optional[int] = None, chunk_records: int = 1 << 24, part: int = 0, parts: int = 1):
    """Yield (k, lo, hi or None, counts) blocks of at most ``chunk_records`` records.  The file is memory-mapped and
    decoded block by block, so a whole-genome index (2.5e9 records, 30 GB on disk) needs ~0.5 GB of host memory at a
    time where `read_index` would need every record decoded at once (Jellyfish itself mmaps the file,
    reference discovery/pipeline.py:286-288)."""
    k, kb, cb, rec, off, n = _index_layout(path, expect_k)
    if n == 0:
        return
    mm = np.memmap(path, dtype=rec, mode="r", offset=off, shape=(n,))
    first, last = n * part // parts, n * (part + 1) // parts      # this part's records (one rank's share of the index)
    try:
        for a in range(first, last, chunk_records):
            lo, hi, counts = _decode(mm[a:min(a + chunk_records, last)], kb, cb)
            yield k, lo, hi, counts
    finally:
        del mm


def load_index_into(engine, path: str, expect_k: Optional[int] = None, chunk_records: int = 1 << 24,
                    part: int = 0, parts: int = 1) -> int:
    """Stream an index into ``engine``'s table (`jellyfish query`'s view of the .jf): the table is sized once for the
    record count, then the blocks are added one by one.  ``part`` of ``parts``: only that share of the records (the
    index sharded over the ranks of a multi-GPU job).  Returns the number of records of the whole index."""
    global LAST_INDEX_CODEC
    if device_index():
        return load_index_into_device(engine, path, expect_k, part, parts)
    k, _, _, _, _, n = _index_layout(path, expect_k)
    if k != engine.k:
        raise ValueError(f"{path}: index has k={k}, the engine counts k={engine.k}")
    if n:
        engine.reserve(max(1, n // parts + 1))
    for _, lo, hi, counts in iter_index(path, expect_k, chunk_records, part, parts):
        engine.add_pairs(lo, hi, counts)
    LAST_INDEX_CODEC = "host"
    return n


def read_index(path: str, expect_k: Optional[int] = None):
    """-> (k, lo, hi, counts) ; hi is all zero for k <= 32; long k: lo = (n, W) rows, hi = None.  Counts saturate at
    2^32-1.  Whole file in memory: callers that only feed an engine use `load_index_into`."""
    k = _index_layout(path, expect_k)[0]
    blocks = [b[1:] for b in iter_index(path, expect_k)] or [(np.zeros(0, np.uint64), None, np.zeros(0, np.uint32))]
    lo, hi, counts = (None if b[0] is None else np.concatenate(b) for b in zip(*blocks))
    return (k, *keys.to_pair(keys.from_pair(lo, hi, k)), counts)


def index_histogram(path: str, high: int = 10000, expect_k: Optional[int] = None,
                    chunk_records: int = 1 << 24) -> np.ndarray:
    """`jellyfish histo -h high file.jf` of an index FILE (``binary/sorted`` or ``kdf/sorted``, any k), on the host:
    uint64[high + 2], bins[c] = records whose count is exactly c, bins[high + 1] = records with a count above
    ``high`` -- the layout of ``KmerEngine.histogram`` (bins[0]: records stored with count 0).  Memory-mapped and
    decoded block by block through `iter_index`; an index is already a compact (key, count) list, so no device."""
    high = int(high)
    if high < 0:
        raise ValueError(f"high={high} must be >= 0")
    bins = np.zeros(high + 2, np.uint64)
    for _, _, _, counts in iter_index(path, expect_k, chunk_records):
        c = np.minimum(counts, np.uint32(min(high + 1, 0xFFFFFFFF))).astype(np.int64)
        bins += np.bincount(c, minlength=high + 2)[:high + 2].astype(np.uint64)
    return bins


def index_stats(path: str, expect_k: Optional[int] = None, chunk_records: int = 1 << 24) -> dict:
    """`jellyfish stats file.jf`: {"unique": records with count 1, "distinct": records with count >= 1, "total":
    sum of all counts (as stored: saturated at 2^32 - 1), "max_count": largest count, 0 for an empty index}."""
    unique = distinct = total = mx = 0
    for _, _, _, counts in iter_index(path, expect_k, chunk_records):
        unique += int(np.count_nonzero(counts == 1))
        distinct += int(np.count_nonzero(counts))
        total += int(counts.sum(dtype=np.uint64))
        mx = max(mx, int(counts.max()) if len(counts) else 0)
    return {"unique": unique, "distinct": distinct, "total": total, "max_count": mx}


def _header_bytes(header: dict) -> bytes:
    """The bytes in front of the records: 9 ASCII digits, the JSON header, NUL padding to a multiple of 8."""
    body = json.dumps(header).encode()
    body += b"\0" * ((-(9 + len(body))) % 8)
    return b"%09d" % len(body) + body


def _kdf_header(k: int, n: int, cmdline=None) -> dict:
    """The header of a ``kdf/sorted`` index of ``n`` records (shared by ``write_index`` and ``write_index_device``)."""
    return {
        "alignment": 8, "canonical": True, "cmdline": list(cmdline or []), "counter_len": 4,
        "format": KDF_FORMAT, "key_len": 2 * k, "size": int(n),
        "exe_path": "kmer_denovo_filter_amd (libkdf.so)",
    }


def write_index(path: str, k: int, lo: np.ndarray, hi: Optional[np.ndarray], counts: np.ndarray,
                cmdline=None) -> str:
    """Write a ``kdf/sorted`` index (keys must already be in ascending order; long k: ``lo`` = (n, W) rows)."""
    kbytes = keys.to_bytes(keys.from_pair(lo, hi, k), k)
    n, kb = kbytes.shape
    rec = np.dtype([("k", "u1", (kb,)), ("c", "<u4")])
    data = np.zeros(n, dtype=rec)
    data["k"] = kbytes
    data["c"] = np.asarray(counts, dtype=np.uint32)
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(_header_bytes(_kdf_header(k, n, cmdline)))
        data.tofile(fh)
    os.replace(tmp, path)
    return path


# ---------------------------------------------------------------------------
# Jellyfish's own binary/sorted files
def jf_reprobes(max_reprobe: int = 126):
    """The reprobe offsets a Jellyfish 2 header lists (the fixture's: 1, then the triangular numbers)."""
    return [1] + [i * (i + 1) // 2 for i in range(1, max_reprobe + 1)]


def _gf2_rank(cols, r: int) -> int:
    rows = [int(c) for c in cols]                       # (column vectors of r bits: rank of the set)
    rank = 0
    for bit in range(r):
        piv = next((j for j in range(rank, len(rows)) if (rows[j] >> bit) & 1), None)
        if piv is None:
            continue
        rows[rank], rows[piv] = rows[piv], rows[rank]
        for j in range(len(rows)):
            if j != rank and (rows[j] >> bit) & 1:
                rows[j] ^= rows[rank]
        rank += 1
    return rank


def jf_make_matrix(key_len: int, r: int, seed: int = 0x6b6466):
    """A pseudo-random r x key_len GF(2) matrix of full row rank, as `key_len` column words (deterministic: the same
    (key_len, r) always gives the same file)."""
    rng = np.random.default_rng([seed, key_len, r])
    while True:
        cols = [int(x) & ((1 << r) - 1) for x in rng.integers(0, 1 << 63, key_len, dtype=np.uint64)]
        if _gf2_rank(cols, r) == min(r, key_len):
            return cols


def jf_positions(columns, key_len: int, lo: np.ndarray, hi: Optional[np.ndarray] = None) -> np.ndarray:
    """Hash position of every key under a header's matrix1: XOR of columns[i] over the set bits key_len - 1 - i of the key
    (bit 0 = the last base's low bit; bits >= 64 live in `hi`).  The bit order is the one under which the reference's
    real Jellyfish file is sorted; for key_len > 64 it is the natural extension and pinned by nothing."""
    words = keys.from_pair(lo, hi, key_len // 2)
    out = np.zeros(len(words[0]), dtype=np.uint64)
    for i, col in enumerate(columns):
        b = key_len - 1 - i
        if b < 0:
            break
        out ^= (np.uint64(0) - keys.bit(words, b)) & np.uint64(col)
    return out


def write_jellyfish_index(path: str, k: int, lo: np.ndarray, hi: Optional[np.ndarray], counts: np.ndarray,
                          size: Optional[int] = None, matrix_columns=None, cmdline=None, header: Optional[dict] = None) -> str:
    """Write a Jellyfish ``binary/sorted`` index of (key, count) records given in ANY order.
    `size` (a power of two; default: the first >= 2 n, at least 2^10) and `matrix_columns` describe the hash the
    records are ordered by; `header` (a dict parsed from another Jellyfish file) supplies both, and every other field,
    unchanged -- re-writing a real Jellyfish file from its own records and header gives its bytes back."""
    if k > 63:
        raise ValueError(f"k={k}: the Jellyfish binary/sorted writer takes k <= 63 (write_index writes kdf/sorted at any k)")
    words = keys.from_pair(lo, hi, k)
    n = len(words[0])
    key_len = 2 * k
    kb = (key_len + 7) // 8
    hd, size, matrix_columns = _jellyfish_header(k, n, size, matrix_columns, cmdline, header)
    pos = jf_positions(matrix_columns, key_len, lo, hi) & np.uint64(size - 1)
    order = keys.order(words, pos)                          # position, then key
    rec = np.dtype([("k", "u1", (kb,)), ("c", "<u4")])
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(_header_bytes(hd))
        step = 1 << 22
        for a in range(0, n, step):                         # (records are assembled a slice at a time)
            o = order[a:a + step]
            data = np.zeros(len(o), dtype=rec)
            data["k"] = keys.to_bytes([w[o] for w in words], k)
            data["c"] = np.asarray(counts, dtype=np.uint32)[o]
            data.tofile(fh)
    os.replace(tmp, path)
    return path


def _jellyfish_header(k: int, n: int, size: Optional[int], matrix_columns, cmdline, header: Optional[dict]):
    """(header dict, size, matrix columns) of a ``binary/sorted`` index of ``n`` records: ``header`` unchanged when
    given, else one made for ``size`` / ``matrix_columns`` (shared by ``write_jellyfish_index`` and its device form)."""
    key_len = 2 * k
    if header is not None:
        hd = dict(header)
        if int(hd["key_len"]) != key_len:
            raise ValueError(f"header is for key_len {hd['key_len']}, the keys have {key_len}")
        size = int(hd["size"]); matrix_columns = list(hd["matrix1"]["columns"])
    else:
        if size is None:
            size = 1 << 10
            while size < 2 * n:
                size <<= 1
        if size & (size - 1):
            raise ValueError("size must be a power of two")
        r = size.bit_length() - 1
        if matrix_columns is None:
            matrix_columns = jf_make_matrix(key_len, r)
        hd = {
            "alignment": 8, "canonical": True, "cmdline": list(cmdline or []), "counter_len": 4,
            "exe_path": "kmer_denovo_filter_amd (libkdf.so)", "format": JF_FORMAT, "key_len": key_len,
            "matrix1": {"c": key_len, "columns": [int(c) for c in matrix_columns], "identity": False, "r": r},
            "max_reprobe": 126, "reprobes": jf_reprobes(126), "size": int(size), "val_len": 7,
        }
    if int(hd.get("counter_len", 4)) != 4:
        raise ValueError("only 4-byte counters are written")
    return hd, int(size), list(matrix_columns)


def _jellyfish_format() -> bool:
    return os.environ.get("KDF_JF_FORMAT", "").lower() in ("jellyfish", "binary/sorted", "jf")


def write_index_auto(path: str, k: int, lo, hi, counts, cmdline=None) -> str:
    """What the mirrors call for a user-visible index: ``kdf/sorted`` unless KDF_JF_FORMAT=jellyfish."""
    global LAST_INDEX_CODEC
    LAST_INDEX_CODEC = "host"
    if _jellyfish_format():
        return write_jellyfish_index(path, k, lo, hi, counts, cmdline=cmdline)
    return write_index(path, k, lo, hi, counts, cmdline=cmdline)


# ---- the same on the device (KmerEngine.index_encode_dev / index_decode_dev / jf_order_dev) ----------------------------
# KDF_DEVICE_INDEX=1 sends the mirrors' index writers and `load_index_into` here; the host functions above stay the
# default and the specification.  LAST_INDEX_CODEC: which codec the last such read or write took ("host" / "device").
LAST_INDEX_CODEC: Optional[str] = None


def device_index() -> bool:
    """The switch ``KDF_DEVICE_INDEX=1`` (default off)."""
    return os.environ.get("KDF_DEVICE_INDEX") == "1"


def _window_bytes() -> int:
    """Bytes of one window of records in flight: ``KDF_INDEX_CHUNK_MB`` MiB (default 64, at least 1), a multiple of 16."""
    try:
        mb = int(os.environ.get("KDF_INDEX_CHUNK_MB", "") or 64)
    except ValueError:
        mb = 64
    return (max(1, mb) << 20) // 16 * 16


def _device_key_form(dlo, dhi, dcounts, k: int):
    """(lo, hi or None, counts as int32 or None, n) of ``devkeys``-form tensors, contiguous, in the form of ``k``."""
    import torch
    n = int(dlo.shape[0])
    dlo = dlo.contiguous()
    dhi = dhi.contiguous() if dhi is not None and 33 <= int(k) <= 63 else None
    if 33 <= int(k) <= 63 and dhi is None:
        dhi = torch.zeros_like(dlo)
    if dcounts is not None:
        dcounts = dcounts.contiguous()
        if dcounts.element_size() != 4:
            dcounts = dcounts.to(torch.int32)
        if int(dcounts.shape[0]) != n:
            raise ValueError(f"{int(dcounts.shape[0])} counts for {n} keys")
    return dlo, dhi, dcounts, n


def _write_records_device(fh, eng, dlo, dhi, dcounts, dperm, n: int, k: int):
    """The record body of (keys, counts[, perm]) in device memory -> ``fh``: encoded window by window into one device
    buffer and copied to two page-locked buffers in turn, so that the copy of window i + 1 runs while ``write()`` takes
    window i (the scheme of ``kmer_fasta.write_kmer_fasta_device``)."""
    import torch
    from .kmer_fasta import _pinned_pair
    total = n * eng.index_record_bytes(k)
    if not total:
        return
    dev = dlo.device
    win = _window_bytes()
    pinned = _pinned_pair(win)
    dbuf = torch.empty(min(win, total), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))                 # (the keys were written on the caller's stream)
    eng.set_stream(stream.cuda_stream)
    p = lambda t: t.data_ptr() if t is not None else None
    try:
        windows = [(a, min(win, total - a)) for a in range(0, total, win)]
        done = [None, None]

        def issue(i):
            a, m = windows[i]
            eng.index_encode_dev(p(dlo), p(dhi), p(dcounts), p(dperm), n, k, a, m, dbuf.data_ptr())
            with torch.cuda.stream(stream):
                torch.from_numpy(pinned[i & 1][:m]).copy_(dbuf[:m], non_blocking=True)
                done[i & 1] = torch.cuda.Event()
                done[i & 1].record(stream)

        issue(0)
        for i, (a, m) in enumerate(windows):
            done[i & 1].synchronize()
            if i + 1 < len(windows):
                issue(i + 1)                                           # (encode and copy run while this window is written)
            fh.write(memoryview(pinned[i & 1][:m]))
        stream.synchronize()
    finally:
        eng.set_stream(None)


def write_index_device(path: str, k: int, dlo, dhi, dcounts, cmdline=None, engine=None) -> str:
    """``write_index`` for keys and counts in device memory (``devkeys`` form: int64 CUDA tensors in ascending key
    order, hi None unless k is 33..63, long k: (n, W) rows; counts a 4-byte integer tensor or None for zeros).  Only the
    file's own bytes cross the bus, in windows of ``KDF_INDEX_CHUNK_MB`` MiB (default 64).  The file is byte-identical
    to ``write_index``'s and is written through ``.tmp`` + ``os.replace``."""
    from .kmer_fasta import codec_engine
    global LAST_INDEX_CODEC
    dlo, dhi, dcounts, n = _device_key_form(dlo, dhi, dcounts, k)
    eng = engine if engine is not None else codec_engine(dlo.device.index or 0)
    if not eng.index_record_bytes(k):
        raise ValueError(f"{path}: no index record for k={k}")
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(_header_bytes(_kdf_header(k, n, cmdline)))
        _write_records_device(fh, eng, dlo, dhi, dcounts, None, n, k)
    os.replace(tmp, path)
    LAST_INDEX_CODEC = "device"
    return path


def write_jellyfish_index_device(path: str, k: int, dlo, dhi, dcounts, size: Optional[int] = None, matrix_columns=None,
                                 cmdline=None, header: Optional[dict] = None) -> str:
    """``write_jellyfish_index`` for keys and counts in device memory, given in ANY order: the record order comes from
    ``KmerEngine.jf_order_dev`` and the records are encoded through that permutation.  Header rules, refusals and file
    bytes are the host writer's."""
    import torch
    from .kmer_fasta import codec_engine
    global LAST_INDEX_CODEC
    if k > 63:
        raise ValueError(f"k={k}: the Jellyfish binary/sorted writer takes k <= 63 (write_index writes kdf/sorted at any k)")
    dlo, dhi, dcounts, n = _device_key_form(dlo, dhi, dcounts, k)
    hd, size, matrix_columns = _jellyfish_header(k, n, size, matrix_columns, cmdline, header)
    dev = dlo.device
    eng = codec_engine(dev.index or 0)
    dperm = None
    if n:
        dperm = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()                   # (the keys were written on the caller's stream)
        eng.jf_order_dev(dlo.data_ptr(), dhi.data_ptr() if dhi is not None else None, n, k, matrix_columns, size, dperm.data_ptr())
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(_header_bytes(hd))
        _write_records_device(fh, eng, dlo, dhi, dcounts, dperm, n, k)
    os.replace(tmp, path)
    LAST_INDEX_CODEC = "device"
    return path


def write_index_auto_device(path: str, k: int, dlo, dhi, dcounts, cmdline=None) -> str:
    """``write_index_auto`` for a dump kept in device memory: ``kdf/sorted`` unless KDF_JF_FORMAT=jellyfish."""
    if _jellyfish_format():
        return write_jellyfish_index_device(path, k, dlo, dhi, dcounts, cmdline=cmdline)
    return write_index_device(path, k, dlo, dhi, dcounts, cmdline=cmdline)


def _decode_file_device(eng, path: str, k: int, kb: int, cb: int, off: int, first: int, last: int, dev, sink):
    """Records first .. last of the record area -> ``sink(a, m, lo, hi, counts)`` per chunk of m records from record a:
    the chunk is read into one of two page-locked buffers, uploaded on a copy stream while the chunk before is decoded,
    and decoded with ``eng.index_decode_dev`` into scratch tensors (valid until sink returns).  Chunks hold whole
    records.  A bad record raises ``IndexRecordError`` naming the file and the record's index in the file."""
    import torch
    from .engine import IndexRecordError
    from .kmer_fasta import _pinned_pair
    rd = kb + cb
    win = _window_bytes()
    chunk = max(1, win // rd)
    W = keys.n_words(k)
    pinned = _pinned_pair(win if win >= rd else rd)
    m_max = min(chunk, last - first)
    dbytes = [torch.empty(m_max * rd, dtype=torch.uint8, device=dev) for _ in range(2)]
    lo = torch.empty((m_max, W) if W > 2 else m_max, dtype=torch.int64, device=dev)
    hi = torch.empty(m_max, dtype=torch.int64, device=dev) if W == 2 else None
    cnt = torch.empty(m_max, dtype=torch.int32, device=dev)
    copy = torch.cuda.Stream(dev)
    torch.cuda.current_stream(dev).synchronize()
    up = [None, None]
    spans = [(a, min(chunk, last - a)) for a in range(first, last, chunk)]

    def decode(i):
        a, m = spans[i]
        up[i & 1].synchronize()
        try:
            eng.index_decode_dev(dbytes[i & 1].data_ptr(), m, k, cb, lo.data_ptr(), hi.data_ptr() if hi is not None else None, cnt.data_ptr())
        except IndexRecordError as e:
            raise IndexRecordError(f"{path}: record {a + e.record} holds a key with a bit at or above 2k = {2 * k}", a + e.record) from None
        sink(a, m, lo[:m], hi[:m] if hi is not None else None, cnt[:m])

    with open(path, "rb", buffering=0) as fh:
        fh.seek(off + first * rd)
        for i, (a, m) in enumerate(spans):
            buf = pinned[i & 1][:m * rd]
            if up[i & 1] is not None:
                up[i & 1].synchronize()                                # (the upload that last read this buffer; its decode has run)
            have = 0
            while have < m * rd:                                       # (short reads: pipes, network files)
                got = fh.readinto(memoryview(buf[have:]))
                if not got:
                    raise ValueError(f"{path}: truncated index")
                have += got
            with torch.cuda.stream(copy):
                dbytes[i & 1][:m * rd].copy_(torch.from_numpy(buf), non_blocking=True)
                up[i & 1] = torch.cuda.Event()
                up[i & 1].record(copy)
            if i:
                decode(i - 1)                                          # (runs while chunk i is uploaded)
        if spans:
            decode(len(spans) - 1)


def load_index_into_device(engine, path: str, expect_k: Optional[int] = None, part: int = 0, parts: int = 1) -> int:
    """``load_index_into`` with the records decoded on the device: the record area goes chunk by chunk
    (``KDF_INDEX_CHUNK_MB``) through two page-locked buffers into HBM, ``KmerEngine.index_decode_dev`` turns it into key
    and count rows there and ``add_pairs_dev`` adds them -- no decoded word crosses the bus.  Both formats, every
    ``counter_len`` 1..16; a rank takes the same share as ``iter_index``.  A record whose key has a bit at or above 2k
    raises ``IndexRecordError`` (the host path does not check).  Returns the number of records of the whole index."""
    import torch
    global LAST_INDEX_CODEC
    k, kb, cb, _, off, n = _index_layout(path, expect_k)
    if k != engine.k:
        raise ValueError(f"{path}: index has k={k}, the engine counts k={engine.k}")
    if not 1 <= cb <= 16:
        raise ValueError(f"{path}: counter_len {cb} outside 1..16")
    first, last = n * part // parts, n * (part + 1) // parts
    if n:
        engine.reserve(max(1, n // parts + 1))
    if last > first:
        dev = torch.device("cuda", getattr(engine, "device", 0) or 0)

        def add(a, m, lo, hi, cnt):
            engine.add_pairs_dev(lo.data_ptr(), hi.data_ptr() if hi is not None else None, cnt.data_ptr(), m)

        _decode_file_device(engine, path, k, kb, cb, off, first, last, dev, add)
    LAST_INDEX_CODEC = "device"
    return n


def read_index_device(path: str, expect_k: Optional[int] = None, device: int = 0):
    """``read_index`` into device memory: -> (k, dlo, dhi, dcounts) in ``devkeys`` form (int64 CUDA tensors, hi None
    unless k is 33..63; long k: (n, W) rows) with the counts as an int32 tensor holding the uint32 values."""
    import torch
    from .kmer_fasta import codec_engine
    global LAST_INDEX_CODEC
    k, kb, cb, _, off, n = _index_layout(path, expect_k)
    if not 1 <= cb <= 16:
        raise ValueError(f"{path}: counter_len {cb} outside 1..16")
    dev = torch.device("cuda", device)
    W = keys.n_words(k)
    dlo = torch.empty((n, W) if W > 2 else n, dtype=torch.int64, device=dev)
    dhi = torch.empty(n, dtype=torch.int64, device=dev) if W == 2 else None
    dcnt = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        def keep(a, m, lo, hi, cnt):
            dlo[a:a + m].copy_(lo)
            if dhi is not None:
                dhi[a:a + m].copy_(hi)
            dcnt[a:a + m].copy_(cnt)
            torch.cuda.current_stream(dev).synchronize()               # (the scratch rows are decoded into again)

        _decode_file_device(codec_engine(device), path, k, kb, cb, off, 0, n, dev, keep)
    LAST_INDEX_CODEC = "device"
    return k, dlo, dhi, dcnt
