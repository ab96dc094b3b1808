"""Plain-Python model of the per-read reduction of the Module-3 scan (``kdf_read_hits`` / ``kdf_hit_list``) at any k.

Built from read strings and a ``{key: count}`` dict on ``tests/depth_truth.py``'s walk of a read (``read_keys``: the valid
windows of a read and their canonical keys, the oracle's ``canonicalize``): window i of read r is a HIT iff it is valid
and ``index[key] > 0`` -- a key stored with count 0 is no hit.  Per read: ``hits`` = number of hit windows, ``distinct`` =
size of the Python ``set`` of their canonical keys, and the ascending hit offsets.  Pinned at k <= 63 to ``OracleTable``
by ``tests/test_read_hits_host.py``.

Stream layout (include/kdf.h): read r starts at ``offsets[r]`` and is followed by one separator position."""
import numpy as np

import depth_truth as DT

COLUMNS = ("hits", "distinct")


def read_hits(reads, k, index, keys=None):
    """-> (rows uint32 (n_reads, 2): hits, distinct; [ascending hit offsets of each read, relative to its start])"""
    keys = DT.keys_of_reads(reads, k) if keys is None else keys
    rows = np.zeros((len(reads), 2), np.uint32)
    per_read = []
    for r, ks in enumerate(keys):
        hit = [(i, v) for i, v in ks if index.get(v, 0) > 0]
        rows[r] = (len(hit), len({v for _, v in hit}))
        per_read.append(np.array([i for i, _ in hit], np.int64))
    return rows, per_read


def hit_list(reads, per_read):
    """per-read hit offsets -> (stream positions int64 ascending, the read of each)"""
    offs = DT.offsets_of(reads)
    pos = [int(offs[r]) + p for r, ps in enumerate(per_read) for p in ps.tolist()]
    rd = [r for r, ps in enumerate(per_read) for _ in range(len(ps))]
    return np.array(pos, np.int64), np.array(rd, np.int64)


def mask_words(reads, per_read, n_words):
    """the hit mask the scan writes for these hits: uint64[n_words], bit i % 64 of word i / 64"""
    bits = np.zeros(n_words * 64, bool)
    pos, _ = hit_list(reads, per_read)
    bits[pos] = True
    return np.packbits(bits, bitorder="little").view(np.uint64)
