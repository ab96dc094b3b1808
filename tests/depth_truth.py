"""Plain-Python model of the count profile along reads: per-window counts, validity and the per-read depth rows of
``kdf_window_counts`` / ``kdf_read_depth`` at any k.

Built on ``tests/kmer_truth.py`` (``key_int``, the oracle's ``canonicalize``) and walked exactly as ``scan_truth``
walks a read: window i of a read is valid iff its k bases are all A/C/G/T (any case); its count is ``index[key]`` of its
canonical key, 0 when the index does not hold it.  Pinned at k <= 63 to ``OracleTable`` by ``tests/test_depth_host.py``.

Stream layout (include/kdf.h): read r starts at ``offsets[r]`` and is followed by one separator position, so
``offsets[r + 1] = offsets[r] + len(read r) + 1`` and n_bases = offsets[-1]."""
import numpy as np

import kmer_truth as KT
from oracle import oracle as O

COLUMNS = ("windows", "present", "low", "min", "max", "sum")


def read_keys(read, k):
    """[(offset, canonical key)] of the valid windows of one read, in offset order"""
    S = read.upper()
    run, out = 0, []
    for j, ch in enumerate(S):
        run = run + 1 if ch in "ACGT" else 0
        if run >= k:
            i = j - k + 1
            out.append((i, KT.key_int(O.canonicalize(S[i:i + k]))))
    return out


def keys_of_reads(reads, k):
    """read_keys of every read (the slow part of the model: computed once, then looked up in any index)"""
    return [read_keys(r, k) for r in reads]


def offsets_of(reads):
    return np.cumsum([0] + [len(r) + 1 for r in reads]).astype(np.int64)


def profile(reads, k, index, keys=None):
    """-> (counts uint32[n_bases], valid bool[n_bases], offsets int64[n_reads + 1]) over the stream of ``reads``"""
    keys = keys_of_reads(reads, k) if keys is None else keys
    offs = offsets_of(reads)
    counts = np.zeros(int(offs[-1]), np.uint32)
    valid = np.zeros(int(offs[-1]), bool)
    for r, ks in enumerate(keys):
        for i, v in ks:
            valid[offs[r] + i] = True
            counts[offs[r] + i] = index.get(v, 0)
    return counts, valid, offs


def depth_rows(reads, k, index, low_max, keys=None):
    """-> uint64 (n_reads, 6): windows, present, low (count <= low_max, absent = 0), min, max, sum per read; all 0
    for a read without valid windows"""
    keys = keys_of_reads(reads, k) if keys is None else keys
    rows = np.zeros((len(reads), 6), np.uint64)
    for r, ks in enumerate(keys):
        if not ks:
            continue
        cs = [index.get(v, 0) for _, v in ks]
        rows[r] = (len(cs), sum(1 for c in cs if c > 0), sum(1 for c in cs if c <= low_max), min(cs), max(cs), sum(cs))
    return rows


def bits(words, n):
    """the first n bits of uint64 words (bit i % 64 of word i / 64) as bool"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)
