"""Reads in a spool without a GPU: the ABI is declared, bound and exported; the offsets model
(tests/spool_reads_model.py) keeps what the header promises -- the gap behind a batch is all invalid, so the valid windows
of every read are those of its batch alone."""
import os
import re

import numpy as np
import pytest

import spool_model as M
import spool_reads_model as R
from conftest import ROOT

NEW = {"kdf_spool_append_reads": 6, "kdf_spool_append_reads_dev": 7, "kdf_spool_append_uploaded_reads": 5,
       "kdf_spool_read_offsets": 5, "kdf_spool_segment_dev": 8, "kdf_spool_read_hits": 3, "kdf_spool_read_depth": 4,
       "kdf_spool_select_reads": 6}


def test_new_symbols_declared_bound_and_exported():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kdf.h")).read(), flags=re.S)
    declared = {name: args.count(",") + 1 for name, args in re.findall(r"\bint\s*(kdf_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)}
    bound = {name: args for name, _, args in _native.SYMBOLS}
    for name, arity in NEW.items():
        assert declared.get(name) == arity, f"{name}: kdf.h declares {declared.get(name)} arguments"
        assert len(bound[name]) == arity, f"{name}: {len(bound[name])} bound arguments"
        assert getattr(lib, name) is not None


def test_python_face():
    from kmer_denovo_filter_amd.spool import ReadSpool
    for m in ("read_hits", "read_depth", "select_reads", "segment_dev", "read_offsets", "read_hits_dev", "read_depth_dev", "select_reads_dev"):
        assert callable(getattr(ReadSpool, m))
    assert isinstance(ReadSpool.n_reads, property) and isinstance(ReadSpool.ordinals, property)


def _windows_per_read(packed, invalid, n, offs, k):
    _, inv = M.unpack(packed, invalid, n)
    bad = np.concatenate([[0], np.cumsum(inv)])
    starts = np.arange(max(n - k + 1, 0))
    valid = np.zeros(n, bool)
    valid[:len(starts)] = bad[starts + k] == bad[starts]
    return np.array([valid[a:b].sum() for a, b in zip(offs[:-1], offs[1:])], np.int64)


@pytest.mark.parametrize("k", [3, 31, 63])
def test_the_gap_gives_no_read_a_window(k):
    """The gap ARGUMENT, checked on the numpy models alone (spool_model + spool_reads_model): no product code runs here,
    so this passes with or without the spool's read offsets.  The device tests (test_gpu_spool_reads.py) hold the spool to
    these models."""
    rng = np.random.default_rng(k)
    batches = []
    for rem, lens in ((0, [1, 0, k - 1, k, 200]), (63, [150]), (1, [40, 0, 0, 90, 77]), (0, [64 * 3 - 1]), (0, [5000]), (63, [33, 70])):
        batches.append(R.make_batch(rng, [None if n == 0 else rng.integers(0, 4, n) for n in lens], rem=rem))
    empty = R.make_batch(rng, [])
    batches.insert(2, empty)
    segs = M.segments([b[:3] for b in batches], 1 << 12)
    offs = R.segment_offsets(batches, 1 << 12)
    assert len(segs) == len(offs) >= 3
    alone = np.concatenate([_windows_per_read(*b[:3], b[3], k) for b in batches])
    got = np.concatenate([_windows_per_read(p, m, n, o, k) for (p, m, n), (o, _, _) in zip(segs, offs)])
    np.testing.assert_array_equal(got, alone)
    assert alone.sum() > 0
    reads = 0
    for (p, m, n), (o, first, nr) in zip(segs, offs):
        assert first == reads and o[0] == 0 and (np.diff(o) >= 0).all() and o[-1] <= n and len(o) == nr + 1
        reads += nr
    assert reads == sum(len(b[3]) - 1 for b in batches)
