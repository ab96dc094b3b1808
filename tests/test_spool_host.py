"""The read spool without a GPU: the ABI is declared, bound and exported; the layout model (tests/spool_model.py) keeps
the invariants the header promises; the Python feeders take ``spool=None``."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import spool_model as M
import stream_truth as T
from conftest import ROOT

NEW = {"kdf_spool_create": 4, "kdf_spool_set_option": 3, "kdf_spool_get_stat": 3, "kdf_spool_append": 4,
       "kdf_spool_append_dev": 5, "kdf_spool_append_uploaded": 3, "kdf_spool_replay": 3, "kdf_spool_read_segment": 5,
       "kdf_spool_clear": 1}


def _declared_arity():
    hdr = open(os.path.join(ROOT, "include", "kdf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(?:int|void|const char \*)\s*(kdf_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_new_symbols_declared_bound_and_exported():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()
    declared = _declared_arity()
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    for name, arity in dict(NEW, kdf_spool_destroy=1, kdf_spool_error=1).items():
        assert name in declared, f"{name} is not declared in kdf.h"
        assert name in bound, f"{name} is not bound in _native.SYMBOLS"
        assert len(bound[name][1]) == declared[name] == arity, f"{name}: {len(bound[name][1])} bound arguments, the header declares {declared[name]}"
        assert getattr(lib, name) is not None


def test_python_face():
    from kmer_denovo_filter_amd.spool import ReadSpool
    for m in ("append", "append_dev", "append_uploaded", "replay", "read_segment", "stat", "clear", "close", "__enter__", "__exit__"):
        assert callable(getattr(ReadSpool, m))
    assert list(inspect.signature(ReadSpool.__init__).parameters)[1:] == ["device", "hbm_budget", "host_budget"]


def test_feeders_take_a_spool_and_are_otherwise_unchanged():
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _stream_bam
    from kmer_denovo_filter_amd.reads import stream_batches_overlapped
    p = inspect.signature(stream_batches_overlapped).parameters
    assert list(p) == ["engine", "readers", "filtered", "ring", "tally", "spool"]
    assert p["spool"].default is None and p["ring"].default == 0 and p["tally"].default is False
    p = inspect.signature(_stream_bam).parameters
    assert list(p) == ["engine", "bam_path", "ref_fasta", "threads", "filtered", "tally", "spool"]
    assert p["spool"].default is None and p["tally"].default is False


def _random_batches(rng, lengths):
    out = []
    for n in lengths:
        codes = rng.integers(0, 4, n).astype(np.uint8)
        inv = rng.random(n) < 0.02
        out.append(M.pack(codes, inv, rng) + (n,))             # dirty at and past n
    return out


def _t(packed, invalid, n):
    return torch.from_numpy(packed.view(np.int64)), torch.from_numpy(invalid.view(np.int64)), n


LENGTHS = [0, 1, 63, 64, 65, 127, 128, 4095, 4096, 700, 1000, 64 * 5, 2111, 12345]


def test_layout_rules():
    rng = np.random.default_rng(5)
    batches = _random_batches(rng, LENGTHS)
    place, seg_tiles = M.layout(LENGTHS, 1 << 12)
    assert place[0] is None and len(seg_tiles) >= 4
    assert max(seg_tiles) == 12345 // 64 + 1                   # the oversized batch has a segment of its own size
    segs = M.segments(batches, 1 << 12)
    for (packed, invalid, npos), tiles in zip(segs, seg_tiles):
        assert npos == 64 * tiles and (len(packed), len(invalid)) == M.stream_words(npos) == (2 * tiles + 4, tiles + 2)
        assert not packed[2 * tiles:].any() and (invalid[tiles:] == ~np.uint64(0)).all()
    # a pure function of the triples: other dirt at and past n_bases, the same words
    again = [M.pack(*M.unpack(p, i, n), np.random.default_rng(6)) + (n,) for p, i, n in batches]
    assert any((a[0] != b[0]).any() for a, b in zip(again, batches) if a[2])
    for s, t in zip(segs, M.segments(again, 1 << 12)):
        np.testing.assert_array_equal(s[0], t[0]); np.testing.assert_array_equal(s[1], t[1])
    # at least one invalid position behind every batch, a whole invalid tile behind one that fills its last tile
    for (packed, invalid, n), at in zip(batches, place):
        if at is None:
            continue
        s, t0 = at
        _, inv = M.unpack(segs[s][0], segs[s][1], segs[s][2])
        end = t0 * 64 + n
        assert inv[end:(t0 + M.batch_tiles(n)) * 64].all() and inv[end]
        if n % 64 == 0:
            assert inv[end:end + 64].all()


@pytest.mark.parametrize("k", [3, 31, 63])
def test_valid_windows_of_a_segment_are_the_union_of_its_batches(k):
    """... so no valid window of the concatenation spans two batches, and none is lost."""
    rng = np.random.default_rng(k)
    batches = _random_batches(rng, LENGTHS)
    place, _ = M.layout(LENGTHS, 1 << 12)
    segs = M.segments(batches, 1 << 12)
    for s, seg in enumerate(segs):
        parts = [T.count_truth(_t(*b), k) for b, at in zip(batches, place) if at is not None and at[0] == s]
        want = T.accumulate(parts)
        got = T.count_truth(_t(*seg), k)
        assert got[3] == sum(p[3] for p in parts)
        for a, b in zip(got[:3], want):
            assert torch.equal(a, b)
