"""The sieve model of the two-pass count (tests/prefilter_model.py) against a brute-force dict, and the ABI's seven
prefilter symbols.  No GPU."""
import os
import re

import numpy as np
import pytest

import prefilter_model as PM
from conftest import ROOT


def random_truth(rng, k, n):
    """n distinct keys of 2k bits with counts that lean towards 1 (the shape of a sequenced sample)"""
    keys = set()
    while len(keys) < n:
        keys.add(int.from_bytes(rng.bytes(32), "little") & ((1 << (2 * k)) - 1))
    counts = rng.choice([1, 1, 1, 1, 2, 2, 3, 4, 7, 40, 100000], size=n)
    return {key: int(c) for key, c in zip(sorted(keys), counts)}


@pytest.mark.parametrize("k", [15, 31, 32, 33, 47, 63])
@pytest.mark.parametrize("L", [2, 3])
def test_model_np_and_torch_equal_the_brute_force(k, L):
    import torch
    rng = np.random.default_rng(1000 * k + L)
    T = random_truth(rng, k, 10_000)
    s = 16 if k != 31 else 13                                 # (13: ~1.2 keys per cell, most cells shared)
    admitted, by_value = PM.model(T, k, s, L)
    ks = sorted(T)
    lo = np.array([v & PM.M64 for v in ks], dtype=np.uint64)
    hi = np.array([v >> 64 for v in ks], dtype=np.uint64)
    cnt = np.array([T[v] for v in ks], dtype=np.int64)
    assert [int(c) for c in PM.cells_np(lo, hi, k, s)] == [PM.cell_of(v, k, s) for v in ks]
    keep, bv = PM.model_np(lo, hi, cnt, k, s, L)
    assert bv == by_value and sum(by_value) == 1 << s
    assert {v for v, a in zip(ks, keep) if a} == set(admitted)
    tlo, thi = torch.from_numpy(lo.view(np.int64)), torch.from_numpy(hi.view(np.int64))
    tkeep, tbv = PM.model_torch(tlo, thi, torch.from_numpy(cnt), k, s, L)
    assert tbv == by_value
    assert np.array_equal(tkeep.numpy(), keep)
    # what the model promises: nothing with count >= L is lost, and leakage needs company in the cell
    assert all(v in admitted for v in ks if T[v] >= L)
    assert all(admitted[v] == T[v] for v in admitted)


def test_model_leaks_only_through_shared_cells():
    T = {5: 1, 9: 1, 1 << 40: 2}
    k, s = 31, 16
    cells = {v: PM.cell_of(v, k, s) for v in T}
    assert len(set(cells.values())) == 3                      # (three keys, three cells: no leakage possible)
    assert PM.model(T, k, s, 2)[0] == {1 << 40: 2}
    assert PM.model(T, k, s, 3)[0] == {}
    # two singletons forced into one cell (s = 1: two cells in all) are admitted at L = 2
    same = [v for v in range(1, 200) if PM.cell_of(v, k, 1) == PM.cell_of(1, k, 1)][:2]
    assert set(PM.model({v: 1 for v in same}, k, 1, 2)[0]) == set(same)


@pytest.mark.parametrize("k", [65, 75, 101, 201])
def test_long_key_cells_use_every_word(k):
    rng = np.random.default_rng(k)
    W = PM.key_words(k)
    base = int.from_bytes(rng.bytes(64), "little") & ((1 << (2 * k)) - 1)
    h0 = PM.stored_form(base, k)
    for j in range(W):                                        # a key that differs in one word only hashes elsewhere
        other = base ^ (1 << (64 * j + 1))
        assert PM.stored_form(other, k) != h0
    assert 0 <= PM.cell_of(base, k, 38) < 1 << 38


def test_header_declares_and_binding_binds_the_prefilter():
    from kmer_denovo_filter_amd import _native
    hdr = open(os.path.join(ROOT, "include", "kdf.h")).read()
    want = {"kdf_prefilter_begin", "kdf_prefilter_add_reads", "kdf_prefilter_add_reads_dev", "kdf_prefilter_add_uploaded",
            "kdf_prefilter_arm", "kdf_prefilter_drop", "kdf_prefilter_fill"}
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert want <= set(re.findall(r"\b(kdf_[a-z0-9_]+)\s*\(", code))
    assert want <= {name for name, _, _ in _native.SYMBOLS}
    lib = _native.load()
    for name in want:
        assert getattr(lib, name) is not None
    # the rule the model restates is the one the header states
    assert "0x9FB21C651E98DF25" in hdr and "0x632BE59BD9B4E019" in hdr and "h >> (64 - s)" in hdr
    from kmer_denovo_filter_amd import KmerEngine
    for m in ("prefilter_begin", "prefilter_add", "prefilter_add_dev", "prefilter_add_uploaded", "prefilter_arm",
              "prefilter_drop", "prefilter_fill"):
        assert callable(getattr(KmerEngine, m))
