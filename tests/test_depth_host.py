"""CPU checks for the count profile (kdf_window_counts / kdf_read_depth): the model of tests/depth_truth.py pinned to
the oracle at k <= 63, the binding of the four entry points, the Python faces, and the tie between the per-read rows
and the discovery chain on the mini trio (computed with the model; tests/test_gpu_depth.py asserts the same of the
engine)."""
import os
import re

import numpy as np
import pytest

import depth_truth as DT
import kmer_truth as KT
from conftest import ROOT

NAMES = {"kdf_window_counts_dev": 6, "kdf_window_counts": 6, "kdf_read_depth_dev": 8, "kdf_read_depth": 8}


def oracle_profile(O, reads, k, table):
    """per-window counts and validity from the ORACLE alone: a window is valid iff its k characters are A/C/G/T (any
    case); its count is OracleTable.query of the oracle's own canonical key of the window"""
    offs = DT.offsets_of(reads)
    counts = np.zeros(int(offs[-1]), np.uint32)
    valid = np.zeros(int(offs[-1]), bool)
    pos, keys = [], []
    for r, s in enumerate(reads):
        S = s.upper()
        ok = np.frombuffer(S.encode(), np.uint8)
        ok = np.isin(ok, np.frombuffer(b"ACGT", np.uint8))
        for i in range(len(S) - k + 1):
            if ok[i:i + k].all():
                pos.append(int(offs[r]) + i)
                keys.append(O.canonical_key(S[i:i + k]))
    if pos:
        lo, hi = O.keys_to_arrays(keys)
        counts[pos] = table.query(lo, hi)
        valid[pos] = True
    return counts, valid, offs


def table_index(table):
    """{key: count} of an OracleTable"""
    lo, hi, cnt = table.export_ge(0)
    return {(int(h) << 64) | int(l): int(c) for l, h, c in zip(lo.tolist(), hi.tolist(), cnt.tolist())}


def numpy_rows(counts, valid, offs, low_max):
    """the six columns by numpy over the per-position arrays"""
    rows = np.zeros((len(offs) - 1, 6), np.uint64)
    for r in range(len(offs) - 1):
        c = counts[offs[r]:offs[r + 1]][valid[offs[r]:offs[r + 1]]].astype(np.uint64)
        if len(c):
            rows[r] = (len(c), (c > 0).sum(), (c <= low_max).sum(), c.min(), c.max(), c.sum())
    return rows


@pytest.mark.parametrize("k", [5, 15, 31, 32, 33, 47, 63])
def test_model_equals_oracle_on_random_reads(oracle, k):
    rng = np.random.default_rng(k)
    reads = KT.random_reads(rng, k, 60, max_len=300) + ["", "N" * 40, "acgt" * 30, "ACGT"[:min(k - 1, 4)]]
    other = KT.random_reads(rng, k, 30, max_len=300) + reads[::3]
    table = oracle.OracleTable(k).count_reads(other)
    index = table_index(table)
    assert index == KT.count_truth(other, k)
    counts, valid, offs = DT.profile(reads, k, index)
    ocounts, ovalid, ooffs = oracle_profile(oracle, reads, k, table)
    assert np.array_equal(offs, ooffs) and np.array_equal(valid, ovalid) and np.array_equal(counts, ocounts)
    assert int(valid.sum()) == oracle.count_windows(reads, k)
    assert (counts > 0).any() and (counts[valid] == 0).any() and not counts[~valid].any()
    for low_max in (0, 1, 2, 2 ** 32 - 1):
        assert np.array_equal(DT.depth_rows(reads, k, index, low_max), numpy_rows(ocounts, ovalid, ooffs, low_max))


@pytest.fixture(scope="module")
def trio_tables(oracle, trio_reads):
    return {who: table_index(oracle.OracleTable(31, 1 << 20).count_reads(trio_reads[who])) for who in ("mother", "father")}


def test_model_equals_oracle_on_trio_child(oracle, trio_reads, trio_tables):
    child = trio_reads["child"]
    table = oracle.OracleTable(31, 1 << 20).count_reads(trio_reads["mother"])
    counts, valid, offs = DT.profile(child, 31, trio_tables["mother"])
    ocounts, ovalid, _ = oracle_profile(oracle, child, 31, table)
    assert int(valid.sum()) == 2348843 == oracle.count_windows(child, 31)
    assert np.array_equal(valid, ovalid) and np.array_equal(counts, ocounts)
    assert np.array_equal(DT.depth_rows(child, 31, trio_tables["mother"], 0), numpy_rows(ocounts, ovalid, offs, 0))


def proband_reads(oracle, trio_reads, keys=None):
    """indices of the child reads that hold at least one of the golden chain's proband-unique k-mers (k = 31,
    min_child_count 3, parent_max_count 0), and their number of k-mers"""
    ref = oracle.read_fasta(os.path.join(ROOT, "tests", "golden", "giab", "mini_ref.fa"))
    rt = oracle.OracleTable(31).count_reads([s for _, s in ref])
    chain = oracle.discovery_chain(trio_reads["child"], trio_reads["mother"], trio_reads["father"], rt, 31, 3, 0)
    lo, hi = chain["proband_unique"]
    unique = {(int(h) << 64) | int(l) for l, h in zip(lo.tolist(), hi.tolist())}
    keys = DT.keys_of_reads(trio_reads["child"], 31) if keys is None else keys
    return [r for r, ks in enumerate(keys) if any(v in unique for _, v in ks)], len(unique)


def test_trio_reads_with_proband_unique_kmers_show_low_depth_in_both_parents(oracle, trio_reads, trio_tables):
    """The 630 proband-unique k-mers have count 0 in both parents, so a child read that holds one has a window that is
    absent from the mother's table and from the father's: low >= 1 at low_max = 0, and min = 0."""
    child = trio_reads["child"]
    keys = DT.keys_of_reads(child, 31)
    holders, n_unique = proband_reads(oracle, trio_reads, keys)
    assert n_unique == 630 and len(holders) > 0
    for who in ("mother", "father"):
        rows = DT.depth_rows(child, 31, trio_tables[who], 0, keys)
        assert (rows[holders, 2] >= 1).all() and (rows[holders, 3] == 0).all(), who
        assert (rows[:, 0] >= rows[:, 1]).all() and (rows[:, 0] == rows[:, 1] + rows[:, 2]).all()   # low_max 0: absent or present


def test_symbols_bound_with_the_headers_argument_counts():
    from kmer_denovo_filter_amd import _native
    hdr = open(os.path.join(ROOT, "include", "kdf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = {name: args for name, _, args in _native.SYMBOLS}
    for name, nargs in NAMES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, f"{name} is not declared in include/kdf.h"
        assert len(m.group(1).split(",")) == nargs == len(bound[name]), name
    lib = _native.load()
    for name in NAMES:
        assert getattr(lib, name) is not None


def test_python_faces_exist():
    from kmer_denovo_filter_amd import engine, kmer_utils
    from kmer_denovo_filter_amd.core import jellyfish_wrappers
    assert engine.READ_DEPTH_COLUMNS == DT.COLUMNS == ("windows", "present", "low", "min", "max", "sum")
    for name in ("window_counts", "window_counts_dev", "read_depth", "read_depth_dev"):
        assert callable(getattr(engine.KmerEngine, name))
    assert callable(kmer_utils.JellyfishKmerQuery.query_read)
    assert callable(jellyfish_wrappers._jellyfish_query_sequences)
