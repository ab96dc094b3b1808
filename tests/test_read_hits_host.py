"""CPU checks for the per-read hits of the scan (kdf_read_hits / kdf_hit_list): the model of tests/hits_truth.py pinned
to the oracle at k <= 63, the binding of the four entry points, the Python faces, and the tie to the discovery chain on
the mini trio (computed with the models; tests/test_gpu_read_hits.py asserts the same of the engine)."""
import os
import re

import numpy as np
import pytest

import depth_truth as DT
import hits_truth as HT
import kmer_truth as KT
from conftest import ROOT
from test_depth_host import oracle_profile, table_index

NAMES = {"kdf_read_hits_dev": 8, "kdf_read_hits": 8, "kdf_hit_list_dev": 9, "kdf_hit_list": 9}


@pytest.mark.parametrize("k", [5, 31, 33, 63])
def test_model_equals_oracle_on_random_reads(oracle, k):
    rng = np.random.default_rng(900 + k)
    reads = KT.random_reads(rng, k, 60, max_len=300) + ["", "N" * 40, "acgt" * 30, "ACGT"[:min(k - 1, 4)]]
    x = "".join(rng.choice(list("ACGT"), k + 3))
    reads.append(x + "N" + x + "n" + oracle.reverse_complement(x))            # every k-mer three times: distinct < hits
    other = KT.random_reads(rng, k, 30, max_len=300) + reads[::3] + [x]
    table = oracle.OracleTable(k).count_reads(other)
    index = table_index(table)
    rows, per_read = HT.read_hits(reads, k, index)
    assert rows[-1].tolist() == [12, 4] or k == 5                             # (k = 5: a 5-mer may repeat inside x)
    # the oracle alone: its canonical key of every valid window, looked up in its table; distinct by (lo, hi) pairs
    ocounts, ovalid, offs = oracle_profile(oracle, reads, k, table)
    assert (ocounts > 0).any() and (ocounts[ovalid] == 0).any()
    pos, rd = HT.hit_list(reads, per_read)
    assert np.array_equal(pos, np.flatnonzero(ocounts > 0))
    assert np.array_equal(rd, np.searchsorted(offs, pos, side="right") - 1)
    for r, s in enumerate(reads):
        S = s.upper()
        at = np.flatnonzero(ocounts[offs[r]:offs[r + 1]] > 0)
        assert np.array_equal(per_read[r], at)
        assert rows[r, 0] == len(at)
        assert rows[r, 1] == len({oracle.canonical_key(S[i:i + k]) for i in at.tolist()})
    assert (rows[:, 1] <= rows[:, 0]).all() and (rows[:, 1] < rows[:, 0]).any()
    # the existing scan model says the same
    shits, sdistinct = KT.scan_truth(reads, k, index)
    assert np.array_equal(rows[:, 1], sdistinct) and all(list(a) == b for a, b in zip(per_read, shits))
    # a key stored with count 0 is no hit
    zrows, zper = HT.read_hits(reads, k, {v: 0 for v in index})
    assert not zrows.any() and not any(len(p) for p in zper)


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
    from kmer_denovo_filter_amd import engine
    from kmer_denovo_filter_amd.core import bam_scanner
    assert engine.READ_HITS_COLUMNS == HT.COLUMNS == ("hits", "distinct")
    for name in ("read_hits", "read_hits_dev", "hit_list", "hit_list_dev", "scan_hits", "scan_informative"):
        assert callable(getattr(engine.KmerEngine, name))
    assert callable(bam_scanner._scan_batch)


def test_trio_distinct_per_child_read_equals_the_chains(oracle, trio_reads):
    """Against the chain's 630 proband-unique k-mers (k = 31, min_child_count 3, parent_max_count 0) the model's
    `distinct` of every child read is what the existing scan model yields, and `hits` is column `present` of the
    count profile's rows."""
    child = trio_reads["child"]
    ref = oracle.read_fasta(os.path.join(ROOT, "tests", "golden", "giab", "mini_ref.fa"))
    rt = oracle.OracleTable(31).count_reads([s for _, s in ref])
    chain = oracle.discovery_chain(child, trio_reads["mother"], trio_reads["father"], rt, 31, 3, 0)
    lo, hi = chain["proband_unique"]
    index = {(int(h) << 64) | int(l): 1 for l, h in zip(lo.tolist(), hi.tolist())}
    assert len(index) == 630
    keys = DT.keys_of_reads(child, 31)
    rows, per_read = HT.read_hits(child, 31, index, keys)
    shits, sdistinct = KT.scan_truth(child, 31, index)
    assert np.array_equal(rows[:, 1], sdistinct) and all(list(a) == b for a, b in zip(per_read, shits))
    assert np.array_equal(rows[:, 0].astype(np.uint64), DT.depth_rows(child, 31, index, 0, keys)[:, 1])
    assert int((rows[:, 1] >= 1).sum()) > 0 and (rows[:, 1] <= rows[:, 0]).all()
