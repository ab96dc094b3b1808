"""The plain-Python truth of tests/kmer_truth.py (what the long-k GPU fuzz is checked against) pinned to the C oracle
at k <= 63: counts, filtered counts and the scan's hits and distinct keys, on the same kind of reads the fuzz draws."""
import numpy as np
import pytest

import kmer_truth as T


@pytest.mark.parametrize("k", [5, 31, 33, 63])
def test_truth_matches_oracle(oracle, k):
    rng = np.random.default_rng(1000 + k)
    genome = "".join(rng.choice(list("ACGT"), 3000))
    reads = T.random_reads(rng, k, 60, genome, max_len=300)
    probe = T.random_reads(rng, k, 30, max_len=300) + reads[:20] + ["", "N" * (k + 3), "acgt" * k]
    tag = f"k={k}"
    # the one-call encoding equals kmer_to_int
    for _ in range(20):
        s = "".join(rng.choice(list("ACGT"), k))
        assert T.key_int(s) == oracle.kmer_to_int(s), tag
    # counts
    d = T.count_truth(reads, k)
    ks, cnt = T.sorted_items(d)
    ot = oracle.OracleTable(k).count_reads(reads)
    lo, hi, ocnt = ot.export_ge(0)
    elo, ehi = T.lohi(ks)
    assert np.array_equal(lo, elo) and np.array_equal(hi, ehi) and np.array_equal(cnt, ocnt), tag
    # the scan against a counted index: hit positions and distinct keys per read
    hits, dist = T.scan_truth(probe, k, d)
    ohit, odist = ot.scan_reads(probe)
    assert np.array_equal(dist, odist), tag
    assert sum(map(len, hits)) > 0 and int(ohit.sum()) == sum(map(len, hits)), tag
    off = 0
    for r, s in enumerate(probe):
        assert np.array_equal(np.nonzero(ohit[off:off + len(s)])[0], np.array(hits[r], dtype=np.int64)), f"{tag} read {r}"
        off += len(s)
    # the bitmap helper puts read r's hits at its stream offset
    offs = np.cumsum([0] + [len(s) + 1 for s in probe])
    words = T.hit_words(offs, hits, (int(offs[-1]) + 63) // 64)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert int(bits.sum()) == sum(map(len, hits)), tag
    # count --if (a subset of the keys plus absent ones) and the scan rule on a table that holds count-0 keys
    sel = [v for i, v in enumerate(ks) if i % 3 == 0]
    absent = [T.key_int(oracle.canonicalize("".join(rng.choice(list("ACGT"), k)))) for _ in range(20)]
    filt = sorted(set(sel) | set(absent))
    f = T.count_truth(probe, k, filt)
    flo, fhi = T.lohi(filt)
    of = oracle.OracleTable(k).load_filter(flo, fhi).count_reads_filtered(probe)
    assert np.array_equal(of.query(flo, fhi), np.array([f[v] for v in filt], np.uint32)), tag
    assert 0 in f.values(), tag
    hits, dist = T.scan_truth(reads, k, f)
    ohit, odist = of.scan_reads(reads)
    assert np.array_equal(dist, odist) and int(ohit.sum()) == sum(map(len, hits)), tag
