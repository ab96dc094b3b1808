"""tests/regions_model.py (the model of include/kdf.h "regions of informative reads") against the mirror's host sweep,
``discovery.regions._cluster_read_hits``: the same regions, the same members, and ``len(region_kmers)`` equal to the
model's distinct counts over the key rows of the same k-mers.  Pins the model; runs without a GPU."""
import numpy as np
import pytest

import regions_model as M

K = 31
NAMES = ["chr1", "chr10", "chr2", "chr21", "chr5", "chrX"]          # name order != numeric order


def _pool(rng, n):
    """n distinct k-mer strings and their one-word key rows (the codec both ways: the rows ARE the strings' keys)"""
    from kmer_denovo_filter_amd.reads import keys_to_kmers, kmers_to_keys
    lo = np.unique(rng.integers(0, 1 << 62, n, dtype=np.uint64))
    strs = keys_to_kmers(lo, None, K)
    back, _ = kmers_to_keys(strs, K, canonical=False)
    assert (np.asarray(back, dtype=np.uint64) == lo).all() and len(set(strs)) == len(lo)
    return strs, lo


def _check(hits, md, pool_strs, pool_keys, picks):
    """hits: [(chrom name, start, end, read name)], picks[i]: indices into the pool = the k-mers of hit i"""
    from kmer_denovo_filter_amd.discovery.regions import _cluster_read_hits
    read_hits = [(c, s, e, name, {pool_strs[j] for j in picks[i]}, False) for i, (c, s, e, name) in enumerate(hits)]
    regions, region_reads, region_kmers = _cluster_read_hits(read_hits, md)
    rank = {name: r for r, name in enumerate(sorted({h[0] for h in hits}))}
    names = sorted(rank, key=rank.get)
    chrom = np.array([rank[h[0]] for h in hits], np.int64)
    start = np.array([h[1] for h in hits], np.int64)
    end = np.array([h[2] for h in hits], np.int64)
    region_of, rows = M.cluster_intervals(chrom, start, end, md)
    assert [(names[c], s, e) for c, s, e, _ in rows.tolist()] == regions
    members = [set() for _ in rows]
    for i, g in enumerate(region_of.tolist()):
        assert g >= 0
        members[g].add(hits[i][3])
    assert [region_reads[key] for key in regions] == members
    group = np.concatenate([np.full(len(picks[i]), region_of[i], np.int64) for i in range(len(hits))] or [np.zeros(0, np.int64)])
    keys = np.concatenate([pool_keys[np.asarray(picks[i], np.int64)] for i in range(len(hits))] or [np.zeros(0, np.uint64)])
    counts = M.group_distinct(group, keys, len(rows))
    assert [len(region_kmers[key]) for key in regions] == counts.tolist()
    return rows


@pytest.mark.parametrize("seed,n,md", [(1, 300, 500), (2, 300, 0), (3, 80, 37), (4, 1000, 150)])
def test_random_hit_lists(seed, n, md):
    rng = np.random.default_rng(seed)
    strs, keys = _pool(rng, 400)
    hits, picks = [], []
    for i in range(n):
        c = NAMES[int(rng.integers(0, len(NAMES)))]
        s = int(rng.integers(0, 40)) * 250 if i % 3 == 0 else int(rng.integers(0, 10_000))     # every third start is one of 40: ties
        ln = int(rng.integers(0, 4000)) if i % 17 == 0 else int(rng.integers(0, 300))          # now and then a long interval
        hits.append((c, s, s + ln, f"read{int(rng.integers(0, n // 2 + 1))}"))
        base = (s // 700) * 7 % len(keys)                                                      # neighbours share k-mers
        picks.append(((base + rng.integers(0, 30, int(rng.integers(0, 12)))) % len(keys)).tolist())
    rows = _check(hits, md, strs, keys, picks)
    assert 1 < len(rows) < n


def test_the_running_end_is_not_the_last_end():
    rng = np.random.default_rng(5)
    strs, keys = _pool(rng, 50)
    # a long interval holds later short ones: the third joins through the first's end, not the second's
    hits = [("chr2", 100, 5000, "a"), ("chr2", 200, 300, "b"), ("chr2", 4000, 4100, "c"), ("chr2", 5601, 5700, "d")]
    rows = _check(hits, 600, strs, keys, [[0, 1], [1, 2], [3], [0]])
    assert rows.tolist() == [[0, 100, 5000, 3], [0, 5601, 5700, 1]]


@pytest.mark.parametrize("md", [0, 1, 500])
def test_the_boundary_joins_and_one_past_it_splits(md):
    rng = np.random.default_rng(6)
    strs, keys = _pool(rng, 50)
    hits = [("chr10", 1000, 2000, "a"), ("chr10", 2000 + md, 2100 + md, "b"), ("chr10", 2100 + 2 * md + 1, 2200 + 2 * md + 1, "c"),
            ("chr5", 0, 10, "a")]
    rows = _check(hits, md, strs, keys, [[0], [0, 1], [0, 1], [2]])
    assert rows[:, 3].tolist() == [2, 1, 1]


def test_a_contig_change_opens_a_region_whatever_the_earlier_end():
    rng = np.random.default_rng(7)
    strs, keys = _pool(rng, 50)
    hits = [("chr1", 10, 1_000_000, "a"), ("chr10", 5, 50, "b"), ("chr10", 60, 70, "c")]
    rows = _check(hits, 100, strs, keys, [[0], [1], [1, 2]])
    assert rows.tolist() == [[0, 10, 1_000_000, 1], [1, 5, 70, 2]]


def test_one_interval_and_none():
    rng = np.random.default_rng(8)
    strs, keys = _pool(rng, 50)
    rows = _check([("chr5", 7, 7, "only")], 0, strs, keys, [[4, 4, 5]])
    assert rows.tolist() == [[0, 7, 7, 1]]
    region_of, rows = M.cluster_intervals([], [], [], 500)
    assert region_of.shape == (0,) and rows.shape == (0, 4)
    from kmer_denovo_filter_amd.discovery.regions import _cluster_read_hits
    assert _cluster_read_hits([], 500) == ([], {}, {})
    assert M.group_distinct([], np.zeros((0, 1), np.uint64), 3).tolist() == [0, 0, 0]


def test_the_model_skips_and_ignores_what_the_header_says():
    region_of, rows = M.cluster_intervals([2, -1, 2, -5], [10, 0, 5, 3], [20, 9, 8, 4], 1)
    assert region_of.tolist() == [1, -1, 0, -1] and rows.tolist() == [[2, 5, 8, 1], [2, 10, 20, 1]]
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.array([[1, 2], [1, 2], [2, 1], [ones, ones], [ones, 0], [1, 2], [1, 2]], np.uint64)
    assert M.group_distinct([0, 0, 0, 0, 0, 1, 9], keys, 3).tolist() == [3, 1, 0]
