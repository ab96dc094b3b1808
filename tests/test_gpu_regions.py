"""kdf_cluster_intervals* and kdf_group_distinct* (include/kdf.h "regions of informative reads"), host and device
forms, against tests/regions_model.py.  Every case is a few thousand entries at most; the one larger case is the n just
past KR_BLOCK^2 that makes the one-workgroup scan of the block maxima run a second round."""
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

import regions_model as M

pytestmark = pytest.mark.gpu

KR_BLOCK = 256                                  # csrc/kdf_regions.h: sorted entries per workgroup; the scan of the block
SCAN_ROUND = 256                                # aggregates (kr_max_scan_kernel, kh_scan_kernel) takes 256 per round
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
GARBAGE = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def eng():
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(31, capacity_hint=1 << 10)
    yield e
    e.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()


def cluster_dev(eng, chrom, start, end, md, cap=None):
    """-> (rc, n_out, region_of, rows[:min(cap, n_out)], the words behind them): outputs pre-filled with garbage"""
    import torch
    n = len(chrom)
    cap = n if cap is None else cap
    dc, ds, de = _dev(np.asarray(chrom, np.int64)), _dev(np.asarray(start, np.int64)), _dev(np.asarray(end, np.int64))
    d_ro = torch.full((max(n, 1),), GARBAGE, dtype=torch.int64, device="cuda")
    d_rows = torch.full((cap + 2, 4), GARBAGE, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc, m = eng._cluster_intervals_dev(dc.data_ptr() if n else 0, ds.data_ptr() if n else 0, de.data_ptr() if n else 0, n, md,
                                       d_ro.data_ptr(), d_rows.data_ptr() if cap else 0, cap)
    eng.synchronize()
    rows = d_rows.cpu().numpy()
    w = min(cap, m)
    assert (rows[w:] == GARBAGE).all(), "a write past the first min(cap, n_out) rows"
    return rc, m, d_ro.cpu().numpy()[:n], rows[:w]


def check_cluster(eng, chrom, start, end, md):
    """both forms against the model, twice: identical bytes"""
    chrom, start, end = (np.asarray(a, np.int64) for a in (chrom, start, end))
    want_of, want_rows = M.cluster_intervals(chrom, start, end, md)
    for _ in range(2):
        rc, m, got_of, got_rows = cluster_dev(eng, chrom, start, end, md)
        assert rc == 0 and m == len(want_rows)
        assert (got_of == want_of).all()
        assert (got_rows == want_rows).all()
    host_of, host_rows = eng.cluster_intervals(chrom, start, end, md)
    assert host_of.dtype == np.int64 and host_rows.dtype == np.int64 and host_rows.shape == want_rows.shape
    assert host_of.tobytes() == want_of.tobytes() and host_rows.tobytes() == want_rows.tobytes()
    return want_of, want_rows


def random_intervals(rng, n, n_chrom=3, span=5000, max_len=60):
    chrom = rng.integers(0, n_chrom, n)
    start = rng.integers(0, span, n)
    return chrom, start, start + rng.integers(0, max_len, n)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257])
def test_cluster_sizes(eng, n):
    rng = np.random.default_rng(100 + n)
    _, rows = check_cluster(eng, *random_intervals(rng, n, span=20 * n + 10), 25)
    assert n == 0 or 1 <= len(rows) <= n


def test_cluster_past_one_round_of_block_aggregates(eng):
    n = KR_BLOCK * SCAN_ROUND + KR_BLOCK + 1                         # 257 blocks: the scan of the aggregates runs two rounds
    rng = np.random.default_rng(7)
    chrom, start, end = random_intervals(rng, n, n_chrom=5, span=4 * n, max_len=12)
    end[3] = start[3] + 3 * n                                         # one long interval whose end is carried over many blocks
    _, rows = check_cluster(eng, chrom, start, end, 2)
    assert len(rows) > SCAN_ROUND * 4


def test_all_in_one_region_and_every_interval_its_own(eng):
    n = 3 * KR_BLOCK + 17
    start = np.arange(n) * 10
    _, rows = check_cluster(eng, np.zeros(n), start, start + 5, 5)   # start == E + md: joins
    assert rows.tolist() == [[0, 0, int(start[-1]) + 5, n]]
    _, rows = check_cluster(eng, np.zeros(n), start, start + 5, 4)   # start == E + md + 1: splits
    assert len(rows) == n and (rows[:, 3] == 1).all()


def test_the_first_interval_of_a_contig_covers_everything_after_it(eng):
    n = 5 * KR_BLOCK + 3
    rng = np.random.default_rng(8)
    start = np.concatenate(([0], 100 + 1000 * np.arange(n - 1)))
    end = start + 1
    end[0] = 2000 * n                                                 # the maximum is carried over five workgroups
    p = rng.permutation(n)
    _, rows = check_cluster(eng, np.full(n, 4)[p], start[p], end[p], 0)
    assert rows.tolist() == [[4, 0, 2000 * n, n]]


def test_contig_change_at_a_workgroup_boundary_and_under_a_larger_earlier_end(eng):
    # contig 0 fills exactly one workgroup and ends far beyond every start of contig 1: contig 1 must open its own region
    # (an unsegmented maximum would let contig 0's end swallow it)
    n0, n1 = KR_BLOCK, KR_BLOCK + 9
    chrom = np.concatenate((np.zeros(n0), np.ones(n1)))
    start = np.concatenate((1000 + np.arange(n0), 5 + 300 * np.arange(n1)))
    end = start + 10
    end[7] = 10 ** 9
    of, rows = check_cluster(eng, chrom, start, end, 100)
    assert rows[0].tolist() == [0, 1000, 10 ** 9, n0] and rows[1, :2].tolist() == [1, 5]
    assert len(rows) == 1 + n1 and of[n0] == 1
    # ... and the same with the change in the middle of a wave
    check_cluster(eng, np.concatenate((np.zeros(37), np.ones(50))), np.concatenate((np.arange(37), np.arange(50))),
                  np.concatenate((np.full(37, 10 ** 6), np.arange(50) + 1)), 0)


def test_shuffled_duplicate_starts_and_skipped_intervals(eng):
    rng = np.random.default_rng(9)
    n = 2 * KR_BLOCK + 100
    chrom = rng.integers(0, 4, n)
    start = rng.integers(0, 40, n) * 50                               # 40 distinct starts: many ties
    end = start + rng.integers(0, 80, n)
    chrom[rng.random(n) < 0.2] = -1
    chrom[5] = -(1 << 40)
    of, rows = check_cluster(eng, chrom, start, end, 7)
    assert (of[chrom < 0] == -1).all() and (of[chrom >= 0] >= 0).all()
    assert rows[:, 3].sum() == (chrom >= 0).sum()
    # nothing but skipped intervals
    of, rows = check_cluster(eng, np.full(70, -1), np.arange(70), np.arange(70), 0)
    assert (of == -1).all() and len(rows) == 0


def test_large_coordinates_and_ranks(eng):
    rng = np.random.default_rng(10)
    n = 300
    chrom = rng.choice([0, 1, (1 << 31) - 2, (1 << 31) - 1], n)
    start = (1 << 40) + rng.integers(0, 3000, n)
    start[::7] = (1 << 61) + rng.integers(0, 3000, len(start[::7]))
    end = start + rng.integers(0, 50, n)
    end[1] = (1 << 62) - 1
    _, rows = check_cluster(eng, chrom, start, end, 20)
    assert rows[:, 0].max() == (1 << 31) - 1
    check_cluster(eng, chrom, start, end, (1 << 62) - 1)


def test_cap_one_too_small_and_the_sizing_call(eng):
    rng = np.random.default_rng(11)
    chrom, start, end = random_intervals(rng, 600, span=100_000)
    want_of, want_rows = M.cluster_intervals(chrom, start, end, 10)
    m = len(want_rows)
    assert m > 3
    from kmer_denovo_filter_amd._native import KDF_ERR_INVALID
    rc, got, of, rows = cluster_dev(eng, chrom, start, end, 10, cap=m - 1)
    assert rc == KDF_ERR_INVALID and got == m and (of == want_of).all() and (rows == want_rows[:m - 1]).all()
    rc, got, of, rows = cluster_dev(eng, chrom, start, end, 10, cap=0)     # regions_out NULL: a sizing call
    assert rc == KDF_ERR_INVALID and got == m and (of == want_of).all()
    rc, got, of, rows = cluster_dev(eng, chrom, start, end, 10, cap=m)
    assert rc == 0 and got == m and (rows == want_rows).all()
    # the host form keeps the convention
    ro, rg = np.full(600, GARBAGE, np.int64), np.full((m - 1, 4), GARBAGE, np.int64)
    c, s, e = (np.ascontiguousarray(a, dtype=np.int64) for a in (chrom, start, end))
    rc, got = eng._cluster_intervals(c, s, e, 600, 10, ro, rg, m - 1)
    assert rc == KDF_ERR_INVALID and got == m and (ro == want_of).all() and (rg == want_rows[:m - 1]).all()


def test_host_form_refuses_bad_input_and_leaves_the_outputs(eng):
    from kmer_denovo_filter_amd._native import KDF_ERR_INVALID
    c, s, e = np.array([0, 0, 1], np.int64), np.array([5, 9, 2], np.int64), np.array([6, 9, 4], np.int64)

    def refused(c, s, e, n, md):
        ro, rg = np.full(3, GARBAGE, np.int64), np.full((3, 4), GARBAGE, np.int64)
        rc, got = eng._cluster_intervals(c, s, e, n, md, ro, rg, 3)
        assert rc == KDF_ERR_INVALID and got == 0
        assert (ro == GARBAGE).all() and (rg == GARBAGE).all()

    bad_end = e.copy(); bad_end[1] = 8                                # end < start
    refused(c, s, bad_end, 3, 0)
    refused(c, s, e, 3, -1)                                           # negative merge_distance
    refused(c, s, e, -1, 0)                                           # n < 0
    neg = s.copy(); neg[0] = -1
    refused(c, neg, e, 3, 0)
    big = c.copy(); big[2] = 1 << 31
    refused(big, s, e, 3, 0)
    # a skipped interval's coordinates are not looked at
    skip = c.copy(); skip[1] = -1
    ro, rg = eng.cluster_intervals(skip, s, bad_end, 0)
    assert ro.tolist() == [0, -1, 1] and rg.tolist() == [[0, 5, 6, 1], [1, 2, 4, 1]]
    with pytest.raises(Exception):
        eng.cluster_intervals(c, s, bad_end, 0)


# ---------------------------------------------------------------------------------------------------------------------


def distinct_dev(eng, group, keys, n_groups):
    import torch
    group = np.ascontiguousarray(group, dtype=np.int64)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    words = 1 if keys.ndim == 1 else keys.shape[1]
    n = len(group)
    dg, dk = _dev(group), _dev(keys)
    d_counts = torch.full((n_groups + 2,), GARBAGE, dtype=torch.int64, device="cuda")       # garbage: must be overwritten
    torch.cuda.synchronize()
    eng.group_distinct_dev(dg.data_ptr() if n else 0, dk.data_ptr() if n else 0, words, n, n_groups, d_counts.data_ptr())
    eng.synchronize()
    out = d_counts.cpu().numpy()
    assert (out[n_groups:] == GARBAGE).all(), "a write past counts_out[n_groups)"
    return out[:n_groups].view(np.uint64)


def check_distinct(eng, group, keys, n_groups):
    want = M.group_distinct(group, keys, n_groups)
    for _ in range(2):
        assert distinct_dev(eng, group, keys, n_groups).tobytes() == want.tobytes()
    host = eng.group_distinct(group, keys, n_groups)
    assert host.dtype == np.uint64 and host.tobytes() == want.tobytes()
    return want


def random_rows(rng, n, words, pool):
    """n rows drawn from `pool` distinct ones"""
    rows = rng.integers(0, 1 << 63, (pool, words), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (pool, words), dtype=np.uint64)
    return rows[rng.integers(0, pool, n)]


@pytest.mark.parametrize("words", [1, 2, 4, 7])
def test_distinct_words(eng, words):
    rng = np.random.default_rng(200 + words)
    n, ng = 3 * KR_BLOCK + 41, 23
    keys = random_rows(rng, n, words, 150)
    group = rng.integers(-2, ng + 3, n)                               # groups < 0 and >= n_groups among them
    group[group == 5] = 6                                             # a group without entries
    keys[rng.random(n) < 0.05] = ONES                                 # "no key" rows
    want = check_distinct(eng, group, keys if words > 1 else keys[:, 0], ng)
    assert want[5] == 0 and want.sum() > ng
    # rows that differ only in the lowest word, and only in the top word
    base = rng.integers(0, 1 << 62, words, dtype=np.uint64)
    rows = np.tile(base, (8, 1))
    rows[1, 0] ^= np.uint64(1); rows[2, 0] ^= np.uint64(1)
    rows[3, words - 1] ^= np.uint64(1 << 63); rows[4, words - 1] ^= np.uint64(1 << 63)
    want = check_distinct(eng, np.zeros(8, np.int64), rows, 1)
    assert want.tolist() == [3]
    # a row with ONE all-ones word is a key like any other (words > 1)
    part = np.tile(base, (3, 1)); part[0, 0] = ONES; part[1, words - 1] = ONES; part[2] = ONES
    assert check_distinct(eng, np.zeros(3, np.int64), part, 1).tolist() == [2 if words > 1 else 0]


def test_distinct_edges(eng):
    rng = np.random.default_rng(12)
    assert check_distinct(eng, np.zeros(0, np.int64), np.zeros((0, 2), np.uint64), 4).tolist() == [0, 0, 0, 0]      # n = 0
    n = 2 * KR_BLOCK + 5
    same = np.tile(rng.integers(1, 1 << 60, 3, dtype=np.uint64), (n, 1))
    assert check_distinct(eng, np.zeros(n, np.int64), same, 2).tolist() == [1, 0]                                  # all rows equal
    uniq = np.arange(n, dtype=np.uint64).reshape(n, 1) * np.uint64(0x9E3779B97F4A7C15)
    assert check_distinct(eng, rng.integers(0, 3, n), uniq, 3).sum() == n                                          # all rows distinct
    # the same row in two groups counts in both
    assert check_distinct(eng, [0, 1, 1, 0], np.array([[7, 7], [7, 7], [7, 7], [7, 8]], np.uint64), 2).tolist() == [2, 1]
    # nothing but ignored entries
    assert check_distinct(eng, [-1, 2, 0], np.array([1, 2, ONES], np.uint64), 2).tolist() == [0, 0]
    # n_groups = 0: KDF_OK, nothing written
    assert len(distinct_dev(eng, [0, 0], np.array([1, 2], np.uint64), 0)) == 0
    assert len(eng.group_distinct([0, 0], np.array([1, 2], np.uint64), 0)) == 0


def test_one_group_over_several_workgroups_and_64_groups_in_one_wave(eng):
    rng = np.random.default_rng(13)
    n = 6 * KR_BLOCK + 77
    keys = random_rows(rng, n, 2, 900)
    want = check_distinct(eng, np.full(n, 3), keys, 5)
    assert want.tolist() == [0, 0, 0, len(np.unique(keys, axis=0)), 0]
    group = np.arange(64)
    check_distinct(eng, group, random_rows(rng, 64, 2, 64), 64)
    group = np.repeat(np.arange(64), 3)
    assert check_distinct(eng, group, random_rows(rng, 192, 1, 20)[:, 0], 64).sum() > 64
    # many groups: the group word takes its own bits of the sort, whatever n_groups
    for ng in (1, 2, 255, 256, 257, (1 << 16) + 1):
        g = rng.integers(0, ng, 500)
        g[0] = ng - 1
        check_distinct(eng, g, random_rows(rng, 500, 1, 40)[:, 0], ng)


def test_refusals(eng):
    from kmer_denovo_filter_amd._native import KDF_ERR_INVALID
    g, k = np.zeros(2, np.int64), np.ones((2, 1), np.uint64)
    out = np.full(3, 77, np.uint64)
    vp = lambda a: a.ctypes.data_as(c_void_p)
    lib = eng._lib
    assert lib.kdf_group_distinct(eng._h, vp(g), vp(k), 0, 2, 3, vp(out)) == KDF_ERR_INVALID
    assert lib.kdf_group_distinct(eng._h, vp(g), vp(k), 9, 2, 3, vp(out)) == KDF_ERR_INVALID
    assert lib.kdf_group_distinct(eng._h, vp(g), vp(k), 1, 2, -1, vp(out)) == KDF_ERR_INVALID
    assert lib.kdf_group_distinct(eng._h, vp(g), vp(k), 1, 1 << 32, 3, vp(out)) == KDF_ERR_INVALID
    assert lib.kdf_group_distinct_dev(eng._h, None, None, 1, 1 << 32, 3, None) == KDF_ERR_INVALID
    assert (out == 77).all()
    m = c_uint64(5)
    assert lib.kdf_cluster_intervals_dev(eng._h, None, None, None, 1 << 32, 0, None, None, 0, byref(m)) == KDF_ERR_INVALID and m.value == 0


def test_profile_stats(eng):
    eng.profile(True)
    before = eng.get_stat("regions_passes")
    check_distinct(eng, [0, 1], np.array([3, 4], np.uint64), 2)
    check_cluster(eng, [0, 0], [1, 9], [2, 10], 1)
    assert eng.get_stat("regions_passes") >= before + 6             # two device calls and at least one host call each
    assert eng.get_stat("regions_us") > 0
    eng.profile(False)


@pytest.mark.parametrize("k", [31, 63, 101])
def test_the_mirrors_device_clustering_for_every_key_width(k):
    """discovery.regions._cluster_read_hits_device over a hand-made ledger (rows of eng.key_words words, ordinals of
    kept reads of which some never reach read_hits) against the host sweep fed the same k-mers as strings"""
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.core.bam_scanner import RegionLedger
    from kmer_denovo_filter_amd.discovery.regions import _cluster_read_hits, _cluster_read_hits_device
    from kmer_denovo_filter_amd.reads import keys_to_kmers
    rng = np.random.default_rng(300 + k)
    refs = ["chr1", "chr10", "chr2", "chr5"]
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        W = e.key_words
        pool = rng.integers(0, 1 << 62, (90, W), dtype=np.uint64)
        pool[:, W - 1] &= np.uint64((1 << min(2 * k - 64 * (W - 1), 62)) - 1)
        strs = keys_to_kmers(pool if W > 2 else np.ascontiguousarray(pool[:, 0]), np.ascontiguousarray(pool[:, 1]) if W == 2 else None, k)
        assert len(set(strs)) == len(pool)
        n_kept = 400
        picks = [rng.integers(0, len(pool), int(rng.integers(1, 30))) for _ in range(n_kept)]
        led = RegionLedger(e, refs)
        for lo in range(0, n_kept, 150):                              # three batches
            part = picks[lo:lo + 150]
            led.keys.append(torch.from_numpy(np.concatenate([pool[p] for p in part]).view(np.int64).reshape(-1).copy()).cuda())
            led.ordinals.append(torch.from_numpy(np.concatenate([np.full(len(p), lo + i, np.int64) for i, p in enumerate(part)])).cuda())
            led.n_reads += len(part)
        reach = np.flatnonzero(rng.random(n_kept) < 0.8)              # the others were dropped by name in the task merge
        host_hits, dev_hits = [], []
        for o in rng.permutation(reach).tolist():
            c, s = refs[int(rng.integers(0, 4))], int(rng.integers(0, 20_000))
            t = (c, s, s + int(rng.integers(1, 200)), f"read{o % 300}")
            host_hits.append(t + ({strs[j] for j in picks[o].tolist()}, False))
            dev_hits.append(t + (o, False))
        want = _cluster_read_hits(host_hits, 100)
        got = _cluster_read_hits_device(e, dev_hits, led, 100, refs)
        assert got[0] == want[0] and got[1] == want[1] and len(want[0]) > 4
        assert got[2] == {key: len(v) for key, v in want[2].items()}
        assert _cluster_read_hits_device(e, [], led, 100, refs) == ([], {}, {})
