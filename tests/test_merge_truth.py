"""tests/merge_truth.py pinned on the CPU: its owner rule against distributed.owner_of, its hash against its own
inverse and against values worked out by hand, keys_with_hash, and the saturating merge."""
import numpy as np
import pytest

import merge_truth as T


def random_keys(rng, k, n):
    lo = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    if k <= 32:
        return (lo & np.uint64((1 << (2 * k)) - 1) if k < 32 else lo), None
    return lo, rng.integers(0, 1 << (2 * k - 64), n, dtype=np.uint64)


def test_mix64_by_hand_and_inverse():
    # Python ints, the formula of kdf_device.h spelled out
    for x in (0, 1, 0xFFFFFFFF, 1 << 32, (1 << 62) - 1, 0x0123456789ABCDEF, T.M64):
        want = ((x ^ (x >> 32)) * 0x9FB21C651E98DF25) & T.M64
        assert int(T.mix64(x)) == want
        assert int(T.unmix64(want)) == x
    assert (0x9FB21C651E98DF25 * 0x02AB9C720D1024AD) & T.M64 == 1
    assert int(T.unmix64(T.EMPTY)) == 0xFD54638D0FBBB8DE               # the key the empty marker would stand for
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 63, 100_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 100_000, dtype=np.uint64)
    assert np.array_equal(T.unmix64(T.mix64(x)), x)
    assert np.array_equal(T.mix64(T.unmix64(x)), x)
    hi = 0x2FFFFFFF12345678
    assert int(T.rot_hi(hi)) == ((hi << 37) | (hi >> 27)) & T.M64
    assert int(T.key_hash(5, hi)) == int(T.mix64(5 ^ int(T.rot_hi(hi))))


@pytest.mark.parametrize("k", [31, 63])
def test_owner_is_distributed_owner_of(k):
    import torch
    from kmer_denovo_filter_amd.distributed import owner_of
    rng = np.random.default_rng(k)
    lo, hi = random_keys(rng, k, 50_000)
    tlo = torch.from_numpy(lo.view(np.int64))
    thi = torch.from_numpy(hi.view(np.int64)) if hi is not None else None
    h = T.key_hash(lo, hi)
    for parts in (1, 2, 3, 5, 7, 8, 17, 33, 63, 64):
        want = owner_of(tlo, thi, parts).numpy()
        got = T.owner(h, parts)
        assert np.array_equal(got.astype(np.int64), want)
        assert int(got.max()) < parts
        if parts > 1:
            assert len(np.unique(got)) == parts


def test_slot_rules_by_hand():
    h = 0xDEADBEEFCAFEF00D
    assert int(T.home(h, 28)) == h >> 36
    assert int(T.home(h, 28, 3)) == ((h << 3) & T.M64) >> 36
    assert int(T.bucket(h, 28, 12)) == h >> 48 and int(T.bucket(h, 28, 13)) == h >> 49
    assert int(T.order_key(h, 28)) == h >> 42
    assert int(T.owner(h, 3)) == ((h >> 48) * 3) >> 16
    # an owner boundary is a 16-bit prefix: the first prefix of owner p is ceil(p * 65536 / parts)
    for parts in (3, 5, 7):
        for p in range(1, parts):
            t = -(-p * 65536 // parts)
            assert int(T.owner(t << 48, parts)) == p and int(T.owner(((t - 1) << 48) | ((1 << 48) - 1), parts)) == p - 1


@pytest.mark.parametrize("k", [31, 32, 33, 63])
def test_keys_with_hash_yields_the_prefix_and_valid_distinct_keys(k):
    rng = np.random.default_rng(100 + k)
    for nbits, top in ((28, 0), (28, (1 << 28) - 1), (28, 43691 << 12), (16, 43690), (1, 1), (0, 0), (40, 0x123456789A)):
        lo, hi = T.keys_with_hash(top, nbits, 300, k, rng)
        assert (hi is None) == (k <= 32) and lo.dtype == np.uint64 and len(lo) == 300
        h = T.key_hash(lo, hi)
        if nbits:
            assert np.all(h >> np.uint64(64 - nbits) == np.uint64(top))
        assert T.valid_keys(lo, hi, k).all()
        if k < 32:
            assert int(lo.max()) < 1 << (2 * k)
        if k > 32:
            assert int(hi.max()) < 1 << (2 * k - 64)
        assert len({(a, b) for a, b in zip(lo.tolist(), (hi if hi is not None else lo).tolist())}) == 300
    tops = rng.integers(0, 1 << 28, 500, dtype=np.uint64)               # one prefix per key
    lo, hi = T.keys_with_hash(tops, 28, 500, k, rng)
    assert np.array_equal(T.home(T.key_hash(lo, hi), 28), tops)


def test_is_canonical_is_the_reverse_complement_test():
    # k = 3: ACG (0b000110) against its reverse complement CGT (0b011011); AAT (3) <-> ATT (15); palindromes do not exist at odd k
    assert T.is_canonical([0b000110, 0b011011, 3, 15], None, 3).tolist() == [True, False, True, False]
    # k = 33, key = 33 x T: reverse complement is 33 x A = 0
    assert T.is_canonical([T.M64, 0], [3, 0], 33).tolist() == [False, True]


@pytest.mark.parametrize("k", [3, 15, 31, 32, 33, 34, 47, 62, 63])
def test_is_canonical_numpy_path_is_the_int_rule(k):
    rng = np.random.default_rng(200 + k)
    lo, hi = random_keys(rng, k, 400)
    if k > 32:                                                           # and keys next to their own reverse complement
        rlo, rhi = T.revcomp_key(lo[:100], hi[:100], k)
        lo, hi = np.concatenate([lo, rlo]), np.concatenate([hi, rhi])
    assert np.array_equal(T.is_canonical(lo, hi, k), T.is_canonical_ints(lo, hi, k))
    rlo, rhi = T.revcomp_key(lo, hi, k)
    blo, bhi = T.revcomp_key(rlo, rhi, k)                                # an involution
    assert np.array_equal(blo, lo) and (hi is None or np.array_equal(bhi, hi))
    for a, b, c, d in list(zip(lo.tolist(), (hi if hi is not None else lo * 0).tolist(), rlo.tolist(), (rhi if rhi is not None else rlo * 0).tolist()))[:20]:
        s = T.kmer_string(a, b if k > 32 else None, k)
        assert T.kmer_string(c, d if k > 32 else None, k) == T.revcomp_string(s)


WIDE_KS = (33, 37, 41, 47, 63)


@pytest.mark.parametrize("canonical", (False, True))
@pytest.mark.parametrize("k", WIDE_KS)
def test_collision_groups_share_all_64_hash_bits(k, canonical):
    import kmer_truth as KT
    rng = np.random.default_rng(300 + k)
    space = 1 << (2 * k - 64)
    hashes = [T.EMPTY, 0] + [int(x) for x in rng.integers(0, 1 << 63, 4, dtype=np.uint64) * np.uint64(2) + np.uint64(1)]
    for h in hashes:
        for n in (2, 3, 65, 300):
            if n > space or (canonical and k < 41):                      # the canonical share of a small space is not known beforehand
                continue
            lo, hi = T.collision_group(h, n, k, rng, canonical=canonical)
            assert lo.dtype == np.uint64 and hi.dtype == np.uint64 and len(lo) == len(hi) == n
            assert (T.key_hash(lo, hi) == np.uint64(h)).all()
            assert len(set(hi.tolist())) == n                            # distinct: one key per high word
            assert T.valid_keys(lo, hi, k).all()
            if canonical:
                assert T.is_canonical_ints(lo[:20], hi[:20], k).all() and T.is_canonical(lo, hi, k).all()
            for a, b in list(zip(lo.tolist(), hi.tolist()))[:5]:
                assert KT.key_int(T.kmer_string(a, b, k)) == a | (b << 64)
    # k = 33: four keys per hash and no more
    lo, hi = T.collision_group(hashes[2], 4, 33, rng)
    assert sorted(hi.tolist()) == [0, 1, 2, 3]
    with pytest.raises(AssertionError, match=r"k=33, h=0x[0-9a-f]{16}: 4 keys, 5 wanted"):
        T.collision_group(hashes[2], 5, 33, rng)


@pytest.mark.parametrize("k", (33, 47, 63))
def test_a_canonical_key_with_the_empty_marker_as_hash_exists(k):
    """One group with h = EMPTY per k: a canonical member is found among the first candidates (k = 33: among all four)."""
    rng = np.random.default_rng(400 + k)
    lo, hi = T.collision_group(T.EMPTY, 1, k, rng, canonical=True)
    assert int(T.key_hash(lo, hi)[0]) == T.EMPTY and T.is_canonical_ints(lo, hi, k).all() and T.valid_keys(lo, hi, k).all()
    assert int(lo[0]) == int(T.unmix64(T.EMPTY)) ^ int(T.rot_hi(hi[0]))


def test_keys_with_hash_canonical_and_pinned_to_64_bits():
    import time
    rng = np.random.default_rng(7)
    for k, nbits, top in ((31, 20, 5), (32, 12, 9), (33, 20, 77), (47, 28, 1 << 27), (63, 16, 43690)):
        lo, hi = T.keys_with_hash(top, nbits, 300, k, rng, canonical=True)
        assert np.all(T.key_hash(lo, hi) >> np.uint64(64 - nbits) == np.uint64(top))
        assert T.valid_keys(lo, hi, k).all() and T.is_canonical_ints(lo, hi, k).all()
        assert len({(a, b) for a, b in zip(lo.tolist(), (hi if hi is not None else lo).tolist())}) == 300
    h = 0x0123456789ABCDEF
    t0 = time.perf_counter()
    lo, hi = T.keys_with_hash(h, 64, 2100, 41, rng, canonical=True)    # a full wide bucket and some more, one hash
    took = time.perf_counter() - t0
    assert (T.key_hash(lo, hi) == np.uint64(h)).all() and len(set(hi.tolist())) == 2100 and T.is_canonical(lo, hi, 41).all()
    assert took < 1.0, f"{took:.2f} s"
    # what canonical=False gives is what it gave before the switch existed: the same draws in the same order
    a = T.keys_with_hash(3, 8, 50, 47, np.random.default_rng(1))
    b = T.keys_with_hash(3, 8, 50, 47, np.random.default_rng(1), canonical=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("canonical", (False, True))
@pytest.mark.parametrize("k", (33, 47, 63))
def test_keys_sharing_hi_differ_in_lo_and_hash_only(k, canonical):
    rng = np.random.default_rng(500 + k)
    for nbits, top in ((20, 0), (20, (1 << 20) - 1), (14, 8191), (28, 12345678)):
        lo, hi = T.keys_sharing_hi(top, nbits, 40, k, rng, canonical=canonical)
        assert len(set(hi.tolist())) == 1 and len(set(lo.tolist())) == 40 and T.valid_keys(lo, hi, k).all()
        h = T.key_hash(lo, hi)
        assert len(set(h.tolist())) == 40 and np.all(h >> np.uint64(64 - nbits) == np.uint64(top))
        assert len(set(T.home(h, nbits).tolist())) == 1
        if canonical:
            assert T.is_canonical_ints(lo, hi, k).all()
    lo, hi = T.keys_sharing_hi(5, 20, 10, k, rng, hi=2)                 # a high word of the caller's
    assert set(hi.tolist()) == {2}


def test_kmer_string_by_hand():
    import kmer_truth as KT
    assert T.kmer_string(0b000110, None, 3) == "ACG" and T.revcomp_string("ACG") == "CGT"
    assert T.kmer_string(T.M64, 3, 33) == "T" * 33 and T.kmer_string(0, 1, 33) == "C" + "A" * 32
    s = "ACGTTGCATGCATGCAAGGCTTAACCGGTTAGCTAGCTAAGCTTCGATCGGATTACA"[:47]
    v = KT.key_int(s)
    assert T.kmer_string(v & T.M64, v >> 64, 47) == s
    assert KT.key_int(T.revcomp_string(s)) == int(T.revcomp_key(v & T.M64, v >> 64, 47)[0]) | (int(T.revcomp_key(v & T.M64, v >> 64, 47)[1]) << 64)


def test_merge_saturates_sums_doubles_and_keeps_zero_counts():
    M = T.U32_MAX
    a = {10: M - 2, 11: M - 2, 12: 0x60000000, 13: 0, 14: 7, 16: M}
    b = {10: 1, 11: 2, 12: 0x60000000, 15: 0, 16: 0}
    c = {10: 0, 11: 0, 12: 0x60000000, 13: 0, 16: 1}
    lo, hi, cnt = T.merge([a, b, c])
    assert hi is None and cnt.dtype == np.uint32
    assert T.as_dict(lo, hi, cnt) == {10: M - 1, 11: M, 12: M, 13: 0, 14: 7, 15: 0, 16: M}
    assert T.as_dict(*T.merge([a, b])) [12] == 0xC0000000                # two of the three do not saturate
    # a key twice in one segment is summed; arrays and NULL counts; wide keys compare both words
    seg = (np.array([5, 5, 9], np.uint64), np.array([1, 1, 1], np.uint64), np.array([2, 3, 4], np.uint32))
    nul = (np.array([5, 6], np.uint64), np.array([2, 1], np.uint64), None)
    lo, hi, cnt = T.merge([seg, nul, {(5, 1): M - 5}])
    assert T.as_dict(lo, hi, cnt) == {(5, 1): M, (9, 1): 4, (5, 2): 0, (6, 1): 0}
    assert np.array_equal(hi, np.sort(hi))                               # ascending (hi, lo)
    lo, hi, cnt = T.merge([])
    assert len(lo) == 0 and len(cnt) == 0
    lo, hi, cnt = T.merge([(np.zeros(0, np.uint64), None, np.zeros(0, np.uint32)), {3: 1}])
    assert T.as_dict(lo, hi, cnt) == {3: 1}
