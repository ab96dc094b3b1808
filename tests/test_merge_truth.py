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
