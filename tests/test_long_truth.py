"""tests/long_truth.py pinned down on the CPU: worked values, the hash's inverse, agreement with the package's host
restatement (distributed.long_hash / owner_of_w) and with the string rules of tests/kmer_truth.py, and every generator
held to what was asked of it."""
import numpy as np
import pytest

import long_truth as T

KS = (65, 97, 129, 161, 201)                 # W = 3, 4, 5, 6, 7
M64 = T.M64


# worked with Python ints outside long_truth: (row, fold of its upper words, hash).  The second row by hand: the fold of
# (0, 0) is mix64(0x632BE59BD9B4E019) + 0x632BE59BD9B4E019 (mix64(0) = 0, so the first step leaves the constant).
WORKED = [
    ([1, 2, 3], 0x11E7D5436339CB7E, 0xF7724CE81210A2AC),
    ([0, 0, 0], 0x21979208D9ACE9E3, 0x34F3DF15CF129DF7),
    ([7, 6, 5, 4, 3, 2, 1], 0xA024C866802B3AFD, 0x1D929C22DB43F48C),
    ([M64, M64 - 1, M64 - 2, M64 - 3, M64 - 4, M64 - 5, (1 << 18) - 1], 0x116BC43B0D4266FE, 0x456ED56511C62179),
]


def test_worked_values():
    assert int(T.mix64(1)) == 0x9FB21C651E98DF25 and int(T.mix64(1 << 32)) == 0xBE4AFB8A1E98DF25
    assert int(T.unmix64(M64)) == 0xFD54638D0FBBB8DE
    assert int(T.fold_step(0, 0)) == T.FOLD_ADD
    for row, f, h in WORKED:
        rows = np.array([row], np.uint64)
        assert int(T.fold(rows)[0]) == f and int(T.long_hash(rows)[0]) == h
        assert int(T.unmix64(h)) ^ f == row[0]                     # w0 back from the stored form
    # fields of a hash, by hand: h = 0xABCD_0000_8000_FFFF
    h = 0xABCD00008000FFFF
    assert int(T.home(h, 10)) == 0xABCD >> 6 and int(T.home(h, 12)) == 0xABC and int(T.bucket(h, 12, 11)) == 1
    assert int(T.owner(h, 2)) == 1 and int(T.owner(h - (1 << 16), 2)) == 0 and int(T.owner(h, 64)) == 32
    assert int(T.slice_of(h, 5)) == 4 and int(T.slice_of(h & ~0xFFFF, 5)) == 0
    w, b1, b2 = T.sieve_word_bits(h, 1023)
    assert (int(w), int(b1), int(b2)) == ((0x8000FFFF >> 12) & 1023, 63, 63)
    assert T.sieve_words(300) == 1024 and T.sieve_words(2048) == 1024 and T.sieve_words(2049) == 2048
    assert T.sieve_words(300, (1 << 20) // 300 + 32) == 32768
    assert [T.W_of(k) for k in (65, 95, 127, 159, 191, 201)] == [3, 3, 4, 5, 6, 7]
    assert [T.top_width(k) for k in (65, 95, 127, 159, 191, 201)] == [2, 62, 62, 62, 62, 18]


def test_unmix_inverts_mix():
    rng = np.random.default_rng(1)
    x = np.concatenate([T._rand64(rng, 5000), np.array([0, 1, M64, 1 << 32, 1 << 63], np.uint64)])
    assert np.array_equal(T.unmix64(T.mix64(x)), x) and np.array_equal(T.mix64(T.unmix64(x)), x)


@pytest.mark.parametrize("k", KS)
def test_hash_and_owner_equal_the_host_restatement(k):
    import torch
    from kmer_denovo_filter_amd.distributed import long_hash, owner_of_w
    rng = np.random.default_rng(k)
    rows = T.random_rows(rng, k, 200)
    t = torch.from_numpy(rows.view(np.int64))
    h = T.long_hash(rows)
    assert np.array_equal(long_hash(t).numpy().view(np.uint64), h)
    for parts in (1, 2, 3, 7, 64):
        assert np.array_equal(owner_of_w(t, parts).numpy().astype(np.uint64), T.owner(h, parts))


@pytest.mark.parametrize("k", KS)
def test_canonical_and_codec_equal_the_string_rules(k, oracle):
    import kmer_truth as KT
    rng = np.random.default_rng(100 + k)
    W = T.W_of(k)
    n_canon = 0
    for _ in range(60):
        s = "".join(rng.choice(list("ACGT"), k))
        row = T.kmer_to_row(s)
        assert T.row_to_int(row) == KT.key_int(s) == oracle.kmer_to_int(s)
        assert T.row_to_kmer(row, k) == s and T.int_to_row(KT.key_int(s), W) == row
        rc = oracle.reverse_complement(s)
        assert T.revcomp_str(s) == rc and T.revcomp(KT.key_int(s), k) == KT.key_int(rc)
        assert T.is_canonical(row, k) == (oracle.canonicalize(s) == s)
        n_canon += T.is_canonical(row, k)
    assert 10 < n_canon < 50
    read = "".join(rng.choice(list("ACGT"), k + 9))
    assert T.window_keys(read, k) == [KT.key_int(oracle.canonicalize(read[i:i + k])) for i in range(10)]


def distinct(rows):
    return len(np.unique(rows, axis=0)) == len(rows)


@pytest.mark.parametrize("k", (65, 95, 127, 159, 191, 201))
def test_generators(k):
    rng = np.random.default_rng(200 + k)
    W, tb = T.W_of(k), T.top_width(k)
    h = int(T._rand64(rng, 1)[0])
    for canonical in (False, True):
        # one key per hash
        hs = T._rand64(rng, 50)
        rows = T.rows_with_hash(hs, k, 50, rng, canonical=canonical)
        assert rows.shape == (50, W) and distinct(rows) and T.valid_rows(rows, k).all()
        assert np.array_equal(T.long_hash(rows), hs)
        assert not canonical or all(T.is_canonical(r, k) for r in rows)
        # a collision group with one top word
        rows = T.rows_with_hash(h, k, 40, rng, share="top", canonical=canonical)
        assert distinct(rows) and T.valid_rows(rows, k).all() and (T.long_hash(rows) == np.uint64(h)).all()
        assert len(set(rows[:, W - 1].tolist())) == 1
        assert not canonical or all(T.is_canonical(r, k) for r in rows)
        # rows that differ in exactly one middle word (and in w0, which the hash fixes)
        for j in range(1, W - 1):
            rows = T.rows_with_hash(h, k, 65, rng, share=("middle", j), canonical=canonical, top=5 % (1 << (tb - 2)))
            assert distinct(rows) and T.valid_rows(rows, k).all() and (T.long_hash(rows) == np.uint64(h)).all()
            for jj in range(1, W):
                assert (len(set(rows[:, jj].tolist())) == 1) == (jj != j)
            assert int(rows[0, W - 1]) == 5 % (1 << (tb - 2))
            assert not canonical or all(T.is_canonical(r, k) for r in rows)
        # rows that differ in the top word only
        n = 2 if tb == 2 else 30
        rows = T.rows_with_hash(h, k, n, rng, share="middles", canonical=canonical)
        assert distinct(rows) and T.valid_rows(rows, k).all() and (T.long_hash(rows) == np.uint64(h)).all()
        assert len(set(rows[:, W - 1].tolist())) == n
        for jj in range(1, W - 1):
            assert len(set(rows[:, jj].tolist())) == 1
        assert not canonical or all(T.is_canonical(r, k) for r in rows)
        # rows that differ in w0 only: one home slot, a hash each
        rows = T.rows_with_hash(lambda m: T.hash_with(rng, m, top_bits=0x5A5A5, nbits=20), k, 30, rng, share="upper", canonical=canonical)
        assert distinct(rows) and T.valid_rows(rows, k).all() and len(np.unique(rows[:, 1:], axis=0)) == 1
        hs = T.long_hash(rows)
        assert len(set(hs.tolist())) == 30 and (T.home(hs, 20) == 0x5A5A5).all()
        assert not canonical or all(T.is_canonical(r, k) for r in rows)


def test_acceptance_of_canonical_draws():
    """With the first base forced to A about 0.87 of the draws are canonical (the rest end in T and lose the tie)."""
    rng = np.random.default_rng(5)
    for k in (97, 201):
        W, tb = T.W_of(k), T.top_width(k)
        rows = T._rand64(rng, (400, W))
        rows[:, W - 1] &= np.uint64((1 << (tb - 2)) - 1)
        acc = np.mean([T.is_canonical(r, k) for r in rows])
        assert 0.8 < acc < 0.94


def test_hash_with():
    rng = np.random.default_rng(6)
    h = T.hash_with(rng, 100, top_bits=0x3D7, nbits=10, owner16=0x8000, slice16=np.arange(100))
    assert (T.home(h, 10) == 0x3D7).all() and (T.owner(h, 2) == 1).all() and ((h & np.uint64(0xFFFF)) == np.arange(100)).all()
    assert len(set(h.tolist())) == 100                             # the other bits are random
    h = T.hash_with(rng, 3, owner16=np.array([0, 1, 0xFFFF]), fill=1)
    assert h.tolist() == [0xFFFFFFFF0000FFFF, 0xFFFFFFFF0001FFFF, M64]
    h = T.hash_with(rng, 2, slice16=7, fill=0)
    assert h.tolist() == [7, 7]
    h = T.hash_with(rng, 4, top_bits=np.arange(4), nbits=12, low22=0x2ABCDE)
    assert (T.home(h, 12) == np.arange(4)).all() and ((h & np.uint64((1 << 22) - 1)) == 0x2ABCDE).all()
    w, b1, b2 = T.sieve_word_bits(h, 1023)
    assert len(set(w.tolist())) == 1 and len(set(b1.tolist())) == 1 and len(set(b2.tolist())) == 1


def test_sort_rows():
    rows = np.array([[5, 0, 1], [4, 0, 1], [9, 9, 0], [0, 1, 0]], np.uint64)
    srt, cnt = T.sort_rows(rows, np.array([1, 2, 3, 4]))
    assert srt.tolist() == [[0, 1, 0], [9, 9, 0], [4, 0, 1], [5, 0, 1]] and cnt.tolist() == [4, 3, 2, 1]
