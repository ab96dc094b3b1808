"""Long k-mers (odd k from 65 to 201) on the host: the W-word canonicaliser against the oracle's string rules, the
kdf/sorted and k-mer FASTA codecs (also at k <= 63), and the range checks that run before any device call (no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest

from kmer_denovo_filter_amd import KmerEngine, _native
from kmer_denovo_filter_amd.engine import key_words, mirror_engine
from kmer_denovo_filter_amd import jf_io, kmer_fasta

KS = (65, 95, 97, 127, 129, 159, 161, 191, 193, 201)
M64 = (1 << 64) - 1


def words_of(v: int, W: int):
    return [(v >> (64 * j)) & M64 for j in range(W)]


def canonical_rows(kmers, k, O):
    W = (2 * k + 63) // 64
    return np.array([words_of(O.kmer_to_int(O.canonicalize(s.upper())), W) for s in kmers], dtype=np.uint64).reshape(-1, W)


def as_pair(rows, k):
    """The (lo, hi) form the helpers take and return for (n, W) rows: (rows, None) for long k, else words 0 and 1
    (hi all zeros for k <= 32)."""
    if k > 63:
        return rows, None
    hi = rows[:, 1] if rows.shape[1] > 1 else np.zeros(len(rows), np.uint64)
    return np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(hi)


def same_hi(got, want, k):
    return got is None if k > 63 else np.array_equal(got, want)


def c_canonical_w(kmer: str, k: int):
    lib = _native.load()
    W = (2 * k + 63) // 64
    out = (ctypes.c_uint64 * W)()
    rc = lib.kdf_canonical_w(kmer.encode(), k, out)
    return rc, [int(x) for x in out]


@pytest.mark.parametrize("k", KS)
def test_canonical_w_matches_string_rule(k, oracle):
    rng = np.random.default_rng(k)
    W = (2 * k + 63) // 64
    kmers = ["".join(rng.choice(list("ACGT"), k)) for _ in range(200)]
    kmers += ["A" * k, "T" * k, "C" * k, "G" * k, "acgt" * (k // 4) + "a" * (k % 4)]
    for s in kmers:
        rc, got = c_canonical_w(s, k)
        assert rc == 0
        assert got == words_of(oracle.kmer_to_int(oracle.canonicalize(s.upper())), W), s
    assert c_canonical_w("A" * (k - 1) + "N", k)[0] == _native.KDF_ERR_INVALID


def test_canonical_w_small_k_agrees_with_lo_hi_form(oracle):
    lib = _native.load()
    rng = np.random.default_rng(1)
    for k in (1, 5, 31, 32, 33, 63):
        for _ in range(20):
            s = "".join(rng.choice(list("ACGT"), k))
            lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
            assert lib.kdf_canonical(s.encode(), k, ctypes.byref(lo), ctypes.byref(hi)) == 0
            rc, w = c_canonical_w(s, k)
            assert rc == 0 and w[0] == lo.value and (k <= 32 or w[1] == hi.value)


def test_key_words():
    lib = _native.load()
    for k in range(0, 210):
        want = 1 if 1 <= k <= 32 else 2 if 33 <= k <= 63 else ((2 * k + 63) // 64 if 65 <= k <= 201 and k % 2 else 0)
        assert lib.kdf_key_words(k) == want, k
        assert key_words(k) == want, k
    assert [lib.kdf_key_words(k) for k in (65, 95, 97, 127, 129, 159, 161, 191, 193, 201)] == [3, 3, 4, 4, 5, 5, 6, 6, 7, 7]


@pytest.mark.parametrize("k", (64, 100, 202, 0, 203, 66))
def test_engine_refuses_k_before_any_device_call(k, monkeypatch):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_native, "load", boom)
    with pytest.raises(ValueError):
        KmerEngine(k)


def test_multi_rank_mirrors_and_vcf_mode_refuse_long_k_before_any_device_call(monkeypatch, tmp_path):
    from kmer_denovo_filter_amd import dist_env
    from kmer_denovo_filter_amd.vcf.pipeline import _collect_child_kmers

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_native, "load", boom)
    monkeypatch.setattr(dist_env, "world_rank", lambda: (2, 1, True))
    with pytest.raises(ValueError, match="k <= 63"):
        mirror_engine(101)
    with pytest.raises(ValueError, match="VCF mode takes k <= 63"):
        _collect_child_kmers("child.bam", None, [], 101, 20, 20, False, str(tmp_path / "c.fa"))


@pytest.mark.parametrize("k", (1, 5, 31, 32, 33, 63, 101, 201))
def test_kdf_sorted_round_trip(k, tmp_path, oracle):
    rng = np.random.default_rng(k)
    kmers = ["".join(rng.choice(list("ACGT"), k)) for _ in range(300)]
    rows = np.unique(canonical_rows(kmers, k, oracle), axis=0)
    order = np.lexsort(rows.T)                     # ascending: the top word is the primary key
    rows = np.ascontiguousarray(rows[order])
    counts = rng.integers(0, 1 << 32, len(rows), dtype=np.uint64).astype(np.uint32)
    lo, hi = as_pair(rows, k)
    path = str(tmp_path / "idx.jf")
    jf_io.write_index(path, k, lo, hi, counts)
    header, off = jf_io.read_header(path)
    kb = (2 * k + 7) // 8
    assert header["key_len"] == 2 * k and header["format"] == jf_io.KDF_FORMAT
    assert os.path.getsize(path) - off == len(rows) * (kb + 4)
    assert jf_io.index_records(path) == len(rows)
    kk, keys, rhi, cnt = jf_io.read_index(path, expect_k=k)
    assert kk == k and same_hi(rhi, hi, k)
    assert np.array_equal(keys, lo) and np.array_equal(cnt, counts)
    blocks = list(jf_io.iter_index(path, chunk_records=64))
    assert np.array_equal(np.concatenate([b[1] for b in blocks]), lo)
    # record i's bytes are the Jellyfish value little-endian
    raw = open(path, "rb").read()[off:off + kb]
    assert int.from_bytes(raw, "little") == sum(int(x) << (64 * j) for j, x in enumerate(rows[0]))


@pytest.mark.parametrize("k", (1, 5, 31, 32, 33, 63, 65, 101, 201))
def test_kmer_fasta_round_trip(k, tmp_path, oracle):
    rng = np.random.default_rng(k + 5)
    kmers = ["".join(rng.choice(list("ACGT"), k)) for _ in range(100)]
    rows = canonical_rows(kmers, k, oracle)
    lo, hi = as_pair(rows, k)
    for sidecar in (False, True):
        path = str(tmp_path / f"k{sidecar}.fa")
        assert kmer_fasta.write_kmer_fasta(path, lo, hi, k, sidecar=sidecar) == len(rows)
        text = open(path).read().split("\n")
        assert text[0] == ">0" and text[1] == oracle.canonicalize(kmers[0])
        assert text[1::2][:len(kmers)] == [oracle.canonicalize(s) for s in kmers]
        keys, rhi = kmer_fasta.read_kmer_fasta_keys(path, k)
        assert same_hi(rhi, hi, k) and np.array_equal(keys, lo)
    # a file of forward k-mers, canonicalised on read
    path = str(tmp_path / "fwd.fa")
    with open(path, "w") as fh:
        fh.write("".join(f">{i}\n{s}\n" for i, s in enumerate(kmers)))
    keys, rhi = kmer_fasta.read_kmer_fasta_keys(path, k)
    assert np.array_equal(keys, lo) and same_hi(rhi, hi, k)
    fwd, fhi = kmer_fasta.read_kmer_fasta_keys(path, k, canonical=False)
    flo, want_hi = as_pair(np.array([words_of(oracle.kmer_to_int(s), rows.shape[1]) for s in kmers], np.uint64), k)
    assert np.array_equal(fwd, flo) and same_hi(fhi, want_hi, k)


def test_jellyfish_writer_refuses_long_k(tmp_path):
    rows = np.zeros((2, 4), np.uint64)
    with pytest.raises(ValueError, match="k <= 63"):
        jf_io.write_jellyfish_index(str(tmp_path / "x.jf"), 101, rows, None, np.ones(2, np.uint32))


ALL_K = tuple(range(1, 64)) + tuple(range(65, 202, 2))


def test_record_bytes_and_ascii_round_trip_at_every_k(tmp_path, oracle):
    """At every k the engine takes: a kdf/sorted record holds the k-mer's value (``kmer_to_int``) as little-endian
    bytes (the Jellyfish writer's records too, k <= 63); ASCII -> key -> ASCII and the k-mer FASTA give the k-mers back;
    and bit b of a key (the Jellyfish hash position) is bit b of the value."""
    from kmer_denovo_filter_amd import keys_to_kmers, kmers_to_keys
    rng = np.random.default_rng(7)
    for k in ALL_K:
        kmers = sorted({"".join(rng.choice(list("ACGT"), k)) for _ in range(6)}, key=oracle.kmer_to_int)
        vals = [oracle.kmer_to_int(s) for s in kmers]
        lo, hi = kmers_to_keys(kmers, k, canonical=False)
        assert keys_to_kmers(lo, hi, k) == kmers, k
        path = str(tmp_path / f"k{k}.jf")
        jf_io.write_index(path, k, lo, hi, np.arange(len(kmers), dtype=np.uint32))
        _, off = jf_io.read_header(path)
        kb = (2 * k + 7) // 8
        raw = open(path, "rb").read()[off:]
        assert [int.from_bytes(raw[i * (kb + 4):i * (kb + 4) + kb], "little") for i in range(len(kmers))] == vals, k
        fa = str(tmp_path / f"k{k}.fa")
        kmer_fasta.write_kmer_fasta(fa, lo, hi, k, sidecar=False)
        assert open(fa).read().split("\n")[1::2][:len(kmers)] == kmers, k
        # columns that put bit b of the key at bit b % 64 of the position: the XOR of the value's 64-bit words
        cols = [1 << ((2 * k - 1 - i) % 64) for i in range(2 * k)]
        fold = [0] * len(vals)
        for i, v in enumerate(vals):
            while v:
                fold[i] ^= v & M64
                v >>= 64
        assert jf_io.jf_positions(cols, 2 * k, lo, hi).tolist() == fold, k
        if k <= 63:
            jf_io.write_jellyfish_index(path, k, lo, hi, np.ones(len(kmers), np.uint32))
            _, off = jf_io.read_header(path)
            raw = open(path, "rb").read()[off:]
            assert sorted(int.from_bytes(raw[i * (kb + 4):i * (kb + 4) + kb], "little") for i in range(len(kmers))) == vals, k
