"""The sizing rule of the bin-major sieve (option ``sieve_bins``): ``kdf_bin_sieve_geometry`` is a pure host function of
libkdf, so this needs no device.  It is checked against a restatement of the rule in a few lines of Python."""
import pytest

from kmer_denovo_filter_amd import _native
from kmer_denovo_filter_amd.engine import bin_sieve_geometry

CAP = 1 << 14            # words: 128 KB of one CU's 160 KB of LDS, the rest holds the kernel's queues and run table
NS = (1, 10**3, 10**6, 16 << 20, 10**8, 260_000_000, 10**9)
BINS = (1, 4, 5, 6, 7, 8, 9, 10)


def pow2ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def rule(n, sieve_bits, sieve_bins):
    """(c1, slice_words, bits_per_key) or None"""
    def slice_words(bpk, c1):
        return max(128, pow2ceil((n * bpk + 63) // 64) >> c1)
    bpk = sieve_bits or (8 if slice_words(8, 10) <= CAP else 4)
    for c1 in (range(4, 11) if sieve_bins == 1 else (sieve_bins,)):
        if slice_words(bpk, c1) <= CAP:
            return c1, slice_words(bpk, c1), bpk
    return None


@pytest.mark.parametrize("kw", (1, 2))
@pytest.mark.parametrize("bins", BINS)
def test_geometry_matches_the_rule(kw, bins):
    for n in NS:
        for bits in (0, 1, 4, 16, 32):
            want = rule(n, bits, bins)
            if want is None:
                with pytest.raises(_native.KdfError):
                    bin_sieve_geometry(n, kw, bits, bins)
                continue
            c1, sw, bpk = bin_sieve_geometry(n, kw, bits, bins)
            assert (c1, sw, bpk) == want, (n, kw, bits, bins)
            assert 4 <= c1 <= 10 and 128 <= sw <= CAP and sw & (sw - 1) == 0
            assert (sw << c1) * 64 >= n * bpk or sw == 128
            if bins != 1:
                assert c1 == bins


def test_auto_bits_and_refusals():
    assert bin_sieve_geometry(1, 1) == (4, 128, 8)
    assert bin_sieve_geometry(10**6, 1) == (4, 8192, 8)
    assert bin_sieve_geometry(16 << 20, 2) == (7, CAP, 8)                 # 16 M keys x 8 bits = 2^21 words
    assert bin_sieve_geometry(10**8, 1) == (10, CAP, 8)                   # 1.6 x 2^23 words -> 2^24
    assert bin_sieve_geometry(260_000_000, 2) == (10, CAP, 4)             # 8 bits per key no longer fit: 4
    for kw in (1, 2):
        with pytest.raises(_native.KdfError):                             # below 4 bits per key
            bin_sieve_geometry(10**9, kw)
        with pytest.raises(_native.KdfError):
            bin_sieve_geometry(10**9, kw, sieve_bins=10)
        for bins in (2, 3, 11, 0, -1):
            with pytest.raises(_native.KdfError):
                bin_sieve_geometry(1000, kw, 0, bins)
    assert bin_sieve_geometry(10**9, 1, sieve_bits=1) == (10, CAP, 1)     # an explicit sieve_bits is honoured
    with pytest.raises(_native.KdfError):
        bin_sieve_geometry(10**8, 1, sieve_bins=8)                        # an explicit c1 whose slice would not fit
    for kw in (0, 3, 4):
        with pytest.raises(_native.KdfError):
            bin_sieve_geometry(1000, kw)


def test_out_pointers_may_be_null():
    lib = _native.load()
    assert lib.kdf_bin_sieve_geometry(1000, 1, 0, 1, None, None, None) == _native.KDF_OK
    assert lib.kdf_bin_sieve_geometry(10**9, 1, 0, 1, None, None, None) == _native.KDF_ERR_INVALID
