"""The MODEL of the merge of counting sieves (include/kdf.h "two-pass counting", several ranks), in numpy alone: no
engine, no package import.

A sieve word holds sixteen cells, cell c in bits [4 (c & 15), +4).  value(nibble) = popcount(bits 0..2) -- bit 3 is
ignored, a non-thermometer code such as 0b101 reads as 2.  merge: new = min(own + sum of the segments' values, 3)
(``replace``: the own value is left out), written as the thermometer code 0 / 1 / 3 / 7.
"""
import numpy as np

CODE = np.array([0, 1, 3, 7], dtype=np.uint64)


def values(words):
    """uint64[n] -> int64[n, 16]: the value of every cell"""
    w = np.asarray(words, dtype=np.uint64)
    nib = (w[:, None] >> (np.arange(16, dtype=np.uint64) * np.uint64(4))[None, :]) & np.uint64(0xF)
    nib = nib.astype(np.int64)
    return (nib & 1) + ((nib >> 1) & 1) + ((nib >> 2) & 1)


def encode(vals):
    """int64[n, 16] values 0..3 -> uint64[n] words of thermometer codes"""
    codes = CODE[np.asarray(vals, dtype=np.int64)]
    return np.bitwise_or.reduce(codes << (np.arange(16, dtype=np.uint64) * np.uint64(4))[None, :], axis=1)


def merge(own, segments, replace=False):
    """own uint64[n], segments a list of uint64[n] -> the merged uint64[n]"""
    own = np.asarray(own, dtype=np.uint64)
    total = np.zeros((len(own), 16), dtype=np.int64) if replace else values(own)
    for s in segments:
        assert len(s) == len(own)
        total = total + values(s)
    return encode(np.minimum(total, 3))


def merge_slice(sieve, first, segments, replace=False):
    """the whole sieve after a merge of `segments` into words [first, first + len): words outside are unchanged"""
    out = np.array(sieve, dtype=np.uint64, copy=True)
    n = len(segments[0]) if segments else 0
    if n:
        out[first:first + n] = merge(out[first:first + n], segments, replace)
    return out


def fill(words):
    """[cells reading 0, 1, 2, 3]"""
    return [int(x) for x in np.bincount(values(words).ravel(), minlength=4)]


def valid_codes(words):
    """every nibble is one of 0 / 1 / 3 / 7"""
    w = np.asarray(words, dtype=np.uint64)
    nib = (w[:, None] >> (np.arange(16, dtype=np.uint64) * np.uint64(4))[None, :]) & np.uint64(0xF)
    return bool(np.isin(nib, CODE).all())
