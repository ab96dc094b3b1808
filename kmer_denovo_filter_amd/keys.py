"""The host-side k-mer key codec: the one place that knows how a key is laid out.

A k-mer is Jellyfish's value of it: A=0 C=1 G=2 T=3, base i at bits ``2(k-1-i)``, so the last base holds bits 0-1.
The value is cut into W = ceil(2k/64) uint64 words, word 0 the least significant (bit ``b`` is bit ``b & 63`` of word
``b >> 6``), and a canonical key is the numeric minimum of the forward and the reverse-complement value.  A record of an
index holds the value as ceil(2k/8) little-endian bytes.

Here a key set is a sequence of W uint64 arrays of one length, ``words[j]`` holding word j of every key: a (W, n)
array -- row j contiguous when built word by word, or the transpose of (n, W) rows -- or a tuple of 1-D arrays.
Callers hold the same keys in their own form, which `to_pair` / `from_pair` convert: ``(lo, hi)`` for k <= 63 (hi all
zeros or None for k <= 32) and ``((n, W) rows, None)`` for long k-mers (odd k from 65 to 201).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

_ENC = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _ENC[_c] = _i
    _ENC[_c + 32] = _i          # lower case
_DEC = np.frombuffer(b"ACGT", dtype=np.uint8)


def key_words(k: int) -> int:
    """Words per key of an engine for k: 1 (k <= 32), 2 (33..63), ceil(2k/64) for odd 65..201; 0 if no engine takes k
    (the rule of ``kdf_key_words``, restated so that it is checked before any device call)."""
    k = int(k)
    if 1 <= k <= 32:
        return 1
    if 33 <= k <= 63:
        return 2
    if 65 <= k <= 201 and k % 2 == 1:
        return (2 * k + 63) // 64
    return 0


def n_words(k: int) -> int:
    """W of the codec: the words a 2k-bit value needs."""
    return (2 * int(k) + 63) // 64


def encode(chars: np.ndarray) -> np.ndarray:
    """ASCII bases -> 2-bit codes (uint8, same shape); 255 where a byte is not A/C/G/T in either case."""
    return _ENC[chars]


def from_codes(codes: np.ndarray, canonical: bool = True) -> np.ndarray:
    """2-bit codes (n, k), all 0..3 -> (W, n) words of the forward value, or with ``canonical`` of the numeric minimum
    of the forward and the reverse-complement value."""
    n, k = codes.shape
    by_base = np.ascontiguousarray(codes.T)              # (k, n): base i of every key, contiguous
    f = np.zeros((n_words(k), n), np.uint64)
    r = np.zeros_like(f)
    for i in range(k):
        c = by_base[i].astype(np.uint64)
        sh = 2 * (k - 1 - i)
        f[sh >> 6] |= c << np.uint64(sh & 63)
        if canonical:                                    # the reverse complement holds 3 - c at bits 2i
            rs = 2 * i
            r[rs >> 6] |= (np.uint64(3) - c) << np.uint64(rs & 63)
    if not canonical:
        return f
    le = np.ones(n, bool)
    for fj, rj in zip(f, r):                             # up to the top word, which decides last
        le = (fj < rj) | ((fj == rj) & le)
    return np.where(le, f, r)


def to_ascii(words, k: int) -> np.ndarray:
    """Key words -> (n, k) uint8 ASCII bases."""
    by_base = np.empty((k, len(words[0])), dtype=np.uint8)   # (k, n): base i of every key, contiguous
    for i in range(k):
        sh = 2 * (k - 1 - i)
        by_base[i] = _DEC[((words[sh >> 6] >> np.uint64(sh & 63)) & np.uint64(3)).astype(np.intp)]
    return np.ascontiguousarray(by_base.T)


def bit(words, b: int) -> np.ndarray:
    """Bit ``b`` of every key (bit 0 = the last base's low bit), as uint64 0 / 1."""
    return (words[b >> 6] >> np.uint64(b & 63)) & np.uint64(1)


def order(words, major: Optional[np.ndarray] = None) -> np.ndarray:
    """Indices that put a key set in ascending key order; with ``major``, in ascending ``major`` order first."""
    return np.lexsort(tuple(words) + (() if major is None else (major,)))   # (np.lexsort: the last sort key leads)


def _rows(words) -> np.ndarray:
    """(n, W) C-contiguous uint64 rows; no copy when ``words`` is the transpose of such rows."""
    if isinstance(words, np.ndarray):
        return np.ascontiguousarray(words.T, dtype="<u8")
    return np.stack(words, axis=1).astype("<u8", copy=False)


def to_bytes(words, k: int) -> np.ndarray:
    """Key words -> (n, ceil(2k/8)) uint8: each key's little-endian record bytes."""
    return _rows(words).view(np.uint8)[:, :(2 * k + 7) // 8]


def from_bytes(kbytes: np.ndarray) -> np.ndarray:
    """(n, kb) little-endian record bytes -> (W, n) key words, W = ceil(kb/8)."""
    n, kb = kbytes.shape
    W = (kb + 7) // 8
    if kb != 8 * W:
        padded = np.zeros((n, 8 * W), np.uint8)
        padded[:, :kb] = kbytes
        kbytes = padded
    return np.ascontiguousarray(kbytes).view("<u8").reshape(n, W).astype(np.uint64, copy=False).T


def to_pair(words, zero_hi: bool = True):
    """Key words -> the callers' form: ``(lo, hi)`` for W <= 2, hi all zeros for W = 1 (None when not ``zero_hi``);
    ``((n, W) rows, None)`` for long keys.  C-contiguous uint64 arrays."""
    if len(words) > 2:
        return _rows(words), None
    lo = np.ascontiguousarray(words[0])
    if len(words) == 2:
        return lo, np.ascontiguousarray(words[1])
    return lo, (np.zeros(len(lo), np.uint64) if zero_hi else None)


def from_pair(lo, hi: Optional[np.ndarray] = None, k: Optional[int] = None):
    """The callers' form -> key words (no copy).  W = n_words(k); without k, W comes from the form: the width of
    (n, W) rows, else 2 with a ``hi`` array and 1 without.  A ``hi`` of None reads as all zeros; hi is unused at W = 1."""
    lo = np.asarray(lo, np.uint64)
    if k is not None:
        W = n_words(k)
    else:
        W = lo.shape[1] if lo.ndim == 2 else 1 if hi is None else 2
    if W > 2:
        return lo.reshape(len(lo), W).T
    if W == 1:
        return (lo,)
    return lo, (np.zeros(len(lo), np.uint64) if hi is None else np.asarray(hi, np.uint64))
