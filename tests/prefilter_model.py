"""The MODEL of the two-pass count's sieve, computed from a truth alone (no engine, no package import).

The cell rule is restated from ``include/kdf.h`` ("two-pass counting"), as ``distributed.owner_of`` restates the owner
hash: cell(key) = h >> (64 - s), the top s bits of the key's 64-bit stored form

    k <= 32        h = mix64(key)                          mix64(x) = (x ^ (x >> 32)) * 0x9FB21C651E98DF25 mod 2^64
    33 <= k <= 63  h = mix64(lo ^ rotl(hi, 37))
    odd 65..201    h = mix64(w0 ^ f),  f = 0;  f = mix64(f ^ w_j) + 0x632BE59BD9B4E019  for j = W - 1 .. 1

value(cell) = min(sum of the truth's counts over the keys of the cell, 3); a key is admitted iff value(cell(key)) >= L;
the table of a gated count holds exactly the admitted keys with their full counts.

Three forms of the same rule: ``cell_of`` (one key, Python ints, any k: the brute force), ``cells_np`` (numpy uint64
arrays, k <= 63) and ``cells_torch`` (int64 tensors holding the bit patterns, k <= 63, any device: full-size truths).
"""
import numpy as np

M64 = (1 << 64) - 1
MUL = 0x9FB21C651E98DF25
FOLD_ADD = 0x632BE59BD9B4E019


def key_words(k):
    return 1 if k <= 32 else 2 if k <= 63 else (2 * k + 63) // 64


def mix64(x):
    x ^= x >> 32
    return (x * MUL) & M64


def stored_form(key, k):
    """h of one canonical key (a Python int of 2k bits)"""
    W = key_words(k)
    w = [(key >> (64 * j)) & M64 for j in range(W)]
    if W == 1:
        return mix64(w[0])
    if W == 2:
        return mix64(w[0] ^ (((w[1] << 37) | (w[1] >> 27)) & M64))
    f = 0
    for j in range(W - 1, 0, -1):
        f = (mix64(f ^ w[j]) + FOLD_ADD) & M64
    return mix64(w[0] ^ f)


def cell_of(key, k, s):
    return stored_form(key, k) >> (64 - s)


def model(truth, k, s, L):
    """truth {key int: count} -> (admitted {key: count}, [cells reading 0, 1, 2, 3]) -- the brute force: a dict of cells"""
    cells = {}
    for key, c in truth.items():
        cell = cell_of(key, k, s)
        cells[cell] = cells.get(cell, 0) + c
    by_value = [0, 0, 0, 0]
    for v in cells.values():
        by_value[min(v, 3)] += 1
    by_value[0] = (1 << s) - len(cells)
    admitted = {key: c for key, c in truth.items() if min(cells[cell_of(key, k, s)], 3) >= L}
    return admitted, by_value


# ---- numpy, k <= 63 ----------------------------------------------------------------------------------------------------

def cells_np(lo, hi, k, s):
    lo = np.asarray(lo, dtype=np.uint64)
    x = lo.copy()
    if k > 32:
        hi = np.asarray(hi, dtype=np.uint64)
        x ^= (hi << np.uint64(37)) | (hi >> np.uint64(27))
    x ^= x >> np.uint64(32)
    with np.errstate(over="ignore"):
        x = x * np.uint64(MUL)
    return x >> np.uint64(64 - s)


def model_np(lo, hi, counts, k, s, L):
    """arrays of a truth -> (bool admitted per key, [cells reading 0, 1, 2, 3])"""
    cells = cells_np(lo, hi, k, s).astype(np.int64)
    sums = np.bincount(cells, weights=np.minimum(np.asarray(counts, dtype=np.int64), 3), minlength=1 << s).astype(np.int64)
    value = np.minimum(sums, 3)
    by_value = np.bincount(value, minlength=4)
    return value[cells] >= L, [int(v) for v in by_value]


# ---- torch, k <= 63: int64 tensors hold the 64-bit patterns (multiplication wraps, right shifts are masked) -------------

def _lsr(x, n):
    return (x >> n) & ((1 << (64 - n)) - 1) if n else x


def cells_torch(lo, hi, k, s):
    x = lo
    if k > 32:
        x = x ^ ((hi << 37) | _lsr(hi, 27))
    x = x ^ _lsr(x, 32)
    x = x * (MUL - (1 << 64))                    # the multiplier as a signed 64-bit number: the product wraps mod 2^64
    return _lsr(x, 64 - s)


def model_torch(lo, hi, counts, k, s, L):
    """(lo, hi, counts) int64 tensors of a truth -> (bool admitted per key, [cells reading 0, 1, 2, 3])"""
    import torch
    cells = cells_torch(lo, hi, k, s)
    sums = torch.zeros(1 << s, dtype=torch.int32, device=lo.device)
    sums.index_add_(0, cells, counts.clamp(max=3).to(torch.int32))       # (a clamped sum reaches 3 iff the sum does)
    value = sums.clamp_(max=3)
    by_value = [int((value == v).sum()) for v in range(4)]          # (four compares: torch.bincount is not made for 2^30 elements)
    return value[cells] >= L, by_value
