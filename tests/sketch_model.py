"""The MODEL of the distinct k-mer sketch, restated from ``include/kdf.h`` ("distinct k-mer sketch") alone: no engine, no
package import.  Canonical keys come from the oracle's string rules (``kmer_truth.count_truth`` = ``oracle.py_count``).

    h      the key's stored form: mix64(key) for k <= 32, mix64(lo ^ rotl(hi, 37)) for 33 <= k <= 63, mix64(w0 ^ f) with
           f = 0; f = mix64(f ^ w_j) + 0x632BE59BD9B4E019 for j = W - 1 .. 1 for long keys;
           mix64(x) = (x ^ (x >> 32)) * 0x9FB21C651E98DF25 mod 2^64
    x      h, or h + hi * 0xD6E8FEB86659FD93 for 33 <= k <= 63
    g      x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
    j      g >> (64 - p)
    r      1 + clz((g << p) | (1 << (p - 1)))                      (64-bit)
    reg[j] max r over the sketched windows -- a max, so the DISTINCT canonical keys of the stream decide it

    estimate: m = 2^p, alpha = 0.7213 / (1 + 1.079 / m), E = alpha m^2 / sum 2^-reg (index order);
              E <= 2.5 m and V = #{reg = 0} > 0: E = m ln(m / V)
"""
import math

import numpy as np

M64 = (1 << 64) - 1
MUL = 0x9FB21C651E98DF25
FOLD_ADD = 0x632BE59BD9B4E019
HI_MUL = 0xD6E8FEB86659FD93
U = np.uint64


def key_words(k):
    return 1 if k <= 32 else 2 if k <= 63 else (2 * k + 63) // 64


def _mul(x, c):
    with np.errstate(over="ignore"):
        return x * U(c)


def _add(x, y):
    with np.errstate(over="ignore"):
        return x + y


def mix64(x):
    x = x ^ (x >> U(32))
    return _mul(x, MUL)


def fin(x):
    x = x ^ (x >> U(30))
    x = _mul(x, 0xBF58476D1CE4E5B9)
    x = x ^ (x >> U(27))
    x = _mul(x, 0x94D049BB133111EB)
    return x ^ (x >> U(31))


def g_of_keys(keys, k):
    """g of canonical keys given as Python ints of 2k bits -> uint64 array"""
    W = key_words(k)
    w = np.array([[(v >> (64 * j)) & M64 for j in range(W)] for v in keys], dtype=np.uint64).reshape(len(keys), W)
    if W == 1:
        return fin(mix64(w[:, 0]))
    if W == 2:
        hi = w[:, 1]
        h = mix64(w[:, 0] ^ ((hi << U(37)) | (hi >> U(27))))
        return fin(_add(h, _mul(hi, HI_MUL)))
    f = np.zeros(len(keys), dtype=np.uint64)
    for j in range(W - 1, 0, -1):
        f = _add(mix64(f ^ w[:, j]), U(FOLD_ADD))
    return fin(mix64(w[:, 0] ^ f))


def clz64(v):
    """leading zeros of non-zero uint64 values"""
    v = v.copy()
    n = np.zeros(len(v), dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        t = (v >> U(64 - s)) == 0
        n[t] += s
        v[t] = v[t] << U(s)
    return n


def registers_of_g(g, p):
    g = np.asarray(g, dtype=np.uint64)
    regs = np.zeros(1 << p, dtype=np.uint8)
    if len(g) == 0:
        return regs
    j = (g >> U(64 - p)).astype(np.int64)
    r = 1 + clz64((g << U(p)) | U(1 << (p - 1)))
    assert r.min() >= 1 and r.max() <= 65 - p
    np.maximum.at(regs, j, r.astype(np.uint8))
    return regs


def registers_of_keys(keys, k, p):
    return registers_of_g(g_of_keys(list(keys), k), p)


def registers_of_reads(reads, k, p):
    from kmer_truth import count_truth
    return registers_of_keys(count_truth(reads, k).keys(), k, p)


def estimate(regs):
    regs = np.asarray(regs, dtype=np.uint8)
    m = len(regs)
    s = 0.0
    for v in regs.tolist():                     # index order, as the engine sums
        s += math.ldexp(1.0, -v)
    e = 0.7213 / (1 + 1.079 / m) * m * m / s
    zeros = int((regs == 0).sum())
    if e <= 2.5 * m and zeros > 0:
        e = m * math.log(m / zeros)
    return e


def hll_bound(p):
    """five standard errors of HyperLogLog"""
    return 5 * 1.04 / math.sqrt(1 << p)


def linear_bound(n, p):
    """five standard errors of linear counting at n distinct keys in m registers (Whang et al. 1990):
    sqrt(m (e^t - t - 1)) / n with t = n / m"""
    m = float(1 << p)
    t = n / m
    return 5 * math.sqrt(m * (math.exp(t) - t - 1)) / n


def prefix_reads(reads, n):
    """The reads a stream of ``reads`` (each followed by one separator position) holds below position n: a prefix may
    cut a read."""
    out, pos = [], 0
    for r in reads:
        if pos >= n:
            break
        out.append(r[:n - pos])
        pos += len(r) + 1
    return out


def valid_windows(reads, k):
    n = 0
    for s in reads:
        run = 0
        for ch in s.upper():
            run = run + 1 if ch in "ACGT" else 0
            n += run >= k
    return n
