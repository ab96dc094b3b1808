"""Plain-Python truth for counts and the Module-3 scan at any k (long k-mers included, where the C oracle stops).

Built on the oracle's string rules (``py_count``, ``canonicalize``; keys as ``kmer_to_int`` encodes them) and pinned to
``OracleTable`` at k <= 63 by ``tests/test_kmer_truth.py``, so that the long-k expectations rest on something checked.
Keys are Python ints; ``rows``/``int_of_row`` convert to and from the engine's long-key layout ((n, W) uint64 rows, word
0 the least significant), ``lohi`` to the (lo, hi) pair of k <= 63."""
import numpy as np

from oracle import oracle as O

M64 = (1 << 64) - 1
_DIGITS = str.maketrans("ACGT", "0123")


def key_int(kmer: str) -> int:
    """``kmer_to_int`` of an upper-case ACGT k-mer (A=0 C=1 G=2 T=3, leftmost base most significant), in one call."""
    return int(kmer.translate(_DIGITS), 4)


def count_truth(reads, k, filt=None) -> dict:
    """{canonical key: count} by ``py_count`` (``filt``: the canonical keys of a --if filter, as ints)."""
    fs = None if filt is None else {O.int_to_kmer(v, k) for v in filt}
    return {key_int(s): c for s, c in O.py_count(reads, k, fs).items()}


def sorted_items(d: dict):
    """(ascending keys, uint32 counts) of a {key: count} dict."""
    ks = sorted(d)
    return ks, np.array([d[v] for v in ks], dtype=np.uint32)


def scan_truth(reads, k, index: dict):
    """The scan rule: window i of a read is a hit iff it holds only A/C/G/T (any case) and its canonical key is stored
    in ``index`` with a count above 0.  -> (per read: sorted hit offsets, uint32 distinct hit keys per read)."""
    hits, distinct = [], np.zeros(len(reads), np.uint32)
    for r, s in enumerate(reads):
        S = s.upper()
        run, pos, seen = 0, [], set()
        for j, ch in enumerate(S):
            run = run + 1 if ch in "ACGT" else 0
            if run >= k:
                i = j - k + 1
                v = key_int(O.canonicalize(S[i:i + k]))
                if index.get(v, 0) > 0:
                    pos.append(i)
                    seen.add(v)
        hits.append(pos)
        distinct[r] = len(seen)
    return hits, distinct


def hit_words(offsets, per_read_hits, n_words):
    """Per-read hit offsets -> the engine's hit bitmap (uint64 words over stream positions; read r starts at
    ``offsets[r]``)."""
    bits = np.zeros(n_words * 64, dtype=bool)
    for r, pos in enumerate(per_read_hits):
        if len(pos):
            bits[int(offsets[r]) + np.asarray(pos, dtype=np.int64)] = True
    return np.packbits(bits, bitorder="little").view(np.uint64)


def random_reads(rng, k, n, genome=None, max_len=1000):
    """Reads in the style of ``test_gpu_long_k.mixed_reads``: lengths k - 1, k, k + 1 and up to ``max_len``, with N,
    IUPAC and lower-case bases; some are reverse complements of earlier reads (the same canonical keys from the other
    strand), some high-copy repeats (a homopolymer, a short period)."""
    if genome is None:
        genome = "".join(rng.choice(list("ACGT"), 6000))
    reads = []
    for i in range(n):
        x = rng.random()
        if reads and x < 0.15:
            reads.append(O.reverse_complement(reads[int(rng.integers(0, len(reads)))]))
            continue
        L = max(1, [k - 1, k, k + 1, int(rng.integers(k, max(k, max_len) + 1))][i % 4])
        if x < 0.2:
            unit = "".join(rng.choice(list("ACGT"), int(rng.integers(1, 7))))
            reads.append((unit * (L // len(unit) + 1))[:L])
            continue
        s = int(rng.integers(0, max(1, len(genome) - L)))
        r = list(genome[s:s + L])
        for j in range(len(r)):
            y = rng.random()
            if y < 0.004:
                r[j] = "N"
            elif y < 0.006:
                r[j] = str(rng.choice(list("RYKMSWBDHV")))
            elif y < 0.05:
                r[j] = r[j].lower()
        reads.append("".join(r))
    return reads


def words_of(v: int, W: int):
    return [(v >> (64 * j)) & M64 for j in range(W)]


def rows(keys, W) -> np.ndarray:
    return np.array([words_of(v, W) for v in keys], dtype=np.uint64).reshape(len(keys), W)


def int_of_row(row) -> int:
    return sum(int(x) << (64 * j) for j, x in enumerate(row))


def lohi(keys):
    return (np.array([v & M64 for v in keys], dtype=np.uint64), np.array([v >> 64 for v in keys], dtype=np.uint64))
