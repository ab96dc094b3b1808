"""An independent truth for the long-key table (odd k 65..201, W = 3..7 words; csrc/kdf_long.h, kdf_long_merge.h,
kdf_long_sieve.h): what a key's hash is, where it lives, who owns it, which slice and which sieve bits it takes, and
generators that write down keys under a CHOSEN hash.  numpy and Python ints only; it imports neither the package nor the
oracle (in the way of ``tests/merge_truth.py``) and restates the rules written in ``csrc/kdf_device.h``,
``csrc/kdf_long.h``, ``csrc/kdf_long_merge.h`` and ``csrc/kdf_engine.hip``:

  key        W = ceil(2k / 64) words, word 0 the least significant 64 bits of the k-mer's value (2 bits per base, A=0
             C=1 G=2 T=3, leftmost base most significant); the top word holds tb = 2k - 64 (W - 1) <= 62 bits.
  hash       mix64(x) = (x ^ x >> 32) * 0x9FB21C651E98DF25 (mod 2^64); unmix64 is its inverse.
             fold_step(f, w) = mix64(f ^ w) + 0x632BE59BD9B4E019; fold = fold_step over w[W-1], ..., w[1] from f = 0;
             h = mix64(w0 ^ fold).  So w0 = unmix64(h) ^ fold(w1 ..): ANY upper words can be given ANY hash.
  home slot  h >> (64 - log2cap) (long tables take no hash_shift); bucket = home >> bucket_bits; probing wraps inside
             the bucket.
  owner      (((h >> 16) & 0xFFFF) * parts) >> 16, parts 1..64.
  slice      ((h & 0xFFFF) * key_parts) >> 16.
  sieve      word (h >> 12) & wmask, bits h & 63 and (h >> 6) & 63; a sieve has max(1024, 2^ceil(log2(n * bpk / 64)))
             words for n keys at bpk bits per key.
  canonical  key <= its reverse complement."""
import numpy as np

M64 = (1 << 64) - 1
MIX_MUL = 0x9FB21C651E98DF25
MIX_MUL_INV = 0x02AB9C720D1024AD
FOLD_ADD = 0x632BE59BD9B4E019
MAX_REDRAWS = 64


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def W_of(k):
    return (2 * k + 63) // 64


def top_width(k):
    """bits of the top word"""
    return 2 * k - 64 * (W_of(k) - 1)


def mix64(x):
    x = _u64(x)
    with np.errstate(over="ignore"):
        return (x ^ (x >> np.uint64(32))) * np.uint64(MIX_MUL)


def unmix64(h):
    with np.errstate(over="ignore"):
        h = _u64(h) * np.uint64(MIX_MUL_INV)
    return h ^ (h >> np.uint64(32))


def fold_step(f, w):
    with np.errstate(over="ignore"):
        return mix64(_u64(f) ^ _u64(w)) + np.uint64(FOLD_ADD)


def fold(rows):
    """The fold of the upper words w[1..W-1] of (n, W) rows, from the top word down."""
    rows = _u64(rows)
    f = np.zeros(rows.shape[0], np.uint64)
    for j in range(rows.shape[1] - 1, 0, -1):
        f = fold_step(f, rows[:, j])
    return f


def long_hash(rows):
    rows = _u64(rows)
    return mix64(rows[:, 0] ^ fold(rows))


def home(h, log2cap):
    return _u64(h) >> np.uint64(64 - log2cap)


def bucket(h, log2cap, bucket_bits):
    return home(h, log2cap) >> np.uint64(bucket_bits)


def owner(h, parts):
    return (((_u64(h) >> np.uint64(16)) & np.uint64(0xFFFF)) * np.uint64(parts)) >> np.uint64(16)


def slice_of(h, parts):
    return ((_u64(h) & np.uint64(0xFFFF)) * np.uint64(parts)) >> np.uint64(16)


def sieve_words(n_keys, bits_per_key=32):
    """words of the sieve the engine sizes for n_keys at bits_per_key (its default for up to 2048 keys is 32)"""
    need = (n_keys * bits_per_key + 63) // 64
    w = 1024
    while w < need:
        w *= 2
    return w


def sieve_word_bits(h, wmask):
    """-> (word index, first bit, second bit) of the membership sieve"""
    h = _u64(h)
    return (h >> np.uint64(12)) & np.uint64(wmask), h & np.uint64(63), (h >> np.uint64(6)) & np.uint64(63)


# ---- rows, ints and strings ---------------------------------------------------------------------------------------

def row_to_int(row):
    return sum(int(x) << (64 * j) for j, x in enumerate(row))


def int_to_row(v, W):
    return [(v >> (64 * j)) & M64 for j in range(W)]


def rows_of_ints(vals, W):
    return np.array([int_to_row(v, W) for v in vals], dtype=np.uint64).reshape(len(vals), W)


def revcomp(v, k):
    """reverse complement of a k-mer's value, base by base"""
    rc = 0
    for _ in range(k):
        rc = (rc << 2) | (3 - (v & 3))
        v >>= 2
    return rc


def is_canonical(row, k):
    v = row_to_int(row)
    return v <= revcomp(v, k)


def row_to_kmer(row, k):
    v = row_to_int(row)
    return "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def kmer_to_row(s, k=None):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return int_to_row(v, W_of(len(s) if k is None else k))


def revcomp_str(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def window_keys(read, k):
    """The canonical key (a Python int) of every window of an upper-case ACGT read, by a plain walk."""
    out = []
    for i in range(len(read) - k + 1):
        v = row_to_int(kmer_to_row(read[i:i + k]))
        out.append(min(v, revcomp(v, k)))
    return out


def valid_rows(rows, k):
    return _u64(rows)[:, -1] < np.uint64(1 << top_width(k))


# ---- generators ---------------------------------------------------------------------------------------------------

def _rand64(rng, shape):
    return rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)


def hash_with(rng, n, top_bits=None, nbits=0, owner16=None, slice16=None, low22=None, fill=None, low_nbits=22):
    """n hashes composed from chosen fields: the top ``nbits`` bits ``top_bits`` (the home slot's), bits 16..31
    ``owner16``, bits 0..15 ``slice16``, bits 0..21 ``low22`` (the word of a 1024-word sieve and its two bits;
    ``low_nbits``: bits 0 .. low_nbits - 1 instead, for a larger sieve).  Every field is a scalar or an array of n.  The
    other bits: random (``fill`` None), all 0 or all 1 (``fill`` 0 / 1).  Fields that overlap must not be given together."""
    assert low22 is None or (slice16 is None and owner16 is None)
    assert nbits <= (32 if owner16 is not None else 64 - low_nbits if low22 is not None else 48 if slice16 is not None else 64)
    h = _rand64(rng, n) if fill is None else np.full(n, M64 if fill else 0, np.uint64)

    def put(h, val, shift, width):
        val = np.broadcast_to(_u64(val), (n,))
        assert int(val.max(initial=0)) < (1 << width)
        mask = np.uint64(((1 << width) - 1) << shift)
        return (h & ~mask) | (val << np.uint64(shift))

    if nbits:
        h = put(h, top_bits, 64 - nbits, nbits)
    if owner16 is not None:
        h = put(h, owner16, 16, 16)
    if slice16 is not None:
        h = put(h, slice16, 0, 16)
    if low22 is not None:
        h = put(h, low22, 0, low_nbits)
    return h


def rows_with_hash(h, k, n, rng, share=None, canonical=False, top=None):
    """n distinct valid key rows of a k-mer engine whose hash is ``h`` (a scalar: one collision group; or an array of n
    values: one key each).  The upper words are drawn, the top word is masked to 2k - 64 (W - 1) bits, and w0 is solved
    from h.  ``share``:
      None           every upper word is each row's own;
      "top"          one top word for all rows, the middle words each row's own;
      ("middle", j)  every upper word shared but middle word j (1 .. W-2), each row's own;
      "middles"      every middle word shared, the top word each row's own;
      "upper"        every upper word shared: the rows differ in w0 only, so each needs a hash of its own.
    ``h`` may be a function m -> m hashes: each row's hash is drawn with it, and drawn again with the row.
    ``top``: the top word (share "top" or ("middle", j)) instead of a drawn one; an array of n gives each row its own.
    ``canonical``: rows that are no canonical k-mer are drawn again (drawn top words then begin with base A, which
    accepts ~0.87 of the draws); at most MAX_REDRAWS times per key."""
    W, tb = W_of(k), top_width(k)
    assert W >= 3 and k % 2 == 1
    draw_h = h if callable(h) else None
    h = _u64(draw_h(n)).copy() if draw_h else np.broadcast_to(_u64(h), (n,)).copy()
    assert share != "upper" or draw_h or not canonical
    full = (1 << tb) - 1
    tmask = full >> 2 if canonical else full                       # canonical: drawn top words have A as the first base
    if isinstance(share, tuple):
        assert share[0] == "middle" and 1 <= share[1] <= W - 2
        free = [share[1]]                                          # the words that are each row's own
    else:
        free = {None: list(range(1, W)), "top": list(range(1, W - 1)), "middles": [W - 1], "upper": []}[share]

    def draw(m, j):
        w = _rand64(rng, m)
        return w & np.uint64(tmask) if j == W - 1 else w

    rows = np.zeros((n, W), np.uint64)
    small_top = share == "middles" and (tmask + 1) < 4 * n      # too few top words to draw again row by row
    if top is not None:
        assert W - 1 not in free and int(_u64(top).max()) <= full
    for j in range(1, W):
        if j not in free:
            rows[:, j] = np.broadcast_to(_u64(top), (n,)) if (j == W - 1 and top is not None) else draw(1, j)[0]
    todo = np.arange(n)
    for turn in range(MAX_REDRAWS + 1):
        if todo.size == 0:
            break
        if small_top:                                              # the whole group again: its middle words, every top word
            todo = np.arange(n)
            for j in range(1, W - 1):
                rows[:, j] = draw(1, j)[0]
            assert n <= full + 1
            # (canonical: the smallest top words -- a k-mer that begins with G or T is hardly ever canonical)
            rows[:, W - 1] = _u64(rng.permutation(n) if canonical else rng.permutation(full + 1)[:n])
        else:
            for j in free:
                rows[todo, j] = draw(todo.size, j)
        if draw_h and turn > 0:                                    # (the first turn keeps the hashes drawn above)
            h[todo] = draw_h(todo.size)
        rows[:, 0] = unmix64(h) ^ fold(rows)
        bad = ~valid_rows(rows, k)
        _, first = np.unique(rows, axis=0, return_index=True)      # distinct: every later copy is drawn again
        dup = np.ones(n, bool)
        dup[first] = False
        bad |= dup
        if canonical:
            for i in (range(n) if small_top else todo):
                if not bad[i] and not is_canonical(rows[i], k):
                    bad[i] = True
        todo = np.nonzero(bad)[0]
    assert todo.size == 0, "rows_with_hash: the redraw cap was reached"
    return rows


def random_rows(rng, k, n):
    """n distinct random valid rows (random hashes)"""
    W = W_of(k)
    rows = _rand64(rng, (n + 8, W))
    rows[:, W - 1] &= np.uint64((1 << top_width(k)) - 1)
    rows = rows[np.sort(np.unique(rows, axis=0, return_index=True)[1])]
    assert len(rows) >= n
    return rows[:n]


def sort_rows(rows, cnt=None):
    """Ascending order of the rows as Python ints (the order of a sorted dump) -> rows or (rows, counts)."""
    rows = _u64(rows)
    order = sorted(range(len(rows)), key=lambda i: row_to_int(rows[i]))
    return rows[order] if cnt is None else (rows[order], np.asarray(cnt)[order])
