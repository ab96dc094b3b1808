"""An independent truth for the multi-GPU merge of k <= 63 counts (csrc/kdf_merge.h): where a key lives, who owns it,
in what order the owner-ordered dump lists it, and what a merge of segments holds.  numpy and Python ints only; it
imports neither the package nor the oracle (in the way of ``tests/stream_truth.py``) and restates the rules written in
``csrc/kdf_device.h`` and ``include/kdf.h``:

  hash       mix64(x) = (x ^ x >> 32) * 0x9FB21C651E98DF25 (mod 2^64); unmix64 is its inverse (multiply by
             0x02ab9c720d1024ad, then x ^ x >> 32).  rot_hi(hi) = hi << 37 | hi >> 27.
             Narrow keys (k <= 32): h = mix64(lo).  Wide keys (33 <= k <= 63): h = mix64(lo ^ rot_hi(hi)).
  owner      ((h >> 48) * parts) >> 16, parts 1..64.
  home slot  (h << hash_shift) >> (64 - log2cap); bucket = home >> bucket_bits.  Probing wraps inside the bucket.
  dump order the top log2cap - 6 bits of h, non-decreasing over the whole owner-ordered dump.
  merge      key by key the sum of all counts, saturating at 2^32 - 1; a key listed with count 0 is inserted with 0.

Keys are uint64 arrays ``lo`` and ``hi`` (``hi`` None for k <= 32).  What the engine requires of a key handed to
``kdf_add_pairs*``: 2k bits (k <= 31: lo < 2^(2k); wide: hi < 2^(2k - 64)) and, narrow keys, a stored form other than
the empty marker 2^64 - 1 (its key, 0xfd54638d0fbbb8de, is no canonical 32-mer).  ``kdf_add_pairs*`` does not ask for
a canonical key -- only ``kdf_load_filter`` and the reads do -- so ``keys_with_hash`` filters for it only when asked
(``canonical=True``); ``is_canonical`` is the plain reverse-complement test.

Wide keys (33 <= k <= 63) are stored as (h, hi) and h is no bijection of the key: ``collision_group`` writes down keys
that share all 64 bits of h and differ in hi, ``keys_sharing_hi`` keys that share hi and the home slot and differ in h.
``kmer_string`` spells a key as the read that holds it."""
import numpy as np

M64 = (1 << 64) - 1
MIX_MUL = 0x9FB21C651E98DF25
MIX_MUL_INV = 0x02AB9C720D1024AD
U32_MAX = (1 << 32) - 1
EMPTY = M64


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix64(x):
    x = _u64(x)
    with np.errstate(over="ignore"):
        return (x ^ (x >> np.uint64(32))) * np.uint64(MIX_MUL)


def unmix64(h):
    with np.errstate(over="ignore"):
        h = _u64(h) * np.uint64(MIX_MUL_INV)
    return h ^ (h >> np.uint64(32))


def rot_hi(hi):
    hi = _u64(hi)
    return (hi << np.uint64(37)) | (hi >> np.uint64(27))


def key_hash(lo, hi=None):
    """The table's hash of a key (the stored form of its low word)."""
    return mix64(_u64(lo) if hi is None else _u64(lo) ^ rot_hi(hi))


def owner(h, parts):
    return ((_u64(h) >> np.uint64(48)) * np.uint64(parts)) >> np.uint64(16)


def home(h, log2cap, hash_shift=0):
    return (_u64(h) << np.uint64(hash_shift)) >> np.uint64(64 - log2cap)


def bucket(h, log2cap, bucket_bits, hash_shift=0):
    return home(h, log2cap, hash_shift) >> np.uint64(bucket_bits)


def order_key(h, log2cap):
    return _u64(h) >> np.uint64(64 - (log2cap - 6))


def valid_keys(lo, hi, k):
    """Which (lo, hi) are keys a k-mer engine takes."""
    lo = _u64(lo)
    if k <= 32:
        ok = mix64(lo) != np.uint64(EMPTY)
        if k < 32:
            ok &= lo < np.uint64(1 << (2 * k))
        return ok
    return _u64(hi) < np.uint64(1 << (2 * k - 64))


def _int_of(lo, hi):
    return int(lo) | (int(hi) << 64 if hi is not None else 0)


def is_canonical_ints(lo, hi, k):
    """key <= its reverse complement (A=0 C=1 G=2 T=3, leftmost base most significant), base by base on Python ints:
    the rule spelled out, slow; ``is_canonical`` is pinned to it by tests/test_merge_truth.py."""
    lo = _u64(lo)
    out = np.zeros(lo.shape, dtype=bool)
    for i in range(lo.size):
        v = _int_of(lo.flat[i], None if hi is None else _u64(hi).flat[i])
        rc, x = 0, v
        for _ in range(k):
            rc = (rc << 2) | (3 - (x & 3))
            x >>= 2
        out.flat[i] = v <= rc
    return out


def _rev2(x):
    """the 32 two-bit groups of every word in reverse order"""
    x = _u64(x)
    for s, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x >> np.uint64(s)) & np.uint64(m)) | ((x & np.uint64(m)) << np.uint64(s))
    return (x >> np.uint64(32)) | (x << np.uint64(32))


def revcomp_key(lo, hi, k):
    """The reverse complement of the keys, as (lo, hi or None): the 2k bits in reverse base order, every base b as
    3 - b (= ~b on two bits).  numpy, arrays of any shape."""
    lo = _u64(lo)
    if k <= 32:
        return (~_rev2(lo)) >> np.uint64(64 - 2 * k), None
    a, b = ~_rev2(lo), ~_rev2(_u64(hi))              # the 128-bit word (a << 64 | b) is the complement of all 64 bases reversed
    s = np.uint64(128 - 2 * k)                       # 2 .. 62
    return (a << (np.uint64(64) - s)) | (b >> s), a >> s


def is_canonical(lo, hi, k):
    """key <= its reverse complement (A=0 C=1 G=2 T=3, leftmost base most significant)."""
    lo = _u64(lo)
    rlo, rhi = revcomp_key(lo, hi, k)
    if k <= 32:
        return lo <= rlo
    hi = _u64(hi)
    return (hi < rhi) | ((hi == rhi) & (lo <= rlo))


def keys_with_hash(h_top, nbits, n, k, rng, canonical=False):
    """n distinct valid keys of a k-mer engine whose hash has the top ``nbits`` bits ``h_top`` (a scalar, or an array of
    n values: one key each).  The free low bits are drawn until the key is valid.  canonical: only keys for which
    ``is_canonical`` holds (32 candidates per key and round, the first canonical one is taken; the others are drawn
    again).  -> (lo, hi or None) uint64."""
    assert 0 <= nbits <= 64 and 1 <= k <= 63
    top = np.broadcast_to(_u64(h_top), (n,)).copy()
    assert nbits == 64 or int(top.max(initial=0)) < (1 << nbits)
    wide = k > 32
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64) if wide else None
    todo = np.arange(n)
    for _ in range(200):
        if todo.size == 0:
            break
        m = todo.size
        shape = (m, 32) if canonical else m
        free = rng.integers(0, 1 << 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)
        t = top[todo][:, None] if canonical else top[todo]
        if nbits == 0:
            h = free
        elif nbits == 64:
            h = np.broadcast_to(t, free.shape)
        else:
            h = (t << np.uint64(64 - nbits)) | (free >> np.uint64(nbits))
        chi = rng.integers(0, 1 << (2 * k - 64), shape, dtype=np.uint64) if wide else None
        clo = unmix64(h) ^ rot_hi(chi) if wide else unmix64(h)
        none = np.zeros(m, bool)
        if canonical:
            ok = valid_keys(clo, chi, k) & is_canonical(clo, chi, k)
            pick, rows = ok.argmax(axis=1), np.arange(m)
            none = ~ok[rows, pick]
            clo, chi = clo[rows, pick], (chi[rows, pick] if wide else None)
        lo[todo] = clo
        if wide:
            hi[todo] = chi
        bad = ~valid_keys(lo, hi, k)
        bad[todo[none]] = True
        # distinct: every later copy of a key is drawn again
        order = np.lexsort((lo,) if not wide else (lo, hi))
        same = (lo[order][1:] == lo[order][:-1]) if not wide else ((lo[order][1:] == lo[order][:-1]) & (hi[order][1:] == hi[order][:-1]))
        bad[order[1:][same]] = True
        todo = np.nonzero(bad)[0]
    assert todo.size == 0, "keys_with_hash: too few valid keys under this prefix"
    return lo, hi


def collision_group(h, n, k, rng, canonical=False):
    """n distinct valid wide keys (33 <= k <= 63) that ALL have the 64-bit hash ``h``: one key per high word, lo =
    unmix64(h) ^ rot_hi(hi).  The key space under one h is the 2^(2k - 64) high words: it is listed whole while it has at
    most 2^20 members, and sampled above that.  -> (lo, hi) in drawn order."""
    assert 33 <= k <= 63 and 0 <= int(h) <= M64
    hb = 2 * k - 64
    if hb <= 20:
        hi = np.arange(1 << hb, dtype=np.uint64)
    else:
        hi = np.zeros(0, np.uint64)
        for _ in range(20):
            hi = np.unique(np.concatenate([hi, rng.integers(0, 1 << hb, 64 * n + 1024, dtype=np.uint64)]))
            if not canonical or int(is_canonical(unmix64(h) ^ rot_hi(hi), hi, k).sum()) >= n:
                break
    lo = unmix64(np.uint64(h)) ^ rot_hi(hi)
    if canonical:
        keep = is_canonical(lo, hi, k)
        lo, hi = lo[keep], hi[keep]
    assert len(hi) >= n, f"collision_group: k={k}, h={int(h):#018x}: {len(hi)} {'canonical ' if canonical else ''}keys, {n} wanted"
    pick = rng.permutation(len(hi))[:n]
    return lo[pick], hi[pick]


def keys_sharing_hi(h_top, nbits, n, k, rng, hi=None, canonical=False):
    """n distinct valid wide keys with ONE high word (``hi``, drawn when None) whose hashes share the top ``nbits`` bits
    ``h_top`` and differ below them: one home slot in every table of up to 2^nbits slots, n different stored forms h --
    the mirror of ``collision_group``, here only lo tells the keys apart.  -> (lo, hi) in drawn order."""
    assert 33 <= k <= 63 and 0 < nbits < 64 and 0 <= int(h_top) < (1 << nbits)
    hb = 2 * k - 64
    for _ in range(64):
        one = np.uint64(rng.integers(0, 1 << hb, dtype=np.uint64) if hi is None else hi)
        low = np.unique(rng.integers(0, 1 << (64 - nbits), 16 * n + 256, dtype=np.uint64))
        h = (np.uint64(h_top) << np.uint64(64 - nbits)) | low
        lo = unmix64(h) ^ rot_hi(one)
        his = np.full(len(lo), one, np.uint64)
        if canonical:
            keep = is_canonical(lo, his, k)
            lo, his = lo[keep], his[keep]
        if len(lo) >= n or hi is not None:
            break
    assert len(lo) >= n, f"keys_sharing_hi: k={k}, hi={int(one):#x}, prefix {int(h_top):#x}/{nbits}: {len(lo)} keys, {n} wanted"
    pick = rng.permutation(len(lo))[:n]
    return lo[pick], his[pick]


def kmer_string(lo, hi, k):
    """The key as its k bases (A=0 C=1 G=2 T=3, leftmost base most significant: what ``kmer_truth.key_int`` reads)."""
    v = _int_of(lo, hi)
    assert v < 1 << (2 * k)
    return "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp_string(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _as_arrays(seg):
    """A segment as (lo, hi or None, cnt uint64): a dict {(lo, hi) or lo: count} or a tuple (lo, hi, cnt); cnt None = zeros."""
    if isinstance(seg, dict):
        ks = list(seg)
        wide = bool(ks) and isinstance(ks[0], tuple)
        lo = np.array([k_[0] if wide else k_ for k_ in ks], dtype=np.uint64)
        hi = np.array([k_[1] for k_ in ks], dtype=np.uint64) if wide else None
        return lo, hi, np.array([seg[k_] for k_ in ks], dtype=np.uint64)
    lo, hi, cnt = seg
    lo = _u64(lo)
    return lo, (None if hi is None else _u64(hi)), (np.zeros(lo.shape, np.uint64) if cnt is None else np.asarray(cnt).astype(np.uint64))


def merge(segments):
    """Key-by-key sum of the segments' counts, saturating at 2^32 - 1.  A key twice in one segment is summed; a zero
    count inserts the key with 0.  -> (lo, hi or None, cnt uint32) in ascending (hi, lo) order."""
    parts = [_as_arrays(s) for s in segments]
    parts = [p for p in parts if p[0].size]
    wide = any(p[1] is not None for p in parts)
    if not parts:
        return np.zeros(0, np.uint64), None, np.zeros(0, np.uint32)
    assert all((p[1] is not None) == wide for p in parts)
    lo = np.concatenate([p[0] for p in parts])
    hi = np.concatenate([p[1] for p in parts]) if wide else None
    cnt = np.concatenate([p[2] for p in parts])
    assert int(cnt.max()) <= U32_MAX and cnt.size < (1 << 31)          # so a uint64 sum cannot wrap
    order = np.lexsort((lo, hi)) if wide else np.argsort(lo, kind="stable")
    lo, cnt = lo[order], cnt[order]
    new = np.ones(lo.size, dtype=bool)
    if wide:
        hi = hi[order]
        new[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    else:
        new[1:] = lo[1:] != lo[:-1]
    starts = np.nonzero(new)[0]
    total = np.minimum(np.add.reduceat(cnt, starts), np.uint64(U32_MAX)).astype(np.uint32)
    return lo[starts], (hi[starts] if wide else None), total


def as_dict(lo, hi, cnt):
    """{lo or (lo, hi): count} with Python ints."""
    if hi is None:
        return {int(a): int(c) for a, c in zip(lo.tolist(), np.asarray(cnt).tolist())}
    return {(int(a), int(b)): int(c) for a, b, c in zip(lo.tolist(), hi.tolist(), np.asarray(cnt).tolist())}


def sorted_triples(lo, hi, cnt):
    """(lo, hi, cnt) in ascending (hi, lo, cnt) order: a multiset of pairs in canonical form."""
    lo, cnt = _u64(lo), np.asarray(cnt).astype(np.uint32)
    if hi is None:
        order = np.lexsort((cnt, lo))
        return lo[order], None, cnt[order]
    hi = _u64(hi)
    order = np.lexsort((cnt, lo, hi))
    return lo[order], hi[order], cnt[order]
