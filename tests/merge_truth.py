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
a canonical key -- only ``kdf_load_filter`` does -- so ``keys_with_hash`` does not filter for it; ``is_canonical`` is
the plain reverse-complement test for the callers that load a filter."""
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


def is_canonical(lo, hi, k):
    """key <= its reverse complement (A=0 C=1 G=2 T=3, leftmost base most significant), on Python ints."""
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


def keys_with_hash(h_top, nbits, n, k, rng):
    """n distinct valid keys of a k-mer engine whose hash has the top ``nbits`` bits ``h_top`` (a scalar, or an array of
    n values: one key each).  The free low bits are drawn until the key is valid.  -> (lo, hi or None) uint64."""
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
        free = rng.integers(0, 1 << 63, m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, m, dtype=np.uint64)
        if nbits == 0:
            h = free
        elif nbits == 64:
            h = top[todo]
        else:
            h = (top[todo] << np.uint64(64 - nbits)) | (free >> np.uint64(nbits))
        if wide:
            hb = 2 * k - 64
            hi[todo] = rng.integers(0, 1 << hb, m, dtype=np.uint64)
            lo[todo] = unmix64(h) ^ rot_hi(hi[todo])
        else:
            lo[todo] = unmix64(h)
        bad = ~valid_keys(lo, hi, k)
        # distinct: every later copy of a key is drawn again
        order = np.lexsort((lo,) if not wide else (lo, hi))
        same = (lo[order][1:] == lo[order][:-1]) if not wide else ((lo[order][1:] == lo[order][:-1]) & (hi[order][1:] == hi[order][:-1]))
        bad[order[1:][same]] = True
        todo = np.nonzero(bad)[0]
    assert todo.size == 0, "keys_with_hash: too few valid keys under this prefix"
    return lo, hi


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
