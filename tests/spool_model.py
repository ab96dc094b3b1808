"""A numpy model of the read spool's segment layout (include/kdf.h "read spool"), position by position.

It shares with the engine the stream layout written in ``include/kdf.h`` and nothing else: base i is bits ``2 * (i % 32)``
of ``packed[i // 32]``, bit ``i % 64`` of ``invalid[i // 64]`` marks an invalid position, a stream of n positions has
``2 * ceil(n / 64) + 4`` packed and ``ceil(n / 64) + 2`` mask words.

The model unpacks every batch to one code and one flag per position, lays the batches out by the header's rules -- a batch
of n positions takes n // 64 + 1 tiles of 64, its positions at and past n are invalid with base 0, a batch that does not
fit the room left opens a new segment, one longer than ``segment_positions`` gets a segment of its own size -- and packs
each segment again: padding words zero (packed) and all ones (mask)."""
import numpy as np

TILE = 64


def stream_words(n):
    t = -(-int(n) // TILE)
    return 2 * t + 4, t + 2


def unpack(packed, invalid, n):
    """(codes uint8[n], inv bool[n]) of the first n positions."""
    n = int(n)
    pos = np.arange(n, dtype=np.uint64)
    codes = ((np.asarray(packed, np.uint64)[(pos >> np.uint64(5)).astype(np.int64)] >> ((pos & np.uint64(31)) << np.uint64(1))) & np.uint64(3)).astype(np.uint8)
    inv = ((np.asarray(invalid, np.uint64)[(pos >> np.uint64(6)).astype(np.int64)] >> (pos & np.uint64(63))) & np.uint64(1)).astype(bool)
    return codes, inv


def pack(codes, inv, rng=None):
    """Arrays of exactly the stream_words(len(codes)) sizes.  Positions at and past n: base 0 / invalid and the padding
    words 0 / all ones -- or, with ``rng``, random bits everywhere there (a producer's dirty buffers)."""
    n = len(codes)
    pw, mw = stream_words(n)
    c = np.zeros(pw * 32, np.uint64)
    m = np.ones(mw * 64, np.uint64)
    if rng is not None:
        c[:] = rng.integers(0, 4, len(c))
        m[:] = rng.integers(0, 2, len(m))
    c[:n] = codes
    m[:n] = inv
    packed = (c.reshape(pw, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(axis=1, dtype=np.uint64)
    invalid = (m.reshape(mw, 64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return packed, invalid


def batch_tiles(n):
    return int(n) // TILE + 1


def layout(lengths, segment_positions):
    """[(segment index, first tile)] per batch, None for an empty batch, and the tiles of every segment."""
    cap = int(segment_positions) // TILE
    place, seg_tiles, seg_cap = [], [], []
    for n in lengths:
        if n == 0:
            place.append(None)
            continue
        t = batch_tiles(n)
        if not seg_tiles or seg_tiles[-1] + t > seg_cap[-1]:
            seg_tiles.append(0)
            seg_cap.append(max(cap, t))
        place.append((len(seg_tiles) - 1, seg_tiles[-1]))
        seg_tiles[-1] += t
    return place, seg_tiles


def segments(batches, segment_positions):
    """batches: [(packed, invalid, n_bases)] -> [(packed, invalid, n_positions)] of every segment, words as the spool
    must hold them (padding words included)."""
    place, seg_tiles = layout([b[2] for b in batches], segment_positions)
    codes = [np.zeros(t * TILE, np.uint8) for t in seg_tiles]
    inv = [np.ones(t * TILE, bool) for t in seg_tiles]
    for (packed, invalid, n), at in zip(batches, place):
        if at is None:
            continue
        s, t0 = at
        c, i = unpack(packed, invalid, n)
        codes[s][t0 * TILE:t0 * TILE + n] = c
        inv[s][t0 * TILE:t0 * TILE + n] = i
    return [pack(c, i) + (len(c),) for c, i in zip(codes, inv)]
