"""A numpy model of the read offsets a spool keeps beside its segments (include/kdf.h "Reads in a spool"), on top of
``spool_model``'s segment layout.

A batch placed at tile t0 of a segment contributes ``64 * t0 + offsets[i]`` for i = 0 .. n_reads; its last entry is
overwritten by the first entry of the next batch in the same segment.  Reads are numbered in append order; a segment owns
the reads of its batches."""
import numpy as np

import spool_model as M

TILE = M.TILE


def segment_offsets(batches, segment_positions):
    """batches: [(packed, invalid, n_bases, offsets)] -> [(offsets int64[n_reads + 1], first_read, n_reads)] per segment.
    Batches of n_bases == 0 must have no reads (they store nothing)."""
    place, seg_tiles = M.layout([b[2] for b in batches], segment_positions)
    offs = [[np.zeros(1, np.int64)] for _ in seg_tiles]
    first = [None] * len(seg_tiles)
    reads = 0
    for (_, _, n, o), at in zip(batches, place):
        o = np.asarray(o, np.int64)
        if at is None:
            assert len(o) <= 1
            continue
        s, t0 = at
        if first[s] is None:
            first[s] = reads
        cur = np.concatenate(offs[s])
        offs[s] = [cur[:-1], TILE * t0 + o]                         # the entry before is overwritten
        reads += len(o) - 1
    out = []
    for s in range(len(seg_tiles)):
        o = np.concatenate(offs[s])
        out.append((o, first[s], len(o) - 1))
    return out


def make_batch(rng, pieces, rem=None, dirty=True):
    """One batch from ``pieces``: a list of reads, each an array of base codes (0..3, 4 = an invalid base) or None for a
    read of length 0 (no stream position at all).  Every other read is followed by one invalid separator, as
    kdf_pack_reads lays reads out.  ``rem``: the last read is lengthened by random bases until n_bases % 64 == rem.
    -> (packed, invalid, n_bases, offsets) with arrays of exactly stream_words(n_bases) words, random bits at and past
    n_bases when ``dirty``."""
    codes, inv, offs = [], [], [0]
    n = 0
    pieces = list(pieces)
    if rem is not None:
        total = sum(0 if p is None else len(p) + 1 for p in pieces)
        last = max(i for i, p in enumerate(pieces) if p is not None)
        pad = (rem - total) % 64
        pieces[last] = np.concatenate([pieces[last], rng.integers(0, 4, pad)])
    for p in pieces:
        if p is not None:
            p = np.asarray(p)
            codes.append(np.where(p > 3, 0, p).astype(np.uint8)); inv.append(p > 3)
            codes.append(np.zeros(1, np.uint8)); inv.append(np.ones(1, bool))
            n += len(p) + 1
        offs.append(n)
    codes = np.concatenate(codes) if codes else np.zeros(0, np.uint8)
    inv = np.concatenate(inv) if inv else np.zeros(0, bool)
    assert rem is None or n % 64 == rem
    return M.pack(codes, inv, rng if dirty else None) + (n, np.asarray(offs, np.int64))
