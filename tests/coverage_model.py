"""Numpy model of "hits in reference coordinates" (kdf_hit_coverage*, kdf_coverage_list*), written from the contract text
of include/kdf.h alone: nothing here is imported from the package.  Slow and plain on purpose -- per read one depth
array over its stream positions and one reference offset per query index."""
import numpy as np

ALIGNED = (0, 7, 8)          # M = X
QUERY_ONLY = (1, 4)          # I S
REF_ONLY = (2, 3)            # D N


def hit_positions(bits, n_bases, k):
    """set bits p of the mask with p + k <= n_bases, ascending int64"""
    n_bases = int(n_bases)
    if n_bases < k:
        return np.zeros(0, np.int64)
    words = np.ascontiguousarray(bits, dtype=np.uint64)[:(n_bases + 63) // 64]
    b = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_bases - k + 1]
    return np.flatnonzero(b).astype(np.int64)


def ref_offsets(ops, qlen):
    """int64[qlen]: the reference offset d each query index is aligned at, -1 for none.  ops: BAM words (len << 4 | op)"""
    d = np.full(qlen, -1, np.int64)
    qc = rc = 0
    for w in np.asarray(ops, dtype=np.uint32).tolist():
        op, ln = w & 15, w >> 4
        if op in ALIGNED:
            lo, hi = min(qc, qlen), min(qc + ln, qlen)
            if hi > lo:
                d[lo:hi] = rc + (np.arange(lo, hi) - qc)
            qc += ln
            rc += ln
        elif op in QUERY_ONLY:
            qc += ln
        elif op in REF_ONLY:
            rc += ln
    return d


def add_coverage(positions, k, offsets, ref_start, cigar, cigar_offsets, kmer_cov, read_cov):
    """the sums of one call, added in place to the two uint32 accumulators; positions: the hits (already masked)"""
    span = len(kmer_cov)
    assert len(read_cov) == span and kmer_cov.dtype == np.uint32 and read_cov.dtype == np.uint32
    pos = np.asarray(positions, dtype=np.int64)
    offs = np.asarray(offsets, dtype=np.int64)
    for r in range(len(offs) - 1):
        if int(ref_start[r]) < 0:
            continue
        b, e = int(offs[r]), int(offs[r + 1])
        mine = pos[(pos >= b) & (pos < e)]
        if e <= b or len(mine) == 0:
            continue
        depth = np.zeros(e - b, np.int64)
        for p in mine.tolist():
            depth[p - b:min(p + k, e) - b] += 1
        d = ref_offsets(cigar[int(cigar_offsets[r]):int(cigar_offsets[r + 1])], e - b)
        sel = (depth > 0) & (d >= 0)
        g = int(ref_start[r]) + d[sel]
        dep = depth[sel]
        ok = g < span
        g, dep = g[ok], dep[ok]
        assert len(np.unique(g)) == len(g)                       # one reference position per aligned query index
        kmer_cov[g] = (kmer_cov[g].astype(np.int64) + dep).astype(np.uint32)      # (modulo 2^32)
        read_cov[g] = (read_cov[g].astype(np.int64) + 1).astype(np.uint32)


def hit_coverage(bits, n_bases, k, offsets, ref_start, cigar, cigar_offsets, kmer_cov, read_cov):
    add_coverage(hit_positions(bits, n_bases, k), k, offsets, ref_start, cigar, cigar_offsets, kmer_cov, read_cov)


def coverage_list(kmer_cov, read_cov, first, n, min_reads):
    """-> (positions uint64, kmer uint32, reads uint32), ascending"""
    thr = max(int(min_reads), 1)
    g = first + np.flatnonzero(np.asarray(read_cov[first:first + n]) >= thr)
    return g.astype(np.uint64), np.asarray(kmer_cov)[g].astype(np.uint32), np.asarray(read_cov)[g].astype(np.uint32)


def coverage_list_dict(kmer_cov, read_cov, first, n, min_reads):
    """the same list from a sorted dict, position by position"""
    thr = max(int(min_reads), 1)
    d = {g: (int(kmer_cov[g]), int(read_cov[g])) for g in range(first, first + n) if int(read_cov[g]) >= thr}
    return [(g, *d[g]) for g in sorted(d)]


# ---- building inputs ----------------------------------------------------------------------------------------------------

def cigar_words(ops):
    """[(op, len), ...] -> uint32 BAM words"""
    return np.array([(ln << 4) | op for op, ln in ops], dtype=np.uint32)


def pack_reads(reads, lead=0):
    """reads: [(length, [(op, len) ...], [hit query indices], ref_start)] laid back to back from stream position
    ``lead`` on -> (bits uint64[words], n_bases, offsets, ref_start, cigar, cigar_offsets); two mask words of room
    behind the last read"""
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[0] = lead
    co = np.zeros(len(reads) + 1, np.int64)
    cg, rs = [], []
    for i, (L, ops, _hits, start) in enumerate(reads):
        offs[i + 1] = offs[i] + L
        co[i + 1] = co[i] + len(ops)
        cg.append(cigar_words(ops))
        rs.append(start)
    n_bases = int(offs[-1])
    b = np.zeros(((n_bases + 63) // 64 + 2) * 64, dtype=bool)
    for i, (L, _ops, hits, _start) in enumerate(reads):
        for h in hits:
            assert 0 <= h < L
            b[int(offs[i]) + h] = True
    bits = np.packbits(b, bitorder="little").view(np.uint64).copy()
    cigar = np.concatenate(cg).astype(np.uint32) if cg else np.zeros(0, np.uint32)
    return bits, n_bases, offs, np.array(rs, dtype=np.int64), cigar, co
