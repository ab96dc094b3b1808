"""The numpy model of kdf_hit_coverage / kdf_coverage_list (tests/coverage_model.py, written from include/kdf.h) against the
host mirror of the reference, ``_collect_kmer_ref_positions``, which the golden bedGraph / read-coverage test pins.  No
GPU: pure numpy on both sides."""
import numpy as np
import pytest

import coverage_model as CM

OPS_ALL = list(range(9))                 # M I D N S H P = X


def random_cigar(rng, qlen, consume_all=True):
    """operations over all nine codes that consume at most qlen query bases (exactly qlen with consume_all)"""
    ops, left = [], qlen
    if rng.random() < 0.3:
        ops.append((5, int(rng.integers(1, 20))))
    if left > 2 and rng.random() < 0.4:
        n = int(rng.integers(1, max(2, left // 4)))
        ops.append((4, n)); left -= n
    while left > 0:
        op = int(rng.choice([0, 0, 0, 7, 8, 1, 2, 3, 6]))
        n = int(rng.integers(1, max(2, left // 2 + 1)))
        if op in (0, 7, 8, 1):
            n = min(n, left); left -= n
        ops.append((op, n))
        if not consume_all and rng.random() < 0.15:
            break
    if rng.random() < 0.3 and left == 0 and ops and ops[-1][0] in (0, 7, 8) and ops[-1][1] > 2:
        op, n = ops[-1]
        c = int(rng.integers(1, n))
        ops[-1] = (op, n - c); ops.append((4, c))
    if rng.random() < 0.2:
        ops.append((5, int(rng.integers(1, 9))))
    return ops


def mirror_counts(ops, qlen, hits, k):
    from kmer_denovo_filter_amd.core.bam_scanner import _collect_kmer_ref_positions
    cov = _collect_kmer_ref_positions(0, ops, qlen, np.asarray(hits, dtype=np.int64), k)
    return dict(cov)


@pytest.mark.parametrize("k", [5, 31])
def test_model_equals_the_host_mirror(k):
    rng = np.random.default_rng(1000 + k)
    STRIDE = 4096
    reads, seen_ops = [], set()
    for i in range(1500):
        qlen = int(rng.integers(1, 260))
        kind = i % 5
        if kind == 3:
            ops = []                                                         # an empty CIGAR
        else:
            ops = random_cigar(rng, qlen, consume_all=kind != 4)             # kind 4: fewer query bases than the read has
        seen_ops |= {op for op, _ in ops}
        dens = [0.02, 0.3, 1.0][i % 3]
        hits = np.flatnonzero(rng.random(qlen) < dens).tolist()
        reads.append((qlen, ops, hits, i * STRIDE))
    assert seen_ops == set(OPS_ALL)
    assert any(sum(n for op, n in ops if op in (0, 1, 4, 7, 8)) < L for L, ops, _, _ in reads if ops)
    bits, n_bases, offs, rs, cigar, co = CM.pack_reads(reads)
    span = len(reads) * STRIDE
    kc, rc = np.zeros(span, np.uint32), np.zeros(span, np.uint32)
    # every hit counts, those in the last k - 1 positions of the last read too: the mask has room behind the reads
    CM.hit_coverage(bits, n_bases + k, k, offs, rs, cigar, co, kc, rc)
    covered = 0
    for i, (qlen, ops, hits, start) in enumerate(reads):
        want = mirror_counts(ops, qlen, hits, k)
        assert all(0 <= p < STRIDE for p in want)
        got_k, got_r = kc[start:start + STRIDE], rc[start:start + STRIDE]
        nz = np.flatnonzero(got_r)
        assert {int(p): int(got_k[p]) for p in nz} == want, i
        assert (got_r[nz] == 1).all() and not got_k[got_r == 0].any()
        covered += len(want)
    assert covered > 10000


def test_model_hits_are_masked_like_the_hit_list():
    k = 5
    reads = [(20, [(0, 20)], [0, 15, 16, 19], 0)]
    bits, n_bases, offs, rs, cigar, co = CM.pack_reads(reads)
    assert CM.hit_positions(bits, n_bases, k).tolist() == [0, 15]             # 16 + 5 > 20
    bits[0] |= np.uint64(1) << np.uint64(40)                                  # garbage past n_bases
    assert CM.hit_positions(bits, n_bases, k).tolist() == [0, 15]
    assert CM.hit_positions(bits, 4, k).tolist() == []


def test_model_list_equals_a_sorted_dict():
    rng = np.random.default_rng(7)
    rc = (rng.random(3000) < 0.2) * rng.integers(1, 6, 3000)
    rc = rc.astype(np.uint32)
    kc = (rc * rng.integers(1, 40, 3000)).astype(np.uint32)
    for first, n in ((0, 3000), (17, 1000), (2999, 1), (100, 0)):
        for min_reads in (0, 1, 3):
            pos, kv, rv = CM.coverage_list(kc, rc, first, n, min_reads)
            assert [(int(a), int(b), int(c)) for a, b, c in zip(pos, kv, rv)] == CM.coverage_list_dict(kc, rc, first, n, min_reads)
            assert (np.diff(pos.astype(np.int64)) > 0).all()
    assert len(CM.coverage_list(kc, rc, 0, 3000, 0)[0]) == len(CM.coverage_list(kc, rc, 0, 3000, 1)[0]) > 0
