"""kdf_hit_coverage / kdf_coverage_list / kdf_hit_keys on the GPU against the numpy model of tests/coverage_model.py
(written from include/kdf.h).  The masks are built directly as bit patterns: no table is needed and every hit is known.
Every case is a few thousand positions."""
import numpy as np
import pytest
import torch

import coverage_model as CM
import kmer_truth as KT
from test_gpu_depth import cuda_words, key_args, new_engine, stream_of

pytestmark = pytest.mark.gpu

KS = [5, 31, 101]
GUARD = 64
PATTERN32 = 0x5A5A5A5A
KDF_ERR_INVALID = 1


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(k):
        if k not in made:
            made[k] = new_engine(k, hint=1 << 10)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def dev(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    if a.nbytes == 0:
        a = np.zeros(1, dt)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def guarded(values):
    """uint32 values between two guard regions on the device"""
    g = np.full(GUARD, PATTERN32, np.uint32)
    return torch.from_numpy(np.concatenate((g, np.asarray(values, np.uint32), g)).view(np.int32).copy()).cuda()


def unguard(t, n):
    a = t.cpu().numpy().view(np.uint32)
    assert (a[:GUARD] == PATTERN32).all() and (a[GUARD + n:] == PATTERN32).all(), "a write outside the accumulator"
    return a[GUARD:GUARD + n].copy()


def device_coverage(e, bits, n_bases, offs, rs, cigar, co, kc0, rc0):
    """hit_coverage_dev into guarded accumulators that start as kc0 / rc0 -> (kmer_cov, read_cov)"""
    span = len(kc0)
    dk, dr = guarded(kc0), guarded(rc0)
    db, do, ds, dc, dco = dev(bits, np.uint64), dev(offs, np.int64), dev(rs, np.int64), dev(cigar, np.uint32), dev(co, np.int64)
    torch.cuda.synchronize()
    e.hit_coverage_dev(db.data_ptr(), n_bases, do.data_ptr(), len(offs) - 1, ds.data_ptr(), dc.data_ptr(), len(cigar),
                       dco.data_ptr(), dk.data_ptr() + 4 * GUARD, dr.data_ptr() + 4 * GUARD, span)
    e.synchronize()
    return unguard(dk, span), unguard(dr, span)


def check(e, k, packed, span, n_bases=None, start=None):
    """host and device forms against the model, on accumulators that start as ``start`` (default zeros) -> the sums"""
    bits, nb, offs, rs, cigar, co = packed
    nb = nb if n_bases is None else n_bases
    kc0, rc0 = (np.zeros(span, np.uint32), np.zeros(span, np.uint32)) if start is None else start
    wk, wr = kc0.copy(), rc0.copy()
    CM.hit_coverage(bits, nb, k, offs, rs, cigar, co, wk, wr)
    hk, hr = kc0.copy(), rc0.copy()
    e.hit_coverage(bits, nb, offs, rs, cigar, co, hk, hr)
    assert np.array_equal(hk, wk), f"host form: kmer_cov differs at {np.flatnonzero(hk != wk)[:8]}"
    assert np.array_equal(hr, wr), f"host form: read_cov differs at {np.flatnonzero(hr != wr)[:8]}"
    dk, dr = device_coverage(e, bits, nb, offs, rs, cigar, co, kc0, rc0)
    assert np.array_equal(dk, wk), f"device form: kmer_cov differs at {np.flatnonzero(dk != wk)[:8]}"
    assert np.array_equal(dr, wr), f"device form: read_cov differs at {np.flatnonzero(dr != wr)[:8]}"
    return wk, wr


def boundaries(ops):
    """query indices at which an operation starts or ends"""
    out, qc = set(), 0
    for op, ln in ops:
        if op in (0, 1, 4, 7, 8):
            out.add(qc)
            qc += ln
            out.add(qc)
    return out


def cigar_cases(k, L):
    a = k + 7
    return {
        "pure M": [(0, L)],
        "soft clips": [(4, 5), (0, L - 12), (4, 7)],
        "insertion": [(0, a), (1, 4), (0, L - a - 4)],
        "deletion": [(0, a), (2, 6), (0, L - a)],
        "N skip": [(0, a), (3, 50), (0, L - a)],
        "= and X": [(7, a), (8, 1), (7, L - a - 1)],
        "H and P": [(5, 10), (0, a), (6, 3), (0, L - a), (5, 4)],
        "empty": [],
        "shorter than the read": [(0, L - k - 3)],
        "longer than the read": [(4, 3), (0, L + 20)],
    }


@pytest.mark.parametrize("k", KS)
def test_cigar_cases_inside_and_at_the_edge_of_a_window(engines, k):
    e = engines(k)
    L = 3 * k + 40
    reads, STRIDE = [], 512
    for name, ops in cigar_cases(k, L).items():
        hits = {0, L - k}
        for qb in boundaries(ops) | {k + 7}:
            # windows that end at, straddle and start at the boundary
            hits |= {h for h in (qb - k, qb - k + 1, qb - k // 2, qb - 1, qb) if 0 <= h <= L - k}
        hits = sorted(hits)
        reads.append((L, ops, hits, len(reads) * STRIDE))
        for h in hits:
            reads.append((L, ops, [h], len(reads) * STRIDE))
    span = len(reads) * STRIDE
    wk, wr = check(e, k, CM.pack_reads(reads), span)
    assert wr.max() == 1 and wk.max() > 1
    # nothing of an empty CIGAR, nothing past a read that its CIGAR overruns
    for i, (_, ops, hits, start) in enumerate(reads):
        got = wr[start:start + STRIDE]
        if not ops:
            assert not got.any()
        if ops == cigar_cases(k, L)["longer than the read"]:
            assert not got[L - 3:].any() and got[:L - 3].any()


@pytest.mark.parametrize("k", KS)
def test_hit_patterns_within_and_across_reads(engines, k):
    e = engines(k)
    L = 4 * k + 20
    M = [(0, L)]
    reads = [
        (L, M, list(range(3, 3 + k + 3)), 0),                   # a run of k + 3 consecutive hits
        (L, M, [2, 2 + k], 1000),                               # exactly k apart
        (L, M, [2, 2 + k - 1], 2000),                           # k - 1 apart
        (L, M, [L - k], 3000),                                  # the last window
        (L, M, [L - 3], 4000),                                  # adjacent reads: this window is cut at the read's end ...
        (L, M, [1], 5000),                                      # ... and must add no depth to its neighbour's first bases
        (L, M, [5, 9], 6000), (L, M, [7], 6004),                # two reads that overlap on the reference
        (L, M, list(range(L)), -1),                             # skipped, though full of hits
        (L, M, [0], 7000),
    ]
    packed = CM.pack_reads(reads, lead=63)                      # the first read starts at bit 63 of a mask word
    span = 8000
    wk, wr = check(e, k, packed, span)
    run = wk[0:L]
    assert run.max() == k and run[3] == 1 and run[3 + k + 2] == k and run[3 + 2 * k + 1] == 1 and run[3 + 2 * k + 2] == 0
    assert (wk[1002:1002 + 2 * k] == 1).all() and wk[1002 + 2 * k] == 0
    assert wk[2002 + k - 1] == 2 and wk[2002 + k - 2] == 1
    assert (wr[3000 + L - k:3000 + L] == 1).all()
    assert (wk[4000 + L - 3:4000 + L] == 1).all() and wk[5000] == 0 and wk[5001] == 1
    assert wr[6004 + 7:6005 + 7].tolist() == [2] and wr.max() == 2
    both = wk[6000:6000 + L]
    assert both[9] == 2 and (k < 7 or both[11] == 3)
    # the same stream with a mask word boundary elsewhere
    check(e, k, CM.pack_reads(reads, lead=0), span)


@pytest.mark.parametrize("k", KS)
def test_span_clips_and_nothing_is_written_behind_it(engines, k):
    e = engines(k)
    L = 3 * k
    reads = [(L, [(0, L)], [0, k, 2 * k], 1000 - k - 2),        # runs past span = 1000
             (L, [(0, 3), (3, 5000), (0, L - 3)], [0], 10),      # its N skip jumps over the end
             (L, [(0, L)], [0], 1000),                           # starts at span
             (L, [(0, L)], [0], 1 << 40)]                        # far beyond
    wk, wr = check(e, k, CM.pack_reads(reads), 1000)
    assert (wr[1000 - k - 2:] == 1).all() and wr[10:13].tolist() == [1, 1, 1] and wr[13:100].sum() == 0


def test_a_long_read_with_many_operations(engines):
    k = 31
    e = engines(k)
    rng = np.random.default_rng(20000)
    ops, left = [], 20000
    for i in range(499):
        op = [0, 1, 0, 2, 7, 3, 8, 0, 6][i % 9]
        n = int(rng.integers(1, 70))
        if op in (0, 1, 7, 8):
            n = min(n, left - 1)
            left -= n
        ops.append((op, n))
    ops.append((0, left))
    assert len(ops) == 500 and sum(n for op, n in ops if op in (0, 1, 7, 8)) == 20000
    hits = np.flatnonzero(rng.random(20000) < 0.6).tolist() + list(range(5000, 5200))
    reads = [(100, [(0, 100)], [3], 0), (20000, ops, sorted(set(hits)), 50), (100, [(0, 100)], [0], 40000)]
    wk, wr = check(e, k, CM.pack_reads(reads), 45000)
    assert wk.max() == k and wr.sum() > 15000


@pytest.mark.parametrize("k", [5, 31])
def test_empty_inputs_prefixes_and_batches(engines, k):
    e = engines(k)
    rng = np.random.default_rng(k)
    L = 5 * k
    # (whole windows only: a window that runs past the end of a BATCH is no hit, and the batches are cut differently below)
    reads = [(L, [(4, 2), (0, L - 2)], np.flatnonzero(rng.random(L - k + 1) < 0.2).tolist(), 100 * i) for i in range(12)]
    packed = CM.pack_reads(reads)
    bits, n, offs, rs, cigar, co = packed
    span = 100 * 12 + L
    # n_reads == 0 and n_bases == 0 add nothing
    zk, zr = check(e, k, (bits, n, offs[:1], rs[:0], cigar[:0], co[:1]), span)
    assert not zk.any() and not zr.any()
    zk, zr = check(e, k, packed, span, n_bases=0)
    assert not zk.any() and not zr.any()
    # a prefix that cuts a read, with garbage in the mask at and past n_bases
    cut = int(offs[7]) + L // 2
    dirty = bits.copy()
    b = np.unpackbits(dirty.view(np.uint8), bitorder="little")
    b[cut:] = 1
    dirty = np.packbits(b, bitorder="little").view(np.uint64).copy()
    pk, pr = check(e, k, (dirty, n, offs, rs, cigar, co), span, n_bases=cut)
    clean = bits.copy()
    cb = np.unpackbits(clean.view(np.uint8), bitorder="little")
    cb[cut - k + 1:] = 0
    ck_, cr_ = check(e, k, (np.packbits(cb, bitorder="little").view(np.uint64).copy(), n, offs, rs, cigar, co), span)
    assert np.array_equal(pk, ck_) and np.array_equal(pr, cr_) and not pr[800:].any()
    # two batches accumulated equal the concatenation in one call
    whole = check(e, k, packed, span)
    first = check(e, k, CM.pack_reads(reads[:5]), span)
    both = check(e, k, CM.pack_reads(reads[5:], lead=17), span, start=first)
    assert np.array_equal(both[0], whole[0]) and np.array_equal(both[1], whole[1]) and whole[1].any()
    # the sums wrap modulo 2^32
    top = (np.full(span, 0xFFFFFFFF, np.uint32), np.full(span, 0xFFFFFFFF, np.uint32))
    wk, wr = check(e, k, packed, span, start=top)
    assert np.array_equal(wr, (whole[1].astype(np.int64) - 1).astype(np.uint32))


def test_host_form_refusals_leave_the_accumulators_alone(engines):
    from kmer_denovo_filter_amd._native import KdfError
    k = 5
    e = engines(k)
    reads = [(30, [(0, 30)], [0, 7], 0), (30, [(0, 10), (1, 2), (0, 18)], [3], 40)]
    bits, n, offs, rs, cigar, co = CM.pack_reads(reads)

    def refused(offs_, co_, cigar_=cigar):
        kc, rc = np.full(100, 7, np.uint32), np.full(100, 9, np.uint32)
        with pytest.raises(KdfError) as ei:
            e.hit_coverage(bits, n, offs_, rs, cigar_, co_, kc, rc)
        assert ei.value.code == KDF_ERR_INVALID
        assert (kc == 7).all() and (rc == 9).all()

    refused(np.array([0, 30, 20]), co)                           # decreasing read offsets
    refused(np.array([-1, 30, 60]), co)                          # a negative offset
    refused(offs, np.array([1, 1, 4]))                           # cigar_offsets[0] != 0
    refused(offs, np.array([0, 3, 1]), cigar[:1])                # decreasing cigar_offsets
    refused(offs, np.array([0, 1, 3]))                           # the last entry is not n_cigar
    kc, rc = np.zeros(100, np.uint32), np.zeros(100, np.uint32)
    rc_ = e._lib.kdf_hit_coverage(e._h, None, 0, None, -1, None, None, 0, None, None, None, 0)
    assert rc_ == KDF_ERR_INVALID                                # n_reads < 0
    e.hit_coverage(bits, n, offs, rs, cigar, co, kc, rc)         # and the engine still works
    assert rc.sum() > 0


def test_coverage_list(engines):
    from kmer_denovo_filter_amd._native import KdfError
    e = engines(31)
    rng = np.random.default_rng(5)
    N = 5000
    rc = np.zeros(N, np.uint32)
    for s in rng.integers(0, N - 80, 40).tolist():               # runs, as coverage comes
        rc[s:s + int(rng.integers(1, 80))] += 1
    rc[1024 - 3:1024 + 3] = 4                                    # a run over a block boundary of the compaction
    kc = (rc * rng.integers(1, 31, N)).astype(np.uint32)
    dk, dr = dev(kc, np.uint32), dev(rc, np.uint32)
    for first, n in ((0, N), (1000, 30), (1023, 2), (N - 1, 1), (200, 0), (0, 1025)):
        for min_reads in (0, 1, 3):
            want = CM.coverage_list(kc, rc, first, n, min_reads)
            got = e.coverage_list(kc, rc, first, n, min_reads)
            for w, g in zip(want, got):
                assert w.dtype == g.dtype and np.array_equal(w, g), (first, n, min_reads)
            m = len(want[0])
            dp = torch.full((m + GUARD,), -1, dtype=torch.int64, device="cuda")
            dko, dro = guarded(np.zeros(m, np.uint32)), guarded(np.zeros(m, np.uint32))
            torch.cuda.synchronize()
            assert e.coverage_list_dev(dk.data_ptr(), dr.data_ptr(), first, n, min_reads, dp.data_ptr(),
                                       dko.data_ptr() + 4 * GUARD, dro.data_ptr() + 4 * GUARD, m) == m
            p = dp.cpu().numpy()
            assert np.array_equal(p[:m].view(np.uint64), want[0]) and (p[m:] == -1).all()
            assert np.array_equal(unguard(dko, m), want[1]) and np.array_equal(unguard(dro, m), want[2])
            # either value column may be left out
            assert e.coverage_list_dev(None, dr.data_ptr(), first, n, min_reads, dp.data_ptr(), None, None, m) == m
            assert np.array_equal(dp.cpu().numpy()[:m].view(np.uint64), want[0])
    assert len(CM.coverage_list(kc, rc, 0, N, 1)[0]) > len(CM.coverage_list(kc, rc, 0, N, 3)[0]) > 0
    # the empty list
    z = np.zeros(300, np.uint32)
    assert all(len(a) == 0 for a in e.coverage_list(z, z, 0, 300, 1))
    # more entries than cap: the count comes back, at most cap entries are written
    total = len(CM.coverage_list(kc, rc, 0, N, 1)[0])
    cap = 10
    dp = torch.full((cap + GUARD,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    code, m = e._coverage_list_dev(dk.data_ptr(), dr.data_ptr(), 0, N, 1, dp.data_ptr(), None, None, cap)
    assert code == KDF_ERR_INVALID and m == total
    p = dp.cpu().numpy()
    assert np.array_equal(p[:cap].view(np.uint64), CM.coverage_list(kc, rc, 0, N, 1)[0][:cap]) and (p[cap:] == -1).all()
    with pytest.raises(KdfError):
        e.coverage_list(kc, rc, 0, N, 1, cap=cap)


def scanned(k, seed):
    """an engine that holds a share of the k-mers of random reads, their stream, and what a scan of it hits"""
    rng = np.random.default_rng(seed)
    reads = KT.random_reads(rng, k, 40, max_len=3 * k + 60)
    truth = KT.count_truth(reads, k)
    keys = sorted(truth)[::3]
    e = new_engine(k, hint=1 << 12)
    if e.long:
        e.add_pairs(KT.rows(keys, e.key_words), None, np.ones(len(keys), np.uint32))
    else:
        e.add_pairs(*key_args(e, keys), np.ones(len(keys), np.uint32))
    st = stream_of(reads)
    per_read, _ = KT.scan_truth(reads, k, {v: 1 for v in keys})
    return e, reads, st, per_read


@pytest.mark.parametrize("k", [31, 33, 63, 101])
def test_hit_keys_equal_the_host_codec(k):
    from kmer_denovo_filter_amd import keys as K
    from oracle import oracle as O
    e, reads, st, per_read = scanned(k, 300 + k)
    try:
        rows, bits = e.read_hits(st, want_bits=True)
        pos = e.hit_list(bits, st.n_bases)
        want_pos = np.concatenate([int(st.offsets[r]) + np.asarray(p, np.int64) for r, p in enumerate(per_read)])
        assert len(pos) > 50 and np.array_equal(pos.astype(np.int64), want_pos)
        W = e.key_words
        # the host codec on the windows' own bases
        text = "".join(s.upper() + "N" for s in reads)
        codes = np.array([["ACGT".index(c) for c in text[p:p + k]] for p in pos.tolist()], dtype=np.uint8)
        words = K.from_codes(codes, canonical=True)
        want = np.stack([np.asarray(words[j], np.uint64) for j in range(W)], axis=1)
        assert [KT.int_of_row(r) for r in want[:5]] == [KT.key_int(O.canonicalize(text[p:p + k])) for p in pos[:5].tolist()]
        # ... with two positions whose window ends past the stream
        n = st.n_bases
        ask = np.concatenate((pos, np.array([n - k + 1, n + 5], np.uint64)))
        want = np.concatenate((want, np.full((2, W), ~np.uint64(0))))
        got = e.hit_keys(st, ask)
        assert got.dtype == np.uint64 and got.shape == (len(ask), W) and np.array_equal(got, want)
        dp, dq = cuda_words(st.packed), cuda_words(ask)
        dk = torch.full((len(ask) * W + GUARD,), 0x5A5A, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.hit_keys_dev(dp.data_ptr(), n, dq.data_ptr(), len(ask), dk.data_ptr())
        e.synchronize()
        out = dk.cpu().numpy()
        assert (out[len(ask) * W:] == 0x5A5A).all() and np.array_equal(out[:len(ask) * W].view(np.uint64).reshape(-1, W), want)
    finally:
        e.close()


@pytest.mark.parametrize("k", [31, 63, 101])
def test_end_to_end_from_a_scan(k):
    e, reads, st, per_read = scanned(k, 900 + k)
    try:
        rng = np.random.default_rng(k)
        nr, n = st.n_reads, st.n_bases
        # one M over the read, a clip in front or an insertion in the middle; every third read skipped
        ops = []
        for r, s in enumerate(reads):
            L = len(s) + 1                                        # (the separator belongs to the read's stream positions)
            ops.append([[(0, L)], [(4, min(3, L)), (0, L - min(3, L))], [(0, L // 2), (1, L - L // 2 - L // 4), (0, L // 4)]][r % 3])
        cigar = np.concatenate([CM.cigar_words(o) for o in ops])
        co = np.concatenate(([0], np.cumsum([len(o) for o in ops]))).astype(np.int64)
        rs = np.where(np.arange(nr) % 4 == 3, -1, rng.integers(0, 300, nr)).astype(np.int64)
        span = 300 + max(len(s) for s in reads) + 8
        e.profile(True)
        before = e.get_stat("coverage_passes")
        dp, dm = cuda_words(st.packed), cuda_words(st.invalid)
        do = dev(st.offsets, np.int64)
        dbits = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
        drows = torch.zeros(nr, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        e.read_hits_dev(dp.data_ptr(), dm.data_ptr(), n, do.data_ptr(), nr, dbits.data_ptr(), drows.data_ptr())
        e.synchronize()
        bits = dbits.cpu().numpy().view(np.uint64)
        pos = e.hit_list(bits, n)
        assert len(pos) > 50 and len(pos) == sum(len(p) for p in per_read)
        wk, wr = np.zeros(span, np.uint32), np.zeros(span, np.uint32)
        CM.add_coverage(pos.astype(np.int64), k, st.offsets, rs, cigar, co, wk, wr)
        dk, dr = guarded(np.zeros(span, np.uint32)), guarded(np.zeros(span, np.uint32))
        ds, dc, dco = dev(rs, np.int64), dev(cigar, np.uint32), dev(co, np.int64)
        torch.cuda.synchronize()
        e.hit_coverage_dev(dbits.data_ptr(), n, do.data_ptr(), nr, ds.data_ptr(), dc.data_ptr(), len(cigar), dco.data_ptr(),
                           dk.data_ptr() + 4 * GUARD, dr.data_ptr() + 4 * GUARD, span)
        e.synchronize()
        gk, gr = unguard(dk, span), unguard(dr, span)
        assert np.array_equal(gk, wk) and np.array_equal(gr, wr) and wr.max() > 1
        lp, lk, lr = e.coverage_list(gk, gr)
        for w, g in zip(CM.coverage_list(wk, wr, 0, span, 1), (lp, lk, lr)):
            assert np.array_equal(w, g)
        assert e.get_stat("coverage_passes") >= before + 2 and e.get_stat("coverage_us") > 0
        e.profile(False)
    finally:
        e.close()
