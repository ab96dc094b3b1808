"""kdf_read_hits / kdf_hit_list on the GPU: exact equality with the model of tests/hits_truth.py AND with the two
existing calls that already hold each column -- ``KmerEngine.scan`` (`distinct`, the hit mask) and ``read_depth``
(`present`) -- at every key width: k = 5, 31, 33, 63 (one and two words) and 75, 201 (long engines)."""
import os
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest
import torch

import depth_truth as DT
import hits_truth as HT
import kmer_truth as KT
from conftest import GIAB
from oracle import oracle as O
from test_gpu_depth import cuda_words, key_args, new_engine, stream_of

pytestmark = pytest.mark.gpu

KS = [5, 31, 33, 63, 75, 201]
PATTERN64 = 0x5A5A5A5A5A5A5A5A
GUARD = 64


def vp(a):
    return a.ctypes.data_as(c_void_p)


def rnd(rng, L):
    return "".join(rng.choice(list("ACGT"), L))


def add_counted(e, keys, counts):
    """add_pairs of integer keys with their counts (a long engine takes the key rows alone, so the counts go third)"""
    if e.long:
        e.add_pairs(KT.rows(keys, e.key_words), None, counts)
    else:
        e.add_pairs(*key_args(e, keys), counts)


def dev_offsets(offs):
    return torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).cuda()


def device_rows(e, dp, dm, n, offs, want_bits=True):
    """read_hits_dev into guarded buffers (guards on BOTH sides of the rows) -> (rows, bit words or None)"""
    nr, T = len(offs) - 1, (n + 63) // 64
    do = dev_offsets(offs)
    dr = torch.full((GUARD + nr + GUARD,), PATTERN64, dtype=torch.int64, device="cuda")      # a row = 2 x uint32 = one word
    db = torch.full((T + GUARD,), PATTERN64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.read_hits_dev(dp.data_ptr(), dm.data_ptr(), n, do.data_ptr(), nr, db.data_ptr() if want_bits else None,
                    dr.data_ptr() + 8 * GUARD)
    e.synchronize()
    r, b = dr.cpu().numpy(), db.cpu().numpy()
    assert (r[:GUARD] == PATTERN64).all() and (r[GUARD + nr:] == PATTERN64).all()
    assert (b[T if want_bits else 0:] == PATTERN64).all()
    return r[GUARD:GUARD + nr].view(np.uint32).reshape(nr, 2), (b[:T].view(np.uint64) if want_bits else None)


def full_check(e, reads, k, index=None, keys=None):
    """every form of the two calls on the stream of ``reads`` against the model (``index``: what the table holds), the
    existing scan and the existing read_depth -> (rows, hit words)"""
    st = stream_of(reads)
    n, T = st.n_bases, (st.n_bases + 63) // 64
    rows, bits = e.read_hits(st, want_bits=True)
    assert rows.dtype == np.uint32 and rows.shape == (len(reads), 2) and bits.dtype == np.uint64
    if index is not None:
        want, per_read = HT.read_hits(reads, k, index, keys)
        assert np.array_equal(rows, want), f"{int((rows != want).any(axis=1).sum())} rows differ from the model"
        assert np.array_equal(bits, HT.mask_words(reads, per_read, len(bits)))
    hits, distinct = e.scan(st)
    assert np.array_equal(bits, hits)                                        # word for word, padding words included
    assert np.array_equal(rows[:, 1], distinct)
    assert np.array_equal(rows[:, 0].astype(np.uint64), e.read_depth(st, 0)[:, 1])
    assert (rows[:, 1] <= rows[:, 0]).all() and np.array_equal(rows[:, 1] == 0, rows[:, 0] == 0)
    assert np.array_equal(e.read_hits(st), rows)                             # hit_bits NULL
    drows, dbits = device_rows(e, cuda_words(st.packed), cuda_words(st.invalid), n, st.offsets)
    assert np.array_equal(drows, rows) and np.array_equal(dbits, bits[:T])
    # the list
    pos, rd = e.hit_list(bits, n, st.offsets)
    want_pos = np.flatnonzero(DT.bits(bits, n))
    assert pos.dtype == np.uint64 and rd.dtype == np.int64
    assert np.array_equal(pos, want_pos) and np.array_equal(e.hit_list(bits, n), pos)
    assert np.array_equal(rd, np.searchsorted(st.offsets, want_pos, side="right") - 1)     # (a separator is never a hit)
    assert np.array_equal(np.bincount(rd, minlength=len(reads)), rows[:, 0])
    return rows, bits


def repeat_reads(rng, k):
    """x twice forward and once as its reverse complement in ONE read; then x in two ADJACENT reads"""
    x = rnd(rng, k)
    return x, [x + "N" + x + "n" + O.reverse_complement(x), x, x]


@pytest.mark.parametrize("k", KS)
def test_random_reads_repeats_and_both_scan_paths(k):
    rng = np.random.default_rng(7000 + k)
    x, rep = repeat_reads(rng, k)
    reads = KT.random_reads(rng, k, 40, max_len=300) + rep + KT.random_reads(rng, k, 10, max_len=300)
    other = KT.random_reads(rng, k, 20, max_len=300) + reads[2:40:3] + [x]
    index = KT.count_truth(other, k)
    keys = DT.keys_of_reads(reads, k)
    with new_engine(k) as e:
        e.count(stream_of(other))
        got = []
        for fp in (0, 1):
            e.set_option("force_path", fp)
            rows, bits = full_check(e, reads, k, index, keys)
            assert e.get_stat("last_scan_path") == (3 if fp == 0 and k <= 63 else 0)
            got.append((rows, bits))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        rows = got[0][0]
        assert rows[40].tolist() == [3, 1]                                   # repeats within a read: distinct < hits
        assert rows[41].tolist() == [1, 1] and rows[42].tolist() == [1, 1]   # the same k-mer in two adjacent reads: both count it
        assert (rows[:, 1] < rows[:, 0]).any() and (rows[:, 0] == 0).any()
        if k == 5:
            assert int((rows[:, 1] < rows[:, 0]).sum()) > 10                 # random reads repeat 5-mers all the time


@pytest.mark.parametrize("k", KS)
def test_long_periodic_read_across_tiles_and_wave_spans(k):
    rng = np.random.default_rng(7100 + k)
    unit = "ACGGTCA"
    per = unit * 3000
    long_read = per[:20000]
    # a read of the same period ends at 4094, its separator is 4095: the 20 000-base read starts exactly at 4096
    reads = [per[3:3 + 4095], long_read, "", rnd(rng, k - 1), "N" * 130, "A" * (2 * k + 50), per[1:k + 20]]
    assert DT.offsets_of(reads)[1] == 4096
    index = KT.count_truth([per[:k + 7]], k)
    assert 1 <= len(index) <= 7
    ks = sorted(index)
    with new_engine(k) as e:
        add_counted(e, ks, np.ones(len(ks), np.uint32))
        rows, _ = full_check(e, reads, k, index)
        assert rows[1].tolist() == [20000 - k + 1, len(index)]               # hits >> distinct, one row
        assert rows[0].tolist() == [4095 - k + 1, len(index)]
        assert rows[2:6].tolist() == [[0, 0]] * 4                            # empty, shorter than k, all N, no hit
        assert rows[6].tolist() == [20, min(20, len(index))]


@pytest.mark.parametrize("k", KS)
def test_zero_counts_are_no_hits_and_owner_tables(k):
    rng = np.random.default_rng(7200 + k)
    x, rep = repeat_reads(rng, k)
    reads = KT.random_reads(rng, k, 30, max_len=300) + rep
    keys = DT.keys_of_reads(reads, k)
    allkeys = sorted(KT.count_truth(reads, k))
    st = stream_of(reads)
    with new_engine(k) as e:
        e.load_filter(*key_args(e, allkeys))                                 # every key stored, every count 0
        rows, bits = full_check(e, reads, k, {v: 0 for v in allkeys}, keys)
        assert not rows.any() and not bits.any()
        some = reads[1:9] + rep[:1]
        e.count_filtered(stream_of(some))
        seen = KT.count_truth(some, k)
        index = {v: seen.get(v, 0) for v in allkeys}
        assert 0 in index.values()
        rows, _ = full_check(e, reads, k, index, keys)
        assert rows.any() and (rows[:, 0] == 0).any()
        e.set_option("force_path", 1)
        assert np.array_equal(e.read_hits(st), rows)
    if k <= 63:                                                              # (hash_shift: k <= 63 engines only)
        with new_engine(k, hash_shift=2) as e:
            cnt = np.array([index[v] for v in allkeys], np.uint32)
            add_counted(e, allkeys, cnt)
            assert np.array_equal(full_check(e, reads, k, index, keys)[0], rows)
    with new_engine(k, key_parts=3, key_part=1) as e:                        # the slice the table holds
        e.count(st)
        part, _ = full_check(e, reads, k)
        whole = HT.read_hits(reads, k, KT.count_truth(reads, k), keys)[0]
        assert (part <= whole).all() and part.any() and (part[:, 0] < whole[:, 0]).any()


def dirty_buffers(st, n_cut, mask_fill):
    """device stream buffers of the kdf_stream_words(n_cut) sizes: the stream below n_cut, every packed bit at and past
    n_cut set, every mask bit there ``mask_fill``"""
    from kmer_denovo_filter_amd.reads import stream_words
    pw, mw = stream_words(n_cut)
    P = np.full(pw, 0xFFFFFFFFFFFFFFFF, np.uint64)
    M = np.full(mw, 0xFFFFFFFFFFFFFFFF if mask_fill else 0, np.uint64)
    a, b = n_cut // 32, n_cut // 64
    P[:a] = st.packed[:a]
    M[:b] = st.invalid[:b]
    if n_cut % 32:
        keep = np.uint64((1 << (2 * (n_cut % 32))) - 1)
        P[a] = (st.packed[a] & keep) | ~keep
    if n_cut % 64:
        keep = np.uint64((1 << (n_cut % 64)) - 1)
        M[b] = (st.invalid[b] & keep) | (~keep if mask_fill else np.uint64(0))
    return cuda_words(P), cuda_words(M)


@pytest.mark.parametrize("k", KS)
def test_dirty_tail_prefix_and_partial_offsets(k):
    rng = np.random.default_rng(7300 + k)
    genome = rnd(rng, 3000)
    reads = [genome[s:s + L] for s, L in zip(rng.integers(0, 2000, 24).tolist(), rng.integers(k, k + 400, 24).tolist())]
    reads[5] = "T" * (k + 30)                                                # what an all-ones packed tail reads as
    reads[12] = genome[100:100 + k + 200]                                    # the read the prefix cuts
    st = stream_of(reads)
    index = KT.count_truth(reads[::2] + ["T" * k], k)
    ks = sorted(index)
    with new_engine(k) as e:
        add_counted(e, ks, np.ones(len(ks), np.uint32))
        rows, bits = full_check(e, reads, k, index)
        assert rows[5].tolist() == [31, 1]
        # the whole stream in dirty buffers
        for mask_fill in (1, 0):
            dp, dm = dirty_buffers(st, st.n_bases, mask_fill)
            drows, dbits = device_rows(e, dp, dm, st.n_bases, st.offsets)
            assert np.array_equal(drows, rows) and np.array_equal(dbits, bits[:(st.n_bases + 63) // 64])
        # a prefix that cuts read m: offsets[n_reads] > n_bases
        m = 12
        cut = len(reads[m]) // 2 + 7
        n_cut = int(st.offsets[m]) + cut
        trunc = reads[:m] + [reads[m][:cut]]
        want, per_read = HT.read_hits(trunc, k, index)
        T = (n_cut + 63) // 64
        for mask_fill in (1, 0):
            dp, dm = dirty_buffers(st, n_cut, mask_fill)
            drows, dbits = device_rows(e, dp, dm, n_cut, st.offsets[:m + 2])
            assert np.array_equal(drows, want)
            assert np.array_equal(dbits, HT.mask_words(trunc, per_read, T + 1)[:T])
            assert not DT.bits(dbits, T * 64)[max(n_cut - k + 1, 0):].any()
        host = e.read_hits(type(st)(st.packed, st.invalid, n_cut, st.offsets[:m + 2]))
        assert np.array_equal(host, want)
        # offsets that cover only the middle reads: the rows of those reads; outside positions belong to no read
        a, b = 7, 17
        mid = st.offsets[a:b + 1]
        drows, _ = device_rows(e, cuda_words(st.packed), cuda_words(st.invalid), st.n_bases, mid, want_bits=False)
        assert np.array_equal(drows, rows[a:b])
        pos, rd = e.hit_list(bits, st.n_bases, mid)
        full = np.searchsorted(st.offsets, pos.astype(np.int64), side="right") - 1
        assert np.array_equal(rd, np.where((full >= a) & (full < b), full - a, -1))
        assert (rd == -1).any() and (rd >= 0).any()


def test_hit_list_cap_and_empty_mask():
    from kmer_denovo_filter_amd import _native
    k = 31
    rng = np.random.default_rng(7400)
    reads = [rnd(rng, 500) for _ in range(6)]
    st = stream_of(reads)
    with new_engine(k) as e:
        e.count(stream_of(reads[::2]))
        rows, bits = e.read_hits(st, want_bits=True)
        n = int(rows[:, 0].sum())
        want = np.flatnonzero(DT.bits(bits, st.n_bases))
        assert n == len(want) == 3 * (500 - k + 1)
        T = (st.n_bases + 63) // 64
        db, do = cuda_words(bits[:T]), dev_offsets(st.offsets)
        for cap in (n + 5, n, n - 1, 1, 0):
            dpos = torch.full((cap + GUARD,), PATTERN64, dtype=torch.int64, device="cuda")
            drd = torch.full((cap + GUARD,), PATTERN64, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            rc, got = e._hit_list_dev(db.data_ptr(), st.n_bases, do.data_ptr(), st.n_reads, dpos.data_ptr(), drd.data_ptr(), cap)
            assert got == n and rc == (_native.KDF_ERR_INVALID if cap < n else 0)
            p, r = dpos.cpu().numpy(), drd.cpu().numpy()
            w = min(cap, n)
            assert np.array_equal(p[:w], want[:w]) and (p[w:] == PATTERN64).all() and (r[w:] == PATTERN64).all()   # the guard past cap
            assert np.array_equal(r[:w], np.searchsorted(st.offsets, want[:w], side="right") - 1)
            if cap < n:
                with pytest.raises(_native.KdfError):
                    e.hit_list_dev(db.data_ptr(), st.n_bases, None, 0, dpos.data_ptr(), None, cap)
        # host form, cap = n - 1
        pos = np.full(n + 1, 7, np.uint64)
        nout = c_uint64(0)
        rc = e._lib.kdf_hit_list(e._h, vp(bits), st.n_bases, None, 0, vp(pos), None, n - 1, byref(nout))
        assert rc == _native.KDF_ERR_INVALID and nout.value == n
        assert np.array_equal(pos[:n - 1], want[:n - 1]) and (pos[n - 1:] == 7).all()
        # only the bits below n_bases count
        cutn = int(want[len(want) // 2])
        assert np.array_equal(e.hit_list(bits, cutn), want[want < cutn])
        # n == 0
        zero = np.zeros_like(bits)
        p0, r0 = e.hit_list(zero, st.n_bases, st.offsets)
        assert len(p0) == 0 and len(r0) == 0
        assert e._hit_list_dev(cuda_words(zero).data_ptr(), st.n_bases, None, 0, None, None, 0) == (0, 0)
        assert e._hit_list_dev(None, 0, None, 0, None, None, 0) == (0, 0)


def test_arguments_empty_inputs_garbage_offsets_and_profile():
    from kmer_denovo_filter_amd import ReadStream, _native
    k = 5
    rng = np.random.default_rng(7500)
    reads = [rnd(rng, 80) for _ in range(40)]
    st = stream_of(reads)
    with new_engine(k) as e:
        e.count(st)
        lib, h = e._lib, e._h
        want = e.read_hits(st)
        rows = np.full((st.n_reads, 2), 7, np.uint32)
        offs = np.ascontiguousarray(st.offsets, np.int64)
        for bad in (offs[::-1].copy(), np.concatenate([[-1], offs[1:]]), np.concatenate([offs[:3], [offs[2] - 1], offs[4:]])):
            bad = np.ascontiguousarray(bad, np.int64)
            assert lib.kdf_read_hits(h, vp(st.packed), vp(st.invalid), st.n_bases, vp(bad), st.n_reads, None, vp(rows)) == _native.KDF_ERR_INVALID
        assert lib.kdf_read_hits(h, vp(st.packed), vp(st.invalid), st.n_bases, vp(offs), -1, None, vp(rows)) == _native.KDF_ERR_INVALID
        assert lib.kdf_hit_list(h, vp(st.invalid), st.n_bases, vp(offs), -1, vp(rows), None, 0, byref(c_uint64(0))) == _native.KDF_ERR_INVALID
        assert (rows == 7).all()
        assert lib.kdf_read_hits(h, vp(st.packed), vp(st.invalid), st.n_bases, vp(offs), 0, None, None) == 0
        assert lib.kdf_read_hits(h, None, None, 0, None, 0, None, None) == 0
        assert lib.kdf_read_hits_dev(h, None, None, 0, None, 0, None, None) == 0
        assert (rows == 7).all()
        empty = ReadStream.empty()
        assert e.read_hits(empty).shape == (0, 2)
        assert lib.kdf_read_hits(h, None, None, 0, vp(offs), st.n_reads, None, vp(rows)) == 0 and not rows.any()    # no base: zero rows
        # the device form's offsets are a precondition -- but whatever they hold, no write lands outside the rows
        dp, dm = cuda_words(st.packed), cuda_words(st.invalid)
        garbage = rng.integers(-2 ** 62, 2 ** 62, st.n_reads + 1)
        garbage[::5] = rng.integers(0, st.n_bases, len(garbage[::5]))
        for g in (garbage, np.full(st.n_reads + 1, -3), offs[::-1].copy()):
            device_rows(e, dp, dm, st.n_bases, g)
        assert np.array_equal(device_rows(e, dp, dm, st.n_bases, offs)[0], want)
        # under kdf_profile the new kernels are timed, one pass per call
        e.profile(True)
        _, bits = e.read_hits(st, want_bits=True)
        e.hit_list(bits, st.n_bases)
        assert e.get_stat("hits_passes") == 2 and e.get_stat("hits_us") > 0
        e.profile(False)
        assert e.get_stat("hits_passes") == 0


def test_run_to_run_on_one_long_lived_engine():
    """the scratch (hit list, pair set) is kept between calls: a small batch after a large one, and the large one again"""
    k = 31
    rng = np.random.default_rng(7600)
    genome = rnd(rng, 20000)
    big = [genome[s:s + 150] for s in rng.integers(0, 19850, 3000).tolist()] + [genome]
    small = [genome[100:260], rnd(rng, 150), genome[5000:5100] + "N" + genome[5000:5100]]
    with new_engine(k) as e:
        e.count(stream_of([genome[:12000]]))
        index = KT.count_truth([genome[:12000]], k)
        sb, ss = stream_of(big), stream_of(small)
        first = e.read_hits(sb)
        assert first[-1].tolist() == [12000 - k + 1, 12000 - k + 1] and first[:, 0].sum() > 200000
        got_small = e.read_hits(ss)
        assert np.array_equal(got_small, HT.read_hits(small, k, index)[0]) and got_small[2].tolist() == [140, 70]
        for _ in range(2):
            assert np.array_equal(e.read_hits(sb), first) and np.array_equal(e.read_hits(ss), got_small)
        assert np.array_equal(first[:, 1], e.scan(sb)[1]) and np.array_equal(first[:, 0].astype(np.uint64), e.read_depth(sb)[:, 1])


def _same_informative(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x.query_name, x.flag, x.ref_id, x.pos, x.n_distinct) == (y.query_name, y.flag, y.ref_id, y.pos, y.n_distinct)
        assert x.kmer_hit_indices.dtype == y.kmer_hit_indices.dtype and np.array_equal(x.kmer_hit_indices, y.kmer_hit_indices)


def test_mirror_with_device_hits_equals_the_default_path(trio_reads, monkeypatch):
    from kmer_denovo_filter_amd.core import bam_scanner
    from kmer_denovo_filter_amd.reads import FLAG_OFF_MODULE3, bam_reader
    k = 31
    child = os.path.join(GIAB, "HG002_child.bam")
    kmers = set()
    for s in trio_reads["child"][::60]:
        S = s.upper()
        for i in range(0, len(S) - k + 1, 9):
            if set(S[i:i + k]) <= set("ACGT"):
                kmers.add(O.canonicalize(S[i:i + k]))
    assert len(kmers) > 500
    bam_scanner._init_scan_worker(kmers, k, 1)
    try:
        for min_dk in (0, 1, 3):
            monkeypatch.delenv("KDF_DEVICE_HITS", raising=False)
            base = list(bam_scanner.scan_bam_for_hits(child, min_dk_per_read=min_dk))
            monkeypatch.setenv("KDF_DEVICE_HITS", "1")
            dev = list(bam_scanner.scan_bam_for_hits(child, min_dk_per_read=min_dk))
            assert [n for n, _ in base] == [n for n, _ in dev] and sum(len(o) for _, o in base) > 0
            for (_, x), (_, y) in zip(base, dev):
                _same_informative(x, y)
            if min_dk == 0:
                assert sum(len(o) for _, o in base) == sum(n for n, _ in base)      # every read kept
            else:
                assert 0 < sum(len(o) for _, o in base) < sum(n for n, _ in base)
        monkeypatch.delenv("KDF_DEVICE_HITS", raising=False)
        eng = bam_scanner._worker_engine
        with bam_reader(child, flag_off=FLAG_OFF_MODULE3, collapse=False, max_bases=bam_scanner.SCAN_BATCH_BASES,
                        max_reads=1 << 20, threads=2, want_meta=True) as rd:
            for batch in rd:
                hits, distinct = eng.scan(batch)
                for min_dk in (0, 1, 3):
                    idx, d, per_read = eng.scan_informative(batch, min_dk)
                    keep = np.flatnonzero(distinct >= min_dk) if min_dk > 0 else np.arange(batch.n_reads)
                    assert np.array_equal(idx, keep) and np.array_equal(d, distinct[keep]) and len(per_read) == len(keep)
                    from kmer_denovo_filter_amd import hit_positions
                    for r, p in list(zip(keep.tolist(), per_read))[::7]:
                        assert np.array_equal(p, hit_positions(hits, int(batch.offsets[r]), int(batch.offsets[r + 1]) - 1))
    finally:
        bam_scanner._worker_engine.close()
        bam_scanner._worker_engine = None
