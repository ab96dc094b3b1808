"""kdf_window_counts / kdf_read_depth on the GPU against the model of tests/depth_truth.py: exact equality everywhere.

Small cases: every key width, tables made three ways, host and device forms, the scan invariant on both scan paths,
saturated counters, deferred work, key_parts, owner tables, and that the table is left as it was.  Then the mini trio
(the read-level form of the discovery chain's parent filter) and the two Python mirrors."""
import numpy as np
import pytest
import torch

import depth_truth as DT
import kmer_truth as KT
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KS = [5, 15, 31, 32, 33, 47, 63, 75, 101, 201]
LOWS = (0, 1, 2, 2 ** 32 - 1)
PATTERN32, PATTERN64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 256


def new_engine(k, hint=1 << 16, **opts):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=hint)
    for name, v in opts.items():
        e.set_option(name, v)
    return e


def stream_of(reads):
    from kmer_denovo_filter_amd import ReadStream
    st = ReadStream.from_strings(reads)
    assert np.array_equal(st.offsets, DT.offsets_of(reads)) and st.n_bases == int(st.offsets[-1])
    return st


def key_args(e, keys):
    """the (lo, hi) / rows arguments of add_pairs, load_filter and query for a list of integer keys"""
    if e.long:
        return (KT.rows(keys, e.key_words),)
    lo, hi = KT.lohi(keys)
    return (lo, hi if e.wide else None)


def handmade(k, rng):
    """shorter than k, exactly k, empty, all N, N every k-th base, lower case, several hundred tiles, many reads per tile"""
    def rd(L):
        return "".join(rng.choice(list("ACGT"), L))
    every = list(rd(6 * k + 3))
    every[k - 1::k] = "N" * len(every[k - 1::k])
    out = [rd(k - 1), rd(k), "", "N" * 70, "".join(every), rd(3 * k + 5).lower(), rd(64 * 300 + 17)]
    out += [rd(int(rng.integers(1, 4))) for _ in range(3000)]
    out += [rd(2 * k + 40)]
    return out


_WORK = {}


def workload(k):
    """(reads, their model keys, other reads) for one k, built once"""
    if k not in _WORK:
        rng = np.random.default_rng(500 + k)
        genome = "".join(rng.choice(list("ACGT"), 6000))
        reads = KT.random_reads(rng, k, 40, genome=genome, max_len=400) + handmade(k, rng)
        other = KT.random_reads(rng, k, 30, max_len=400) + reads[3:40:4]
        _WORK[k] = (reads, DT.keys_of_reads(reads, k), other)
    return _WORK[k]


def make_table(e, kind, reads, other, k):
    """fill ``e`` -> the {key: count} it must hold.  same: counted from the reads; other: counted from other reads (most
    windows absent); filter: every key of the reads loaded as a filter, a few of the reads counted into it (most keys
    stay stored with count 0)"""
    if kind == "same":
        e.count(stream_of(reads))
        return KT.count_truth(reads, k)
    if kind == "other":
        e.count(stream_of(other))
        return KT.count_truth(other, k)
    assert kind == "filter"
    allkeys = sorted(KT.count_truth(reads, k))
    e.load_filter(*key_args(e, allkeys))
    some = reads[1:4] + reads[-1:]
    e.count_filtered(stream_of(some))
    seen = KT.count_truth(some, k)
    index = {v: seen.get(v, 0) for v in allkeys}
    assert 0 in index.values() and max(index.values()) > 0
    return index


def cuda_words(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def device_forms(e, st, low_max, want_valid=True):
    """window_counts_dev and read_depth_dev into guarded buffers -> (counts, valid words or None, rows); the guards
    must keep their pattern"""
    n, nr = st.n_bases, st.n_reads
    T = (n + 63) // 64
    dp, dm = cuda_words(st.packed), cuda_words(st.invalid)
    do = torch.from_numpy(np.ascontiguousarray(st.offsets, dtype=np.int64)).cuda()
    dc = torch.full((n + GUARD,), PATTERN32, dtype=torch.int32, device="cuda")
    dv = torch.full((T + GUARD,), PATTERN64, dtype=torch.int64, device="cuda")
    dr = torch.full((nr * 6 + GUARD,), PATTERN64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    e.window_counts_dev(dp.data_ptr(), dm.data_ptr(), n, dc.data_ptr(), dv.data_ptr() if want_valid else None)
    e.read_depth_dev(dp.data_ptr(), dm.data_ptr(), n, do.data_ptr(), nr, low_max, dr.data_ptr())
    e.synchronize()
    c, v, r = dc.cpu().numpy(), dv.cpu().numpy(), dr.cpu().numpy()
    assert (c[n:] == PATTERN32).all() and (r[nr * 6:] == PATTERN64).all()
    assert (v[T if want_valid else 0:] == PATTERN64).all()
    return c[:n].view(np.uint32), (v[:T].view(np.uint64) if want_valid else None), r[:nr * 6].view(np.uint64).reshape(nr, 6)


def numpy_rows(counts, valid, offs, low_max):
    """the six columns as a numpy reduction of the per-position arrays over the same offsets"""
    rows = np.zeros((len(offs) - 1, 6), np.uint64)
    c64 = np.where(valid, counts, 0).astype(np.uint64)
    cv = np.concatenate([[0], np.cumsum(valid)]).astype(np.uint64)
    cp = np.concatenate([[0], np.cumsum(valid & (counts > 0))]).astype(np.uint64)
    cl = np.concatenate([[0], np.cumsum(valid & (counts <= low_max))]).astype(np.uint64)
    cs = np.concatenate([[0], np.cumsum(c64)]).astype(np.uint64)
    a, b = offs[:-1], offs[1:]
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 5] = cv[b] - cv[a], cp[b] - cp[a], cl[b] - cl[a], cs[b] - cs[a]
    for r in np.flatnonzero(rows[:, 0]):
        c = counts[a[r]:b[r]][valid[a[r]:b[r]]]
        rows[r, 3], rows[r, 4] = c.min(), c.max()
    return rows


@pytest.mark.parametrize("kind", ["same", "other", "filter"])
@pytest.mark.parametrize("k", KS)
def test_counts_and_rows_equal_model(k, kind):
    reads, keys, other = workload(k)
    st = stream_of(reads)
    n, T = st.n_bases, (st.n_bases + 63) // 64
    with new_engine(k) as e:
        index = make_table(e, kind, reads, other, k)
        want_c, want_v, offs = DT.profile(reads, k, index, keys)
        assert want_v.any() and (want_c > 0).any()
        before = (e.histogram(64).tolist(), e.count_stats(), e.stats())
        # host forms, valid_bits_out NULL and not
        c0 = e.window_counts(st)
        c1, v1 = e.window_counts(st, want_valid=True)
        assert c0.dtype == np.uint32 and np.array_equal(c0, want_c) and np.array_equal(c1, want_c)
        assert np.array_equal(DT.bits(v1, n), want_v) and not v1[T:].any()
        if n % 64:
            assert int(v1[T - 1]) >> (n % 64) == 0
        for low_max in LOWS:
            want_r = DT.depth_rows(reads, k, index, low_max, keys)
            rows = e.read_depth(st, low_max)
            assert rows.dtype == np.uint64 and rows.shape == (len(reads), 6)
            assert np.array_equal(rows, want_r), f"low_max={low_max}: {int((rows != want_r).any(axis=1).sum())} rows differ"
            assert np.array_equal(rows, numpy_rows(c0, want_v, offs, low_max))
            dc, dv, dr = device_forms(e, st, low_max, want_valid=low_max != 1)
            assert np.array_equal(dc, c0) and np.array_equal(dr, rows)
            if dv is not None:
                assert np.array_equal(dv, v1[:T])
        assert np.array_equal(e.read_depth(st, LOWS[-1]), rows)                    # (run to run)
        assert (e.histogram(64).tolist(), e.count_stats(), e.stats()) == before    # the table is only read
        # the scan is one bit of it, on both scan paths
        rows0 = e.read_depth(st, 0)
        for fp in (0, 1):
            e.set_option("force_path", fp)
            hits, distinct = e.scan(st)
            assert e.get_stat("last_scan_path") == (3 if fp == 0 and k <= 63 else 0)
            assert np.array_equal(DT.bits(hits, n), want_c != 0), f"force_path={fp}"
            assert (distinct <= rows0[:, 1]).all() and np.array_equal(distinct == 0, rows0[:, 1] == 0)
            assert np.array_equal(e.window_counts(st), want_c) and np.array_equal(e.read_depth(st, 0), rows0)
        # (the direct scan kernel adds the windows it saw to kdf_stats' `windows`: everything but that counter)
        assert (e.histogram(64).tolist(), e.count_stats(), e.stats()[:2]) == before[:2] + (before[2][:2],)


@pytest.mark.parametrize("k", [31, 63, 101])
def test_saturated_counter_reads_as_stored(k):
    rng = np.random.default_rng(k)
    x = "".join(rng.choice(list("ACGT"), k))
    key = KT.key_int(O.canonicalize(x))
    reads = [x + "N" + O.reverse_complement(x), x[:-1]]
    with new_engine(k) as e:
        if e.long:
            e.add_pairs(KT.rows([key], e.key_words), None, np.array([2 ** 32 - 1], np.uint32))
        else:
            lo, hi = KT.lohi([key])
            e.add_pairs(lo, hi if e.wide else None, np.array([2 ** 32 - 1], np.uint32))
        st = stream_of(reads)
        c = e.window_counts(st)
        assert int(c[0]) == int(c[k + 1]) == 2 ** 32 - 1 and int(c.astype(np.uint64).sum()) == 2 * (2 ** 32 - 1)
        rows = e.read_depth(st, 5)
        assert rows[0].tolist() == [2, 2, 0, 2 ** 32 - 1, 2 ** 32 - 1, 2 * (2 ** 32 - 1)]
        assert rows[1].tolist() == [0] * 6
        assert e.read_depth(st, 2 ** 32 - 1)[0, 2] == 2


@pytest.mark.parametrize("k", [31, 47, 101])
def test_deferred_count_work_is_applied_first(k):
    reads, keys, other = workload(k)
    st = stream_of(reads)
    index = KT.count_truth(reads + other, k)
    want_c, _, _ = DT.profile(reads, k, index, keys)
    with new_engine(k) as e:
        e.count(stream_of(reads)); e.count(stream_of(other))
        assert e.long or e.get_stat("pending_positions") > 0        # (a long engine counts at the call: nothing to defer)
        c = e.window_counts(st)
        assert e.get_stat("pending_positions") == 0
        e.flush()
        assert np.array_equal(c, want_c) and np.array_equal(e.window_counts(st), c)
    with new_engine(k) as e:
        e.count(stream_of(reads)); e.count(stream_of(other))
        assert e.long or e.get_stat("pending_positions") > 0
        rows = e.read_depth(st, 1)
        assert e.get_stat("pending_positions") == 0
        assert np.array_equal(rows, DT.depth_rows(reads, k, index, 1, keys))


@pytest.mark.parametrize("k", [31, 63, 75])
def test_key_parts_slices_sum_to_the_whole(k):
    reads, keys, other = workload(k)
    st = stream_of(reads)
    want_c, _, _ = DT.profile(reads, k, KT.count_truth(reads, k), keys)
    total = np.zeros(st.n_bases, np.uint64)
    sums = []
    for part in range(3):
        with new_engine(k, key_parts=3, key_part=part) as e:
            e.count(st)
            c = e.window_counts(st)
            rows = e.read_depth(st, 0)
        assert np.array_equal(rows[:, 5], numpy_rows(c, DT.profile(reads, k, {}, keys)[1], st.offsets, 0)[:, 5])
        total += c
        sums.append(int(c.astype(np.uint64).sum()))
    assert np.array_equal(total, want_c.astype(np.uint64)) and all(s > 0 for s in sums)


@pytest.mark.parametrize("k", [31, 63])
def test_owner_table_reads_like_a_plain_table(k):
    reads, keys, other = workload(k)
    st = stream_of(reads)
    index = KT.count_truth(reads[::2] + other, k)
    ks = sorted(index)
    cnt = np.array([index[v] for v in ks], np.uint32)
    got = []
    for shift in (0, 2):
        with new_engine(k, hash_shift=shift) as e:
            assert e.get_stat("hash_shift") == shift
            e.add_pairs(*key_args(e, ks), cnt)
            got.append((e.window_counts(st), e.read_depth(st, 2)))
    want_c, _, _ = DT.profile(reads, k, index, keys)
    assert np.array_equal(got[0][0], want_c) and np.array_equal(got[1][0], want_c)
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[1][1], DT.depth_rows(reads, k, index, 2, keys))


def test_arguments_and_empty_inputs():
    from ctypes import c_void_p
    from kmer_denovo_filter_amd import ReadStream, _native
    reads = ["ACGTACGTACGTACGTAAAC", "GGGTTTACGTACGTACGTAC"]
    st = stream_of(reads)
    vp = lambda a: a.ctypes.data_as(c_void_p)
    with new_engine(5) as e:
        e.count(st)
        lib, h = e._lib, e._h
        rows = np.full((2, 6), 7, np.uint64)
        for bad in ([0, 30, 21], [-1, 21, 42], [5, 4, 42]):
            offs = np.array(bad, np.int64)
            assert lib.kdf_read_depth(h, vp(st.packed), vp(st.invalid), st.n_bases, vp(offs), 2, 0, vp(rows)) == _native.KDF_ERR_INVALID
        offs = np.ascontiguousarray(st.offsets, np.int64)
        assert lib.kdf_read_depth(h, vp(st.packed), vp(st.invalid), st.n_bases, vp(offs), -1, 0, vp(rows)) == _native.KDF_ERR_INVALID
        assert (rows == 7).all()
        assert lib.kdf_read_depth(h, vp(st.packed), vp(st.invalid), st.n_bases, vp(offs), 0, 0, vp(rows)) == 0
        assert lib.kdf_read_depth_dev(h, None, None, 0, None, 0, 0, None) == 0
        assert lib.kdf_window_counts_dev(h, None, None, 0, None, None) == 0
        assert (rows == 7).all()
        empty = ReadStream.empty()
        assert e.window_counts(empty).shape == (0,) and e.read_depth(empty).shape == (0, 6)
        # offsets of a prefix: the rows of the reads named, the windows outside them in no row
        first = e.read_depth(ReadStream(st.packed, st.invalid, st.n_bases, st.offsets[:2]), 0)
        assert np.array_equal(first, e.read_depth(st, 0)[:1])
        last = e.read_depth(ReadStream(st.packed, st.invalid, st.n_bases, st.offsets[1:]), 0)
        assert np.array_equal(last, e.read_depth(st, 0)[1:])
        # under kdf_profile the kernels are timed
        e.profile(True)
        e.window_counts(st); e.read_depth(st)
        assert e.get_stat("depth_passes") == 2 and e.get_stat("depth_us") >= 0
        e.profile(False)
        assert e.get_stat("depth_passes") == 0


def test_mini_trio_read_depth_against_both_parents(oracle, trio_reads):
    """The read-level form of the parent filter on the mini trio: read_depth(low_max = 0) of the child's reads against the
    mother's and the father's counted tables equals the model, and every child read that holds one of the chain's 630
    proband-unique k-mers shows a window absent from either parent."""
    from test_depth_host import proband_reads, table_index
    child = trio_reads["child"]
    keys = DT.keys_of_reads(child, 31)
    holders, n_unique = proband_reads(oracle, trio_reads, keys)
    assert n_unique == 630 and len(holders) > 0
    st = stream_of(child)
    for who in ("mother", "father"):
        index = table_index(oracle.OracleTable(31, 1 << 20).count_reads(trio_reads[who]))
        with new_engine(31, 1 << 20) as e:
            e.count(stream_of(trio_reads[who]))
            rows = e.read_depth(st, 0)
            c = e.window_counts(st)
        assert np.array_equal(rows, DT.depth_rows(child, 31, index, 0, keys)), who
        assert np.array_equal(c, DT.profile(child, 31, index, keys)[0]), who
        assert (rows[holders, 2] >= 1).all() and (rows[holders, 3] == 0).all(), who


def test_python_mirrors(tmp_path):
    from kmer_denovo_filter_amd import jf_io
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _jellyfish_query_sequences
    from kmer_denovo_filter_amd.kmer_utils import JellyfishKmerQuery
    k = 31
    reads, keys, other = workload(k)
    seqs = reads[:44] + reads[-1:]
    index = KT.count_truth(other, k)
    want = [[(i, index.get(v, 0)) for i, v in DT.read_keys(s, k)] for s in seqs]
    assert any(c for pairs in want for _, c in pairs)
    with new_engine(k) as e:
        e.count(stream_of(other))
        assert _jellyfish_query_sequences(e, seqs) == want
    ks = sorted(index)
    lo, hi = KT.lohi(ks)
    path = str(tmp_path / "other.jf")
    jf_io.write_index(path, k, lo, None, np.array([index[v] for v in ks], np.uint32))
    assert _jellyfish_query_sequences(path, seqs) == want
    q = JellyfishKmerQuery(path)
    for s, pairs in zip(seqs[:12], want[:12]):
        got = q.query_read(s, k)
        d = dict(pairs)
        assert got == [d.get(i) for i in range(max(len(s) - k + 1, 0))]
    q.release()
