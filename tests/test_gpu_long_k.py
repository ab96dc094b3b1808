"""Long k-mers (odd k from 65 to 201) on the GPU, checked against the oracle's string rules (py_count, canonicalize,
kmer_to_int), which hold for any k.  Keys are (n, W) uint64 rows, word 0 the least significant."""
import numpy as np
import pytest

from kmer_denovo_filter_amd import KmerEngine, ReadStream
from kmer_denovo_filter_amd.engine import key_words
from kmer_denovo_filter_amd._native import KdfError

pytestmark = pytest.mark.gpu

KS = (65, 95, 97, 127, 129, 159, 161, 191, 193, 201)
M64 = (1 << 64) - 1


def words_of(v: int, W: int):
    return [(v >> (64 * j)) & M64 for j in range(W)]


def rows_of(kmers, k, O):
    W = key_words(k)
    a = np.array([words_of(O.kmer_to_int(O.canonicalize(s.upper())), W) for s in kmers], dtype=np.uint64)
    return a.reshape(len(kmers), W)


def int_of_row(row):
    return sum(int(x) << (64 * j) for j, x in enumerate(row))


def expected(reads, k, O, filt=None):
    """py_count as ascending (int key, count) arrays."""
    d = O.py_count(reads, k, filt)
    items = sorted((O.kmer_to_int(s), c) for s, c in d.items())
    return [v for v, _ in items], np.array([c for _, c in items], dtype=np.uint32)


def got_sorted(keys, cnt):
    return [int_of_row(r) for r in keys], cnt


def mixed_reads(rng, k, n=120):
    """N / IUPAC / lowercase bases; reads shorter than k, exactly k, and up to 1000 bp."""
    genome = "".join(rng.choice(list("ACGT"), 6000))
    reads = []
    for i in range(n):
        L = [k - 1, k, k + 1, int(rng.integers(k, 1001))][i % 4]
        s = int(rng.integers(0, len(genome) - L))
        r = list(genome[s:s + L])
        for j in range(L):
            x = rng.random()
            if x < 0.004:
                r[j] = "N"
            elif x < 0.006:
                r[j] = str(rng.choice(list("RYKMSWBDHV")))
            elif x < 0.05:
                r[j] = r[j].lower()
        reads.append("".join(r))
    return reads


@pytest.mark.parametrize("k", KS)
def test_full_dump_matches_py_count(k, oracle):
    rng = np.random.default_rng(k)
    reads = mixed_reads(rng, k)
    want_keys, want_cnt = expected(reads, k, oracle)
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        assert e.long and e.key_words == (2 * k + 63) // 64
        e.count(ReadStream.from_strings(reads))
        assert e.get_stat("last_count_path") == 0
        keys, hi, cnt = e.export_ge(0)
        assert hi is None and keys.shape == (len(want_keys), e.key_words) and keys.flags.c_contiguous
        gk, gc = got_sorted(keys, cnt)
        assert gk == want_keys                      # ascending key order, every key
        assert np.array_equal(gc, want_cnt)
        _, distinct, windows = e.stats()
        assert distinct == len(want_keys) and windows == int(want_cnt.sum())
        # dump -L 2 and count_ge
        assert e.count_ge(2) == int((want_cnt >= 2).sum())
        k2, _, c2 = e.export_ge(2)
        assert [int_of_row(r) for r in k2] == [v for v, c in zip(want_keys, want_cnt) if c >= 2]


def test_stream_ending_at_buffer_edge(oracle):
    """>= 10^6 windows at k = 101 in device buffers sized exactly by kdf_stream_words, one read ending at the last base
    (no separator).  The mask bits past n_bases are left CLEAR and the packed words there are 0 (all A): only the
    kernel's "positions at or past n_bases are invalid" rule keeps the windows that would run past the end out."""
    import torch
    from kmer_denovo_filter_amd.reads import stream_words
    k, n = 101, 1_000_000 + 100 + 37
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 4, n).astype(np.uint64)
    pw, mw = stream_words(n)
    packed = np.zeros(pw, np.uint64)
    idx = np.arange(n)
    np.bitwise_or.at(packed, idx >> 5, codes << ((idx & 31) * 2).astype(np.uint64))
    invalid = np.zeros(mw, np.uint64)                          # every mask bit clear, past n_bases too
    dp = torch.from_numpy(packed.view(np.int64)).cuda()
    dm = torch.from_numpy(invalid.view(np.int64)).cuda()
    torch.cuda.synchronize()
    seq = "".join("ACGT"[c] for c in codes.tolist())
    with KmerEngine(k, capacity_hint=1 << 21) as e:
        e.count_dev(dp.data_ptr(), dm.data_ptr(), n)
        _, distinct, windows = e.stats()
        assert windows == n - k + 1
        last = seq[n - k:]
        first = seq[:k]
        q = e.query(rows_of([first, last, seq[n // 2:n // 2 + k]], k, oracle))
        assert q.min() >= 1
        assert e.count_ge(0) == distinct
        keys, _, cnt = e.export_ge(0)
        assert int(cnt.sum()) == n - k + 1
    # the distinct count by the string rule
    want = {oracle.canonicalize(seq[i:i + k]) for i in range(n - k + 1)}
    assert distinct == len(want)


def test_high_copy_repeat_pending_path(oracle):
    """One k-mer thousands of times inside each wave: claimers and matchers of the same key collide (PENDING /
    BLOCKED)."""
    k = 101
    reads = ["A" * 6000, "ACGTTGCA" * 800, "a" * 3000 + "N" + "T" * 2000]
    want_keys, want_cnt = expected(reads, k, oracle)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        for _ in range(2):
            e.count(ReadStream.from_strings(reads))
        keys, _, cnt = e.export_ge(0)
        assert [int_of_row(r) for r in keys] == want_keys
        assert np.array_equal(cnt, want_cnt * 2)


@pytest.mark.parametrize("k", (95, 201))
def test_growth_from_one_slot(k, oracle):
    rng = np.random.default_rng(3)
    reads = ["".join(rng.choice(list("ACGT"), 600)) for _ in range(60)]
    want_keys, want_cnt = expected(reads, k, oracle)
    with KmerEngine(k, capacity_hint=1) as e:
        cap0 = e.stats()[0]
        e.count(ReadStream.from_strings(reads))
        cap1 = e.stats()[0]
        assert cap1 >= cap0 * 8                              # several grows
        keys, _, cnt = e.export_ge(0)
        assert [int_of_row(r) for r in keys] == want_keys and np.array_equal(cnt, want_cnt)
        e.reserve(len(want_keys) * 8)
        keys2, _, cnt2 = e.export_ge(0)
        assert np.array_equal(keys2, keys) and np.array_equal(cnt2, cnt)


def test_accumulation_and_double_buffered_upload(oracle):
    k = 129
    rng = np.random.default_rng(11)
    batches = [mixed_reads(rng, k, 40) for _ in range(4)]
    allr = [r for b in batches for r in b]
    want_keys, want_cnt = expected(allr, k, oracle)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        for b in batches:
            e.count(ReadStream.from_strings(b))
        keys, _, cnt = e.export_ge(0)
        assert [int_of_row(r) for r in keys] == want_keys and np.array_equal(cnt, want_cnt)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        streams = [ReadStream.from_strings(b) for b in batches]
        e.upload_async(0, streams[0])
        for i in range(len(streams)):
            if i + 1 < len(streams):
                e.upload_async((i + 1) % 2, streams[i + 1])
            e.count_uploaded(i % 2)
        keys, _, cnt = e.export_ge(0)
        assert [int_of_row(r) for r in keys] == want_keys and np.array_equal(cnt, want_cnt)


def test_key_parts_union_is_whole(oracle):
    k = 161
    rng = np.random.default_rng(5)
    reads = mixed_reads(rng, k, 80)
    want_keys, want_cnt = expected(reads, k, oracle)
    got = {}
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        e.set_option("key_parts", 4)
        for p in range(4):
            e.clear()
            e.set_option("key_part", p)
            e.count(ReadStream.from_strings(reads))
            keys, _, cnt = e.export_ge(0)
            for r, c in zip(keys, cnt):
                v = int_of_row(r)
                assert v not in got                          # the slices are disjoint
                got[v] = int(c)
    assert sorted(got) == want_keys
    assert np.array_equal(np.array([got[v] for v in want_keys], np.uint32), want_cnt)


def test_count_if_reset_counts_second_parent(oracle):
    k = 97
    rng = np.random.default_rng(9)
    child = mixed_reads(rng, k, 60)
    mother, father = mixed_reads(rng, k, 60), mixed_reads(rng, k, 60)
    cand = sorted(oracle.py_count(child, k))
    filt_rows = rows_of(cand, k, oracle)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        e.load_filter(filt_rows)
        for parent in (mother, father):
            e.reset_counts()
            e.count_filtered(ReadStream.from_strings(parent))
            want = oracle.py_count(parent, k, set(cand))
            got = e.query(filt_rows)
            assert np.array_equal(got, np.array([want[c] for c in cand], np.uint32))
        with pytest.raises(KdfError):
            e.count(ReadStream.from_strings(child))           # a filter is loaded: insert mode refused


@pytest.mark.parametrize("k", (65, 129, 201))
def test_query_input_order_and_near_keys(k, oracle):
    rng = np.random.default_rng(k + 1)
    reads = mixed_reads(rng, k, 40)
    d = oracle.py_count(reads, k)
    kmers = list(d)
    rows = rows_of(kmers, k, oracle)
    W = rows.shape[1]
    tb = 2 * k - 64 * (W - 1)
    near_top = rows.copy()
    near_top[:, W - 1] ^= np.uint64(1 << (tb - 1))                # differs only in the top word
    near_w0 = rows.copy()
    near_w0[:, 0] ^= np.uint64(1)                                 # differs only in word 0
    absent = rng.integers(0, 1 << 62, size=(50, W), dtype=np.uint64)
    absent[:, W - 1] &= np.uint64((1 << tb) - 1)
    q_in = np.concatenate([rows, near_top, near_w0, absent])
    perm = rng.permutation(len(q_in))
    q_in = np.ascontiguousarray(q_in[perm])
    truth = {int_of_row(r): c for r, c in zip(rows, d.values())}
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        e.count(ReadStream.from_strings(reads))
        got = e.query(q_in)
    want = np.array([truth.get(int_of_row(r), 0) for r in q_in], np.uint32)
    assert np.array_equal(got, want)


def test_add_pairs_counts_and_saturation(oracle):
    k = 191
    W = key_words(k)
    rng = np.random.default_rng(2)
    keys = rows_of(["".join(rng.choice(list("ACGT"), k)) for _ in range(500)], k, oracle)
    keys = np.unique(keys, axis=0)
    cnt = rng.integers(1, 1000, len(keys)).astype(np.uint32)
    cnt[0] = 0xFFFFFFF0
    with KmerEngine(k, capacity_hint=1) as e:
        e.add_pairs(keys, None, cnt)
        e.add_pairs(keys[:10], None, np.full(10, 100, np.uint32))
        e.add_pairs(keys[10:20])                                   # plain insertion: + 0
        got = e.query(keys)
        want = cnt.astype(np.uint64)
        want[:10] += 100
        want = np.minimum(want, 0xFFFFFFFF).astype(np.uint32)
        assert got[0] == 0xFFFFFFFF                                # saturated
        assert np.array_equal(got, want)
        assert e.stats()[1] == len(keys)
        out, _, oc = e.export_ge(0)
        order = sorted(range(len(keys)), key=lambda i: int_of_row(keys[i]))
        assert np.array_equal(out, keys[order]) and np.array_equal(oc, want[order])
        assert out.shape[1] == W


def test_export_dev_sorted_and_unsorted(oracle):
    import torch
    k = 159
    rng = np.random.default_rng(4)
    reads = mixed_reads(rng, k, 60)
    want_keys, want_cnt = expected(reads, k, oracle)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        W = e.key_words
        e.count(ReadStream.from_strings(reads))
        n = e.count_ge(2)
        assert n == int((want_cnt >= 2).sum())
        dk = torch.zeros((n, W), dtype=torch.int64, device="cuda")
        dc = torch.zeros(n, dtype=torch.int32, device="cuda")
        assert e.export_ge_dev(2, dk.data_ptr(), None, dc.data_ptr(), n, sorted_=True) == n
        keys = dk.cpu().numpy().view(np.uint64)
        assert [int_of_row(r) for r in keys] == [v for v, c in zip(want_keys, want_cnt) if c >= 2]
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), want_cnt[want_cnt >= 2])
        dk.zero_(); dc.zero_()
        assert e.export_ge_dev(2, dk.data_ptr(), None, dc.data_ptr(), n, sorted_=False) == n
        keys = dk.cpu().numpy().view(np.uint64)
        cnt = dc.cpu().numpy().view(np.uint32)
        got = sorted(zip([int_of_row(r) for r in keys], cnt.tolist()))
        assert got == [(v, int(c)) for v, c in zip(want_keys, want_cnt) if c >= 2]
        with pytest.raises(KdfError):                             # too small: refused, nothing written past cap
            e.export_ge_dev(2, dk.data_ptr(), None, dc.data_ptr(), n - 1)


@pytest.mark.parametrize("k", KS)
def test_scan_hits_and_distinct(k, oracle):
    from kmer_denovo_filter_amd import hit_positions
    rng = np.random.default_rng(k * 3)
    index_reads = mixed_reads(rng, k, 30)
    probe = mixed_reads(rng, k, 30) + index_reads[:10]
    idx = oracle.py_count(index_reads, k)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        e.count(ReadStream.from_strings(index_reads))
        st = ReadStream.from_strings(probe)
        hits, distinct = e.scan(st)
    for r, s in enumerate(probe):
        b, end = int(st.offsets[r]), int(st.offsets[r + 1])
        got = set(hit_positions(hits, b, end).tolist())
        S = s.upper()
        want, seen = set(), set()
        for i in range(len(S) - k + 1):
            w = S[i:i + k]
            if all(ch in "ACGT" for ch in w) and oracle.canonicalize(w) in idx:
                want.add(i)
                seen.add(oracle.canonicalize(w))
        assert got == want, r
        assert distinct[r] == len(seen), r


@pytest.mark.parametrize("k", (127, 191))          # (top words of 62 bits: room for 40 000 keys that differ only there)
def test_hash_spread_shared_words(k, oracle):
    """Keys sharing word 0, or sharing every word but the top one, must not pile into one bucket: ~0.67 load
    (where the direct count grows the table) through the stream, and 40 000 keys through add_pairs."""
    W = key_words(k)
    rng = np.random.default_rng(k)
    # (a) through the stream: reads of exactly k bases, forward canonical (first base A, last base A), the last 32
    # bases shared -> word 0 shared by every key
    suffix = "".join(rng.choice(list("ACGT"), 31)) + "A"
    cap = 1 << 14
    n = int(cap * 0.66)
    reads = list({"A" + "".join(rng.choice(list("ACGT"), k - 33)) + suffix for _ in range(n)})
    with KmerEngine(k, capacity_hint=cap // 2) as e:
        assert e.stats()[0] == cap
        e.count(ReadStream.from_strings(reads))
        c, d, _ = e.stats()
        assert d == len(reads) and c == cap                        # no TABLE_FULL, and no grow
        rows = rows_of(reads, k, oracle)
        assert len(set(rows[:, 0].tolist())) == 1
        assert (e.query(rows) == 1).all()
    # (b) add_pairs: all but the top word shared, then word 0 shared
    base = rng.integers(0, 1 << 62, W, dtype=np.uint64)
    tb = 2 * k - 64 * (W - 1)
    m = 40_000
    a = np.tile(base, (m, 1))
    a[:, W - 1] = np.unique(rng.integers(0, 1 << min(tb, 40), 2 * m, dtype=np.uint64))[:m]
    b = np.tile(base, (m, 1))
    b[:, 0] = np.unique(rng.integers(0, 1 << 40, 2 * m, dtype=np.uint64))[:m]
    b[:, W - 1] = base[W - 1] ^ np.uint64(1)
    with KmerEngine(k, capacity_hint=1) as e:
        e.add_pairs(a, None, np.ones(m, np.uint32))
        e.add_pairs(b, None, np.full(m, 2, np.uint32))
        assert e.stats()[1] == 2 * m
        assert (e.query(a) == 1).all() and (e.query(b) == 2).all()


def test_wrong_form_calls_raise():
    import torch
    with KmerEngine(101, capacity_hint=1 << 10) as e:
        lo = np.zeros(4, np.uint64)
        for call in (lambda: e._ck(e._lib.kdf_query(e._h, lo.ctypes.data, lo.ctypes.data, 4, np.zeros(4, np.uint32).ctypes.data)),
                     lambda: e._ck(e._lib.kdf_add_pairs(e._h, lo.ctypes.data, lo.ctypes.data, None, 4)),
                     lambda: e._ck(e._lib.kdf_load_filter(e._h, lo.ctypes.data, lo.ctypes.data, 4))):
            with pytest.raises(KdfError, match="_w"):
                call()
        with pytest.raises(ValueError):
            e.query(lo)                                            # 1-D keys on a long engine
        bad = np.zeros((3, 4), np.uint64)
        bad[1, 3] = np.uint64(0x7FFFFFFFFFFFFFFF)                  # no key of any long k (would read as EMPTY when claimed)
        with pytest.raises(KdfError, match="top word"):
            e.add_pairs(bad)
        assert e.stats()[1] == 1 and e.query(bad[:1])[0] == 0       # the good keys went in, the table is usable
        e.add_pairs(bad[:1], None, np.array([5], np.uint32))
        assert e.query(bad[:1])[0] == 5
        for opt in (2, 4):
            with pytest.raises(KdfError, match="force_path"):
                e.set_option("force_path", opt)
        with pytest.raises(KdfError):
            e.set_option("hash_shift", 1)
        with pytest.raises(KdfError):
            e.set_option("fused_dump", 1)
        d = torch.zeros(1024, dtype=torch.int64, device="cuda")
        with pytest.raises(KdfError):
            e.export_parts_dev(0, 2, d.data_ptr(), d.data_ptr(), d.data_ptr(), 8)
        with pytest.raises(KdfError):
            e.set_counts_dev(d.data_ptr(), None, d.data_ptr(), 1)
        with pytest.raises(KdfError):
            e.add_pairs_multi_dev([(d.data_ptr(), None, d.data_ptr(), 1)])
    with KmerEngine(31, capacity_hint=1 << 10) as e:
        rows = np.zeros((4, 3), np.uint64)
        out = np.zeros(4, np.uint32)
        for call in (lambda: e._ck(e._lib.kdf_query_w(e._h, rows.ctypes.data, 4, out.ctypes.data)),
                     lambda: e._ck(e._lib.kdf_add_pairs_w(e._h, rows.ctypes.data, None, 4)),
                     lambda: e._ck(e._lib.kdf_load_filter_w(e._h, rows.ctypes.data, 4))):
            with pytest.raises(KdfError, match="odd k"):
                call()
