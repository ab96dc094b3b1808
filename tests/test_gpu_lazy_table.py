"""The dump-only flush (option ``lazy_table``): ``clear -> count -> export_ge_dev(L)`` writes the dump out of
kernel C and leaves the table unwritten; the passes stay in the ring and whatever needs the table later applies them.

Small shapes: forced binned (``force_path`` 2), 2^18 slots (64 / 128 buckets), 3 000 synthetic 150 bp reads with N bases and
flipped strands over a 20 kb genome (22x: plenty of counts >= 3).  Truth: ``tests/stream_truth.py`` (torch ops on the packed
words, nothing shared with the engine), computed once per (k, stream) and left unchanged; the scan is compared with the
direct path (``force_path`` 1) on a second engine.

Saturation (g): one flush adds fewer than 2^32 to a slot (kernel C's wrap test compares with the count the slot had in HBM:
DESIGN.md 3.2), so the k-mer is repeated past 2^32 - 1 over five flushes of 2^30 positions each; a homopolymer stream sets
the skew flag, so this is one more sequence that must not take the path."""
import functools
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

import stream_truth as ST

pytestmark = pytest.mark.gpu

HINT = 1 << 17
KS = [31, 32, 63]
SENT = -7
WITNESSES = ("flushes", "fused_dumps", "pending_passes", "pending_positions", "binned_passes", "heavy_buckets", "replayed_buckets",
             "log2cap", "bucket_bits", "last_count_path")


@functools.lru_cache(maxsize=None)
def _stream(which, n_reads=3000):
    from kmer_denovo_filter_amd.synth import synth_stream
    seed = {"a": 11, "b": 23, "other": 37, "small": 41}[which]
    return synth_stream(200 if which == "small" else n_reads, 150, genome_len=20_000, seed=seed, device="cuda:0", sub_rate=0.001, n_rate=0.002,
                        genome_seed=5 if which != "other" else 6)


@functools.lru_cache(maxsize=None)
def _truth(k, names):
    """sorted (lo, hi, cnt) uint64 / uint64 / uint64 arrays and the valid windows of the named streams together"""
    parts = [ST.count_truth(_stream(n), k) for n in names]
    lo, hi, cnt = ST.accumulate(parts) if len(parts) > 1 else parts[0][:3]
    out = (lo.cpu().numpy().view(np.uint64), hi.cpu().numpy().view(np.uint64), cnt.cpu().numpy().astype(np.uint64), sum(p[3] for p in parts))
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _engine(k, lazy=1, hint=HINT):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=hint)
    e.set_option("force_path", 2); e.set_option("lazy_table", lazy)
    return e


def _count(e, which):
    ds = _stream(which)
    e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)


def _raw_dump_dev(e, min_count, cap):
    """kdf_export_ge_dev into sentinel-filled buffers with 64 words of guard -> (rc, n, lo, hi, cnt), the buffers still on the device"""
    import torch
    lo = torch.full((cap + 64,), SENT, dtype=torch.int64, device="cuda:0")
    hi = torch.full((cap + 64,), SENT, dtype=torch.int64, device="cuda:0") if e.wide else None
    cnt = torch.full((cap + 64,), SENT, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    n = c_uint64(0)
    rc = e._lib.kdf_export_ge_dev(e._h, int(min_count), c_void_p(lo.data_ptr()), c_void_p(hi.data_ptr()) if e.wide else None,
                                  c_void_p(cnt.data_ptr()), int(cap), 0, byref(n))
    torch.cuda.synchronize()
    return rc, int(n.value), lo, hi, cnt


def _raw_dump(e, min_count, cap):
    """... -> (rc, n, lo, hi, cnt) on the host"""
    rc, n, lo, hi, cnt = _raw_dump_dev(e, min_count, cap)
    return rc, n, lo.cpu().numpy(), hi.cpu().numpy() if e.wide else None, cnt.cpu().numpy()


def _sorted(lo, hi, cnt):
    o = np.lexsort((lo, hi))
    return lo[o], hi[o], cnt[o]


def _dump(e, min_count, cap=1 << 17):
    rc, n, lo, hi, cnt = _raw_dump(e, min_count, cap)
    assert rc == 0 and n <= cap
    assert (lo[n:] == SENT).all() and (cnt[n:] == SENT).all() and (hi is None or (hi[n:] == SENT).all())
    return _sorted(lo[:n].view(np.uint64), hi[:n].view(np.uint64) if hi is not None else np.zeros(n, np.uint64), cnt[:n].view(np.uint32).astype(np.uint64))


def _same(got, truth, min_count=0):
    keep = truth[2] >= min_count
    assert len(got[0]) == int(keep.sum())
    for g, w in zip(got, truth[:3]):
        np.testing.assert_array_equal(g, w[keep])


def _lazy_stats(e):
    return e.get_stat("dump_only_flushes"), e.get_stat("materialisations")


def _query_all(e, k, truth, absent_from="other"):
    """every key of the truth and the keys of another stream that are not in it"""
    other = _truth(k, (absent_from,))
    have = set(zip(truth[0].tolist(), truth[1].tolist()))
    absent = np.array([i for i, p in enumerate(zip(other[0].tolist(), other[1].tolist())) if p not in have][:5000])
    assert len(absent) > 1000
    lo = np.concatenate([truth[0], other[0][absent]]); hi = np.concatenate([truth[1], other[1][absent]])
    got = e.query(lo, hi if k > 32 else None).astype(np.uint64)
    np.testing.assert_array_equal(got[:len(truth[0])], truth[2])
    assert not got[len(truth[0]):].any()


# ---- (a) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("L", [1, 3])
def test_a_clear_count_dump_is_dump_only(k, L):
    truth = _truth(k, ("a",))
    assert int((truth[2] >= 3).sum()) > 1000
    with _engine(k) as e:
        assert e.get_stat("lazy_table") == 1
        e.clear(); _count(e, "a")
        assert e.get_stat("pending_passes") == 1 and e.get_stat("retained_passes") == 0
        _same(_dump(e, L), truth, L)
        assert _lazy_stats(e) == (1, 0)
        assert (e.get_stat("fused_dumps"), e.get_stat("flushes"), e.get_stat("pending_passes"), e.get_stat("pending_positions")) == (1, 1, 0, 0)
        assert e.get_stat("retained_passes") == 1 and e.get_stat("log2cap") > e.get_stat("bucket_bits")


# ---- (b) --------------------------------------------------------------------------------------------------------------------
READERS = ["stats", "query", "count_ge", "histogram", "scan", "export_ge_dev", "export"]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("reader", READERS)
def test_b_every_reader_after_a_dump_only_flush(k, reader):
    from kmer_denovo_filter_amd import ReadStream
    from kmer_denovo_filter_amd.synth import stream_to_ascii
    truth = _truth(k, ("a",))
    with _engine(k) as e:
        e.clear(); _count(e, "a")
        _same(_dump(e, 3), truth, 3)
        assert _lazy_stats(e) == (1, 0)
        cap, distinct, windows = e.stats()                     # the counters of the dump-only flush: no table needed
        assert (distinct, windows) == (len(truth[0]), truth[3]) and cap == 1 << e.get_stat("log2cap")
        assert _lazy_stats(e) == (1, 0) and e.get_stat("retained_passes") == 1
        if reader == "stats":
            return
        if reader == "query":
            _query_all(e, k, truth)
        elif reader == "count_ge":
            assert e.count_ge(2) == int((truth[2] >= 2).sum())
        elif reader == "histogram":
            high = 40
            want = np.bincount(np.minimum(truth[2], high + 1).astype(np.int64), minlength=high + 2).astype(np.uint64)
            np.testing.assert_array_equal(e.histogram(high), want)
        elif reader == "scan":
            chars, offs = stream_to_ascii(_stream("a"), 400)
            reads = [chars[offs[i]:offs[i + 1]].tobytes().decode() for i in range(400)]
            st = ReadStream.from_strings(reads)
            with _engine(k, 0) as d:
                d.set_option("force_path", 1); _count(d, "a")
                want_hits, want_distinct = d.scan(st)
            hits, dist = e.scan(st)
            np.testing.assert_array_equal(hits, want_hits); np.testing.assert_array_equal(dist, want_distinct)
            assert int(dist.sum()) > 0
        elif reader == "export_ge_dev":
            _same(_dump(e, 1), truth, 1)
            assert e.get_stat("fused_dumps") == 1              # (nothing new was pending: the table pass, as without lazy_table)
        elif reader == "export":
            lo, hi, cnt = e.export_ge(2)
            _same((lo, hi, cnt.astype(np.uint64)), truth, 2)
        assert _lazy_stats(e) == (1, 1) and e.get_stat("retained_passes") == 0 and e.get_stat("flushes") == 1
        _same(_dump(e, 1), truth, 1)                           # the table is whole now
        assert e.stats()[1:] == (len(truth[0]), truth[3])
        assert _lazy_stats(e) == (1, 1)


# ---- (c) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_c_a_second_batch_after_the_dump(k):
    ta, tab = _truth(k, ("a",)), _truth(k, ("a", "b"))
    with _engine(k) as e:
        e.clear(); _count(e, "a")
        _same(_dump(e, 3), ta, 3)
        _count(e, "b")
        assert e.get_stat("pending_passes") == 1 and e.get_stat("retained_passes") == 1
        _same(_dump(e, 3), tab, 3)                             # dump-only again, over both passes
        assert _lazy_stats(e) == (2, 0) and (e.get_stat("fused_dumps"), e.get_stat("flushes")) == (2, 2)
        assert e.stats()[1:] == (len(tab[0]), tab[3])
        _query_all(e, k, tab)
        assert _lazy_stats(e) == (2, 1) and e.get_stat("flushes") == 2
        _same(_dump(e, 1), tab, 1)


# ---- (d) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_d_clear_drops_the_retained_passes(k):
    ta, to = _truth(k, ("a",)), _truth(k, ("other",))
    with _engine(k) as e:
        e.clear(); _count(e, "a")
        _same(_dump(e, 1), ta, 1)
        e.clear()
        assert e.get_stat("retained_passes") == 0 and e.stats()[1:] == (0, 0)
        _count(e, "other")
        _same(_dump(e, 1), to, 1)
        assert _lazy_stats(e) == (2, 0)
        _query_all(e, k, to, absent_from="a")                  # nothing of the dropped passes: the keys of "a" read 0
        assert _lazy_stats(e) == (2, 1)
        _same(_dump(e, 1), to, 1)
        assert e.stats()[1:] == (len(to[0]), to[3])


# ---- (e) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_e_a_buffer_that_is_too_small(k):
    truth = _truth(k, ("a",))
    full = int((truth[2] >= 2).sum())
    pairs = set(zip(truth[0].tolist(), truth[1].tolist(), truth[2].tolist()))
    for cap in (full - 1, 100):
        res = []
        for lazy in (1, 0):
            with _engine(k, lazy) as e:
                e.clear(); _count(e, "a")
                rc, n, lo, hi, cnt = _raw_dump(e, 2, cap)
                err = e._lib.kdf_last_error(e._h)
                assert (lo[cap:] == SENT).all() and (cnt[cap:] == SENT).all() and (hi is None or (hi[cap:] == SENT).all())
                got = set(zip(lo[:cap].view(np.uint64).tolist(), hi[:cap].view(np.uint64).tolist() if hi is not None else [0] * cap,
                              cnt[:cap].view(np.uint32).tolist()))
                assert len(got) == cap and got <= pairs
                assert e.get_stat("dump_only_flushes") == lazy
                res.append((rc, n, err, e.get_stat("fused_dumps"), e.get_stat("flushes"), e.get_stat("pending_passes")))
                _same(_dump(e, 2), truth, 2)                   # usable and correct afterwards
                _count(e, "b")
                _same(_dump(e, 1), _truth(k, ("a", "b")), 1)
        assert res[0] == res[1] and res[0][0] != 0 and res[0][1] == full, (cap, res)


# ---- (f) --------------------------------------------------------------------------------------------------------------------
def _f_live_table(e, k):
    e.clear(); _count(e, "a"); e.flush(); _count(e, "b")
    return _dump(e, 2), _truth(k, ("a", "b")), 2


def _f_filter_mode(e, k):
    t = _truth(k, ("a",))
    sel = np.arange(0, len(t[0]), 3)
    e.load_filter(t[0][sel], t[1][sel] if k > 32 else None)
    ds = _stream("a")
    e.count_filtered_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
    return _dump(e, 1), (t[0][sel], t[1][sel], t[2][sel]), 1


def _f_key_parts(e, k):
    """the two halves of the key space (ranges of the low hash bits, include/kdf.h), one after the other on one engine: each
    dump is a part of the truth, together they are the whole of it"""
    e.set_option("key_parts", 2)
    t = _truth(k, ("a",))
    parts = []
    for part in (0, 1):
        e.set_option("key_part", part)
        e.clear(); _count(e, "a")
        parts.append(_dump(e, 1))
        assert 0 < len(parts[-1][0]) < len(t[0])
    return _sorted(*(np.concatenate([p[i] for p in parts]) for i in range(3))), t, 1


def _f_prefilter(e, k):
    ds = _stream("a")
    e.prefilter_begin(2)
    e.prefilter_add_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
    e.prefilter_arm()
    e.clear(); _count(e, "a")
    got = _dump(e, 2)                                          # (the sieve lets every key with count >= 2 through, with its full count)
    e.prefilter_drop()
    return got, _truth(k, ("a",)), 2


def _f_skew(e, k):
    """a repeat-rich small genome: the homopolymer's coarse bin holds far more than its share, which sets the skew flag (VAR 2
    of kernel C; its bucket goes to the heavy-bucket kernels).  Truth: the direct path on a second engine."""
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    st = ReadStream.from_strings(["A" * 200] * 1200 + ["ACGT" * 50, "AACCGGTT" * 25] * 300)
    e.clear(); e.count(st)
    got = _dump(e, 2)
    assert e.get_stat("heavy_buckets") > 0
    with KmerEngine(k, capacity_hint=1 << 12) as d:
        d.set_option("force_path", 1); d.count(st)
        lo, hi, cnt = d.export_ge(0)
    return got, _sorted(lo, hi, cnt.astype(np.uint64)) + (0,), 2


def _f_grow(e, k):
    e.clear(); _count(e, "a")
    return _dump(e, 1), _truth(k, ("a",)), 1


F_CASES = {"live table": (_f_live_table, HINT), "filter mode": (_f_filter_mode, HINT), "key_parts": (_f_key_parts, HINT),
           "armed prefilter": (_f_prefilter, HINT), "skew": (_f_skew, 1 << 22), "table must grow": (_f_grow, 1 << 12)}


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", list(F_CASES))
def test_f_sequences_that_must_not_take_the_path(k, case):
    fn, hint = F_CASES[case]
    res = []
    for lazy in (1, 0):
        with _engine(k, lazy, hint) as e:
            got, want, L = fn(e, k)
            _same(got, want, L)
            assert _lazy_stats(e) == (0, 0), case
            # the case is the one it says (a changed default must not turn it into a vacuous pass)
            if case == "live table":
                assert e.get_stat("flushes") == 2
            elif case == "table must grow":
                assert e.get_stat("replayed_buckets") > 0 and e.get_stat("log2cap") > 13
            elif case == "filter mode":
                assert e.get_stat("fused_dumps") == 0 and e.get_stat("binned_passes") == 1
            elif case == "key_parts":
                assert e.get_stat("fused_dumps") == 2 and e.get_stat("flushes") == 2
            elif case == "armed prefilter":
                assert e.get_stat("fused_dumps") == 1 and e.get_stat("flushes") == 1
            res.append((got, {n: e.get_stat(n) for n in WITNESSES}))
    assert res[0][1] == res[1][1], (case, res[0][1], res[1][1])
    for a, b in zip(res[0][0], res[1][0]):
        np.testing.assert_array_equal(a, b)


# ---- (g) --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _poly_a(n_bases=1 << 30):
    """n_bases positions of A as one record: packed words 0, every position valid, the padding words invalid"""
    import torch
    tiles = (n_bases + 63) // 64
    packed = torch.zeros(tiles * 2 + 4, dtype=torch.int64, device="cuda:0")
    invalid = torch.zeros(tiles + 2, dtype=torch.int64, device="cuda:0")
    invalid[tiles:] = -1
    return packed, invalid, n_bases


@pytest.mark.parametrize("k", [31, 63])
def test_g_one_kmer_counted_past_the_ceiling(k):
    """A^k (key 0) five times 2^30 - k + 1 times: 4 294 967 296 - 4 (k - 1) after four flushes (exact, below the ceiling of
    2^32 - 1 that kdf.h documents), saturated by the fifth, whose dump is asked for with the pass pending.  The dump and the
    table read afterwards (query, count_ge, histogram, a second dump) agree, with lazy_table at 1 and at 0."""
    packed, invalid, n = _poly_a()
    per = n - k + 1
    assert 4 * per < 0xFFFFFFFF < 5 * per
    zero = np.zeros(1, np.uint64)
    res = []
    for lazy in (1, 0):
        with _engine(k, lazy, 1 << 22) as e:
            e.clear()
            for _ in range(4):
                e.count_dev(packed.data_ptr(), invalid.data_ptr(), n); e.flush()
            assert int(e.query(zero, zero if k > 32 else None)[0]) == 4 * per
            e.count_dev(packed.data_ptr(), invalid.data_ptr(), n)
            assert e.get_stat("pending_passes") == 1
            dump = _dump(e, 1, cap=64)
            assert [a.tolist() for a in dump] == [[0], [0], [0xFFFFFFFF]]
            assert int(e.query(zero, zero if k > 32 else None)[0]) == 0xFFFFFFFF
            assert e.count_ge(0xFFFFFFFF) == 1 and e.count_ge(1) == 1
            bins = e.histogram(10)
            assert int(bins[11]) == 1 and int(bins.sum()) == 1
            assert [a.tolist() for a in _dump(e, 3, cap=64)] == [[0], [0], [0xFFFFFFFF]]
            assert e.stats()[1:] == (1, 5 * per)
            assert _lazy_stats(e) == (0, 0) and e.get_stat("heavy_buckets") > 0
            res.append({w: e.get_stat(w) for w in WITNESSES})
    assert res[0] == res[1]


# ---- a small batch behind retained passes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 63])
def test_a_small_batch_after_the_dump_goes_the_way_it_would_without_lazy_table(k):
    """clear, count (binned), dump, then a small batch under the automatic path choice: without lazy_table the ring is empty
    and the table live, and the batch goes through the direct kernels; with it the retained passes are applied first and the
    batch goes the same way -- same table, same witnesses"""
    from kmer_denovo_filter_amd import KmerEngine
    tab = _truth(k, ("a", "small"))
    res = []
    for lazy in (1, 0):
        with KmerEngine(k, capacity_hint=HINT) as e:
            e.set_option("lazy_table", lazy); e.set_option("binned_min_positions", 1)
            e.clear(); _count(e, "a")                          # 453 000 positions x 116 bytes >= the table's 3.1 MB: binned
            assert e.get_stat("pending_positions") > 0 and e.get_stat("pending_passes") == 0      # waits in the pending stream
            _same(_dump(e, 3), _truth(k, ("a",)), 3)
            assert e.get_stat("last_count_path") == 1 and e.get_stat("dump_only_flushes") == lazy
            _count(e, "small")                                  # 30 200 positions x 70 bytes < 3.1 MB: direct into a live table
            assert e.get_stat("pending_positions") > 0 and e.get_stat("pending_passes") == 0
            _query_all(e, k, tab)
            assert e.get_stat("last_count_path") == 0 and e.get_stat("materialisations") == lazy
            res.append({w: e.get_stat(w) for w in WITNESSES})
            _same(_dump(e, 1), tab, 1)
    assert res[0] == res[1], res


# ---- a finished dump request is gone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("cap", [1 << 17, 100])
def test_h_a_finished_dump_request_is_gone(k, lazy, cap):
    """The buffers of a dump belong to that call alone: no later flush, count or dump of the engine writes them again, whether
    the dump fitted (2^17) or not (100: the call fails).  The first call's device buffers stay alive, so nothing else is
    allocated where they lie."""
    import torch
    ta = _truth(k, ("a",))
    full = int((ta[2] >= 2).sum())
    with _engine(k, lazy) as e:
        e.clear(); _count(e, "a")
        rc, n, lo, hi, cnt = _raw_dump_dev(e, 2, cap)
        first = [lo, cnt] + ([hi] if hi is not None else [])
        copies = [t.cpu().numpy().copy() for t in first]
        assert n == full and (rc == 0) == (cap >= full)
        assert e.get_stat("fused_dumps") == 1 and e.get_stat("dump_only_flushes") == lazy
        _count(e, "b"); e.flush()
        _count(e, "small"); e.stats()
        _same(_dump(e, 2), _truth(k, ("a", "b", "small")), 2)
        torch.cuda.synchronize()
        for t, c in zip(first, copies):
            assert t.cpu().numpy().tobytes() == c.tobytes()
