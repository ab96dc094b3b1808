"""The fused dump's tail (kernel C, every ``DUMP`` instantiation): the kept slots of a bucket are compacted in LDS
and written out densely, ``n = min(kept, dump_cap - base)`` entries per bucket.

Small shapes: forced binned (``force_path`` 2), ``capacity_hint`` 2^17, 3 000 synthetic 150 bp reads with N bases and flipped
strands over a 70 kb genome (6x) -- about 80 000 distinct k-mers, so a bucket holds more keys than its workgroup has threads
(768 narrow, 512 wide: asserted below) and the dense pass of an L = 1 dump takes more than one round.  Truth:
``tests/stream_truth.py``, computed once per (k, streams) and left unchanged.  Dumps go into sentinel-filled buffers with 64
words of guard behind ``cap`` and are compared exactly after sorting: keys, high words, counts.

The ``BIG`` instantiation (buckets of twice the slots) needs a table of 2^32 slots: it is compiled and inspected, not run here."""
import functools
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

import stream_truth as ST

pytestmark = pytest.mark.gpu

HINT = 1 << 17
KS = [31, 32, 33, 63]
SENT = -7
GUARD = 64


@functools.lru_cache(maxsize=None)
def _stream(which):
    from kmer_denovo_filter_amd.synth import synth_stream
    return synth_stream(3000, 150, genome_len=70_000, seed={"a": 11, "b": 23}[which], device="cuda:0", sub_rate=0.001, n_rate=0.002, genome_seed=5)


@functools.lru_cache(maxsize=None)
def _truth(k, names):
    """sorted (lo, hi, cnt) uint64 arrays of the named streams together"""
    parts = [ST.count_truth(_stream(n), k) for n in names]
    lo, hi, cnt = ST.accumulate(parts) if len(parts) > 1 else parts[0][:3]
    out = (lo.cpu().numpy().view(np.uint64), hi.cpu().numpy().view(np.uint64), cnt.cpu().numpy().astype(np.uint64))
    for a in out:
        a.setflags(write=False)
    return out


def _engine(k, lazy=1, fused=1, flags=0):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=HINT)
    e.set_option("force_path", 2); e.set_option("lazy_table", lazy); e.set_option("fused_dump", fused)
    if flags:
        e.set_option("debug_flags", flags)
    return e


def _count(e, which):
    ds = _stream(which)
    e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)


def _raw_dump(e, min_count, cap, with_hi=True, with_cnt=True):
    """kdf_export_ge_dev into sentinel-filled buffers -> (rc, n, lo, hi, cnt) on the host, guard words included; an array that
    was not passed (NULL pointer) comes back as None"""
    import torch
    lo = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda:0")
    hi = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda:0") if e.wide and with_hi else None
    cnt = torch.full((cap + GUARD,), SENT, dtype=torch.int32, device="cuda:0") if with_cnt else None
    torch.cuda.synchronize()
    n = c_uint64(0)
    rc = e._lib.kdf_export_ge_dev(e._h, int(min_count), c_void_p(lo.data_ptr()), c_void_p(hi.data_ptr()) if hi is not None else None,
                                  c_void_p(cnt.data_ptr()) if cnt is not None else None, int(cap), 0, byref(n))
    torch.cuda.synchronize()
    return rc, int(n.value), lo.cpu().numpy(), None if hi is None else hi.cpu().numpy(), None if cnt is None else cnt.cpu().numpy()


def _untouched_from(at, *arrays):
    for a in arrays:
        assert a is None or (a[at:] == SENT).all()


def _sorted(lo, hi, cnt):
    o = np.lexsort((lo, hi))
    return lo[o], hi[o], cnt[o]


def _dump(e, min_count, cap=1 << 17):
    rc, n, lo, hi, cnt = _raw_dump(e, min_count, cap)
    assert rc == 0 and n <= cap
    _untouched_from(n, lo, hi, cnt)
    return _sorted(lo[:n].view(np.uint64), hi[:n].view(np.uint64) if hi is not None else np.zeros(n, np.uint64), cnt[:n].view(np.uint32).astype(np.uint64))


def _same(got, truth, min_count=0):
    keep = truth[2] >= min_count
    assert len(got[0]) == int(keep.sum())
    for g, w in zip(got, truth):
        np.testing.assert_array_equal(g, w[keep])


def _more_keys_than_threads(e, truth):
    """the average bucket keeps more entries at L = 1 than its workgroup has threads: the dense pass runs more than once"""
    buckets = 1 << (e.get_stat("log2cap") - e.get_stat("bucket_bits"))
    assert len(truth[0]) > (512 if e.wide else 768) * buckets, (len(truth[0]), buckets)


# ---- (a) multi-round dense pass; nothing kept ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("L", [1, 3, 1000])
def test_a_dense_pass(k, L):
    truth = _truth(k, ("a",))
    assert int((truth[2] >= 3).sum()) > 1000 and int(truth[2].max()) < 1000
    with _engine(k) as e:
        e.clear(); _count(e, "a")
        got = _dump(e, L)                                        # (L = 1000: n = 0, the buffers stay as they were)
        _same(got, truth, L)
        assert (e.get_stat("dump_only_flushes"), e.get_stat("fused_dumps"), e.get_stat("replayed_buckets")) == (1, 1, 0)
        _more_keys_than_threads(e, truth)


# ---- (b) small buffers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_b_small_buffers(k):
    truth = _truth(k, ("a",))
    full = len(truth[0])
    pairs = set(zip(truth[0].tolist(), truth[1].tolist(), truth[2].tolist()))
    for cap in (0, 1, 63, 64, 65, full - 1, full):
        with _engine(k) as e:
            e.clear(); _count(e, "a")
            rc, n, lo, hi, cnt = _raw_dump(e, 1, cap)
            assert n == full and (rc == 0) == (cap >= full), (cap, rc, n)
            assert (e.get_stat("dump_only_flushes"), e.get_stat("fused_dumps")) == (1, 1)
            _untouched_from(cap, lo, hi, cnt)                      # nothing at or past cap
            got = list(zip(lo[:cap].view(np.uint64).tolist(), hi[:cap].view(np.uint64).tolist() if hi is not None else [0] * cap,
                           cnt[:cap].view(np.uint32).tolist()))
            assert len(set(k_[:2] for k_ in got)) == cap and set(got) <= pairs, cap      # true pairs, no key twice
            if cap < full:
                _same(_dump(e, 1), truth, 1)                       # usable and correct afterwards


# ---- (c) every tail variant ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("L", [1, 2])
def test_c_every_tail_variant(k, L):
    ta, tab = _truth(k, ("a",)), _truth(k, ("a", "b"))
    res, res2 = {}, {}
    for name, lazy, fused in (("dump-only", 1, 1), ("fused", 0, 1), ("table pass", 0, 0)):
        with _engine(k, lazy, fused) as e:
            e.clear(); _count(e, "a")
            res[name] = _dump(e, L)
            assert (e.get_stat("dump_only_flushes"), e.get_stat("fused_dumps")) == {"dump-only": (1, 1), "fused": (0, 1), "table pass": (0, 0)}[name]
            # a second batch into the LIVE table (materialised first): the tail with the write-back and the saturation compare
            e.flush(); _count(e, "b")
            res2[name] = _dump(e, L)
            assert e.get_stat("dump_only_flushes") == (1 if name == "dump-only" else 0) and e.get_stat("fused_dumps") == (0 if name == "table pass" else 2)
            assert e.get_stat("flushes") == 2 and e.get_stat("replayed_buckets") == 0
            _same(_dump(e, 1), tab, 1)                             # the table the write-back left
    for name in res:
        _same(res[name], ta, L); _same(res2[name], tab, L)


# ---- (d) null output pointers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("lazy", [1, 0])
def test_d_no_counts_array(k, lazy):
    truth = _truth(k, ("a",))
    keep = truth[2] >= 2
    with _engine(k, lazy) as e:
        e.clear(); _count(e, "a")
        rc, n, lo, hi, cnt = _raw_dump(e, 2, 1 << 17, with_cnt=False)
        assert rc == 0 and n == int(keep.sum()) and cnt is None
        assert (e.get_stat("dump_only_flushes"), e.get_stat("fused_dumps")) == (lazy, 1)
        _untouched_from(n, lo, hi)
        glo, ghi, _ = _sorted(lo[:n].view(np.uint64), hi[:n].view(np.uint64) if hi is not None else np.zeros(n, np.uint64), np.zeros(n, np.uint64))
        np.testing.assert_array_equal(glo, truth[0][keep]); np.testing.assert_array_equal(ghi, truth[1][keep])


@pytest.mark.parametrize("k", [33, 63])
def test_d_no_high_words_array(k):
    """wide keys without the high-word array: kdf_export_ge_dev allows it for cap = 0 only (a count of the entries)"""
    truth = _truth(k, ("a",))
    with _engine(k) as e:
        e.clear(); _count(e, "a")
        rc, n, lo, hi, cnt = _raw_dump(e, 1, 0, with_hi=False)
        assert rc != 0 and n == len(truth[0])
        _untouched_from(0, lo, cnt)
        rc, n, lo, hi, cnt = _raw_dump(e, 1, 1 << 17, with_hi=False)     # refused, nothing written
        assert rc != 0
        _untouched_from(0, lo, cnt)
        _same(_dump(e, 1), truth, 1)


# ---- (e) the skew instantiation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("L", [1, 3])
def test_e_skew_instantiation(k, L):
    truth = _truth(k, ("a",))
    with _engine(k, flags=4096) as e:                              # (debug flag 4096: VAR 2 of kernel C whatever the input)
        e.clear(); _count(e, "a")
        _same(_dump(e, L), truth, L)
        assert (e.get_stat("dump_only_flushes"), e.get_stat("fused_dumps"), e.get_stat("heavy_buckets")) == (0, 1, 0)
        _more_keys_than_threads(e, truth)
