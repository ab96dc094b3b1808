"""`dump -L n` written by the flush that applies the pending passes (kb_bucket_kernel<.., DUMP>) is the DEFAULT dump path of
a binned count: every case below compares the fused dump, sorted by key, with the table dump (``fused_dump`` 0) and with
the oracle's counts, on the smallest tables the binned path accepts (a few buckets, so several workgroups)."""
import os
import subprocess
import sys
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7                     # fills every output buffer before a dump
HINT = 1 << 16


def _reads(k, n=1500, seed=0):
    from test_gpu_parity_basic import rand_reads
    rng = np.random.default_rng(5200 + k + seed)
    genome = rng.integers(0, 4, 12000).astype(np.uint8)
    return rand_reads(rng, n, k, 260, genome=genome) + ["ACGT" * 70, "N" * 80, ""]


def _by_key(lo, hi, cnt):
    o = np.lexsort((lo, hi))
    return lo[o], hi[o], cnt[o]


_WANT = {}


def _want(oracle, k, reads_key, reads):
    """the oracle's (lo, hi, cnt), sorted by key; computed once per input"""
    if (k, reads_key) not in _WANT:
        lo, hi, cnt = oracle.OracleTable(k, 1 << 12).count_reads(reads).export_ge(0)
        r = _by_key(lo, hi, cnt)
        for a in r:
            a.setflags(write=False)
        _WANT[(k, reads_key)] = r
    return _WANT[(k, reads_key)]


def _engine(k, fused=None, big=False, skew=False):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=HINT)
    e.set_option("force_path", 2)
    if fused is not None:
        e.set_option("fused_dump", fused)
    if big:
        e.set_option("big_bucket_log2cap", 10)               # every binned table: the BIG instantiation
    if skew:
        e.set_option("debug_flags", 4096)                    # the skew instantiation (VAR 2)
    return e


def _raw_dump(e, min_count, cap, with_cnt=True):
    """kdf_export_ge_dev, unsorted, into sentinel-filled buffers of cap + 64 entries -> (rc, n, lo, hi, cnt) with the WHOLE buffers"""
    import torch
    room = cap + 64
    lo = torch.full((room,), SENT, dtype=torch.int64, device="cuda:0")
    hi = torch.full((room,), SENT, dtype=torch.int64, device="cuda:0") if e.wide else None
    cnt = torch.full((room,), SENT, dtype=torch.int32, device="cuda:0") if with_cnt else None
    torch.cuda.synchronize()
    n = c_uint64(0)
    rc = e._lib.kdf_export_ge_dev(e._h, int(min_count), c_void_p(lo.data_ptr()), c_void_p(hi.data_ptr()) if e.wide else None,
                                  c_void_p(cnt.data_ptr()) if with_cnt else None, int(cap), 0, byref(n))
    torch.cuda.synchronize()
    return (rc, int(n.value), lo.cpu().numpy(), hi.cpu().numpy() if e.wide else None, cnt.cpu().numpy() if with_cnt else None)


def _dump(e, min_count, cap=1 << 17):
    """a dump that fits, sorted by key; nothing may be written past the n entries"""
    rc, n, lo, hi, cnt = _raw_dump(e, min_count, cap)
    assert rc == 0 and n <= cap
    assert (lo[n:] == SENT).all() and (cnt[n:] == SENT).all() and (hi is None or (hi[n:] == SENT).all())
    return _by_key(lo[:n].view(np.uint64), hi[:n].view(np.uint64) if hi is not None else np.zeros(n, np.uint64), cnt[:n].view(np.uint32))


def _same(got, want, min_count=0):
    keep = want[2] >= min_count
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w[keep])


def _default_run(k, out):
    """a fresh engine, `fused_dump` untouched, forced binned: count_dev, then export_ge_dev"""
    import torch
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    st = ReadStream.from_strings(_reads(k))
    dp = torch.from_numpy(np.ascontiguousarray(st.packed).view(np.int64)).to("cuda:0")
    di = torch.from_numpy(np.ascontiguousarray(st.invalid).view(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    with KmerEngine(k, capacity_hint=HINT) as e:
        e.set_option("force_path", 2)
        e.count_dev(dp.data_ptr(), di.data_ptr(), st.n_bases)
        assert e.get_stat("pending_passes") == 1
        lo, hi, cnt = _dump(e, 2)
        fused = e.get_stat("fused_dumps")
        assert e.get_stat("log2cap") > e.get_stat("bucket_bits") and e.get_stat("pending_passes") == 0
    if out:
        np.savez(out, lo=lo, hi=hi, cnt=cnt, fused=np.int64(fused))
    return fused, (lo, hi, cnt)


@pytest.mark.parametrize("k", [31, 63])
def test_the_default_dump_of_a_binned_count_is_the_fused_one(oracle, k, tmp_path):
    fused, got = _default_run(k, None)
    assert fused == 1
    _same(got, _want(oracle, k, "a", _reads(k)), 2)
    # KDF_FUSED_DUMP=0 in a fresh process: the table dump, the same pairs
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, KDF_FUSED_DUMP="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(k), out], env=env, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    assert int(z["fused"]) == 0
    for g, name in zip(got, ("lo", "hi", "cnt")):
        np.testing.assert_array_equal(g, z[name])


# narrow: B / 2 = 2048 slot pairs over 768 threads (a partial last step); wide: 1024 over 512 (none); BIG: 4096 / 2048 over 1024
@pytest.mark.parametrize("k,big,skew", [(31, False, False), (63, False, False), (31, True, False), (63, True, False),
                                        (31, False, True), (63, False, True)])
def test_thresholds_and_every_instantiation(oracle, k, big, skew):
    reads = _reads(k) + (["ACGT" * 70, "AACCGGTT" * 40] * 150 if skew else [])      # (repeat-rich, far below the heavy-bucket threshold)
    want = _want(oracle, k, "a+rep" if skew else "a", reads)
    top = int(want[2].max())
    assert top >= 3
    from kmer_denovo_filter_amd import ReadStream
    st = ReadStream.from_strings(reads)
    for min_count in (1, 2, 3, top + 1):
        res = []
        for fused in (1, 0):
            with _engine(k, fused, big, skew) as e:
                e.count(st)
                bb = e.get_stat("bucket_bits")
                assert bb == (12 if k <= 32 else 11) + (1 if big else 0) and e.get_stat("log2cap") > bb
                res.append(_dump(e, min_count))
                assert e.get_stat("fused_dumps") == fused and e.get_stat("heavy_buckets") == 0 and e.get_stat("replayed_buckets") == 0
        _same(res[0], want, min_count)
        _same(res[1], want, min_count)
        assert len(res[0][0]) == (0 if min_count == top + 1 else int((want[2] >= min_count).sum()))


@pytest.mark.parametrize("k", [31, 63])
def test_no_counts_array(oracle, k):
    from kmer_denovo_filter_amd import ReadStream
    want = _want(oracle, k, "a", _reads(k))
    with _engine(k) as e:
        e.count(ReadStream.from_strings(_reads(k)))
        rc, n, lo, hi, cnt = _raw_dump(e, 2, 1 << 17, with_cnt=False)
        assert rc == 0 and e.get_stat("fused_dumps") == 1 and cnt is None
        assert (lo[n:] == SENT).all()
        keep = want[2] >= 2
        glo = lo[:n].view(np.uint64); ghi = hi[:n].view(np.uint64) if hi is not None else np.zeros(n, np.uint64)
        o = np.lexsort((glo, ghi))
        np.testing.assert_array_equal(glo[o], want[0][keep]); np.testing.assert_array_equal(ghi[o], want[1][keep])
        if k > 32:                                            # wide keys without the high words: refused, as by the table dump
            e.count(ReadStream.from_strings(_reads(k)))
            import torch
            buf = torch.zeros(16, dtype=torch.int64, device="cuda:0")
            nn = c_uint64(0)
            assert e._lib.kdf_export_ge_dev(e._h, 1, c_void_p(buf.data_ptr()), None, None, 16, 0, byref(nn)) != 0


@pytest.mark.parametrize("k", [31, 63])
def test_a_short_buffer_gets_the_full_count_and_nothing_past_its_end(oracle, k):
    from kmer_denovo_filter_amd import ReadStream
    want = _want(oracle, k, "a", _reads(k))
    keep = want[2] >= 2
    full = int(keep.sum())
    pairs = set(zip(want[0][keep].tolist(), want[1][keep].tolist(), want[2][keep].tolist()))
    st = ReadStream.from_strings(_reads(k))
    for cap in (0, 1, 63, 64, 65, full - 1):
        for fused in (1, 0):
            with _engine(k, fused) as e:
                e.count(st)
                rc, n, lo, hi, cnt = _raw_dump(e, 2, cap)
                assert rc != 0 and n == full, (cap, fused, rc, n, full)
                assert e.get_stat("fused_dumps") == fused
                assert (lo[cap:] == SENT).all() and (cnt[cap:] == SENT).all() and (hi is None or (hi[cap:] == SENT).all())
                got = set(zip(lo[:cap].view(np.uint64).tolist(), hi[:cap].view(np.uint64).tolist() if hi is not None else [0] * cap,
                              cnt[:cap].view(np.uint32).tolist()))
                assert len(got) == cap and got <= pairs           # the first `cap` places hold `cap` different entries of the dump
                _same(_dump(e, 2), want, 2)                       # (the table is whole: the table pass, nothing pending)


@pytest.mark.parametrize("k", [31, 63])
def test_saturated_counts_of_a_live_table(oracle, k):
    """keys loaded at 2^32 - 2 and 2^32 - 1, then counted again by a binned pass: a slot that wrapped in LDS is dumped as 0xFFFFFFFF,
    whatever the threshold"""
    from kmer_denovo_filter_amd import ReadStream
    reads = _reads(k)
    lo, hi, cnt = _want(oracle, k, "a", reads)
    ones = np.flatnonzero(cnt == 1)[:3]; many = np.flatnonzero(cnt >= 3)[:3]
    assert len(ones) == 3 and len(many) == 3
    idx = np.concatenate([ones, many])
    base = np.array([2**32 - 2] * 2 + [2**32 - 1] + [2**32 - 2] * 2 + [2**32 - 1], np.uint32)
    want_cnt = cnt.astype(np.uint64)
    want_cnt[idx] = np.minimum(want_cnt[idx] + base.astype(np.uint64), 2**32 - 1)
    want = (lo, hi, want_cnt.astype(np.uint32))
    assert (want[2][ones[:2]] == 0xFFFFFFFF).all() and (want[2][many] == 0xFFFFFFFF).all() and want[2][ones[2]] == 0xFFFFFFFF
    st = ReadStream.from_strings(reads)
    for min_count in (1, 3, 100):                             # (a wrapped slot holds 0 .. a few: below the last two thresholds)
        res = []
        for fused in (1, 0):
            with _engine(k, fused) as e:
                e.add_pairs(lo[idx], hi[idx] if k > 32 else None, base)
                e.count(st)
                assert e.get_stat("pending_passes") == 1
                res.append(_dump(e, min_count))
                assert e.get_stat("fused_dumps") == fused
        _same(res[0], want, min_count); _same(res[1], want, min_count)
        assert np.isin(lo[idx], res[0][0]).all()


@pytest.mark.parametrize("k", [31, 63])
def test_two_flushes_on_one_engine(oracle, k):
    from kmer_denovo_filter_amd import ReadStream
    a, b = _reads(k), _reads(k, n=900, seed=7)
    with _engine(k) as e:
        e.count(ReadStream.from_strings(a))
        _same(_dump(e, 2), _want(oracle, k, "a", a), 2)
        e.count(ReadStream.from_strings(b))                   # into the live table
        _same(_dump(e, 3), _want(oracle, k, "a+b", a + b), 3)
        assert e.get_stat("fused_dumps") == 2 and e.get_stat("flushes") == 2


if __name__ == "__main__":                                    # the child of the default-path test
    sys.path.insert(0, ROOT)
    _default_run(int(sys.argv[1]), sys.argv[2])
