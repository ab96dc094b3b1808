"""The scans of the partition kernels (csrc/kdf_scan.h: kernel A's strip scan, the block scans of the piece sort and the
bucket kernel, ``KbRunIndex::setup``) at every split of the bucket bits they take another path at, on streams whose slab
counts sit around the group and wave boundaries.  Forced binned (``force_path`` 2) must EQUAL the direct path
(``force_path`` 1) on the same reads: the fused ``dump -L n``, then the count of every key (``query``; with ``lazy_table`` 1
that applies the retained passes through the ordinary flush).

The split is chosen with ``KDF_C1`` (read when a plan is made, so it is set before the engine exists) and read back through
``get_stat("c1")`` / ``get_stat("c2")``.  ``capacity_hint`` 2^21 gives 2^10 buckets (k = 31; 2^11 at k = 63): nb = 2^c1 = 32, 64,
128, 256 and 1024 coarse bins.  One bin (nb = 1) cannot be asked of that table -- the fine radix has at most 9 bits -- so
that case runs on ``capacity_hint`` 2^17 (2^8 buckets and fewer), where the plan has no coarse bits.

* streams of 1, 2, 17, 33 and 65 slabs (a slab: 16 384 stream positions at k = 31, 8 192 at k = 63), 150 bp reads with N;
* ``edges``: a stream with more than a slab of N-only reads (a slab without a valid window) and one read of 2.5 slabs of
  bases (a slab whose every window is valid) between ordinary reads;
* nb = 1024 on a stream of 1 003 slabs: a full first group (kb_make_plan before the engine's first flush: 0.98 x 1024
  slabs), threads of eight waves of the piece sort hold the runs of two slabs each;
* 1, 2, 16, 17 and 64 pending passes before the one flush (a 3-slab stream counted n times; the reference is the direct
  counts x n): ``setup``'s scan crosses every row of 16 lanes, and a single pass takes its scan-free path."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [31, 63]
SMALL, LARGE = 1 << 17, 1 << 21
SENT = -7
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _slab(k):
    return 16384 if k <= 32 else 8192


@functools.lru_cache(maxsize=None)
def _pool():
    """150 bp reads over a 30 kb genome, 0.3 % N -- every stream is a prefix of it"""
    rng = np.random.default_rng(11)
    genome = ACGT[rng.integers(0, 4, 30_000)]
    out = []
    for a in rng.integers(0, len(genome) - 150, 111_000):
        r = genome[a:a + 150].copy()
        r[rng.random(150) < 0.003] = ord("N")
        out.append(r.tobytes())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _stream(which, k):
    """which: a number of slabs, or "edges"; -> (ReadStream, slabs)"""
    from kmer_denovo_filter_amd import ReadStream
    pool, slab = _pool(), _slab(k)
    if which == "edges":
        rng = np.random.default_rng(12)
        n_only = [b"N" * 150] * (2 * slab // 150 + 40)                     # more than two slabs of N: one slab holds nothing else
        long_read = ACGT[rng.integers(0, 4, 5 * slab // 2)].tobytes()     # 2.5 slabs of bases: one slab holds nothing else
        reads = pool[:60] + tuple(n_only) + pool[60:90] + (long_read,) + pool[90:140]
    else:
        per_read = ReadStream.from_strings(pool[:200]).n_bases / 200.0
        reads = pool[:int((which - 0.5) * slab / per_read)]
    s = ReadStream.from_strings(reads)
    slabs = -(-s.n_bases // slab)
    assert which == "edges" or slabs == which, (which, slabs, s.n_bases)
    return s, slabs


@functools.lru_cache(maxsize=None)
def _reference(which, k):
    """(lo, hi, cnt) of the direct path on the same reads, ascending keys; built once and left unchanged"""
    from kmer_denovo_filter_amd import KmerEngine
    with KmerEngine(k, capacity_hint=LARGE) as e:
        e.set_option("force_path", 1)
        e.count(_stream(which, k)[0])
        assert e.last_count_path() == "direct"
        lo, hi, cnt = e.export_ge(0)
    cnt = cnt.astype(np.uint64)
    assert len(lo) > 0
    for a in (lo, hi, cnt):
        a.setflags(write=False)
    return lo, hi, cnt


def _binned(k, lazy, hint):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=hint)
    e.set_option("force_path", 2); e.set_option("lazy_table", lazy); e.set_option("fused_dump", 1)
    e.clear()                                          # (the dump-only flush is for a table that was only cleared)
    return e


def _fused_dump(e, min_count, cap):
    import torch
    lo = torch.full((cap + 64,), SENT, dtype=torch.int64, device="cuda:0")
    hi = torch.full((cap + 64,), SENT, dtype=torch.int64, device="cuda:0")
    cnt = torch.full((cap + 64,), SENT, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    n = e.export_ge_dev(min_count, lo.data_ptr(), hi.data_ptr() if e.wide else None, cnt.data_ptr(), cap)
    torch.cuda.synchronize()
    lo, hi, cnt = lo.cpu().numpy(), hi.cpu().numpy(), cnt.cpu().numpy()
    assert n <= cap and (lo[n:] == SENT).all() and (cnt[n:] == SENT).all()
    lo, cnt = lo[:n].view(np.uint64), cnt[:n].view(np.uint32).astype(np.uint64)
    hi = hi[:n].view(np.uint64) if e.wide else np.zeros(n, np.uint64)
    o = np.lexsort((lo, hi))
    return lo[o], hi[o], cnt[o]


def _check(e, ref, times):
    """fused dump -L (2 x times), then every key's count, of an engine that holds `times` passes of the reference's stream"""
    lo, hi, cnt = ref
    cnt = cnt * np.uint64(times)
    assert int(cnt.max()) < 1 << 32
    min_count = 2 * times if int((cnt >= 2 * times).sum()) else times
    keep = cnt >= min_count
    before = {n: e.get_stat(n) for n in ("fused_dumps", "flushes")}
    got = _fused_dump(e, min_count, len(lo) + 64)
    for g, w in zip(got, (lo[keep], hi[keep], cnt[keep])):               # (the reference is in ascending key order already)
        np.testing.assert_array_equal(g, w)
    # the dump came out of kernel C, in one flush, every bucket resolved by it (none failed, replayed or split as heavy)
    assert e.get_stat("fused_dumps") == before["fused_dumps"] + 1 and e.get_stat("flushes") == before["flushes"] + 1
    assert (e.get_stat("replayed_buckets"), e.get_stat("heavy_buckets")) == (0, 0)
    np.testing.assert_array_equal(e.query(lo, hi if e.wide else None).astype(np.uint64), cnt)
    assert e.get_stat("replayed_buckets") == 0


def _count_and_check(e, k, which, c1, times=1):
    s, slabs = _stream(which, k)
    e.clear()
    for _ in range(times):
        e.count(s)
    assert e.last_count_path() == "binned" and e.get_stat("pending_passes") == times
    if c1 is not None:
        assert e.get_stat("c1") == c1 and e.get_stat("c1") + e.get_stat("c2") == e.get_stat("log2cap") - e.get_stat("bucket_bits")
    _check(e, _reference(which, k), times)
    return slabs


def _engine_with_split(monkeypatch, k, lazy, nb):
    c1 = nb.bit_length() - 1
    monkeypatch.setenv("KDF_C1", str(c1))
    e = _binned(k, lazy, SMALL if nb == 1 else LARGE)
    nb_bits = e.get_stat("log2cap") - e.get_stat("bucket_bits")
    assert (nb_bits <= 8) if nb == 1 else (nb_bits == (10 if k == 31 else 11)), nb_bits
    assert e.get_stat("c1") == c1, "KDF_C1 did not take effect"
    return e, c1


@pytest.mark.parametrize("nb", [1, 32, 64, 128, 256, 1024])
@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
@pytest.mark.parametrize("k", KS)
def test_streams_of_few_slabs_at_every_split(monkeypatch, k, lazy, nb):
    e, c1 = _engine_with_split(monkeypatch, k, lazy, nb)
    with e:
        for which in (1, 2, 17, 33, 65, "edges"):
            _count_and_check(e, k, which, c1)


@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
@pytest.mark.parametrize("k", KS)
def test_full_group_of_1003_slabs_at_1024_bins(monkeypatch, k, lazy):
    e, c1 = _engine_with_split(monkeypatch, k, lazy, 1024)
    with e:
        assert _count_and_check(e, k, 1003, c1) == 1003


@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
@pytest.mark.parametrize("k", KS)
def test_pending_passes_across_the_rows_of_the_wave_scan(monkeypatch, k, lazy):
    monkeypatch.delenv("KDF_C1", raising=False)
    with _binned(k, lazy, LARGE) as e:
        for times in (1, 2, 16, 17, 64):
            _count_and_check(e, k, 3, None, times)
