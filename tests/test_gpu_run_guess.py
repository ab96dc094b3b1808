"""The run guesses of the binned path (``kb_guess_scale`` / ``kb_guess_run``, csrc/kdf_device.h: a float reciprocal where the
kernels divided integers) on inputs where a guess is furthest from the run that holds the entry.  A guess is only where
a search starts, so the results must EQUAL the direct path's (``force_path`` 1) on the same reads: the fused ``dump -L n``,
then the count of every key (``query``: with ``lazy_table`` 1 that applies the retained passes through the ordinary flush).

Forced binned (``force_path`` 2) on small tables, geometry read from ``get_stat``: ``capacity_hint`` 2^17 gives at most 2^8
buckets -- no coarse bits (kb_make_plan: c1 = 0, one bin, a piece per slab) -- and 2^21 gives 2^10 and more buckets -- c1 >= 1:
several bins, pieces of several slabs.  A slab is 16 384 stream positions (k <= 32) or 8 192 (k = 63).

* ``mixed``: 2 600 reads of 150 bp over a 30 kb genome, with N, and in their middle 50 reads that are one k-mer repeated
  (a homopolymer: 6 000 windows at k = 31, less than a slab of stream).  That key's bucket has one run (two, where the
  50 reads straddle a slab boundary) with thousands of entries -- more than all its other runs together, which hold a few
  hundred each at c1 = 0 and a few dozen at c1 >= 1 -- so the interpolated guess is runs away from the truth for most
  entries (kernel C: the walk behind the window; the piece sort: the walk over the slab runs).  The stream is no
  multiple of a slab, so its last piece is cut short, and with c1 >= 1 the last group has fewer slabs than the others.
  (Far below 65 536 surplus entries: no skew flag.)
* ``single``: one read of k bases -- one window: a bucket with ONE entry (total = 1) beside buckets with none (total = 0),
  and a bin with exactly one piece.
* ``rounds``: a stream of 10 slabs (k = 31; 19 at k = 63) counted 56 times before the one flush: 56 pending passes, 560
  runs per bucket and more at c1 = 0 -- kernel C stages 512 (k = 31) or 256 (k = 63) per round, so it takes two rounds or
  more.  The direct engine counts the stream once; the counts are additive, so its counts times 56 are the reference."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [31, 63]
SMALL, LARGE = 1 << 17, 1 << 21
SLAB_MAX = 16384
CALLS = 56
SENT = -7


@functools.lru_cache(maxsize=None)
def _reads(which, k):
    rng = np.random.default_rng({"mixed": 5, "single": 6, "rounds": 7}[which])
    acgt = np.frombuffer(b"ACGT", np.uint8)
    if which == "single":
        return (acgt[rng.integers(0, 4, k)].tobytes(),)
    genome = acgt[rng.integers(0, 4, 30_000)]
    n = 2600 if which == "mixed" else 1030
    out = []
    for i in range(n):
        a = int(rng.integers(0, len(genome) - 150))
        r = genome[a:a + 150].copy()
        r[rng.random(150) < 0.003] = ord("N")
        out.append(r.tobytes())
        if which == "mixed" and i == n // 2:
            out.extend([b"C" * 150] * 50)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _stream(which, k):
    from kmer_denovo_filter_amd import ReadStream
    return ReadStream.from_strings(_reads(which, k))


@functools.lru_cache(maxsize=None)
def _reference(which, k, hint):
    """(lo, hi, cnt) of the direct path on the same reads, ascending keys; built once and left unchanged"""
    from kmer_denovo_filter_amd import KmerEngine
    with KmerEngine(k, capacity_hint=hint) as e:
        e.set_option("force_path", 1)
        e.count(_stream(which, k))
        assert e.last_count_path() == "direct"
        lo, hi, cnt = e.export_ge(0)
    cnt = cnt.astype(np.uint64) * (CALLS if which == "rounds" else 1)
    assert len(lo) > 0 and int(cnt.max()) < 1 << 32
    for a in (lo, hi, cnt):
        a.setflags(write=False)
    return lo, hi, cnt


def _binned(k, lazy, hint):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=hint)
    e.set_option("force_path", 2); e.set_option("lazy_table", lazy); e.set_option("fused_dump", 1)
    e.clear()                                          # (the dump-only flush is for a table that was only cleared)
    return e


def _geometry(e, hint):
    """table buckets, from the engine; the hint chose between no coarse bits and some (kb_make_plan: 8 fine bits first)"""
    nb_bits = e.get_stat("log2cap") - e.get_stat("bucket_bits")
    assert (nb_bits <= 8) if hint == SMALL else (nb_bits > 8), (hint, nb_bits)
    return nb_bits


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


def _check(e, ref, min_count, lazy, flushes_before=0):
    lo, hi, cnt = ref
    keep = cnt >= min_count
    assert 0 < int(keep.sum())
    o = np.lexsort((lo[keep], hi[keep]))
    got = _fused_dump(e, min_count, len(lo) + 64)
    for g, w in zip(got, (lo[keep][o], hi[keep][o], cnt[keep][o])):
        np.testing.assert_array_equal(g, w)
    # the dump came out of kernel C, in one flush, every bucket resolved by it (none failed, replayed or split as heavy)
    assert e.get_stat("fused_dumps") == 1 and e.get_stat("dump_only_flushes") == lazy
    assert e.get_stat("flushes") == flushes_before + 1
    assert (e.get_stat("replayed_buckets"), e.get_stat("heavy_buckets")) == (0, 0)
    # every key's count (lazy: the retained passes go through the ordinary flush now)
    np.testing.assert_array_equal(e.query(lo, hi if e.wide else None).astype(np.uint64), cnt)
    assert e.get_stat("replayed_buckets") == 0
    elo, ehi, ecnt = e.export_ge(0)
    np.testing.assert_array_equal(elo, lo); np.testing.assert_array_equal(ecnt.astype(np.uint64), cnt)
    if e.wide:
        np.testing.assert_array_equal(ehi, hi)


@pytest.mark.parametrize("hint", [SMALL, LARGE], ids=["c1=0", "c1>0"])
@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
@pytest.mark.parametrize("k", KS)
def test_one_long_run_among_short_ones(k, lazy, hint):
    s = _stream("mixed", k)
    assert s.n_bases % SLAB_MAX != 0 and s.n_bases > 20 * SLAB_MAX           # many slabs, the last cut short
    ref = _reference("mixed", k, hint)
    rep = int(ref[2].max())
    assert rep >= 50 * (150 - k + 1) and rep > 20 * int(np.sort(ref[2])[-2])     # the repeated k-mer, far above every other key
    with _binned(k, lazy, hint) as e:
        nb_bits = _geometry(e, hint)
        # its bucket: the long run holds more than an even share of everything else
        assert rep > (int(ref[2].sum()) - rep) // (1 << nb_bits)
        e.count(s)
        assert e.last_count_path() == "binned" and e.get_stat("pending_passes") == 1
        _check(e, ref, 2, lazy)


@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
@pytest.mark.parametrize("k", KS)
def test_bucket_with_one_entry(k, lazy):
    s = _stream("single", k)
    assert s.n_bases <= k + 1
    ref = _reference("single", k, SMALL)
    assert len(ref[0]) == 1 and int(ref[2][0]) == 1
    with _binned(k, lazy, SMALL) as e:
        _geometry(e, SMALL)
        e.count(s)
        assert e.last_count_path() == "binned" and e.get_stat("pending_passes") == 1
        _check(e, ref, 1, lazy)


@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
@pytest.mark.parametrize("k", KS)
def test_more_runs_than_one_round_stages(k, lazy):
    s = _stream("rounds", k)
    slabs = -(-s.n_bases // SLAB_MAX)
    assert slabs * CALLS > 512 and s.n_bases % SLAB_MAX != 0                  # (k = 63 has twice the slabs and stages 256 runs)
    ref = _reference("rounds", k, SMALL)
    with _binned(k, lazy, SMALL) as e:
        _geometry(e, SMALL)                                                   # c1 = 0: every bucket reads every piece
        for _ in range(CALLS):
            e.count(s)
        assert e.last_count_path() == "binned" and e.get_stat("pending_passes") == CALLS and e.get_stat("flushes") == 0
        _check(e, ref, 3 * CALLS, lazy)
