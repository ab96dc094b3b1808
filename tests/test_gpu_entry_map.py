"""The entry map of the binned path's two gathers (``kb_entry_off``, csrc/kdf_device.h): a group of S adjacent lanes owns a
contiguous S x E entries of a wave's block, in kernel C's narrow path (``KB_C_SEG``, E = 12) and in the pipelined piece sort
(``KB_B_SEG``, E = 16).  A lane's run cursor is searched once and then only advanced, so the shapes here are those where a
remapped walk can go wrong, not the workload's.  Results must EQUAL the direct path's (``force_path`` 1) on the same reads:
the fused ``dump -L n``, then the count of every key (``query``: with ``lazy_table`` 1 that applies the retained passes through
the ordinary flush), with ``lazy_table`` 0 and 1, at k = 31 (the wide path keeps its per-entry search).

Forced binned (``force_path`` 2) on small tables, geometry read back through ``get_stat``: ``capacity_hint`` 2^17 gives 2^6
buckets and no coarse bits (one bin, a piece per slab of 16 384 stream positions), 2^21 gives 2^10 buckets, coarse bins and
pieces of several slabs.  The segment widths are compile-time constants the test cannot read, so the totals cover every S
in {8, 16, 32, 64}.

* ``totals``: one bucket each receives exactly T entries, T in {0, 1, S - 1, S, S + 1, S E - 1, S E, S E + 1, 64 E - 1,
  64 E + 1, CT E - 1, CT E, CT E + 1} (CT E = 768 x 12 = 9 216: the last three take a second batch).  The keys are chosen by
  their stored form (the mix is invertible: ``merge_truth.keys_with_hash``), canonical ones only, one read of k bases per
  entry, at most 200 distinct keys per bucket (a bucket has 4 096 slots), shuffled over ~64 slabs.
* ``empty``: 42 pending passes of a 6-slab stream -- 252 runs per bucket without coarse bits -- where one bucket's entries all
  lie in the FIRST slab of the first pass and another's all at the END of the last pass (its last slab or two): hundreds of
  zero-length runs behind / before the ones that hold everything, and no step past ``total``.
* ``mixed``: the homopolymer reads of tests/test_gpu_run_guess.py -- one run of thousands of entries among short ones, far
  below the skew threshold.
* ``rounds``: 56 pending passes of a 10-slab stream: more runs per bucket than kernel C stages per round (512).
* binned ``count --if`` of ``totals`` (``load_filter`` of every other key, then the forced-binned count): the same gather in
  the FILTERED instantiation.  ``load_filter`` sizes the table for the filter, so it is padded with keys the reads do not
  hold: 2^17 keys give 2^6 buckets again, 2^20 keys 2^9 buckets (one coarse bit).
* piece sort: ``KDF_C1`` forcing nb = 1, 2, 256 and 1 024 coarse bins, on ``sparse`` (reads of k bases with random keys over
  three slabs: with 1 024 bins runs of length 0 and 1 everywhere), ``slab+1`` (one slab plus one read of k + 6 bases: the
  last piece has at most 7 entries, less than any S, and the last group is short) and ``full`` (a read of 2.5 slabs of
  bases: without coarse bits a slab whose every window is valid is a piece of exactly 16 384 entries)."""
import functools

import numpy as np
import pytest

import merge_truth as MT

pytestmark = pytest.mark.gpu

K = 31
SMALL, LARGE = 1 << 17, 1 << 21
NB_BITS = {SMALL: 6, LARGE: 10}
SLAB = 16384
SENT = -7
ACGT = np.frombuffer(b"ACGT", np.uint8)
E_C, CT = 12, 768
TOTALS = sorted({0, 1} | {s + d for s in (8, 16, 32, 64) for d in (-1, 0, 1)} | {s * E_C + d for s in (8, 16, 32, 64) for d in (-1, 0, 1)}
                | {64 * E_C - 1, 64 * E_C + 1} | {CT * E_C - 1, CT * E_C, CT * E_C + 1})
CALLS_EMPTY, CALLS_ROUNDS = 42, 56
FIRST10, LAST10 = 37, 1000                             # the two buckets of ``empty``, as 10-bit hash prefixes (6-bit: 2 and 62)


def _prefix10(i):
    """the i-th bucket of ``totals`` as a 10-bit hash prefix; the 6-bit prefixes 2 i + 1 differ too"""
    return ((2 * i + 1) << 4) | (i & 15)


def _kmer_reads(lo, reps):
    """one read of k bases per occurrence, every other KEY as its reverse complement"""
    out = []
    for i, (a, c) in enumerate(zip(lo.tolist(), np.asarray(reps).tolist())):
        s = MT.kmer_string(a, None, K)
        out += [(MT.revcomp_string(s) if i & 1 else s).encode()] * int(c)
    return out


@functools.lru_cache(maxsize=None)
def _totals_keys():
    """per total T: (distinct keys of its bucket, multiplicities summing to T)"""
    rng = np.random.default_rng(21)
    assert len(TOTALS) <= 31
    out = []
    for i, t in enumerate(TOTALS):
        d = min(t, 200)
        lo = MT.keys_with_hash(_prefix10(i), 10, d, K, rng, canonical=True)[0] if d else np.zeros(0, np.uint64)
        reps = np.full(d, t // d if d else 0, np.int64)
        reps[:t - int(reps.sum())] += 1
        assert int(reps.sum()) == t
        out.append((lo, reps))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _pool():
    """150 bp reads over a 30 kb genome, 0.3 % N"""
    rng = np.random.default_rng(22)
    genome = ACGT[rng.integers(0, 4, 30_000)]
    out = []
    for a in rng.integers(0, len(genome) - 150, 2000):
        r = genome[a:a + 150].copy()
        r[rng.random(150) < 0.003] = ord("N")
        out.append(r.tobytes())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _case(which):
    """the ReadStreams an engine counts, in order"""
    from kmer_denovo_filter_amd import ReadStream
    S = ReadStream.from_strings
    rng = np.random.default_rng({"totals": 31, "empty": 32, "mixed": 5, "rounds": 7, "sparse": 33, "slab+1": 34, "full": 35}[which])
    if which == "totals":
        reads = [r for lo, reps in _totals_keys() for r in _kmer_reads(lo, reps)]
        reads = [reads[i] for i in rng.permutation(len(reads))]
        return (S(reads),)
    if which == "empty":
        lo = MT.keys_with_hash(0, 0, 3200, K, rng, canonical=True)[0]
        top6 = MT.key_hash(lo) >> np.uint64(58)
        bg = _kmer_reads(lo[(top6 != np.uint64(FIRST10 >> 4)) & (top6 != np.uint64(LAST10 >> 4))][:3000], np.ones(3000, int))
        assert len(bg) == 3000
        ends = []
        for p in (FIRST10, LAST10):
            klo = MT.keys_with_hash(p, 10, 100, K, rng, canonical=True)[0]
            ends.append(_kmer_reads(klo, np.full(100, 3)))
        first, mid, last = S(ends[0] + bg), S(bg), S(bg + ends[1])
        assert 5 * SLAB < mid.n_bases <= 6 * SLAB and first.n_bases - mid.n_bases < SLAB and last.n_bases - mid.n_bases < SLAB
        return (first,) + (mid,) * (CALLS_EMPTY - 2) + (last,)
    if which in ("mixed", "rounds"):                     # (tests/test_gpu_run_guess.py)
        genome = ACGT[rng.integers(0, 4, 30_000)]
        n = 2600 if which == "mixed" else 1030
        out = []
        for i in range(n):
            a = int(rng.integers(0, len(genome) - 150))
            r = genome[a:a + 150].copy()
            r[rng.random(150) < 0.003] = ord("N")
            out.append(r.tobytes())
            if which == "mixed" and i == n // 2:
                out.extend([b"C" * 150] * 50)
        s = S(out)
        assert s.n_bases % SLAB != 0 and (s.n_bases > 20 * SLAB if which == "mixed" else -(-s.n_bases // SLAB) * CALLS_ROUNDS > 512)
        return (s,) * (1 if which == "mixed" else CALLS_ROUNDS)
    if which == "sparse":
        lo = MT.keys_with_hash(0, 0, 1500, K, rng, canonical=True)[0]
        s = S(_kmer_reads(lo, np.ones(1500, int)))
        assert 2 * SLAB < s.n_bases <= 3 * SLAB
        return (s,)
    pool = _pool()
    if which == "slab+1":
        per = S(pool[:2]).n_bases - S(pool[:1]).n_bases                    # stream positions a 150 bp read takes
        n = SLAB // per - 1
        room = SLAB - S(pool[:n]).n_bases                                   # what is left of the first slab
        fill = ACGT[rng.integers(0, 4, room - (per - 150))].tobytes()      # a read that ends the slab
        tail = ACGT[rng.integers(0, 4, K + 6)].tobytes()                    # 7 windows
        assert S(pool[:n] + (fill,)).n_bases == SLAB, (per, n, room)
        s = S(pool[:n] + (fill, tail))
        assert SLAB < s.n_bases <= SLAB + K + 6 + 8
        return (s,)
    assert which == "full"
    long_read = ACGT[rng.integers(0, 4, 5 * SLAB // 2)].tobytes()          # 2.5 slabs of bases: one slab holds nothing else
    return (S(pool[:30] + (long_read,) + pool[30:60]),)


@functools.lru_cache(maxsize=None)
def _reference(which):
    """(lo, hi, cnt) of the direct path on the same calls, ascending keys; built once and left unchanged"""
    from kmer_denovo_filter_amd import KmerEngine
    with KmerEngine(K, capacity_hint=LARGE) as e:
        e.set_option("force_path", 1)
        for s in _case(which):
            e.count(s)
            assert e.last_count_path() == "direct"
        lo, hi, cnt = e.export_ge(0)
    cnt = cnt.astype(np.uint64)
    assert len(lo) > 0 and int(cnt.max()) < 1 << 32
    for a in (lo, hi, cnt):
        a.setflags(write=False)
    return lo, hi, cnt


def _binned(lazy, hint):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(K, capacity_hint=hint)
    e.set_option("force_path", 2); e.set_option("lazy_table", lazy); e.set_option("fused_dump", 1)
    e.clear()                                          # (the dump-only flush is for a table that was only cleared)
    return e


def _geometry(e, hint):
    nb_bits = e.get_stat("log2cap") - e.get_stat("bucket_bits")
    assert nb_bits == NB_BITS[hint] and e.get_stat("bucket_bits") == 12, (hint, nb_bits)
    return nb_bits


def _fused_dump(e, min_count, cap):
    import torch
    lo = torch.full((cap + 64,), SENT, dtype=torch.int64, device="cuda:0")
    cnt = torch.full((cap + 64,), SENT, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    n = e.export_ge_dev(min_count, lo.data_ptr(), None, cnt.data_ptr(), cap)
    torch.cuda.synchronize()
    lo, cnt = lo.cpu().numpy(), cnt.cpu().numpy()
    assert n <= cap and (lo[n:] == SENT).all() and (cnt[n:] == SENT).all()
    lo, cnt = lo[:n].view(np.uint64), cnt[:n].view(np.uint32).astype(np.uint64)
    o = np.argsort(lo)
    return lo[o], cnt[o]


def _count_and_check(e, which, min_count, lazy=None):
    """count the case's streams, then: fused dump -L min_count, every key's count, the whole table"""
    lo, _, cnt = _reference(which)
    streams = _case(which)
    e.clear()
    before = {n: e.get_stat(n) for n in ("fused_dumps", "flushes", "dump_only_flushes")}
    for s in streams:
        e.count(s)
    assert e.last_count_path() == "binned" and e.get_stat("pending_passes") == len(streams) and e.get_stat("flushes") == before["flushes"]
    keep = cnt >= min_count
    assert 0 < int(keep.sum())
    glo, gcnt = _fused_dump(e, min_count, len(lo) + 64)
    np.testing.assert_array_equal(glo, lo[keep]); np.testing.assert_array_equal(gcnt, cnt[keep])
    # the dump came out of kernel C, in one flush, every bucket resolved by it (none failed, replayed or split as heavy)
    assert e.get_stat("fused_dumps") == before["fused_dumps"] + 1 and e.get_stat("flushes") == before["flushes"] + 1
    if lazy is not None:
        assert e.get_stat("dump_only_flushes") == before["dump_only_flushes"] + lazy
    assert (e.get_stat("replayed_buckets"), e.get_stat("heavy_buckets")) == (0, 0)
    np.testing.assert_array_equal(e.query(lo, None).astype(np.uint64), cnt)
    assert e.get_stat("replayed_buckets") == 0
    elo, _, ecnt = e.export_ge(0)
    np.testing.assert_array_equal(elo, lo); np.testing.assert_array_equal(ecnt.astype(np.uint64), cnt)


def _bucket_totals(hint):
    """entries per bucket of ``totals`` under the table's geometry, from the reference"""
    lo, _, cnt = _reference("totals")
    b = MT.bucket(MT.key_hash(lo), NB_BITS[hint] + 12, 12).astype(np.int64)
    return np.bincount(b, weights=cnt.astype(np.float64), minlength=1 << NB_BITS[hint]).astype(np.int64)


@pytest.mark.parametrize("hint", [SMALL, LARGE], ids=["c1=0", "c1>0"])
@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
def test_bucket_totals_at_the_edges_of_the_map(lazy, hint):
    per_bucket = _bucket_totals(hint)
    shift = 10 - NB_BITS[hint]
    assert [int(per_bucket[_prefix10(i) >> shift]) for i in range(len(TOTALS))] == TOTALS      # exactly T entries each ...
    assert int(per_bucket.sum()) == sum(TOTALS) and int((per_bucket == 0).sum()) >= 1           # ... and buckets with none
    assert -(-_case("totals")[0].n_bases // SLAB) >= 32
    with _binned(lazy, hint) as e:
        _geometry(e, hint)
        _count_and_check(e, "totals", 1, lazy)


@pytest.mark.parametrize("hint", [SMALL, LARGE], ids=["c1=0", "c1>0"])
@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
def test_hundreds_of_empty_runs_before_and_after(lazy, hint):
    lo, _, cnt = _reference("empty")
    top10 = (MT.key_hash(lo) >> np.uint64(54)).astype(np.int64)
    shift = 10 - NB_BITS[hint]
    for p in (FIRST10, LAST10):                                   # the two buckets hold their 300 entries and nothing else
        inb = (top10 >> shift) == (p >> shift)
        assert int(cnt[inb].sum()) == 300 and (top10[inb] == p).all()
    with _binned(lazy, hint) as e:
        _geometry(e, hint)
        _count_and_check(e, "empty", 2, lazy)


@pytest.mark.parametrize("hint", [SMALL, LARGE], ids=["c1=0", "c1>0"])
@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
def test_one_long_run_among_short_ones(lazy, hint):
    cnt = _reference("mixed")[2]
    rep = int(cnt.max())
    assert rep >= 50 * (150 - K + 1) and rep > 20 * int(np.sort(cnt)[-2]) and rep > (int(cnt.sum()) - rep) >> NB_BITS[hint]
    with _binned(lazy, hint) as e:
        _geometry(e, hint)
        _count_and_check(e, "mixed", 2, lazy)


@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
def test_more_runs_than_one_round_stages(lazy):
    with _binned(lazy, SMALL) as e:
        _geometry(e, SMALL)                                       # c1 = 0: every bucket reads every piece
        _count_and_check(e, "rounds", 3 * CALLS_ROUNDS, lazy)


@pytest.mark.parametrize("hint", [SMALL, LARGE], ids=["c1=0", "c1>0"])
def test_binned_count_if_through_the_same_gather(hint):
    from kmer_denovo_filter_amd import KmerEngine
    lo, _, cnt = _reference("totals")
    flo, want = np.ascontiguousarray(lo[::2]), cnt[::2]
    # (load_filter sizes the table for the filter: padded with keys the reads do not hold, to hint keys = 2^6 buckets without
    # coarse bits, or hint / 2 keys = 2^9 buckets with one coarse bit)
    n_filter, nb_bits = (hint, 6) if hint == SMALL else (hint // 2, 9)
    pads = np.setdiff1d(np.unique(np.random.default_rng(36).integers(0, 1 << 62, n_filter, dtype=np.uint64)), lo)[:n_filter - len(flo)]
    full = np.concatenate([flo, pads])
    assert len(full) == n_filter and MT.valid_keys(full, None, K).all()
    s = _case("totals")[0]
    with KmerEngine(K, capacity_hint=hint) as d:                  # the direct path agrees with the insert-mode reference
        d.load_filter(full, None)
        d.set_option("force_path", 1)
        d.count_filtered(s)
        np.testing.assert_array_equal(d.query(flo, None).astype(np.uint64), want)
    with KmerEngine(K, capacity_hint=hint) as e:
        e.load_filter(full, None)
        e.set_option("force_path", 2)
        assert e.get_stat("log2cap") - e.get_stat("bucket_bits") == nb_bits and e.get_stat("bucket_bits") == 12
        e.count_filtered(s)
        assert e.last_count_path() == "binned"
        np.testing.assert_array_equal(e.query(flo, None).astype(np.uint64), want)
        np.testing.assert_array_equal(e.query(np.ascontiguousarray(lo[1::2]), None), np.zeros(len(lo[1::2]), np.uint32))
        assert int(e.query(pads, None).sum()) == 0
        assert (e.get_stat("replayed_buckets"), e.get_stat("heavy_buckets")) == (0, 0)
        e.reset_counts()
        e.count_filtered(s); e.count_filtered(s)                  # two pending passes into the live counts
        np.testing.assert_array_equal(e.query(flo, None).astype(np.uint64), want * np.uint64(2))


@pytest.mark.parametrize("nb", [1, 2, 256, 1024])
@pytest.mark.parametrize("lazy", [1, 0], ids=["dump-only", "ordinary"])
def test_piece_sort_at_forced_splits(monkeypatch, lazy, nb):
    c1 = nb.bit_length() - 1
    hint = SMALL if nb == 1 else LARGE
    monkeypatch.setenv("KDF_C1", str(c1))                         # (read when a plan is made: set before the engine exists)
    with _binned(lazy, hint) as e:
        _geometry(e, hint)
        assert e.get_stat("c1") == c1, "KDF_C1 did not take effect"
        for which in ("sparse", "slab+1", "full"):
            _count_and_check(e, which, 1)
            assert e.get_stat("c1") == c1 and e.get_stat("c1") + e.get_stat("c2") == NB_BITS[hint]
