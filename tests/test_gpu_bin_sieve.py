"""count --if through the bin-major sieve (option ``sieve_bins``): kernel A, the transposer and ``kdf_bin_sieve_kernel``.

Truth is ``oracle.py_count(reads, k, set(filter))`` -- counts and ``stats()`` windows, bit for bit -- and the same engine
under ``force_path`` 1 (direct kernel) and 2 (binned pipeline).  Every case asserts ``last_count_path == 5`` and
``last_sieve_bins``, so that a silent fall-back to another path fails the case.

Shapes are the smallest at which the kernels can still go wrong: one tile, less than a slab, exactly two slabs, three
slabs and a part; 16 / 256 / 1024 bins (1024 is the ``nb == NT`` corner of kernel A's offset row); ~100 windows over 1024
bins (most runs empty); one read 20 000 times and a poly-A set (whole slabs in one bin); a saturated sieve (the queues
drain all the time); several passes per call; dirty words at and past ``n_bases``; the sieve's lifetime."""
import numpy as np
import pytest
import torch

from kmer_denovo_filter_amd import KmerEngine, ReadStream, kmers_to_keys
from kmer_denovo_filter_amd._native import KdfError
from kmer_denovo_filter_amd.spool import ReadSpool
from test_gpu_parity_basic import rand_reads
from test_gpu_stream_tail import cpu, cut_reads, layout, words

pytestmark = pytest.mark.gpu

KS = (5, 31, 32, 33, 63)
BINS = (4, 8, 10)
_RNG = np.random.default_rng(20261020)
_G = _RNG.integers(0, 4, 40_000).astype(np.uint8)
READS = rand_reads(_RNG, 360, 150, 150, n_frac=0.004, genome=_G)
READS[7] = READS[7][:40].upper() + READS[7][40:95].lower() + READS[7][95:].upper()     # a lowercase stretch
_TRUTH = {}


def all_counts(O, reads, k):
    """py_count of the first `reads` of READS (an int) or of a read list, computed once"""
    key = (reads, k) if isinstance(reads, int) else (tuple(reads), k)
    if key not in _TRUTH:
        _TRUTH[key] = O.py_count(READS[:reads] if isinstance(reads, int) else reads, k)
    return _TRUTH[key]


def rand_kmers(rng, n, k):
    return ["".join("ACGT"[c] for c in row) for row in rng.integers(0, 4, (n, k))]


def make_filter(O, k, seed=3, present=300, absent=300):
    """~present k-mers of READS and ~absent random ones (canonical, distinct, in a fixed order)"""
    rng = np.random.default_rng(seed)
    have = sorted(all_counts(O, len(READS), k))
    pick = [have[i] for i in sorted(rng.choice(len(have), min(present, len(have)), replace=False))]
    extra = {O.canonicalize(s) for s in rand_kmers(rng, absent, k)} - set(pick)
    return pick + sorted(extra)


def expect(O, reads, k, kmers):
    """(counts of kmers, valid windows) of a count --if of the reads: oracle.py_count(reads, k, set(filter)), computed once"""
    key = (reads if isinstance(reads, int) else tuple(reads), k, tuple(kmers))
    if key not in _TRUTH:
        d = O.py_count(READS[:reads] if isinstance(reads, int) else reads, k, set(kmers))
        _TRUTH[key] = np.array([d[c] for c in kmers], np.uint32)
    return _TRUTH[key], sum(all_counts(O, reads, k).values())


def filter_engine(k, kmers, bins, reserve=1 << 14):
    e = KmerEngine(k, capacity_hint=1 << 12)
    lo, hi = kmers_to_keys(kmers, k)
    e.load_filter(lo, hi)
    if reserve:
        e.reserve(reserve)                    # more than one bucket: force_path 2 really takes the binned pipeline
    e.set_option("sieve_bins", bins)
    return e, (lo, hi)


def run_paths(e, keys, count_fn, bins, tag):
    """count_fn() under the bin sieve, the direct kernel and the binned pipeline -> (counts, windows) of the first"""
    out = []
    for fp, path in ((0, 5), (1, 0), (2, 1)):
        e.set_option("force_path", fp)
        e.reset_counts()
        w0 = e.stats()[2]
        count_fn()
        got = e.get_stat("last_count_path")
        assert got == path, f"{tag}: force_path {fp} took path {got}"
        if fp == 0:
            assert e.get_stat("last_sieve_bins") == bins, tag
        out.append((e.query(*keys), e.stats()[2] - w0))
    e.set_option("force_path", 0)
    for fp, (c, w) in zip((1, 2), out[1:]):
        assert np.array_equal(out[0][0], c), f"{tag}: counts differ from force_path {fp}"
        assert out[0][1] == w, f"{tag}: windows {out[0][1]} differ from force_path {fp}: {w}"
    return out[0]


def n_reads_for(k, which):
    """read prefixes of READS (150 bp + separator = 151 positions each) for the four stream lengths"""
    slab = 16384 if k <= 32 else 8192
    return {"sub_slab": 30, "two_slabs": 2 * slab // 151 - 1, "three_and_a_bit": 360 if k <= 32 else 180}[which]


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("k", KS)
def test_counts_match_oracle_and_other_paths(oracle, k, bins):
    kmers = make_filter(oracle, k)
    slab = 16384 if k <= 32 else 8192
    streams = {"one_tile": [READS[0][:63]]}
    for which in ("sub_slab", "three_and_a_bit"):
        streams[which] = READS[:n_reads_for(k, which)]
    n2 = n_reads_for(k, "two_slabs")
    streams["two_slabs"] = READS[:n2] + [(READS[n2] + READS[n2 + 1])[:2 * slab - 151 * n2 - 1]]      # exactly 2 slabs of positions
    e, keys = filter_engine(k, kmers, bins)
    with e:
        for name, reads in streams.items():
            st = ReadStream.from_strings(reads)
            if name == "one_tile":
                assert st.n_bases == 64
            if name == "two_slabs":
                assert st.n_bases == 2 * slab
            got, win = run_paths(e, keys, lambda: e.count_filtered(st), bins, f"k={k} bins={bins} {name}")
            want, want_win = expect(oracle, reads, k, kmers)
            assert np.array_equal(got, want), f"k={k} bins={bins} {name}: counts"
            assert win == want_win, f"k={k} bins={bins} {name}: windows"
            assert e.get_stat("last_sieve_slice_words") == 128


@pytest.mark.parametrize("k", (31, 63))
def test_few_windows_over_1024_bins(oracle, k):
    reads = [READS[1][:k + 49], READS[2][:k + 49]]                  # 100 windows: most bins and most runs are empty
    kmers = make_filter(oracle, k)
    e, keys = filter_engine(k, kmers, 10)
    with e:
        st = ReadStream.from_strings(reads)
        got, win = run_paths(e, keys, lambda: e.count_filtered(st), 10, f"k={k}")
        want, want_win = expect(oracle, reads, k, kmers)
        assert want_win <= 100 and np.array_equal(got, want) and win == want_win


@pytest.mark.parametrize("k,bins", ((31, 4), (31, 10), (63, 8)))
def test_long_runs_one_read_many_times_and_poly_a(oracle, k, bins):
    one = READS[3].upper().replace("N", "A")
    poly = "A" * 150
    kmers = sorted(set(all_counts(oracle, [one], k)) | {"A" * k}) + make_filter(oracle, k, seed=9, present=0, absent=200)
    kmers = list(dict.fromkeys(kmers))
    e, keys = filter_engine(k, kmers, bins)
    with e:
        for name, read, copies in (("copies", one, 20_000), ("poly_a", poly, 2_000)):
            st = ReadStream.from_strings([read] * copies)
            got, win = run_paths(e, keys, lambda: e.count_filtered(st), bins, f"k={k} {name}")
            c1, w1 = expect(oracle, [read], k, kmers)
            assert np.array_equal(got, c1 * np.uint32(copies)), f"k={k} {name}: counts"
            assert win == w1 * copies, f"k={k} {name}: windows"


@pytest.mark.parametrize("k", (31, 33))
def test_saturated_sieve_drains_all_the_time(oracle, k):
    rng = np.random.default_rng(5)
    present = make_filter(oracle, k, absent=0)
    noise = sorted({oracle.canonicalize(s) for s in rand_kmers(rng, 120_000, k)} - set(present))
    kmers = present + noise
    reads = READS[:240]
    e = KmerEngine(k, capacity_hint=1 << 12)
    with e:
        e.set_option("sieve_bits", 1)                              # 120 K keys on 16 x 128 words: most words are nearly full
        lo, hi = kmers_to_keys(kmers, k)
        e.load_filter(lo, hi)
        e.set_option("sieve_bins", 4)
        got, win = run_paths(e, (lo, hi), lambda: e.count_filtered(ReadStream.from_strings(reads)), 4, f"k={k}")
        assert e.get_stat("last_sieve_slice_words") == 128
        want, want_win = expect(oracle, 240, k, kmers)
        assert np.array_equal(got, want) and win == want_win


@pytest.mark.parametrize("k", (31, 63))
def test_several_passes_in_one_call(oracle, k):
    kmers = make_filter(oracle, k)
    e, keys = filter_engine(k, kmers, 8)
    with e:
        e.set_option("binned_max_positions", 6400)                 # 100 tiles per pass: passes end inside reads
        st = ReadStream.from_strings(READS[:200])
        p0 = e.get_stat("bin_sieve_passes")
        e.count_filtered(st)
        assert e.get_stat("last_count_path") == 5
        assert e.get_stat("bin_sieve_passes") - p0 == -(-st.n_bases // 6400) >= 4
        want, want_win = expect(oracle, 200, k, kmers)
        assert np.array_equal(e.query(*keys), want) and e.stats()[2] == want_win
        e.count_filtered(st)                                       # and two calls back to back
        assert np.array_equal(e.query(*keys), 2 * want) and e.stats()[2] == 2 * want_win


@pytest.mark.parametrize("k", (31, 33))
def test_dirty_words_at_and_past_n_bases(oracle, k):
    reads = READS[:60]
    tail = READS[300:303]                                          # what a longer stream goes on with
    codes, inv = layout(reads + tail)
    n = 60 * 151 - 37                                              # the cut lies inside the last read
    cut = cut_reads(reads, n)
    # the filter holds what a kernel that trusts the dirty words would find: the rest of the cut read, the reads behind it, poly-A
    phantom = sorted(set(oracle.py_count([reads[-1]] + tail, k)) | {"A" * k})
    kmers = list(dict.fromkeys(make_filter(oracle, k) + phantom))
    want, want_win = expect(oracle, cut, k, kmers)
    e, keys = filter_engine(k, kmers, 8)
    with e:
        for filling in ("clean", "zeros", "live", "prefix"):
            p, m = words(codes, inv, n, filling, seed=11)
            dp, dm = cpu(p).cuda(), cpu(m).cuda()
            torch.cuda.synchronize()
            e.reset_counts()
            w0 = e.stats()[2]
            e.count_filtered_dev(dp.data_ptr(), dm.data_ptr(), n)
            assert e.get_stat("last_count_path") == 5 and e.get_stat("last_sieve_bins") == 8
            assert np.array_equal(e.query(*keys), want), f"k={k} {filling}: counts"
            assert e.stats()[2] - w0 == want_win, f"k={k} {filling}: windows"


@pytest.mark.parametrize("k", (31, 63))
def test_sieve_lifetime(oracle, k):
    reads = READS[:120]
    st = ReadStream.from_strings(reads)
    have = sorted(all_counts(oracle, 120, k))
    kmers, late, other = have[0:400:2], have[401], have[1:400:2]
    e, keys = filter_engine(k, kmers, 8, reserve=0)
    with e:
        base = e.count_filtered(st).get_stat("last_count_path")     # sieve_bins 8 is on: 5
        assert base == 5
        want, want_win = expect(oracle, 120, k, kmers)
        assert np.array_equal(e.query(*keys), want)
        # a key joins the table in filter mode: the sieve is rebuilt and the new key is counted
        llo, lhi = kmers_to_keys([late], k)
        e.add_pairs(llo, lhi, np.zeros(1, np.uint32))
        e.count_filtered(st)
        assert e.get_stat("last_count_path") == 5
        assert e.query(llo, lhi)[0] == all_counts(oracle, 120, k)[late]
        assert np.array_equal(e.query(*keys), 2 * want)
        # reset_counts and a rehash keep it (a rehash keeps h)
        e.reset_counts()
        e.reserve(1 << 15)
        assert e.get_stat("log2cap") >= 16
        e.count_filtered(st)
        assert e.get_stat("last_count_path") == 5
        assert np.array_equal(e.query(*keys), want) and e.query(llo, lhi)[0] == all_counts(oracle, 120, k)[late]
        # another filter replaces it
        olo, ohi = kmers_to_keys(other, k)
        e.load_filter(olo, ohi)
        e.count_filtered(st)
        assert e.get_stat("last_count_path") == 5
        assert np.array_equal(e.query(olo, ohi), expect(oracle, 120, k, other)[0])
        assert not e.query(*keys).any()
        # the option back to 0: the path the engine takes without it
        e.set_option("sieve_bins", 0)
        e.reset_counts()
        e.count_filtered(st)
        off_path = e.get_stat("last_count_path")
        assert off_path == 3                                        # (a small filter: the L2 / LDS sieve)
        assert np.array_equal(e.query(olo, ohi), expect(oracle, 120, k, other)[0])
        # clear drops it: count --if needs a filter again, and the next one gets a sieve of its own
        e.set_option("sieve_bins", 1)
        e.clear()
        with pytest.raises(KdfError):
            e.count_filtered(st)
        e.load_filter(*keys)
        e.count_filtered(st)
        assert e.get_stat("last_count_path") == 5 and e.get_stat("last_sieve_bins") == 4
        assert np.array_equal(e.query(*keys), want) and e.stats()[2] == want_win


def test_pending_binned_passes_then_bin_sieve(oracle):
    k = 31
    kmers = make_filter(oracle, k)
    st = ReadStream.from_strings(READS[:200])
    e, keys = filter_engine(k, kmers, 8)
    with e:
        e.set_option("force_path", 2)
        e.count_filtered(st)                                       # binned, deferred
        assert e.get_stat("last_count_path") == 1 and e.get_stat("pending_passes") >= 1
        e.set_option("force_path", 0)                              # (an option change applies what is pending)
        e.count_filtered(st)
        assert e.get_stat("last_count_path") == 5 and e.get_stat("pending_passes") == 0
        want, want_win = expect(oracle, 200, k, kmers)
        assert np.array_equal(e.query(*keys), 2 * want) and e.stats()[2] == 2 * want_win


@pytest.mark.parametrize("k", (31, 63))
def test_uploaded_batches_and_spool_replay_take_the_path(oracle, k):
    kmers = make_filter(oracle, k)
    st = ReadStream.from_strings(READS[:150])
    want, want_win = expect(oracle, 150, k, kmers)
    e, keys = filter_engine(k, kmers, 10)
    with e:
        e.upload_async(0, st)
        e.count_uploaded(0, filtered=True)
        assert e.get_stat("last_count_path") == 5 and e.get_stat("last_sieve_bins") == 10
        assert np.array_equal(e.query(*keys), want) and e.stats()[2] == want_win
        e.reset_counts()
        e.set_option("force_path", 1)                              # (last_count_path away from 5)
        e.count_filtered(st)
        e.set_option("force_path", 0)
        e.reset_counts()
        w0 = e.stats()[2]
        with ReadSpool(0, 1 << 28, 0) as sp:
            sp.set_option("segment_positions", 1 << 13)            # several segments: one count --if per segment
            sp.append(st, keep_reads=False)
            sp.replay(e, 1)
        assert e.get_stat("last_count_path") == 5
        assert np.array_equal(e.query(*keys), want) and e.stats()[2] - w0 == want_win


def test_refusals_and_ignored_cases(oracle):
    with KmerEngine(101, capacity_hint=1 << 10) as e:              # a long engine refuses the option
        for v in (1, 4, 10):
            with pytest.raises(KdfError):
                e.set_option("sieve_bins", v)
        e.set_option("sieve_bins", 0)
        assert e.get_stat("sieve_bins") == 0
    k = 31
    kmers = make_filter(oracle, k)
    lo, hi = kmers_to_keys(kmers, k)
    st = ReadStream.from_strings(READS[:50])
    want, want_win = expect(oracle, 50, k, kmers)
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        for v in (2, 3, 11, -1):
            with pytest.raises(KdfError):
                e.set_option("sieve_bins", v)
        assert e.get_stat("sieve_bins") == 0
        with pytest.raises(KdfError):
            e.set_option("force_path", 3)
        e.set_option("hash_shift", 2)                              # an owner table: the option is ignored
        e.load_filter(lo, hi)
        e.count_filtered(st)
        before = e.get_stat("last_count_path")
        e.reset_counts()
        e.set_option("sieve_bins", 8)
        e.count_filtered(st)
        assert e.get_stat("last_count_path") == before != 5
        assert e.get_stat("bin_sieve_passes") == 0
        assert np.array_equal(e.query(lo, hi), want)
