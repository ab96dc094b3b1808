"""Full-size counts, key by key, against a truth that shares no code with the engine (tests/stream_truth.py: torch
sorts over the packed stream words; pinned to the oracle on the CPU by tests/test_stream_truth.py).

Every comparison is exact and covers EVERY key: ``torch.equal`` on the sorted dump's lo, hi and ``counts &
0xFFFFFFFF`` against the truth's rows, and the window total.  Every case also asserts a witness from ``kdf_get_stat``
(``last_count_path``, ``binned_passes``, ``flushes``, ``pending_passes``, ``heavy_buckets``) that the path it names
is the path that ran.

  a  configs[1]: 10 M x 150 bp, k = 31, the exact bench seeds; direct, binned, auto + flush; histogram, dump -L 3
  b  configs[4]: the same reads at k = 63; binned, direct
  c  the product's shape: the eight batches of ``bench.py --scaling strong --batches 8`` deferred into ONE table
  d  one count call of 4.53 G positions (30 M reads, past 2^32), and one of just over 2^31
  e  the parent-filter chain at 64 Mbp, 30x: exact sets, and per-key ``count --if`` counts of the candidates
  f  the repeat-rich genome of test_gpu_skew.py: binned (a heavy bucket is split) and direct

Workloads are built once (``workloads``: the streams and their truths) and dropped before the next one is built.
Jobs whose windows exceed one torch.sort (2^31 elements) are counted batch by batch -- sub-streams cut at a tile
boundary between reads -- and compared with the dump in S key slices (``stream_truth.slice_of``); S is chosen so that
the largest slice (the first: ~1 - (1 - 1/S)^2 of the rows) sorts within a few tens of GB next to the engine's table,
ring and dump (DESIGN.md section 6 has the measured figures)."""
import os
import sys
import time

import numpy as np
import pytest

import stream_truth as ST

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# configs[1]: what the 16-core oracle counted for the whole bench batch (BENCH_r01.json cpu_baseline)
BENCH_WINDOWS, BENCH_DISTINCT, BENCH_GE3 = 1_163_397_354, 266_204_130, 99_718_792
SLICES_C, SLICES_D = 8, 4


def timed_truth(label, stream, k, **kw):
    """count_truth with its seconds and peak bytes printed (pytest -s shows them)"""
    import torch
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    t = ST.count_truth(stream, k, **kw)
    torch.cuda.synchronize()
    dt, peak = time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base
    print(f"[truth] {label}: k={k} valid_windows={t[3]} rows={t[0].numel()} seconds={dt:.2f} peak_bytes={peak} "
          f"peak_bytes_per_valid_window={peak / max(t[3], 1):.1f}", flush=True)
    torch.cuda.empty_cache()                                # (the sort's buffers go back to the device: the engine allocates beside torch)
    return t


class Workloads:
    """one workload (streams + truths) alive at a time"""

    def __init__(self):
        self.name, self.value = None, None

    def get(self, name, build):
        import torch
        if self.name != name:
            self.name, self.value = None, None
            torch.cuda.empty_cache()
            self.value = build()
            self.name = name
        return self.value

    def drop(self):
        import torch
        self.name, self.value = None, None
        torch.cuda.empty_cache()


WORKLOADS = Workloads()                                     # (tests/test_gpu_configs.py builds the parent-filter workload first and leaves it here)


@pytest.fixture(scope="module")
def workloads():
    yield WORKLOADS
    WORKLOADS.drop()


def bench_stream(batch=0, reads=10_000_000):
    """batch b of the bench job: bench.py run_count's seeds"""
    import torch
    from kmer_denovo_filter_amd.synth import synth_stream
    ds = synth_stream(reads, 150, 100_000_000, seed=20260417 + 1000 * batch, device=DEV, genome_seed=20260417)
    torch.cuda.synchronize()
    return ds


def engine(k, hint):
    """a new engine, after torch's cached blocks went back to the device (the engine allocates beside torch)"""
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    torch.cuda.empty_cache()
    return KmerEngine(k, capacity_hint=hint)


def count(e, ds, n_bases=None):
    e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases if n_bases is None else n_bases)


def sorted_dump(e, min_count, n):
    """ascending (lo, hi, counts as int64 in 0 .. 2^32 - 1) of the table's entries with count >= min_count"""
    import torch
    lo = torch.empty(n, dtype=torch.int64, device=DEV)
    hi = torch.empty(n, dtype=torch.int64, device=DEV) if e.wide else None
    cnt = torch.empty(n, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    got = e.export_ge_dev(min_count, lo.data_ptr(), hi.data_ptr() if e.wide else None, cnt.data_ptr(), n, sorted_=True)
    e.synchronize()
    assert got == n, f"dump -L {min_count}: {got} entries, expected {n}"
    if hi is None:
        hi = torch.zeros(n, dtype=torch.int64, device=DEV)
    return lo, hi, cnt.to(torch.int64) & 0xFFFFFFFF


def assert_rows_equal(got, want, what):
    import torch
    for name, g, w in zip(("lo", "hi", "counts"), got, want):
        assert g.numel() == w.numel(), f"{what}: {g.numel()} rows, the truth has {w.numel()}"
        assert torch.equal(g, w), f"{what}: {name} differs from the truth in {int((g != w).sum())} of {g.numel()} rows"


def assert_table_equals_truth(e, truth, what, min_counts=(0,)):
    """stats, count_ge and the sorted dump(s) of a flushed engine against a whole truth (lo, hi, counts, windows)"""
    cap, distinct, windows = e.stats()
    assert windows == truth[3], f"{what}: {windows} windows, the truth has {truth[3]}"
    assert distinct == truth[0].numel(), f"{what}: {distinct} distinct keys, the truth has {truth[0].numel()}"
    for m in min_counts:
        want = truth[:3] if m == 0 else ST.rows_ge(truth, m)
        assert e.count_ge(m) == want[0].numel(), f"{what}: count_ge({m})"
        got = sorted_dump(e, m, want[0].numel())
        assert_rows_equal(got, want, f"{what}: dump -L {m}")
        if m == 0:
            assert int(got[2].sum().item()) == windows, f"{what}: sum of the counts != windows"
        del got


# ---------------------------------------------------------------------------------------------------------------------
# e: the parent-filter chain (first: its workload is the one tests/test_gpu_configs.py leaves behind)
# ---------------------------------------------------------------------------------------------------------------------

def _parent_filter():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "benchmarks"))
    import parent_filter
    res, keys, streams = parent_filter.run(64_000_000, 30, 31, 20260418, DEV)
    T = {name: timed_truth(f"parent filter {name}", streams[name], 31) for name in ("ref", "child", "mother", "father")}
    return res, keys, streams, T


def assert_chain_equals_truth(res, keys, T):
    """The sets of the discovery chain from the truths of the four streams -- candidates (child >= 3), minus the
    reference's keys, minus the keys the mother has, minus the keys the father has -- against the chain's sizes and
    the keys it returned.  -> the candidate rows (lo, hi, counts)."""
    import torch
    lo, hi = keys
    cand = ST.rows_ge(T["child"], 3)
    non_ref = ST.keys_minus(cand[:2], T["ref"])
    m = ST.filtered_truth(T["mother"], non_ref)
    after_mother = (non_ref[0][m <= 0], non_ref[1][m <= 0])
    f = ST.filtered_truth(T["father"], after_mother)
    after_father = (after_mother[0][f <= 0], after_mother[1][f <= 0])
    assert res["child_windows"] == T["child"][3] and res["child_distinct"] == T["child"][0].numel()
    assert (res["candidates"], res["non_ref"], res["after_mother"], res["after_father"], res["proband_unique"]) == \
        (cand[0].numel(), non_ref[0].numel(), after_mother[0].numel(), after_father[0].numel(), after_father[0].numel())
    assert res["stages"]["mother_count_if"]["windows"] == T["mother"][3] and res["stages"]["father_count_if"]["windows"] == T["father"][3]
    assert res["stages"]["mother_count_if"]["filter_keys"] == non_ref[0].numel()
    assert res["stages"]["father_count_if"]["filter_keys"] == after_mother[0].numel()
    # the returned keys (the chain keeps the dump's order: compared as a sorted set; no key twice)
    assert hi is None or not np.any(hi)
    got = torch.from_numpy(np.ascontiguousarray(lo).view(np.int64)).to(DEV)
    got = torch.sort(got ^ ST.SIGN).values ^ ST.SIGN
    assert got.numel() == after_father[0].numel() and torch.equal(got, after_father[0])
    assert 0 < after_father[0].numel() < after_mother[0].numel() < non_ref[0].numel() < cand[0].numel()
    return cand


def test_e_parent_filter_chain_exact_sets(workloads):
    """benchmarks/parent_filter.run at 64 Mbp, 30x: candidates (child >= 3), non-reference, after-mother and
    after-father computed from the truths of the four streams; the chain's sizes and its surviving keys must be
    those.  Then the CANDIDATES as the filter (64 M keys, most of them genome k-mers that the mother has too): the
    mother's per-key ``count --if`` counts on the sieve (8 bits per key: by default a filter of this size gets none),
    binned and direct paths against ``filtered_truth``.  (Defined first: the workload is the one that
    tests/test_gpu_configs.py::test_config2_parent_filter_chain_full_64mbp has just built.)"""
    import torch
    res, keys, streams, T = workloads.get("parent filter", _parent_filter)
    cand = assert_chain_equals_truth(res, keys, T)
    # count --if of the candidates over the mother's reads
    flo = cand[0].contiguous()
    want = ST.filtered_truth(T["mother"], (flo, cand[1]))
    assert int((want > 0).sum().item()) > flo.numel() // 2       # most candidates are genome k-mers: the mother has them
    mother = streams["mother"]
    for name, path, last in (("sieve", 4, "sieve"), ("binned", 2, "binned"), ("direct", 1, "direct")):
        with engine(31, flo.numel()) as e:
            if path == 4:
                e.set_option("sieve_bits", 8)
            e.load_filter_dev(flo.data_ptr(), None, flo.numel())
            e.set_option("force_path", path)
            e.count_filtered_dev(mother.packed.data_ptr(), mother.invalid.data_ptr(), mother.n_bases)
            assert e.last_count_path() == last, name
            if path == 2:
                assert e.get_stat("binned_passes") == 1
            else:
                assert e.get_stat("binned_passes") == 0
            q = torch.empty(flo.numel(), dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            e.query_dev(flo.data_ptr(), None, flo.numel(), q.data_ptr()); e.synchronize()
            got = q.to(torch.int64) & 0xFFFFFFFF
            assert torch.equal(got, want), f"count --if, {name}: {int((got != want).sum())} of {flo.numel()} counts differ from the truth"
            assert e.stats()[2] == T["mother"][3]
            if path == 2:
                assert e.get_stat("flushes") == 1


# ---------------------------------------------------------------------------------------------------------------------
# a / b: the bench batch at k = 31 and k = 63
# ---------------------------------------------------------------------------------------------------------------------

def _bench_batch(k):
    ds = bench_stream()
    return ds, timed_truth("configs bench batch 10 M x 150 bp", ds, k)


PATHS = {"direct": 1, "binned": 2, "auto": 0}


def run_bench_path(e, ds, path):
    """count ``ds`` into ``e`` on the named path and assert the witnesses that it was that path"""
    e.set_option("force_path", PATHS[path])
    count(e, ds)
    passes = (ds.n_bases + (1 << 31) - 1) >> 31           # binned_max_positions: 2^31 positions per partition pass
    if path == "direct":
        assert e.last_count_path() == "direct"
        assert (e.get_stat("binned_passes"), e.get_stat("pending_passes"), e.get_stat("flushes")) == (0, 0, 0)
    else:                                                   # partitioned now, applied by the flush (defer is the default)
        assert e.get_stat("defer") == 1
        assert e.last_count_path() == "binned"
        assert e.get_stat("binned_passes") == passes
        if passes == 1:
            assert (e.get_stat("pending_passes"), e.get_stat("flushes")) == (1, 0)
        else:                                               # (a pass that finds the ring full applies the earlier ones first)
            assert 0 < e.get_stat("pending_passes") <= passes
        before = e.get_stat("flushes")
        e.flush()
        assert (e.get_stat("binned_passes"), e.get_stat("pending_passes"), e.get_stat("flushes")) == (passes, 0, before + 1)


@pytest.mark.parametrize("path", ["direct", "binned", "auto"])
def test_a_config1_bench_batch_every_key(workloads, path):
    """configs[1] (10 M x 150 bp, k = 31, the bench seeds): the truth reproduces the totals of the 16-core oracle run,
    and every path's sorted dump, its -L 3 dump and its histogram are the truth's."""
    import torch
    ds, truth = workloads.get("bench k=31", lambda: _bench_batch(31))
    assert (truth[3], truth[0].numel(), int((truth[2] >= 3).sum().item())) == (BENCH_WINDOWS, BENCH_DISTINCT, BENCH_GE3)
    assert not bool(truth[1].any()) and int(truth[2].sum().item()) == truth[3]
    with engine(31, 1 << 28) as e:
        run_bench_path(e, ds, path)
        assert_table_equals_truth(e, truth, path, min_counts=(0, 3))
        high = 255
        bins = torch.bincount(truth[2].clamp(max=high + 1), minlength=high + 2)
        assert np.array_equal(e.histogram(high).astype(np.int64), bins.cpu().numpy()), f"{path}: histogram({high})"
        assert int(bins[0]) == 0 and int(bins.sum()) == truth[0].numel()


@pytest.mark.parametrize("path", ["binned", "direct"])
def test_b_config4_k63_every_key(workloads, path):
    """configs[4]: the same reads at k = 63 (128-bit keys), all of them."""
    ds, truth = workloads.get("bench k=63", lambda: _bench_batch(63))
    assert bool((truth[1] > 0).any()) and bool((truth[0] < 0).any())      # both words in use, lo on both sides of the sign bit
    with engine(63, 1 << 28) as e:
        run_bench_path(e, ds, path)
        assert_table_equals_truth(e, truth, path, min_counts=(0, 3))


# ---------------------------------------------------------------------------------------------------------------------
# c / d: jobs of several batches, compared in key slices
# ---------------------------------------------------------------------------------------------------------------------

def assert_dump_equals_batches_in_slices(dump, parts, k, S, what, min_count=0):
    """``dump``: ascending (lo, hi, counts) of a table; ``parts``: the truths of the batches counted into it.  Slice by
    slice of the key space: the batches' rows of the slice are accumulated and compared with the dump's rows of the slice.
    -> (distinct, sum of counts, keys with count >= 3) of the accumulated truth."""
    import torch
    sl = ST.slice_of(dump[0], dump[1], k, S)
    assert bool((sl[1:] >= sl[:-1]).all()), f"{what}: the dump is not ascending"
    distinct = total = ge3 = 0
    for s in range(S):
        acc = ST.accumulate([ST.take_slice(p, k, s, S) for p in parts])
        distinct += acc[0].numel(); total += int(acc[2].sum().item()); ge3 += int((acc[2] >= 3).sum().item())
        want = ST.rows_ge(acc, min_count) if min_count else acc
        keep = sl == s
        assert_rows_equal(tuple(x[keep] for x in dump), want, f"{what}: key slice {s} of {S}")
        del acc, want, keep
    return distinct, total, ge3


def _strong8():
    import torch
    streams, truths = [], []
    for b in range(8):
        ds = bench_stream(b)
        streams.append(ds)
        truths.append(timed_truth(f"strong-8 batch {b}", ds, 31))
    return streams, truths


def strong8_hint(n_batches=8):
    per_batch = 1 << 28                                     # bench.py run_count: reads >= 5 M
    return int(per_batch * (0.4 + 0.62 * n_batches))


@pytest.mark.parametrize("fused", [0, 1])
def test_c_strong8_batches_deferred_into_one_table(workloads, fused):
    """The job of ``bench.py --scaling strong --batches 8`` on one GPU: eight 10 M-read batches (seeds 20260417 +
    1000 b, one genome) counted into ONE engine on the auto path, every batch partitioned into the ring of pending
    passes and applied by the flush.  fused = 0: ``flush()``, then the whole sorted dump in key slices.  fused = 1: the
    ``-L 3`` dump is asked for while the passes are pending and is written by the flush itself (or, when the engine
    falls back -- ``fused_dumps == 0`` -- by the table pass): the truth's rows with count >= 3, in key slices."""
    import torch
    streams, truths = workloads.get("strong-8", _strong8)
    want_windows = sum(t[3] for t in truths)
    if fused:                                                # the size of the -L 3 dump, from the truth
        n3 = sum(int((ST.accumulate([ST.take_slice(t, 31, s, SLICES_C) for t in truths])[2] >= 3).sum().item()) for s in range(SLICES_C))
    with engine(31, strong8_hint()) as e:
        e.set_option("fused_dump", fused)
        for ds in streams:
            count(e, ds)
        assert e.last_count_path() == "binned"
        assert e.get_stat("binned_passes") == 8 and 0 < e.get_stat("pending_passes") <= 8
        before = e.get_stat("flushes")                       # (a new engine's ring grows as the batches come: a pass that finds it full applies the earlier ones)
        print(f"[engine] strong-8 pending: pending_passes={e.get_stat('pending_passes')} flushes={before} ring_bytes={e.get_stat('ring_bytes')} log2cap={e.get_stat('log2cap')}", flush=True)
        if fused:
            dump = sorted_dump(e, 3, n3)                     # asked for with the eight passes pending
            assert e.get_stat("fused_dumps") in (0, 1)
            print(f"[engine] strong-8 fused_dumps={e.get_stat('fused_dumps')} heavy_buckets={e.get_stat('heavy_buckets')}", flush=True)
        else:
            e.flush()
        assert (e.get_stat("pending_passes"), e.get_stat("flushes"), e.get_stat("binned_passes")) == (0, before + 1, 8)
        cap, distinct, windows = e.stats()
        assert windows == want_windows
        if not fused:
            dump = sorted_dump(e, 0, distinct)
        ge3 = e.count_ge(3)
        print(f"[engine] strong-8: log2cap={e.get_stat('log2cap')} distinct={distinct} windows={windows} ge3={ge3}", flush=True)
    torch.cuda.empty_cache()                                # (the engine's table and ring are gone: the slices sort in their place)
    t_distinct, t_total, t_ge3 = assert_dump_equals_batches_in_slices(dump, truths, 31, SLICES_C, f"strong-8 fused={fused}", min_count=3 if fused else 0)
    assert (distinct, windows, ge3) == (t_distinct, t_total, t_ge3)
    if not fused:
        assert int(dump[2].sum().item()) == windows
    print(f"[truth] strong-8: distinct={t_distinct} windows={t_total} ge3={t_ge3}", flush=True)


BIG_READS = 30_000_000                                      # x 151 = 4.53 G positions in one stream
PIECE_READS = 10_000_000                                    # x 151 positions = a whole number of 64-position tiles
OVER_2_31_READS = 14_222_336                                # x 151 = 2 147 572 736 positions = 2^31 + 89 088; a multiple of 64 reads


def _sub_stream(ds, first_read, n_reads):
    """reads [first_read, first_read + n_reads) of a stream as a stream of their own (first_read * 151 must be a
    multiple of 64: the words are then shared, not copied)"""
    off, n = first_read * (ds.read_len + 1), n_reads * (ds.read_len + 1)
    assert off % 64 == 0
    return ds.packed[off // 32:], ds.invalid[off // 64:], n


def _big_stream():
    ds = bench_stream(reads=BIG_READS)
    assert ds.n_bases > 1 << 32
    truths = [timed_truth(f"30 M-read stream, reads {a} ..", _sub_stream(ds, a, PIECE_READS), 31) for a in range(0, BIG_READS, PIECE_READS)]
    return ds, truths


@pytest.mark.parametrize("path", ["auto", "direct"])
def test_d_one_call_past_2_32_positions(workloads, path):
    """ONE ``count_dev`` of 4.53 G positions (30 M x 150 bp, 1.1 GB of packed words): positions, cursors and window
    totals past 32 bits.  The truth is built from three 10 M-read pieces of the same words and compared in key slices."""
    import torch
    ds, truths = workloads.get("30 M reads", _big_stream)
    with engine(31, 1 << 30) as e:
        run_bench_path(e, ds, path)                          # (auto: three partition passes of at most 2^31 positions)
        cap, distinct, windows = e.stats()
        assert windows == sum(t[3] for t in truths) and windows > 1 << 31
        dump = sorted_dump(e, 0, distinct)
        ge3 = e.count_ge(3)
        print(f"[engine] 30 M reads {path}: log2cap={e.get_stat('log2cap')} distinct={distinct} windows={windows}", flush=True)
    torch.cuda.empty_cache()
    t = assert_dump_equals_batches_in_slices(dump, truths, 31, SLICES_D, f"30 M reads, {path}")
    assert (distinct, windows, ge3) == t and int(dump[2].sum().item()) == windows


def _check_prefix(ds, n, what):
    """one count_dev of the stream's first n positions, on auto and direct, against the truth of that prefix"""
    import torch
    prefix = (ds.packed, ds.invalid, n)
    halves = [timed_truth(f"{what}, key slice {s} of 2", prefix, 31, key_slice=(s, 2)) for s in range(2)]
    assert halves[0][3] == halves[1][3]
    truth = tuple(torch.cat([h[i] for h in halves]) for i in range(3)) + (halves[0][3],)
    del halves
    for path in ("auto", "direct"):
        with engine(31, 1 << 29) as e:
            e.set_option("force_path", PATHS[path])
            count(e, ds, n)
            if path == "auto":
                assert e.last_count_path() == "binned" and e.get_stat("binned_passes") == 2 and 0 < e.get_stat("pending_passes") <= 2
                before = e.get_stat("flushes")
                e.flush()
                assert e.get_stat("flushes") == before + 1 and e.get_stat("pending_passes") == 0
            else:
                assert e.last_count_path() == "direct" and e.get_stat("binned_passes") == 0
            assert_table_equals_truth(e, truth, f"{what}, {path}")
    return truth[3]


def test_d_one_call_just_over_2_31_positions(workloads):
    """The first 14 222 336 reads of the same stream (2^31 + 89 088 positions: two partition passes, the second one
    tiny), against a truth taken key slice by key slice over the whole prefix.  Then a prefix that is cut in the MIDDLE
    of the next read, 75 bases in, with n % 64 != 0: the words past it are the rest of the stream (valid bases, mask
    bits 0), and no window may reach into them (include/kdf.h, "Read streams")."""
    ds, _ = workloads.get("30 M reads", _big_stream)
    n = OVER_2_31_READS * 151
    assert (1 << 31) < n < (1 << 31) + (1 << 17) and n % 64 == 0
    aligned = _check_prefix(ds, n, "2^31 prefix")
    n2 = n + 75
    assert n2 % 64 != 0 and n2 % 151 == 75 and ds.read_len == 150
    cut = _check_prefix(ds, n2, "2^31 prefix cut inside a read")
    assert aligned <= cut <= aligned + 75 - 31 + 1             # the cut read adds at most its 45 whole windows


# ---------------------------------------------------------------------------------------------------------------------
# f: skewed input
# ---------------------------------------------------------------------------------------------------------------------

def _repeat_rich(k):
    import torch
    from kmer_denovo_filter_amd.synth import synth_stream
    from test_gpu_skew import _repeat_rich_genome
    g = torch.from_numpy(_repeat_rich_genome(np.random.default_rng(7), 3_000_000)).to(DEV)
    ds = synth_stream(300_000, 150, seed=11, device=DEV, genome=g)
    torch.cuda.synchronize()
    return ds, timed_truth("repeat-rich 300 k reads", ds, k)


@pytest.mark.parametrize("k", [31, 63])
def test_f_repeat_rich_genome_every_key(workloads, k):
    """300 k reads of the 3 Mbp repeat-rich genome of test_gpu_skew.py (Alu-like copies, microsatellites, poly-A):
    the binned path -- which must split a heavy bucket over several workgroups -- and the direct path."""
    ds, truth = workloads.get(f"repeat-rich k={k}", lambda: _repeat_rich(k))
    assert int(truth[2].max().item()) > 2000                   # the microsatellite k-mers are heavy hitters
    for path in ("binned", "direct"):
        with engine(k, 1 << 24) as e:
            run_bench_path(e, ds, path)
            heavy = e.get_stat("heavy_buckets")
            print(f"[engine] repeat-rich k={k} {path}: heavy_buckets={heavy}", flush=True)
            assert (heavy > 0) == (path == "binned"), f"{path}: heavy_buckets = {heavy}"
            assert_table_equals_truth(e, truth, f"repeat-rich k={k}, {path}", min_counts=(0, 3))
