"""The count histogram and the table statistics of the live table (`jellyfish histo` / `jellyfish stats`:
kdf_histogram, kdf_histogram_dev, kdf_count_stats) against numpy.bincount of the oracle's dump (k <= 63) and of
tests/kmer_truth.count_truth (long k): every key width, skewed and saturated counts, filter mode, deferred count
passes, growth, key-space slices, owner tables, and two ranks over gloo."""
import socket

import numpy as np
import pytest

import kmer_truth as KT

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF


def bins_of(counts, high):
    """numpy.bincount with everything above `high` in bin high + 1."""
    c = np.minimum(np.asarray(counts, dtype=np.uint64), np.uint64(high + 1)).astype(np.int64)
    return np.bincount(c, minlength=high + 2).astype(np.uint64)


def stats_of(counts):
    c = np.asarray(counts, dtype=np.uint64)
    return {"unique": int((c == 1).sum()), "distinct": int((c >= 1).sum()), "total": int(c.sum(dtype=np.uint64)),
            "max_count": int(c.max()) if len(c) else 0}


def highs_for(counts):
    mx = int(max(counts)) if len(counts) else 0
    return sorted({0, 1, 3, 10000, mx + 1, max(0, mx - 1), max(0, mx // 2)})


def check_engine(e, counts, highs=None, tag=""):
    """Host and device forms for several `high`, the two invariants with count_ge, count_stats."""
    import torch
    counts = np.asarray(counts, dtype=np.uint64)
    for high in highs if highs is not None else highs_for(counts):
        want = bins_of(counts, high)
        got = e.histogram(high)
        assert got.dtype == np.uint64 and got.shape == (high + 2,)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{tag} high={high}: bins {bad[:8]} got {got[bad[:8]]} want {want[bad[:8]]}"
        d = torch.full((high + 2,), -7, dtype=torch.int64, device="cuda:0")   # stale contents must not survive
        torch.cuda.synchronize()
        e.histogram_dev(high, d.data_ptr())
        assert np.array_equal(d.cpu().numpy().view(np.uint64), got), f"{tag} high={high}: _dev differs from the host form"
        assert int(got.sum()) == e.count_ge(0) == len(counts), f"{tag} high={high}"
        for m in sorted({0, 1, 2, 3, high, high + 1} & set(range(high + 2))):
            assert int(got[m:].sum()) == e.count_ge(m) == int((counts >= m).sum()), f"{tag} high={high} m={m}"
    assert e.count_stats() == stats_of(counts), tag


def trio_child(trio_reads):
    return trio_reads["child"]


def synth_reads(n_reads=1500, genome_len=20_000, seed=11):
    """A synth batch (the bench workload's generator) deep enough that most k-mers repeat."""
    import torch
    from kmer_denovo_filter_amd.synth import stream_to_ascii, synth_stream
    ds = synth_stream(n_reads, 150, genome_len, seed=seed, device="cuda:0")
    torch.cuda.synchronize()
    chars, offs = stream_to_ascii(ds, n_reads)
    return ds, [chars[offs[i]:offs[i + 1]].tobytes().decode() for i in range(n_reads)]


@pytest.mark.parametrize("k", [15, 31, 33, 63])
def test_histogram_matches_oracle_trio_child(oracle, trio_reads, k):
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    reads = trio_child(trio_reads)
    _, _, cnt = oracle.OracleTable(k).count_reads(reads).export_ge(0)
    with KmerEngine(k, capacity_hint=1 << 20) as e:
        e.count(ReadStream.from_strings(reads))
        check_engine(e, cnt, tag=f"trio k={k}")
        assert np.array_equal(e.histogram(), bins_of(cnt, 10000))            # the default high


@pytest.mark.parametrize("k", [15, 31, 33, 63])
def test_histogram_matches_oracle_synth_with_repeats(oracle, k):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    ds, reads = synth_reads()
    _, _, cnt = oracle.OracleTable(k).count_reads(reads).export_ge(0)
    assert int(cnt.max()) > 8                                                 # deep: the LDS bins are used
    with KmerEngine(k, capacity_hint=1 << 16) as e:
        torch.cuda.synchronize()
        e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
        check_engine(e, cnt, tag=f"synth k={k}")


@pytest.mark.parametrize("k", [75, 101, 201])
def test_histogram_long_k_matches_truth(k):
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    rng = np.random.default_rng(k)
    reads = KT.random_reads(rng, k, 300)
    truth = KT.count_truth(reads, k)
    cnt = np.array(list(truth.values()), dtype=np.uint64)
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        e.count(ReadStream.from_strings(reads))
        assert e.count_ge(0) == len(truth)
        check_engine(e, cnt, tag=f"long k={k}")


def _random_keys(rng, k, n):
    """n distinct canonical keys as python ints."""
    M = (1 << (2 * k)) - 1
    out = set()
    while len(out) < n:
        v = int.from_bytes(rng.bytes((2 * k + 7) // 8), "little") & M
        rc, x = 0, v ^ M                                     # reverse complement: complement, then reverse the 2-bit groups
        for _ in range(k):
            rc = (rc << 2) | (x & 3); x >>= 2
        out.add(min(v, rc))
    return sorted(out)


def _add(e, k, keys, counts):
    counts = None if counts is None else np.asarray(counts, dtype=np.uint32)
    if k > 63:
        e.add_pairs(KT.rows(keys, (2 * k + 63) // 64), None, counts)
    else:
        lo, hi = KT.lohi(keys)
        e.add_pairs(lo, hi if k > 32 else None, counts)


@pytest.mark.parametrize("k", [31, 63, 101])
def test_skewed_tables(k):
    """> 99 % of the keys at count 1 (the register tallies), and every key at the same large count (every lane of
    every wave on one bin: LDS, global and overflow)."""
    from kmer_denovo_filter_amd import KmerEngine
    rng = np.random.default_rng(3 * k)
    keys = _random_keys(rng, k, 40_000)
    c = np.ones(len(keys), np.uint32)
    c[rng.choice(len(keys), 200, replace=False)] = rng.choice(np.array([2, 3, 4, 5, 100, 4095, 4096, 9999, 10000, 10001, 70000]), 200)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        _add(e, k, keys, c)
        check_engine(e, c, highs=[0, 1, 3, 4, 4095, 4096, 10000, 70001], tag=f"99% ones k={k}")
    for same in (1000, 5000, 3):
        c = np.full(len(keys), same, np.uint32)
        with KmerEngine(k, capacity_hint=1 << 16) as e:
            _add(e, k, keys, c)
            check_engine(e, c, highs=[0, 2, 3, same - 1, same, same + 1, 10000], tag=f"all {same} k={k}")


@pytest.mark.parametrize("k", [31, 63, 101])
def test_zero_counts_and_saturation(k):
    """Pairs added with counts 2^32 - 1 and 2^32 - 2 twice saturate; keys added with a NULL / zero count are in bin 0."""
    from kmer_denovo_filter_amd import KmerEngine
    rng = np.random.default_rng(5 * k)
    keys = _random_keys(rng, k, 3000)
    c = rng.integers(1, 50, len(keys)).astype(np.uint32)
    c[:100] = U32; c[100:200] = U32 - 1; c[200:300] = 0
    with KmerEngine(k, capacity_hint=1 << 13) as e:
        _add(e, k, keys, c)
        _add(e, k, keys, c)
        stored = np.minimum(c.astype(np.uint64) * 2, U32)
        assert int((stored == U32).sum()) == 200 and int((stored == 0).sum()) == 100
        check_engine(e, stored, highs=[0, 1, 3, 98, 10000, (1 << 20) - 1], tag=f"saturated k={k}")
        st = e.count_stats()
        assert st["max_count"] == U32 and st["total"] == int(stored.sum(dtype=np.uint64)) > 200 * U32 - 1
        assert int(e.histogram(0)[0]) == 100
    with KmerEngine(k, capacity_hint=1 << 13) as e:          # NULL counts: plain insertion, everything in bin 0
        _add(e, k, keys, None)
        check_engine(e, np.zeros(len(keys), np.uint64), highs=[0, 5], tag=f"null counts k={k}")


@pytest.mark.parametrize("k", [31, 47])
def test_filter_mode_keeps_the_sieve(oracle, k):
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    _, reads = synth_reads(800, 30_000, seed=3)
    lo, hi, _ = oracle.OracleTable(k).count_reads(reads).export_ge(0)
    flo, fhi = lo[::3], hi[::3]
    parent = reads[::2]
    ot = oracle.OracleTable(k).load_filter(flo, fhi).count_reads_filtered(parent)
    want = ot.query(flo, fhi)
    assert int((want == 0).sum()) > 0 and int((want > 0).sum()) > 0
    with KmerEngine(k) as e:
        e.load_filter(flo, fhi if k > 32 else None)
        assert int(e.histogram(3)[0]) == len(flo)            # a fresh filter: every key at 0
        e.set_option("force_path", 4)                        # through the sieve only
        e.count_filtered(ReadStream.from_strings(parent))
        assert e.last_count_path() == "sieve"
        check_engine(e, want, tag=f"filter k={k}")
        assert int(e.histogram(10)[0]) == int((want == 0).sum())
        e.set_option("force_path", 4)                        # still accepted: the sieve is still valid
        e.count_filtered(ReadStream.from_strings(parent))
        assert e.last_count_path() == "sieve"
        assert np.array_equal(e.query(flo, fhi if k > 32 else None), want * 2)
        check_engine(e, want.astype(np.uint64) * 2, tag=f"filter twice k={k}")
        e.reset_counts()
        assert int(e.histogram(3)[0]) == len(flo) and e.count_stats() == stats_of(np.zeros(len(flo)))


@pytest.mark.parametrize("path", [1, 2])
def test_pending_count_passes_are_applied_first(oracle, trio_reads, path):
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    reads = trio_child(trio_reads)
    k = 31
    with KmerEngine(k, capacity_hint=1 << 20) as one:
        one.set_option("force_path", path)
        one.count(ReadStream.from_strings(reads))
        want = one.histogram(100)
        want_stats = one.count_stats()
    _, _, cnt = oracle.OracleTable(k).count_reads(reads).export_ge(0)
    assert np.array_equal(want, bins_of(cnt, 100)) and want_stats == stats_of(cnt)
    step = len(reads) // 7 + 1
    for first in ("histogram", "count_stats"):
        with KmerEngine(k, capacity_hint=1 << 20) as e:
            e.set_option("force_path", path)
            for a in range(0, len(reads), step):             # no reader in between
                e.count(ReadStream.from_strings(reads[a:a + step]))
            if first == "histogram":
                assert np.array_equal(e.histogram(100), want)
            assert e.count_stats() == want_stats
            assert np.array_equal(e.histogram(100), want)


def test_growth_slices_owner_table_and_unchanged_table(oracle):
    import torch
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    k = 31
    ds, reads = synth_reads(2000, 60_000, seed=9)
    st = ReadStream.from_strings(reads)
    lo, hi, cnt = oracle.OracleTable(k).count_reads(reads).export_ge(0)
    want = bins_of(cnt, 50)
    # growth: a tiny table rehashes several times under the count
    with KmerEngine(k, capacity_hint=1 << 9) as e:
        e.count(st)
        assert e.stats()[0] >= 2 * len(lo)
        before = e.export_ge(0)
        check_engine(e, cnt, tag="grown")
        after = e.export_ge(0)                               # the table is unchanged by the calls
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        assert np.array_equal(after[0], lo) and np.array_equal(after[2], cnt)
    # key_parts: the slices' histograms sum to the whole table's
    for parts in (2, 5):
        acc = np.zeros(52, np.uint64)
        tot = {"unique": 0, "distinct": 0, "total": 0}
        mx = 0
        with KmerEngine(k, capacity_hint=1 << 12) as e:
            e.set_option("key_parts", parts)
            for p in range(parts):
                e.clear(); e.set_option("key_part", p)
                e.count(st)
                h = e.histogram(50)
                assert int(h.sum()) == e.stats()[1] == e.count_ge(0)
                acc += h
                s = e.count_stats()
                for n in tot:
                    tot[n] += s[n]
                mx = max(mx, s["max_count"])
        assert np.array_equal(acc, want), parts
        assert dict(tot, max_count=mx) == stats_of(cnt)
    # an owner table (hash_shift): direct count and the multi-segment merge
    for shift in (1, 3):
        with KmerEngine(k, capacity_hint=1 << 12) as e:
            e.set_option("hash_shift", shift)
            tl = torch.from_numpy(lo.view(np.int64).copy()).to("cuda:0")
            tc = torch.from_numpy(cnt.view(np.int32).copy()).to("cuda:0")
            torch.cuda.synchronize()
            e.add_pairs_multi_dev([(tl.data_ptr(), None, tc.data_ptr(), len(lo))] * 2)
            e.synchronize()
            check_engine(e, cnt.astype(np.uint64) * 2, tag=f"owner shift={shift}")


@pytest.mark.parametrize("k", [31, 63, 101])
def test_empty_cleared_and_refused(k):
    from kmer_denovo_filter_amd import KmerEngine, ReadStream, _native
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        assert not e.histogram(10).any() and e.histogram(0).shape == (2,)
        assert e.count_stats() == {"unique": 0, "distinct": 0, "total": 0, "max_count": 0}
        e.count(ReadStream.from_strings(["ACGTTGCA" * 40, "ACGTTGCA" * 40]))
        assert e.count_stats()["distinct"] > 0
        e.clear()                                            # a deferred clear: logically empty at once
        assert not e.histogram(10).any()
        assert e.count_stats() == {"unique": 0, "distinct": 0, "total": 0, "max_count": 0}
        assert e.histogram((1 << 20) - 1).shape == ((1 << 20) + 1,)
        lib = _native.load()
        buf = np.zeros(4, np.uint64)
        rc = lib.kdf_histogram(e._h, KmerEngine.HISTO_MAX_HIGH + 1, buf.ctypes.data)
        assert rc == _native.KDF_ERR_INVALID
        assert str(KmerEngine.HISTO_MAX_HIGH).encode() in lib.kdf_last_error(e._h)     # the message names the limit
        assert lib.kdf_histogram_dev(e._h, KmerEngine.HISTO_MAX_HIGH + 1, buf.ctypes.data) == _native.KDF_ERR_INVALID
        with pytest.raises(ValueError):
            e.histogram(KmerEngine.HISTO_MAX_HIGH + 1)
        assert lib.kdf_count_stats(e._h, None, None, None, None) == 0               # any pointer may be NULL


def test_profile_names_the_histogram_kernel():
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    with KmerEngine(31, capacity_hint=1 << 16) as e:
        e.count(ReadStream.from_strings(["ACGTTGCAAGGCTTAACCGGTATTAGC" * 10]))
        e.histogram(10)
        assert e.get_stat("histo_passes") == 0               # only under kdf_profile
        e.profile(True)
        e.histogram(10); e.count_stats()
        assert e.get_stat("histo_passes") == 2 and e.get_stat("histo_us") > 0
        e.profile(True)
        assert e.get_stat("histo_passes") == 0


def test_wrappers_on_a_live_engine(oracle, trio_reads):
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as jw
    reads = trio_child(trio_reads)
    _, _, cnt = oracle.OracleTable(31).count_reads(reads).export_ge(0)
    with KmerEngine(31, capacity_hint=1 << 20) as e:
        e.count(ReadStream.from_strings(reads))
        b = bins_of(cnt, 20)
        assert jw._jellyfish_histo(e, low=3, high=20) == [(c, int(b[c])) for c in range(3, 22) if b[c]]
        assert jw._jellyfish_stats(e) == stats_of(cnt)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _rank(rank, world, port, reads, k, q):
    try:
        import datetime
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=120))
        from kmer_denovo_filter_amd import KmerEngine, ReadStream
        from kmer_denovo_filter_amd.distributed import EngineOps, OwnerPartitionedCount
        dev = torch.device("cuda:0")
        with KmerEngine(k, capacity_hint=1 << 20) as le, KmerEngine(k, capacity_hint=1 << 20) as oe:
            opc = OwnerPartitionedCount(EngineOps(le, dev), device=dev, owner_ops=EngineOps(oe, dev), stage_through_host=True)
            le.count(ReadStream.from_strings(reads[rank::world]))
            local = le.histogram(100)
            opc.exchange()
            bins = opc.histogram(100)
            stats = opc.count_stats()
            own = oe.histogram(100)
            q.put(("ok", rank, bins.cpu().numpy().view(np.uint64), stats, local, own, str(bins.device)))
            dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # noqa: BLE001
        import traceback
        q.put(("err", rank, f"{ex}\n{traceback.format_exc()}"))


def test_two_ranks_global_histogram(oracle, trio_reads):
    """Each rank counts its half of the child reads; after the owner exchange one all-reduce gives every rank the
    histogram and the stats of ALL reads."""
    import torch.multiprocessing as mp
    k, world = 31, 2
    reads = trio_child(trio_reads)
    _, _, cnt = oracle.OracleTable(k).count_reads(reads).export_ge(0)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, reads, k, q)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        res = [q.get(timeout=300) for _ in range(world)]
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:                                      # no GPU-holding child outlives the test
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
                if p.is_alive():
                    p.kill()
    for r in res:
        assert r[0] == "ok", r[2]
    want = bins_of(cnt, 100)
    owners = np.zeros(102, np.uint64)
    for _, rank, bins, stats, local, own, device in res:
        assert np.array_equal(bins, want), rank
        assert stats == stats_of(cnt), rank
        assert device.startswith("cuda")
        assert not np.array_equal(local, want)               # a half-sample's table is not the answer
        owners += own
    assert np.array_equal(owners, want)                      # every key on exactly one owner
