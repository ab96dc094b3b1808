"""Two-pass counting over several ranks on the GPU (include/kdf.h "two-pass counting": several ranks): the ranks tally
their shards, merge their sieves (``OwnerPartitionedCount.prefilter_merge`` over ``kdf_pf_merge_kernel``), count gated
and exchange -- and the owners end with exactly what ONE engine's two-pass count of all the reads holds.

Process layout of test_gpu_sharded_mirrors.py: world 2 and 3 on the one GPU of the test box, one fresh child process
per rank, gloo with host-staged collectives (RCCL needs one GPU per rank: unmeasured on hardware).  The ranks of one
world run once and do both parts:
(a) ``OwnerPartitionedCount`` + ``EngineOps`` on synthetic shards (shared genome, one read seed per rank);
(b) the drop-in mirror ``_extract_child_kmers_discovery`` on the mini trio with ``KDF_PREFILTER=1``."""
import os
import socket

import numpy as np
import pytest

from conftest import GIAB

pytestmark = pytest.mark.gpu

K, L, S = 31, 3, 18
CHUNK = 3000                 # 2^14 words: world 2 -> 8192 = 2 x 3000 + 2192; world 3 -> 5461 / 5462 = 3000 + 2461 / 2462
N_READS, GENOME = 1500, 60_000


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _shard(rank):
    from kmer_denovo_filter_amd.synth import synth_stream
    return synth_stream(N_READS, read_len=150, genome_len=GENOME, seed=1000 + rank, genome_seed=77, sub_rate=0.01)


def _rank(rank, world, port, tmp, q):
    try:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        from kmer_denovo_filter_amd import KmerEngine
        from kmer_denovo_filter_amd.distributed import EngineOps, OwnerPartitionedCount
        dev = torch.device("cuda", 0)
        # ---- (a) synthetic shards
        ds = _shard(rank)
        torch.cuda.synchronize()
        with KmerEngine(K, capacity_hint=1 << 16) as eng, KmerEngine(K, capacity_hint=1 << 16) as own:
            opc = OwnerPartitionedCount(EngineOps(eng, dev), device=dev, owner_ops=EngineOps(own, dev), stage_through_host=True)
            n_plain = opc.count_and_merge(ds.packed, ds.invalid, ds.n_bases, L)      # the same run without the prefilter
            pairs_plain = opc.last_exchange_pairs
            opc.clear()
            assert opc.prefilter_begin(L, S) == S
            opc.tally_local(ds.packed, ds.invalid, ds.n_bases)
            opc.prefilter_merge(chunk_words=CHUNK)
            assert eng.get_stat("prefilter_state") == 2 and own.get_stat("prefilter_state") == 0
            sieve = eng.prefilter_export()
            windows = opc.prefilter_windows()
            opc.count_local(ds.packed, ds.invalid, ds.n_bases)
            n_pf = opc.merge(L)
            lo, _, cnt = own.export_ge(0)
            synth = dict(n_plain=n_plain, n_pf=n_pf, pairs_plain=pairs_plain, pairs_pf=opc.last_exchange_pairs, sieve=sieve,
                         windows=windows, rounds=opc.last_prefilter_rounds, lo=lo, cnt=cnt)
            opc.prefilter_drop()
        # ---- (b) the mirror
        os.environ["KDF_READER_PIPELINES"] = "2"                    # two BGZF ranges per rank
        os.environ["KDF_PREFILTER"] = "1"
        from kmer_denovo_filter_amd.discovery import pipeline
        from kmer_denovo_filter_amd.kmer_fasta import read_kmer_fasta_keys
        fa, n1 = pipeline._extract_child_kmers_discovery(os.path.join(GIAB, "HG002_child.bam"), None, 31, 3, 4, tmp)
        cand = np.sort(read_kmer_fasta_keys(fa, 31)[0])
        q.put(("ok", rank, synth, n1, cand, dict(pipeline.LAST_CHILD_COUNT)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # noqa: BLE001
        import traceback
        q.put(("err", rank, f"{ex}\n{traceback.format_exc()}"))


@pytest.fixture(scope="module", params=[2, 3])
def ranks(request, tmp_path_factory):
    import torch.multiprocessing as mp
    world = request.param
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    tmp = str(tmp_path_factory.mktemp(f"world{world}"))
    procs = [ctx.Process(target=_rank, args=(r, world, port, tmp, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
    for r in res:
        assert r[0] == "ok", r[2]
    return world, sorted(res, key=lambda r: r[1])


@pytest.fixture(scope="module")
def single_engine():
    """world -> what ONE engine holds after a two-pass count of the concatenated shards: (sieve, lo, counts, tallied windows)"""
    cache = {}

    def get(world):
        if world not in cache:
            import torch
            from kmer_denovo_filter_amd import KmerEngine
            shards = [_shard(r) for r in range(world)]
            torch.cuda.synchronize()
            with KmerEngine(K, capacity_hint=1 << 16) as e:
                e.prefilter_begin(L, S)
                for ds in shards:
                    e.prefilter_add_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
                sieve, windows = e.prefilter_export(), e.get_stat("prefilter_windows")
                e.prefilter_arm()
                for ds in shards:
                    e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
                lo, _, cnt = e.export_ge(0)
            cache[world] = (sieve, lo, cnt, windows)
        return cache[world]
    return get


def test_owner_dumps_equal_the_single_engine_two_pass_count(ranks, single_engine):
    world, res = ranks
    sieve, lo, cnt, windows = single_engine(world)
    got_lo = np.concatenate([r[2]["lo"] for r in res])
    got_cnt = np.concatenate([r[2]["cnt"] for r in res])
    order = np.argsort(got_lo, kind="stable")
    assert len(np.unique(got_lo)) == len(got_lo), "two ranks own the same key"
    np.testing.assert_array_equal(got_lo[order], lo)                # export_ge: ascending keys
    np.testing.assert_array_equal(got_cnt[order], cnt)
    n_words = 1 << (S - 4)
    longest = max((r + 1) * n_words // world - r * n_words // world for r in range(world))
    for _, rank, s, _, _, _ in res:
        np.testing.assert_array_equal(s["sieve"], sieve)            # every rank held the sieve of all reads
        assert s["windows"] == windows
        assert s["n_pf"] == s["n_plain"] == int((cnt >= L).sum())   # dump -L is the plain sharded count's
        assert s["rounds"] == -(-longest // CHUNK) >= 2 and longest % CHUNK != 0
    # the exchange moved admitted keys only
    assert sum(r[2]["pairs_pf"] for r in res) < sum(r[2]["pairs_plain"] for r in res)
    assert sum(r[2]["pairs_pf"] for r in res) >= len(lo)


@pytest.fixture(scope="module")
def oracle_candidates(oracle, trio_reads):
    ref = oracle.read_fasta(os.path.join(GIAB, "mini_ref.fa"))
    rt = oracle.OracleTable(31).count_reads([s for _, s in ref])
    return oracle.discovery_chain(trio_reads["child"], trio_reads["mother"], trio_reads["father"], rt, 31, 3, 0)["candidates"][0]


def test_child_count_mirror_takes_the_sharded_two_pass_path(ranks, oracle_candidates):
    world, res = ranks
    for _, rank, _, n1, cand, mode in res:
        assert n1 == 51125 == len(oracle_candidates)
        np.testing.assert_array_equal(cand, oracle_candidates)
        assert (mode["mode"], mode["L"], mode["world"]) == ("two_pass_sharded", 3, world), mode
        assert 16 <= mode["log2_cells"] <= 38
