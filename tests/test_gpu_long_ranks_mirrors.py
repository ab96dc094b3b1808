"""The drop-in mirrors at long k as a multi-rank job (KDF_LONG_RANKS=1): world 2 and world 3 over gloo on the one GPU
of the test box run the mini-trio discovery chain at k = 75 through the SAME functions a one-process run calls.  Every
rank's stage counts, key sets and parent-scan dict are checked against the pure-Python restatement of the chain
(oracle.py_count, as tests/test_gpu_long_k_pipeline.py) and against a one-process run of the same functions, whose
contract FASTA files rank 0 must reproduce byte for byte.  The path has only ever run like this -- several ranks on one
GPU, host-staged collectives; RCCL needs one GPU per rank."""
import os
import shutil
import socket

import pytest

from conftest import GIAB

pytestmark = pytest.mark.gpu

K, MIN_CHILD, PARENT_MAX = 75, 3, 0
CHILD, MOTHER, FATHER = (os.path.join(GIAB, n) for n in ("HG002_child.bam", "HG004_mother.bam", "HG003_father.bam"))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _chain(tmp, ref_jf, barrier=lambda: None):
    """The chain through the mirrors; -> {"n": the three stage counts, "fa": the three FASTA files' bytes, "scan"}."""
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _scan_parent_jellyfish
    from kmer_denovo_filter_amd.discovery.pipeline import (
        _extract_child_kmers_discovery, _filter_parents_discovery, _subtract_reference_kmers)
    fa, n1 = _extract_child_kmers_discovery(CHILD, None, K, MIN_CHILD, 4, tmp)
    b1 = _read(fa)
    barrier()                                                       # (the next stage deletes the file on rank 0)
    fa2, n2 = _subtract_reference_kmers(ref_jf, fa, tmp)
    barrier()
    gone = not os.path.exists(fa)
    b2 = _read(fa2)
    scan = _scan_parent_jellyfish(MOTHER, None, fa2, K, os.path.join(tmp, f"scan{os.getpid()}"), 4)
    n3, fa3 = _filter_parents_discovery(MOTHER, FATHER, None, fa2, K, 4, tmp, PARENT_MAX)
    barrier()
    return {"n": (n1, n2, n3), "fa": (b1, b2, _read(fa3)), "gone": gone, "scan": scan}


def _rank(rank, world, port, tmp, ref_jf, env, q):
    try:
        import torch
        import torch.distributed as dist
        os.environ.update(env)
        os.environ["KDF_LONG_RANKS"] = "1"
        os.environ["KDF_READER_PIPELINES"] = "2"                    # two BGZF ranges per rank
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        from kmer_denovo_filter_amd.discovery import pipeline
        res = _chain(tmp, ref_jf, dist.barrier)
        res["mode"] = dict(pipeline.LAST_CHILD_COUNT or {})
        q.put(("ok", rank, res))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # noqa: BLE001
        import traceback
        q.put(("err", rank, f"{ex}\n{traceback.format_exc()}"))


@pytest.fixture(scope="module")
def reference(tmp_path_factory, oracle, trio_reads):
    """Built once: the chain restated in Python, and a one-process run of the mirrors (no process group, switch unset)."""
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _ensure_ref_jf
    tmp = str(tmp_path_factory.mktemp("long_ranks_ref"))
    fa = os.path.join(tmp, "mini_ref.fa")
    shutil.copy(os.path.join(GIAB, "mini_ref.fa"), fa)              # nothing is written under tests/golden
    ref_jf = _ensure_ref_jf(fa, K, 4)
    assert ref_jf.startswith(tmp)
    one = _chain(tmp, ref_jf)
    ref_seqs = [s for _, s in oracle.read_fasta(os.path.join(GIAB, "mini_ref.fa"))]
    child = oracle.py_count(trio_reads["child"], K)
    cand = {c for c, v in child.items() if v >= MIN_CHILD}
    non_ref = cand - set(oracle.py_count(ref_seqs, K))
    m = oracle.py_count(trio_reads["mother"], K, non_ref)
    after_m = {c for c in non_ref if m[c] <= PARENT_MAX}
    f = oracle.py_count(trio_reads["father"], K, after_m)
    want = {"sets": (cand, non_ref, {c for c in after_m if f[c] <= PARENT_MAX}),
            "scan": {c: v for c, v in m.items() if v >= 1}}
    return ref_jf, one, want


def _kmers_of(fasta_bytes):
    return [ln for ln in fasta_bytes.decode().split("\n") if ln and not ln.startswith(">")]


def _run_ranks(world, tmp, ref_jf, env):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, tmp, ref_jf, env, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, failure = [], None
    try:
        for _ in range(world):
            res.append(q.get(timeout=600))
    except Exception as ex:  # noqa: BLE001  (queue.Empty: a rank never reported)
        failure = f"a rank did not report: {ex!r}"
    for p in procs:
        p.join(timeout=5 if failure else 120)
    for p in procs:
        if p.is_alive():                                            # never left running, never retried
            p.terminate()
            p.join(timeout=30)
            failure = failure or "a rank did not exit"
    assert failure is None, failure
    for r in res:
        assert r[0] == "ok", r[2]
    return sorted(res, key=lambda r: r[1])


def _check(res, reference, mode):
    _, one, want = reference
    assert one["gone"] and all(len(s) > 0 for s in want["sets"])
    # the one-process run against the restatement
    for b, s, n in zip(one["fa"], want["sets"], one["n"]):
        ks = _kmers_of(b)
        assert n == len(ks) == len(s) and set(ks) == s
    assert one["scan"] == want["scan"]
    for _, rank, got in res:
        assert got["n"] == one["n"], rank
        assert got["fa"] == one["fa"], f"rank {rank}: a contract FASTA differs from the one-process run's bytes"
        assert got["gone"]
        assert got["scan"] == want["scan"], rank
        assert got["mode"].get("mode") == mode and got["mode"].get("world") == len(res)


@pytest.mark.parametrize("world", [2, 3])
def test_long_k_chain_sharded_over_ranks(reference, tmp_path, world):
    _check(_run_ranks(world, str(tmp_path), reference[0], {}), reference, "plain")


def test_long_k_chain_with_key_parts(reference, tmp_path):
    _check(_run_ranks(2, str(tmp_path), reference[0], {"KDF_KEY_PARTS": "2"}), reference, "plain")


def test_long_k_chain_with_prefilter(reference, tmp_path):
    res = _run_ranks(2, str(tmp_path), reference[0], {"KDF_PREFILTER": "1"})
    _check(res, reference, "two_pass_sharded")
    assert all(r[2]["mode"]["L"] == 3 for r in res)
