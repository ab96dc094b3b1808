"""bench.py's options, without a GPU: --full is off by default, and --dump-outputs writes the
(key, count) pairs sorted by key, as exact float64, within its size bound, whatever the dump order."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_not_full():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full


def _words_to_u64(w):
    w = w.astype(np.uint64)
    return w[:, 0::2] | (w[:, 1::2] << np.uint64(32))


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("n", [1000, bench.DUMP_SAMPLE + 12345])
def test_dump_outputs(tmp_path, wide, n):
    rng = np.random.default_rng(5)
    lo = rng.integers(-2**63, 2**63 - 1, n + 17, dtype=np.int64)
    hi = rng.integers(-2**63, 2**63 - 1, n + 17, dtype=np.int64) if wide else None
    cnt = rng.integers(3, 500, n + 17).astype(np.int32)
    t = lambda a: None if a is None else torch.from_numpy(a)       # noqa: E731
    bench.dump_outputs(str(tmp_path / "a"), t(lo), t(hi), t(cnt), n, {"windows": 99})
    perm = rng.permutation(n)                                       # the same pairs in another dump order
    bench.dump_outputs(str(tmp_path / "b"), t(lo[:n][perm]), t(None if hi is None else hi[:n][perm]),
                       t(cnt[:n][perm]), n, {"windows": 99})

    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["kmer_keys.npy", "kmer_counts.npy", "n_kmers.npy", "count_sum.npy", "key_digest.npy",
                            "key_count_digest.npy", "windows.npy"])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 << 20
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b), f

    keys = _words_to_u64(np.load(tmp_path / "a" / "kmer_keys.npy")).view(np.int64)
    counts = np.load(tmp_path / "a" / "kmer_counts.npy")
    order = np.lexsort((lo[:n], hi[:n])) if wide else np.argsort(lo[:n], kind="stable")
    m = min(n, bench.DUMP_SAMPLE)
    assert keys.shape == (m, 2 if wide else 1) and counts.shape == (m,)
    if n > m:
        order = order[np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, m, replace=False))]
    assert np.array_equal(keys[:, 0], lo[:n][order]) and np.array_equal(counts, cnt[:n][order])
    if wide:
        assert np.array_equal(keys[:, 1], hi[:n][order])
    assert np.load(tmp_path / "a" / "n_kmers.npy")[0] == n
    assert np.load(tmp_path / "a" / "count_sum.npy")[0] == cnt[:n].sum()


def test_dump_outputs_needs_one_gpu(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs",
                        str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--gpus 1" in r.stderr
