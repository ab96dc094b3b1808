"""Two-pass counting over several ranks, host logic under gloo (CPU tensors): ``OwnerPartitionedCount.prefilter_begin /
tally_local / prefilter_merge`` with a MODEL standing in for the per-rank table -- the oracle counts, ``prefilter_model``
places the cells, ``prefilter_merge_model`` is the saturating sum.  What is tested is the hand-made reduce-scatter +
all-gather (slices that are not equal, several rounds, a ragged last round) and that the gated sharded count ends
with the single-process two-pass table on the owners.  Without the feature this fails with AttributeError."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import prefilter_merge_model as MM
import prefilter_model as PM

S = 16                       # 2^16 cells: 4096 words, not divisible by 3
CHUNK = 500                  # words per peer and round: world 2 -> 2048 = 4 x 500 + 48; world 3 -> 1365 / 1366 = 2 x 500 + 365 / 366
L = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _make_reads(seed, n=150, k=21):
    """about 2x coverage of a small genome: counts of 1, 2, 3 and more all occur, and a key's sightings spread over the ranks"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, 6000)
    out = []
    for _ in range(n):
        ln = int(rng.integers(k, 160))
        st = int(rng.integers(0, len(genome) - ln))
        r = np.frombuffer(b"ACGT", np.uint8)[genome[st:st + ln]].copy()
        r[rng.random(ln) < 0.01] = ord("N")
        out.append(r.tobytes().decode())
    return out


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy())


class ModelOps:
    """TableOps over the oracle and the sieve models (tests only): the table is a dict, the sieve an array of cell values."""

    def __init__(self, O, k):
        self.O, self.k, self.wide = O, k, k > 32
        self.device = torch.device("cpu")
        self.vals = None                                   # int64[n_words, 16]: the value of every cell
        self.state = "off"
        self.tallied = 0
        self.clear()

    def clear(self):
        self.table = {}                                    # (hi, lo) -> count
        self.windows = 0

    def _truth(self, reads):
        return self.O.OracleTable(self.k).count_reads(reads).export_ge(0)

    def _cells(self, lo, hi):
        return PM.cells_np(lo, hi, self.k, self.s).astype(np.int64)

    # ---- table
    def count_stream(self, reads, _invalid, _n):
        assert self.state != "tallying", "an insert-mode count while tallying is refused by the engine"
        lo, hi, c = self._truth(reads)
        keep = np.ones(len(lo), bool)
        if self.state == "armed":
            keep = self.vals.ravel()[self._cells(lo, hi)] >= self.L
        self.add_pairs(_i64(lo[keep]), _i64(hi[keep]), torch.from_numpy(c[keep].astype(np.uint32).view(np.int32).copy()))
        self.windows += int(c[keep].sum())

    def export_pairs(self, min_count):
        items = [(k, v) for k, v in self.table.items() if v >= min_count]
        lo = np.array([a for (_, a), _ in items], dtype=np.uint64)
        hi = np.array([b for (b, _), _ in items], dtype=np.uint64)
        c = np.array([v for _, v in items], dtype=np.uint32)
        return _i64(lo), (_i64(hi) if self.wide else None), torch.from_numpy(c.view(np.int32).copy())

    def add_pairs(self, lo, hi, cnt):
        lo_u = lo.numpy().view(np.uint64)
        hi_u = hi.numpy().view(np.uint64) if hi is not None else np.zeros(len(lo_u), np.uint64)
        for a, b, c in zip(lo_u.tolist(), hi_u.tolist(), cnt.numpy().view(np.uint32).tolist()):
            self.table[(b, a)] = min(self.table.get((b, a), 0) + c, 0xFFFFFFFF)

    def count_ge(self, min_count):
        return sum(1 for v in self.table.values() if v >= min_count)

    def stats(self):
        return (0, len(self.table), self.windows)

    # ---- sieve
    def prefilter_begin(self, min_count, log2_cells):
        assert self.state == "off" and min_count in (2, 3) and 16 <= log2_cells <= 38
        self.L, self.s = min_count, log2_cells
        self.vals = np.zeros((1 << (log2_cells - 4), 16), dtype=np.int64)
        self.state, self.tallied = "tallying", 0

    def prefilter_tally_stream(self, reads, _invalid, _n):
        assert self.state == "tallying"
        lo, hi, c = self._truth(reads)
        add = np.bincount(self._cells(lo, hi), weights=c, minlength=1 << self.s).astype(np.int64)
        self.vals = np.minimum(self.vals + add.reshape(-1, 16), 3)
        self.tallied += int(c.sum())

    def prefilter_words(self):
        assert self.state != "off"
        return len(self.vals)

    def prefilter_export(self, first, n):
        assert self.state != "off" and 0 <= first and first + n <= len(self.vals)
        return _i64(MM.encode(self.vals[first:first + n])) if n else torch.zeros(0, dtype=torch.int64)

    def prefilter_merge(self, first, segments, replace=False):
        assert self.state == "tallying", "the sieve is immutable once armed"
        segs = [s.numpy().view(np.uint64) for s in segments]
        n = len(segs[0])
        assert all(len(s) == n for s in segs) and first + n <= len(self.vals)
        self.merge_calls.append((first, n, len(segs), bool(replace)))
        self.vals[first:first + n] = MM.values(MM.merge(MM.encode(self.vals[first:first + n]), segs, replace))

    merge_calls = None

    def prefilter_arm(self):
        assert self.state == "tallying"
        self.state = "armed"

    def prefilter_drop(self):
        assert self.state != "off"
        self.state, self.vals = "off", None

    def prefilter_windows(self):
        return self.tallied


def _worker(rank, world, port, k, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from oracle import oracle as O
        from kmer_denovo_filter_amd.distributed import OwnerPartitionedCount
        shard = _make_reads(11, k=k)[rank::world]
        batches = [shard[i:i + 20] for i in range(0, len(shard), 20)]
        local = ModelOps(O, k)
        local.merge_calls = []
        opc = OwnerPartitionedCount(local, owner_ops=ModelOps(O, k))
        try:
            opc.prefilter_begin(L)                         # several ranks: the sieve size must be given
            raise AssertionError("prefilter_begin without log2_cells must be refused under several ranks")
        except ValueError:
            pass
        assert opc.prefilter_begin(L, S - rank if rank else S) == S      # the ranks agree on the largest proposal
        for b in batches:
            opc.tally_local(b, None, 0)
        own_before = local.prefilter_export(0, local.prefilter_words()).numpy().view(np.uint64).copy()
        opc.prefilter_merge(chunk_words=CHUNK)
        assert local.state == "armed"
        sieve = local.prefilter_export(0, local.prefilter_words()).numpy().view(np.uint64).copy()
        windows = opc.prefilter_windows()
        for b in batches:
            opc.count_local(b, None, 0)
        n_ge = opc.merge(L)
        opc.prefilter_drop()
        q.put((rank, own_before, sieve, windows, dict(opc.owner.table), n_ge, opc.last_exchange_pairs, opc.last_prefilter_rounds,
               list(local.merge_calls)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("k,world", [(21, 2), (41, 3), (31, 3)])
def test_sieves_merge_and_gated_sharded_count(oracle, k, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, k, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    reads = _make_reads(11, k=k)
    lo, hi, cnt = oracle.OracleTable(k).count_reads(reads).export_ge(0)
    cells = PM.cells_np(lo, hi, k, S).astype(np.int64)
    value = np.minimum(np.bincount(cells, weights=cnt, minlength=1 << S).astype(np.int64), 3)
    expect_sieve = MM.encode(value.reshape(-1, 16))
    admitted = value[cells] >= L
    expect = {(int(b), int(a)): int(c) for a, b, c in zip(lo[admitted], hi[admitted], cnt[admitted])}
    assert 0 < len(expect) < len(lo) and (cnt < L).any()             # the gate keeps some keys out and lets some in
    n_words = 1 << (S - 4)
    assert n_words % 3 != 0
    got = {}
    for rank, own_before, sieve, windows, owned, n_ge, pairs, rounds, calls in res:
        # the rank's own sieve under-counts (else the merge would have nothing to do) ...
        assert not np.array_equal(own_before, expect_sieve)
        # ... and after the merge every rank holds the sieve of ALL reads, word for word
        np.testing.assert_array_equal(sieve, expect_sieve)
        assert windows == int(cnt.sum())
        assert not (set(owned) & set(got)), "two ranks own the same key"
        got.update(owned)
        assert n_ge == sum(1 for v in expect.values() if v >= L)
        # several rounds with a ragged last one; ONE merge call for all received segments of a round
        b = [r * n_words // world for r in range(world + 1)]
        longest = max(b[j + 1] - b[j] for j in range(world))
        assert rounds == -(-longest // CHUNK) >= 3 and longest % CHUNK != 0
        mine = [c for c in calls if not c[3]]
        assert len(mine) == rounds and all(c[2] == world - 1 for c in mine)
        assert sum(c[1] for c in mine) == b[rank + 1] - b[rank] and mine[-1][1] < CHUNK
        assert sum(c[1] for c in calls if c[3]) == n_words - (b[rank + 1] - b[rank])
    assert got == expect                                             # the single-process two-pass table, on the owners
    # the exchange moved admitted keys only: fewer pairs than the ranks' shards hold distinct keys
    plain_pairs = sum(len(oracle.OracleTable(k).count_reads(reads[r::world]).export_ge(0)[0]) for r in range(world))
    assert sum(r[6] for r in res) < plain_pairs
