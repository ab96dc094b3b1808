"""Long k-mers across ranks, host side (no GPU): the owner rule for W-word keys against a big-int restatement of the
formulas in include/kdf.h / csrc/kdf_long.h, its balance, the owner exchange and the count --if merge carrying (n, W)
rows under gloo on CPU tensors (a dict-backed TableOps without a packed export, so the torch fallback builds the wire
format), and the opt-in switch of mirror_engine."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

M64 = (1 << 64) - 1
MIX_MUL = 0x9FB21C651E98DF25
FOLD_ADD = 0x632BE59BD9B4E019


def _mix64(x):
    x ^= x >> 32
    return (x * MIX_MUL) & M64


def _owner_int(words, world):
    """kdf.h, "long keys across ranks": h = mix64(w0 ^ fold(w1 .. w_{W-1})), the fold from the top word down."""
    f = 0
    for w in reversed(words[1:]):
        f = (_mix64(f ^ w) + FOLD_ADD) & M64
    h = _mix64(words[0] ^ f)
    return (((h >> 16) & 0xFFFF) * world) >> 16


def _rows_t(rows_u64):
    return torch.from_numpy(np.ascontiguousarray(rows_u64, dtype=np.uint64).view(np.int64))


def _top_mask(W):
    return (1 << 62) - 1                     # a top word of a long key holds at most 62 bits


def _families(n, W, seed):
    """Three key families: random, w0 sequential (all else shared), top word sequential (all else shared)."""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 1 << 63, (n, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, W), dtype=np.uint64)
    rnd[:, W - 1] &= np.uint64(_top_mask(W))
    base = rnd[0].copy()
    seq0 = np.tile(base, (n, 1)); seq0[:, 0] = np.arange(n, dtype=np.uint64)
    seqt = np.tile(base, (n, 1)); seqt[:, W - 1] = np.arange(n, dtype=np.uint64)
    return {"random": rnd, "w0 sequential": seq0, "top word sequential": seqt}


@pytest.mark.parametrize("W", (3, 4, 5, 6, 7))
def test_owner_of_w_against_restatement(W):
    from kmer_denovo_filter_amd.distributed import owner_of_w
    rng = np.random.default_rng(W)
    rows = rng.integers(0, 1 << 63, (300, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (300, W), dtype=np.uint64)
    rows[:, W - 1] &= np.uint64(_top_mask(W))
    rows[0] = 0                                                    # the all-zero key (poly-A)
    rows[1:40] = rows[40]                                          # keys that differ only in the top word
    rows[1:40, W - 1] = np.arange(39, dtype=np.uint64)
    rows[41] = M64; rows[41, W - 1] = np.uint64(_top_mask(W))     # every bit set
    for world in (1, 2, 3, 8, 64):
        got = owner_of_w(_rows_t(rows), world).tolist()
        want = [_owner_int([int(x) for x in r], world) for r in rows]
        assert got == want, (W, world)
        assert 0 <= min(got) and max(got) < world
    assert len(set(owner_of_w(_rows_t(rows[1:40]), 64).tolist())) > 10   # the top word reaches the owner bits
    with pytest.raises(ValueError):
        owner_of_w(_rows_t(rows), 65)
    with pytest.raises(ValueError):
        owner_of_w(_rows_t(rows)[:, 0], 2)


@pytest.mark.parametrize("W", (3, 7))
def test_owner_of_w_balance(W):
    """Every owner's share within 5 % of 1 / world (relative) for 200 000 keys of each family."""
    from kmer_denovo_filter_amd.distributed import owner_of_w
    for name, rows in _families(200_000, W, 100 + W).items():
        t = _rows_t(rows)
        for world in (2, 3, 8):
            share = torch.bincount(owner_of_w(t, world), minlength=world).double() / len(rows)
            worst = float(((share - 1 / world).abs() * world).max())
            print(f"W={W} {name} world={world}: worst relative deviation {worst:.4f}")
            assert worst < 0.05, (W, name, world, share.tolist())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class RowDictOps:
    """TableOps over a dict {key row (tuple of W uint64 words) -> count} (tests only): no packed export, so
    OwnerPartitionedCount.exchange builds the wire format with torch."""

    def __init__(self, W):
        self.key_words, self.wide = W, True
        self.device = torch.device("cpu")
        self.d = {}
        self.segments_seen = 0

    def clear(self):
        self.d = {}

    def export_pairs(self, min_count):
        items = [(k, c) for k, c in self.d.items() if c >= min_count]
        rows = np.array([k for k, _ in items], dtype=np.uint64).reshape(len(items), self.key_words)
        cnt = np.array([c for _, c in items], dtype=np.uint32)
        return _rows_t(rows), None, torch.from_numpy(cnt.view(np.int32).copy())

    def add_pairs(self, rows, hi, cnt):
        assert hi is None and rows.dim() == 2 and rows.shape[1] == self.key_words and rows.shape[0] == cnt.shape[0]
        self.segments_seen += 1
        r = rows.contiguous().numpy().view(np.uint64)
        for k, c in zip(map(tuple, r.tolist()), cnt.contiguous().numpy().view(np.uint32).tolist()):
            self.d[k] = min(self.d.get(k, 0) + c, 0xFFFFFFFF)

    def query(self, rows, hi):
        assert hi is None
        r = rows.contiguous().numpy().view(np.uint64)
        c = np.array([self.d.get(k, 0) for k in map(tuple, r.tolist())], dtype=np.uint32)
        return torch.from_numpy(c.view(np.int32).copy())

    def count_ge(self, min_count):
        return sum(1 for c in self.d.values() if c >= min_count)

    def stats(self):
        return (0, len(self.d), 0)


def _local_table(rank, world, W):
    """Rank r's local (row -> count) table.  The ranks share most keys (their counts must sum).  At world 3 the last
    rank's table is empty and no key is owned by it (a destination that receives nothing)."""
    from kmer_denovo_filter_amd.distributed import owner_of_w
    rng = np.random.default_rng(7 * W)
    pool = rng.integers(0, 1 << 62, (700, W), dtype=np.uint64)
    pool[:50, 1:] = pool[0, 1:]                                    # keys that share everything but w0
    pool[50:100, :W - 1] = pool[50, :W - 1]                        # ... everything but the top word
    if world == 3:
        pool = pool[owner_of_w(_rows_t(pool), world).numpy() != world - 1]
    if world == 3 and rank == world - 1:
        return {}
    r2 = np.random.default_rng(1000 + rank)
    pick = r2.random(len(pool)) < 0.7
    pick[:3] = True
    cnt = r2.integers(1, 1000, len(pool))
    cnt[:3] = (0xFFFFFFFF, 0xFFFFFFF0, 1 << 31)                   # sums that saturate / pass 2^31
    return {tuple(int(x) for x in row): int(c) for row, c, p in zip(pool, cnt, pick) if p}


def _exchange_worker(rank, world, port, W, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmer_denovo_filter_amd.distributed import OwnerPartitionedCount, ShardedFilterCount, owner_of_w
        local, owner = RowDictOps(W), RowDictOps(W)
        local.d = _local_table(rank, world, W)
        opc = OwnerPartitionedCount(local, owner_ops=owner)
        opc.exchange()
        rows, _, _ = owner.export_pairs(0)
        own = owner_of_w(rows, world) if rows.shape[0] else torch.zeros(0, dtype=torch.int64)
        assert bool((own == rank).all()), "a rank holds a key it does not own"
        assert opc.last_exchange_pairs == len(local.d)
        n1 = owner.count_ge(1)
        # count --if merge with rows: every rank queries the same keys of its own shard's counts
        keys = _rows_t(np.array(sorted(_local_table(0, world, W)), dtype=np.uint64).reshape(-1, W))
        sfc = ShardedFilterCount(local)
        merged = sfc.merged_counts(keys, None)
        q.put((rank, dict(owner.d), owner.segments_seen, merged.tolist(), str(sfc.last_reduce_dtype), n1))
    finally:
        dist.destroy_process_group()


def _run(target, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=120) for _ in range(world)]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    return sorted(res, key=lambda r: r[0])


@pytest.mark.parametrize("W,world", [(3, 2), (7, 2), (3, 3), (7, 3)])
def test_owner_exchange_of_key_rows_over_gloo(W, world):
    res = _run(_exchange_worker, world, W)
    exp = {}
    locals_ = [_local_table(r, world, W) for r in range(world)]
    assert all(len(t) > 300 for t in locals_[:2]) and (world == 2 or locals_[2] == {})
    for t in locals_:
        for k, c in t.items():
            exp[k] = min(exp.get(k, 0) + c, 0xFFFFFFFF)
    got = {}
    for _, owned, _, _, _, _ in res:
        assert not (set(owned) & set(got)), "two ranks own the same key"
        got.update(owned)
    assert got == exp                                              # the union is the sum of the local tables
    assert sum(1 for v in exp.values() if v == 0xFFFFFFFF) == 3   # the sums that pass 2^32 - 1 saturate
    if world == 3:
        assert res[2][1] == {} and res[2][2] == 0                  # the last rank owns nothing and received nothing
        assert res[0][2] == 2 and res[1][2] == 2                   # the empty rank sent no segment
    # the count --if merge of rows: the sum of the ranks' counts, clamped, the same on every rank
    keys = sorted(locals_[0])
    want = [min(sum(t.get(k, 0) for t in locals_), 0xFFFFFFFF) for k in keys]
    for r in res:
        assert r[3] == want
        assert r[4] == "torch.int64"                               # counts near 2^32: 8-byte words


def _small_counts_worker(rank, world, port, W, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmer_denovo_filter_amd.distributed import ShardedFilterCount
        ops = RowDictOps(W)
        rows = np.arange(5 * W, dtype=np.uint64).reshape(5, W)
        ops.d = {tuple(int(x) for x in r): (rank + 1) * (i + 1) for i, r in enumerate(rows)}
        ops.d[tuple(int(x) for x in rows[4])] = 0x7FFFFFFF // world    # world x max just inside the signed range
        sfc = ShardedFilterCount(ops)
        m = sfc.merged_counts(_rows_t(rows), None)
        a = (str(sfc.last_reduce_dtype), m.tolist())
        ops.d[tuple(int(x) for x in rows[4])] = 0x7FFFFFFF // world + 1   # ... just outside: the int64 fallback
        m = sfc.merged_counts(_rows_t(rows), None)
        q.put((rank, a, (str(sfc.last_reduce_dtype), m.tolist())))
    finally:
        dist.destroy_process_group()


def test_merged_counts_with_rows_int32_path_and_int64_fallback():
    world, W = 2, 5
    res = _run(_small_counts_worker, world, W)
    tri = sum(r + 1 for r in range(world))
    for _, a, b in res:
        assert a == ("torch.int32", [tri * (i + 1) for i in range(4)] + [(0x7FFFFFFF // world) * world])
        big = (0x7FFFFFFF // world + 1) * world
        assert big >= 2 ** 31
        assert b == ("torch.int64", [tri * (i + 1) for i in range(4)] + [big])


def test_mirror_engine_long_k_under_ranks_is_opt_in(monkeypatch):
    from kmer_denovo_filter_amd import dist_env, engine

    class Stub:
        MAX_K, LONG_MIN_K, LONG_MAX_K = 63, 65, 201

        def __init__(self, k, *a, **kw):
            self.k, self.args = k, (a, kw)

    monkeypatch.setattr(engine, "KmerEngine", Stub)                # no library load
    monkeypatch.setattr(dist_env, "world_rank", lambda: (2, 1, True))
    monkeypatch.delenv("KDF_LONG_RANKS", raising=False)
    with pytest.raises(ValueError, match=r"k=101: long k-mers \(odd 65\.\.201\) run in one process; the multi-GPU mirrors "
                                         r"\(2 ranks\) take k <= 63"):
        engine.mirror_engine(101)
    monkeypatch.setenv("KDF_LONG_RANKS", "0")
    with pytest.raises(ValueError, match="k <= 63"):
        engine.mirror_engine(101)
    monkeypatch.setenv("KDF_LONG_RANKS", "1")
    e = engine.mirror_engine(101, capacity_hint=5)
    assert isinstance(e, Stub) and e.k == 101 and e.args == ((), {"capacity_hint": 5})
    assert isinstance(engine.mirror_engine(31), Stub)              # k <= 63: untouched either way
