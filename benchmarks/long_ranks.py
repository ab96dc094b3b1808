#!/usr/bin/env python3
"""The owner exchange for long k-mers (kdf_export_parts_w_packed_dev, per-segment kdf_add_pairs_w_dev) against its
yardsticks in the SAME run, on ONE MI355X, at k = 101 and k = 201, on a table counted from a synthetic read stream.

  (a) dump    ``export_parts_w_packed_dev`` at 2 and 8 parts against ``export_ge_w_dev`` (unsorted, keys and counts) of
              the same table: both dump every entry; the partitioned one reads the table twice (count pass, write pass)
              and synchronises once in between.
  (b) insert  the parts of (a) added segment by segment (``add_pairs_w_dev`` per segment, what an owner does with what
              it receives) into a fresh table of the final size, against ONE ``add_pairs_w_dev`` of all pairs.

No ratio is fixed in advance: the plain dump and the single insert are the yardsticks.  Wall clock around synchronised
calls, warm, best and median of --reps.  ``--rehearse`` instead runs a 2-rank owner exchange over gloo on the one GPU
(host-staged collectives) and checks the owners' tables against a one-table count of both shards -- a check, not a
measurement: nothing here says anything about RCCL or about scaling over GPUs.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def summary(ts):
    return {"best_ms": round(min(ts), 3), "median_ms": round(statistics.median(ts), 3)}


def measure(k, args):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.synth import synth_stream
    dev = torch.device("cuda", 0)
    ds = synth_stream(args.reads, args.read_len, args.genome, seed=20261019 + k, device=dev)
    torch.cuda.synchronize()
    out = {"k": k}
    with KmerEngine(k, capacity_hint=args.genome * 2) as e:
        e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
        cap, n, windows = e.stats()
        W = e.key_words
        esz = 8 * W + 4
        out.update(key_words=W, entries=n, table_slots=cap, windows=windows, entry_bytes=esz)
        keys = torch.empty((n, W), dtype=torch.int64, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        plain = wall(lambda: e.export_ge_dev(0, keys.data_ptr(), None, cnt.data_ptr(), n), args.reps + 1)[1:]
        out["export_ge_w_dev"] = summary(plain)
        bufs = {}
        for parts in (2, 8):
            cap_bytes = n * esz + 8 * parts
            buf = torch.empty(cap_bytes, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            res = {}

            def dump():
                res["r"] = e.export_parts_w_packed_dev(0, parts, buf.data_ptr(), cap_bytes)
            ts = wall(dump, args.reps + 1)[1:]
            got, counts, offs = res["r"]
            assert got == n == sum(counts)
            s = summary(ts)
            s["vs_export_ge_w_dev"] = round(s["median_ms"] / out["export_ge_w_dev"]["median_ms"], 3)
            s["largest_share"] = round(max(counts) / n, 4)
            out[f"export_parts_w_packed_dev_{parts}"] = s
            bufs[parts] = (buf, counts, offs)
    def timed_insert(fn):
        ts = []
        for _ in range(args.reps + 1):
            with KmerEngine(k, capacity_hint=n) as f:               # a fresh table of the final size: no rehash is timed
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(f)
                f.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                assert f.stats()[1] == n
        return summary(ts[1:])
    out["add_pairs_w_dev_single"] = timed_insert(lambda e: e.add_pairs_dev(keys.data_ptr(), None, cnt.data_ptr(), n))
    for parts, (buf, counts, offs) in bufs.items():
        base = buf.data_ptr()

        def per_segment(e):
            for p in range(parts):
                if counts[p]:
                    e.add_pairs_dev(base + offs[p], None, base + offs[p] + 8 * W * counts[p], counts[p])
        s = timed_insert(per_segment)
        s["vs_single"] = round(s["median_ms"] / out["add_pairs_w_dev_single"]["median_ms"], 3)
        out[f"add_pairs_w_dev_{parts}_segments"] = s
    return out


def _rehearse_rank(rank, world, port, k, args, q):
    try:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        from kmer_denovo_filter_amd import KmerEngine
        from kmer_denovo_filter_amd.distributed import EngineOps, OwnerPartitionedCount
        from kmer_denovo_filter_amd.synth import synth_stream
        dev = torch.device("cuda", 0)
        shards = [synth_stream(args.reads // world, args.read_len, args.genome, seed=7 + r, genome_seed=7, device=dev) for r in range(world)]
        torch.cuda.synchronize()
        with KmerEngine(k, capacity_hint=1 << 16) as local, KmerEngine(k, capacity_hint=1 << 16) as owner:
            opc = OwnerPartitionedCount(EngineOps(local, dev), device=dev, owner_ops=EngineOps(owner, dev), stage_through_host=True)
            mine = shards[rank]
            n3 = opc.count_and_merge(mine.packed, mine.invalid, mine.n_bases, min_count=3)
            st = opc.count_stats()
        with KmerEngine(k, capacity_hint=1 << 16) as one:           # every shard into one table: the truth
            for s in shards:
                one.count_dev(s.packed.data_ptr(), s.invalid.data_ptr(), s.n_bases)
            want = one.count_stats()
            want3 = one.count_ge(3)
        q.put(("ok", rank, {"ok": st == want and n3 == want3, "global": st, "one_table": want, "ge3": [n3, want3],
                            "pairs_sent": opc.last_exchange_pairs}))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # noqa: BLE001
        import traceback
        q.put(("err", rank, f"{ex}\n{traceback.format_exc()}"))


def rehearse(k, args):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    world = 2
    procs = [ctx.Process(target=_rehearse_rank, args=(r, world, port, k, args, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=600))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    bad = [r for r in res if r[0] != "ok" or not r[2]["ok"]]
    if bad or len(res) != world:
        raise SystemExit(f"rehearsal failed: {bad or 'a rank did not report'}")
    return {"k": k, "world": world, "backend": "gloo, one GPU, host-staged", **res[0][2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=400_000)
    ap.add_argument("--read-len", type=int, default=250)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--k", type=int, nargs="*", default=[101, 201])
    ap.add_argument("--rehearse", action="store_true", help="2-rank exchange over gloo on one GPU: a check, not a measurement")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/long_ranks.py runs on the GPU: no device visible")
    if args.rehearse:
        args.reads, args.genome = min(args.reads, 40_000), min(args.genome, 1_000_000)
        print(json.dumps({"bench": "long_ranks_rehearse", "results": [rehearse(k, args) for k in args.k]}))
        return
    print(json.dumps({"bench": "long_ranks", "reads": args.reads, "read_len": args.read_len, "genome": args.genome,
                      "reps": args.reps, "results": [measure(k, args) for k in args.k]}))


if __name__ == "__main__":
    main()
