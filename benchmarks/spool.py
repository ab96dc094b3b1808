#!/usr/bin/env python3
"""The read spool (kdf_spool_*) against what it replaces, in ONE run on ONE MI355X.  Prints one JSON line.

  replay   the bench workload (synth.py: 10 M x 150 bp, k = 31) appended in 64 batches, then replay(mode 0) against
           count_dev over the original resident stream: same engine settings, clear + count + flush + synchronise, HIP
           events on the engine's stream, a warm-up and --reps repetitions, best and median.  Replay runs the same kernels
           over the same positions plus one padding tile per batch.
  append   append_dev of the 64 batches (HBM tier) against hipMemcpyDtoD of the same words, GB/s over the batch words; and
           for the host tier (--host-gb > 0) append and replay against a plain pinned D2H / H2D copy of the same bytes.
  chain    (--e2e-reads N > 0) a synthetic N x 150 bp BAM written with the test suite's BAM writer, then
           _extract_child_kmers_discovery under KDF_KEY_PARTS=3 and under KDF_PREFILTER=1, each without and with
           KDF_SPOOL=1: wall seconds and passes through the BAM feeder.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def timed(fn, stream, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        s.record(stream)
        fn()
        e.record(stream)
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return round(min(ts), 3), round(statistics.median(ts), 3)


def cut(ds, n_batches):
    """The resident stream as n_batches device batches cut on tile boundaries (views of its words: a prefix of a longer
    stream is a valid batch, kdf.h "Read streams")."""
    tiles = -(-ds.n_bases // 64)
    per = -(-tiles // n_batches)
    out = []
    for t0 in range(0, tiles, per):
        n = min(per * 64, ds.n_bases - t0 * 64)
        out.append((ds.packed[2 * t0:], ds.invalid[t0:], n))
    return out


def replay_and_append(args, stream):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.spool import ReadSpool
    from kmer_denovo_filter_amd.synth import synth_stream
    ds = synth_stream(args.reads, args.read_len, seed=20260417, device=DEV, genome_seed=20260417)
    torch.cuda.synchronize()
    batches = cut(ds, args.batches)
    words = sum(3 * -(-n // 64) for _, _, n in batches)
    res = {"reads": args.reads, "read_len": args.read_len, "k": args.k, "batches": len(batches), "batch_bytes": words * 8}
    e = KmerEngine(args.k, capacity_hint=1 << 28 if args.reads >= 5_000_000 else max(1 << 16, args.reads * 40))
    e.set_stream(stream.cuda_stream)

    def direct():
        e.clear(); e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases); e.flush()

    def direct_batches():
        e.clear()
        for p, m, n in batches:
            e.count_dev(p.data_ptr(), m.data_ptr(), n)
        e.flush()
    res["direct_ms"], res["direct_median_ms"] = timed(direct, stream, args.reps)
    windows = e.stats()[2]
    res["direct_batches_ms"], res["direct_batches_median_ms"] = timed(direct_batches, stream, args.reps)
    assert e.stats()[2] <= windows                                  # (a cut on a tile boundary may split a read)
    windows_b, distinct_b = e.stats()[2], e.stats()[1]
    sp = ReadSpool(0, 8 << 30, 0)

    def append_all():
        sp.clear()
        for p, m, n in batches:
            sp.append_dev(p.data_ptr(), m.data_ptr(), n, stream.cuda_stream)
    res["append_ms"], res["append_median_ms"] = timed(append_all, stream, args.reps)
    sp.set_option("profile", 1); append_all(); torch.cuda.synchronize()
    res["append_kernel_ms"] = round(sp.stat("append_us") / 1000.0, 3)
    sp.set_option("profile", 0)
    dst = [(torch.empty(2 * -(-n // 64), dtype=torch.int64, device=DEV), torch.empty(-(-n // 64), dtype=torch.int64, device=DEV)) for _, _, n in batches]

    def dtod():
        with torch.cuda.stream(stream):
            for (p, m, n), (dp, dm) in zip(batches, dst):
                dp.copy_(p[:len(dp)], non_blocking=True); dm.copy_(m[:len(dm)], non_blocking=True)
    res["dtod_ms"], res["dtod_median_ms"] = timed(dtod, stream, args.reps)
    res["append_gb_s"] = round(words * 8 / res["append_ms"] / 1e6, 1)
    res["dtod_gb_s"] = round(words * 8 / res["dtod_ms"] / 1e6, 1)
    res.update(segments=sp.stat("segments"), positions=sp.stat("positions"), hbm_bytes=sp.stat("hbm_bytes"))

    def replay():
        e.clear(); sp.replay(e, sp.COUNT); e.flush()
    res["replay_ms"], res["replay_median_ms"] = timed(replay, stream, args.reps)
    assert (e.stats()[2], e.stats()[1]) == (windows_b, distinct_b), "replay and the direct count of the same batches differ"
    res.update(windows=int(windows), windows_batches=int(windows_b),
               replay_over_direct=round(res["replay_ms"] / res["direct_ms"], 4),
               replay_over_direct_batches=round(res["replay_ms"] / res["direct_batches_ms"], 4),
               direct_gkmer_s=round(windows / res["direct_ms"] / 1e6, 1), replay_gkmer_s=round(windows_b / res["replay_ms"] / 1e6, 1))
    sp.close()
    if args.host_gb > 0:
        hs = ReadSpool(0, 0, int(args.host_gb * 1e9))

        def happend():
            hs.clear()
            for p, m, n in batches:
                hs.append_dev(p.data_ptr(), m.data_ptr(), n, stream.cuda_stream)
        res["host_append_ms"], res["host_append_median_ms"] = timed(happend, stream, max(2, args.reps // 2))

        def hreplay():
            e.clear(); hs.replay(e, hs.COUNT); e.flush()
        res["host_replay_ms"], res["host_replay_median_ms"] = timed(hreplay, stream, max(2, args.reps // 2))
        assert (e.stats()[2], e.stats()[1]) == (windows_b, distinct_b)
        res["host_bytes"] = hs.stat("host_bytes")
        hs.close()
        pin = torch.empty(words, dtype=torch.int64).pin_memory()
        src = torch.empty(words, dtype=torch.int64, device=DEV)

        def d2h():
            with torch.cuda.stream(stream):
                pin.copy_(src, non_blocking=True)

        def h2d():
            with torch.cuda.stream(stream):
                src.copy_(pin, non_blocking=True)
        res["pinned_d2h_ms"], res["pinned_d2h_median_ms"] = timed(d2h, stream, args.reps)
        res["pinned_h2d_ms"], res["pinned_h2d_median_ms"] = timed(h2d, stream, args.reps)
    e.close()
    return res


def chain(args):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import write_bam
    from kmer_denovo_filter_amd.discovery import pipeline as P
    tmp = tempfile.mkdtemp(prefix="kdf_spool_bench_")
    path = os.path.join(tmp, "synth.bam")
    rng = np.random.default_rng(1)
    glen = 5 * args.e2e_reads
    genome = rng.integers(0, 4, glen)
    B = np.frombuffer(b"ACGT", np.uint8)
    starts = np.sort(rng.integers(0, glen - 150, args.e2e_reads))
    write_bam(path, [("chr1", glen)], [{"name": f"r{i}", "seq": B[genome[s:s + 150]].tobytes().decode(), "pos": int(s),
                                        "flag": 0x41 if i & 1 else 0x81} for i, s in enumerate(starts)])
    res = {"reads": args.e2e_reads, "bam_bytes": os.path.getsize(path), "threads": args.threads, "runs": []}
    for env in ({"KDF_KEY_PARTS": "3"}, {"KDF_PREFILTER": "1"}):
        fas = []
        for spool in ("0", "1", "0", "1"):                           # (each twice: the first of a kind also warms up)
            for name in ("KDF_KEY_PARTS", "KDF_PREFILTER", "KDF_SPOOL"):
                os.environ.pop(name, None)
            os.environ.update(env, KDF_SPOOL=spool)
            out = tempfile.mkdtemp(dir=tmp)
            t = time.monotonic()
            fa, n = P._extract_child_kmers_discovery(path, None, 31, 3, args.threads, out)
            dt = time.monotonic() - t
            fas.append(open(fa, "rb").read())
            res["runs"].append(dict(env, KDF_SPOOL=spool, seconds=round(dt, 3), candidates=n, **P.LAST_CHILD_SPOOL))
        assert all(f == fas[0] for f in fas), "the candidate FASTA differs with the spool"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-gb", type=float, default=2.0, help="host-tier budget of the host-tier measurements (0: skip them)")
    ap.add_argument("--e2e-reads", type=int, default=4_000_000, help="reads of the synthetic BAM of the chain measurement (0: skip it)")
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/spool.py measures on the GPU: no device visible")
    stream = torch.cuda.Stream()
    out = {"bench": "spool", "device": torch.cuda.get_device_name(0), "workload": "synth", "stream": replay_and_append(args, stream)}
    if args.e2e_reads:
        out["chain"] = chain(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
