#!/usr/bin/env python3
"""The per-read consumers over a read spool (kdf_spool_read_hits / read_depth / select_reads) against what they
replace, in ONE run on ONE MI355X.  Prints one JSON line.

  replay   the bench workload (synth.py: 10 M x 150 bp, k = 31) appended with its read offsets in 64 batches cut on read
           boundaries, then spool.read_hits / spool.read_depth against read_hits_dev / read_depth_dev over the ORIGINAL
           resident stream with its own offsets: same engine, same table (the k-mers of the first batch), HIP events on the
           engine's stream, a warm-up and --reps repetitions, best and median.  The replay runs the same kernels plus one
           padding tile per batch and one call per segment; the direct figure is the baseline and the rows must be equal.
  append   append_dev with offsets against append_dev without, same batches; under `profile` the offsets kernel and the
           append kernel alone.  The offsets are 8 bytes per read against about 57 per 150-bp read of stream.
  select   select_reads over the rows on the device against copying the rows to the host and numpy there: wall time.
"""
import argparse
import json
import os
import statistics
import sys
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


def walled(fn, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(min(ts), 3), round(statistics.median(ts), 3)


def cut_reads(ds, n_batches):
    """The resident stream as device batches of whole reads.  Every read takes read_len + 1 positions; a batch starts on
    a tile boundary when its first read is a multiple of 64.  -> [(packed, invalid, n_bases, first_read, n_reads)]"""
    stride = ds.read_len + 1
    per = -(-(-(-ds.n_reads // n_batches)) // 64) * 64
    out = []
    for r0 in range(0, ds.n_reads, per):
        nr = min(per, ds.n_reads - r0)
        t0 = r0 * stride // 64
        out.append((ds.packed[2 * t0:], ds.invalid[t0:], nr * stride, r0, nr))
    return out


def run(args, stream):
    import numpy as np
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.spool import ReadSpool
    from kmer_denovo_filter_amd.synth import synth_stream
    ds = synth_stream(args.reads, args.read_len, seed=20260417, device=DEV, genome_seed=20260417)
    stride = ds.read_len + 1
    assert ds.n_bases == ds.n_reads * stride
    offs = torch.arange(ds.n_reads + 1, dtype=torch.int64, device=DEV) * stride
    batches = cut_reads(ds, args.batches)
    boffs = [torch.arange(nr + 1, dtype=torch.int64, device=DEV) * stride for _, _, _, _, nr in batches]
    torch.cuda.synchronize()
    res = {"reads": ds.n_reads, "read_len": ds.read_len, "k": args.k, "batches": len(batches)}
    e = KmerEngine(args.k, capacity_hint=max(1 << 16, batches[0][2] * 2))
    e.set_stream(stream.cuda_stream)
    e.count_dev(batches[0][0].data_ptr(), batches[0][1].data_ptr(), batches[0][2]); e.flush()
    res["table_keys"] = e.stats()[1]

    # (b) append with and without offsets
    sp = ReadSpool(0, 8 << 30, 0)

    def append_plain():
        sp.clear()
        for p, m, n, _, _ in batches:
            sp.append_dev(p.data_ptr(), m.data_ptr(), n, stream.cuda_stream)

    def append_reads():
        sp.clear()
        for (p, m, n, _, nr), o in zip(batches, boffs):
            sp.append_dev(p.data_ptr(), m.data_ptr(), n, stream.cuda_stream, d_offsets=o.data_ptr(), n_reads=nr)
    res["append_ms"], res["append_median_ms"] = timed(append_plain, stream, args.reps)
    res["append_reads_ms"], res["append_reads_median_ms"] = timed(append_reads, stream, args.reps)
    sp.set_option("profile", 1); append_reads(); torch.cuda.synchronize()
    res["append_kernel_ms"] = round(sp.stat("append_us") / 1000.0, 3)
    res["offsets_kernel_ms"] = round(sp.stat("offsets_us") / 1000.0, 3)
    sp.set_option("profile", 0)
    res["append_reads_over_append"] = round(res["append_reads_ms"] / res["append_ms"], 4)
    res.update(segments=sp.stat("segments"), hbm_bytes=sp.stat("hbm_bytes"), offset_bytes=sp.stat("offset_bytes"), spool_reads=sp.n_reads)

    # (a) replay against the direct call over the original stream
    rows_d = torch.zeros(ds.n_reads, dtype=torch.int64, device=DEV)
    rows_s = torch.zeros(ds.n_reads, dtype=torch.int64, device=DEV)
    depth_d = torch.zeros(ds.n_reads * 6, dtype=torch.int64, device=DEV)
    depth_s = torch.zeros(ds.n_reads * 6, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    res["hits_direct_ms"], res["hits_direct_median_ms"] = timed(
        lambda: e.read_hits_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases, offs.data_ptr(), ds.n_reads, None, rows_d.data_ptr()),
        stream, args.reps)
    res["hits_replay_ms"], res["hits_replay_median_ms"] = timed(lambda: sp.read_hits_dev(e, rows_s.data_ptr()), stream, args.reps)
    res["depth_direct_ms"], res["depth_direct_median_ms"] = timed(
        lambda: e.read_depth_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases, offs.data_ptr(), ds.n_reads, args.low_max, depth_d.data_ptr()),
        stream, args.reps)
    res["depth_replay_ms"], res["depth_replay_median_ms"] = timed(lambda: sp.read_depth_dev(e, args.low_max, depth_s.data_ptr()), stream, args.reps)
    torch.cuda.synchronize()
    assert torch.equal(rows_d, rows_s), "read_hits over the spool and over the original stream differ"
    assert torch.equal(depth_d, depth_s), "read_depth over the spool and over the original stream differ"
    res["hits_replay_over_direct"] = round(res["hits_replay_ms"] / res["hits_direct_ms"], 4)
    res["depth_replay_over_direct"] = round(res["depth_replay_ms"] / res["depth_direct_ms"], 4)

    # (c) select on the device against rows to the host + numpy
    out = torch.zeros(ds.n_reads, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    got = {}

    def select_dev():
        rc, n = sp.select_reads_dev(rows_s.data_ptr(), args.min_distinct, out.data_ptr(), ds.n_reads)
        assert rc == 0
        got["dev"] = out[:n].cpu().numpy()

    def select_host():
        rows = rows_s.cpu().numpy().view(np.uint32).reshape(-1, 2)
        got["host"] = np.flatnonzero(rows[:, 1] >= args.min_distinct)
    res["select_dev_ms"], res["select_dev_median_ms"] = walled(select_dev, args.reps)
    res["select_host_ms"], res["select_host_median_ms"] = walled(select_host, args.reps)
    assert np.array_equal(got["dev"], got["host"]), "select_reads and numpy differ"
    res.update(selected=int(len(got["dev"])), min_distinct=args.min_distinct,
               select_dev_over_host=round(res["select_dev_ms"] / res["select_host_ms"], 4))
    sp.close(); e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--low-max", type=int, default=0)
    ap.add_argument("--min-distinct", type=int, default=1)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/spool_reads.py measures on the GPU: no device visible")
    stream = torch.cuda.Stream()
    print(json.dumps({"bench": "spool_reads", "device": torch.cuda.get_device_name(0), "workload": "synth", "reads_replay": run(args, stream)}))


if __name__ == "__main__":
    main()
