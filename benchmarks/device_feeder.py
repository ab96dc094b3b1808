#!/usr/bin/env python3
"""The device BAM feeder (KDF_DEVICE_FEEDER=1: BGZF inflate, record walk and packing on the GPU) against the host
feeder at --threads host threads, in ONE run on ONE MI355X, on the synthetic BAM benchmarks/spool.py also writes.
Prints one JSON line.

  host     the count pass of the file through the host feeder (zlib inflate + parser threads + H2D of the packed
           stream): wall seconds from the first byte to the flushed table, best of --reps after a warm-up.
  device   the same pass through reads.stream_bam_device for each --subrange-mb: wall seconds, the table asserted equal to
           the host feeder's (sorted export), then one more pass under kdf_profile for the HIP-event time of inflate /
           walk / pack per batch, with the planner's host seconds, the H2D bytes and the fallback and replay counts.
The yardstick is the host feeder of the same run; no figure is fixed in advance.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_synth_bam(path, n_reads):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import write_bam
    rng = np.random.default_rng(1)
    glen = 5 * n_reads
    genome = rng.integers(0, 4, glen)
    B = np.frombuffer(b"ACGT", np.uint8)
    starts = np.sort(rng.integers(0, glen - 150, n_reads))
    write_bam(path, [("chr1", glen)], [{"name": f"r{i}", "seq": B[genome[s:s + 150]].tobytes().decode(), "pos": int(s),
                                        "flag": 0x41 if i & 1 else 0x81} for i, s in enumerate(starts)])


def table(eng):
    import numpy as np
    lo, hi, cnt = eng.export_ge(0)
    o = np.argsort(lo, kind="stable")
    return lo[o], cnt[o]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--subrange-mb", type=float, nargs="+", default=[0.0625, 0.25, 1.0, 4.0])
    ap.add_argument("--comp-mb", type=int, default=64, help="compressed bytes per batch of the device feeder")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/device_feeder.py measures on the GPU: no device visible")
    from kmer_denovo_filter_amd import KmerEngine, reads as R
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as jw
    tmp = tempfile.mkdtemp(prefix="kdf_feeder_bench_")
    path = os.path.join(tmp, "synth.bam")
    t = time.monotonic()
    write_synth_bam(path, args.reads)
    bases = args.reads * 150
    out = {"bench": "device_feeder", "device": torch.cuda.get_device_name(0), "reads": args.reads, "bases": bases, "k": args.k,
           "bam_bytes": os.path.getsize(path), "bam_write_seconds": round(time.monotonic() - t, 1), "threads": args.threads}
    os.environ.pop("KDF_DEVICE_FEEDER", None)
    hint = max(1 << 20, 6 * args.reads)

    def host_pass(eng):
        eng.clear()
        t0 = time.perf_counter()
        n = jw._stream_bam(eng, path, None, args.threads, filtered=False)
        eng.flush(); eng.synchronize()
        return time.perf_counter() - t0, n

    with KmerEngine(args.k, capacity_hint=hint) as eng:
        host_pass(eng)                                               # warm-up: pinned buffers, kernels, page cache
        ts = [host_pass(eng) for _ in range(args.reps)]
        want_reads = ts[0][1]
        out["host"] = {"seconds": round(min(x for x, _ in ts), 4), "gbase_s": round(bases / min(x for x, _ in ts) / 1e9, 3),
                       "pipelines": jw._reader_pipelines(args.threads)}
        want = table(eng)
        want_stats = eng.stats()
    local = jw._reader_pipelines(args.threads)
    parts = [(j, local) for j in range(local)]
    out["device"] = []
    for mb in args.subrange_mb:
        sub = int(mb * (1 << 20))

        def dev_pass(eng):
            eng.clear()
            t0 = time.perf_counter()
            n = R.stream_bam_device(eng, path, parts, subrange_bytes=sub, comp_cap=args.comp_mb << 20, producers=min(args.threads, 16))
            eng.flush(); eng.synchronize()
            return time.perf_counter() - t0, n

        with KmerEngine(args.k, capacity_hint=hint) as eng:
            dev_pass(eng)
            ts = [dev_pass(eng) for _ in range(args.reps)]
            assert all(n == want_reads for _, n in ts), "the device feeder yields another number of reads"
            assert eng.stats() == want_stats
            got = table(eng)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "the device feeder's table differs"
            info = dict(R.LAST_FEEDER)
            eng.profile(True)
            dev_pass(eng)
            nb = max(1, R.LAST_FEEDER["batches"])
            stage = {s: round(eng.get_stat(f"bamdev_{s}_us") / 1000.0 / nb, 3) for s in ("inflate", "walk", "pack")}
            eng.profile(False)
            best = min(x for x, _ in ts)
            out["device"].append({"subrange_mb": mb, "seconds": round(best, 4), "gbase_s": round(bases / best / 1e9, 3),
                                  "over_host": round(out["host"]["seconds"] / best, 3), "batches": info["batches"],
                                  "subranges": info["subranges"], "ms_per_batch": stage, "plan_seconds": round(info["plan_seconds"], 4),
                                  "h2d_bytes": info["h2d_bytes"], "fallback_blocks": info["fallback_blocks"], "replays": info["replays"]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
