#!/usr/bin/env python3
"""The device FASTA feeder (kdf_fasta_pack_dev, ``reads.stream_fasta_device``) against the host FASTA leg it stands beside
(``fasta_reader`` + ``count``: what ``_count_fasta_to_index`` does by default), ONE MI355X, one synthetic multi-FASTA of
``--mb`` MiB in a temporary directory (60-column lines, LF, ``--records`` records, N runs), everything in one run:

  host     ``fasta_reader(path, k)`` batches into ``engine.count`` -- one thread, gzgets, a push_back and a put per base
  device   ``stream_fasta_device(engine, path, k)`` end to end: read() into page-locked buffers, upload, pack, count_dev
  pack     ``fasta_pack_dev`` alone over one chunk of the text resident in HBM (one call: it ends in the synchronisation
           that returns the sizes), as GB/s of text, against a device-to-device copy of the same bytes

Host and device alternate, one untimed run of each first, medians of ``--reps`` with the spread; the file was written a
moment before, so it is read from the page cache on both sides.  The two tables are compared key by key and count by count
after the last repetition.  ``pack_kernels_ms`` is stat fastafeed_us of one more call (HIP events).  One JSON line, also
written to ``--out`` (profiles/fasta_feeder_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": len(ts)}


def gbps(nbytes, s):
    return round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 2)


def write_fasta(path, mb, records, seed):
    """-> bytes written.  60 bases + LF per line; every record has a few runs of N."""
    import numpy as np
    rng = np.random.default_rng(seed)
    lines_total = (mb << 20) // 61
    per = lines_total // records
    with open(path, "wb") as f:
        for r in range(records):
            f.write(b">chr%d synthetic\n" % (r + 1))
            a = np.empty((per, 61), np.uint8)
            a[:, :60] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (per, 60), dtype=np.uint8)]
            a[:, 60] = 10
            for _ in range(4):                                       # N runs of 1 .. 50 000 bases (whole lines)
                s = int(rng.integers(0, per))
                a[s:s + int(rng.integers(1, 50_000 // 60 + 2)), :60] = ord("N")
            f.write(a.tobytes())
        return f.tell()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256, help="size of the synthetic FASTA in MiB")
    ap.add_argument("--records", type=int, default=24)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5, help="repetitions of each path (host and device alternate)")
    ap.add_argument("--pack-reps", type=int, default=9)
    ap.add_argument("--dir", default=None, help="where the FASTA is written (default: a temporary directory)")
    ap.add_argument("--parent", default="", help="the parent commit, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_feeder_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/fasta_feeder.py measures on the GPU: no device visible")
    if args.reps < 5:
        raise SystemExit("--reps >= 5: a median wants repetitions")
    from kmer_denovo_filter_amd import KmerEngine, reads
    from kmer_denovo_filter_amd._native import FastaState
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import BATCH_BASES
    k = args.k
    out = {"bench": "fasta_feeder", "gpu": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "parent": args.parent, "k": k,
           "workload": "synthetic multi-FASTA, 60-column lines, LF, N runs, page cache warm", "records": args.records,
           "feed_mb": int(float(os.environ.get("KDF_FASTA_FEED_MB", "64")))}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "synthetic.fa")
        out["text_bytes"] = nbytes = write_fasta(path, args.mb, args.records, 20261021)
        host_eng = KmerEngine(k, capacity_hint=nbytes)
        dev_eng = KmerEngine(k, capacity_hint=nbytes)

        def host():
            host_eng.clear()
            with reads.fasta_reader(path, k, max_bases=BATCH_BASES) as rd:
                for batch in rd:
                    host_eng.count(batch)
            host_eng.synchronize()

        def device():
            dev_eng.clear()
            n = reads.stream_fasta_device(dev_eng, path, k)
            dev_eng.synchronize()
            assert n == args.records

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        host(); device()
        t = {"host": [], "device": []}
        for _ in range(args.reps):
            t["host"].append(wall(host))
            t["device"].append(wall(device))
        out["host"], out["device"] = spread(t["host"]), spread(t["device"])
        out["host_MBps"], out["device_MBps"] = round(gbps(nbytes, out["host"]) * 1e3), round(gbps(nbytes, out["device"]) * 1e3)
        out["host_over_device"] = round(out["host"]["median_ms"] / out["device"]["median_ms"], 2)
        out["feeder"] = {x: reads.LAST_FASTA_FEEDER[x] for x in ("chunks", "bytes", "carries", "records", "positions")}
        a, b = host_eng.export_ge(0), dev_eng.export_ge(0)
        same = all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))
        assert same, "the device path's table differs from the host path's"
        out["tables_equal"], out["distinct"] = True, int(len(a[0]))
        del a, b
        host_eng.close()

        # the pack alone: one chunk of the text in HBM
        n = min(nbytes, out["feed_mb"] << 20)
        with open(path, "rb") as f:
            text = torch.from_numpy(np.frombuffer(f.read(n), np.uint8).copy()).cuda()
        other = torch.empty_like(text)
        pw, mw = reads.stream_words(n + 1)
        packed, invalid = torch.empty(pw, dtype=torch.int64, device="cuda"), torch.empty(mw, dtype=torch.int64, device="cuda")

        def pack():
            dev_eng.fasta_pack_dev(text.data_ptr(), n, True, FastaState(), packed.data_ptr(), invalid.data_ptr(), n + 1)
        pack(); other.copy_(text)
        out["pack_bytes"] = n
        out["pack"] = spread([wall(pack) for _ in range(args.pack_reps)])
        out["d2d_copy"] = spread([wall(lambda: other.copy_(text)) for _ in range(args.pack_reps)])
        out["pack_GBps"], out["d2d_copy_GBps"] = gbps(n, out["pack"]), gbps(n, out["d2d_copy"])
        dev_eng.profile(True)
        u0 = dev_eng.get_stat("fastafeed_us"); pack()
        out["pack_kernels_ms"] = round((dev_eng.get_stat("fastafeed_us") - u0) / 1000.0, 3)
        out["pack_kernels_GBps"] = round(n / (out["pack_kernels_ms"] * 1e-3) / 1e9, 2) if out["pack_kernels_ms"] else None
        dev_eng.profile(False)
        dev_eng.close()
    out["not_measured"] = ["a real 3 GB reference", "a slow disk (the file is in the page cache)", "a gzip or BGZF reference", "CRLF or unwrapped lines"]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
