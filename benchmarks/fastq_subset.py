#!/usr/bin/env python3
"""The informative reads of a FASTQ sample (kdf_fq_extract, ``reads.informative_fastq``), ONE MI355X, one process,
synthetic 150 bp reads with runs of N and mixed qualities:

  kernels   on one chunk (``--chunk-mb``, 64 MiB) of the text resident in HBM, a call that is not the last:
            ``fastq_extract_dev`` at the keep fractions 1e-4, 1e-2, 0.5 and 1.0 (seeded random flags), ``fastq_pack_dev`` on
            the same chunk, and a device-to-device copy of each fraction's ``out_bytes``; the three alternate within a
            repetition, medians of ``--kernel-reps`` (7) with the spread.  Every call ends in the synchronisation that
            returns its sizes.  ``extract_kernels_ms`` is stat fastqextract_us of one more call (HIP events).
  files     on a file of ``--reads`` (10^6) reads, from the page cache: ``informative_fastq`` unpaired and paired (the file
            split into R1 / R2 by alternating reads) against a table that holds one 31-mer of one read in a hundred, and a
            HOST subset writer given the same flags -- read the file, find the line ends with numpy, write the slices of the
            selected records -- which does no selecting of its own.  Device and host alternate, one untimed run of each
            first, medians of ``--file-reps`` (5).  The outputs are compared byte for byte.

One JSON line, also written to ``--out`` (profiles/fastq_subset_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READ_LEN = 150
FRACTIONS = (1e-4, 1e-2, 0.5, 1.0)


def spread(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": len(ts)}


def gbps(nbytes, s):
    return round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 2) if s["median_ms"] else None


def synth(n_reads, seed):
    """-> (bases uint8 (n, 150) over ACGTN, qualities uint8 (n, 150) in '!' .. 'I'): one read in eight has a run of N"""
    import numpy as np
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n_reads, READ_LEN), dtype=np.uint8)]
    for r in np.flatnonzero(rng.integers(0, 8, n_reads) == 0).tolist():
        a = int(rng.integers(0, READ_LEN))
        seq[r, a:a + int(rng.integers(1, 12))] = ord("N")
    return seq, rng.integers(33, 74, (n_reads, READ_LEN), dtype=np.uint8)


def fastq_bytes(seq, qual, first=0, step=1):
    import numpy as np
    n = len(seq)
    names = np.frombuffer(b"".join(b"@r%08d\n" % (first + step * i) for i in range(n)), np.uint8).reshape(n, 11)
    rec = np.empty((n, 11 + READ_LEN + 3 + READ_LEN + 1), np.uint8)
    rec[:, :11] = names
    rec[:, 11:11 + READ_LEN] = seq
    rec[:, 11 + READ_LEN:14 + READ_LEN] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 14 + READ_LEN:14 + 2 * READ_LEN] = qual
    rec[:, -1] = 10
    return rec.tobytes()


def host_subset(src, dst, keep):
    """the host writer: the whole file read, its line ends found with numpy, the slices of the kept records written"""
    import numpy as np
    with open(src, "rb") as f:
        data = f.read()
    ends = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)[3::4] + 1
    starts = np.concatenate([[0], ends[:-1]])
    view = memoryview(data)
    with open(dst, "wb") as g:
        g.write(b"".join(view[a:b] for a, b in zip(starts[keep].tolist(), ends[keep].tolist())))


def same_file(a, b):
    with open(a, "rb") as f, open(b, "rb") as g:
        return f.read() == g.read()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--chunk-mb", type=float, default=64.0)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--kernel-reps", type=int, default=7)
    ap.add_argument("--file-reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--parent", default="", help="the parent commit, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_subset_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/fastq_subset.py measures on the GPU: no device visible")
    if args.kernel_reps < 7 or args.file_reps < 5:
        raise SystemExit("--kernel-reps >= 7 and --file-reps >= 5: a median wants repetitions")
    from kmer_denovo_filter_amd import KmerEngine, reads
    from kmer_denovo_filter_amd._native import FastqState
    k = args.k
    out = {"bench": "fastq_subset", "gpu": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "parent": args.parent, "k": k,
           "workload": "synthetic FASTQ, %d bp reads, LF, runs of N in one read of eight, qualities '!' .. 'I', page cache warm" % READ_LEN, "runs": "one run"}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # ---- kernels: one chunk in HBM ---------------------------------------------------------------------------------------
    rec_bytes = 11 + 2 * READ_LEN + 4
    n_chunk_reads = int(args.chunk_mb * (1 << 20)) // rec_bytes
    seq, qual = synth(n_chunk_reads, 20261021)
    raw = fastq_bytes(seq, qual)
    n = len(raw)
    text = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
    del raw, seq, qual
    eng = KmerEngine(k, capacity_hint=1 << 20)
    pw, mw = reads.stream_words(n // 2)
    packed, invalid = torch.empty(pw, dtype=torch.int64, device="cuda"), torch.empty(mw, dtype=torch.int64, device="cuda")
    dst, other = torch.empty(n + 2, dtype=torch.uint8, device="cuda"), torch.empty(n + 2, dtype=torch.uint8, device="cuda")

    def pack():
        return eng.fastq_pack_dev(text.data_ptr(), n, False, FastqState(), packed.data_ptr(), invalid.data_ptr(), n // 2, None, 0, 0)
    nb, nr, used = pack()
    assert nr == n_chunk_reads and used == n
    out["chunk_bytes"], out["chunk_records"] = n, nr
    rng = np.random.default_rng(7)
    out["kernels"] = {}
    eng.profile(True)
    for frac in FRACTIONS:
        flags = np.ones(nr, np.uint8) if frac >= 1.0 else (rng.random(nr) < frac).astype(np.uint8)
        keep = torch.from_numpy(flags).cuda()

        def extract():
            return eng.fastq_extract_dev(text.data_ptr(), n, False, keep.data_ptr(), nr, dst.data_ptr(), n + 2)
        ob, nk, m = extract()
        assert nk == int(flags.sum()) and ob == nk * rec_bytes and m == n

        def d2d():
            other[:ob].copy_(dst[:ob])
        d2d(); pack()
        t = {"extract": [], "pack": [], "d2d": []}
        for _ in range(args.kernel_reps):                    # the three alternate
            t["extract"].append(wall(extract))
            t["pack"].append(wall(pack))
            t["d2d"].append(wall(d2d))
        u0 = eng.get_stat("fastqextract_us"); extract()
        ek = (eng.get_stat("fastqextract_us") - u0) / 1000.0
        u0 = eng.get_stat("fastqfeed_us"); pack()
        pk = (eng.get_stat("fastqfeed_us") - u0) / 1000.0
        e, p, c = spread(t["extract"]), spread(t["pack"]), spread(t["d2d"])
        out["kernels"]["%g" % frac] = {
            "kept": nk, "out_bytes": ob, "extract": e, "pack": p, "d2d_copy_of_out_bytes": c,
            "extract_kernels_ms": round(ek, 3), "pack_kernels_ms": round(pk, 3),
            "extract_over_pack": round(e["median_ms"] / p["median_ms"], 3), "extract_kernels_over_pack_kernels": round(ek / pk, 3) if pk else None,
            "extract_GBps_of_text": gbps(n, e), "extract_GBps_of_output": gbps(ob, e), "d2d_GBps": gbps(ob, c),
            "extract_over_d2d": round(e["median_ms"] / c["median_ms"], 2) if c["median_ms"] else None}
    eng.profile(False)
    eng.close()
    del text, dst, other, packed, invalid

    # ---- files -----------------------------------------------------------------------------------------------------------
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        seq, qual = synth(args.reads, 20261022)
        fq, r1, r2 = (os.path.join(d, x) for x in ("sample.fastq", "sample_R1.fastq", "sample_R2.fastq"))
        half = args.reads // 2
        with open(fq, "wb") as f:
            f.write(fastq_bytes(seq, qual))
        with open(r1, "wb") as f:
            f.write(fastq_bytes(seq[0:2 * half:2], qual[0:2 * half:2], 0, 2))
        with open(r2, "wb") as f:
            f.write(fastq_bytes(seq[1:2 * half:2], qual[1:2 * half:2], 1, 2))
        out["reads"], out["file_bytes"] = args.reads, os.path.getsize(fq)
        # the table: one k-mer of one read in a hundred, from a stretch without N
        picks = [r for r in range(0, args.reads, 100) if ord("N") not in seq[r, 40:40 + k].tolist()]
        kmers = [seq[r, 40:40 + k].tobytes().decode() for r in picks]
        lo, hi = reads.kmers_to_keys(kmers, k)
        eng = KmerEngine(k, capacity_hint=max(len(lo), 1 << 10))
        eng.add_pairs(lo, hi, np.ones(len(lo), np.uint32))
        del seq, qual
        o_dev, o_host, p1, p2, h1, h2 = (os.path.join(d, x) for x in ("dev.fastq", "host.fastq", "dev_R1.fastq", "dev_R2.fastq", "host_R1.fastq", "host_R2.fastq"))
        res = reads.informative_fastq(eng, fq, [o_dev], min_distinct=1)
        keep = np.zeros(args.reads, bool)
        keep[res[0]["ordinals"]] = True
        resp = reads.informative_fastq(eng, [r1, r2], [p1, p2], min_distinct=1)
        keep_p = np.zeros(half, bool)
        keep_p[resp[0]["ordinals"]] = True
        host_subset(fq, o_host, keep)
        out["kept"], out["kept_pairs"], out["out_bytes"] = int(keep.sum()), int(keep_p.sum()), os.path.getsize(o_dev)
        t = {"unpaired": [], "host": [], "paired": [], "host_paired": []}
        for _ in range(args.file_reps):
            t["unpaired"].append(wall(lambda: reads.informative_fastq(eng, fq, [o_dev], min_distinct=1)))
            t["host"].append(wall(lambda: host_subset(fq, o_host, keep)))
            t["paired"].append(wall(lambda: reads.informative_fastq(eng, [r1, r2], [p1, p2], min_distinct=1)))
            t["host_paired"].append(wall(lambda: (host_subset(r1, h1, keep_p), host_subset(r2, h2, keep_p))))
        out["subset_info"] = dict(reads.LAST_FASTQ_SUBSET)
        for name, ts in t.items():
            out[name] = spread(ts)
        out["unpaired_GBps_of_text"] = gbps(out["file_bytes"], out["unpaired"])
        out["outputs_equal"] = bool(same_file(o_dev, o_host) and same_file(p1, h1) and same_file(p2, h2))
        assert out["outputs_equal"], "the device's output differs from the host writer's"
        eng.close()
    out["not_measured"] = ["a real 30x sample", "long reads", "gzip input (bound by the host's inflate)", "a disk slower than the page cache"]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
