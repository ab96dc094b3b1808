#!/usr/bin/env python3
"""The device FASTQ feeder (kdf_fastq_pack, ``reads.stream_fastq_device``) against the default host BAM leg it spares a
parent (``bam_reader`` + ``count``), ONE MI355X, one process, one synthetic sample of ``--reads`` x 150 bp reads with runs of
N and mixed qualities, written to a temporary directory as FASTQ, as gzip FASTQ, as a FASTA of the same sequences and as a
BAM of the same reads:

  pack      ``fastq_pack_dev`` alone over one chunk (``KDF_FASTQ_FEED_MB``, 64 MiB) of the text resident in HBM, a call that is
            not the last (it takes the whole records of the chunk and ends in the synchronisation that returns the sizes),
            with ``min_qual`` 0 and set; as GB/s of text, against a device-to-device copy of the same bytes and against
            ``fasta_pack_dev`` (the closest existing kernel) on the FASTA of the same sequences
  device    ``stream_fastq_device(engine, path)`` end to end: read() into page-locked buffers, upload, pack, count_dev
  host      ``bam_reader(bam)`` batches into ``engine.count``: the default feeder of ``_stream_bam_pass``
  gzip      ``stream_fastq_device`` on the gzip file: the text is inflated by ONE host thread (zlib)

Host and device alternate, one untimed run of each first, medians of ``--reps`` with the spread; the files were written a
moment before, so they are read from the page cache.  The two tables are compared key by key and count by count after the
last repetition.  ``pack_kernels_ms`` is stat fastqfeed_us of one more call (HIP events).  One JSON line, also written to
``--out`` (profiles/fastq_feeder_bench.json)."""
import argparse
import gzip
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READ_LEN = 150


def spread(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": len(ts)}


def gbps(nbytes, s):
    return round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 2)


def synth(n_reads, seed):
    """-> (bases uint8 (n, 150) over ACGTN, qualities uint8 (n, 150) in '!' .. 'I'): one read in eight has a run of N"""
    import numpy as np
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n_reads, READ_LEN), dtype=np.uint8)]
    for r in np.flatnonzero(rng.integers(0, 8, n_reads) == 0).tolist():
        a = int(rng.integers(0, READ_LEN))
        seq[r, a:a + int(rng.integers(1, 12))] = ord("N")
    return seq, rng.integers(33, 74, (n_reads, READ_LEN), dtype=np.uint8)


def write_fastq(path, seq, qual):
    import numpy as np
    n = len(seq)
    names = np.frombuffer(b"".join(b"@r%08d\n" % i for i in range(n)), np.uint8).reshape(n, 11)
    rec = np.empty((n, 11 + READ_LEN + 3 + READ_LEN + 1), np.uint8)
    rec[:, :11] = names
    rec[:, 11:11 + READ_LEN] = seq
    rec[:, 11 + READ_LEN:14 + READ_LEN] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 14 + READ_LEN:14 + 2 * READ_LEN] = qual
    rec[:, -1] = 10
    with open(path, "wb") as f:
        f.write(rec.tobytes())
    return rec.size


def write_fasta(path, seq):
    import numpy as np
    n = len(seq)
    rec = np.empty((n, 3 + READ_LEN + 1), np.uint8)
    rec[:, :3] = np.frombuffer(b">r\n", np.uint8)
    rec[:, 3:3 + READ_LEN] = seq
    rec[:, -1] = 10
    with open(path, "wb") as f:
        f.write(rec.tobytes())
    return rec.size


def write_bam(path, seq, qual):
    """the same reads as unaligned-looking single-end records (flag 0, one 150M CIGAR), BGZF blocks of 60 000 bytes"""
    import numpy as np
    n = len(seq)
    nt16 = np.zeros(256, np.uint8)
    for ch, v in zip(b"ACGTN", (1, 2, 4, 8, 15)):
        nt16[ch] = v
    nib = nt16[seq]
    name_len, body = 10, 32 + 10 + 4 + READ_LEN // 2 + READ_LEN
    rec = np.zeros((n, 4 + body), np.uint8)
    fixed = struct.pack("<iiiBBHHHiiii", body, 0, 0, name_len, 60, 4680, 1, 0, READ_LEN, -1, -1, 0)
    rec[:, :36] = np.frombuffer(fixed, np.uint8)
    rec[:, 8:12] = (np.arange(n, dtype="<i4") * 5).view(np.uint8).reshape(n, 4)           # pos
    rec[:, 36:46] = np.frombuffer(b"".join(b"r%08d\0" % i for i in range(n)), np.uint8).reshape(n, 10)
    rec[:, 46:50] = np.frombuffer(struct.pack("<I", READ_LEN << 4), np.uint8)
    rec[:, 50:50 + READ_LEN // 2] = nib[:, 0::2] << 4 | nib[:, 1::2]
    rec[:, 50 + READ_LEN // 2:] = qual - 33
    text = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:%d\n" % (5 * n + READ_LEN)
    head = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chr1\0" + struct.pack("<i", 5 * n + READ_LEN)
    data = head + rec.tobytes()
    with open(path, "wb") as f:
        for a in list(range(0, len(data), 60000)) + [len(data)]:
            raw = data[a:a + 60000]
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            comp = c.compress(raw) + c.flush()
            f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(raw), len(raw)))
    return os.path.getsize(path)


def table(eng):
    import numpy as np
    lo, hi, cnt = eng.export_ge(0)
    o = np.argsort(lo, kind="stable")
    return lo[o], cnt[o]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--min-qual", type=int, default=53, help="the quality byte below which the second pack run masks (the middle of '!' .. 'I')")
    ap.add_argument("--reps", type=int, default=5, help="repetitions of each path (host and device alternate)")
    ap.add_argument("--pack-reps", type=int, default=9)
    ap.add_argument("--threads", type=int, default=4, help="inflate threads of the host BAM reader")
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--parent", default="", help="the parent commit, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_feeder_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/fastq_feeder.py measures on the GPU: no device visible")
    if args.reps < 5:
        raise SystemExit("--reps >= 5: a median wants repetitions")
    from kmer_denovo_filter_amd import KmerEngine, reads
    from kmer_denovo_filter_amd._native import FastaState, FastqState
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import BATCH_BASES
    k = args.k
    feed = int(float(os.environ.get("KDF_FASTQ_FEED_MB", "64")) * (1 << 20))
    out = {"bench": "fastq_feeder", "gpu": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "parent": args.parent, "k": k,
           "workload": "synthetic FASTQ, %d x %d bp, LF, runs of N in one read of eight, qualities '!' .. 'I', page cache warm" % (args.reads, READ_LEN),
           "reads": args.reads, "feed_bytes": feed, "runs": "one run"}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        seq, qual = synth(args.reads, 20261021)
        fq, fa, bam, gz = (os.path.join(d, n) for n in ("sample.fastq", "sample.fa", "sample.bam", "sample.fastq.gz"))
        out["text_bytes"] = nbytes = write_fastq(fq, seq, qual)
        out["fasta_bytes"] = write_fasta(fa, seq)
        out["bam_bytes"] = write_bam(bam, seq, qual)
        with open(fq, "rb") as f, gzip.open(gz, "wb", compresslevel=1) as g:
            while True:
                piece = f.read(1 << 24)
                if not piece:
                    break
                g.write(piece)
        out["gzip_bytes"] = os.path.getsize(gz)
        del seq, qual
        host_eng = KmerEngine(k, capacity_hint=nbytes // 2)
        dev_eng = KmerEngine(k, capacity_hint=nbytes // 2)

        def host():
            host_eng.clear()
            with reads.bam_reader(bam, max_bases=BATCH_BASES, max_reads=1 << 21, threads=args.threads) as rd:
                for batch in rd:
                    host_eng.count(batch)
            host_eng.synchronize()

        def device(path=fq):
            dev_eng.clear()
            n = reads.stream_fastq_device(dev_eng, path)
            dev_eng.synchronize()
            assert n == args.reads

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
        out["host_bam"], out["device"] = spread(t["host"]), spread(t["device"])
        out["device_GBps_of_text"] = gbps(nbytes, out["device"])
        out["host_over_device"] = round(out["host_bam"]["median_ms"] / out["device"]["median_ms"], 2)
        out["feeder"] = {x: reads.LAST_FASTQ_FEEDER[x] for x in ("chunks", "bytes", "records", "positions")}
        a, b = table(host_eng), table(dev_eng)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the FASTQ path's table differs from the BAM path's"
        out["tables_equal"], out["distinct"] = True, int(len(a[0]))
        del a, b
        host_eng.close()
        device(gz)
        out["device_gzip"] = spread([wall(lambda: device(gz)) for _ in range(3)])
        t0 = time.perf_counter()
        with open(gz, "rb") as f:
            z = zlib.decompressobj(31)
            while True:
                piece = f.read(1 << 20)
                if not piece:
                    break
                z.decompress(piece)
        out["gzip_inflate_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)

        # the pack alone: one chunk of the text in HBM
        n = min(nbytes, feed)
        with open(fq, "rb") as f:
            text = torch.from_numpy(np.frombuffer(f.read(n), np.uint8).copy()).cuda()
        other = torch.empty_like(text)
        pw, mw = reads.stream_words(n // 2)
        packed, invalid = torch.empty(pw, dtype=torch.int64, device="cuda"), torch.empty(mw, dtype=torch.int64, device="cuda")

        def pack(mq=0):
            return dev_eng.fastq_pack_dev(text.data_ptr(), n, False, FastqState(), packed.data_ptr(), invalid.data_ptr(), n // 2, None, 0, mq)
        nb, nr, used = pack(); other.copy_(text)
        out["pack_bytes"], out["pack_records"], out["pack_positions"], out["pack_consumed"] = n, nr, nb, used
        out["pack"] = spread([wall(pack) for _ in range(args.pack_reps)])
        out["pack_min_qual"] = spread([wall(lambda: pack(args.min_qual)) for _ in range(args.pack_reps)])
        out["d2d_copy"] = spread([wall(lambda: other.copy_(text)) for _ in range(args.pack_reps)])
        out["pack_GBps"], out["pack_min_qual_GBps"], out["d2d_copy_GBps"] = gbps(n, out["pack"]), gbps(n, out["pack_min_qual"]), gbps(n, out["d2d_copy"])
        dev_eng.profile(True)
        for name, mq in (("pack_kernels_ms", 0), ("pack_min_qual_kernels_ms", args.min_qual)):
            u0 = dev_eng.get_stat("fastqfeed_us"); pack(mq)
            out[name] = round((dev_eng.get_stat("fastqfeed_us") - u0) / 1000.0, 3)
        out["pack_kernels_GBps"] = round(n / (out["pack_kernels_ms"] * 1e-3) / 1e9, 2) if out["pack_kernels_ms"] else None
        dev_eng.profile(False)
        del text, other
        # the closest existing kernel on the same sequences
        m = min(out["fasta_bytes"], feed)
        with open(fa, "rb") as f:
            ftext = torch.from_numpy(np.frombuffer(f.read(m), np.uint8).copy()).cuda()
        fpw, fmw = reads.stream_words(m + 1)
        fpacked, finvalid = torch.empty(fpw, dtype=torch.int64, device="cuda"), torch.empty(fmw, dtype=torch.int64, device="cuda")

        def fasta_pack():
            return dev_eng.fasta_pack_dev(ftext.data_ptr(), m, True, FastaState(), fpacked.data_ptr(), finvalid.data_ptr(), m + 1)
        out["fasta_pack_positions"] = fasta_pack()[0]
        out["fasta_pack_bytes"] = m
        out["fasta_pack"] = spread([wall(fasta_pack) for _ in range(args.pack_reps)])
        out["fasta_pack_GBps"] = gbps(m, out["fasta_pack"])
        out["pack_Gpositions_per_s"] = round(nb / (out["pack"]["median_ms"] * 1e-3) / 1e9, 2)
        out["fasta_pack_Gpositions_per_s"] = round(out["fasta_pack_positions"] / (out["fasta_pack"]["median_ms"] * 1e-3) / 1e9, 2)
        dev_eng.close()
    out["not_measured"] = ["a real 30x sample", "long reads", "a disk slower than the page cache", "CRLF text", "jellyfish count -Q itself (no binary here)"]
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
