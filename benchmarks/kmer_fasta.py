#!/usr/bin/env python3
"""The k-mer FASTA codec on the device (kdf_format_kmers_dev, kdf_parse_kmer_fasta_dev and the two wrappers of
``kmer_fasta.py``) against the host codec it stands beside, ONE MI355X, the same random canonical key sets of ``--n`` keys
at every k of ``--ks`` on both sides, everything in one run:

  format   the format kernel alone, the whole text into one device buffer, against a device-to-device copy of the same
           number of bytes (the floor of anything that writes that text once)
  write    ``write_kmer_fasta_device`` (format -> pinned buffers -> ``write()``, sidecar included) against
           ``devkeys.to_host`` + ``write_kmer_fasta``, alternating, into ``--dir`` (the same directory for both)
  parse    the parse kernels alone over the text in device memory (one call: it ends in the synchronisation that
           returns the number of keys)
  read     ``read_kmer_fasta_keys_device`` against ``read_kmer_fasta_keys``, the sidecar removed, alternating; both
           results compared key by key.  ``--n`` is chosen so that the host parser's (n, k) int64 gather index fits host
           memory (2 M keys: 1.6 GB at k = 101); the JSON says which n ran.

Wall clock around work that ends in a synchronisation, warm (one untimed run of each first), median of ``--reps`` with the
spread; ``kernels_ms`` is stat kmerfasta_us of one more call (HIP events).  One JSON line, also written to
profiles/kmer_fasta_bench.json."""
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


def gbps(nbytes, s):
    return round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 2)


def case(k, n, reps, file_reps, out_dir, seed):
    import numpy as np
    import torch
    from kmer_denovo_filter_amd import KmerEngine, devkeys, keys, kmer_fasta
    from kmer_denovo_filter_amd.engine import TEXT_FASTA

    rng = np.random.default_rng(seed)
    words = keys.from_codes(rng.integers(0, 4, (n, k), dtype=np.uint8), canonical=True)
    lo, hi = keys.to_pair(words, zero_hi=False)
    W = keys.n_words(k)
    dlo, dhi = devkeys.from_host(lo, hi, W == 2)
    eng = KmerEngine(31, capacity_hint=1 << 10)                       # (the table is not used: any engine serves)
    total = eng.kmer_text_bytes(k, TEXT_FASTA, 0, n)
    text = torch.empty(total, dtype=torch.uint8, device="cuda")
    other = torch.empty(total, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr() if t is not None else None
    out = {"k": k, "words": W, "n": n, "text_bytes": total}

    # format: the kernel alone against a copy of the same bytes
    def fmt():
        eng.format_kmers_dev(p(dlo), p(dhi), n, k, TEXT_FASTA, 0, 0, total, text.data_ptr())
        eng.synchronize()
    fmt(); other.copy_(text)
    out["format"] = spread(wall(fmt, reps))
    out["d2d_copy"] = spread(wall(lambda: other.copy_(text), reps))
    out["format_GBps"], out["d2d_copy_GBps"] = gbps(total, out["format"]), gbps(total, out["d2d_copy"])
    eng.profile(True)
    u0 = eng.get_stat("kmerfasta_us"); fmt()
    out["format_kernels_ms"] = round((eng.get_stat("kmerfasta_us") - u0) / 1000.0, 3)

    # parse: the kernels alone over the text in device memory
    plo = torch.empty((n, W) if W > 2 else n, dtype=torch.int64, device="cuda")
    phi = torch.empty(n, dtype=torch.int64, device="cuda") if W == 2 else None

    def parse():
        got = eng.parse_kmer_fasta_dev(text.data_ptr(), total, k, True, True, plo.data_ptr(), p(phi), n)
        assert got == (n, total)
    parse()
    assert torch.equal(plo, dlo) and (phi is None or torch.equal(phi, dhi)), f"k={k}: the parsed keys differ from the formatted ones"
    out["parse"] = spread(wall(parse, reps))
    out["parse_GBps"] = gbps(total, out["parse"])
    u0 = eng.get_stat("kmerfasta_us"); parse()
    out["parse_kernels_ms"] = round((eng.get_stat("kmerfasta_us") - u0) / 1000.0, 3)
    eng.profile(False)
    del text, other, plo, phi

    # write and read: the wrappers against the host codec, alternating, in one directory
    host_fa, dev_fa = os.path.join(out_dir, f"host_k{k}.fa"), os.path.join(out_dir, f"dev_k{k}.fa")

    def host_write():
        kmer_fasta.write_kmer_fasta(host_fa, *devkeys.to_host(dlo, dhi), k)

    def dev_write():
        kmer_fasta.write_kmer_fasta_device(dev_fa, dlo, dhi, k, engine=eng)
    host_write(); dev_write()
    tw = {"host": [], "device": []}
    for _ in range(file_reps):
        tw["host"] += wall(host_write, 1)
        tw["device"] += wall(dev_write, 1)
    with open(host_fa, "rb") as a, open(dev_fa, "rb") as b:
        same = True
        while same:
            x, y = a.read(1 << 24), b.read(1 << 24)
            same = x == y
            if not x:
                break
    assert same, f"k={k}: the device writer's file differs from the host writer's"
    out["write_host"], out["write_device"] = spread(tw["host"]), spread(tw["device"])
    out["write_host_over_device"] = round(out["write_host"]["median_ms"] / out["write_device"]["median_ms"], 2)
    # ... the device writer's stages, each closed by a synchronisation: which one bounds it
    pinned = kmer_fasta._pinned_pair(kmer_fasta._window_bytes())
    win = min(kmer_fasta._window_bytes(), total)
    dbuf = torch.empty(win, dtype=torch.uint8, device="cuda")
    eng.format_kmers_dev(p(dlo), p(dhi), n, k, TEXT_FASTA, 0, 0, win, dbuf.data_ptr()); eng.synchronize()
    t_copy = wall(lambda: torch.from_numpy(pinned[0][:win]).copy_(dbuf, non_blocking=True), reps)
    with open(dev_fa, "wb") as fh:
        t0 = time.perf_counter()
        for _ in range((total + win - 1) // win):
            fh.write(memoryview(pinned[0][:win]))
        t_file = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    devkeys.to_host(dlo, dhi)
    t_keys = (time.perf_counter() - t0) * 1e3
    out["write_device_stages"] = {"window_bytes": win, "d2h_copy_GBps": gbps(win, spread(t_copy)), "file_write_ms": round(t_file, 1),
                                  "file_write_GBps": round(total / (t_file * 1e-3) / 1e9, 2), "keys_to_host_ms": round(t_keys, 1)}
    dev_write()

    for f in (host_fa, dev_fa):
        os.remove(f + ".kdfkeys.npz")

    def host_read():
        return kmer_fasta.read_kmer_fasta_keys(host_fa, k)

    def dev_read():
        return kmer_fasta.read_kmer_fasta_keys_device(dev_fa, k, engine=eng)
    want, got = host_read(), dev_read()
    got = devkeys.to_host(*got)
    assert all(np.array_equal(a, b) for a, b in zip(want, got)), f"k={k}: the device reader's keys differ from the host reader's"
    del want, got
    tr = {"host": [], "device": []}
    for _ in range(file_reps):
        tr["host"] += wall(host_read, 1)
        tr["device"] += wall(dev_read, 1)
    out["read_host"], out["read_device"] = spread(tr["host"]), spread(tr["device"])
    out["read_host_over_device"] = round(out["read_host"]["median_ms"] / out["read_device"]["median_ms"], 2)
    for f in (host_fa, dev_fa):
        os.remove(f)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000, help="keys per set (the host parser's index is n x k x 8 bytes)")
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 63, 101])
    ap.add_argument("--reps", type=int, default=7, help="repetitions of the kernel-only timings")
    ap.add_argument("--file-reps", type=int, default=5, help="repetitions of the file-to-file timings (host and device alternate)")
    ap.add_argument("--dir", default=None, help="where both writers write (default: a temporary directory)")
    ap.add_argument("--parent", default="", help="the parent commit, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmer_fasta_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/kmer_fasta.py measures on the GPU: no device visible")
    if args.reps < 5 or args.file_reps < 3:
        raise SystemExit("--reps >= 5 and --file-reps >= 3: a median wants repetitions")
    from kmer_denovo_filter_amd import kmer_fasta
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        out = {"bench": "kmer_fasta", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "parent": args.parent,
               "workload": "random canonical keys", "window_mb": kmer_fasta._window_bytes() >> 20, "dir": "tmp" if args.dir is None else args.dir,
               "cases": [case(k, args.n, args.reps, args.file_reps, d, 20261020 + k) for k in args.ks]}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
