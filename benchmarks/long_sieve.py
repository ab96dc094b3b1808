#!/usr/bin/env python3
"""Long k-mers through the membership sieve (option long_sieve) against the direct long kernels in the same run.

Input: the synthetic reads of benchmarks/long_k.py (100 Mbp uniform genome, synth.py), resident in HBM:
  k = 101 (W = 4 key words)  10 M x 150 bp
  k = 201 (W = 7)             4 M x 250 bp
For filters of 630, 60 000 and ~2 M keys drawn from the reads' own k-mers (the dump of a count of the first reads,
every `stride`-th key) one engine runs count_reads_filtered_dev and scan_reads_dev with long_sieve 0 and 1: a warm-up
pass, then `--reps` timed passes (the fastest is reported; HIP events of the stream kernel through kdf_profile).
Counts (query of the filter keys) and hit masks must be equal, or the run stops.  The floor is sketch_add_dev over the
same stream: the same walker and hash, no table.  Writes one JSON to profiles/long_sieve_bench.json and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILTERS = (630, 60_000, 2_000_000)


def timed(eng, fn, reps):
    fn()                                         # warm-up (and, after the option changed, the sieve's build)
    best = None
    for _ in range(reps):
        eng.profile(True)
        fn()
        ms, _, _ = eng.profile_read()
        eng.profile(False)
        best = ms if best is None else min(best, ms)
    return best


def own_keys(k, ds, n_keys, read_len):
    """at least n_keys distinct canonical k-mers of the stream's first reads, as device rows (ascending)"""
    import torch
    from kmer_denovo_filter_amd import KmerEngine, devkeys
    per_read = read_len - k + 1
    n_reads = min(ds.n_reads, (n_keys * 5 // 4) // per_read + 64)
    n_bases = n_reads * (read_len + 1)           # (synth_stream: fixed-length reads, one separator each)
    with KmerEngine(k, capacity_hint=max(n_keys * 2, 1 << 12)) as e:
        e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), n_bases)
        keys, _ = devkeys.dump_ge(e, 0)
    torch.cuda.synchronize()
    return keys


def run_k(k, n_reads, read_len, seed, reps):
    import torch
    from kmer_denovo_filter_amd import KmerEngine, devkeys
    from kmer_denovo_filter_amd.reads import stream_words
    from kmer_denovo_filter_amd.synth import synth_stream

    ds = synth_stream(n_reads, read_len, seed=seed, device="cuda:0", genome_seed=20260417)
    torch.cuda.synchronize()
    _, mw = stream_words(ds.n_bases)
    P, M, N = ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases
    pool = own_keys(k, ds, max(FILTERS), read_len)
    res = {"k": k, "reads": n_reads, "read_len": read_len, "filters": {}}
    stream = torch.cuda.Stream()
    with KmerEngine(k, capacity_hint=1 << 12) as e:          # the floor: the walker and the hash alone
        e.set_stream(stream.cuda_stream)
        e.sketch_begin()
        e.sketch_add_dev(P, M, N)                            # warm-up
        e.profile(True)
        best = None
        for _ in range(reps):
            us0 = e.get_stat("sketch_us")
            e.sketch_add_dev(P, M, N)
            ms = (e.get_stat("sketch_us") - us0) / 1000.0
            best = ms if best is None else min(best, ms)
        e.profile(False)
        res["sketch_ms"] = round(best, 3)
    for n_keys in FILTERS:
        stride = max(1, pool.shape[0] // n_keys)
        keys = pool[::stride][:n_keys].contiguous()
        n = int(keys.shape[0])
        torch.cuda.synchronize()
        row = {"keys": n}
        counts, masks = {}, {}
        with KmerEngine(k, capacity_hint=max(n, 1)) as e:
            e.set_stream(stream.cuda_stream)
            e.load_filter_dev(keys.data_ptr(), None, n)
            for ls in (0, 1):
                e.set_option("long_sieve", ls)
                tag = "sieve" if ls else "direct"
                ms = timed(e, lambda: e.count_filtered_dev(P, M, N), reps)
                assert e.get_stat("last_count_path") == (3 if ls else 0)
                e.reset_counts()
                e.count_filtered_dev(P, M, N)
                windows = e.stats()[2]
                counts[ls] = devkeys.query(e, keys, None).clone()
                row["windows"] = int(windows)
                row[f"count_{tag}_ms"] = round(ms, 3)
                row[f"count_{tag}_Gkmer_per_s"] = round(windows / (ms * 1e-3) / 1e9, 2)
                hits = torch.zeros(mw, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                ms = timed(e, lambda: e.scan_dev(P, M, N, hits.data_ptr()), reps)
                e.synchronize()
                assert e.get_stat("last_scan_path") == (3 if ls else 0)
                masks[ls] = hits
                row[f"scan_{tag}_ms"] = round(ms, 3)
                row[f"scan_{tag}_Gkmer_per_s"] = round(windows / (ms * 1e-3) / 1e9, 2)
                if ls:
                    row["sieve_in_lds"] = e.get_stat("last_sieve_in_lds")
        assert torch.equal(counts[0], counts[1]), f"k={k}, {n} keys: count --if differs between the sieve and the direct kernel"
        assert torch.equal(masks[0], masks[1]), f"k={k}, {n} keys: the scan's mask differs"
        row["hit_windows"] = int(counts[1].sum().item())
        row["count_speedup"] = round(row["count_direct_ms"] / row["count_sieve_ms"], 2)
        row["scan_speedup"] = round(row["scan_direct_ms"] / row["scan_sieve_ms"], 2)
        res["filters"][str(n_keys)] = row
        del keys, counts, masks, hits
    del pool, ds
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reads201", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_sieve_bench.json"))
    args = ap.parse_args()
    out = {"genome": 100_000_000, "reps": args.reps, "cases": {
        "k101": run_k(101, args.reads, 150, 11, args.reps),
        "k201": run_k(201, args.reads201, 250, 13, args.reps),
    }}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
