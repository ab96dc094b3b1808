#!/usr/bin/env python3
"""count --if through the bin-major sieve (option sieve_bins = 1) against the engine's automatic choice, in the same run.

Input: the bench reads (10 M x 150 bp over the 100 Mbp synthetic genome of synth.py), resident in HBM, at k = 31 and
k = 63.  Filters of 2 M, 20 M, 100 M and 250 M keys: the k-mers of the stream's first reads (at most half of the filter
and at most ~1 M) padded with random keys.  Per filter ONE engine runs count_filtered_dev + flush with sieve_bins 0 (the
existing selection: the L2 sieve for 2 M keys, the binned count --if beyond) and with sieve_bins 1: a warm-up pass, then
`--reps` timed passes (HIP events on the engine's stream around the call and its flush; the fastest is reported).  The
counts of every filter key and the windows must be equal, or the run stops.  One more profiled pass of the new path gives
its stage split (kernel A / transposer / bin kernel).  Writes one JSON to profiles/bin_sieve_bench.json and prints it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILTERS = (2_000_000, 20_000_000, 100_000_000, 250_000_000)
PATHS = {0: "direct", 1: "binned", 3: "sieve", 5: "bin_sieve"}


def own_keys(k, ds, n_keys, read_len):
    """about n_keys distinct canonical k-mers of the stream's first reads, as device tensors (ascending)"""
    import torch
    from kmer_denovo_filter_amd import KmerEngine, devkeys
    n_reads = min(ds.n_reads, (n_keys * 5 // 4) // (read_len - k + 1) + 64)
    with KmerEngine(k, capacity_hint=max(n_keys * 2, 1 << 12)) as e:
        e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), n_reads * (read_len + 1))
        lo, hi = devkeys.dump_ge(e, 0)
    torch.cuda.synchronize()
    return lo, hi


def make_filter(k, own, n_keys, gen):
    """(lo, hi or None): own keys first, random keys behind them (random words below 4^k: hardly any is a k-mer of the reads)"""
    import torch
    n_own = min(own[0].shape[0], n_keys // 2)
    n_rnd = n_keys - n_own
    if k <= 31:
        rlo = torch.randint(0, 1 << (2 * k), (n_rnd,), dtype=torch.int64, device="cuda", generator=gen)
        return torch.cat([own[0][:n_own], rlo]).contiguous(), None
    rlo = torch.randint(-(1 << 63), (1 << 63) - 1, (n_rnd,), dtype=torch.int64, device="cuda", generator=gen)
    rhi = torch.randint(0, 1 << (2 * k - 64), (n_rnd,), dtype=torch.int64, device="cuda", generator=gen)
    return torch.cat([own[0][:n_own], rlo]).contiguous(), torch.cat([own[1][:n_own], rhi]).contiguous()


def timed(e, stream, fn, reps):
    import torch
    best = None
    for i in range(reps + 1):                        # the first pass warms up (and builds the sieve after the option changed)
        e.reset_counts()
        e.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(stream)
        fn()
        ev1.record(stream)
        ev1.synchronize()
        ms = ev0.elapsed_time(ev1)
        if i:
            best = ms if best is None else min(best, ms)
    return best


def run_k(k, n_reads, read_len, seed, reps, filters):
    import torch
    from kmer_denovo_filter_amd import KmerEngine, devkeys
    from kmer_denovo_filter_amd.engine import bin_sieve_geometry
    from kmer_denovo_filter_amd.synth import synth_stream

    ds = synth_stream(n_reads, read_len, seed=seed, device="cuda:0", genome_seed=20260417)
    torch.cuda.synchronize()
    P, M, N = ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases
    own = own_keys(k, ds, 1_000_000, read_len)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    res = {"k": k, "reads": n_reads, "read_len": read_len, "filters": {}}
    stream = torch.cuda.Stream()
    for n_keys in filters:
        lo, hi = make_filter(k, own, n_keys, gen)
        torch.cuda.synchronize()
        row = {"keys": n_keys}
        counts, windows = {}, {}
        with KmerEngine(k, capacity_hint=n_keys) as e:
            e.set_stream(stream.cuda_stream)
            e.load_filter_dev(lo.data_ptr(), hi.data_ptr() if hi is not None else None, n_keys)
            row["distinct"] = e.stats()[1]

            def call():
                e.count_filtered_dev(P, M, N)
                e.flush()

            for sb in (0, 1):
                e.set_option("sieve_bins", sb)
                tag = "bin_sieve" if sb else "auto"
                ms = timed(e, stream, call, reps)
                path = e.get_stat("last_count_path")
                if sb:
                    assert path == 5, f"k={k}, {n_keys} keys: sieve_bins 1 took path {path}"
                    row["c1"], row["slice_words"] = e.get_stat("last_sieve_bins"), e.get_stat("last_sieve_slice_words")
                    row["bits_per_key"] = bin_sieve_geometry(row["distinct"], e.key_words)[2]
                else:
                    row["auto_path"] = PATHS.get(path, str(path))
                e.reset_counts()
                w0 = e.stats()[2]
                call()
                windows[sb] = e.stats()[2] - w0
                counts[sb] = devkeys.query(e, lo, hi).clone()
                row[f"{tag}_ms"] = round(ms, 3)
                row[f"{tag}_Gkmer_per_s"] = round(windows[sb] / (ms * 1e-3) / 1e9, 2)
            e.reset_counts()                                     # the new path's stages, in a pass of their own
            e.profile(True)
            call()
            e.synchronize()
            st, passes = e.profile_stages()
            e.profile(False)
            row["stage_ms"] = {"slabsort": round(st[0], 3), "transpose": round(st[1], 3), "bin_kernel": round(st[2], 3), "passes": passes}
        assert windows[0] == windows[1], f"k={k}, {n_keys} keys: windows differ ({windows[0]} / {windows[1]})"
        assert torch.equal(counts[0], counts[1]), f"k={k}, {n_keys} keys: count --if differs between the paths"
        row["windows"] = int(windows[1])
        row["hit_windows"] = int(counts[1].sum().item())
        row["speedup"] = round(row["auto_ms"] / row["bin_sieve_ms"], 2)
        res["filters"][str(n_keys)] = row
        print(json.dumps({"k": k, **row}), file=sys.stderr, flush=True)
        del lo, hi, counts
        torch.cuda.empty_cache()
    del own, ds
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--filters", type=int, nargs="*", default=list(FILTERS))
    ap.add_argument("--ks", type=int, nargs="*", default=[31, 63])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bin_sieve_bench.json"))
    args = ap.parse_args()
    out = {"genome": 100_000_000, "reps": args.reps, "timing": "HIP events around count_filtered_dev + flush, fastest pass",
           "cases": {f"k{k}": run_k(k, args.reads, 150, 11 + k, args.reps, args.filters) for k in args.ks}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
