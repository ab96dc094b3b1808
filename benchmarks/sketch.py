#!/usr/bin/env python3
"""The distinct k-mer sketch (kdf_sketch_*) against the two passes it can replace or ride on, on the SAME stream in the
SAME run, on ONE MI355X.

Workload: the bench batch (synth.py: 10 M x 150 bp reads of a 100 Mbp uniform genome, 0.5 % substitutions, 0.1 % N, the
seed of bench.py), k = 31, 63 and 101, p = 16.  Per k, a warm-up and --reps repetitions, best and median:

  sketch     sketch_add_dev into a fresh sketch       (HIP events around the call, and the engine's own "sketch_us")
  count      clear + count_dev + flush                (the plain count pass: the yardstick)
  tally      prefilter_begin + prefilter_add_dev      (pass 1 of the two-pass count: the other yardstick)

and the sketch's estimate against the engine's exact ``stats()`` distinct of the same stream.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def timed(fn, stream, reps, warmup=1, before=None):
    import torch
    ts = []
    for r in range(warmup + reps):
        if before:
            before()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record(stream)
        fn()
        e.record(stream)
        torch.cuda.synchronize()
        if r >= warmup:
            ts.append(s.elapsed_time(e))
    return round(min(ts), 3), round(statistics.median(ts), 3)


def one_k(k, p, ds, hint, reps, stream):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    torch.cuda.empty_cache()
    args = (ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
    res = {"k": k, "log2_registers": p}
    with KmerEngine(k, capacity_hint=hint) as e:
        e.set_stream(stream.cuda_stream)
        state = {"on": False}

        def fresh():
            if state["on"]:
                e.sketch_drop()
            e.sketch_begin(p)
            e.synchronize()
            state["on"] = True
        res["sketch_ms"], res["sketch_median_ms"] = timed(lambda: e.sketch_add_dev(*args), stream, reps, before=fresh)
        e.profile(True)
        fresh()
        e.sketch_add_dev(*args)
        res["sketch_kernel_ms"] = round(e.get_stat("sketch_us") / 1000.0, 3)
        e.profile(False)
        estimate, windows = e.sketch_estimate(), e.get_stat("sketch_windows")
        # a second pass over a warm sketch: almost no window raises a register any more
        res["sketch_warm_ms"], res["sketch_warm_median_ms"] = timed(lambda: e.sketch_add_dev(*args), stream, reps)
        e.sketch_drop()

        def count():
            e.clear(); e.count_dev(*args); e.flush()
        res["count_flush_ms"], res["count_flush_median_ms"] = timed(count, stream, reps)
        cap, distinct, win = e.stats()
        assert win == windows, "the sketch and the count disagree on the stream's valid windows"
        e.clear()
        s = min(38, max(16, (8 * hint - 1).bit_length()))
        state["pf"] = False

        def pf_fresh():
            if state["pf"]:
                e.prefilter_drop()
            e.prefilter_begin(3, s)
            e.synchronize()
            state["pf"] = True
        res["tally_ms"], res["tally_median_ms"] = timed(lambda: e.prefilter_add_dev(*args), stream, reps, before=pf_fresh)
        e.prefilter_drop()
        res.update(windows=int(windows), distinct=int(distinct), table_slots=int(cap), estimate=round(estimate, 1),
                   rel_error=round(abs(estimate - distinct) / distinct, 5), std_error=round(1.04 / (1 << p) ** 0.5, 5),
                   sketch_gwindows_s=round(windows / res["sketch_ms"] / 1e6, 1), prefilter_log2_cells=s)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2m", type=int, default=16)
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 63, 101])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/sketch.py measures on the GPU: no device visible")
    from kmer_denovo_filter_amd.synth import synth_stream
    ds = synth_stream(a.reads, a.read_len, seed=20260417, device=DEV, genome_seed=20260417)
    torch.cuda.synchronize()
    hint = 1 << 28 if a.reads >= 5_000_000 else max(1 << 16, a.reads * 40)
    stream = torch.cuda.Stream()
    out = {"bench": "sketch", "device": torch.cuda.get_device_name(0), "workload": "synth", "reads": a.reads, "read_len": a.read_len,
           "n_bases": int(ds.n_bases), "per_k": [one_k(k, a.log2m, ds, hint, a.reps, stream) for k in a.ks]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
