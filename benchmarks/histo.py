#!/usr/bin/env python3
"""The count histogram (kdf_histogram_dev, high = 10000) against `dump -L 1`'s counting pass (kdf_count_ge(h, 1)) on the
SAME table in the SAME run, on ONE MI355X.

Both read the table's 4-byte count array once (4 x capacity bytes) and nothing else in an insert-mode table;
count_ge does strictly less arithmetic, so it is the yardstick for the histogram kernel.

Tables: the bench workload (synth.py: 10 M x 150 bp reads of a 100 Mbp uniform genome, 0.5 % substitutions, 0.1 % N;
capacity hint 2^28 like bench.py) counted once at k = 31, k = 63 and k = 101.
Per table, warm: best and median of --reps calls, HIP events on the engine's stream around the whole call (both calls
end in a stream synchronisation and a small device-to-host copy), plus the histogram KERNEL's own event time (engine
stats "histo_us" under profile) -- and the bytes read and the implied GB/s.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, stream, reps):
    import torch
    fn(); fn()                                   # warm-up: code objects, scratch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        s.record(stream)
        fn()
        e.record(stream)
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return min(ts), statistics.median(ts)


def table_case(k, n_reads, read_len, high, reps):
    import numpy as np
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.synth import synth_stream

    ds = synth_stream(n_reads, read_len, seed=20260417, device="cuda:0", genome_seed=20260417)
    torch.cuda.synchronize()
    per_batch = 1 << 28 if n_reads >= 5_000_000 else max(1 << 16, n_reads * 40)
    eng = KmerEngine(k, capacity_hint=per_batch)
    stream = torch.cuda.Stream()                 # (the default stream's handle is 0, which set_stream reads as "own stream")
    eng.set_stream(stream.cuda_stream)
    eng.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
    cap, distinct, windows = eng.stats()
    del ds
    torch.cuda.empty_cache()
    bins = torch.zeros(high + 2, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()

    # alternate the two calls, so that drift of the box hits both alike
    ge, hi = [], []
    for _ in range(3):
        ge.append(timed(lambda: eng.count_ge(1), stream, reps))
        hi.append(timed(lambda: eng.histogram_dev(high, bins.data_ptr()), stream, reps))
    ge_best, ge_med = min(t[0] for t in ge), statistics.median(t[1] for t in ge)
    hi_best, hi_med = min(t[0] for t in hi), statistics.median(t[1] for t in hi)
    eng.profile(True)
    for _ in range(reps):
        eng.histogram_dev(high, bins.data_ptr())
    kern_ms = eng.get_stat("histo_us") / 1000.0 / max(1, eng.get_stat("histo_passes"))
    eng.profile(False)

    b = bins.cpu().numpy().view(np.uint64)
    n_ge1 = eng.count_ge(1)
    assert int(b.sum()) == eng.count_ge(0) == distinct and int(b[1:].sum()) == n_ge1, "histogram disagrees with count_ge"
    st = eng.count_stats()
    assert st["total"] == windows and st["distinct"] == n_ge1, "count_stats disagrees with the table"
    nbytes = 4 * cap

    def gbs(ms):
        return round(nbytes / (ms * 1e-3) / 1e9, 1)
    res = {"k": k, "key_words": eng.key_words, "reads": n_reads, "read_len": read_len, "log2cap": cap.bit_length() - 1,
           "distinct": int(distinct), "table_bytes_read": int(nbytes), "high": high,
           "count_ge1_ms": round(ge_best, 4), "count_ge1_median_ms": round(ge_med, 4), "count_ge1_GBps": gbs(ge_best),
           "histogram_ms": round(hi_best, 4), "histogram_median_ms": round(hi_med, 4), "histogram_GBps": gbs(hi_best),
           "histogram_kernel_ms": round(kern_ms, 4), "histogram_kernel_GBps": gbs(kern_ms) if kern_ms > 0 else None,
           "histogram_over_count_ge": round(hi_best / ge_best, 3),
           "bins_1_to_5": [int(x) for x in b[1:6]], "max_count": st["max_count"]}
    eng.close()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--high", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 63, 101])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/histo.py measures on the GPU: no device visible")
    out = {"bench": "histo", "device": torch.cuda.get_device_name(0), "workload": "synth",
           "tables": [table_case(k, args.reads, args.read_len, args.high, args.reps) for k in args.ks]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
