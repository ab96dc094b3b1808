#!/usr/bin/env python3
"""The merge of counting sieves (kdf_prefilter_merge_dev, csrc/kdf_prefilter.h kdf_pf_merge_kernel) on ONE MI355X.

A sieve of 2^32 cells (2 GB) and nseg = 1, 3, 7 device segments of the same size (what a rank of 2, 4, 8 receives for
its slice -- here over the WHOLE sieve, so the figure is a rate, not a merge time of a real exchange).  The kernel is a
stream of (nseg + 1) reads and 1 write per word; GB/s counts those bytes.  In the same run, alternating with it, a
torch elementwise ``a | b`` into a preallocated output over the same bytes: 2 reads and 1 write per word, the traffic
of nseg = 1.  HIP events on one stream, a warm-up and --reps repetitions, best and median.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-cells", type=int, default=32)
    ap.add_argument("--nseg", type=int, nargs="+", default=[1, 3, 7])
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    if not torch.cuda.is_available():
        raise SystemExit("prefilter_merge.py needs the GPU: nothing here can be measured without it")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n_words = 1 << (args.log2_cells - 4)
    nbytes = n_words * 8
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    segs = [torch.randint(-2 ** 62, 2 ** 62, (n_words,), dtype=torch.int64, device=dev, generator=g) for _ in range(max(args.nseg))]
    a, b = segs[0], torch.randint(-2 ** 62, 2 ** 62, (n_words,), dtype=torch.int64, device=dev, generator=g)
    out = torch.empty_like(a)
    torch.cuda.synchronize()
    e = KmerEngine(31, capacity_hint=1 << 16)
    e.set_stream(stream.cuda_stream)
    e.prefilter_begin(3, args.log2_cells)

    def timed(fn):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record(stream)
        fn()
        t.record(stream)
        torch.cuda.synchronize()
        return s.elapsed_time(t)

    def torch_or():
        with torch.cuda.stream(stream):
            torch.bitwise_or(a, b, out=out)

    res = {"bench": "prefilter_merge", "log2_cells": args.log2_cells, "sieve_bytes": nbytes, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "merge": {}}
    t_or = []
    for nseg in args.nseg:
        ptrs = [s.data_ptr() for s in segs[:nseg]]
        merge = lambda: e.prefilter_merge_dev(ptrs, 0, n_words)     # noqa: E731
        merge(); torch_or()                                         # warm-up of both
        tm, to = [], []
        for _ in range(args.reps):                                  # alternating: both see the same machine
            tm.append(timed(merge))
            to.append(timed(torch_or))
        t_or += to
        gb = (nseg + 2) * nbytes / 1e9
        res["merge"][str(nseg)] = {"ms_best": round(min(tm), 3), "ms_median": round(statistics.median(tm), 3),
                                   "bytes": (nseg + 2) * nbytes, "gbps_best": round(gb / min(tm) * 1e3, 1),
                                   "gbps_median": round(gb / statistics.median(tm) * 1e3, 1)}
    gb_or = 3 * nbytes / 1e9
    res["torch_or"] = {"ms_best": round(min(t_or), 3), "ms_median": round(statistics.median(t_or), 3), "bytes": 3 * nbytes,
                       "gbps_best": round(gb_or / min(t_or) * 1e3, 1), "gbps_median": round(gb_or / statistics.median(t_or) * 1e3, 1)}
    if "1" in res["merge"]:
        res["ratio_nseg1_vs_torch_or"] = round(res["merge"]["1"]["gbps_median"] / res["torch_or"]["gbps_median"], 3)
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
