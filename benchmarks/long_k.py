#!/usr/bin/env python3
"""Long k-mers (odd k from 65 to 201) on ONE MI355X against the k = 63 direct path in the same run.

Input: synthetic reads of a 100 Mbp uniform genome (synth.py: 0.5 % substitutions, 0.1 % N), resident in HBM.
Cases (each: a warm-up pass, clear, then the timed pass; ms = the stream kernels' HIP-event time of the pass):
  k63_direct   k = 63, force_path 1 (the direct global-table kernels), 10 M x 150 bp -- the same-run baseline
  k101         k = 101 (W = 4 key words), 10 M x 150 bp
  k201         k = 201 (W = 7), 4 M x 250 bp
  k101_query   query_dev of the k = 101 table's dump -L 2 (input order), keys/s
  k101_scan    scan_dev (Module 3 probe) of the k = 101 reads against the k = 101 table, windows/s
Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def count_case(k, n_reads, read_len, seed, force_path=0, capacity_hint=1 << 29, keep=False):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.synth import synth_stream

    ds = synth_stream(n_reads, read_len, seed=seed, device="cuda:0", genome_seed=20260417)
    torch.cuda.synchronize()
    eng = KmerEngine(k, capacity_hint=capacity_hint)
    stream = torch.cuda.Stream()                 # (the default stream's handle is 0, which set_stream reads as "own stream")
    eng.set_stream(stream.cuda_stream)
    if force_path:
        eng.set_option("force_path", force_path)

    def one_pass():
        eng.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
        eng.flush()
        return eng.stats()

    one_pass()                                   # warm-up: code objects, table growth to its final size
    eng.clear()
    eng.profile(True)
    cap, distinct, windows = one_pass()
    ms, launches, _ = eng.profile_read()
    eng.profile(False)
    res = {"k": k, "key_words": getattr(eng, "key_words", 2), "reads": n_reads, "read_len": read_len,
           "ms": round(ms, 3), "windows": int(windows), "distinct": int(distinct), "log2cap": cap.bit_length() - 1,
           "launches": int(launches), "Gkmer_per_s": round(windows / (ms * 1e-3) / 1e9, 2),
           "path": eng.last_count_path()}
    if keep:
        return res, (eng, stream), ds
    eng.close()
    del ds
    torch.cuda.empty_cache()
    return res, None, None


def timed_events(fn, stream, reps=3):
    """Fastest of `reps` runs, HIP events on the engine's stream."""
    import torch
    fn()                                         # warm-up
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        s.record(stream)
        fn()
        e.record(stream)
        torch.cuda.synchronize()
        t = s.elapsed_time(e)
        best = t if best is None else min(best, t)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reads201", type=int, default=4_000_000)
    args = ap.parse_args()
    import torch
    from kmer_denovo_filter_amd import devkeys
    from kmer_denovo_filter_amd.reads import stream_words

    out = {"genome": 100_000_000, "cases": {}}
    out["cases"]["k63_direct"], _, _ = count_case(63, args.reads, 150, 11, force_path=1)
    res, (eng, stream), ds = count_case(101, args.reads, 150, 11, keep=True)
    out["cases"]["k101"] = res
    # query: the dump -L 2 of the table, input order
    keys, _ = devkeys.dump_ge(eng, 2)
    n = int(keys.shape[0])
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    ms = timed_events(lambda: eng.query_dev(keys.data_ptr(), None, n, cnt.data_ptr()), stream)
    out["cases"]["k101_query"] = {"keys": n, "ms": round(ms, 3), "Gkeys_per_s": round(n / (ms * 1e-3) / 1e9, 3),
                                  "all_found": bool((cnt >= 2).all().item())}
    # scan: Module 3's probe of the same reads
    _, mw = stream_words(ds.n_bases)
    hits = torch.zeros(mw, dtype=torch.int64, device="cuda")
    ms = timed_events(lambda: eng.scan_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases, hits.data_ptr()), stream)
    w = res["windows"]
    out["cases"]["k101_scan"] = {"windows": w, "ms": round(ms, 3), "Gkmer_per_s": round(w / (ms * 1e-3) / 1e9, 2)}
    eng.close()
    del keys, cnt, hits, ds
    torch.cuda.empty_cache()
    out["cases"]["k201"], _, _ = count_case(201, args.reads201, 250, 13)
    base = out["cases"]["k63_direct"]["Gkmer_per_s"]
    out["k101_vs_k63_direct"] = round(out["cases"]["k101"]["Gkmer_per_s"] / base, 3)
    out["k201_vs_k63_direct"] = round(out["cases"]["k201"]["Gkmer_per_s"] / base, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
