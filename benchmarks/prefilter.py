#!/usr/bin/env python3
"""Two-pass counting (kdf_prefilter_*) against the plain count on the SAME workload in the SAME run, on ONE MI355X.

Workload: the bench batch (synth.py: 10 M x 150 bp reads of a 100 Mbp uniform genome, 0.5 % substitutions, 0.1 % N),
k = 31 and k = 63, L = 3.  Per k, HIP events around each phase, a warm-up and --reps repetitions, best and median:

  plain      clear + count + count_ge(3)                     (one pass, the table holds every distinct key)
  tally      begin-time sieve + prefilter_add_dev            (pass 1: no key is stored)
  gated      clear + count (armed) + count_ge(3)             (pass 2: only admitted keys are stored)

and the keys stored / table slots with and without the prefilter.  Then the strong-8 shape -- eight batches of the same
genome deferred into ONE table -- both ways: milliseconds, table slots and Gk-mer/s (the two-pass figure counts the
windows once although it reads them twice).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def batch(i, n_reads, read_len):
    import torch
    from kmer_denovo_filter_amd.synth import synth_stream
    ds = synth_stream(n_reads, read_len, seed=20260417 + 1000 * i, device=DEV, genome_seed=20260417)
    torch.cuda.synchronize()
    return ds


def timed(fn, stream, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        s.record(stream)
        fn()
        e.record(stream)
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return round(min(ts), 3), round(statistics.median(ts), 3)


def engine(k, hint, stream):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    torch.cuda.empty_cache()
    e = KmerEngine(k, capacity_hint=hint)
    e.set_stream(stream.cuda_stream)
    return e


def count(e, ds):
    e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)


def tally(e, ds):
    e.prefilter_add_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)


def one_batch(k, L, n_reads, read_len, reps, stream):
    ds = batch(0, n_reads, read_len)
    hint = 1 << 28 if n_reads >= 5_000_000 else max(1 << 16, n_reads * 40)
    res = {"k": k, "L": L, "reads": n_reads, "read_len": read_len}
    # plain
    e = engine(k, hint, stream)

    def plain():
        e.clear(); count(e, ds); return e.count_ge(L)
    res["plain_count_ge_ms"], res["plain_count_ge_median_ms"] = timed(plain, stream, reps)
    cap, distinct, windows = e.stats()
    ge = e.count_ge(L)
    res.update(windows=int(windows), plain_distinct=int(distinct), plain_slots=int(cap), count_ge_L=int(ge))
    e.close()
    # two passes: the table is sized for what the sieve admits
    e = engine(k, 1 << 16, stream)

    def tally_pass():
        e.prefilter_begin(L, s); tally(e, ds); e.synchronize()
    s = min(38, max(16, (8 * hint - 1).bit_length()))
    e.prefilter_begin(L, s); tally(e, ds); e.synchronize(); e.prefilter_drop()          # warm-up
    ts = []
    for _ in range(reps):
        ts.append(timed(tally_pass, stream, 1, warmup=0)[0])
        if _ < reps - 1:
            e.prefilter_drop()
    res["tally_ms"], res["tally_median_ms"] = round(min(ts), 3), round(statistics.median(ts), 3)
    e.profile(True)
    e.prefilter_drop(); e.prefilter_begin(L, s); tally(e, ds)
    res["tally_kernel_ms"] = round(e.get_stat("prefilter_us") / 1000.0, 3)
    e.profile(False)
    fill = e.prefilter_fill()
    e.prefilter_arm()
    e.reserve(fill[3] + (fill[2] if L == 2 else 0) + 1)

    def gated():
        e.clear(); count(e, ds); return e.count_ge(L)
    res["gated_count_ge_ms"], res["gated_count_ge_median_ms"] = timed(gated, stream, reps)
    cap2, distinct2, windows2 = e.stats()
    assert e.count_ge(L) == ge, "the gated count lost or gained keys with count >= L"
    res.update(log2_cells=s, sieve_bytes=e.get_stat("prefilter_bytes"), cells_by_value=fill, gated_windows=int(windows2),
               gated_distinct=int(distinct2), gated_slots=int(cap2),
               two_pass_ms=round(res["tally_ms"] + res["gated_count_ge_ms"], 3))
    e.close()
    return res


def strong8(k, L, n_reads, read_len, n_batches, reps, stream):
    import torch
    bs = [batch(i, n_reads, read_len) for i in range(n_batches)]
    hint = n_batches * (1 << 27) if n_reads >= 5_000_000 else max(1 << 16, n_batches * n_reads * 20)
    res = {"k": k, "L": L, "batches": n_batches}
    e = engine(k, hint, stream)

    def plain():
        e.clear()
        for b in bs:
            count(e, b)
        return e.count_ge(L)
    res["plain_ms"], res["plain_median_ms"] = timed(plain, stream, reps)
    cap, distinct, windows = e.stats()
    ge = e.count_ge(L)
    res.update(windows=int(windows), plain_distinct=int(distinct), plain_slots=int(cap), count_ge_L=int(ge),
               plain_gkmer_s=round(windows / res["plain_ms"] / 1e6, 1))
    e.close()
    e = engine(k, 1 << 16, stream)
    s = min(38, max(16, (8 * hint - 1).bit_length()))
    ts = []
    for r in range(reps + 1):

        def tally_all():
            e.prefilter_begin(L, s)
            for b in bs:
                tally(e, b)
            e.synchronize()
        t = timed(tally_all, stream, 1, warmup=0)[0]
        if r:
            ts.append(t)
        if r < reps:
            e.prefilter_drop()
    res["tally_ms"], res["tally_median_ms"] = round(min(ts), 3), round(statistics.median(ts), 3)
    fill = e.prefilter_fill()
    e.prefilter_arm()
    e.reserve(fill[3] + (fill[2] if L == 2 else 0) + 1)

    def gated():
        e.clear()
        for b in bs:
            count(e, b)
        return e.count_ge(L)
    res["gated_ms"], res["gated_median_ms"] = timed(gated, stream, reps)
    cap2, distinct2, windows2 = e.stats()
    assert e.count_ge(L) == ge, "the gated count lost or gained keys with count >= L"
    two = res["tally_ms"] + res["gated_ms"]
    res.update(log2_cells=s, sieve_bytes=e.get_stat("prefilter_bytes"), cells_by_value=fill, gated_distinct=int(distinct2),
               gated_slots=int(cap2), two_pass_ms=round(two, 3), two_pass_gkmer_s=round(windows / two / 1e6, 1),
               gated_pass_gkmer_s=round(windows / res["gated_ms"] / 1e6, 1))
    e.close()
    del bs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-count", type=int, default=3)
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 63])
    ap.add_argument("--strong", type=int, default=8, help="batches of the strong shape (0: skip it)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/prefilter.py measures on the GPU: no device visible")
    stream = torch.cuda.Stream()
    out = {"bench": "prefilter", "device": torch.cuda.get_device_name(0), "workload": "synth",
           "one_batch": [one_batch(k, args.min_count, args.reads, args.read_len, args.reps, stream) for k in args.ks]}
    if args.strong:
        out["strong"] = [strong8(k, args.min_count, args.reads, args.read_len, args.strong, max(2, args.reps // 2), stream)
                         for k in args.ks[:1]]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
