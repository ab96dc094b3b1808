#!/usr/bin/env python3
"""The table join (kdf_count_join + kdf_export_join*_dev) against the chain of existing calls it replaces, on the SAME two
tables in the SAME run, on ONE MI355X.

Tables: A is the bench workload counted (synth.py: 10 M x 150 bp reads of a 100 Mbp uniform genome, 0.5 % substitutions,
0.1 % N; capacity hint 2^28 like bench.py); B is that genome's own k-mers (the genome as one record: the reference
index of the workload).  Widths: k = 31, 63 and 101.

What is timed, per width, as the discovery mirrors call it (devkeys.py):
  join   devkeys.dump_join(A, B, 3, other_max=0): count_join sizes the buffers, export_join_dev writes the survivors,
         sorted.  Also timed unsorted, and the kernel alone (stats "join_us" under profile).
  chain  devkeys.dump_ge(A, 3) sorted, devkeys.query(B, keys), devkeys.select(keys, counts == 0): reference subtraction
         as _extract_child_kmers_discovery + _subtract_reference_kmers do it, without the FASTA file and the host copy
         between them (those only add to the chain).
HIP events on the stream both engines and torch use, around the whole call sequence; fastest and median of --reps warm
passes, the two paths alternating.  The key sets are asserted equal, in order.  Bytes, two figures per path:
"*_buffer_bytes", the caller-owned device buffers the path needs at once, from the sizes; "*_torch_peak_bytes", the
peak the caller's allocator saw over one call of the path (torch.cuda.max_memory_allocated: the tensors above and the
temporaries of the query's widening and the select).  Neither holds the radix sort's own scratch, which the library
allocates and frees inside the call (index and key copies, proportional to what is sorted: every candidate for the
chain, the survivors for the join).  Prints one JSON line; there is no threshold -- the yardstick is the chain.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIN_CHILD = 3


def timed(fn, stream, reps):
    import torch
    fn(); fn()                                   # warm-up: code objects, scratch, the allocator's blocks
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        s.record(stream)
        fn()
        e.record(stream)
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return ts


def table_case(k, n_reads, read_len, genome_len, reps):
    import torch
    from kmer_denovo_filter_amd import KmerEngine, devkeys
    from kmer_denovo_filter_amd.synth import genome_stream, synth_genome, synth_stream

    dev = torch.device("cuda", 0)
    genome = synth_genome(genome_len, 20260417, dev)
    stream = torch.cuda.Stream()                 # (the default stream's handle is 0, which set_stream reads as "own stream")
    a = KmerEngine(k, capacity_hint=1 << 28 if n_reads >= 5_000_000 else max(1 << 16, n_reads * 40))
    b = KmerEngine(k, capacity_hint=max(1 << 16, genome_len))
    for e in (a, b):
        e.set_stream(stream.cuda_stream)
    ds = synth_stream(n_reads, read_len, seed=20260417, device=dev, genome=genome)
    torch.cuda.synchronize()
    a.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
    a.flush(); a.synchronize()
    del ds
    gs = genome_stream(genome)
    torch.cuda.synchronize()
    b.count_dev(gs.packed.data_ptr(), gs.invalid.data_ptr(), gs.n_bases)
    b.flush(); b.synchronize()
    del gs, genome
    torch.cuda.empty_cache()
    cap_a, distinct_a, _ = a.stats()
    cap_b, distinct_b, _ = b.stats()

    out = {}

    def join_sorted():
        out["join"] = devkeys.dump_join(a, b, MIN_CHILD, None, 0, 0, 0)

    def chain():
        lo, hi = devkeys.dump_ge(a, MIN_CHILD, 0)
        keep = devkeys.query(b, lo, hi, 0) == 0
        out["chain"] = devkeys.select([(lo, hi)], keep)

    n_cand = a.count_ge(MIN_CHILD)
    n_join = a.count_join(b, MIN_CHILD, None, 0, 0)
    W = a.key_words
    rows = (max(n_join, 1), W) if a.long else (max(n_join, 1),)
    u_lo = torch.empty(rows, dtype=torch.int64, device=dev)
    u_hi = torch.empty(max(n_join, 1), dtype=torch.int64, device=dev) if (a.wide and not a.long) else None

    def join_unsorted():
        a.count_join(b, MIN_CHILD, None, 0, 0)
        a.export_join_dev(b, MIN_CHILD, None, 0, 0, u_lo.data_ptr(), u_hi.data_ptr() if u_hi is not None else None, None, None, n_join)

    def torch_peak(fn):
        out.clear()
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    tj, tc, tu = [], [], []
    with torch.cuda.stream(stream):
        peak_join, peak_chain = torch_peak(join_sorted), torch_peak(chain)
        for _ in range(3):                       # alternate, so that drift of the box hits both alike
            tj += timed(join_sorted, stream, reps)
            tc += timed(chain, stream, reps)
            tu += timed(join_unsorted, stream, reps)
        torch.cuda.synchronize()
        for x, y in zip(out["join"], out["chain"]):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), "the join and the chain disagree"
        assert out["join"][0].shape[0] == n_join
        a.profile(True)
        for _ in range(reps):
            a.export_join_dev(b, MIN_CHILD, None, 0, 0, u_lo.data_ptr(), u_hi.data_ptr() if u_hi is not None else None, None, None, n_join)
        kern_ms = a.get_stat("join_us") / 1000.0 / max(1, a.get_stat("join_passes"))
        a.profile(False)

    kb = 8 * W
    # chain: the sorted dump (keys + counts), the query's counts (int32, then the int64 view devkeys.query returns), the mask,
    # the selected keys;  join: the survivors' keys and the counts the sort carries
    chain_bytes = n_cand * (kb + 4) + n_cand * (4 + 8) + n_cand + n_join * kb
    join_bytes = n_join * (kb + 4)
    res = {"k": k, "key_words": W, "reads": n_reads, "read_len": read_len, "genome_len": genome_len,
           "a_log2cap": cap_a.bit_length() - 1, "a_distinct": int(distinct_a), "b_log2cap": cap_b.bit_length() - 1, "b_distinct": int(distinct_b),
           "candidates": int(n_cand), "survivors": int(n_join),
           "join_sorted_ms": round(min(tj), 3), "join_sorted_median_ms": round(statistics.median(tj), 3),
           "join_unsorted_ms": round(min(tu), 3), "join_unsorted_median_ms": round(statistics.median(tu), 3),
           "chain_ms": round(min(tc), 3), "chain_median_ms": round(statistics.median(tc), 3),
           "chain_over_join_sorted": round(min(tc) / min(tj), 3),
           "join_kernel_ms": round(kern_ms, 4),
           "join_probes_per_s": round(n_cand / (kern_ms * 1e-3)) if kern_ms > 0 else None,
           "join_slots_per_s": round(cap_a / (kern_ms * 1e-3)) if kern_ms > 0 else None,
           "chain_buffer_bytes": int(chain_bytes), "join_buffer_bytes": int(join_bytes),
           "chain_torch_peak_bytes": peak_chain, "join_torch_peak_bytes": peak_join}
    a.close(); b.close()
    del out, u_lo, u_hi
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome-len", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 63, 101])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/table_join.py measures on the GPU: no device visible")
    out = {"bench": "table_join", "device": torch.cuda.get_device_name(0), "workload": "synth", "min_count": MIN_CHILD,
           "tables": [table_case(k, args.reads, args.read_len, args.genome_len, args.reps) for k in args.ks]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
