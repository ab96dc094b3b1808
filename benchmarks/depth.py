#!/usr/bin/env python3
"""Per-window counts (kdf_window_counts_dev) and per-read depth rows (kdf_read_depth_dev) against the Module-3 scan
(kdf_scan_reads_dev, force_path 1: the direct kernel) on the SAME table and the SAME stream in the SAME run, on ONE
MI355X.

The three calls make the same lookups -- every valid window's canonical k-mer probed in the table.  The scan writes one
bit per window; window_counts writes 4 bytes per stream position; read_depth writes 48 bytes per read.  So the scan is
the yardstick: window_counts should cost it plus the time of its store, read_depth no more than it plus the atomics.

Workload: the bench workload (synth.py: 10 M x 150 bp reads of a 100 Mbp uniform genome, 0.5 % substitutions, 0.1 % N;
capacity hint 2^28 like bench.py), the table counted from it once, stream and table resident in HBM, at k = 31, 63 and
101.  Plus the long-sequence case: a --contig Mbp sequence as ONE read (where per-read atomics would pile onto one row)
against the same table.  Warm; best and median of --reps calls, HIP events on the engine's stream.  One JSON line.
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
    fn(); fn()                                   # warm-up: code objects
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


def measure(eng, stream, reps, packed, invalid, n_bases, offsets, n_reads, low_max):
    import torch
    T = (n_bases + 63) // 64
    hits = torch.zeros(T + 2, dtype=torch.int64, device="cuda:0")
    counts = torch.zeros(n_bases, dtype=torch.int32, device="cuda:0")
    rows = torch.zeros(n_reads * 6, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    calls = {
        "scan": lambda: eng.scan_dev(packed.data_ptr(), invalid.data_ptr(), n_bases, hits.data_ptr()),
        "window_counts": lambda: eng.window_counts_dev(packed.data_ptr(), invalid.data_ptr(), n_bases, counts.data_ptr()),
        "read_depth": lambda: eng.read_depth_dev(packed.data_ptr(), invalid.data_ptr(), n_bases, offsets.data_ptr(), n_reads,
                                                 low_max, rows.data_ptr()),
    }
    runs = {name: [] for name in calls}
    for _ in range(2):                           # alternate, so that drift of the box hits all three alike
        for name, fn in calls.items():
            runs[name].append(timed(fn, stream, reps))
    assert eng.get_stat("last_scan_path") == 0, "the yardstick must be the direct scan kernel"
    out = {}
    for name, ts in runs.items():
        out[name + "_ms"] = round(min(t[0] for t in ts), 4)
        out[name + "_median_ms"] = round(statistics.median(t[1] for t in ts), 4)
    # the three agree: hit bit == (count != 0), and the rows' `present` sums to the hits
    pos = torch.arange(n_bases, dtype=torch.int64, device="cuda:0")
    bit = ((hits[pos >> 6] >> (pos & 63)) & 1) != 0
    assert torch.equal(bit, counts != 0), "window counts disagree with the scan"
    r = rows.view(n_reads, 6)
    assert int(r[:, 1].sum().item()) == int(bit.sum().item()), "read depth rows disagree with the scan"
    assert int(r[:, 5].sum().item()) == int((counts.to(torch.int64) & 0xFFFFFFFF).sum().item())
    out["hits"] = int(bit.sum().item())
    out["valid_windows"] = int(r[:, 0].sum().item())
    out["window_counts_over_scan"] = round(out["window_counts_ms"] / out["scan_ms"], 3)
    out["read_depth_over_scan"] = round(out["read_depth_ms"] / out["scan_ms"], 3)
    out["count_bytes_stored"] = 4 * n_bases
    out["window_counts_store_GBps"] = round(4 * n_bases / (out["window_counts_ms"] * 1e-3) / 1e9, 1)
    extra = out["window_counts_ms"] - out["scan_ms"]
    out["store_GBps_over_the_yardstick"] = round(4 * n_bases / (extra * 1e-3) / 1e9, 1) if extra > 0 else None
    out["positions_per_s_read_depth"] = round(n_bases / (out["read_depth_ms"] * 1e-3) / 1e9, 2)
    return out


def table_case(k, n_reads, read_len, contig_mbp, reps, low_max):
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
    eng.set_option("force_path", 1)
    offsets = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda:0") * (read_len + 1)
    res = {"k": k, "key_words": eng.key_words, "reads": n_reads, "read_len": read_len, "positions": ds.n_bases,
           "log2cap": cap.bit_length() - 1, "distinct": int(distinct)}
    res.update(measure(eng, stream, reps, ds.packed, ds.invalid, ds.n_bases, offsets, n_reads, low_max))
    assert res["valid_windows"] == windows
    eng.profile(True)
    eng.read_depth_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases, offsets.data_ptr(), n_reads, low_max,
                       torch.zeros(n_reads * 6, dtype=torch.int64, device="cuda:0").data_ptr())
    res["read_depth_kernels_ms"] = round(eng.get_stat("depth_us") / 1000.0 / max(1, eng.get_stat("depth_passes")), 4)
    eng.profile(False)
    if contig_mbp:
        # one read of contig_mbp Mbp: the first positions of the same stream with its separators and N made valid bases
        n = min(contig_mbp * 1_000_000, ds.n_bases - 64) // 64 * 64
        mask = ds.invalid.clone()
        mask[:n // 64] = 0
        one = torch.tensor([0, n], dtype=torch.int64, device="cuda:0")
        c = measure(eng, stream, reps, ds.packed, mask, n, one, 1, low_max)
        assert c["valid_windows"] == n - k + 1
        res["contig"] = {"positions": n, **c}
    eng.close()
    del ds
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--contig", type=int, default=100, help="Mbp of the single-read case (0: skip)")
    ap.add_argument("--low-max", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 63, 101])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/depth.py measures on the GPU: no device visible")
    out = {"bench": "depth", "device": torch.cuda.get_device_name(0), "workload": "synth",
           "tables": [table_case(k, args.reads, args.read_len, args.contig, args.reps, args.low_max) for k in args.ks]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
