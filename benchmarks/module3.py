#!/usr/bin/env python3
"""The per-read reduction of the Module-3 scan: the host loop of ``KmerEngine.scan`` against the device path
(kdf_read_hits_dev + kdf_hit_list_dev) on the SAME table and the SAME stream in the SAME run, on ONE MI355X.

  (a) scan          ``KmerEngine.scan(stream)`` from host arrays: upload, scan kernel, the whole hit mask copied back,
                    then one CPU thread walks every read and rebuilds, sorts and uniques the keys of its hit windows.
                    Unchanged by the device path, so this is what the parent commit does.
  (b) device        ``read_hits_dev`` + ``hit_list_dev`` on the stream resident in HBM, plus the copy of the rows
                    (8 bytes per read) and of the compacted hit list (8 bytes per hit) to the host.
  (b') device_from_host   ``KmerEngine.scan_hits(stream)``: (b) with the upload of the stream from host arrays in front,
                    the like-for-like of (a) for a caller whose stream is NOT in HBM yet.

Two hit densities at k = 31 on the bench workload (synth.py: 150 bp reads of a 100 Mbp uniform genome, 0.5 %
substitutions, 0.1 % N):
  sparse   the table counted from the first reads / 10^5 reads of the stream (Module 3's regime: few reads carry hits);
  dense    the table counted from the stream itself (every valid window is a hit), on the first --dense-reads reads
           only: the host loop of (a) takes minutes on the full stream at this density.
Wall clock (the paths differ in host work, copies and synchronisation, so events on one stream would not see them);
warm; best and median of --reps calls, the two paths alternated.  `hits_kernels_ms` (stat hits_us: the kh_* kernels,
HIP events) is reported next to the scan kernel's time (kdf_profile_read).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def density_case(name, k, ds, n_reads, table_reads, reps):
    import numpy as np
    import torch
    from kmer_denovo_filter_amd import KmerEngine, ReadStream

    L1 = ds.read_len + 1
    n = n_reads * L1
    T = (n + 63) // 64
    eng = KmerEngine(k, capacity_hint=max(1 << 16, table_reads * L1 * 2))
    eng.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), table_reads * L1)        # a prefix of the stream
    cap, distinct_keys, _ = eng.stats()
    offsets = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda:0") * L1
    host = ReadStream(ds.packed[:2 * T + 4].cpu().numpy().view(np.uint64), ds.invalid[:T + 2].cpu().numpy().view(np.uint64), n,
                      offsets.cpu().numpy())
    bits = torch.zeros(T, dtype=torch.int64, device="cuda:0")
    rows = torch.zeros(n_reads, dtype=torch.int64, device="cuda:0")                    # a row = 2 x uint32
    got = {}

    def scan_host():
        got["a"] = eng.scan(host)

    def device():
        eng.read_hits_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), n, offsets.data_ptr(), n_reads, bits.data_ptr(), rows.data_ptr())
        eng.synchronize()
        r = rows.cpu().numpy().view(np.uint32).reshape(n_reads, 2)
        cap_ = max(int(r[:, 0].sum(dtype=np.int64)), 1)
        pos = torch.empty(cap_, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        m = eng.hit_list_dev(bits.data_ptr(), n, None, 0, pos.data_ptr(), None, cap_)
        got["b"] = (r, pos[:m].cpu().numpy())

    def device_from_host():
        got["c"] = eng.scan_hits(host)

    calls = {"scan": scan_host, "device": device, "device_from_host": device_from_host}
    for fn in calls.values():                    # warm-up: code objects, staging buffers, the engine's scratch
        fn()
    runs = {name_: [] for name_ in calls}
    for _ in range(2):                           # alternate, so that drift of the box hits all alike
        for name_, fn in calls.items():
            runs[name_] += wall(fn, max(1, reps // 2))
    hits_mask, distinct = got["a"]
    r, pos = got["b"]
    assert np.array_equal(r[:, 1], distinct), "device rows disagree with the host reduction"
    assert np.array_equal(got["c"][0], r) and np.array_equal(got["c"][1], pos)
    want = np.flatnonzero(np.unpackbits(hits_mask[:T].view(np.uint8), bitorder="little")[:n])
    assert np.array_equal(pos, want), "hit list disagrees with the mask"
    out = {"case": name, "reads": n_reads, "positions": n, "table_reads": table_reads, "log2cap": cap.bit_length() - 1,
           "table_keys": int(distinct_keys), "hits": int(len(pos)), "reads_with_hits": int((r[:, 0] > 0).sum())}
    for name_, ts in runs.items():
        out[name_ + "_ms"] = round(min(ts), 3)
        out[name_ + "_median_ms"] = round(statistics.median(ts), 3)
    out["scan_over_device"] = round(out["scan_ms"] / out["device_ms"], 2)
    out["scan_over_device_from_host"] = round(out["scan_ms"] / out["device_from_host_ms"], 2)
    eng.profile(True)
    device()
    ms, launches, _ = eng.profile_read()
    out["scan_kernel_ms"] = round(ms / max(1, launches), 4)
    out["hits_kernels_ms"] = round(eng.get_stat("hits_us") / 1000.0 / max(1, eng.get_stat("hits_passes")), 4)
    out["last_scan_path"] = eng.get_stat("last_scan_path")
    eng.profile(False)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--dense-reads", type=int, default=200_000, help="reads of the dense case (the host loop is slow there)")
    ap.add_argument("--sparse-one-in", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--k", type=int, default=31)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/module3.py measures on the GPU: no device visible")
    from kmer_denovo_filter_amd.synth import synth_stream
    ds = synth_stream(args.reads, args.read_len, seed=20260417, device="cuda:0", genome_seed=20260417)
    torch.cuda.synchronize()
    dense = min(args.dense_reads, args.reads)
    out = {"bench": "module3", "device": torch.cuda.get_device_name(0), "workload": "synth", "k": args.k, "cases": [
        density_case("sparse", args.k, ds, args.reads, max(1, args.reads // args.sparse_one_in), args.reps),
        density_case("dense", args.k, ds, dense, dense, args.reps)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
