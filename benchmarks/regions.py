#!/usr/bin/env python3
"""Module 3's regions on the device (kdf_cluster_intervals_dev + a gather + kdf_group_distinct_dev) against the host
path it replaces under ``KDF_DEVICE_REGIONS=1``: per kept read ``np.unique`` + ``keys_to_kmers`` + ``set`` (what
``_DeviceCoverage.batch`` does today to hand ``read_hits`` a set of k-mer STRINGS), then ``_cluster_read_hits`` over
those sets.  ONE MI355X, the same reads and the same key rows on both sides.

  (a) device   the intervals of all reads -> ``cluster_intervals_dev`` (cap = reads) -> every hit's group =
               region_of[its read] (a torch gather) -> ``group_distinct_dev`` over the resident key rows.  Timed whole
               and per stage (cluster / gather / distinct, each closed by a synchronisation).
  (b) host     the string sets and the sweep over ``--host-reads`` reads, cut at a region boundary (the reads of the first
               G regions); ``host_scaled_ms`` is that time x (reads / reads timed) and is labelled as scaled: both
               parts are linear in the reads and their hits.
  equal        the device calls over exactly the host's subset against the host's regions and ``len(region_kmers)``.

Workload: ``--reads`` informative reads of 150 bp clustered around random centres of a 3 Gbp line cut into 24 contigs
(ranks 0..23), ``--hits`` hits per read on average, every read's keys drawn from a pool of 60 keys of its centre, so the
reads of a region share keys.  Key rows of k = 31 (one word) and k = 101 (four words).  Wall clock, warm, median of
``--reps`` with the spread; ``regions_kernels_ms`` is stat regions_us of one (a) (HIP events, the sort included).  One
JSON line, also written to profiles/regions_bench.json."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINE = 3_000_000_000
CONTIGS = 24
READ_LEN = 150
POOL = 60


def mix(x):
    """splitmix64 over a uint64 array"""
    import numpy as np
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def workload(rng, n_reads, hits, k, words):
    """-> chrom, start, end int64[n_reads]; hit_read int64[h] (ascending), keys uint64 (h, words)"""
    import numpy as np
    n_centres = max(1, n_reads // 20)
    centre = np.sort(rng.integers(0, LINE - 1000, n_centres))
    of = np.sort(rng.integers(0, n_centres, n_reads))                 # each read's centre; reads in line order, roughly
    pos = centre[of] + rng.integers(0, 400, n_reads)
    band = LINE // CONTIGS
    chrom = np.minimum(pos // band, CONTIGS - 1)
    start = pos - chrom * band
    per_read = rng.integers(max(1, hits - 10), hits + 11, n_reads)
    hit_read = np.repeat(np.arange(n_reads), per_read)
    key_id = (of[hit_read] * 64 + rng.integers(0, POOL, len(hit_read))).astype(np.uint64)
    keys = np.empty((len(hit_read), words), np.uint64)
    for j in range(words):
        keys[:, j] = mix(key_id * np.uint64(words) + np.uint64(j))
    top_bits = 2 * k - 64 * (words - 1)
    if top_bits < 64:
        keys[:, words - 1] &= np.uint64((1 << top_bits) - 1)
    return chrom.astype(np.int64), start.astype(np.int64), (start + READ_LEN).astype(np.int64), hit_read.astype(np.int64), keys


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


def spread(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": len(ts)}


def device_run(eng, d, md, stages=None):
    """one (a) over the device arrays of d; -> (n_regions, d_region_of, d_rows, d_counts); stages: {name: [ms]} to append to"""
    import torch
    n, h, words = d["n"], d["h"], d["words"]
    t = [time.perf_counter()]

    def lap():
        if stages is not None:
            torch.cuda.synchronize(); eng.synchronize()
            t.append(time.perf_counter())
    m = eng.cluster_intervals_dev(d["chrom"].data_ptr(), d["start"].data_ptr(), d["end"].data_ptr(), n, md, d["region_of"].data_ptr(),
                                  d["rows"].data_ptr(), n)
    lap()
    group = d["region_of"][d["hit_read"]]
    torch.cuda.synchronize()
    lap()
    eng.group_distinct_dev(group.data_ptr(), d["keys"].data_ptr(), words, h, m, d["counts"].data_ptr())
    eng.synchronize()
    lap()
    if stages is not None:
        for name, a, b in zip(("cluster", "gather", "distinct"), t, t[1:]):
            stages.setdefault(name, []).append((b - a) * 1e3)
    return m


def to_device(chrom, start, end, hit_read, keys):
    import numpy as np
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).cuda()
    n, h = len(chrom), len(hit_read)
    return {"n": n, "h": h, "words": keys.shape[1], "chrom": up(chrom), "start": up(start), "end": up(end), "hit_read": up(hit_read),
            "keys": up(keys), "region_of": torch.empty(max(n, 1), dtype=torch.int64, device="cuda"),
            "rows": torch.empty((max(n, 1), 4), dtype=torch.int64, device="cuda"),
            "counts": torch.empty(max(n, 1), dtype=torch.int64, device="cuda")}


def case(k, n_reads, hits, md, host_reads, reps, seed):
    import numpy as np
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.discovery.regions import _cluster_read_hits
    from kmer_denovo_filter_amd.keys import key_words
    from kmer_denovo_filter_amd.reads import keys_to_kmers

    W = key_words(k)
    rng = np.random.default_rng(seed)
    chrom, start, end, hit_read, keys = workload(rng, n_reads, hits, k, W)
    eng = KmerEngine(k, capacity_hint=1 << 10)                        # (the table is not used: any engine serves)
    d = to_device(chrom, start, end, hit_read, keys)
    torch.cuda.synchronize()
    m = device_run(eng, d, md)                                        # warm-up: code objects, scratch
    whole = wall(lambda: device_run(eng, d, md), reps)
    stages = {}
    for _ in range(reps):
        device_run(eng, d, md, stages)
    eng.profile(True)
    device_run(eng, d, md)
    kernels_ms = eng.get_stat("regions_us") / 1000.0
    eng.profile(False)
    region_of = d["region_of"][:n_reads].cpu().numpy()

    # (b) the host path over the reads of the first G regions
    per_region = np.bincount(region_of, minlength=m)
    G = int(np.searchsorted(np.cumsum(per_region), host_reads, side="left")) + 1
    take = np.flatnonzero(region_of < G)
    lo = np.searchsorted(hit_read, take, side="left")
    hi = np.searchsorted(hit_read, take, side="right")
    names = [f"contig{c:02d}" for c in range(CONTIGS)]                 # (name order = rank order)
    t0 = time.perf_counter()
    sets = []
    for a, b in zip(lo.tolist(), hi.tolist()):                        # _DeviceCoverage.batch, per kept read
        u = np.unique(keys[a:b], axis=0)
        sets.append(set(keys_to_kmers(u if W > 2 else np.ascontiguousarray(u[:, 0]), np.ascontiguousarray(u[:, 1]) if W == 2 else None, k)))
    t1 = time.perf_counter()
    read_hits = [(names[chrom[i]], int(start[i]), int(end[i]), f"r{i}", s, False) for i, s in zip(take.tolist(), sets)]
    h_regions, h_reads, h_kmers = _cluster_read_hits(read_hits, md)
    t2 = time.perf_counter()
    sets_ms, sweep_ms = (t1 - t0) * 1e3, (t2 - t1) * 1e3

    # equal: the device calls over exactly that subset
    sub_hits = np.concatenate([np.arange(a, b) for a, b in zip(lo.tolist(), hi.tolist())] or [np.zeros(0, np.int64)])
    ds = to_device(chrom[take], start[take], end[take], np.searchsorted(take, hit_read[sub_hits]), keys[sub_hits])
    torch.cuda.synchronize()
    ms = device_run(eng, ds, md)
    rows = ds["rows"][:ms].cpu().numpy()
    counts = ds["counts"][:ms].cpu().numpy()
    equal = ([(names[c], s, e) for c, s, e, _ in rows.tolist()] == h_regions
             and rows[:, 3].tolist() == [len(h_reads[key]) for key in h_regions]
             and counts.tolist() == [len(h_kmers[key]) for key in h_regions])
    assert equal, f"k={k}: the device's regions or counts differ from the host path's on the subset"
    scale = n_reads / max(1, len(take))
    dev = spread(whole)
    out = {"k": k, "words": W, "reads": n_reads, "hits": int(len(hit_read)), "regions": int(m), "merge_distance": md,
           "device": dev, "device_stages": {name: spread(ts) for name, ts in stages.items()},
           "regions_kernels_ms": round(kernels_ms, 3),
           "host_reads": int(len(take)), "host_regions": len(h_regions), "host_sets_ms": round(sets_ms, 1), "host_sweep_ms": round(sweep_ms, 1),
           "host_scaled_ms": round((sets_ms + sweep_ms) * scale, 1), "host_is_scaled": bool(len(take) < n_reads),
           "host_scaling": f"x {n_reads} / {len(take)} reads (linear in reads and hits)", "equal": bool(equal)}
    out["host_scaled_over_device"] = round(out["host_scaled_ms"] / dev["median_ms"], 1)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--hits", type=int, default=25, help="hits per read on average")
    ap.add_argument("--merge-distance", type=int, default=500)
    ap.add_argument("--host-reads", type=int, default=4000, help="reads the host path is timed on (cut at a region boundary)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 101])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/regions.py measures on the GPU: no device visible")
    if args.reps < 5:
        raise SystemExit("--reps: the median is taken over at least 5 warm repetitions")
    out = {"bench": "regions", "device": torch.cuda.get_device_name(0), "workload": "synth", "line_bp": LINE, "contigs": CONTIGS,
           "cases": [case(k, args.reads, args.hits, args.merge_distance, args.host_reads, args.reps, 20261020 + k) for k in args.ks]}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
