#!/usr/bin/env python3
"""Module 3's coverage sums on the device (kdf_hit_coverage_dev + kdf_coverage_list_dev) against the host loop of
``scan_bam_module3`` (``_collect_kmer_ref_positions`` per informative read) over the SAME hits of the SAME stream in the
SAME run, on ONE MI355X, with ``read_hits_dev`` over that stream as the yardstick.

  (a) device     ``hit_coverage_dev`` of the resident hit mask, offsets and alignment arrays into two zeroed accumulators
                 of the genome's length, then ``coverage_list_dev`` (min_reads 1) over them; the list stays in HBM.
  (b) read_hits  ``read_hits_dev`` over the same stream: the scan and the per-read reduction that come before (a).
  (c) host loop  per read that holds a hit: ``_collect_kmer_ref_positions`` and the two Counter updates, from the hit
                 list already on the host.  On ``--host-reads`` reads only (the loop takes minutes on the whole stream
                 when hits are dense); ``host_loop_scaled_ms`` is that time x (reads with hits / reads timed) and is
                 labelled as scaled.
  equal          the device sums of exactly the reads the host loop took (every other ref_start = -1) against the host
                 loop's Counters, position by position.

Stream: synth.py's 150 bp reads; per read a random CIGAR (150M, soft clips, an insertion, a deletion) and a random
leftmost position on a ``--genome`` bp line.  Two hit densities at k = 31, as benchmarks/module3.py cuts them: sparse
(table counted from reads / 10^5 reads) and dense (table counted from the stream itself, first --dense-reads reads).
Wall clock, warm, best and median of --reps; ``coverage_kernels_ms`` is stat coverage_us per call (HIP events).  One
JSON line."""
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


def random_alignments(rng, n_reads, read_len, genome):
    """-> (cigar uint32, cigar_offsets int64[n + 1], ref_start int64[n]): four CIGAR shapes that consume read_len bases"""
    import numpy as np
    kind = rng.integers(0, 10, n_reads)
    n_ops = np.where(kind < 6, 1, 3)
    co = np.concatenate(([0], np.cumsum(n_ops))).astype(np.int64)
    cg = np.zeros(int(co[-1]), np.uint32)
    a = rng.integers(20, read_len - 40, n_reads)
    w = lambda op, ln: (ln.astype(np.uint32) << np.uint32(4)) | np.uint32(op)
    full = np.full(n_reads, read_len)
    one = kind < 6
    cg[co[:-1][one]] = w(0, full[one])
    clip = (kind >= 6) & (kind < 8)                                   # aS (L - a - 5)M 5S
    cg[co[:-1][clip]] = w(4, a[clip]); cg[co[:-1][clip] + 1] = w(0, full[clip] - a[clip] - 5); cg[co[:-1][clip] + 2] = w(4, np.full(clip.sum(), 5))
    ins = kind == 8                                                   # aM 3I (L - a - 3)M
    cg[co[:-1][ins]] = w(0, a[ins]); cg[co[:-1][ins] + 1] = w(1, np.full(ins.sum(), 3)); cg[co[:-1][ins] + 2] = w(0, full[ins] - a[ins] - 3)
    dele = kind == 9                                                  # aM 7D (L - a)M
    cg[co[:-1][dele]] = w(0, a[dele]); cg[co[:-1][dele] + 1] = w(2, np.full(dele.sum(), 7)); cg[co[:-1][dele] + 2] = w(0, full[dele] - a[dele])
    return cg, co, rng.integers(0, genome, n_reads).astype(np.int64)


def density_case(name, k, ds, n_reads, table_reads, genome, host_reads, reps, seed):
    import collections
    import numpy as np
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.core.bam_scanner import _collect_kmer_ref_positions

    L1 = ds.read_len + 1
    n = n_reads * L1
    T = (n + 63) // 64
    span = genome + 2 * L1
    eng = KmerEngine(k, capacity_hint=max(1 << 16, table_reads * L1 * 2))
    eng.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), table_reads * L1)
    rng = np.random.default_rng(seed)
    cg, co, rs = random_alignments(rng, n_reads, ds.read_len, genome)
    up = lambda a: torch.from_numpy(a).cuda()
    d_cg, d_co, d_rs = up(cg.view(np.int32)), up(co), up(rs)
    offsets = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda:0") * L1
    bits = torch.zeros(T, dtype=torch.int64, device="cuda:0")
    rows = torch.zeros(n_reads, dtype=torch.int64, device="cuda:0")
    kcov = torch.zeros(span, dtype=torch.int32, device="cuda:0")
    rcov = torch.zeros(span, dtype=torch.int32, device="cuda:0")
    got = {}

    def read_hits():
        eng.read_hits_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), n, offsets.data_ptr(), n_reads, bits.data_ptr(), rows.data_ptr())
        eng.synchronize()

    def coverage(d_start=None):
        kcov.zero_(); rcov.zero_()
        torch.cuda.synchronize()
        eng.hit_coverage_dev(bits.data_ptr(), n, offsets.data_ptr(), n_reads, (d_rs if d_start is None else d_start).data_ptr(),
                             d_cg.data_ptr(), len(cg), d_co.data_ptr(), kcov.data_ptr(), rcov.data_ptr(), span)
        _, m = eng._coverage_list_dev(kcov.data_ptr(), rcov.data_ptr(), 0, span, 1, None, None, None, 0)
        pos = torch.empty(max(m, 1), dtype=torch.int64, device="cuda:0")
        kv = torch.empty(max(m, 1), dtype=torch.int32, device="cuda:0")
        rv = torch.empty(max(m, 1), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        eng.coverage_list_dev(kcov.data_ptr(), rcov.data_ptr(), 0, span, 1, pos.data_ptr(), kv.data_ptr(), rv.data_ptr(), m)
        got["list"] = (pos[:m], kv[:m], rv[:m])

    read_hits(); coverage()                                           # warm-up: code objects, scratch
    runs = {"device": [], "read_hits": []}
    for _ in range(2):
        runs["read_hits"] += wall(read_hits, max(1, reps // 2))
        runs["device"] += wall(coverage, max(1, reps // 2))
    r = rows.cpu().numpy().view(np.uint32).reshape(n_reads, 2)
    with_hits = np.flatnonzero(r[:, 0] > 0)
    n_hits = int(r[:, 0].sum(dtype=np.int64))
    covered = int(len(got["list"][0]))
    # the host loop over the first host_reads reads that hold hits, from the hit list on the host
    take = with_hits[:host_reads]
    dpos = torch.empty(max(n_hits, 1), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    m = eng.hit_list_dev(bits.data_ptr(), n, None, 0, dpos.data_ptr(), None, max(n_hits, 1))
    pos = dpos[:m].cpu().numpy()
    lo = np.searchsorted(pos, take * L1)
    hi = np.searchsorted(pos, take * L1 + ds.read_len)
    tuples = [[(int(w) & 15, int(w) >> 4) for w in cg[co[i]:co[i + 1]]] for i in take.tolist()]
    t0 = time.perf_counter()
    hk, hr = collections.Counter(), collections.Counter()
    for j, i in enumerate(take.tolist()):
        cov = _collect_kmer_ref_positions(int(rs[i]), tuples[j], ds.read_len, pos[lo[j]:hi[j]] - i * L1, k)
        hk.update(cov)
        for p in cov:
            hr[p] += 1
    host_ms = (time.perf_counter() - t0) * 1e3
    only = np.full(n_reads, -1, np.int64)
    only[take] = rs[take]
    coverage(up(only))
    lp, lk, lr = (x.cpu().numpy() for x in got["list"])
    equal = (dict(zip(lp.tolist(), lk.view(np.uint32).tolist())) == dict(hk)
             and dict(zip(lp.tolist(), lr.view(np.uint32).tolist())) == dict(hr))
    out = {"case": name, "reads": n_reads, "positions": n, "table_reads": table_reads, "hits": n_hits,
           "reads_with_hits": int(len(with_hits)), "cigar_ops": int(len(cg)), "span": span, "covered_positions": covered,
           "host_loop_reads": int(len(take)), "host_loop_ms": round(host_ms, 3),
           "host_loop_scaled_ms": round(host_ms * len(with_hits) / max(1, len(take)), 1),
           "host_loop_is_scaled": bool(len(take) < len(with_hits)), "equal": bool(equal)}
    for name_, ts in runs.items():
        out[name_ + "_ms"] = round(min(ts), 3)
        out[name_ + "_median_ms"] = round(statistics.median(ts), 3)
    out["host_scaled_over_device"] = round(out["host_loop_scaled_ms"] / out["device_ms"], 1)
    out["device_over_read_hits"] = round(out["device_ms"] / out["read_hits_ms"], 3)
    eng.profile(True)
    coverage()
    out["coverage_kernels_ms"] = round(eng.get_stat("coverage_us") / 1000.0, 4)       # the two calls of one (a)
    eng.profile(False)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--dense-reads", type=int, default=200_000, help="reads of the dense case (its table holds every window)")
    ap.add_argument("--sparse-one-in", type=int, default=100_000)
    ap.add_argument("--genome", type=int, default=100_000_000, help="length of the line the reads are placed on")
    ap.add_argument("--host-reads", type=int, default=2000, help="reads with hits the host loop is timed on")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--k", type=int, default=31)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/coverage.py measures on the GPU: no device visible")
    from kmer_denovo_filter_amd.synth import synth_stream
    ds = synth_stream(args.reads, args.read_len, seed=20260417, device="cuda:0", genome_seed=20260417)
    torch.cuda.synchronize()
    dense = min(args.dense_reads, args.reads)
    out = {"bench": "coverage", "device": torch.cuda.get_device_name(0), "workload": "synth", "k": args.k, "cases": [
        density_case("sparse", args.k, ds, args.reads, max(1, args.reads // args.sparse_one_in), args.genome, args.host_reads, args.reps, 1),
        density_case("dense", args.k, ds, dense, dense, args.genome, args.host_reads, args.reps, 2)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
