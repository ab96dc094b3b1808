#!/usr/bin/env python3
"""VCF mode on the device (kdf_variant_windows_dev + kdf_hit_keys_dev, kdf_variant_evidence_dev) against the host loop
of the VCF pipeline (``extract_variant_spanning_kmers`` + ``read_supports_alt`` per (read, variant), then
``annotate_variants`` over the k-mer string sets) on the SAME reads and variants in the SAME run, on ONE MI355X.

  (a) windows    ``variant_windows_dev`` (the sizing call and the writing call, as the driver runs them) and
                 ``hit_keys_dev`` over the resident stream, alignment arrays and variant arrays.
  (b) evidence   ``variant_evidence_dev`` of (a)'s key rows against a table that holds those keys as a filter with a
                 "parent" counted into it (every second read of the same stream, ``count --if``).
  (c) host loop  per read: an ``AlignedRead``, and for every variant inside its reference interval the two helpers;
                 then ``annotate_variants`` with the parent counts as a dict.  On the first ``--host-reads`` reads
                 only; ``host_loop_scaled_ms`` is that time x (reads / reads timed) and is labelled as scaled.
  equal          the device annotations of exactly the reads the host loop took (every other ref_start = -1) against
                 ``annotate_variants`` of the host loop, variant by variant.

Reads: ``--depth`` reads of ``--read-len`` bases over each of ``--variants`` variants (SNVs, insertions, deletions) on
a random genome, each with a random CIGAR (all M, soft clips, an insertion, a deletion) and random base qualities.
Nothing outside the repository is read.  Wall clock, warm, best and median of --reps; ``*_kernels_ms`` is stat
variants_us (HIP events around the kv_* kernels; hit_keys' kernel is not in it).  One JSON line."""
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


def make_case(rng, n_var, depth, read_len, genome_len):
    """-> dict: ascii reads, per-read alignment, qualities, the variant arrays and the variant dicts of the host path"""
    import numpy as np
    genome = rng.integers(0, 4, genome_len).astype(np.uint8)
    letters = np.frombuffer(b"ACGT", np.uint8)
    cand = np.unique(rng.integers(read_len, genome_len - 2 * read_len, n_var + n_var // 4 + 16))
    vpos = np.sort(rng.choice(cand, n_var, replace=False)).astype(np.int64)
    kind = rng.integers(0, 3, n_var)                                  # 0 SNV, 1 insertion, 2 deletion
    span = np.where(kind == 1, rng.integers(2, 13, n_var), 1).astype(np.uint32)
    ref_len = np.where(kind == 2, rng.integers(2, 9, n_var), 1).astype(np.uint32)
    alts = []
    for v in range(n_var):
        a = letters[genome[vpos[v]:vpos[v] + 1]].tobytes()            # the reference base first: reads that carry it match a SNV
        alts.append(a + letters[rng.integers(0, 4, int(span[v]) - 1)].tobytes())
    n_reads = n_var * depth
    start = (np.repeat(vpos, depth) - rng.integers(10, read_len - 10, n_reads)).astype(np.int64)
    order = np.argsort(start, kind="stable")
    start = start[order]
    shape = rng.integers(0, 10, n_reads)
    a = rng.integers(20, read_len - 40, n_reads)
    cg, co = [], [0]
    for i in range(n_reads):
        L, x = read_len, int(a[i])
        ops = ([(0, L)] if shape[i] < 6 else [(4, x), (0, L - x - 5), (4, 5)] if shape[i] < 8
               else [(0, x), (1, 3), (0, L - x - 3)] if shape[i] == 8 else [(0, x), (2, 7), (0, L - x)])
        cg += [(ln << 4) | op for op, ln in ops]
        co.append(len(cg))
    ascii_ = np.empty(n_reads * read_len, np.uint8)
    for i0 in range(0, n_reads, 1 << 16):                             # (in pieces: the index array is 8 bytes per base)
        idx = start[i0:i0 + (1 << 16), None] + np.arange(read_len)[None, :]
        ascii_[i0 * read_len:i0 * read_len + idx.size] = letters[genome[idx]].reshape(-1)
    quals = rng.integers(25, 41, n_reads * read_len).astype(np.uint8)
    quals[rng.random(len(quals)) < 0.01] = 5                          # one base in a hundred fails --min-baseq
    variants = [{"chrom": "g", "pos": int(vpos[v]), "ref": "A" * int(ref_len[v]), "alt": alts[v].decode()} for v in range(n_var)]
    ao = np.concatenate(([0], np.cumsum([len(x) for x in alts]))).astype(np.int64)
    return {"ascii": ascii_, "offs": np.arange(n_reads + 1, dtype=np.int64) * read_len, "start": start,
            "cigar": np.asarray(cg, np.uint32), "cigar_offsets": np.asarray(co, np.int64), "quals": quals,
            "qual_offsets": np.arange(n_reads + 1, dtype=np.int64) * read_len, "var_pos": vpos, "var_span": span,
            "var_ref_len": ref_len, "alt": b"".join(alts), "alt_offsets": ao, "variants": variants, "n_reads": n_reads}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=10000)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--host-reads", type=int, default=3000, help="reads the host loop is timed on")
    ap.add_argument("--min-baseq", type=int, default=20)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--k", type=int, default=31)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/vcf_device.py measures on the GPU: no device visible")
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    from kmer_denovo_filter_amd.alignment import AlignedRead
    from kmer_denovo_filter_amd.kmer_utils import extract_variant_spanning_kmers, read_supports_alt
    from kmer_denovo_filter_amd.reads import kmers_to_keys, stream_words
    from kmer_denovo_filter_amd.vcf.device import annotations_from_rows
    from kmer_denovo_filter_amd.vcf.pipeline import _variant_key, annotate_variants

    k, L = args.k, args.read_len
    rng = np.random.default_rng(20261019)
    c = make_case(rng, args.variants, args.depth, L, args.genome)
    st = ReadStream.from_ascii(c["ascii"], c["offs"])
    n, nr, nv = int(st.n_bases), c["n_reads"], args.variants
    pw, mw = stream_words(n)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
    d_p, d_m, d_o = up(st.packed[:pw]), up(st.invalid[:mw]), up(st.offsets)
    d_rs, d_cg, d_co = up(c["start"]), up(c["cigar"]), up(c["cigar_offsets"])
    d_q, d_qo = up(c["quals"]), up(c["qual_offsets"])
    d_vp, d_vs, d_vr = up(c["var_pos"]), up(c["var_span"]), up(c["var_ref_len"])
    d_alt, d_ao = up(np.frombuffer(c["alt"], np.uint8)), up(c["alt_offsets"])
    eng = KmerEngine(k, capacity_hint=1 << 16)
    W = eng.key_words
    got = {}

    def windows(d_start=None):
        args_ = (d_p.data_ptr(), d_m.data_ptr(), n, d_o.data_ptr(), nr, (d_rs if d_start is None else d_start).data_ptr(), d_cg.data_ptr(),
                 len(c["cigar"]), d_co.data_ptr(), d_q.data_ptr(), len(c["quals"]), d_qo.data_ptr(), args.min_baseq, d_vp.data_ptr(),
                 d_vs.data_ptr(), d_vr.data_ptr(), nv, d_alt.data_ptr(), len(c["alt"]), d_ao.data_ptr())
        n_pairs, n_ent = eng.variant_windows_dev(*args_, None, None, None, 0, None, None, 0)
        o = {"pr": torch.empty(max(n_pairs, 1), dtype=torch.int64, device=dev), "pv": torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev),
             "pf": torch.empty(max(n_pairs, 1), dtype=torch.uint8, device=dev), "ep": torch.empty(max(n_ent, 1), dtype=torch.int64, device=dev),
             "epair": torch.empty(max(n_ent, 1), dtype=torch.int64, device=dev), "keys": torch.empty((max(n_ent, 1), W), dtype=torch.int64, device=dev)}
        torch.cuda.synchronize()
        eng.variant_windows_dev(*args_, o["pr"].data_ptr(), o["pv"].data_ptr(), o["pf"].data_ptr(), n_pairs, o["ep"].data_ptr(), o["epair"].data_ptr(), n_ent)
        eng.hit_keys_dev(d_p.data_ptr(), n, o["ep"].data_ptr(), n_ent, o["keys"].data_ptr())
        eng.synchronize()
        o["n_pairs"], o["n_ent"] = n_pairs, n_ent
        got["w"] = o

    def evidence():
        o = got["w"]
        o["prow"] = torch.empty((max(o["n_pairs"], 1), 2), dtype=torch.int32, device=dev)
        o["vrow"] = torch.empty((nv, 8), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        eng.variant_evidence_dev(o["keys"].data_ptr(), o["epair"].data_ptr(), o["n_ent"], o["pv"].data_ptr(), o["pf"].data_ptr(), o["n_pairs"], nv,
                                 o["prow"].data_ptr(), o["vrow"].data_ptr())
        eng.synchronize()

    windows()                                                         # warm-up, and the keys of the filter
    o = got["w"]
    keys = o["keys"][:o["n_ent"]]
    if W <= 2:
        lo = keys[:, 0].contiguous()
        hi = keys[:, 1].contiguous() if W == 2 else None
        torch.cuda.synchronize()
        eng.load_filter_dev(lo.data_ptr(), hi.data_ptr() if W == 2 else None, o["n_ent"])
    else:
        eng.load_filter_dev(keys.contiguous().data_ptr(), None, o["n_ent"])
    half = ReadStream.from_ascii(c["ascii"][:(nr // 2) * L * 2].reshape(-1, 2 * L)[:, :L].reshape(-1), np.arange(nr // 2 + 1, dtype=np.int64) * L)
    eng.count_filtered(half)                                          # the "parent": every second read
    evidence()
    runs = {"windows": [], "evidence": []}
    for _ in range(2):
        runs["windows"] += wall(windows, max(1, args.reps // 2))
        runs["evidence"] += wall(evidence, max(1, args.reps // 2))
    out = {"bench": "vcf_device", "device": torch.cuda.get_device_name(0), "workload": "synth", "k": k, "reads": nr, "variants": nv,
           "positions": n, "cigar_ops": int(len(c["cigar"])), "pairs": int(o["n_pairs"]), "entries": int(o["n_ent"]),
           "distinct_child_keys": int(eng.count_ge(0)), "parent_found_keys": int(eng.count_ge(1))}
    for name, ts in runs.items():
        out[name + "_ms"] = round(min(ts), 3)
        out[name + "_median_ms"] = round(statistics.median(ts), 3)
    eng.profile(True)
    windows()
    out["windows_kernels_ms"] = round(eng.get_stat("variants_us") / 1000.0, 4)           # (both calls of one (a))
    evidence()
    out["evidence_kernels_ms"] = round(eng.get_stat("variants_us") / 1000.0 - out["windows_kernels_ms"], 4)
    eng.profile(False)

    # ---- the host loop on the first host_reads reads, and the device path on exactly those
    take = min(args.host_reads, nr)
    seqs = c["ascii"][:take * L].tobytes().decode()
    tuples = [[(int(w) & 15, int(w) >> 4) for w in c["cigar"][c["cigar_offsets"][i]:c["cigar_offsets"][i + 1]]] for i in range(take)]
    refl = [sum(ln for op, ln in t if op in (0, 2, 3, 7, 8)) for t in tuples]
    lo_v = np.searchsorted(c["var_pos"], c["start"][:take], side="left")
    hi_v = np.searchsorted(c["var_pos"], c["start"][:take] + np.asarray(refl), side="left")
    variants = c["variants"]
    t0 = time.perf_counter()
    per_variant = {}
    for i in range(take):
        read = AlignedRead(f"r{i}", 0, 0, "g", int(c["start"][i]), 60, tuples[i], seqs[i * L:(i + 1) * L], c["quals"][i * L:(i + 1) * L])
        for v in range(int(lo_v[i]), int(hi_v[i])):
            var = variants[v]
            ks = extract_variant_spanning_kmers(read, var["pos"], k, args.min_baseq, ref=var["ref"], alt=var["alt"])
            if ks:
                sup = read_supports_alt(read, var["pos"], var["ref"], var["alt"], min_baseq=args.min_baseq)
                per_variant.setdefault(_variant_key(var), []).append((read.query_name, ks, sup))
    host_windows_ms = (time.perf_counter() - t0) * 1e3
    every = sorted({x for recs in per_variant.values() for _n, ks, _s in recs for x in ks})
    klo, khi = kmers_to_keys(every, k) if every else (np.zeros(0, np.uint64), None)
    cnt = eng.query(klo, khi) if every else np.zeros(0, np.uint32)
    found = {x: int(v) for x, v in zip(every, cnt.tolist()) if v > 0}
    t0 = time.perf_counter()
    want = annotate_variants(variants, per_variant, found)
    host_annotate_ms = (time.perf_counter() - t0) * 1e3
    only = np.full(nr, -1, np.int64)
    only[:take] = c["start"][:take]
    windows(up(only))
    evidence()
    o = got["w"]
    P = o["n_pairs"]
    rows, _ = annotations_from_rows(nv, o["pv"][:P].cpu().numpy().view(np.uint32), o["pr"][:P].cpu().numpy(), o["pf"][:P].cpu().numpy(),
                                    o["prow"][:P].cpu().numpy().view(np.uint32), o["vrow"].cpu().numpy().view(np.uint64))
    equal = all(rows[v] == want[_variant_key(var)] for v, var in enumerate(variants))
    host_ms = host_windows_ms + host_annotate_ms
    out.update({"host_loop_reads": take, "host_windows_ms": round(host_windows_ms, 1), "host_annotate_ms": round(host_annotate_ms, 1),
                "host_loop_scaled_ms": round(host_ms * nr / max(1, take), 1), "host_loop_is_scaled": bool(take < nr),
                "sample_pairs": int(P), "equal": bool(equal)})
    out["host_scaled_over_device"] = round(out["host_loop_scaled_ms"] / (out["windows_ms"] + out["evidence_ms"]), 1)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
