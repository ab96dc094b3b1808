#!/usr/bin/env python3
"""The index record codec on the device (kdf_index_encode, kdf_index_decode, kdf_jf_order and the device writers and
loaders of ``jf_io.py``) against the host codec it stands beside, ONE MI355X, the same ``--n`` distinct random canonical
keys with counts at every k of ``--ks`` on both sides, everything in one run:

  encode   the encode kernel alone, the whole body into one device buffer, against a device-to-device copy of the same
           number of bytes (the floor of anything that writes that body once)
  decode   the decode kernel alone over the body in device memory (one call: it ends in the synchronisation that
           returns the bad record), against the same copy
  write    ``devkeys.dump_ge_counts`` + ``write_index_device`` against ``export_ge`` + ``write_index``, from one engine
           that holds the keys, alternating, into ``--dir`` (the same directory for both)
  load     ``load_index_into_device`` against ``load_index_into`` into a cleared engine each, alternating; the two
           tables are compared key by key and count by count
  jf       ``write_jellyfish_index_device`` (``jf_order_dev`` + encode through the permutation) against
           ``write_jellyfish_index``, k <= 63 only

Wall clock around work that ends in a synchronisation, warm (one untimed run of each first), median of ``--reps``
(kernels) and ``--file-reps`` (files) with the spread; ``*_kernels_ms`` is stat indexcodec_us of one more call (HIP
events).  Every pair of files is compared byte for byte.  One JSON line, also written to
profiles/index_codec_bench.json."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": len(ts)}


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


def gbps(nbytes, s):
    return round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 2)


def same_file(a, b):
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 24), fb.read(1 << 24)
            if x != y:
                return False
            if not x:
                return True


def alternate(host, device, reps):
    host(); device()
    t = {"host": [], "device": []}
    for _ in range(reps):
        t["host"] += wall(host, 1)
        t["device"] += wall(device, 1)
    h, d = spread(t["host"]), spread(t["device"])
    return h, d, round(h["median_ms"] / d["median_ms"], 2)


def case(k, n, reps, file_reps, out_dir, seed):
    import numpy as np
    import torch
    from kmer_denovo_filter_amd import KmerEngine, devkeys, jf_io, keys

    rng = np.random.default_rng(seed)
    words = keys.from_codes(rng.integers(0, 4, (n, k), dtype=np.uint8), canonical=True)
    rows = np.unique(np.ascontiguousarray(words.T), axis=0)
    words = np.ascontiguousarray(rows.T)
    words = np.ascontiguousarray(words[:, keys.order(words)])          # distinct, ascending
    n = words.shape[1]
    counts = rng.integers(1, 1 << 16, n, dtype=np.uint64).astype(np.uint32)
    lo, hi = keys.to_pair(words, zero_hi=False)
    W = keys.n_words(k)
    dlo, dhi = devkeys.from_host(lo, hi, W == 2)
    dcnt = torch.from_numpy(counts.view(np.int32)).cuda()
    eng = KmerEngine(31, capacity_hint=1 << 10)                       # (the table is not used: any engine serves)
    R = eng.index_record_bytes(k)
    total = n * R
    body = torch.empty(total, dtype=torch.uint8, device="cuda")
    other = torch.empty(total, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr() if t is not None else None
    out = {"k": k, "words": W, "n": n, "record_bytes": R, "body_bytes": total}

    # encode and decode: the kernels alone against a copy of the same bytes
    def enc():
        eng.index_encode_dev(p(dlo), p(dhi), p(dcnt), None, n, k, 0, total, body.data_ptr())
        eng.synchronize()
    enc(); other.copy_(body)
    out["encode"] = spread(wall(enc, reps))
    out["d2d_copy"] = spread(wall(lambda: other.copy_(body), reps))
    out["encode_GBps"], out["d2d_copy_GBps"] = gbps(total, out["encode"]), gbps(total, out["d2d_copy"])
    plo = torch.empty((n, W) if W > 2 else n, dtype=torch.int64, device="cuda")
    phi = torch.empty(n, dtype=torch.int64, device="cuda") if W == 2 else None
    pcnt = torch.empty(n, dtype=torch.int32, device="cuda")

    def dec():
        eng.index_decode_dev(body.data_ptr(), n, k, 4, plo.data_ptr(), p(phi), pcnt.data_ptr())
    dec()
    assert torch.equal(plo, dlo) and (phi is None or torch.equal(phi, dhi)) and torch.equal(pcnt, dcnt), f"k={k}: decode(encode(x)) != x"
    out["decode"] = spread(wall(dec, reps))
    out["decode_GBps"] = gbps(total, out["decode"])
    eng.profile(True)
    u0 = eng.get_stat("indexcodec_us"); enc()
    out["encode_kernels_ms"] = round((eng.get_stat("indexcodec_us") - u0) / 1000.0, 3)
    u0 = eng.get_stat("indexcodec_us"); dec()
    out["decode_kernels_ms"] = round((eng.get_stat("indexcodec_us") - u0) / 1000.0, 3)
    eng.profile(False)
    del body, other, plo, phi, pcnt

    # write: from an engine that holds the keys, to a file
    host_jf, dev_jf = os.path.join(out_dir, f"host_k{k}.jf"), os.path.join(out_dir, f"dev_k{k}.jf")
    with KmerEngine(k, capacity_hint=n) as table:
        table.add_pairs(lo, hi, counts)

        def host_write():
            jf_io.write_index(host_jf, k, *table.export_ge(0))

        def dev_write():
            jf_io.write_index_device(dev_jf, k, *devkeys.dump_ge_counts(table, 0), engine=eng)
        out["write_host"], out["write_device"], out["write_host_over_device"] = alternate(host_write, dev_write, file_reps)
        assert same_file(host_jf, dev_jf), f"k={k}: the device writer's file differs from the host writer's"
        # ... the host path's two halves, once each: which one bounds it
        t0 = time.perf_counter(); dump = table.export_ge(0); t1 = time.perf_counter()
        jf_io.write_index(host_jf, k, *dump); t2 = time.perf_counter()
        out["write_host_stages"] = {"export_ge_ms": round((t1 - t0) * 1e3, 1), "write_index_ms": round((t2 - t1) * 1e3, 1)}
        del dump
    out["file_bytes"] = os.path.getsize(dev_jf)

    # load: the file into a cleared engine
    with KmerEngine(k, capacity_hint=n) as eh, KmerEngine(k, capacity_hint=n) as ed:
        def host_load():
            eh.clear()
            jf_io.load_index_into(eh, host_jf, expect_k=k)

        def dev_load():
            ed.clear()
            jf_io.load_index_into_device(ed, dev_jf, expect_k=k)
        os.environ.pop("KDF_DEVICE_INDEX", None)
        out["load_host"], out["load_device"], out["load_host_over_device"] = alternate(host_load, dev_load, file_reps)
        a, b = eh.export_ge(0), ed.export_ge(0)
        assert all(x is None and y is None or np.array_equal(x, y) for x, y in zip(a, b)), f"k={k}: the loaded tables differ"
        assert np.array_equal(a[2], counts) and len(a[0]) == n
        del a, b

    # Jellyfish's binary/sorted order
    if k <= 63:
        order = rng.permutation(n)
        slo, shi, scnt = lo[order], None if hi is None else hi[order], counts[order]
        dslo, dshi = devkeys.from_host(slo, shi, W == 2)
        dscnt = torch.from_numpy(scnt.view(np.int32)).cuda()

        def host_jfw():
            jf_io.write_jellyfish_index(host_jf, k, slo, shi, scnt)

        def dev_jfw():
            jf_io.write_jellyfish_index_device(dev_jf, k, dslo, dshi, dscnt)
        out["jf_write_host"], out["jf_write_device"], out["jf_write_host_over_device"] = alternate(host_jfw, dev_jfw, file_reps)
        assert same_file(host_jf, dev_jf), f"k={k}: the device Jellyfish writer's file differs from the host writer's"
        size = jf_io.read_header(dev_jf)[0]["size"]
        cols = jf_io.read_header(dev_jf)[0]["matrix1"]["columns"]
        perm = torch.empty(n, dtype=torch.int32, device="cuda")
        out["jf_order"] = spread(wall(lambda: eng.jf_order_dev(p(dslo), p(dshi), n, k, cols, size, perm.data_ptr()), reps))
    for f in (host_jf, dev_jf):
        os.remove(f)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000, help="keys per set (before duplicates are dropped)")
    ap.add_argument("--ks", type=int, nargs="+", default=[31, 63, 101])
    ap.add_argument("--reps", type=int, default=7, help="repetitions of the kernel-only timings")
    ap.add_argument("--file-reps", type=int, default=5, help="repetitions of the file timings (host and device alternate)")
    ap.add_argument("--dir", default=None, help="where both writers write (default: a temporary directory)")
    ap.add_argument("--parent", default="", help="the parent commit, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_codec_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/index_codec.py measures on the GPU: no device visible")
    if args.reps < 5 or args.file_reps < 3:
        raise SystemExit("--reps >= 5 and --file-reps >= 3: a median wants repetitions")
    from kmer_denovo_filter_amd import jf_io
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        out = {"bench": "index_codec", "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "parent": args.parent,
               "workload": "distinct random canonical keys, counts 1 .. 65535", "window_mb": jf_io._window_bytes() >> 20,
               "dir": "tmp" if args.dir is None else args.dir,
               "not_measured": ["a 30 GB index", "a disk slower than the page cache", "k = 201"],
               "cases": [case(k, args.n, args.reps, args.file_reps, d, 20261021 + k) for k in args.ks]}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
