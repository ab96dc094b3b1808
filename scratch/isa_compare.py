#!/usr/bin/env python3
"""usage: scratch/isa_compare.py PARENT.s BUILD.s  -- device assembly of one unit (hipcc ... -S --cuda-device-only) before and
after a change: per function the static instruction counts vector / scalar / LDS / global+scratch, the ds_bpermute_b32
among them, and .vgpr_count / .vgpr_spill_count / .sgpr_spill_count of its metadata; functions compared with labels
normalised.  Lists the three flagship kernels, every function that changed, and any register figure above the parent's
(how profiles/*_isa.txt are made)."""
import re
import subprocess
import sys

FLAG = ["kb_slabsort_kernel<1, false>", "kb_piecesort_pipe_kernel<1>", "kb_bucket_kernel<1, 0, 1, false, true, true>"]


def parse(path):
    text = open(path).read()
    names = sorted(set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M)))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = {m: re.sub(r"^void ", "", d).split("(")[0] for m, d in zip(names, dem)}
    fn = {}
    for m in names:
        a = text.find("\n%s:" % m)
        b = text.find(".Lfunc_end", a)
        if a < 0 or b < 0:
            continue
        body = []
        for ln in text[a:b].split("\n")[2:]:
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith(".") or ln.endswith(":"):
                continue
            body.append(re.sub(r"\.LBB\d+_\d+", "L", ln))
        op = [l.split()[0] for l in body]
        fn[short[m]] = dict(
            v=sum(o.startswith("v_") for o in op), s=sum(o.startswith("s_") for o in op), ds=sum(o.startswith("ds_") for o in op),
            mem=sum(o.startswith(("global_", "scratch_", "buffer_", "flat_")) for o in op), bperm=op.count("ds_bpermute_b32"),
            scratch=sum(o.startswith("scratch_") for o in op), body=body)
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size:", text, re.S):
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and m.group(1) in short and short[m.group(1)] in fn:
            g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
            fn[short[m.group(1)]].update(vg=g("vgpr_count"), vs=g("vgpr_spill_count"), ss=g("sgpr_spill_count"))
    return fn


def line(n, a, b):
    f = lambda x: "%d / %d / %d / %d  bpermute %d  regs %s / %s / %s" % (x["v"], x["s"], x["ds"], x["mem"], x["bperm"], x.get("vg"), x.get("vs"), x.get("ss"))
    return "%-52s %s  ->  %s" % (n, f(a), f(b))


def main():
    pa, bu = parse(sys.argv[1]), parse(sys.argv[2])
    print("## the three kernels of the flagship step (bench.py, k = 31)")
    for n in FLAG:
        if n not in pa or n not in bu:                             # (a unit other than the core)
            continue
        print(line(n, pa[n], bu[n]) + ("   scratch instructions %d -> %d" % (pa[n]["scratch"], bu[n]["scratch"])))
    ch = [n for n in sorted(bu) if n in pa and pa[n]["body"] != bu[n]["body"]]
    print("\n## every function whose instructions changed: %d of %d" % (len(ch), len(bu)))
    for n in ch:
        print(line(n, pa[n], bu[n]))
    print("\n## only in one of the two:", sorted(set(pa) ^ set(bu)) or "none")
    up = [n for n in sorted(bu) if n in pa and "vg" in bu[n] and (bu[n]["vg"] > pa[n]["vg"] or bu[n]["vs"] > pa[n]["vs"] or bu[n]["ss"] > pa[n]["ss"])]
    print("\n# .vgpr_count, .vgpr_spill_count or .sgpr_spill_count above the parent's:", "none" if not up else "")
    for n in up:
        print(line(n, pa[n], bu[n]))


if __name__ == "__main__":
    main()
