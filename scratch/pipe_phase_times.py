"""usage: scratch/pipe_phase_times.py K new|parent  -- phase tick sums of the pipelined piece sort (wave 0 of every workgroup) at bench size,
from a library built with -DKB_TIMING (KB_PT, kdf_binned.h); `parent`: a library whose stamps only split work from barrier waits
(how profiles/piece_phases_phase_counters.txt was made)"""
import sys, torch
sys.path.insert(0, '.')
from kmer_denovo_filter_amd import KmerEngine
from kmer_denovo_filter_amd.synth import synth_stream
k = int(sys.argv[1]); shape = sys.argv[2]
ds = synth_stream(10_000_000, 150, 100_000_000, seed=20260417, device="cuda:0"); torch.cuda.synchronize()
with KmerEngine(k, capacity_hint=1 << 28) as e:
    for it in range(2):
        e.clear(); e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases); e.flush(); e.synchronize()
    t0 = [e.get_stat(f"trash{8 + 20 + i}") for i in range(7)]
    e.clear(); e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases); e.flush(); e.synchronize()
    t1 = [e.get_stat(f"trash{8 + 20 + i}") for i in range(7)]
    d = [b - a for a, b in zip(t0, t1)]
    n = max(d[6], 1)
    if shape == "parent":
        names = ["work between barriers (all phases)", "wait at the 9 barriers"]; d = d[:2] + [0, 0, 0, 0] + d[6:]
    else:
        names = ["T0 rank+scatter, histogram, gather", "wait at B1", "T1 row, wave scans", "wait at B2", "T2 offs, run table, write-out, requests", "wait at B3"]
    tot = sum(d[:6])
    print(f"k={k} {shape}: pieces {n}, cycles per piece {tot / n:.0f} (s_memtime ticks, thread 0's wave, prologue iterations included)")
    for nm, v in zip(names, d[:6]):
        print(f"  {nm:44s} {v / n:9.0f} per piece  {100 * v / tot:5.1f} %")
    bar = d[1] if shape == "parent" else d[1] + d[3] + d[5]
    print(f"  barrier wait share {100 * bar / tot:.1f} %")
