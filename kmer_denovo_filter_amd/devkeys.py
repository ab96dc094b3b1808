"""Key sets that stay in HBM between the discovery stages.

The reference hands k-mer sets from stage to stage as FASTA files
(``child_candidates.fa`` -> ``child_non_ref_kmers.fa`` -> ``after_mother.fa`` ->
``proband_unique.fa``; discovery/pipeline.py:207-226,286-304,515-532).  The
mirror keeps that contract -- every file is still written, in the reference's
``>{i}\\n{KMER}\\n`` form -- but a stage that finds the set of its input path in
this registry takes the keys from device memory (``kdf_load_filter_dev`` /
``kdf_query_dev``) instead of parsing the text back and copying it up again.
torch is the holder of the device arrays here, nothing more.

Long k-mers (odd k from 65 to 201): one (n, W) int64 tensor of key rows in place of
(lo, hi), hi = None -- the form a long KmerEngine takes in the lo position.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np

from . import keys

_registry: Dict[str, Tuple[object, Optional[object], int, Tuple[int, int]]] = {}


def _key(path: str) -> str:
    return os.path.abspath(path)


def _stamp(path: str):
    st = os.stat(path)
    return (st.st_size, st.st_mtime_ns)


def register(path: str, lo, hi, k: int):
    """``lo`` / ``hi``: int64 CUDA tensors (bit patterns of the uint64 key words); hi None for k <= 32.
    Call right after the FASTA at ``path`` was written: its size and mtime are the set's identity."""
    _registry[_key(path)] = (lo, hi, int(k), _stamp(path))


def lookup(path: str, k: int):
    """(lo, hi) device tensors registered for ``path`` at this k, or None.  A file that was rewritten since
    (a resumed run, an edited FASTA, a second trio in the same tmpdir) no longer matches and is parsed instead."""
    ent = _registry.get(_key(path))
    if ent is None:
        return None
    try:
        same = ent[2] == int(k) and _stamp(path) == ent[3]
    except OSError:
        same = False
    if not same:
        _registry.pop(_key(path), None)
        return None
    return ent[0], ent[1]


def forget(path: str):
    _registry.pop(_key(path), None)


def to_host(lo, hi) -> Tuple[np.ndarray, np.ndarray]:
    """Device key tensors -> the (lo, hi) uint64 arrays the FASTA writer takes (long keys: ((n, W) rows, None))."""
    return keys.to_pair(keys.from_pair(*(None if t is None else t.cpu().numpy().view(np.uint64) for t in (lo, hi))))


def from_host(lo: np.ndarray, hi: Optional[np.ndarray], wide: bool, device: int = 0):
    """Host keys -> device key tensors (hi None unless ``wide``; long keys: ((n, W) rows, None))."""
    import torch
    dev = torch.device("cuda", device)
    pair = keys.to_pair(keys.from_pair(lo, hi if wide else None), zero_hi=False)
    return tuple(None if a is None else torch.from_numpy(a.view(np.int64)).to(dev) for a in pair)


def select(sets, idx=None):
    """One device key set from ``sets`` (a list of (lo, hi or None) sets, concatenated in order), masked or reordered
    by ``idx`` (a bool mask or an index tensor) when given; contiguous."""
    import torch
    out = []
    for parts in zip(*sets):
        if parts[0] is None:
            out.append(None)
            continue
        t = torch.cat(parts) if len(parts) > 1 else parts[0]
        out.append(t if idx is None else t[idx].contiguous())
    return tuple(out)


def dump_ge_counts(eng, min_count: int, device: int = 0):
    """``jellyfish dump -c -L min_count`` into device tensors, ascending key order, WITH the counts: -> (lo, hi or None,
    counts int32 holding the uint32 values) -- what the device index writers take (``jf_io.write_index_device``)."""
    import torch
    dev = torch.device("cuda", device)
    n = eng.count_ge(min_count)
    if getattr(eng, "long", False):                      # (n, W) rows, no hi
        lo = torch.empty((max(n, 1), eng.key_words), dtype=torch.int64, device=dev)
        hi = None
    else:
        lo = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        hi = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if eng.wide else None
    cnt = torch.empty(max(n, 1), dtype=torch.int32, device=dev)      # (the device sort carries the counts along)
    torch.cuda.current_stream(dev).synchronize()
    got = eng.export_ge_dev(min_count, lo.data_ptr(), hi.data_ptr() if hi is not None else None, cnt.data_ptr(), n,
                            sorted_=True) if n else 0
    if got != n:
        raise RuntimeError(f"dump -L {min_count}: {got} entries written, {n} counted")
    return lo[:n], (hi[:n] if hi is not None else None), cnt[:n]


def dump_ge(eng, min_count: int, device: int = 0):
    """``jellyfish dump -c -L min_count`` into device tensors, ascending key order (the reference does not rely on
    the order, but a sorted dump makes the contract FASTA files byte-reproducible from run to run)."""
    return dump_ge_counts(eng, min_count, device)[:2]


def dump_join(eng, other, min_count: int, max_count: Optional[int] = None, other_min: int = 0, other_max: Optional[int] = 0,
              device: int = 0):
    """The keys of ``eng`` with min_count <= count <= max_count whose count in ``other`` lies in other_min..other_max
    (``KmerEngine.count_join``; ``other=None``: ``dump -L min_count -U max_count``) into device tensors, ascending key
    order like ``dump_ge``.  One pass over ``eng``'s table that probes ``other``'s: nothing but the answer is written."""
    import torch
    dev = torch.device("cuda", device)
    n = eng.count_join(other, min_count, max_count, other_min, other_max)
    if getattr(eng, "long", False):                      # (n, W) rows, no hi
        lo = torch.empty((max(n, 1), eng.key_words), dtype=torch.int64, device=dev)
        hi = None
    else:
        lo = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        hi = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if eng.wide else None
    cnt = torch.empty(max(n, 1), dtype=torch.int32, device=dev)      # (the device sort carries the counts along)
    torch.cuda.current_stream(dev).synchronize()
    got = eng.export_join_dev(other, min_count, max_count, other_min, other_max, lo.data_ptr(),
                              hi.data_ptr() if hi is not None else None, cnt.data_ptr(), None, n, sorted_=True) if n else 0
    if got != n:
        raise RuntimeError(f"join dump: {got} entries written, {n} counted")
    return lo[:n], (hi[:n] if hi is not None else None)


def query(eng, lo, hi, device: int = 0):
    """``jellyfish query``: uint32 counts (as int64 values) of the keys, input order, on the device."""
    import torch
    dev = torch.device("cuda", device)
    n = lo.shape[0]                                      # (long keys: rows)
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    if n:
        torch.cuda.current_stream(dev).synchronize()
        eng.query_dev(lo.data_ptr(), hi.data_ptr() if hi is not None else None, n, out.data_ptr())
        eng.synchronize()
    return out.to(torch.int64) & 0xFFFFFFFF
