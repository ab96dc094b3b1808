"""The entry points of include/kdf.h "regions of informative reads" are declared in the header, bound in ``_native.py``
with the header's arguments and exported by the library when it is built (no compute calls: runs without a GPU)."""
import os
import re
from ctypes import POINTER, c_int, c_int64, c_uint32, c_uint64, c_void_p

from conftest import ROOT

NEW = ("kdf_cluster_intervals_dev", "kdf_cluster_intervals", "kdf_group_distinct_dev", "kdf_group_distinct")
CTYPE = {"uint64_t": c_uint64, "int64_t": c_int64, "uint32_t": c_uint32, "int": c_int}


def _declared():
    """{name: [ctypes type of every argument]}: the out count ``n_out`` is POINTER(c_uint64), every other pointer c_void_p"""
    hdr = open(os.path.join(ROOT, "include", "kdf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(kdf_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S):
        if name not in NEW:
            continue
        types = []
        for a in (x.strip() for x in args.split(",")):
            if "*" in a:
                types.append(POINTER(c_uint64) if re.search(r"\*\s*n_out$", a) else c_void_p)
            else:
                types.append(CTYPE[a.replace("const ", "").split()[0]])
        out[name] = types
    return out


def test_new_symbols_declared_and_bound():
    from kmer_denovo_filter_amd import _native
    declared = _declared()
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    for name in NEW:
        assert name in declared, f"{name} is not declared in kdf.h"
        assert name in bound, f"{name} is not bound in _native.SYMBOLS"
        assert bound[name][0] is c_int
        assert list(bound[name][1]) == declared[name], f"{name}: the bound argument types differ from the header's"
    assert [len(declared[n]) for n in NEW] == [10, 10, 7, 7]
    # the host and device forms take the same arguments in the same order
    assert declared[NEW[0]] == declared[NEW[1]] and declared[NEW[2]] == declared[NEW[3]]
    assert declared[NEW[0]][4:6] == [c_int64, c_int64] and declared[NEW[2]][3:6] == [c_int, c_uint64, c_int64]


def test_exported_by_the_built_library():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()                                 # (builds the library when the tree has none)
    for name in NEW:
        assert getattr(lib, name) is not None


def test_python_face():
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd import engine as E
    for m in ("cluster_intervals", "cluster_intervals_dev", "group_distinct", "group_distinct_dev"):
        assert callable(getattr(KmerEngine, m)) and getattr(KmerEngine, m).__doc__
    assert E.REGION_COLUMNS == ("chrom", "start", "end", "members")
    from kmer_denovo_filter_amd.discovery import regions as R
    assert callable(R._cluster_read_hits_device)
    assert R._n_kmers({"a", "b"}) == 2 and R._n_kmers(7) == 7 and R._n_kmers(()) == 0
