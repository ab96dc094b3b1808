"""The VCF-mode entry points (include/kdf.h "VCF mode on the device") are declared in the header, exported by the
library and bound in ``_native.py`` with the header's arguments (no compute calls: runs without a GPU)."""
import os
import re
from ctypes import POINTER, c_int, c_int64, c_uint32, c_uint64, c_void_p

import pytest

from conftest import ROOT

NEW = ("kdf_variant_windows_dev", "kdf_variant_windows", "kdf_variant_evidence_dev", "kdf_variant_evidence")
CTYPE = {"uint64_t": c_uint64, "int64_t": c_int64, "uint32_t": c_uint32, "int": c_int}


def _declared():
    """{name: [ctypes type of every argument]}: a pointer that is an out count is POINTER(c_uint64), every other pointer c_void_p"""
    hdr = open(os.path.join(ROOT, "include", "kdf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(kdf_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S):
        if name not in NEW:
            continue
        types = []
        for a in (x.strip() for x in args.split(",")):
            if "*" in a:
                types.append(POINTER(c_uint64) if re.search(r"\*\s*n_\w+_out$", a) else c_void_p)
            else:
                types.append(CTYPE[a.replace("const ", "").split()[0]])
        out[name] = types
    return out


def test_new_symbols_declared_bound_and_exported():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()
    declared = _declared()
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    for name in NEW:
        assert name in declared, f"{name} is not declared in kdf.h"
        assert name in bound, f"{name} is not bound in _native.SYMBOLS"
        assert bound[name][0] is c_int
        assert list(bound[name][1]) == declared[name], f"{name}: the bound argument types differ from the header's"
        assert getattr(lib, name) is not None
    assert [len(declared[n]) for n in NEW] == [30, 30, 10, 10]
    # the host and device forms take the same arguments in the same order
    assert declared[NEW[0]] == declared[NEW[1]] and declared[NEW[2]] == declared[NEW[3]]


def test_python_face():
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.vcf import device
    for m in ("variant_windows", "variant_windows_dev", "variant_evidence", "variant_evidence_dev"):
        assert callable(getattr(KmerEngine, m)) and getattr(KmerEngine, m).__doc__
    assert callable(device.annotate_vcf_device) and "outside ACGT" in device.annotate_vcf_device.__doc__


def test_several_ranks_are_refused_before_any_device_call(monkeypatch):
    from kmer_denovo_filter_amd import dist_env
    from kmer_denovo_filter_amd.vcf import device as D
    monkeypatch.setattr(dist_env, "world_rank", lambda: (2, 0, False))
    with pytest.raises(ValueError, match="one process"):
        D.annotate_vcf_device("/nonexistent/child.bam", "/nonexistent/m.bam", "/nonexistent/f.bam", [], 75, 20, 20)


def test_the_host_path_keeps_its_rule():
    from kmer_denovo_filter_amd.vcf.pipeline import _require_vcf_k
    with pytest.raises(ValueError):
        _require_vcf_k(75)
