"""The sieve export / merge entry points (include/kdf.h "two-pass counting": several ranks) are declared in the header,
exported by the library and bound in ``_native.py`` with the header's number of arguments (no compute calls: runs
without a GPU)."""
import os
import re

from conftest import ROOT

NEW = ("kdf_prefilter_words", "kdf_prefilter_export_dev", "kdf_prefilter_export", "kdf_prefilter_merge_dev", "kdf_prefilter_merge")


def _declared_arity():
    hdr = open(os.path.join(ROOT, "include", "kdf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(kdf_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_new_symbols_declared_bound_and_exported():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()
    declared = _declared_arity()
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    for name in NEW:
        assert name in declared, f"{name} is not declared in kdf.h"
        assert name in bound, f"{name} is not bound in _native.SYMBOLS"
        assert len(bound[name][1]) == declared[name], f"{name}: {len(bound[name][1])} bound arguments, the header declares {declared[name]}"
        assert getattr(lib, name) is not None
    assert [declared[n] for n in NEW] == [2, 4, 4, 6, 6]


def test_python_face():
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.distributed import EngineOps, OwnerPartitionedCount, TableOps
    for m in ("prefilter_words", "prefilter_export", "prefilter_export_dev", "prefilter_merge", "prefilter_merge_dev"):
        assert callable(getattr(KmerEngine, m))
    for m in ("prefilter_begin", "prefilter_tally_stream", "prefilter_words", "prefilter_export", "prefilter_merge", "prefilter_arm", "prefilter_drop"):
        assert callable(getattr(TableOps, m)) and getattr(EngineOps, m) is not getattr(TableOps, m)
    for m in ("prefilter_begin", "tally_local", "prefilter_merge"):
        assert callable(getattr(OwnerPartitionedCount, m))


def test_the_header_no_longer_calls_the_prefilter_single_gpu():
    hdr = open(os.path.join(ROOT, "include", "kdf.h")).read()
    assert "Single GPU only" not in hdr
