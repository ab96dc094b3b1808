"""kdf_fq_extract (include/kdf.h "FASTQ record extract") is declared in the header, exported by libkdf.so and bound in
``_native.SYMBOLS`` with the header's signature; the engine has its two methods; the argument errors that need no device
are refused.  No GPU."""
import ctypes
import inspect
import os
import re
from ctypes import byref, c_uint32, c_uint64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "kdf_fq_extract"


def _header():
    with open(os.path.join(ROOT, "include", "kdf.h")) as f:
        return f.read()


def test_declared_exported_and_bound():
    from kmer_denovo_filter_amd import _native
    hdr = _header()
    assert "FASTQ record extract" in hdr
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    lib = _native.load()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % NAME, hdr, re.S)
    assert m, f"{NAME} is not declared in include/kdf.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["kdf_engine *h", "int mem", "const void *text", "uint64_t n_bytes", "int final_chunk", "const void *keep", "uint64_t n_reads",
                      "void *out", "uint64_t cap_out", "void *out_offsets", "uint64_t *out_bytes", "uint64_t *n_kept", "uint64_t *consumed",
                      "uint64_t *bad_offset", "uint32_t *bad_rule"]
    assert NAME in bound, f"{NAME} is not bound in _native.SYMBOLS"
    res, args = bound[NAME]
    assert res is ctypes.c_int and len(args) == len(params)
    want = {"int": ctypes.c_int, "uint64_t": c_uint64}
    for p, a in zip(params, args):
        kind = p.rsplit(" ", 1)[0]
        if p.endswith(("*out_bytes", "*n_kept", "*consumed", "*bad_offset")):
            assert a._type_ is c_uint64, p
        elif p.endswith("*bad_rule"):
            assert a._type_ is c_uint32, p
        elif "*" in p:
            assert a is ctypes.c_void_p, p
        else:
            assert a is want[kind], p
    assert getattr(lib, NAME) is not None
    assert not any(n.startswith(NAME) and n != NAME for n in bound), "one entry point with a mem argument, no host / _dev pair"
    with open(os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc", "libkdf.map")) as f:
        assert re.search(r"\b%s\s*;" % NAME, f.read())
    # it shares the feeder's line index: the same translation unit, no new one
    with open(os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc", "kdf_fastqfeed.hip")) as f:
        assert re.search(r"\bint\s+%s\s*\(" % NAME, f.read())


def test_header_names_the_stats_and_the_bound():
    hdr = _header()
    sec = hdr[hdr.index("FASTQ record extract"):hdr.index("int %s" % NAME)]
    for word in ("fastqextract_us", "fastqextract_passes", "n_bytes + 2", "*consumed + 2", "KDF_MEM_HOST", "kdf_fastq_pack", "any byte alignment"):
        assert word in sec, word


def test_engine_methods():
    from kmer_denovo_filter_amd.engine import KmerEngine
    sig = inspect.signature(KmerEngine.fastq_extract_dev)
    assert list(sig.parameters) == ["self", "d_text", "n_bytes", "final_chunk", "d_keep", "n_reads", "d_out", "cap_out", "d_out_offsets"]
    assert sig.parameters["d_out_offsets"].default is None
    sig = inspect.signature(KmerEngine.fastq_extract)
    assert list(sig.parameters) == ["self", "text", "final_chunk", "keep", "want_offsets"] and sig.parameters["want_offsets"].default is False


def test_refusals_without_a_device():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()
    buf = (ctypes.c_uint8 * 64)()
    for mem in (_native.KDF_MEM_HOST, _native.KDF_MEM_DEVICE):
        ob, nk, used, bad, rule = c_uint64(7), c_uint64(7), c_uint64(7), c_uint64(7), c_uint32(7)
        rc = getattr(lib, NAME)(None, mem, buf, 8, 1, buf, 1, buf, 64, None, byref(ob), byref(nk), byref(used), byref(bad), byref(rule))
        assert rc == _native.KDF_ERR_INVALID
        assert NAME.encode() in lib.kdf_last_error(None)
        assert bad.value == 2 ** 64 - 1 and rule.value == 0
