"""The device FASTQ feeder's entry point (include/kdf.h "device FASTQ feeder") is declared in the header, exported by
libkdf.so and bound in ``_native.SYMBOLS``; the state's layout and the constants agree between the header, the bindings and
the test model; the argument errors that need no device are refused.  No GPU."""
import ctypes
import os
import re
from ctypes import byref, c_uint32, c_uint64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "kdf_fastq_pack"


def _header():
    with open(os.path.join(ROOT, "include", "kdf.h")) as f:
        return f.read()


def test_declared_exported_and_bound():
    from kmer_denovo_filter_amd import _native
    hdr = _header()
    assert "device FASTQ feeder" in hdr
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    lib = _native.load()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % NAME, hdr, re.S)
    assert m, f"{NAME} is not declared in include/kdf.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params[1] == "int mem" and len(params) == 17
    res, args = bound[NAME]
    assert res is ctypes.c_int and len(args) == 17
    assert args[1] is ctypes.c_int and args[5] is c_uint32 and args[16]._type_ is c_uint32
    assert getattr(lib, NAME) is not None
    assert not any(n.startswith("kdf_fastq") and n != NAME for n in bound), "one entry point with a mem argument, no host / _dev pair"
    with open(os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc", "libkdf.map")) as f:
        assert re.search(r"\b%s\s*;" % NAME, f.read())
    from kmer_denovo_filter_amd import build
    assert any(src == "kdf_fastqfeed.hip" for src, _ in build._SOURCES)


def test_state_layout_and_constants():
    from kmer_denovo_filter_amd import _native
    hdr = _header()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*kdf_fastq_state\s*;", hdr)
    assert m and [x.strip() for x in m.group(1).replace("uint64_t", "").strip(" ;").split(",")] == ["records", "positions", "bytes"]
    S = _native.FastqState
    assert ctypes.sizeof(S) == 24
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [("records", 0, 8), ("positions", 8, 8), ("bytes", 16, 8)]
    s = S()
    assert (s.records, s.positions, s.bytes) == (0, 0, 0)
    want = {"KDF_FQ_BAD_HEADER": 1, "KDF_FQ_BAD_PLUS": 2, "KDF_FQ_LENGTH": 3, "KDF_FQ_TRUNCATED": 4, "KDF_FASTQ_TILE_BYTES": 4096,
            "KDF_MEM_HOST": 0, "KDF_MEM_DEVICE": 1}
    for name, value in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, hdr)
        assert m and int(m.group(1)) == value, name
        assert getattr(_native, name) == value
    import fastq_stream_model as M
    assert (M.BAD_HEADER, M.BAD_PLUS, M.LENGTH, M.TRUNCATED, M.TILE) == (1, 2, 3, 4, 4096)
    assert issubclass(_native.FastqFormatError, _native.KdfError)
    e = _native.FastqFormatError(_native.KDF_ERR_IO, "x", 7, 3)
    assert (e.code, e.offset, e.rule) == (_native.KDF_ERR_IO, 7, 3)


def test_refusals_without_a_device():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()
    st = _native.FastqState(1, 2, 3)
    nb, nr, used, bad, rule = c_uint64(7), c_uint64(7), c_uint64(7), c_uint64(7), c_uint32(7)
    buf = (ctypes.c_uint64 * 16)()
    for mem in (_native.KDF_MEM_HOST, _native.KDF_MEM_DEVICE):
        rc = getattr(lib, NAME)(None, mem, None, 0, 1, 0, byref(st), buf, buf, 1, None, 0, byref(nb), byref(nr), byref(used), byref(bad), byref(rule))
        assert rc == _native.KDF_ERR_INVALID
        assert NAME.encode() in lib.kdf_last_error(None)
        assert (st.records, st.positions, st.bytes) == (1, 2, 3)
        assert bad.value == 2 ** 64 - 1 and rule.value == 0
