"""The device FASTA feeder's entry points (include/kdf.h "device FASTA feeder") are declared in the header, exported by
libkdf.so and bound in ``_native.SYMBOLS``; the state's layout and the constants agree between the three; the argument
errors that need no device are refused.  No GPU."""
import ctypes
import os
import re
from ctypes import byref, c_uint64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kdf_fasta_pack_dev", "kdf_fasta_pack")


def _header():
    with open(os.path.join(ROOT, "include", "kdf.h")) as f:
        return f.read()


def test_declared_exported_and_bound():
    from kmer_denovo_filter_amd import _native
    hdr = _header()
    assert "device FASTA feeder" in hdr
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    lib = _native.load()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, f"{name} is not declared in include/kdf.h"
        assert name in bound, f"{name} is not bound in _native.SYMBOLS"
        res, args = bound[name]
        assert res is ctypes.c_int
        assert len(args) == len(m.group(1).split(",")) == 17
        assert getattr(lib, name) is not None
    with open(os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc", "libkdf.map")) as f:
        text = f.read()
    assert all(re.search(r"\b%s\s*;" % name, text) for name in NAMES)


def test_state_layout_and_constants():
    from kmer_denovo_filter_amd import _native
    hdr = _header()
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*kdf_fasta_state\s*;", hdr)
    assert m
    fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+)\s*;", m.group(1))
    assert fields == [("uint32_t", "flags"), ("uint32_t", "reserved"), ("uint64_t", "records"), ("uint64_t", "positions")]
    S = _native.FastaState
    assert ctypes.sizeof(S) == 24
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [("flags", 0, 4), ("reserved", 4, 4), ("records", 8, 8),
                                                                                     ("positions", 16, 8)]
    s = S()
    assert (s.flags, s.reserved, s.records, s.positions) == (0, 0, 0, 0)
    want = {"KDF_FA_IN_RECORD": 1, "KDF_FA_MID_LINE": 2, "KDF_FA_IN_HEADER": 4, "KDF_FASTA_TILE_BYTES": 4096}
    for name, value in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, hdr)
        assert m and int(m.group(1)) == value, name
        assert getattr(_native, name) == value
    import fasta_stream_model as M
    assert (M.IN_RECORD, M.MID_LINE, M.IN_HEADER) == (1, 2, 4)


def test_refusals_without_a_device():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()
    st = _native.FastaState()
    nb, nr, used = c_uint64(7), c_uint64(7), c_uint64(7)
    buf = (ctypes.c_uint64 * 16)()
    for name in NAMES:
        rc = getattr(lib, name)(None, None, 0, 1, byref(st), None, None, 0, 0, buf, buf, 1, None, 0, byref(nb), byref(nr), byref(used))
        assert rc == _native.KDF_ERR_INVALID
        assert name.encode() in lib.kdf_last_error(None)
        assert (st.flags, st.records, st.positions) == (0, 0, 0)
