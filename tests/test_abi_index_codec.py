"""The entry points of include/kdf.h "index record codec" are declared in the header, bound in ``_native.py`` with the
header's types and exported by the built library; the record size is the closed form; the header bytes of an index come
from one helper (no device call: runs without a GPU).

The stream-order table (``tests/test_stream_order_table.py``) asks a case of every ``kdf_*_dev`` name of the header in an
existing test file, so the codec's entry points are ONE function each with a ``mem`` argument, and none of the new names
ends in ``_dev``.  Their stream-order contract is observed in ``tests/test_gpu_index_codec_stream_order.py``."""
import json
import os
import re
from ctypes import POINTER, c_int, c_uint64, c_void_p

import numpy as np
import pytest

from conftest import ROOT

NEW = ("kdf_index_record_bytes", "kdf_index_encode", "kdf_index_decode", "kdf_jf_positions", "kdf_jf_order")
CTYPE = {"uint64_t": c_uint64, "int": c_int}
WORDS = ("columns", "bad_record_out")                   # uint64_t * arguments in host memory: POINTER(c_uint64); every other pointer c_void_p


def _header():
    return open(os.path.join(ROOT, "include", "kdf.h")).read()


def _declared():
    """{name: (ctypes result, [ctypes type of every argument])}"""
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int|uint64_t)\s+(kdf_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S):
        if name not in NEW:
            continue
        types = []
        for a in (x.strip() for x in args.split(",")):
            if "*" in a:
                types.append(POINTER(c_uint64) if a.split("*")[-1].strip() in WORDS else c_void_p)
            else:
                types.append(CTYPE[a.replace("const ", "").split()[0]])
        out[name] = (CTYPE[res], types)
    return out


def test_new_symbols_declared_and_bound():
    from kmer_denovo_filter_amd import _native
    declared = _declared()
    bound = {name: (res, args) for name, res, args in _native.SYMBOLS}
    for name in NEW:
        assert name in declared, f"{name} is not declared in kdf.h"
        assert name in bound, f"{name} is not bound in _native.SYMBOLS"
        assert bound[name][0] is declared[name][0], f"{name}: the bound result type differs from the header's"
        assert list(bound[name][1]) == declared[name][1], f"{name}: the bound argument types differ from the header's"
    assert [len(declared[n][1]) for n in NEW] == [2, 11, 10, 9, 9]
    assert declared[NEW[0]][0] is c_uint64
    for name in NEW[1:]:                                 # (engine, mem, ...)
        assert declared[name][1][:2] == [c_void_p, c_int], name


def test_no_new_name_ends_in_dev_and_mem_is_a_pair_of_constants():
    from kmer_denovo_filter_amd import _native
    hdr = _header()
    assert re.search(r"#define\s+KDF_MEM_HOST\s+0\b", hdr) and re.search(r"#define\s+KDF_MEM_DEVICE\s+1\b", hdr)
    assert (_native.KDF_MEM_HOST, _native.KDF_MEM_DEVICE) == (0, 1)
    section = hdr[hdr.index("index record codec ----"):hdr.index("count profile of a stream ----")]
    names = set(re.findall(r"\b(kdf_(?:index|jf)_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", section, flags=re.S)))
    assert names == set(NEW)
    assert not [n for n in names if n.endswith("_dev")], "a _dev name needs a case in the stream-order table of an existing test file"
    assert not [n for n, _, _ in _native.SYMBOLS if n.startswith(("kdf_index_", "kdf_jf_")) and n.endswith("_dev")]


def test_exported_by_the_built_library():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()                                 # (builds the library when the tree has none)
    for name in NEW:
        assert getattr(lib, name) is not None
    listed = open(os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc", "libkdf.map")).read()
    for name in NEW:
        assert re.search(rf"\b{name}\b", listed), f"{name} is not named in libkdf.map"


@pytest.mark.parametrize("k", [1, 4, 5, 31, 32, 33, 47, 63, 65, 101, 201])
def test_record_bytes(k):
    from kmer_denovo_filter_amd import KmerEngine
    for cb in range(1, 17):
        assert KmerEngine.index_record_bytes(k, cb) == -(-2 * k // 8) + cb, (k, cb)
    assert KmerEngine.index_record_bytes(k) == -(-2 * k // 8) + 4
    for cb in (0, 17, -1):
        assert KmerEngine.index_record_bytes(k, cb) == 0, (k, cb)


def test_record_bytes_refuses_other_k():
    from kmer_denovo_filter_amd import KmerEngine
    for k in (0, 64, 66, 202, -1, 100):
        for cb in (0, 4, 17):
            assert KmerEngine.index_record_bytes(k, cb) == 0, (k, cb)


def test_python_face():
    from kmer_denovo_filter_amd import KmerEngine, jf_io
    from kmer_denovo_filter_amd import engine as E
    for m in ("index_record_bytes", "index_encode", "index_encode_dev", "index_decode", "index_decode_dev", "jf_positions", "jf_positions_dev",
              "jf_order_dev"):
        assert callable(getattr(KmerEngine, m)) and getattr(KmerEngine, m).__doc__, m
    assert issubclass(E.IndexRecordError, ValueError) and E.IndexRecordError("x", 7).record == 7
    for f in ("write_index_device", "write_jellyfish_index_device", "load_index_into_device", "read_index_device", "device_index"):
        assert callable(getattr(jf_io, f)) and getattr(jf_io, f).__doc__, f
    assert jf_io.LAST_INDEX_CODEC in (None, "host", "device")


def test_the_switch_is_off_by_default(monkeypatch):
    from kmer_denovo_filter_amd import jf_io
    monkeypatch.delenv("KDF_DEVICE_INDEX", raising=False)
    assert jf_io.device_index() is False
    monkeypatch.setenv("KDF_DEVICE_INDEX", "0")
    assert jf_io.device_index() is False
    monkeypatch.setenv("KDF_DEVICE_INDEX", "1")
    assert jf_io.device_index() is True
    monkeypatch.setenv("KDF_INDEX_CHUNK_MB", "3")
    assert jf_io._window_bytes() == 3 << 20 and jf_io._window_bytes() % 16 == 0
    monkeypatch.delenv("KDF_INDEX_CHUNK_MB")
    assert jf_io._window_bytes() == 64 << 20


@pytest.mark.parametrize("k, n, cmdline", [(31, 0, None), (31, 7, ["count", "-m", "31"]), (47, 100_003, ["x"]), (101, 12, None)])
def test_shared_header_helper_reproduces_write_index(tmp_path, k, n, cmdline):
    """the bytes in front of the records of a file ``write_index`` wrote are ``_header_bytes(_kdf_header(...))``, and they
    are what the format says: 9 digits, the JSON, NUL padding to a multiple of 8"""
    from kmer_denovo_filter_amd import jf_io, keys
    rng = np.random.default_rng(k)
    W = keys.n_words(k)
    rows = np.sort(rng.integers(0, 1 << 62, (min(n, 50), W), dtype=np.uint64), axis=0) if n else np.zeros((0, W), np.uint64)
    rows[:, -1] &= np.uint64((1 << (2 * k - 64 * (W - 1))) - 1) if 2 * k - 64 * (W - 1) < 64 else np.uint64(2 ** 64 - 1)
    lo, hi = keys.to_pair(rows.T)
    m = len(rows)
    path = str(tmp_path / "x.jf")
    jf_io.write_index(path, k, lo, hi, np.arange(m, dtype=np.uint32), cmdline=cmdline)
    raw = open(path, "rb").read()
    head = jf_io._header_bytes(jf_io._kdf_header(k, m, cmdline))
    assert raw[:len(head)] == head and len(raw) == len(head) + m * (-(-2 * k // 8) + 4)
    assert len(head) % 8 == 0 and head[:9].isdigit() and int(head[:9]) == len(head) - 9
    hd = json.loads(head[9:].rstrip(b"\0"))
    assert hd == {"alignment": 8, "canonical": True, "cmdline": list(cmdline or []), "counter_len": 4, "format": "kdf/sorted",
                  "key_len": 2 * k, "size": m, "exe_path": "kmer_denovo_filter_amd (libkdf.so)"}
    assert jf_io.read_header(path) == (hd, len(head))


def test_jellyfish_header_helper_keeps_a_given_header():
    from kmer_denovo_filter_amd import jf_io
    fixture = os.path.join(ROOT, "tests", "golden", "giab", "mini_ref.fa.k31.jf")
    hd, off = jf_io.read_header(fixture)
    got, size, cols = jf_io._jellyfish_header(31, 45275, None, None, None, hd)
    assert got == hd and size == hd["size"] and cols == hd["matrix1"]["columns"]
    head = jf_io._header_bytes(got)                       # (Jellyfish spaces its JSON text differently: the fields are what is kept)
    assert len(head) % 8 == 0 and int(head[:9]) == len(head) - 9 and json.loads(head[9:].rstrip(b"\0")) == hd
    made, size, cols = jf_io._jellyfish_header(15, 300, None, None, ["c"], None)
    assert size == 1024 and len(cols) == 30 and made["matrix1"]["r"] == 10 and made["format"] == "binary/sorted"
    with pytest.raises(ValueError):
        jf_io._jellyfish_header(15, 300, 1000, None, None, None)
    with pytest.raises(ValueError):
        jf_io._jellyfish_header(31, 1, None, None, None, dict(hd, key_len=60))
