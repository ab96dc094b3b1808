"""The entry points of include/kdf.h "k-mer FASTA codec" are declared in the header, bound in ``_native.py`` with the
header's types and exported by the built library, and the closed form of the text's size equals the length of the text a
plain Python loop writes (no device call: runs without a GPU)."""
import os
import re
from ctypes import POINTER, c_int, c_uint64, c_void_p

import pytest

from conftest import ROOT

NEW = ("kdf_kmer_text_bytes", "kdf_format_kmers_dev", "kdf_format_kmers", "kdf_parse_kmer_fasta_dev", "kdf_parse_kmer_fasta")
CTYPE = {"uint64_t": c_uint64, "int": c_int}
OUT = ("n_out", "consumed_out", "bad_offset_out")          # uint64_t * results: POINTER(c_uint64); every other pointer c_void_p


def _declared():
    """{name: (ctypes result, [ctypes type of every argument])}"""
    hdr = open(os.path.join(ROOT, "include", "kdf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for res, name, args in re.findall(r"\b(int|uint64_t)\s+(kdf_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S):
        if name not in NEW:
            continue
        types = []
        for a in (x.strip() for x in args.split(",")):
            if "*" in a:
                types.append(POINTER(c_uint64) if a.split("*")[-1].strip() in OUT else c_void_p)
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
    assert [len(declared[n][1]) for n in NEW] == [4, 10, 10, 12, 12]
    assert declared[NEW[0]][0] is c_uint64
    # the host and device forms take the same arguments in the same order
    assert declared[NEW[1]][1] == declared[NEW[2]][1] and declared[NEW[3]][1] == declared[NEW[4]][1]
    hdr = open(os.path.join(ROOT, "include", "kdf.h")).read()
    assert re.search(r"#define\s+KDF_TEXT_FASTA\s+0\b", hdr) and re.search(r"#define\s+KDF_TEXT_ROWS\s+1\b", hdr)


def test_exported_by_the_built_library():
    from kmer_denovo_filter_amd import _native
    lib = _native.load()                                 # (builds the library when the tree has none)
    for name in NEW:
        assert getattr(lib, name) is not None


def test_python_face():
    from kmer_denovo_filter_amd import KmerEngine, kmer_fasta
    from kmer_denovo_filter_amd import engine as E
    for m in ("kmer_text_bytes", "format_kmers", "format_kmers_dev", "parse_kmer_fasta", "parse_kmer_fasta_dev"):
        assert callable(getattr(KmerEngine, m)) and getattr(KmerEngine, m).__doc__
    assert (E.TEXT_FASTA, E.TEXT_ROWS) == (0, 1)
    assert issubclass(E.KmerFastaError, ValueError)
    assert callable(kmer_fasta.write_kmer_fasta_device) and callable(kmer_fasta.read_kmer_fasta_keys_device)
    assert kmer_fasta.LAST_FASTA_CODEC is None or isinstance(kmer_fasta.LAST_FASTA_CODEC, str)


def _loop_bytes(k, first, n):
    kmer = "A" * k
    return sum(len(f">{i}\n{kmer}\n") for i in range(first, first + n))


# (first_index, n): the digit count changes inside the range -- 9 -> 10, 99 -> 100, 99 999 -> 100 000, 9 999 999 999 -> 10^10
# -- once, several times, at the first and at the last record, and not at all; n = 0
RANGES = [(0, 0), (7, 0), (0, 1), (0, 9), (0, 10), (0, 11), (9, 1), (9, 2), (10, 1), (5, 10), (95, 10), (99, 1), (99, 2), (0, 101),
          (0, 1234), (99_990, 20), (99_999, 1), (99_999, 2), (100_000, 3), (90, 100_000), (9_999_999_990, 25), (9_999_999_999, 1),
          (9_999_999_999, 2), (10_000_000_000, 5), (9_999_999_990, 0)]


@pytest.mark.parametrize("k", [1, 31, 33, 101])
def test_text_bytes_equals_the_python_loop(k):
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.engine import TEXT_FASTA, TEXT_ROWS
    for first, n in RANGES:
        assert KmerEngine.kmer_text_bytes(k, TEXT_FASTA, first, n) == _loop_bytes(k, first, n), (k, first, n)
        assert KmerEngine.kmer_text_bytes(k, TEXT_ROWS, first, n) == n * k, (k, first, n)


def test_text_bytes_closed_form_far_out():
    """Ranges no loop can walk: the sum over the digit classes, written out independently here."""
    from kmer_denovo_filter_amd import KmerEngine

    def classes(k, first, n):
        total, d = 0, 1
        while first + n > 0 and d <= 20:
            a, b = max(first, 0 if d == 1 else 10 ** (d - 1)), min(first + n, 10 ** d)
            total += max(b - a, 0) * (d + k + 3)
            d += 1
        return total

    for k in (1, 31, 63, 201):
        for first, n in ((0, 10 ** 12), (123_456_789, 10 ** 15 + 7), (10 ** 18 - 5, 10), (0, 2 ** 55)):
            assert KmerEngine.kmer_text_bytes(k, 0, first, n) == classes(k, first, n), (k, first, n)
        assert classes(k, 0, 1234) == _loop_bytes(k, 0, 1234)


def test_text_bytes_refusals():
    from kmer_denovo_filter_amd import KmerEngine
    tb = KmerEngine.kmer_text_bytes
    assert tb(31, 0, 0, 5) > 0 and tb(63, 0, 0, 5) > 0 and tb(65, 0, 0, 5) > 0 and tb(201, 0, 0, 5) > 0
    for k in (0, -1, 64, 66, 100, 200, 202, 203):                      # k = 64, even k > 63, beyond the range
        assert tb(k, 0, 0, 5) == 0 and tb(k, 1, 0, 5) == 0, k
    assert tb(31, 2, 0, 5) == 0 and tb(31, -1, 0, 5) == 0               # layout
    assert tb(31, 0, 2 ** 63 - 1, 1) == 19 + 31 + 3                     # the last index a call takes
    assert tb(31, 0, 2 ** 63 - 1, 2) == 0 and tb(31, 0, 2 ** 63, 1) == 0 and tb(31, 0, 2 ** 64 - 1, 1) == 0   # first_index + n > 2^63
    assert tb(31, 0, 0, 2 ** 62) == 0 and tb(201, 0, 0, 2 ** 56) == 0   # the size passes 2^63
    assert tb(31, 1, 0, 2 ** 59) == 0 and tb(31, 1, 0, 2 ** 58) == 31 * 2 ** 58
