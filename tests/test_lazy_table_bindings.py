"""The names the dump-only flush adds to the C ABI's option / stat tables are spelled the same in the engine source, the
header and the Python wrapper's documentation (no GPU: the sources are read)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION = "lazy_table"
STATS = ["lazy_table", "dump_only_flushes", "materialisations", "retained_passes"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_the_engine_knows_the_option_and_the_stats():
    src = _read("kmer_denovo_filter_amd", "csrc", "kdf_engine.hip")
    set_option = src[src.index("int kdf_set_option("):src.index("int kdf_get_stat(")]
    get_stat = src[src.index("int kdf_get_stat("):]
    assert f'n == "{OPTION}"' in set_option
    for name in STATS:
        assert f'n == "{name}"' in get_stat, name
    # (the option's default is read where struct kdf_engine is declared: the header the engine's units share)
    assert 'getenv("KDF_LAZY_TABLE")' in src + _read("kmer_denovo_filter_amd", "csrc", "kdf_engine_priv.h")


def test_the_header_documents_them():
    hdr = _read("include", "kdf.h")
    for name in [OPTION] + STATS:
        assert re.search(r'"%s"' % name, hdr), name
    assert "KDF_LAZY_TABLE" in hdr


def test_the_bindings_take_any_name():
    """kdf_set_option / kdf_get_stat are bound with the name as a C string: nothing to register for a new option or stat"""
    from ctypes import POINTER, c_char_p, c_int64
    from kmer_denovo_filter_amd import _native
    sig = {name: args for name, _, args in _native.SYMBOLS}
    assert sig["kdf_set_option"][1:] == [c_char_p, c_int64]
    assert sig["kdf_get_stat"][1:] == [c_char_p, POINTER(c_int64)]
