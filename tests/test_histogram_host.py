"""The count histogram and the table statistics of an index FILE (`jellyfish histo` / `jellyfish stats`), on the host:
jf_io.index_histogram / index_stats and the _jellyfish_histo / _jellyfish_stats mirrors against numpy.bincount of
the decoded records -- the reference's real Jellyfish file at k = 31, hand-made kdf/sorted indexes at k = 63 and
k = 101 -- and the text check that header and binding declare the engine's entry points (no GPU needed)."""
import os
import re

import numpy as np
import pytest

from conftest import GIAB, ROOT
from kmer_denovo_filter_amd import jf_io
from kmer_denovo_filter_amd.core import jellyfish_wrappers as jw

JF = os.path.join(GIAB, "mini_ref.fa.k31.jf")
# the real file, counted on the CPU: 45 275 records
JF_BINS_1_12 = [45050, 179, 7, 2, 3, 0, 0, 0, 2, 24, 2, 6]
JF_STATS = {"unique": 45050, "distinct": 45275, "total": 45804, "max_count": 12}
U32 = 0xFFFFFFFF


def bins_of(counts, high):
    """numpy.bincount with everything above `high` in bin high + 1."""
    c = np.minimum(np.asarray(counts, dtype=np.uint64), np.uint64(high + 1)).astype(np.int64)
    return np.bincount(c, minlength=high + 2).astype(np.uint64)


def stats_of(counts):
    c = np.asarray(counts, dtype=np.uint64)
    return {"unique": int((c == 1).sum()), "distinct": int((c >= 1).sum()), "total": int(c.sum(dtype=np.uint64)),
            "max_count": int(c.max()) if len(c) else 0}


def test_real_jellyfish_file_histogram():
    _, _, _, counts = jf_io.read_index(JF)
    assert len(counts) == 45275
    got = jf_io.index_histogram(JF)
    assert got.dtype == np.uint64 and got.shape == (10002,)
    assert np.array_equal(got, bins_of(counts, 10000))
    assert got[0] == 0 and [int(x) for x in got[1:13]] == JF_BINS_1_12 and int(got[13:].sum()) == 0
    assert int(got.sum()) == 45275


@pytest.mark.parametrize("high", [0, 1, 3, 11, 12, 13])
def test_real_jellyfish_file_overflow_bin(high):
    _, _, _, counts = jf_io.read_index(JF)
    got = jf_io.index_histogram(JF, high=high)
    assert got.shape == (high + 2,)
    assert np.array_equal(got, bins_of(counts, high))
    assert int(got[high + 1]) == sum(JF_BINS_1_12[high:])          # everything above `high`
    assert int(got.sum()) == 45275
    # small blocks: the bins add up over the blocks of iter_index
    assert np.array_equal(jf_io.index_histogram(JF, high=high, chunk_records=1000), got)


def test_real_jellyfish_file_stats():
    _, _, _, counts = jf_io.read_index(JF)
    assert jf_io.index_stats(JF) == JF_STATS == stats_of(counts)
    assert jf_io.index_stats(JF, chunk_records=777) == JF_STATS


@pytest.mark.parametrize("k", [63, 101])
def test_kdf_sorted_index_hand_made_counts(k, tmp_path):
    rng = np.random.default_rng(k)
    W = (2 * k + 63) // 64
    n = 5000
    vals = sorted({int.from_bytes(rng.bytes(W * 8), "little") >> (64 * W - 2 * k) for _ in range(n)})
    rows = np.array([[(v >> (64 * j)) & ((1 << 64) - 1) for j in range(W)] for v in vals], dtype=np.uint64)
    counts = rng.choice(np.array([0, 1, 1, 1, 1, 2, 3, 7, 10000, 10001, 1 << 20, U32 - 1, U32], dtype=np.uint64),
                        len(vals)).astype(np.uint32)
    counts[:4] = [0, U32, 1, U32]
    lo, hi = (rows, None) if k > 63 else (np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1]))
    path = jf_io.write_index(str(tmp_path / f"t{k}.jf"), k, lo, hi, counts)
    for high in (0, 1, 3, 10000, 10001, (1 << 20) - 1):
        got = jf_io.index_histogram(path, high=high, chunk_records=1024)
        assert np.array_equal(got, bins_of(counts, high)), high
        assert int(got.sum()) == len(vals) and int(got[0]) == int((counts == 0).sum())
    st = jf_io.index_stats(path, chunk_records=1024)
    assert st == stats_of(counts)
    assert st["max_count"] == U32 and st["total"] > U32           # summed as uint64, not wrapped
    assert jw._jellyfish_stats(path) == st
    rows_ = jw._jellyfish_histo(path, low=0, high=3)
    assert rows_ == [(c, int(x)) for c, x in enumerate(bins_of(counts, 3)) if x]


def test_empty_index(tmp_path):
    path = jf_io.write_index(str(tmp_path / "e.jf"), 31, np.zeros(0, np.uint64), None, np.zeros(0, np.uint32))
    assert not jf_io.index_histogram(path, high=5).any()
    assert jf_io.index_stats(path) == {"unique": 0, "distinct": 0, "total": 0, "max_count": 0}
    assert jw._jellyfish_histo(path) == []


def test_jellyfish_histo_lines(tmp_path):
    want = [(c + 1, n) for c, n in enumerate(JF_BINS_1_12) if n]
    assert jw._jellyfish_histo(JF) == want                         # zero bins (6, 7, 8) left out
    assert [c for c, _ in want] == [1, 2, 3, 4, 5, 9, 10, 11, 12]
    out = str(tmp_path / "histo.txt")
    got = jw._jellyfish_histo(JF, low=2, high=10, out_path=out)
    assert got == [(2, 179), (3, 7), (4, 2), (5, 3), (9, 2), (10, 24), (11, 2 + 6)]    # (high + 1, above high)
    assert open(out).read() == "".join(f"{c} {n}\n" for c, n in got)
    assert jw._jellyfish_histo(JF, low=1, high=1) == [(1, 45050), (2, 225)]
    with pytest.raises(ValueError):
        jw._jellyfish_histo(JF, low=5, high=4)
    with pytest.raises(RuntimeError, match="jellyfish histo failed"):
        jw._jellyfish_histo(str(tmp_path / "missing.jf"))


def test_jellyfish_stats_text(tmp_path):
    out = str(tmp_path / "stats.txt")
    st = jw._jellyfish_stats(JF, out_path=out)
    assert st == JF_STATS
    text = open(out).read()
    assert text == jw._format_jellyfish_stats(st)
    lines = text.splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["Unique", "Distinct", "Total", "Max_count"]
    assert [int(ln.split()[1]) for ln in lines] == [45050, 45275, 45804, 12]


def test_symbols_declared_in_header_and_binding():
    """Text only (no library load): header and ctypes binding move together."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kdf.h")).read(), flags=re.S)
    nat = open(os.path.join(ROOT, "kmer_denovo_filter_amd", "_native.py")).read()
    for name in ("kdf_histogram", "kdf_histogram_dev", "kdf_count_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert '("%s", c_int,' % name in nat, name
    assert re.search(r"kdf_histogram\s*\(\s*kdf_engine\s*\*\s*h\s*,\s*uint32_t\s+high\s*,\s*uint64_t\s*\*\s*bins_out\s*\)", hdr)
    assert re.search(r"kdf_count_stats\s*\(\s*kdf_engine\s*\*\s*h\s*,\s*uint64_t\s*\*\s*unique\s*,\s*uint64_t\s*\*\s*distinct\s*,"
                     r"\s*uint64_t\s*\*\s*total\s*,\s*uint64_t\s*\*\s*max_count\s*\)", hdr)
