"""The table of ``tests/test_gpu_stream_order.py`` covers the header, and the harness's decoy builders build what they
promise (CPU only: nothing here touches a GPU or the native library).

A device entry point added to ``include/kdf.h`` fails ``test_every_device_entry_point_has_a_contract_case`` until it has a
case in ``CASES`` or an entry with a reason in ``EXCLUDED``."""
import os
import re

import numpy as np
import pytest

import spool_model as SM
import stream_order as SO
import test_gpu_stream_order as T
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "kdf.h")
UPLOADED = {"kdf_count_uploaded", "kdf_prefilter_add_uploaded", "kdf_sketch_add_uploaded"}


def declarations():
    """{name: parameter text} of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(kdf_\w+)\s*\(([^;{]*?)\)\s*;", text)}


def device_entry_points():
    """every kdf_*_dev, the three calls on an upload slot, and the kdf_spool_* calls that take a stream or an engine"""
    decl = declarations()
    names = {n for n in decl if n.endswith("_dev")} | (UPLOADED & decl.keys())
    names |= {n for n, args in decl.items() if n.startswith("kdf_spool_") and ("hip_stream" in args or "kdf_engine" in args)}
    return names, decl


def test_the_parser_sees_the_header():
    names, decl = device_entry_points()
    assert len(decl) > 120 and UPLOADED <= names
    for n in ("kdf_count_reads_dev", "kdf_export_join_w_dev", "kdf_variant_windows_dev", "kdf_spool_append_dev", "kdf_spool_replay",
              "kdf_spool_sketch", "kdf_spool_read_hits", "kdf_spool_append_uploaded_reads", "kdf_bamdev_decode_dev", "kdf_fasta_pack_dev"):
        assert n in names, n
    for n in ("kdf_spool_create", "kdf_spool_append", "kdf_spool_read_segment", "kdf_count_reads", "kdf_stream_words"):
        assert n not in names, n


def test_every_device_entry_point_has_a_contract_case():
    names, decl = device_entry_points()
    covered = {n for c in T.CASES for n in c.entry_points}
    assert not covered - decl.keys(), f"cases name functions the header does not declare: {sorted(covered - decl.keys())}"
    assert not T.EXCLUDED.keys() - names, f"excluded names that are no device entry points: {sorted(T.EXCLUDED.keys() - names)}"
    assert not covered & T.EXCLUDED.keys(), f"both covered and excluded: {sorted(covered & T.EXCLUDED.keys())}"
    missing = names - covered - T.EXCLUDED.keys()
    assert not missing, f"device entry points without a stream-order case or an exclusion: {sorted(missing)}"
    assert all(isinstance(r, str) and len(r) > 20 for r in T.EXCLUDED.values())
    assert len(T.EXCLUDED) <= 8, "the exclusion list is meant to stay short"


def test_the_table_is_well_formed():
    seen = set()
    for c in T.CASES:
        assert c.cls in (SO.NO_SYNC, SO.SYNCS) and c.ks and c.entry_points and callable(c.fn), c.name
        assert set(c.ks) <= set(T.KS), c.name
        assert c.name not in seen, c.name
        seen.add(c.name)
    for name, cls in T.CLASS.items():
        assert any(name in c.entry_points and c.cls == cls for c in T.CASES), name
    # every key width somewhere for the entry points that take keys or streams
    for name in ("kdf_count_reads_dev", "kdf_scan_reads_dev", "kdf_window_counts_dev", "kdf_hit_keys_dev", "kdf_sketch_add_reads_dev",
                 "kdf_prefilter_add_reads_dev", "kdf_count_reads_filtered_dev", "kdf_format_kmers_dev", "kdf_count_uploaded"):
        ks = {k for c in T.CASES if name in c.entry_points for k in c.ks}
        assert ks == set(T.KS), (name, ks)


# ------------------------------------------------------------------------------------------------ decoy builders

@pytest.fixture(scope="module")
def small_world():
    return SO.World(seed=3, n_reads=120)


def test_decoy_stream_has_the_words_and_the_layout_of_the_true_one(small_world):
    w = small_world
    pw, mw = SM.stream_words(w.n_bases)
    for packed, invalid, reads, offs in ((w.packed, w.invalid, w.reads, w.offsets), (w.d_packed, w.d_invalid, w.decoy_reads, w.d_offsets)):
        assert packed.dtype == invalid.dtype == np.uint64 and (len(packed), len(invalid)) == (pw, mw)
        codes, inv = SM.unpack(packed, invalid, w.n_bases)
        assert len(offs) == len(reads) + 1 and offs[0] == 0 and offs[-1] == w.n_bases
        for r, a in zip(reads, offs[:-1].tolist()):
            assert inv[a + len(r)]                                            # the separator
            assert "".join("ACGT"[c] if not i else "N" for c, i in zip(codes[a:a + len(r)], inv[a:a + len(r)])) == r
        # the padding: mask bits past n_bases set, packed bits there clear
        assert all(int(invalid[j]) == (1 << 64) - 1 for j in range(-(-w.n_bases // 64), mw))
        assert not packed[-(-w.n_bases // 32):].any()
    assert len(w.reads) == len(w.decoy_reads) and sorted(map(len, w.reads)) == sorted(map(len, w.decoy_reads))
    assert not np.array_equal(w.packed, w.d_packed) and not np.array_equal(w.offsets, w.d_offsets)
    assert np.all(np.diff(w.d_offsets) >= 1)


def test_decoy_offsets_do_not_decrease_and_end_at_the_same_total():
    rng = np.random.default_rng(1)
    for offs in ([0, 5, 5, 9, 40], [0, 100], [0], [7, 7, 7, 7], np.cumsum(np.r_[0, rng.integers(0, 50, 1000)])):
        offs = np.asarray(offs, np.int64)
        d = SO.decoy_offsets(offs, rng)
        assert d.dtype == np.int64 and d.shape == offs.shape and np.all(np.diff(d) >= 0)
        if len(offs):
            assert d[0] == offs[0] and d[-1] == offs[-1]
        if len(offs) > 100:
            assert not np.array_equal(d, offs)


def test_decoy_indices_are_in_range():
    rng = np.random.default_rng(2)
    for bound in (1, 2, 97, 1 << 40):
        for dtype in (np.uint64, np.uint32, np.int64):
            if bound > np.iinfo(dtype).max:
                continue
            d = SO.decoy_indices(1000, bound, rng, dtype)
            assert d.dtype == dtype and len(d) == 1000 and int(d.min()) >= 0 and int(d.max()) < bound
    assert not SO.decoy_indices(50, 0, rng).any()


def test_decoy_like_draws_rows_of_the_pool():
    rng = np.random.default_rng(4)
    pool = rng.integers(0, 1 << 62, (37, 3)).astype(np.uint64)
    true = np.zeros((500, 3), np.uint64)
    d = SO.decoy_like(true, pool, rng)
    assert d.shape == true.shape and d.dtype == true.dtype
    assert {tuple(r) for r in d.tolist()} <= {tuple(r) for r in pool.tolist()}
    with pytest.raises(AssertionError):
        SO.decoy_like(true, pool.astype(np.int64), rng)


def test_the_spool_batches_have_decoys_of_the_same_size():
    B = T.batches()
    assert len(B.true) == T.N_BATCHES
    for (p, m, n, offs), (dp, dm, dn, doffs) in zip(B.true, B.decoy):
        assert n == dn and (len(p), len(m)) == (len(dp), len(dm)) == SM.stream_words(n)
        assert len(offs) == len(doffs) and offs[-1] == doffs[-1] == n and np.all(np.diff(doffs) >= 1)
    assert sum(b[2] for b in B.true) == T.world().n_bases


def test_the_harness_refuses_a_decoy_of_another_shape():
    with pytest.raises(AssertionError):
        SO.StreamOrder._check_pairs({"x": (np.zeros(4, np.uint64), np.zeros(5, np.uint64))})
    with pytest.raises(AssertionError):
        SO.StreamOrder._check_pairs({"x": (np.zeros(4, np.uint64), np.zeros(4, np.int64))})
    SO.StreamOrder._check_pairs({"x": (np.zeros(4, np.uint64), np.ones(4, np.uint64))})
