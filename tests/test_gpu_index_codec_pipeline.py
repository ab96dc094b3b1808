"""The mirrors' chain on the GIAB mini trio under ``KDF_DEVICE_INDEX=1`` against the default path run in the same test:
every index file (the reference index, ``parent.jf``, ``proband_unique.jf``, a merged index) is byte-identical, the
stage counts, the k-mer sets and the Module 3 scan are equal, and the device codec is what read and wrote them.  With
``KDF_JF_FORMAT=jellyfish`` the reference counted on the GPU and written by the device writer has the records of the real
Jellyfish file committed under tests/golden."""
import os
import shutil

import numpy as np
import pytest

from conftest import GIAB

pytestmark = pytest.mark.gpu

CHILD = os.path.join(GIAB, "HG002_child.bam")
MOTHER = os.path.join(GIAB, "HG004_mother.bam")
FATHER = os.path.join(GIAB, "HG003_father.bam")
FIXTURE = os.path.join(GIAB, "mini_ref.fa.k31.jf")
MIN_CHILD = 3
INDEXES = ("mini_ref.jf", "parent.jf", "proband_unique.jf", "merged.jf")


def chain(k, tmp, monkeypatch):
    """reference index, Module 1, subtraction, a parent index written and queried, the parent filter, the proband index, Module 3
    and a merge -> {"indexes": bytes per file, "counts", "sets", "module3", "codecs"}"""
    from kmer_denovo_filter_amd import jf_io
    from kmer_denovo_filter_amd.core import bam_scanner
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _build_proband_jf_index, _ensure_ref_jf, _merge_jf_files
    from kmer_denovo_filter_amd.discovery import pipeline
    from kmer_denovo_filter_amd.kmer_fasta import read_kmer_fasta_keys
    out = {"indexes": {}, "codecs": [], "sets": {}}
    fa = os.path.join(tmp, "mini_ref.fa")
    shutil.copy(os.path.join(GIAB, "mini_ref.fa"), fa)              # nothing is written under tests/golden
    wrote, loader = [], jf_io.load_index_into

    def loading(*a, **kw):
        got = loader(*a, **kw)
        out["codecs"].append(("read", jf_io.LAST_INDEX_CODEC))
        return got

    def keep(path, name):
        with open(path, "rb") as f:
            out["indexes"][name] = f.read()
        wrote.append(jf_io.LAST_INDEX_CODEC)

    monkeypatch.setattr(jf_io, "load_index_into", loading)
    try:
        jf_io.LAST_INDEX_CODEC = None
        ref = _ensure_ref_jf(fa, k, 4, ref_jf=os.path.join(tmp, "mini_ref.jf"))
        keep(ref, "mini_ref.jf")
        fa1, n1 = pipeline._extract_child_kmers_discovery(CHILD, None, k, MIN_CHILD, 4, tmp)
        fa2, n2 = pipeline._subtract_reference_kmers(ref, fa1, tmp)                    # (loads the reference index)
        out["sets"]["non_ref"] = [a.tobytes() for a in read_kmer_fasta_keys(fa2, k) if a is not None]
        jf_io.LAST_INDEX_CODEC = None
        pjf = pipeline._count_parent_jellyfish(MOTHER, None, fa2, k, os.path.join(tmp, "mother"), 4, label="Mother")
        keep(pjf, "parent.jf")
        lo, hi = read_kmer_fasta_keys(fa2, k)
        out["sets"]["mother_counts"] = pipeline._query_index(pjf, lo, hi, k, "mother").tobytes()      # (loads parent.jf)
        n3, fa3 = pipeline._filter_parents_discovery(MOTHER, FATHER, None, fa2, k, 4, tmp, 0)
        out["sets"]["proband_unique"] = [a.tobytes() for a in read_kmer_fasta_keys(fa3, k) if a is not None]
        jf_io.LAST_INDEX_CODEC = None
        proband = _build_proband_jf_index(fa3, k, tmp, n3)
        keep(proband, "proband_unique.jf")
        bam_scanner._init_scan_worker(proband, k)                                        # (loads proband_unique.jf)
        out["module3"] = bam_scanner.scan_bam_module3(CHILD)
        a, b = os.path.join(tmp, "a.jf"), os.path.join(tmp, "b.jf")
        shutil.copy(ref, a); shutil.copy(proband, b)
        jf_io.LAST_INDEX_CODEC = None
        keep(_merge_jf_files([a, b], os.path.join(tmp, "merged.jf")), "merged.jf")
    finally:
        monkeypatch.setattr(jf_io, "load_index_into", loader)
    out["counts"] = (n1, n2, n3)
    out["wrote"] = wrote
    return out


def same_module3(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_module3(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_module3(a[x], b[x]) for x in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


@pytest.mark.parametrize("k", [31, 75])
def test_chain_through_the_device_index_codec(k, tmp_path, monkeypatch):
    run = str(tmp_path / "run")                          # (one directory for both runs: the headers record the paths)
    os.makedirs(run)
    monkeypatch.delenv("KDF_DEVICE_INDEX", raising=False)
    monkeypatch.delenv("KDF_JF_FORMAT", raising=False)
    default = chain(k, run, monkeypatch)
    assert set(default["indexes"]) == set(INDEXES)
    assert all(c == ("read", "host") for c in default["codecs"]) and len(default["codecs"]) >= 3
    assert "device" not in default["wrote"]
    if k == 31:
        assert default["counts"] == (51125, 6679, 630)
    shutil.rmtree(run)
    os.makedirs(run)
    monkeypatch.setenv("KDF_DEVICE_INDEX", "1")
    monkeypatch.setenv("KDF_INDEX_CHUNK_MB", "1")
    device = chain(k, run, monkeypatch)
    assert device["wrote"] == ["device"] * 4
    assert len(device["codecs"]) == len(default["codecs"]) and all(c == ("read", "device") for c in device["codecs"])
    assert device["counts"] == default["counts"] and device["sets"] == default["sets"]
    assert same_module3(device["module3"], default["module3"])
    for name in INDEXES:
        assert device["indexes"][name] == default["indexes"][name], name


def test_jellyfish_format_reference_is_the_golden_fixture(tmp_path, monkeypatch):
    """``mini_ref.fa`` counted on the GPU and written as ``binary/sorted`` by the device writer: the host writer's file, and
    under the fixture's own header the fixture's records byte for byte"""
    from kmer_denovo_filter_amd import devkeys, jf_io
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _count_fasta_to_index
    from kmer_denovo_filter_amd.engine import mirror_engine
    from kmer_denovo_filter_amd.reads import fasta_reader
    fa = str(tmp_path / "mini_ref.fa")
    shutil.copy(os.path.join(GIAB, "mini_ref.fa"), fa)
    monkeypatch.setenv("KDF_JF_FORMAT", "jellyfish")
    host, dev = str(tmp_path / "host.jf"), str(tmp_path / "dev.jf")
    monkeypatch.delenv("KDF_DEVICE_INDEX", raising=False)
    n = _count_fasta_to_index(fa, 31, host, 1 << 16, ["count"])
    assert jf_io.LAST_INDEX_CODEC == "host"
    monkeypatch.setenv("KDF_DEVICE_INDEX", "1")
    assert _count_fasta_to_index(fa, 31, dev, 1 << 16, ["count"]) == n == 45275
    assert jf_io.LAST_INDEX_CODEC == "device"
    assert open(dev, "rb").read() == open(host, "rb").read()
    assert jf_io.read_header(dev)[0]["format"] == "binary/sorted"
    # ... and with the header of the real Jellyfish file: its records, byte for byte
    header, off = jf_io.read_header(FIXTURE)
    with mirror_engine(31, capacity_hint=1 << 16) as eng:
        with fasta_reader(fa, 31) as rd:
            for batch in rd:
                eng.count(batch)
        dlo, dhi, dcnt = devkeys.dump_ge_counts(eng, 0, eng.device)
    out = str(tmp_path / "golden.jf")
    jf_io.write_jellyfish_index_device(out, 31, dlo, dhi, dcnt, header=header)
    h2, off2 = jf_io.read_header(out)
    assert h2 == header
    assert open(out, "rb").read()[off2:] == open(FIXTURE, "rb").read()[off:]
