"""The discovery chain of the GIAB mini trio under ``KDF_DEVICE_FASTA=1`` against the default path run in the same test:
the four contract files (``child_candidates.fa``, ``child_non_ref_kmers.fa``, ``after_mother.fa``,
``proband_unique.fa``), their sidecars' keys and the stage counts (51 125 / 6 679 / 1 513 / 630 at k = 31) are equal, also
when the registry is cleared and the sidecars are removed between the stages, so that the device reader feeds each."""
import os
import shutil

import numpy as np
import pytest

from conftest import GIAB

pytestmark = pytest.mark.gpu

CHILD = os.path.join(GIAB, "HG002_child.bam")
MOTHER = os.path.join(GIAB, "HG004_mother.bam")
FATHER = os.path.join(GIAB, "HG003_father.bam")
MIN_CHILD = 3
FILES = ("child_candidates.fa", "child_non_ref_kmers.fa", "after_mother.fa", "proband_unique.fa")


@pytest.fixture(scope="module")
def ref_jf(tmp_path_factory):
    """k -> reference index of mini_ref.fa: the committed Jellyfish file at k = 31, one built on the way of
    tests/test_gpu_long_k_pipeline.py at k = 75"""
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _ensure_ref_jf
    made = {31: os.path.join(GIAB, "mini_ref.fa.k31.jf")}

    def get(k):
        if k not in made:
            tmp = str(tmp_path_factory.mktemp(f"ref{k}"))
            fa = os.path.join(tmp, "mini_ref.fa")
            shutil.copy(os.path.join(GIAB, "mini_ref.fa"), fa)       # nothing is written under tests/golden
            made[k] = _ensure_ref_jf(fa, k, 4)
        return made[k]
    return get


def _keep(path, out):
    """the file's bytes and its sidecar's keys, as the stage left them"""
    with open(path, "rb") as f:
        out["files"][os.path.basename(path)] = f.read()
    z = np.load(path + ".kdfkeys.npz")
    out["sidecars"][os.path.basename(path)] = (z["lo"].tobytes(), z["hi"].tobytes(), z["lo"].shape, int(z["k"]))


def chain(k, ref, tmp, monkeypatch, unregistered=False):
    """Module 1, the reference subtraction and the parent filter in turn -> {"counts", "files", "sidecars", "reads",
    "codecs"}; ``unregistered``: every stage finds neither its input's set in the registry nor a sidecar."""
    from kmer_denovo_filter_amd import devkeys, kmer_fasta
    from kmer_denovo_filter_amd.discovery import pipeline
    out = {"files": {}, "sidecars": {}, "reads": [], "codecs": []}
    remove, read_dev = pipeline.remove_with_sidecar, pipeline.read_kmer_fasta_keys_device

    def keeping(path):                                             # (a stage removes its input when it is done with it)
        if os.path.basename(path) not in out["files"]:
            _keep(path, out)
        remove(path)

    def reading(path, *a, **kw):
        got = read_dev(path, *a, **kw)
        out["reads"].append((os.path.basename(path), kmer_fasta.LAST_FASTA_CODEC))
        return got

    def hand_over(path):
        _keep(path, out)
        out["codecs"].append(kmer_fasta.LAST_FASTA_CODEC)          # (the codec that wrote it)
        if unregistered:
            devkeys.forget(path)
            os.remove(path + ".kdfkeys.npz")

    monkeypatch.setattr(pipeline, "remove_with_sidecar", keeping)
    monkeypatch.setattr(pipeline, "read_kmer_fasta_keys_device", reading)
    try:
        fa1, n1 = pipeline._extract_child_kmers_discovery(CHILD, None, k, MIN_CHILD, 4, tmp)
        hand_over(fa1)
        fa2, n2 = pipeline._subtract_reference_kmers(ref, fa1, tmp)
        hand_over(fa2)
        n3, fa3 = pipeline._filter_parents_discovery(MOTHER, FATHER, None, fa2, k, 4, tmp, 0)
        _keep(fa3, out)
        out["codecs"].append(kmer_fasta.LAST_FASTA_CODEC)
    finally:
        monkeypatch.setattr(pipeline, "remove_with_sidecar", remove)
        monkeypatch.setattr(pipeline, "read_kmer_fasta_keys_device", read_dev)
    assert [os.path.basename(p) for p in (fa1, fa2, fa3)] == [FILES[0], FILES[1], FILES[3]] and set(out["files"]) == set(FILES)
    out["counts"] = (n1, n2, out["files"]["after_mother.fa"].count(b">"), n3)
    return out


@pytest.mark.parametrize("k", [31, 75])
def test_chain_through_the_device_codec(k, tmp_path, ref_jf, monkeypatch):
    ref = ref_jf(k)
    dirs = {}
    for name in ("default", "device", "fed"):
        dirs[name] = str(tmp_path / name)
        os.makedirs(dirs[name])
    monkeypatch.delenv("KDF_DEVICE_FASTA", raising=False)
    default = chain(k, ref, dirs["default"], monkeypatch)
    assert default["codecs"] == ["host"] * 3 and default["reads"] == []
    if k == 31:
        assert default["counts"] == (51125, 6679, 1513, 630)
    assert default["counts"][0] > default["counts"][1] >= default["counts"][2] >= default["counts"][3] > 0

    monkeypatch.setenv("KDF_DEVICE_FASTA", "1")
    monkeypatch.setenv("KDF_FASTA_CHUNK_MB", "1")                   # (child_candidates.fa then takes two windows)
    device = chain(k, ref, dirs["device"], monkeypatch)
    assert device["codecs"] == ["device"] * 3 and device["reads"] == []     # (every set was still registered)
    # ... and with nothing handed on but the files: the device reader feeds the subtraction and the parent filter
    fed = chain(k, ref, dirs["fed"], monkeypatch, unregistered=True)
    assert fed["codecs"] == ["device"] * 3
    assert fed["reads"] == [(FILES[0], "device"), (FILES[1], "device")]
    for got in (device, fed):
        assert got["counts"] == default["counts"]
        for name in FILES:
            assert got["files"][name] == default["files"][name], name
            assert got["sidecars"][name] == default["sidecars"][name], name


def test_fused_stage_and_host_readers_through_the_device_codec(tmp_path, ref_jf, monkeypatch):
    """``_extract_child_non_ref_kmers`` writes its file with the device codec, and the readers that want host arrays
    (``_count_parent_jellyfish``'s filter) get the host reader's"""
    from kmer_denovo_filter_amd import devkeys, kmer_fasta
    from kmer_denovo_filter_amd.discovery import pipeline
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    os.makedirs(a); os.makedirs(b)
    monkeypatch.delenv("KDF_DEVICE_FASTA", raising=False)
    fa, n1, n2 = pipeline._extract_child_non_ref_kmers(CHILD, None, ref_jf(31), 31, MIN_CHILD, 4, a)
    assert (n1, n2) == (51125, 6679) and kmer_fasta.LAST_FASTA_CODEC == "host"
    want = open(fa, "rb").read()
    monkeypatch.setenv("KDF_DEVICE_FASTA", "1")
    fb, m1, m2 = pipeline._extract_child_non_ref_kmers(CHILD, None, ref_jf(31), 31, MIN_CHILD, 4, b)
    assert (m1, m2) == (n1, n2) and kmer_fasta.LAST_FASTA_CODEC == "device"
    assert open(fb, "rb").read() == want
    za, zb = np.load(fa + ".kdfkeys.npz"), np.load(fb + ".kdfkeys.npz")
    assert all(za[f].tobytes() == zb[f].tobytes() for f in ("lo", "hi", "k"))
    # the host-array readers: without a sidecar the text is parsed, on the device under the switch
    os.remove(fb + ".kdfkeys.npz")
    devkeys.forget(fb)
    got = kmer_fasta.load_kmer_set(fb, 31)
    assert kmer_fasta.LAST_FASTA_CODEC == "device"
    monkeypatch.delenv("KDF_DEVICE_FASTA")
    host = kmer_fasta.load_kmer_set(fb, 31)
    assert kmer_fasta.LAST_FASTA_CODEC == "host"
    assert all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(got, host))
