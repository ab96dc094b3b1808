"""KDF_DEVICE_COVERAGE=1 on the GIAB mini trio: Module 3 with its coverage sums kept on the device returns what the
host path returns, and the bedGraph / read-coverage BED written from it are the reference's committed goldens."""
import os

import pytest

from conftest import GIAB, GOLDEN

pytestmark = pytest.mark.gpu

CHILD = os.path.join(GIAB, "HG002_child.bam")


@pytest.fixture(scope="module")
def proband_jf(tmp_path_factory):
    """the discovery chain of tests/test_gpu_trio_golden.py up to the proband-unique index (630 k-mers)"""
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _build_proband_jf_index
    from kmer_denovo_filter_amd.discovery.pipeline import (
        _extract_child_kmers_discovery, _filter_parents_discovery, _subtract_reference_kmers)
    tmp = str(tmp_path_factory.mktemp("cov"))
    fa, _ = _extract_child_kmers_discovery(CHILD, None, 31, 3, 4, tmp)
    fa2, _ = _subtract_reference_kmers(os.path.join(GIAB, "mini_ref.fa.k31.jf"), fa, tmp)
    n3, fa3 = _filter_parents_discovery(os.path.join(GIAB, "HG004_mother.bam"), os.path.join(GIAB, "HG003_father.bam"),
                                        None, fa2, 31, 4, tmp, 0)
    assert n3 == 630
    return _build_proband_jf_index(fa3, 31, tmp, 630)


def anchor(proband_jf):
    from kmer_denovo_filter_amd.discovery import regions as R
    return R._anchor_and_cluster(CHILD, None, None, 31, merge_distance=500, threads=4, min_distinct_kmers_per_read=7,
                                 proband_jf=proband_jf, n_proband_unique=630)


def test_device_coverage_equals_the_host_path_and_the_goldens(proband_jf, tmp_path, monkeypatch):
    from kmer_denovo_filter_amd.core import bam_scanner
    from kmer_denovo_filter_amd.discovery import regions as R
    monkeypatch.delenv("KDF_DEVICE_HITS", raising=False)
    monkeypatch.delenv("KDF_DEVICE_COVERAGE", raising=False)
    base = anchor(proband_jf)
    used = []
    real = bam_scanner._DeviceCoverage.batch
    monkeypatch.setattr(bam_scanner._DeviceCoverage, "batch", lambda self, *a: used.append(1) or real(self, *a))
    monkeypatch.setenv("KDF_DEVICE_COVERAGE", "1")
    dev = anchor(proband_jf)
    assert used, "the device path did not run"
    assert len(base) == len(dev) == 8
    for i, (x, y) in enumerate(zip(base, dev)):
        assert x == y, f"element {i} of the tuple differs"
    kcov, rcov = dev[6], dev[7]
    assert sum(len(c) for c in rcov.values()) > 1000
    gold = os.path.join(GOLDEN, "example_output_discovery")
    out = {n: str(tmp_path / n) for n in ("bedgraph", "readcov")}
    R._write_bedgraph(kcov, out["bedgraph"], read_coverage=rcov, min_reads=3)
    R._write_read_coverage_bed(kcov, rcov, out["readcov"], min_reads=3)
    for ours, theirs in (("bedgraph", "giab_discovery.kmer_coverage.bedgraph"), ("readcov", "giab_discovery.read_coverage.bed")):
        assert open(out[ours]).read() == open(os.path.join(gold, theirs)).read(), theirs


def test_reference_lengths_equal_the_header():
    from kmer_denovo_filter_amd.reads import FLAG_OFF_MODULE3, bam_reader
    import gzip
    import struct
    raw = gzip.open(CHILD).read(1 << 22)                     # BGZF is a gzip stream: magic, l_text, text, n_ref, then (l_name, name, l_ref) each
    assert raw[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", raw, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    names, lens = [], []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", raw, p)[0]
        names.append(raw[p + 4:p + 4 + l_name - 1].decode())
        lens.append(struct.unpack_from("<i", raw, p + 4 + l_name)[0])
        p += 8 + l_name
    with bam_reader(CHILD, flag_off=FLAG_OFF_MODULE3, collapse=False) as rd:
        assert rd.references() == names and rd.reference_lengths() == lens
        assert len(lens) > 0 and all(x > 0 for x in lens)
        assert rd._lib.kdf_reader_ref_length(rd._h, len(lens)) == -1 and rd._lib.kdf_reader_ref_length(rd._h, -1) == -1
