"""KDF_DEVICE_REGIONS=1 on the GIAB mini trio: Module 3 with its clustering and its regions' k-mer counts made on the
device returns what the host path returns (region_kmers as numbers instead of sets), and the discovery BED written from
it is the reference's committed golden."""
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
    tmp = str(tmp_path_factory.mktemp("regions"))
    fa, _ = _extract_child_kmers_discovery(CHILD, None, 31, 3, 4, tmp)
    fa2, _ = _subtract_reference_kmers(os.path.join(GIAB, "mini_ref.fa.k31.jf"), fa, tmp)
    n3, fa3 = _filter_parents_discovery(os.path.join(GIAB, "HG004_mother.bam"), os.path.join(GIAB, "HG003_father.bam"),
                                        None, fa2, 31, 4, tmp, 0)
    assert n3 == 630
    return _build_proband_jf_index(fa3, 31, tmp, 630)


def anchor(proband_jf, merge_distance, min_dk):
    from kmer_denovo_filter_amd.discovery import regions as R
    return R._anchor_and_cluster(CHILD, None, None, 31, merge_distance=merge_distance, threads=4, min_distinct_kmers_per_read=min_dk,
                                 proband_jf=proband_jf, n_proband_unique=630)


def both_paths(proband_jf, monkeypatch, merge_distance, min_dk):
    """-> (the host path's tuple, the tuple under KDF_DEVICE_REGIONS=1), having seen both device calls run"""
    from kmer_denovo_filter_amd import KmerEngine
    for name in ("KDF_DEVICE_HITS", "KDF_DEVICE_COVERAGE", "KDF_DEVICE_REGIONS"):
        monkeypatch.delenv(name, raising=False)
    base = anchor(proband_jf, merge_distance, min_dk)
    used = []
    real_d, real_c = KmerEngine.group_distinct_dev, KmerEngine.cluster_intervals_dev
    monkeypatch.setattr(KmerEngine, "group_distinct_dev", lambda self, *a: used.append("distinct") or real_d(self, *a))
    monkeypatch.setattr(KmerEngine, "cluster_intervals_dev", lambda self, *a: used.append("cluster") or real_c(self, *a))
    monkeypatch.setenv("KDF_DEVICE_REGIONS", "1")
    dev = anchor(proband_jf, merge_distance, min_dk)
    assert sorted(used) == ["cluster", "distinct"], "the device path did not run"
    assert len(base) == len(dev) == 8
    regions, region_reads, total, region_kmers, unmapped, sv_meta, kcov, rcov = base
    assert dev[0] == regions and dev[1] == region_reads
    assert dev[2] == total and dev[4] == unmapped and dev[5] == sv_meta
    assert dev[6] == kcov and dev[7] == rcov
    assert set(dev[3]) == set(regions) == set(region_kmers)
    for key in regions:
        assert isinstance(dev[3][key], int) and dev[3][key] == len(region_kmers[key]), key
    return base, dev


def test_device_regions_equal_the_host_path_and_the_golden_bed(proband_jf, tmp_path, monkeypatch):
    from kmer_denovo_filter_amd.discovery import regions as R
    base, dev = both_paths(proband_jf, monkeypatch, 500, 7)
    regions, region_reads, region_kmers, sv_meta = dev[0], dev[1], dev[3], dev[5]
    assert len(regions) == 21
    ann, links = R._annotate_and_link_from_metadata(regions, region_reads, sv_meta)
    R._classify_regions(regions, ann, links)
    out = str(tmp_path / "discovery.bed")
    R._write_bed(regions, region_reads, region_kmers, out, region_annotations=ann,
                 filters={"min_distinct_kmers_per_read": 7, "min_supporting_reads": 1, "min_distinct_kmers": 1})
    gold = os.path.join(GOLDEN, "example_output_discovery", "giab_discovery.bed")
    assert open(out).read() == open(gold).read()
    # the region filter takes the numbers as it takes the sets
    kept_host = R._filter_regions(list(base[0]), dict(base[1]), dict(base[3]), 3, 18)
    kept_dev = R._filter_regions(list(regions), dict(region_reads), dict(region_kmers), 3, 18)
    assert kept_host == kept_dev and len(kept_dev) == 13             # (the golden BED's rows with reads >= 3 and unique_kmers >= 18)


def test_another_clustering(proband_jf, monkeypatch):
    """merge_distance 0 and every read with a hit kept: more reads, more regions"""
    base, dev = both_paths(proband_jf, monkeypatch, 0, 1)
    assert len(dev[0]) > 21
