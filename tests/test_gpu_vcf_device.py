"""VCF mode through the device path (kmer_denovo_filter_amd/vcf/device.py) on the GIAB mini trio: the reference's
committed metrics.json and summary.txt, the host path's informative reads, and at k = 75 -- which the host path refuses
-- the pure-Python chain."""
import collections
import json
import os

import numpy as np
import pytest

import kmer_truth as KT
from conftest import GIAB, GOLDEN

pytestmark = pytest.mark.gpu

CHILD, MOTHER, FATHER = (os.path.join(GIAB, n) for n in ("HG002_child.bam", "HG004_mother.bam", "HG003_father.bam"))


@pytest.fixture(scope="module")
def variants():
    from kmer_denovo_filter_amd.vcf.pipeline import _parse_vcf_variants
    return _parse_vcf_variants(os.path.join(GIAB, "candidates.vcf.gz"), proband_id="HG002")


@pytest.fixture(scope="module")
def device_k31(variants):
    from kmer_denovo_filter_amd.vcf.device import annotate_vcf_device
    return annotate_vcf_device(CHILD, MOTHER, FATHER, variants, 31, 20, 20)


def test_metrics_and_summary_goldens(variants, device_k31):
    metrics, ann, _inf = device_k31
    gold = os.path.join(GOLDEN, "example_output")
    m = json.load(open(os.path.join(gold, "metrics.json")))
    assert len(variants) == m["total_variants"] == 22
    assert metrics["total_child_kmers"] == m["total_child_kmers"] == 1484
    assert metrics["parent_found_kmers"] == m["parent_found_kmers"] == 1294
    assert metrics["child_unique_kmers"] == m["child_unique_kmers"] == 190
    assert metrics["variants_with_unique_reads"] == m["variants_with_unique_reads"] == 12
    rows = {}
    for line in open(os.path.join(gold, "summary.txt")):
        f = line.split()
        if len(f) == 14 and f[0].startswith("chr") and ">" in f[1]:
            chrom, pos = f[0].split(":")
            ref, alt = f[1].split(">")
            rows[f"{chrom}:{int(pos) - 1}:{ref}:{alt}"] = f[2:13]
    assert len(rows) == 22
    for key, g in rows.items():
        a = ann[key]
        got = [a["dku"], a["dkt"], a["dka"], a["dku_dkt"], a["dka_dkt"], a["max_pkc"], a["avg_pkc"], a["min_pkc"],
               a["max_pkc_alt"], a["avg_pkc_alt"], a["min_pkc_alt"]]
        exp = [int(g[0]), int(g[1]), int(g[2]), float(g[3]), float(g[4]), int(g[5]), float(g[6]), int(g[7]),
               int(g[8]), float(g[9]), int(g[10])]
        assert got == exp, (key, got, exp)
    assert ann["chr19:15018719:G:A"]["max_pkc"] == 2177 and ann["chr18:62805215:A:ATAATATACACTGCATAGGTTATACATATACAGTG"]["avg_pkc"] == 683.58


def test_informative_reads_equal_the_host_path(variants, device_k31, tmp_path):
    from kmer_denovo_filter_amd.vcf.pipeline import (_collect_child_kmers, annotate_variants, informative_reads_by_variant,
                                                     scan_parents)
    _metrics, ann, inf = device_k31
    fa = str(tmp_path / "child_kmers.fa")
    total, per_variant = _collect_child_kmers(CHILD, None, variants, 31, 20, 20, False, fa)
    found = scan_parents(MOTHER, FATHER, None, fa, 31, str(tmp_path), 4, total)
    want = informative_reads_by_variant(variants, per_variant, found)
    assert len(want) == 12 and inf == want
    assert ann == annotate_variants(variants, per_variant, found)


def python_chain(variants, k, min_baseq, min_mapq):
    """_collect_child_kmers' loop without its k <= 63 rule and without the FASTA: {variant key: [(name, k-mers, supports)]}"""
    from kmer_denovo_filter_amd.alignment import reads_from_batch
    from kmer_denovo_filter_amd.kmer_utils import _is_symbolic, extract_variant_spanning_kmers, read_supports_alt
    from kmer_denovo_filter_amd.reads import bam_reader
    from kmer_denovo_filter_amd.vcf.pipeline import _records_over_positions, _variant_key
    by_chrom = collections.defaultdict(list)
    for v in variants:
        by_chrom[v["chrom"]].append(v)
    per_variant = {_variant_key(v): [] for v in variants}
    vpos = {c: np.unique(np.asarray([v["pos"] for v in vs], dtype=np.int64)) for c, vs in by_chrom.items()}
    rd = bam_reader(CHILD, flag_off=0, collapse=False, max_bases=1 << 24, threads=4, want_aux=True)
    refs = rd.references()
    with rd:
        for batch in rd:
            n = batch.n_reads
            eligible = ((np.asarray(batch.flags[:n]) & (0x4 | 0x100 | 0x800 | 0x400)) == 0) & (np.asarray(batch.mapq[:n]) >= min_mapq)
            keep, _ = _records_over_positions(batch, refs, vpos, eligible)
            for read in reads_from_batch(batch, refs, keep.tolist()):
                for var in by_chrom[read.reference_name]:
                    if not (read.reference_start <= var["pos"] < read.reference_end):
                        continue
                    if var["alt"] is not None and _is_symbolic(var["alt"]):
                        continue
                    kmers = extract_variant_spanning_kmers(read, var["pos"], k, min_baseq, ref=var["ref"], alt=var["alt"])
                    if kmers:
                        sup = read_supports_alt(read, var["pos"], var["ref"], var["alt"], min_baseq=min_baseq)
                        per_variant[_variant_key(var)].append((read.query_name, kmers, sup))
    return per_variant


def test_k75_equals_the_pure_python_chain(variants):
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _stream_bam
    from kmer_denovo_filter_amd.vcf.device import annotate_vcf_device
    from kmer_denovo_filter_amd.vcf.pipeline import annotate_variants, informative_reads_by_variant
    k = 75
    metrics, ann, inf = annotate_vcf_device(CHILD, MOTHER, FATHER, variants, k, 20, 20)
    per_variant = python_chain(variants, k, 20, 20)
    kmers = sorted({x.upper() for recs in per_variant.values() for _n, ks, _s in recs for x in ks})
    assert len(kmers) > 500
    with KmerEngine(k, capacity_hint=len(kmers)) as e:
        rows = KT.rows([KT.key_int(x) for x in kmers], e.key_words)
        e.load_filter(rows)
        for bam in (MOTHER, FATHER):
            _stream_bam(e, bam, None, 4, filtered=True)
        counts = e.query(rows)
    found = {x: int(c) for x, c in zip(kmers, counts.tolist()) if c > 0}
    want = annotate_variants(variants, per_variant, found)
    assert ann == want
    assert any(a["dku"] for a in want.values()) and any(a["dka"] for a in want.values()) and any(a["max_pkc_alt"] for a in want.values())
    assert inf == informative_reads_by_variant(variants, per_variant, found)
    assert metrics["total_child_kmers"] == len(kmers) and metrics["parent_found_kmers"] == len(found)
