"""The mini trio with its samples given as FASTQ: the reads of the golden GIAB BAMs, as ``bam_reader`` delivers them to the
counting legs (collapse on), written out as four-line FASTQ with their qualities, go through the discovery chain's
alignment-free steps -- the child count and both parent ``count --if`` passes -- and give the numbers and the key sets of
the BAM path; ``KDF_FASTQ_MIN_QUAL`` masks low qualities as N; the paths that need an alignment refuse a FASTQ child by
name; and without a FASTQ path the counting leg reports the feeder it always did."""
import os

import numpy as np
import pytest

import bamdev_cases as bc
from conftest import GIAB

pytestmark = pytest.mark.gpu

CHILD, MOTHER, FATHER = (os.path.join(GIAB, n) for n in ("HG002_child.bam", "HG004_mother.bam", "HG003_father.bam"))


def _reads_of(bam):
    """[(sequence over ACGTN, quality string)] of the BAM as the counting legs read it"""
    from kmer_denovo_filter_amd.reads import bam_reader
    out = []
    with bam_reader(bam, max_bases=1 << 24, max_reads=1 << 18, want_aux=True) as rd:
        for b in rd:
            seqs = bc.stream_reads(b)
            for i, s in enumerate(seqs):
                q = b.qualities(i)
                q = bytes((np.asarray(q, np.uint8) + 33).tolist()) if q is not None else b"I" * len(s)
                assert len(q) == len(s)
                out.append((s.encode(), q))
    return out


def _write_fastq(path, reads):
    with open(path, "wb") as f:
        for i, (s, q) in enumerate(reads):
            f.write(b"@read%d\n%s\n+\n%s\n" % (i, s, q))
    return path


@pytest.fixture(scope="module")
def trio(tmp_path_factory):
    d = tmp_path_factory.mktemp("trio_fastq")
    reads = {n: _reads_of(p) for n, p in (("child", CHILD), ("mother", MOTHER), ("father", FATHER))}
    paths = {n: _write_fastq(str(d / (n + ".fastq")), r) for n, r in reads.items()}
    return paths, reads, d


def _chain(tmp, child, mother, father):
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_kmers_discovery, _filter_parents_discovery, _subtract_reference_kmers
    from kmer_denovo_filter_amd.kmer_fasta import read_kmer_fasta_keys
    os.makedirs(tmp)
    fa, n = _extract_child_kmers_discovery(child, None, 31, 3, 4, tmp)
    k1 = np.sort(read_kmer_fasta_keys(fa, 31)[0])
    fa2, n2 = _subtract_reference_kmers(os.path.join(GIAB, "mini_ref.fa.k31.jf"), fa, tmp)
    n3, fa3 = _filter_parents_discovery(mother, father, None, fa2, 31, 4, tmp, 0)
    return (n, n2, n3), (k1, np.sort(read_kmer_fasta_keys(fa3, 31)[0]))


def test_discovery_chain_from_fastq(trio, tmp_path, monkeypatch):
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as jw
    paths, reads, _ = trio
    for name in ("KDF_DEVICE_FEEDER", "KDF_FASTQ_MIN_QUAL"):
        monkeypatch.delenv(name, raising=False)
    counts_b, sets_b = _chain(str(tmp_path / "bam"), CHILD, MOTHER, FATHER)
    assert jw.LAST_FEEDER == {"path": "host"}                # no FASTQ path given: the feeder it always was
    monkeypatch.setenv("KDF_FASTQ_FEED_MB", "0.25")          # several chunks per sample
    counts_f, sets_f = _chain(str(tmp_path / "fastq"), paths["child"], paths["mother"], paths["father"])
    assert jw.LAST_FEEDER["path"] == "fastq" and jw.LAST_FEEDER["records"] == len(reads["father"]) and jw.LAST_FEEDER["chunks"] > 1
    assert counts_f == counts_b and counts_f[0] == 51125 and counts_f[2] == 630
    for a, b in zip(sets_f, sets_b):
        np.testing.assert_array_equal(a, b)


def test_min_qual_from_the_environment(trio, monkeypatch):
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as jw
    from kmer_denovo_filter_amd.reads import ReadStream
    paths, reads, _ = trio
    quals = np.frombuffer(b"".join(q for _, q in reads["child"]), np.uint8)
    mq = int(np.sort(quals)[len(quals) // 20])               # one base in twenty is below it
    assert 33 < mq < 127 and (quals < mq).any()
    masked = [bytes(ord("N") if y < mq else x for x, y in zip(s, q)) for s, q in reads["child"]]

    def table(e):
        lo, hi, cnt = e.export_ge(0)
        o = np.argsort(lo, kind="stable")
        return lo[o].tolist(), cnt[o].tolist()
    for setting in (chr(mq), str(mq)):                       # a character or a number
        monkeypatch.setenv("KDF_FASTQ_MIN_QUAL", setting)
        with KmerEngine(31, capacity_hint=1 << 20) as dev, KmerEngine(31, capacity_hint=1 << 20) as host:
            jw._stream_bam(dev, paths["child"], None, 4, filtered=False)
            assert jw.LAST_FEEDER["path"] == "fastq" and jw.LAST_FEEDER["min_qual"] == mq
            host.count(ReadStream.from_strings(masked))
            assert table(dev) == table(host)
            host.clear()
            host.count(ReadStream.from_strings([s for s, _ in reads["child"]]))
            assert table(dev) != table(host)                 # (the mask took windows away)


def test_alignment_paths_refuse_a_fastq_child(trio):
    from kmer_denovo_filter_amd.core.bam_scanner import scan_bam_for_hits, scan_bam_module3
    from kmer_denovo_filter_amd.discovery.pipeline import _write_informative_reads_discovery
    from kmer_denovo_filter_amd.vcf.pipeline import _collect_child_kmers, _write_informative_reads
    child = trio[0]["child"]
    with pytest.raises(ValueError, match=r"scan_bam_module3.*FASTQ"):
        scan_bam_module3(child, kmer_size=31)
    with pytest.raises(ValueError, match=r"scan_bam_for_hits.*FASTQ"):
        next(iter(scan_bam_for_hits(child)))
    with pytest.raises(ValueError, match="FASTQ"):
        _write_informative_reads_discovery(child, None, [], 31, "out.bam")
    with pytest.raises(ValueError, match=r"VCF mode.*FASTQ"):
        _collect_child_kmers(child, None, [], 31, 0, 0, False, None)
    with pytest.raises(ValueError, match="FASTQ"):
        _write_informative_reads(child, None, {}, "out.bam")


def test_sizing_from_the_bases(trio):
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as jw
    from kmer_denovo_filter_amd.discovery.pipeline import _child_table_bytes
    paths, reads, d = trio
    size = os.path.getsize(paths["child"])
    assert jw._fastq_bases(paths["child"]) == size // 2
    assert jw._fastq_bases(paths["child"] + "," + paths["mother"]) == size // 2 + os.path.getsize(paths["mother"]) // 2
    gz = str(d / "x.fq.gz")
    with open(gz, "wb") as f:
        f.write(b"\x1f\x8b" + b"\0" * 998)
    assert jw._fastq_bases(gz) == 2000
    assert jw._engine_capacity_hint("1G", paths["child"]) == max(1 << 20, size // 2 * 6 // 10 * 3 // 10)
    assert _child_table_bytes(paths["child"]) == pytest.approx(4.6 * (size // 2 * 6 // 10))
    assert jw._engine_capacity_hint("1G", CHILD) == max(1 << 20, os.path.getsize(CHILD) * 3 // 10)      # a BAM: as before


def test_several_ranks_refuse_a_fastq_sample(trio, monkeypatch):
    from kmer_denovo_filter_amd import dist_env
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as jw
    monkeypatch.setattr(dist_env, "world_rank", lambda: (2, 0, False))
    with pytest.raises(ValueError, match="not sharded"):
        jw._stream_bam(None, trio[0]["child"], None, 4, filtered=False)       # (no engine: refused before any device call)
