"""The discovery chain and Module 3 at long k (odd 65..201), one process, on the GIAB mini trio: every stage's k-mer
set and the informative reads against a pure-Python restatement of the same chain (oracle.py_count / canonicalize on
the oracle's own BAM and FASTA readers; the C oracle table stops at k = 64).  VCF mode and mirrors under a process
group of several ranks refuse long k by name."""
import os
import shutil

import pytest

from conftest import GIAB

pytestmark = pytest.mark.gpu

MIN_CHILD, PARENT_MAX, MIN_DK = 3, 0, 1


def _kmer_set(rows, k):
    from kmer_denovo_filter_amd.reads import keys_to_kmers
    return set(keys_to_kmers(rows, None, k))


def _windows(seq, k, O):
    s = seq.upper()
    return {O.canonicalize(s[i:i + k]) for i in range(len(s) - k + 1) if all(ch in "ACGT" for ch in s[i:i + k])}


@pytest.fixture(scope="module", params=(75, 101))
def chain(request, tmp_path_factory, oracle, trio_reads):
    """Run the mirrors' chain at k and restate it in Python."""
    from kmer_denovo_filter_amd import jf_io
    from kmer_denovo_filter_amd.core import bam_scanner
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _build_proband_jf_index, _ensure_ref_jf, _merge_jf_files
    from kmer_denovo_filter_amd.discovery.pipeline import (
        _extract_child_kmers_discovery, _filter_parents_discovery, _subtract_reference_kmers,
        _write_informative_reads_discovery)
    from kmer_denovo_filter_amd.kmer_fasta import read_kmer_fasta_keys
    k = request.param
    tmp = str(tmp_path_factory.mktemp(f"long{k}"))
    fa = os.path.join(tmp, "mini_ref.fa")
    shutil.copy(os.path.join(GIAB, "mini_ref.fa"), fa)              # nothing is written under tests/golden
    child_bam = os.path.join(GIAB, "HG002_child.bam")
    got = {"k": k, "tmp": tmp}
    ref_jf = _ensure_ref_jf(fa, k, 4)
    assert ref_jf.startswith(tmp)
    got["ref_index"] = jf_io.read_index(ref_jf, expect_k=k)
    cand_fa, n = _extract_child_kmers_discovery(child_bam, None, k, MIN_CHILD, 4, tmp)
    got["candidates"] = (n, _kmer_set(read_kmer_fasta_keys(cand_fa, k)[0], k))
    nr_fa, n2 = _subtract_reference_kmers(ref_jf, cand_fa, tmp)
    got["non_ref"] = (n2, _kmer_set(read_kmer_fasta_keys(nr_fa, k)[0], k))
    n3, pu_fa = _filter_parents_discovery(os.path.join(GIAB, "HG004_mother.bam"), os.path.join(GIAB, "HG003_father.bam"),
                                          None, nr_fa, k, 4, tmp, PARENT_MAX)
    got["proband_unique"] = (n3, _kmer_set(read_kmer_fasta_keys(pu_fa, k)[0], k) if pu_fa else set())
    pjf = _build_proband_jf_index(pu_fa, k, tmp, n3)
    got["proband_index"] = jf_io.read_index(pjf, expect_k=k)
    bam_scanner._init_scan_worker(pjf, k, MIN_DK)
    got["module3"] = bam_scanner.scan_bam_module3(child_bam)
    out_bam = os.path.join(tmp, "informative.bam")
    got["informative_bam"] = (_write_informative_reads_discovery(child_bam, None, pu_fa, k, out_bam), out_bam)
    # _merge_jf_files: two copies of the reference index sum to twice its counts
    a, b = os.path.join(tmp, "a.jf"), os.path.join(tmp, "b.jf")
    shutil.copy(ref_jf, a); shutil.copy(ref_jf, b)
    got["merged"] = jf_io.read_index(_merge_jf_files([a, b], os.path.join(tmp, "merged.jf")), expect_k=k)

    # the same chain as plain Python over the oracle's readers
    ref_seqs = [s for _, s in oracle.read_fasta(os.path.join(GIAB, "mini_ref.fa"))]
    want = {"ref_index": oracle.py_count(ref_seqs, k)}
    child = oracle.py_count(trio_reads["child"], k)
    cand = {c for c, v in child.items() if v >= MIN_CHILD}
    non_ref = cand - set(want["ref_index"])
    m = oracle.py_count(trio_reads["mother"], k, non_ref)
    after_m = {c for c in non_ref if m[c] <= PARENT_MAX}
    f = oracle.py_count(trio_reads["father"], k, after_m)
    want.update(candidates=cand, non_ref=non_ref, proband_unique={c for c in after_m if f[c] <= PARENT_MAX})
    return got, want


def test_every_stage_set(chain, oracle):
    from kmer_denovo_filter_amd.reads import keys_to_kmers
    got, want = chain
    k = got["k"]
    _, keys, hi, cnt = got["ref_index"]
    assert hi is None and keys.shape[1] == (2 * k + 63) // 64
    assert dict(zip(keys_to_kmers(keys, None, k), cnt.tolist())) == want["ref_index"]
    for stage in ("candidates", "non_ref", "proband_unique"):
        n, s = got[stage]
        assert n == len(s) == len(want[stage]) and s == want[stage], stage
    assert len(want["proband_unique"]) > 0
    _, pkeys, _, pcnt = got["proband_index"]
    assert _kmer_set(pkeys, k) == want["proband_unique"] and (pcnt == 1).all()
    _, mkeys, _, mcnt = got["merged"]
    assert dict(zip(keys_to_kmers(mkeys, None, k), mcnt.tolist())) == {c: 2 * v for c, v in want["ref_index"].items()}


def test_module3_informative_reads(chain, oracle):
    got, want = chain
    k = got["k"]
    pu = want["proband_unique"]
    refs, recs = oracle.read_bam(os.path.join(GIAB, "HG002_child.bam"))
    tasks = {}
    for r in recs:
        if r.is_secondary or r.is_duplicate:
            continue
        tasks.setdefault(r.ref_id, []).append(r)
    informative, unmapped, first_hits = set(), 0, {}
    for ref_id in [i for i in range(len(refs)) if i in tasks] + ([-1] if -1 in tasks else []):
        seen = set()
        for r in tasks[ref_id]:
            hits = _windows(r.seq, k, oracle) & pu
            if len(hits) < MIN_DK:
                continue
            key = (r.qname, r.is_supplementary)
            if key in seen:
                continue
            seen.add(key)
            if r.is_unmapped:
                unmapped += 1
            elif key not in informative:
                first_hits[key] = hits
        informative |= seen
    read_hits, reads_seen, unmapped_inf, total, _, _, _ = got["module3"]
    assert reads_seen == informative and len(informative) > 0
    assert unmapped_inf == unmapped
    assert {(h[3], h[5]): h[4] for h in read_hits} == first_hits
    n_bam, _ = got["informative_bam"]
    assert n_bam == len(informative)


def test_kmer_query_and_automaton_at_long_k(chain):
    from kmer_denovo_filter_amd.kmer_utils import JellyfishKmerQuery, build_kmer_automaton
    got, want = chain
    k = got["k"]
    pu = sorted(want["proband_unique"])
    absent = sorted(want["non_ref"] - want["proband_unique"])[:20]
    q = JellyfishKmerQuery(os.path.join(got["tmp"], "proband_unique.jf"))
    assert q.query_batch(pu[:50] + absent) == set(pu[:50])
    read = "N" + pu[0] + "ACGT" + pu[1]
    uniq, idx = q.scan_read(read, k)
    assert {pu[0], pu[1]} <= uniq and {1, k + 5} <= idx
    q.release()
    auto = build_kmer_automaton(pu[:10])
    assert [c for _, c in auto.iter(pu[3])] == [pu[3]]


def test_vcf_mode_and_multi_rank_mirrors_refuse_long_k(tmp_path, monkeypatch):
    from kmer_denovo_filter_amd import dist_env
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_kmers_discovery
    from kmer_denovo_filter_amd.vcf.pipeline import _collect_child_kmers, scan_parents
    child = os.path.join(GIAB, "HG002_child.bam")
    with pytest.raises(ValueError, match="VCF mode takes k <= 63"):
        _collect_child_kmers(child, None, [], 101, 20, 20, False, str(tmp_path / "c.fa"))
    with pytest.raises(ValueError, match="VCF mode takes k <= 63"):
        scan_parents(os.path.join(GIAB, "HG004_mother.bam"), os.path.join(GIAB, "HG003_father.bam"), None,
                     str(tmp_path / "c.fa"), 101, str(tmp_path), 4, 0)
    monkeypatch.setattr(dist_env, "world_rank", lambda: (2, 0, True))    # a rank of a two-process group
    with pytest.raises(ValueError, match="2 ranks"):
        _extract_child_kmers_discovery(child, None, 101, 3, 4, str(tmp_path))
