"""The model of "VCF mode on the device" (tests/variants_model.py, written from include/kdf.h) against the host path it
restates: extract_variant_spanning_kmers and read_supports_alt on alignment.AlignedRead, annotate_variants and
informative_reads_by_variant on k-mer string sets.  No GPU."""
import numpy as np
import pytest

import variants_model as VM


def aligned(seq, ops, start, quals=None):
    from kmer_denovo_filter_amd.alignment import AlignedRead
    return AlignedRead("r", 0, 0, "chr1", start, 60, list(ops), seq, None if quals is None else np.asarray(quals, np.uint8))


def model_kmers(case, k, pair, got):
    """the canonical k-mer strings of the entries of one pair of the model's output"""
    from kmer_denovo_filter_amd.kmer_utils import canonicalize
    pr, _pv, _pf, ep, epair = got
    r = int(pr[pair])
    seq, b = case["reads"][r][0].upper(), int(case["offsets"][r])
    return {canonicalize(seq[int(p) - b:int(p) - b + k]) for p in ep[epair == pair]}


def host_pairs(case, k):
    """{(read, variant): (k-mer set, supports_alt)} by the host helpers, for literal and missing ALTs"""
    from kmer_denovo_filter_amd.kmer_utils import extract_variant_spanning_kmers, read_supports_alt
    out = {}
    mb = case["min_baseq"]
    for r, (seq, ops, rs, q) in enumerate(case["reads"]):
        if rs < 0:
            continue
        read = aligned(seq, ops, rs, q)
        for v, (pos, span, ref_len, alt) in enumerate(case["variants"]):
            if span == 0:
                continue
            a = alt.decode() if alt else None
            ks = extract_variant_spanning_kmers(read, pos, k, mb, ref="A" * ref_len, alt=a)
            if ks:
                out[(r, v)] = ({x.upper() for x in ks}, read_supports_alt(read, pos, "A" * ref_len, a, min_baseq=mb))
    return out


@pytest.mark.parametrize("k", [5, 11, 23])
@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_host_helpers_on_random_cases(seed, k):
    case = VM.random_case(1000 * k + seed, n_reads=40, n_var=16, min_baseq=20 if seed % 3 else 0, ragged=False)
    got = VM.variant_windows(case, k)
    pr, pv, pf, ep, epair = got
    want = host_pairs(case, k)
    assert [(int(r), int(v)) for r, v in zip(pr, pv)] == sorted(want), "the pairs, in (read, variant) order"
    assert len(pr) > 0 and np.array_equal(epair, np.sort(epair)) and len(set(epair.tolist())) == len(pr)
    for i, (r, v) in enumerate(zip(pr.tolist(), pv.tolist())):
        ks, sup = want[(r, v)]
        assert model_kmers(case, k, i, got) == ks, (r, v)
        p = ep[epair == i]
        assert (np.diff(p.astype(np.int64)) > 0).all(), "entries of a pair ascend"
        alt = case["variants"][v][3]
        if all(ch in b"ACGTacgt" for ch in alt):            # (an ALT with an N: the host path compares strings)
            assert bool(pf[i] & 1) == sup, (r, v, case["reads"][r], case["variants"][v])
        else:
            assert pf[i] == 0


def test_random_cases_cover_the_ground():
    """anchors in deletions, in front of and behind reads, before insertions; pairs that support and do not; entries
    dropped for quality and for N"""
    stats = {"pairs": 0, "alt": 0, "no_anchor": 0, "ins_alt": 0, "del_alt": 0, "empty": 0}
    for seed in range(12):
        case = VM.random_case(seed, n_reads=40, n_var=16, min_baseq=20, ragged=False)
        pr, pv, pf, ep, epair = VM.variant_windows(case, 7)
        stats["pairs"] += len(pr)
        stats["alt"] += int(pf.sum())
        for i, v in enumerate(pv.tolist()):
            _pos, span, ref_len, _alt = case["variants"][v]
            stats["ins_alt"] += int(pf[i] and span > 1)
            stats["del_alt"] += int(pf[i] and ref_len > 1)
        for r, (seq, ops, rs, _q) in enumerate(case["reads"]):
            for pos, span, *_x in case["variants"]:
                if rs >= 0 and span and rs <= pos < rs + VM.walk(ops)[2]:
                    a = VM.anchor(ops, pos - rs)
                    stats["no_anchor"] += a is None
                    stats["empty"] += a is not None and not ((pr == r) & (case["var_pos"][pv] == pos)).any()
    assert stats["pairs"] > 200 and 20 < stats["alt"] < stats["pairs"], stats
    assert stats["no_anchor"] > 5 and stats["ins_alt"] > 0 and stats["del_alt"] > 0 and stats["empty"] > 0, stats


def test_the_reference_unit_cases():
    """tests/test_vcf_host.py's AlignedRead calls, restated as model calls"""
    def run(seq, start, pos, k, ops=None, quals=None, min_baseq=0, span=1, ref_len=1, alt=b""):
        case = VM.pack_case([(seq, ops or [(0, len(seq))], start, None if quals is None else np.asarray(quals, np.uint8))],
                            [(pos, span, ref_len, alt)], min_baseq, with_qual=quals is not None)
        return VM.variant_windows(case, k)
    pr, pv, pf, ep, epair = run("ACGTACGT", 100, 102, 4)
    assert ep.tolist() == [0, 1, 2] and pr.tolist() == [0] and epair.tolist() == [0, 0, 0]
    assert len(run("ACGT", 100, 200, 3)[0]) == 0
    assert len(run("ACGTACGT", 100, 102, 4, quals=[30, 30, 5, 30, 30, 30, 30, 30], min_baseq=20)[0]) == 0
    assert len(run("ACNTACGT", 100, 102, 4)[0]) == 0
    assert run("TTTTAAAA", 100, 103, 4)[3].tolist() == [0, 1, 2, 3]
    ins = [(0, 4), (1, 3), (0, 4)]
    got = run("ACGTTTTACGT", 100, 103, 4, ops=ins, span=4, alt=b"TTTT")
    assert got[3].tolist() == [0, 1, 2, 3, 4, 5, 6] and got[2].tolist() == [1]      # GTTT at 2, TTTA at 4; supports TTTT
    # read_supports_alt
    assert run("ACGTACGT", 100, 102, 4, alt=b"G")[2].tolist() == [1]
    assert run("ACGTACGT", 100, 102, 4, alt=b"T")[2].tolist() == [0]
    assert len(run("ACGTACGT", 100, 102, 4, span=0, alt=b"<DEL>")[0]) == 0          # symbolic: skipped entirely
    assert run("ACGTACGT", 100, 102, 4, alt=b"")[2].tolist() == [0]                 # missing ALT: a pair, never a match
    assert len(run("ACGTACGT", 100, 300, 4, alt=b"G")[0]) == 0
    assert run("ACGACGT", 100, 102, 3, ops=[(0, 3), (2, 2), (0, 4)], ref_len=3, alt=b"G")[2].tolist() == [1]
    low = run("ACGTACGTAC", 100, 106, 4, quals=[30, 30, 30, 30, 30, 30, 30, 5, 30, 30], min_baseq=20, ref_len=2, alt=b"GT")
    assert len(low[0]) == 1 and low[2].tolist() == [0]                               # a low base inside the ALT span only


def variant_dicts(case):
    return [{"chrom": f"v{v}", "pos": int(pos), "ref": "A" * ref_len, "alt": (alt.decode() if alt else None)}
            for v, (pos, _span, ref_len, alt) in enumerate(case["variants"])]


@pytest.mark.parametrize("seed", range(4))
def test_evidence_rows_equal_annotate_variants(seed):
    from kmer_denovo_filter_amd.vcf.device import annotations_from_rows
    from kmer_denovo_filter_amd.vcf.pipeline import _variant_key, annotate_variants, informative_reads_by_variant
    k = 9
    rng = np.random.default_rng(77 + seed)
    case = VM.random_case(500 + seed, n_reads=60, n_var=14, min_baseq=20, ragged=False)
    got = VM.variant_windows(case, k)
    pr, pv, pf, ep, epair = got
    variants = variant_dicts(case)
    name_id = [int(r) // 2 for r in pr]                      # two records share a name (mates)
    per_variant, every = {}, set()
    for i in range(len(pr)):
        ks = model_kmers(case, k, i, got)
        every |= ks
        per_variant.setdefault(_variant_key(variants[int(pv[i])]), []).append((f"n{name_id[i]}", ks, bool(pf[i] & 1)))
    every = sorted(every)
    found = {x: int(rng.integers(1, 50)) for x in every if rng.random() < 0.6}
    want = annotate_variants(variants, per_variant, found)
    want_inf = informative_reads_by_variant(variants, per_variant, found)
    # the model's keys: the canonical strings themselves
    from kmer_denovo_filter_amd.kmer_utils import canonicalize
    keys = []
    for p, i in zip(ep.tolist(), epair.tolist()):
        r = int(pr[i])
        s = int(p) - int(case["offsets"][r])
        keys.append(canonicalize(case["reads"][r][0].upper()[s:s + k]))
    pair_rows, var_rows = VM.variant_evidence(keys, epair, pv, pf, len(variants), found)
    rows, inf = annotations_from_rows(len(variants), pv, name_id, pf, pair_rows, var_rows)
    assert any(a["dku"] for a in rows) and any(a["dka"] for a in rows) and any(a["max_pkc_alt"] for a in rows)
    for v, var in enumerate(variants):
        assert rows[v] == want[_variant_key(var)], (v, rows[v], want[_variant_key(var)])
        assert {f"n{x}" for x in inf[v]} == want_inf.get(_variant_key(var), set())


def test_evidence_ignores_out_of_range_indices_and_missing_keys():
    keys = ["a", "b", None, "a", "c", "a"]
    entry_pair = np.asarray([0, 0, 0, 1, 7, 2], np.uint64)       # entry 4: no such pair
    pair_var = np.asarray([1, 1, 9], np.uint32)                  # pair 2: no such variant
    pair_flags = np.asarray([0, 1, 1], np.uint8)
    pair_rows, var_rows = VM.variant_evidence(keys, entry_pair, pair_var, pair_flags, 2, {"a": 5, "b": 0, "c": 3})
    assert pair_rows.tolist() == [[3, 2], [1, 0], [0, 0]]
    assert var_rows.tolist() == [[0] * 8, [1, 5, 5, 5, 1, 5, 5, 5]]
