"""VCF mode on the device: the variant-spanning windows of the child's reads, the parents' counts of their k-mers and the
per-variant evidence without a k-mer string or a k-mer FASTA anywhere (``include/kdf.h``, "VCF mode on the device").

The host path (``vcf/pipeline.py``: ``_collect_child_kmers`` -> FASTA -> ``scan_parents`` -> ``annotate_variants``)
builds an ``AlignedRead`` per read over a variant and Python sets of k-mer strings per (read, variant); it stays the
default and keeps its k <= 63 rule.  Here the same answers come from two engine calls per child batch
(``variant_windows_dev`` + ``hit_keys_dev``), one ``count --if`` of both parents against the child's keys, one
``variant_evidence_dev`` and a numpy reduction of the pair rows by read name.  Keys travel as (n, key_words) rows, so
every k the engine takes works, odd 65..201 included.

One difference to the host path: an ALT with a byte outside ACGT never matches here, while the host path would match a
read ``N`` against an ALT ``N`` (``read_supports_alt`` compares strings)."""
from __future__ import annotations

import numpy as np

from .. import dist_env
from ..core.jellyfish_wrappers import _stream_bam
from ..engine import KmerEngine
from ..kmer_utils import _is_symbolic
from ..reads import bam_reader, stream_words
from .pipeline import _records_over_positions, _variant_key

_SKIP_FLAGS = 0x4 | 0x100 | 0x800 | 0x400


def variant_arrays(variants, refs, ref_lengths):
    """The variants as the arrays ``variant_windows`` takes, in a linear coordinate (contig offset + pos), ascending.
    -> (var_pos int64, var_span uint32, var_ref_len uint32, alt bytes, alt_offsets int64, keys: the variant key of each
    row, contig offsets int64[len(refs)]).  Variants with one key share a row; a contig the BAM does not know is left out."""
    coff = np.concatenate(([0], np.cumsum(np.asarray(ref_lengths, dtype=np.int64)))).astype(np.int64)
    rid = {name: i for i, name in enumerate(refs)}
    rows = {}
    for v in variants:
        if v["chrom"] not in rid:
            continue
        alt = v["alt"]
        if alt is None:
            span, ab = 1, b""
        elif _is_symbolic(alt):
            span, ab = 0, b""
        else:
            span, ab = len(alt), alt.encode()
        rows.setdefault(_variant_key(v), (int(coff[rid[v["chrom"]]]) + int(v["pos"]), span, len(v["ref"]), ab))
    keys = sorted(rows, key=lambda key: rows[key][0])
    vals = [rows[key] for key in keys]
    ao = np.concatenate(([0], np.cumsum([len(x[3]) for x in vals]))).astype(np.int64)
    return (np.asarray([x[0] for x in vals], np.int64), np.asarray([x[1] for x in vals], np.uint32),
            np.asarray([x[2] for x in vals], np.uint32), b"".join(x[3] for x in vals), ao, keys, coff[:-1])


def annotations_from_rows(n_var, pair_var, pair_name, pair_flags, pair_rows, var_rows):
    """The reduction of the pair rows by (variant, name id) and of the variant rows into what ``annotate_variants``
    reports, per variant index: DKT = distinct names, DKU = distinct names of informative pairs (absent > 0), DKA =
    distinct names of informative pairs that support the ALT.  -> ([annotation dict], [informative name ids])"""
    pair_var = np.asarray(pair_var, dtype=np.int64)
    pair_name = np.asarray(pair_name, dtype=np.int64)
    inf = np.asarray(pair_rows, dtype=np.uint32).reshape(-1, 2)[:, 1] > 0
    alt = (np.asarray(pair_flags, dtype=np.uint8) & 1) != 0

    def distinct(mask):
        pairs = np.unique(np.stack((pair_var[mask], pair_name[mask]), axis=1), axis=0) if mask.any() else np.zeros((0, 2), np.int64)
        return np.bincount(pairs[:, 0], minlength=n_var), pairs
    dkt, _ = distinct(np.ones(len(pair_var), dtype=bool))
    dku, inf_pairs = distinct(inf)
    dka, _ = distinct(inf & alt)
    var_rows = np.asarray(var_rows, dtype=np.uint64).reshape(-1, 8)
    out, names = [], [[] for _ in range(n_var)]
    for v, nm in inf_pairs.tolist():
        names[v].append(nm)
    for v in range(n_var):
        t, u, a = int(dkt[v]), int(dku[v]), int(dka[v])
        n, sm, mn, mx, na, sa, mna, mxa = (int(x) for x in var_rows[v])
        out.append({"dku": u, "dkt": t, "dka": a,
                    "dku_dkt": round(u / t, 4) if t else 0.0, "dka_dkt": round(a / t, 4) if t else 0.0,
                    "max_pkc": mx, "avg_pkc": round(sm / n, 2) if n else 0.0, "min_pkc": mn,
                    "max_pkc_alt": mxa, "avg_pkc_alt": round(sa / na, 2) if na else 0.0, "min_pkc_alt": mna})
    return out, names


def _no_evidence():
    return annotations_from_rows(1, [], [], [], np.zeros((0, 2), np.uint32), np.zeros((1, 8), np.uint64))[0][0]


def annotate_vcf_device(child_bam, mother_bam, father_bam, variants, kmer_size, min_baseq, min_mapq, threads=4, device=0):
    """VCF mode through the engine's device path -> (metrics, annotations, informative_reads_by_variant).

    ``annotations`` and ``informative_reads_by_variant`` equal what ``annotate_variants`` and
    ``informative_reads_by_variant`` of the host path return; ``metrics`` holds ``total_child_kmers``,
    ``parent_found_kmers``, ``child_unique_kmers`` and ``variants_with_unique_reads``.  Every k the engine takes (1..63,
    odd 65..201).  Single process: under a process group of several ranks it raises ``ValueError`` before any device
    call.  An ALT with a byte outside ACGT never matches here (the host path would match a read ``N`` against an ALT
    ``N``)."""
    world = dist_env.world_rank()[0]
    if world > 1:
        raise ValueError(f"annotate_vcf_device runs in one process; {world} ranks are up (the multi-GPU VCF mode is the host path)")
    import torch
    dev = torch.device("cuda", int(device))
    k = int(kmer_size)
    rd = bam_reader(child_bam, flag_off=0, collapse=False, max_bases=1 << 24, threads=4, want_aux=True)
    refs = rd.references()
    var_pos, var_span, var_ref_len, alt, alt_offsets, var_keys, coff = variant_arrays(variants, refs, rd.reference_lengths())
    n_var = len(var_keys)
    by_chrom = {}
    for v in variants:
        by_chrom.setdefault(v["chrom"], []).append(int(v["pos"]))
    vpos = {c: np.unique(np.asarray(ps, dtype=np.int64)) for c, ps in by_chrom.items()}
    has_var = np.asarray([name in vpos for name in refs], dtype=bool)

    def up(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        return torch.from_numpy((a if a.size else np.zeros(1, dt)).view(np.uint8).copy()).to(dev)
    name_ids = {}
    keys_parts, ep_parts, pv_parts, pf_parts, pn_parts = [], [], [], [], []
    n_pairs_total = 0
    with KmerEngine(k, capacity_hint=1 << 12, device=int(device)) as eng, rd:
        W = eng.key_words
        d_vp, d_vs, d_vr = up(var_pos, np.int64), up(var_span, np.uint32), up(var_ref_len, np.uint32)
        d_alt, d_ao = up(np.frombuffer(alt, np.uint8), np.uint8), up(alt_offsets, np.int64)
        for batch in rd if n_var else ():
            n = batch.n_reads
            rid = np.asarray(batch.ref_ids[:n], dtype=np.int64)
            ok = ((np.asarray(batch.flags[:n]) & _SKIP_FLAGS) == 0) & (np.asarray(batch.mapq[:n]) >= min_mapq)
            ok &= (rid >= 0) & (rid < len(refs))
            ok[ok] = has_var[rid[ok]]
            ref_start = np.where(ok, coff[np.clip(rid, 0, max(len(refs) - 1, 0))] + np.asarray(batch.positions[:n], dtype=np.int64), -1)
            if not ok.any():
                continue
            # qualities only of the reads that lie over a variant, and of those only when the BAM stores some
            keep, _ = _records_over_positions(batch, refs, vpos, ok)
            qo_all = np.asarray(batch.qual_offsets, dtype=np.int64)
            qlen = np.zeros(n, dtype=np.int64)
            if min_baseq > 0 and len(keep) and len(batch.quals):
                ln = qo_all[keep + 1] - qo_all[keep]
                stored = (ln > 0) & (batch.quals[np.minimum(qo_all[keep], len(batch.quals) - 1)] != 0xFF)
                qlen[keep] = np.where(stored, ln, 0)
            qoff = np.concatenate(([0], np.cumsum(qlen))).astype(np.int64)
            src = np.repeat(qo_all[:n] - qoff[:n], qlen) + np.arange(int(qoff[-1]), dtype=np.int64)
            qual = batch.quals[src] if len(src) else np.zeros(0, np.uint8)
            nb = int(batch.n_bases)
            pw, mw = stream_words(nb)
            d_p, d_m = up(batch.packed[:pw], np.uint64), up(batch.invalid[:mw], np.uint64)
            d_o, d_rs = up(batch.offsets, np.int64), up(ref_start, np.int64)
            d_cg, d_co = up(batch.cigar, np.uint32), up(batch.cigar_offsets, np.int64)
            d_q, d_qo = up(qual, np.uint8), up(qoff, np.int64)
            torch.cuda.synchronize(dev)
            args = (d_p.data_ptr(), d_m.data_ptr(), nb, d_o.data_ptr(), n, d_rs.data_ptr(), d_cg.data_ptr(), len(batch.cigar), d_co.data_ptr(),
                    d_q.data_ptr() if min_baseq > 0 else None, len(qual), d_qo.data_ptr() if min_baseq > 0 else None, int(min_baseq),
                    d_vp.data_ptr(), d_vs.data_ptr(), d_vr.data_ptr(), n_var, d_alt.data_ptr(), len(alt), d_ao.data_ptr())
            n_pairs, n_ent = eng.variant_windows_dev(*args, None, None, None, 0, None, None, 0)
            if n_pairs == 0:
                continue
            d_pr = torch.empty(n_pairs, dtype=torch.int64, device=dev)
            d_pv = torch.empty(n_pairs, dtype=torch.int32, device=dev)
            d_pf = torch.empty(n_pairs, dtype=torch.uint8, device=dev)
            d_ep = torch.empty(n_ent, dtype=torch.int64, device=dev)
            d_epair = torch.empty(n_ent, dtype=torch.int64, device=dev)
            d_keys = torch.empty((n_ent, W), dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            eng.variant_windows_dev(*args, d_pr.data_ptr(), d_pv.data_ptr(), d_pf.data_ptr(), n_pairs, d_ep.data_ptr(), d_epair.data_ptr(), n_ent)
            eng.hit_keys_dev(d_p.data_ptr(), nb, d_ep.data_ptr(), n_ent, d_keys.data_ptr())
            eng.synchronize()
            # kept: the key rows, entry_pair re-based, the pair arrays and a name id per pair; the stream goes
            keys_parts.append(d_keys)
            ep_parts.append(d_epair + n_pairs_total)
            pv_parts.append(d_pv)
            pf_parts.append(d_pf)
            pn_parts.append(np.asarray([name_ids.setdefault(batch.name(r), len(name_ids)) for r in d_pr.cpu().tolist()], dtype=np.int64))
            n_pairs_total += n_pairs
        if not keys_parts:
            ann = {_variant_key(v): _no_evidence() for v in variants}
            return {"total_child_kmers": 0, "parent_found_kmers": 0, "child_unique_kmers": 0, "variants_with_unique_reads": 0}, ann, {}
        d_keys, d_ep = torch.cat(keys_parts).contiguous(), torch.cat(ep_parts).contiguous()
        d_pv, d_pf = torch.cat(pv_parts).contiguous(), torch.cat(pf_parts).contiguous()
        pair_name = np.concatenate(pn_parts)
        n_ent = int(d_ep.numel())
        torch.cuda.synchronize(dev)
        if W <= 2:
            d_lo = d_keys[:, 0].contiguous()
            d_hi = d_keys[:, 1].contiguous() if W == 2 else None
            torch.cuda.synchronize(dev)
            eng.load_filter_dev(d_lo.data_ptr(), d_hi.data_ptr() if W == 2 else None, n_ent)
        else:
            eng.load_filter_dev(d_keys.data_ptr(), None, n_ent)
        total = eng.count_ge(0)
        for bam in (mother_bam, father_bam):
            _stream_bam(eng, bam, None, threads, filtered=True)
        found = eng.count_ge(1)
        d_prow = torch.empty((n_pairs_total, 2), dtype=torch.int32, device=dev)
        d_vrow = torch.empty((n_var, 8), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        eng.variant_evidence_dev(d_keys.data_ptr(), d_ep.data_ptr(), n_ent, d_pv.data_ptr(), d_pf.data_ptr(), n_pairs_total, n_var,
                                 d_prow.data_ptr(), d_vrow.data_ptr())
        eng.synchronize()
        pair_rows = d_prow.cpu().numpy().view(np.uint32)
        var_rows = d_vrow.cpu().numpy().view(np.uint64)
        pair_var = d_pv.cpu().numpy().view(np.uint32)
        pair_flags = d_pf.cpu().numpy()
    rows, inf_names = annotations_from_rows(n_var, pair_var, pair_name, pair_flags, pair_rows, var_rows)
    name_of = {i: nm for nm, i in name_ids.items()}
    ann = {key: rows[i] for i, key in enumerate(var_keys)}
    for v in variants:                                     # (a contig the child BAM does not know: no read, no evidence)
        ann.setdefault(_variant_key(v), _no_evidence())
    informative = {var_keys[i]: {name_of[x] for x in ids} for i, ids in enumerate(inf_names) if ids}
    metrics = {"total_child_kmers": int(total), "parent_found_kmers": int(found), "child_unique_kmers": max(0, int(total) - int(found)),
               "variants_with_unique_reads": sum(1 for a in ann.values() if a["dku"] > 0)}
    return metrics, ann, informative
