"""Plain-Python / numpy model of "VCF mode on the device" (kdf_variant_windows*, kdf_variant_evidence*), written from
the contract text of include/kdf.h alone: a walk per (read, variant), no prefix sums, no search.  Slow and obvious.

A case is a dict of arrays, as ``pack_case`` builds it from per-read tuples; the generator ``random_case`` is shared by
the CPU test (model against the AlignedRead helpers) and the GPU test (engine against the model)."""
import numpy as np

ALIGNED, QUERY_ONLY, REF_ONLY = (0, 7, 8), (1, 4), (2, 3)
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def stream_arrays(packed, invalid, n_bases):
    """(base codes uint8[n_bases], bad bool[n_bases]) of a packed stream; nothing at or past n_bases exists"""
    pos = np.arange(int(n_bases), dtype=np.int64)
    packed, invalid = np.asarray(packed, np.uint64), np.asarray(invalid, np.uint64)
    codes = ((packed[pos >> 5] >> (2 * (pos & 31)).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
    bad = ((invalid[pos >> 6] >> (pos & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    return codes, bad


def walk(ops):
    """[(op, length, query bases before, reference bases before)] and the two totals"""
    out, qc, rc = [], 0, 0
    for op, ln in ops:
        out.append((op, ln, qc, rc))
        if op in ALIGNED:
            qc += ln; rc += ln
        elif op in QUERY_ONLY:
            qc += ln
        elif op in REF_ONLY:
            rc += ln
    return out, qc, rc


def anchor(ops, d):
    """the query index aligned at reference offset d, or None"""
    for op, ln, qc, rc in walk(ops)[0]:
        if op in ALIGNED and rc <= d < rc + ln:
            return qc + (d - rc)
    return None


def query_end(ops, e):
    """query bases consumed when the walk first stands on a reference offset >= e inside M, =, X, D or N"""
    steps, qtot, _ = walk(ops)
    for op, ln, qc, rc in steps:
        if (op in ALIGNED or op in REF_ONLY) and ln > 0 and rc + ln > e:
            return qc + (max(e - rc, 0) if op in ALIGNED else 0)
    return qtot


def variant_windows(case, k, n_bases=None):
    """-> (pair_read int64, pair_var uint32, pair_flags uint8, entry_pos uint64, entry_pair uint64)"""
    n_bases = case["n_bases"] if n_bases is None else n_bases
    codes, badmask = stream_arrays(case["packed"], case["invalid"], n_bases)
    offs, rs, cg, co = case["offsets"], case["ref_start"], case["cigar"], case["cigar_offsets"]
    qual, qo, min_baseq = case.get("qual"), case.get("qual_offsets"), case.get("min_baseq", 0)
    alt, ao = case["alt"], case["alt_offsets"]
    pr, pv, pf, ep, epair = [], [], [], [], []
    for r in range(len(offs) - 1):
        if rs[r] < 0:
            continue
        ops = [(int(w) & 15, int(w) >> 4) for w in cg[co[r]:co[r + 1]]]
        b, lim = int(offs[r]), min(int(offs[r + 1]), int(n_bases))

        def bad(c):                                         # query index c, b + c < lim
            if badmask[b + c]:
                return True
            if qual is not None and min_baseq > 0 and c < qo[r + 1] - qo[r]:
                return qual[qo[r] + c] < min_baseq
            return False
        for v in range(len(case["var_pos"])):
            span = int(case["var_span"][v])
            if span == 0:
                continue
            d = int(case["var_pos"][v]) - int(rs[r])
            at = anchor(ops, d) if d >= 0 else None
            if at is None:
                continue
            entries = []
            for s in range(max(0, at - k + 1), at + span):
                p = b + s
                if p + k > lim:
                    break
                if not any(bad(s + j) for j in range(k)):
                    entries.append(p)
            if not entries:
                continue
            a = bytes(alt[ao[v]:ao[v + 1]]).decode("latin-1").upper()
            qe = query_end(ops, d + int(case["var_ref_len"][v]))
            sup = bool(a) and all(ch in CODE for ch in a) and qe - at == len(a) and b + qe <= lim
            if sup:
                sup = all(not bad(at + j) and codes[b + at + j] == CODE[a[j]] for j in range(len(a)))
            for p in entries:
                ep.append(p)
                epair.append(len(pr))
            pr.append(r); pv.append(v); pf.append(1 if sup else 0)
    return (np.asarray(pr, np.int64), np.asarray(pv, np.uint32), np.asarray(pf, np.uint8), np.asarray(ep, np.uint64),
            np.asarray(epair, np.uint64))


def variant_evidence(keys, entry_pair, pair_var, pair_flags, n_var, counts):
    """keys: one hashable per entry (None: no key); counts: {key: stored count}.  -> (pair_rows uint32 (n_pairs, 2),
    var_rows uint64 (n_var, 8))"""
    n_pairs = len(pair_var)
    pair_rows = np.zeros((n_pairs, 2), np.uint32)
    seen = [(dict(), dict()) for _ in range(n_var)]
    for key, p in zip(keys, entry_pair):
        p = int(p)
        if p >= n_pairs or int(pair_var[p]) >= n_var:
            continue
        c = counts.get(key, 0) if key is not None else 0
        pair_rows[p, 0] += 1
        if c == 0:
            pair_rows[p, 1] += 1
            continue
        v = int(pair_var[p])
        seen[v][0][key] = c
        if pair_flags[p] & 1:
            seen[v][1][key] = c
    var_rows = np.zeros((n_var, 8), np.uint64)
    for v in range(n_var):
        for t in (0, 1):
            c = list(seen[v][t].values())
            if c:
                var_rows[v, 4 * t:4 * t + 4] = (len(c), sum(c), min(c), max(c))
    return pair_rows, var_rows


# ---- cases ------------------------------------------------------------------------------------------------------------------

def pack_case(reads, variants, min_baseq=0, with_qual=True):
    """reads: [(sequence str, [(op, length)], ref_start, qualities uint8 array or None)]; variants: [(pos, span, ref_len,
    alt bytes)], sorted here by position (stable).  The stream is packed as kdf_pack_reads packs it: a separator after
    every read, everything but ACGT (either case) invalid."""
    variants = sorted(variants, key=lambda x: x[0])
    n = sum(len(s) + 1 for s, *_ in reads)
    pw, mw = 2 * ((n + 63) // 64) + 4, (n + 63) // 64 + 2
    packed, invalid = np.zeros(pw, np.uint64), np.full(mw, ~np.uint64(0), np.uint64)
    offs, p = [0], 0
    for s, *_ in reads:
        for ch in s.upper():
            if ch in CODE:
                packed[p >> 5] |= np.uint64(CODE[ch] << (2 * (p & 31)))
                invalid[p >> 6] &= ~np.uint64(1 << (p & 63))
            p += 1
        p += 1
        offs.append(p)
    cg, co, ql, qo = [], [0], [], [0]
    for s, ops, _rs, q in reads:
        cg += [(ln << 4) | op for op, ln in ops]
        co.append(len(cg))
        if with_qual and q is not None:
            ql += list(q)
        qo.append(len(ql))
    alt = b"".join(a for *_x, a in variants)
    ao = np.concatenate(([0], np.cumsum([len(a) for *_x, a in variants]))).astype(np.int64)
    return {"packed": packed, "invalid": invalid, "n_bases": n, "offsets": np.asarray(offs, np.int64),
            "ref_start": np.asarray([r[2] for r in reads], np.int64), "cigar": np.asarray(cg, np.uint32),
            "cigar_offsets": np.asarray(co, np.int64), "qual": np.asarray(ql, np.uint8) if with_qual else None,
            "qual_offsets": np.asarray(qo, np.int64) if with_qual else None, "min_baseq": min_baseq,
            "var_pos": np.asarray([x[0] for x in variants], np.int64), "var_span": np.asarray([x[1] for x in variants], np.uint32),
            "var_ref_len": np.asarray([x[2] for x in variants], np.uint32), "alt": alt, "alt_offsets": ao,
            "reads": reads, "variants": variants}


def random_read(rng, lo=20, hi=60, max_ops=6, start_hi=400, ragged=True):
    """(sequence, ops, ref_start, qualities): up to max_ops operations drawn from M I D N S H = X, the sequence as long
    as the CIGAR's query bases (ragged: sometimes a few more or fewer), some N bases, some low qualities"""
    L = int(rng.integers(lo, hi + 1))
    n_ops = int(rng.integers(1, max_ops + 1))
    cuts = np.sort(rng.choice(np.arange(1, L), size=min(n_ops - 1, L - 1), replace=False)) if n_ops > 1 else []
    lens = np.diff(np.concatenate(([0], cuts, [L]))).astype(int)
    ops = []
    for i, ln in enumerate(lens):
        op = int(rng.choice([0, 0, 0, 7, 8, 1, 2, 3, 4, 5]))
        if op in (4, 5) and 0 < i < len(lens) - 1:
            op = 0
        if i == 0 and op in (1, 2, 3):
            op = 0
        ops.append((op, int(ln) if op not in (2, 3) else int(rng.integers(1, 9))))
    qlen = sum(ln for op, ln in ops if op in ALIGNED + QUERY_ONLY)
    slen = max(1, qlen + (int(rng.choice([0, 0, 0, 0, -3, 4])) if ragged else 0))
    seq = "".join(rng.choice(list("ACGT"), slen))
    seq = "".join("N" if rng.random() < 0.02 else ch for ch in seq)
    if rng.random() < 0.2:
        seq = seq.lower()
    q = rng.integers(25, 41, slen).astype(np.uint8)
    q[rng.random(slen) < 0.03] = 5
    return seq, ops, int(rng.integers(0, start_hi)), q


def variants_for(rng, reads, n, equal_runs=True):
    """n variants aimed at the reads: positions on aligned bases, inside deletions, in front of and behind a read and
    directly before an insertion; SNVs, insertions up to 12 bases, deletions with ref_len up to 8, a missing ALT, a
    symbolic one (span 0) and an ALT with an N"""
    out = []
    while len(out) < n:
        seq, ops, rs, _q = reads[int(rng.integers(len(reads)))]
        steps, _qt, rtot = walk(ops)
        kind = rng.random()
        pos = rs + int(rng.integers(0, max(rtot, 1)))
        if kind < 0.15:
            # directly before an insertion or a deletion of the read, with the allele the read then carries
            edge = [(cur, nxt) for cur, nxt in zip(steps, steps[1:]) if nxt[0] in (1, 2) and cur[0] in ALIGNED and cur[1] > 0]
            if edge:
                cur, nxt = edge[int(rng.integers(len(edge)))]
                pos, at = rs + nxt[3] - 1, nxt[2] - 1
                if nxt[0] == 1 and at + 1 + nxt[1] <= len(seq):
                    a = seq[at:at + 1 + nxt[1]]
                    out.append((pos, len(a), 1, a.encode()))
                else:
                    out.append((pos, 1, 1 + (nxt[1] if nxt[0] == 2 else 0), seq[at:at + 1].encode()))
                continue
        elif kind < 0.25:
            dl = [(rc, ln) for op, ln, _qc, rc in steps if op in REF_ONLY]
            if dl:
                pos = rs + dl[0][0] + int(rng.integers(dl[0][1]))
        elif kind < 0.30:
            pos = rs - 1 - int(rng.integers(3))
        elif kind < 0.35:
            pos = rs + rtot + int(rng.integers(3))
        if pos < 0:
            continue
        shape = rng.random()
        if shape < 0.45:                                    # SNV, often the read's own base so that some support the ALT
            at = anchor(ops, pos - rs)
            base = seq[at].upper() if at is not None and at < len(seq) and rng.random() < 0.7 else str(rng.choice(list("ACGT")))
            out.append((pos, 1, 1, base.encode()))
        elif shape < 0.70:                                  # insertion: the anchor base and up to 11 more, often the read's own
            m = int(rng.integers(2, 13))
            at = anchor(ops, pos - rs)
            if at is not None and at + m <= len(seq) and rng.random() < 0.7:
                a = seq[at:at + m]
            else:
                a = "".join(rng.choice(list("ACGT"), m))
            out.append((pos, m, 1, a.encode()))
        elif shape < 0.88:                                  # deletion
            at = anchor(ops, pos - rs)
            base = seq[at].upper() if at is not None and at < len(seq) else "A"
            out.append((pos, 1, int(rng.integers(2, 9)), base.encode()))
        elif shape < 0.93:
            out.append((pos, 1, 1, b""))                    # missing ALT
        elif shape < 0.97:
            out.append((pos, 0, 1, b"<DEL>"))               # symbolic: skipped
        else:
            out.append((pos, 2, 1, b"AN"))
        if equal_runs and rng.random() < 0.25 and len(out) < n:
            out.append((pos, 1, 1, str(rng.choice(list("ACGT"))).encode()))
    return out[:n]


def random_case(seed, n_reads=40, n_var=12, min_baseq=20, lo=20, hi=60, ragged=True):
    rng = np.random.default_rng(seed)
    reads = [random_read(rng, lo=lo, hi=hi, ragged=ragged) for _ in range(n_reads)]
    for i in rng.choice(n_reads, size=max(1, n_reads // 20), replace=False):
        reads[i] = reads[i][:2] + (-1,) + reads[i][3:]      # skipped reads
    return pack_case(reads, variants_for(rng, [r for r in reads if r[2] >= 0], n_var), min_baseq)
