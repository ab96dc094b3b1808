"""tests/stream_truth.py (the torch truth the full-size GPU cases are compared with) pinned on the CPU to the oracle's
plain-Python counter (``py_count`` through ``kmer_truth.count_truth``) and to the C ``OracleTable``, before anything
rests on it.  The streams are packed here, bit by bit from the strings by the layout of ``include/kdf.h``, not by
the package's packer."""
import numpy as np
import pytest
import torch

import kmer_truth as KT
import stream_truth as ST

KS = [1, 2, 5, 16, 31, 32, 33, 47, 63]
M64 = (1 << 64) - 1


def _i64(words):
    return torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64))


def pack(reads, garbage=None, pad_words=0):
    """Strings -> (packed, invalid, n_bases): every read is followed by one invalid separator position.  ``garbage``
    (an rng): every bit at or past n_bases -- the tail of the last words and ``pad_words`` extra words -- is random,
    in the packed AND in the mask words (so some of them read "valid")."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    codes, inv = [], []
    for r in reads:
        for ch in r.upper():
            codes.append(code.get(ch, 0)); inv.append(ch not in code)
        codes.append(0); inv.append(True)
    n = len(codes)
    pw, mw = (n + 31) // 32 + pad_words, (n + 63) // 64 + pad_words
    if garbage is None:
        P, M = [0] * pw, [M64] * mw
    else:
        P = [int(garbage.integers(0, 1 << 63)) * 2 + int(garbage.integers(0, 2)) for _ in range(pw)]
        M = [int(garbage.integers(0, 1 << 63)) * 2 + int(garbage.integers(0, 2)) for _ in range(mw)]
    for i in range(n):
        P[i >> 5] = (P[i >> 5] & ~(3 << (2 * (i & 31)))) | (codes[i] << (2 * (i & 31)))
        M[i >> 6] = (M[i >> 6] & ~(1 << (i & 63))) | (int(inv[i]) << (i & 63))
    return _i64(P), _i64(M), n


def as_dict(t):
    lo, hi, cnt = (x.tolist() for x in t[:3])
    keys = [((h & M64) << 64) | (l & M64) for l, h in zip(lo, hi)]
    assert keys == sorted(set(keys)), "truth keys are not ascending and distinct"
    return dict(zip(keys, cnt))


def edge_reads(rng, k):
    """The reads the issue names: N at the first and at the last base, reads shorter than k, of exactly k and k + 1,
    an all-N read, an empty one, lower case, and (even k) a reverse-complement palindrome."""
    genome = "".join(rng.choice(list("ACGT"), 1500))
    reads = []
    for _ in range(40):
        L = int(rng.integers(max(1, k - 2), k + 90))
        s = int(rng.integers(0, len(genome) - L))
        r = list(genome[s:s + L])
        if rng.random() < 0.5:
            r = [{"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(r)]
        for j in np.flatnonzero(rng.random(L) < 0.01):
            r[j] = "N"
        reads.append("".join(r))
    body = genome[100:100 + k + 20]
    reads += ["N" + body, body + "N", "N" + body + "N", body[:k], body[:k + 1], "N" * (k + 2), "", body.lower(), "A" * (k + 40)]
    if k > 1:
        reads += [body[:k - 1], "ACGT"[:min(k - 1, 4)]]
    if k % 2 == 0:
        half = genome[300:300 + k // 2]
        pal = half + "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(half))
        reads += [pal, "G" + pal + "T", pal]
    return reads


@pytest.mark.parametrize("k", KS)
def test_count_truth_equals_py_count_and_oracle_table(oracle, k):
    rng = np.random.default_rng(4200 + k)
    reads = edge_reads(rng, k)
    want = KT.count_truth(reads, k)
    packed, invalid, n = pack(reads)
    assert n % 64 != 0                                        # (the stream ends inside a mask word)
    t = ST.count_truth((packed, invalid, n), k)
    assert as_dict(t) == want
    assert t[3] == sum(want.values()) == oracle.count_windows(reads, k)
    assert t[2].dtype == torch.int64
    if k % 2 == 0:                                            # the palindrome was counted once per occurrence, as itself
        half = reads[-1][:k // 2]
        assert want[KT.key_int(reads[-1])] >= 3 and oracle.canonicalize(reads[-1]) == reads[-1] and half
    olo, ohi, ocnt = oracle.OracleTable(k).count_reads(reads).export_ge(0)
    assert np.array_equal(t[0].numpy().view(np.uint64), olo) and np.array_equal(t[1].numpy().view(np.uint64), ohi)
    assert np.array_equal(t[2].numpy(), ocnt.astype(np.int64))


@pytest.mark.parametrize("k", [5, 32, 33, 63])
def test_garbage_past_n_bases_is_never_read(k):
    """Padding words full of random bits, and random bits in the last words past n_bases: the same truth.  The stream
    is also cut in the middle of a read (n_bases smaller than what the words hold): the cut read ends there."""
    rng = np.random.default_rng(77 + k)
    reads = edge_reads(rng, k)
    clean = ST.count_truth(pack(reads), k)
    dirty = ST.count_truth(pack(reads, garbage=rng, pad_words=3), k)
    assert all(torch.equal(a, b) for a, b in zip(clean[:3], dirty[:3])) and clean[3] == dirty[3]
    long_read = "".join(rng.choice(list("ACGT"), k + 40))
    packed, invalid, n = pack(reads + [long_read, "ACG"], garbage=rng, pad_words=2)
    start = sum(len(r) + 1 for r in reads)
    for keep in (k - 1, k, k + 10):                           # the cut read keeps no window, one window, eleven
        cut = start + keep                                    # position `cut` holds a valid base of the same read
        head = reads + [long_read[:keep]]
        assert as_dict(ST.count_truth((packed, invalid, cut), k)) == KT.count_truth(head, k)
        assert ST.count_truth((packed, invalid, cut), k)[3] == clean[3] + max(keep - k + 1, 0)


@pytest.mark.parametrize("k", [2, 31, 33, 63])
@pytest.mark.parametrize("chunk", [1, 7, 64, 1000])
def test_chunk_boundaries(k, chunk):
    """Window starts formed ``chunk`` at a time: windows straddle every boundary (chunk < k too) and are formed once."""
    rng = np.random.default_rng(9 + k)
    reads = edge_reads(rng, k)[::3]
    st = pack(reads)
    whole, parts = ST.count_truth(st, k), ST.count_truth(st, k, chunk=chunk)
    assert all(torch.equal(a, b) for a, b in zip(whole[:3], parts[:3])) and whole[3] == parts[3]
    assert as_dict(parts) == KT.count_truth(reads, k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("S", [1, 3, 8])
def test_key_slices_partition_the_truth(k, S):
    rng = np.random.default_rng(500 + k)
    reads = edge_reads(rng, k) + ["".join(rng.choice(list("ACGT"), 400)) for _ in range(6)]
    st = pack(reads)
    whole = ST.count_truth(st, k)
    sl = ST.slice_of(whole[0], whole[1], k, S)
    assert int(sl.min()) >= 0 and int(sl.max()) < S and bool((sl[1:] >= sl[:-1]).all())      # ranges of the sorted keys
    # the slice is the key's top bits, whatever the words: the 2k-bit integer scaled to 16 bits
    for key, s in zip(as_dict(whole), sl.tolist()):
        top = key >> (2 * k - 16) if 2 * k >= 16 else key << (16 - 2 * k)
        assert s == top * S >> 16
    parts = [ST.count_truth(st, k, key_slice=(s, S)) for s in range(S)]
    assert all(p[3] == whole[3] for p in parts)
    for i in range(3):
        assert torch.equal(torch.cat([p[i] for p in parts]), whole[i])                      # in slice order = ascending
    for s in range(S):
        assert all(torch.equal(a, b) for a, b in zip(ST.take_slice(whole, k, s, S), parts[s][:3]))
    if S > 1 and k >= 5:
        assert sum(p[0].numel() > 0 for p in parts) > 1


@pytest.mark.parametrize("k", [5, 32, 47, 63])
def test_accumulate_and_filtered_truth_against_dicts(oracle, k):
    rng = np.random.default_rng(31 + k)
    batches = [edge_reads(rng, k) for _ in range(3)]
    batches[2] = batches[2] + batches[0][:10]                  # keys shared between batches
    truths = [ST.count_truth(pack(b), k) for b in batches]
    want = {}
    for b in batches:
        for key, c in KT.count_truth(b, k).items():
            want[key] = want.get(key, 0) + c
    acc = ST.accumulate(truths)
    assert as_dict(acc) == want and acc[2].dtype == torch.int64
    assert as_dict(ST.accumulate(truths[:1])) == as_dict(truths[0])
    # count --if: filter = every third key of batch 0 + absent keys + the extremes, in a shuffled order
    d0 = as_dict(truths[0])
    absent = [KT.key_int(oracle.canonicalize("".join(rng.choice(list("ACGT"), k)))) for _ in range(30)]
    filt = list(dict.fromkeys(list(d0)[::3] + absent + [0, min(d0), max(d0)]))
    rng.shuffle(filt)
    flo, fhi = _i64([v & M64 for v in filt]), _i64([v >> 64 for v in filt])
    parent = ST.count_truth(pack(batches[1]), k)
    got = ST.filtered_truth(parent, (flo, fhi)).tolist()
    pd = KT.count_truth(batches[1], k, filt)
    assert got == [pd[v] for v in filt] and 0 in got and max(got) > 0
    olo, ohi = np.array([v & M64 for v in filt], np.uint64), np.array([v >> 64 for v in filt], np.uint64)
    ot = oracle.OracleTable(k).load_filter(olo, ohi).count_reads_filtered(batches[1])
    assert np.array_equal(ot.query(olo, ohi).astype(np.int64), np.array(got))
    empty = ST.count_truth(pack(["N" * 5]), k)
    assert empty[0].numel() == 0 and empty[3] == 0 and ST.filtered_truth(empty, (flo, fhi)).tolist() == [0] * len(filt)
    # set helpers
    p = as_dict(parent)
    assert as_dict(ST.rows_ge(parent, 2)) == {a: c for a, c in p.items() if c >= 2}
    assert as_dict(ST.rows_le(parent, 1)) == {a: c for a, c in p.items() if c <= 1}
    mlo, mhi = ST.keys_minus((flo, fhi), parent)
    assert [((h & M64) << 64) | (l & M64) for l, h in zip(mlo.tolist(), mhi.tolist())] == [v for v in filt if v not in p]
    assert ST.member(parent[0], parent[1], flo, fhi).tolist() == [v in p for v in filt]
    assert ST.lower_bound(parent[0], parent[1], flo, fhi).tolist() == [sum(a < v for a in p) for v in filt]


def test_unsigned_order_at_the_word_edges():
    """k = 32 fills all 64 bits of lo and k = 33..63 compares hi, then unsigned lo: keys on both sides of the sign bit
    of lo, with equal and with different hi words, come out in unsigned 128-bit order."""
    for k, reads in ((32, ["T" * 32, "A" * 32, "G" + "A" * 31, "C" + "T" * 31, "A" + "T" * 31 + "G"]),
                     (33, ["A" * 33, "A" + "G" + "A" * 31, "A" + "C" + "T" * 31, "C" + "A" * 32, "C" + "G" + "A" * 31]),
                     (63, ["A" * 31 + "G" + "C" * 31, "A" * 31 + "C" + "C" * 31, "A" * 30 + "C" + "T" + "C" * 31])):
        t = ST.count_truth(pack(reads), k)
        assert as_dict(t) == KT.count_truth(reads, k)
        lo = t[0].tolist()
        assert min(lo) < 0 <= max(lo) or k == 63               # lo words on both sides of the sign bit
