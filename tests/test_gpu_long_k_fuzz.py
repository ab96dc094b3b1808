"""Seeded randomised parity for long k-mers (odd k 65..201), in the style of test_gpu_fuzz.test_random_cases_match_oracle.

The C oracle stops at k = 64, so the truth is the string rules of tests/kmer_truth.py (pinned to the oracle at k <= 63
by tests/test_kmer_truth.py).  Each case draws k over all 69 valid values (every W from 3 to 7 and the top-word widths 2
and 62 come up in the even cases of every seed), reads with N / IUPAC / lower case, reverse complements and high-copy
repeats, a table size from one slot up, and the way the reads are fed (one call, halves, small batches with reserves,
double-buffered uploads, device buffers, key-space slices); then checks the counted table (full and threshold dumps,
the device dump sorted and unsorted, stats, query with near keys), a merge of 2-4 engines' dumps into one table (two dumps
in one add_pairs call at least once per seed), count --if over 1-3 batches with a second parent, and the scan against
the counted, the merged and the filter table."""
import numpy as np
import pytest

import kmer_truth as T
from kmer_denovo_filter_amd.engine import key_words

pytestmark = pytest.mark.gpu

LONG_KS = list(range(65, 202, 2))                       # the 69 valid long k
FORCED = (65, 95, 97, 127, 129, 159, 161, 191, 193, 201)  # W = 3..7 at top-word widths 2 and 62 (201: the widest)


def _stream(reads):
    from kmer_denovo_filter_amd import ReadStream
    return ReadStream.from_strings(reads)


def _check_table(e, k, truth, tag):
    ks, cnt = T.sorted_items(truth)
    keys, hi, c = e.export_ge(0)
    assert hi is None and keys.shape == (len(ks), key_words(k)), tag + ": export shape"
    assert [T.int_of_row(r) for r in keys] == ks, tag + ": export_ge(0) keys"
    assert np.array_equal(c, cnt), tag + ": export_ge(0) counts"
    return ks, cnt


def _check_scan(e, k, probe, truth, tag):
    from kmer_denovo_filter_amd.reads import stream_words
    st = _stream(probe)
    hits, distinct = e.scan(st)
    want_pos, want_dist = T.scan_truth(probe, k, truth)
    assert np.array_equal(hits, T.hit_words(st.offsets, want_pos, stream_words(st.n_bases)[1])), tag + ": scan hits"
    assert np.array_equal(distinct, want_dist), tag + ": scan distinct"
    return sum(map(len, want_pos))


def long_k_case(O, rng, it, tag0, force_pair=False):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd._native import KdfError
    k = int(FORCED[(it // 2) % len(FORCED)]) if it % 2 == 0 else int(rng.choice(LONG_KS))   # 20+ cases: every FORCED k
    W = key_words(k)
    tb = 2 * k - 64 * (W - 1)                                       # bits of the top word
    genome = "".join(rng.choice(list("ACGT"), int(rng.integers(2000, 8000))))
    reads = T.random_reads(rng, k, int(rng.integers(8, 50)), genome, max_len=int(rng.integers(k + 1, 1001)))
    if force_pair:                                                  # one read at both ends: the merge's two parts share keys
        reads = [genome[:k + 20]] + reads + [genome[:k + 20]]
    hint = int(rng.choice([1, 1 << 6, 1 << 10, 1 << 14]))
    feed = str(rng.choice(["one", "halves", "small", "upload", "dev", "parts"]))
    tag = f"{tag0}: k={k} W={W} reads={len(reads)} hint={hint} feed={feed}"
    truth = T.count_truth(reads, k)

    def count_with(e, rs, how):
        if how == "one":
            e.count(_stream(rs))
        elif how == "halves":
            h = len(rs) // 2
            e.count(_stream(rs[:h]))
            if rng.random() < 0.5:
                e.reserve(int(rng.integers(1, 4 * len(truth) + 2)))
            e.count(_stream(rs[h:]))
        elif how == "small":
            step = int(rng.integers(1, 9))
            for a in range(0, len(rs), step):
                e.count(_stream(rs[a:a + step]))
                if rng.random() < 0.1:
                    e.reserve(int(rng.integers(1, 4 * len(truth) + 2)))
        elif how == "upload":                                       # double-buffered: slot i % 2
            nb = int(rng.integers(2, 6))
            sts = [_stream(rs[a::nb]) for a in range(nb)]
            e.upload_async(0, sts[0])
            for i in range(nb):
                if i + 1 < nb:
                    e.upload_async((i + 1) % 2, sts[i + 1])
                e.count_uploaded(i % 2)
        else:                                                       # "dev": torch buffers sized by stream_words
            from kmer_denovo_filter_amd.reads import stream_words
            nb = int(rng.integers(1, 4))
            keep = []
            for a in range(nb):
                st = _stream(rs[a::nb])
                pw, mw = stream_words(st.n_bases)
                dp = torch.from_numpy(st.packed[:pw].view(np.int64).copy()).cuda()
                dm = torch.from_numpy(st.invalid[:mw].view(np.int64).copy()).cuda()
                keep.append((dp, dm))
                torch.cuda.synchronize()
                e.count_dev(dp.data_ptr(), dm.data_ptr(), st.n_bases)
            e.synchronize()

    # ---- the counted table
    with KmerEngine(k, capacity_hint=hint) as e:
        if feed == "parts":                                         # key-space slices, cleared in between: union == whole
            parts = int(rng.integers(2, 5))
            e.set_option("key_parts", parts)
            got = {}
            for p in range(parts):
                e.clear()
                e.set_option("key_part", p)
                count_with(e, reads, str(rng.choice(["one", "halves", "small"])))
                keys, _, c = e.export_ge(0)
                for r, x in zip(keys, c):
                    v = T.int_of_row(r)
                    assert v not in got, tag + f": slice {p} repeats a key"
                    got[v] = int(x)
            assert got == truth, tag + f": union of {parts} slices"
            e.set_option("key_parts", 0)
            e.clear()
            count_with(e, reads, "one")
        else:
            count_with(e, reads, feed)
        ks, cnt = _check_table(e, k, truth, tag)
        cap, distinct, windows = e.stats()
        assert distinct == len(ks) and windows == int(cnt.sum()) and cap >= len(ks), tag + f": stats {cap, distinct, windows}"
        t = int(rng.integers(1, 6))
        assert e.count_ge(t) == int((cnt >= t).sum()), tag + f": count_ge({t})"
        kt, _, ct = e.export_ge(t)
        assert [T.int_of_row(r) for r in kt] == [v for v, c in zip(ks, cnt) if c >= t] and np.array_equal(ct, cnt[cnt >= t]), tag + f": export_ge({t})"
        n = int((cnt >= t).sum())
        if n:
            for srt in (True, False):
                dk = torch.zeros((n, W), dtype=torch.int64, device="cuda")
                dc = torch.zeros(n, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                assert e.export_ge_dev(t, dk.data_ptr(), None, dc.data_ptr(), n, sorted_=srt) == n, tag
                pairs = list(zip([T.int_of_row(r) for r in dk.cpu().numpy().view(np.uint64)], dc.cpu().numpy().view(np.uint32).tolist()))
                want = [(v, int(c)) for v, c in zip(ks, cnt) if c >= t]
                assert (pairs if srt else sorted(pairs)) == want, tag + f": export_ge_dev({t}, sorted={srt})"
        # query: present, absent, and keys one bit away in the top word or in word 0, shuffled
        sel = [ks[i] for i in rng.choice(len(ks), size=min(len(ks), 200), replace=False)] if ks else []
        near = [v ^ (1 << (64 * (W - 1) + int(rng.integers(0, tb)))) for v in sel] + [v ^ (1 << int(rng.integers(0, 64))) for v in sel]
        absent = [T.key_int(O.canonicalize("".join(rng.choice(list("ACGT"), k)))) for _ in range(30)]
        q = sel + near + absent
        q = [q[i] for i in rng.permutation(len(q))]
        assert np.array_equal(e.query(T.rows(q, W)), np.array([truth.get(v, 0) for v in q], np.uint32)), tag + ": query"
        # scan against the counted table
        other = T.random_reads(rng, k, 12, max_len=int(rng.integers(k, 600)))
        probe = [reads[i] for i in rng.permutation(len(reads))[: max(1, len(reads) // 2)]] + other + ["", "N" * k, reads[0][: k - 1]]
        nhit = _check_scan(e, k, probe, truth, tag + " (counted)")

    # ---- merge: 2-4 engines' dumps add_pairs-ed into one table, fresh or holding a counted first part
    m = 2 if force_pair else int(rng.integers(2, 5))
    cut = [int(rng.integers(1, len(reads)))] if force_pair else sorted(rng.integers(0, len(reads) + 1, m - 1).tolist())
    parts = [reads[a:b] for a, b in zip([0] + cut, cut + [len(reads)])]
    pre = not force_pair and rng.random() < 0.4
    dumps = []
    for pr in (parts[1:] if pre else parts):
        with KmerEngine(k, capacity_hint=int(rng.choice([1, 1 << 8]))) as pe:
            pe.count(_stream(pr))
            keys, _, c = pe.export_ge(0)
            dumps.append((keys, c))
    paired = len(dumps) >= 2 and (force_pair or rng.random() < 0.5)
    with KmerEngine(k, capacity_hint=int(rng.choice([1, 1 << 6, 1 << 12]))) as me:
        if pre:
            me.count(_stream(parts[0]))
        calls = [(np.concatenate([dumps[0][0], dumps[1][0]]), np.concatenate([dumps[0][1], dumps[1][1]]))] + dumps[2:] if paired else dumps
        twice = len(calls[0][0]) - len(np.unique(calls[0][0].reshape(-1, W), axis=0)) if paired else 0
        for keys, c in calls:
            me.add_pairs(keys.reshape(-1, W), None, c)              # same key twice in one launch when paired
        _check_table(me, k, truth, tag + f" merge m={m} pre={pre} paired={paired}")
        # keys the probe meets, stored with count 0: they must not hit
        pk = [v for v in T.count_truth(other, k) if v not in truth][:50]
        if pk:
            me.add_pairs(T.rows(pk, W))
            assert not me.query(T.rows(pk, W)).any(), tag + ": add_pairs without counts"
        _check_scan(me, k, probe, truth, tag + f" (merged, {len(pk)} count-0 keys)")

    # ---- count --if: a subset of the keys plus absent ones, 1-3 batches, then a second parent
    if not ks:
        return twice, nhit
    sub = [ks[i] for i in rng.choice(len(ks), size=min(len(ks), int(rng.integers(1, 1500))), replace=False)]
    filt = sorted(set(sub) | set(absent[:10]))
    with KmerEngine(k, capacity_hint=int(rng.choice([1, 1 << 10]))) as fe:
        fe.load_filter(T.rows(filt, W))
        for pi in range(2):
            if pi:
                fe.reset_counts()
            parent = T.random_reads(rng, k, int(rng.integers(5, 30)), genome, max_len=600) + reads[pi::3]
            nb = int(rng.integers(1, 4))
            for a in range(nb):
                fe.count_filtered(_stream(parent[a::nb]))
            ft = T.count_truth(parent, k, filt)
            ptag = tag + f" filter={len(filt)} parent {pi} batches={nb}"
            assert np.array_equal(fe.query(T.rows(filt, W)), np.array([ft[v] for v in filt], np.uint32)), ptag + ": query"
            _check_table(fe, k, ft, ptag)                           # zeros included
            _check_scan(fe, k, probe + parent[:5], ft, ptag + " (filter table)")
        with pytest.raises(KdfError):
            fe.count(_stream(reads[:2]))                            # a filter is loaded: insert mode is refused
    return twice, nhit


def run_cases(O, seed, n_cases):
    rng = np.random.default_rng(seed)
    twice, nhit = 0, 0
    for it in range(n_cases):
        t, h = long_k_case(O, rng, it, f"seed {seed} case {it}", force_pair=(it == 0))
        twice, nhit = twice + t, nhit + h
    assert twice > 0, f"seed {seed}: no add_pairs call held the same key twice"
    assert nhit > 0, f"seed {seed}: no scan hit in {n_cases} cases"


@pytest.mark.parametrize("seed", [611, 622, 633])
def test_long_k_random_cases(oracle, seed):
    run_cases(oracle, seed, 24)
