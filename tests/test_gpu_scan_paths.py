"""The Module-3 scan (kdf_scan_reads / kdf_scan_reads_dev) at k <= 63 against the C oracle, path by path.

Every case draws its reads from a seed and crosses four dimensions: where the index comes from (a: load_filter +
count_filtered, b: add_pairs of an oracle dump with some counts set to 0 -- the production load, c: count, d: add_pairs
without counts, so every key is stored with 0 and nothing may hit), the sieve geometry (in LDS, in L2, saturated by one
or two bits per key so that the table must reject almost every survivor, or no sieve: force_path 1, the direct scan
kernel), a state change between two scans on the same engine, and the probe reads (the index's own reads, another
genome's, a mix with N / IUPAC / lower case and reads shorter than k, or many reads under 64 bp, so that one hit word
spans several reads).  Each scan is checked twice: kdf_scan_reads (bitmap + distinct per read) and kdf_scan_reads_dev
into a caller-sized device buffer whose stream ends with the last base of the last read."""
import numpy as np
import pytest

import kmer_truth as T
from test_gpu_parity_basic import rand_reads

pytestmark = pytest.mark.gpu

# (k, index source, sieve geometry, state change between the two scans, probe reads); every entry of every dimension
# appears at a narrow (k <= 32) and at a wide k.  Geometry: lds = default sizing at <= 65 536 keys; l2 = sieve_bits 32
# at > 16 384 keys; l2def = default sizing at > 65 536 keys; sat = sieve_bits 1 or 2 at tens of thousands of keys;
# direct = force_path 1.
CASES = [
    (1, "c", "lds", None, "mix"),
    (1, "d", "direct", None, "own"),
    (5, "a", "lds", "reset", "mix"),
    (5, "b", "direct", "add", "short"),
    (16, "b", "sat", None, "mix"),
    (16, "c", "l2", "count", "own"),
    (21, "c", "l2def", None, "other"),
    (21, "a", "sat", None, "own"),
    (31, "a", "l2", "reset", "other"),
    (31, "b", "lds", "reserve", "mix"),
    (31, "c", "direct", "count", "short"),
    (32, "d", "lds", "clear", "mix"),
    (32, "c", "sat", "add", "other"),
    (32, "c", "l2", "defer", "own"),
    (33, "a", "lds", None, "mix"),
    (33, "b", "sat", "count", "mix"),
    (33, "c", "direct", "reserve", "other"),
    (47, "c", "l2def", None, "mix"),
    (47, "d", "sat", None, "own"),
    (47, "a", "direct", "reset", "own"),
    (47, "b", "l2", "clear", "short"),
    (63, "a", "l2", None, "mix"),
    (63, "c", "lds", "defer", "mix"),
    (63, "d", "l2", "add", "mix"),
    (63, "c", "sat", "clear", "own"),
    (63, "b", "direct", "add", "other"),
]

N_READS = {"lds": 150, "direct": 150, "l2": 700, "l2def": 1400, "sat": 450}   # 150 bp reads; keys ~ reads x 120


def _genome(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _probe(rng, kind, k, own, G1, G2):
    other = rand_reads(rng, 120, max(1, k - 2), 200, n_frac=0.01, genome=G2)
    if kind == "own":
        return list(own)
    if kind == "other":
        return other
    if kind == "mix":
        g1 = "".join("ACGT"[c] for c in G1[:20000])
        out = list(own[: len(own) // 2]) + other[:60] + T.random_reads(rng, k, 60, g1, max_len=200)
        out += ["", "N" * (k + 2), "ACGT" * (k // 4 + 1)]
        return [out[i] for i in rng.permutation(len(out))]
    # many reads under 64 bp (one hit word spans several reads), shorter than k, of exactly k, from both genomes
    out = []
    for i in range(600):
        g = G1 if i % 3 else G2
        L = [max(0, k - 1), k, int(rng.integers(0, 64))][i % 3]
        s = int(rng.integers(0, len(g) - L))
        r = "".join("ACGT"[c] for c in g[s:s + L])
        out.append(r.lower() if i % 7 == 0 else r)
    return out


def _stream(reads):
    """The probe's stream, made so that the stream without its final separator has n_bases % 64 != 0."""
    from kmer_denovo_filter_amd import ReadStream
    st = ReadStream.from_strings(reads)
    if (st.n_bases - 1) % 64 == 0:
        reads = reads + ["ACG"]
        st = ReadStream.from_strings(reads)
    return reads, st


def check_scan(e, ot, reads, st, tag, expect_hits):
    """kdf_scan_reads and kdf_scan_reads_dev against the oracle's scan of the same reads."""
    import torch
    from kmer_denovo_filter_amd.reads import stream_words
    hits, distinct = e.scan(st)
    ohit, odist = ot.scan_reads(reads)
    per_read, off = [], 0
    for s in reads:
        per_read.append(np.nonzero(ohit[off:off + len(s)])[0])
        off += len(s)
    want = T.hit_words(st.offsets, per_read, len(hits))
    assert np.array_equal(hits, want), tag + f": hit bitmap ({int(np.unpackbits(hits.view(np.uint8)).sum())} bits, oracle {int(ohit.sum())})"
    assert np.array_equal(distinct, odist), tag + ": distinct per read"
    if expect_hits is not None:
        assert bool(ohit.any()) == expect_hits, tag + ": the case does not test what it means to"
    # scan_dev: the stream ends at the last base of the last read (its separator left out), n_bases % 64 != 0
    n = st.n_bases - 1
    pw, mw = stream_words(n)
    nt = (n + 63) // 64
    dp = torch.from_numpy(st.packed[:pw].view(np.int64).copy()).cuda()
    dm = torch.from_numpy(st.invalid[:mw].view(np.int64).copy()).cuda()
    dh = torch.full((mw,), -1, dtype=torch.int64, device="cuda")          # the engine must write every word it owns
    torch.cuda.synchronize()
    e.scan_dev(dp.data_ptr(), dm.data_ptr(), n, dh.data_ptr())
    e.synchronize()
    got = dh.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:nt], hits[:nt]), tag + ": scan_dev differs from scan"
    assert (got[nt:] == ~np.uint64(0)).all(), tag + ": scan_dev wrote past its tiles"
    assert n % 64 and int(got[nt - 1]) >> (n % 64) == 0, tag + ": a hit at or past n_bases"
    return hits


def run_case(O, k, src, geom, change, probe_kind, seed):
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    rng = np.random.default_rng(seed)
    tag = f"seed {seed}: k={k} src={src} geom={geom} change={change} probe={probe_kind}"
    wide = k > 32
    G1, G2 = _genome(rng, 200_000), _genome(rng, 200_000)
    idx_reads = rand_reads(rng, N_READS[geom], 100, 200, n_frac=0.005, genome=G1)
    more = rand_reads(rng, 150, 100, 200, n_frac=0.005, genome=G2)      # keys the index does not hold yet
    H = (lambda a: a if wide else None)
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        if geom == "direct":
            e.set_option("force_path", 1)
        elif geom == "l2":
            e.set_option("sieve_bits", 32)
        elif geom == "sat":
            e.set_option("sieve_bits", int(rng.choice([1, 2])))
        # ---- the index
        if src == "a":
            clo, chi, _ = O.OracleTable(k, 1 << 16).count_reads(idx_reads).export_ge(0)
            sel = rng.random(len(clo)) < 0.5
            flo, fhi = clo[sel], chi[sel]
            own = idx_reads[::2] + more[:20]
            e.load_filter(flo, H(fhi))
            e.count_filtered(ReadStream.from_strings(own))
            ot = O.OracleTable(k, 1 << 16).load_filter(flo, fhi).count_reads_filtered(own)
            nkeys = len(flo)
            assert np.array_equal(e.query(flo, H(fhi)), ot.query(flo, fhi)), tag + ": count --if"
            if probe_kind == "mix":
                own = idx_reads[1::2][:40] + own               # filter keys stored with count 0 (the mix takes own's first half)
        else:
            own = idx_reads
            lo, hi, cnt = O.OracleTable(k, 1 << 16).count_reads(idx_reads).export_ge(0)
            nkeys = len(lo)
            if src == "b":
                c2 = cnt.copy()
                c2[rng.random(len(c2)) < 0.3] = 0
                e.add_pairs(lo, H(hi), c2)
                pos = c2 > 0
                ot = O.OracleTable(k, 1 << 16).load_filter(lo[pos], hi[pos]).count_reads_filtered(idx_reads)
                assert np.array_equal(e.query(lo, H(hi)), c2), tag + ": add_pairs counts"
            elif src == "c":
                if change == "defer":
                    own = idx_reads[: len(idx_reads) // 2]
                e.count(ReadStream.from_strings(own))
                ot = O.OracleTable(k, 1 << 16).count_reads(own)
            else:
                e.add_pairs(lo, H(hi))
                ot = O.OracleTable(k, 1 << 16).load_filter(lo, hi)
        # the geometry holds what its name says
        if geom == "lds":
            assert nkeys <= 65536, tag
        elif geom == "l2":
            assert nkeys > 16384, tag
        elif geom == "l2def":
            assert nkeys > 65536, tag
        elif geom == "sat":
            assert nkeys > 20000, tag
        probe, st = _stream(_probe(rng, probe_kind, k, own, G1, G2))
        no_hit = src == "d"
        check_scan(e, ot, probe, st, tag + " (first scan)", False if no_hit else None)
        if change is None:
            return
        # ---- the state change, then the second scan
        mlo, mhi, mcnt = O.OracleTable(k, 1 << 16).count_reads(more).export_ge(0)
        if change == "add":                                   # new keys must hit: the sieve of the first scan is stale
            e.add_pairs(mlo, H(mhi), mcnt)
            ot.count_reads(more)
            probe, st = _stream(probe + more[:60])
            no_hit = False
        elif change == "count":
            e.count(ReadStream.from_strings(more))
            ot.count_reads(more)
            probe, st = _stream(probe + more[:60])
            no_hit = False
        elif change == "reserve":                             # a rehash: the same result
            cap0, distinct, _ = e.stats()
            e.reserve(4 * distinct)
            assert e.stats()[0] > cap0, tag + ": reserve did not rehash"
        elif change == "clear":                               # the old keys no longer hit
            e.clear()
            e.add_pairs(mlo, H(mhi), mcnt)
            ot = O.OracleTable(k, 1 << 16).count_reads(more)
            probe, st = _stream(probe + more[:60])
            no_hit = False
        elif change == "reset":                               # a filter table with every count 0: no hits
            e.reset_counts()
            ot = O.OracleTable(k, 1 << 16).load_filter(flo, fhi)
            no_hit = True
        elif change == "defer":                               # small batches still pending when the scan comes
            e.set_option("defer", 1)
            if geom == "l2":
                e.set_option("force_path", 2)                 # binned passes wait in the ring for kernel C
            rest = idx_reads[len(idx_reads) // 2:]
            for a in range(0, len(rest), 16):
                e.count(ReadStream.from_strings(rest[a:a + 16]))
            ot.count_reads(rest)
            assert e.get_stat("pending_positions") > 0 or e.get_stat("pending_passes") > 0, tag + ": nothing pending"
            probe, st = _stream(probe + rest[:40])
        check_scan(e, ot, probe, st, tag + " (second scan)", False if no_hit else None)
        if change == "defer":
            assert e.get_stat("pending_positions") == 0 and e.get_stat("pending_passes") == 0, tag


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"k{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}" for c in CASES])
def test_scan_path_matches_oracle(oracle, case):
    k, src, geom, change, probe = CASES[case]
    run_case(oracle, k, src, geom, change, probe, seed=9000 + case)
