"""Long k-mers (odd k 65..201) through the membership sieve: option ``long_sieve`` / env KDF_LONG_SIEVE.

Truth is twofold and every comparison is exact: ``oracle.py_count`` (the string rules, any k) for counts, windows and
hit positions, and the SAME engine with ``long_sieve`` 0 -- the direct long kernels -- for hit words and distinct
counts.  The stats ``last_count_path`` / ``last_scan_path`` (3: sieve, 0: direct) and ``last_sieve_in_lds`` prove which
kernel and which form of it answered."""
import os

import numpy as np
import pytest

from kmer_denovo_filter_amd import KmerEngine, ReadStream, hit_positions
from kmer_denovo_filter_amd._native import KdfError
from test_gpu_long_k import int_of_row, mixed_reads, rows_of
from test_gpu_parity_basic import rand_reads

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------

def l2_bits(n_keys):
    """sieve_bits that put the sieve of n_keys keys past the 8192 words (64 KB) the LDS form takes"""
    return (1 << 20) // max(n_keys, 1) + 32


def genome(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def kmers_of(O, reads, k):
    """the canonical k-mers of the reads, in a fixed order"""
    return sorted(O.py_count(reads, k))


def n_windows(O, reads, k):
    return sum(O.py_count(reads, k).values())


def truth_counts(O, reads, k, kmers):
    d = O.py_count(reads, k, set(kmers))
    return np.array([d[c] for c in kmers], np.uint32)


def py_hits(O, probe, k, present):
    """per read: (window starts whose canonical k-mer is in `present`, number of distinct such k-mers)"""
    out = []
    for s in probe:
        S = s.upper()
        pos, seen = [], set()
        for i in range(len(S) - k + 1):
            w = S[i:i + k]
            if all(ch in "ACGT" for ch in w):
                c = O.canonicalize(w)
                if c in present:
                    pos.append(i)
                    seen.add(c)
        out.append((pos, len(seen)))
    return out


def check_py_hits(O, st, probe, k, present, hits, distinct, tag):
    for r, (pos, nd) in enumerate(py_hits(O, probe, k, present)):
        got = hit_positions(hits, int(st.offsets[r]), int(st.offsets[r + 1])).tolist()
        assert got == pos, f"{tag}: hits of read {r}"
        assert int(distinct[r]) == nd, f"{tag}: distinct of read {r}"


def count_if(e, st, rows, long_sieve, form=None, tag=""):
    """reset_counts, one count --if of st with the option at long_sieve -> (counts of rows, windows)"""
    e.set_option("long_sieve", long_sieve)
    e.reset_counts()
    e.count_filtered(st)
    assert e.get_stat("last_count_path") == (3 if long_sieve else 0), tag
    if long_sieve and form is not None:
        assert e.get_stat("last_sieve_in_lds") == form, tag + ": form"
    return e.query(rows), e.stats()[2]


def scan_both(e, st, form=None, tag=""):
    """the scan of st by the direct kernel and through the sieve (rebuilt from the table): equal, bit for bit"""
    e.set_option("long_sieve", 0)
    h0, d0 = e.scan(st)
    assert e.get_stat("last_scan_path") == 0, tag
    e.set_option("long_sieve", 1)
    h1, d1 = e.scan(st)
    assert e.get_stat("last_scan_path") == 3, tag
    if form is not None:
        assert e.get_stat("last_sieve_in_lds") == form, tag + ": form"
    assert np.array_equal(h0, h1), tag + ": hit words"
    assert np.array_equal(d0, d1), tag + ": distinct per read"
    return h1, d1


# ---------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------

def test_option_and_path_stats(oracle):
    k = 101
    rng = np.random.default_rng(1)
    G = genome(rng, 50_000)
    reads = rand_reads(rng, 200, 150, 150, n_frac=0.002, genome=G)
    kmers = kmers_of(oracle, reads[::2], k)
    rows = rows_of(kmers, k, oracle)
    st = ReadStream.from_strings(reads)
    with KmerEngine(31) as e:
        for v in (0, 1):
            with pytest.raises(KdfError):
                e.set_option("long_sieve", v)
        assert e.get_stat("long_sieve") == 0
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        assert e.get_stat("long_sieve") == 0                      # the default
        e.load_filter(rows)
        e.count_filtered(st)
        e.scan(st)
        assert e.get_stat("last_count_path") == 0 and e.get_stat("last_scan_path") == 0
        direct = e.query(rows)
        with pytest.raises(KdfError):
            e.set_option("long_sieve", 2)
        e.set_option("long_sieve", 1)                             # after the filter was loaded: built from the table
        assert e.get_stat("long_sieve") == 1
        e.reset_counts()
        e.count_filtered(st)
        e.scan(st)
        assert e.get_stat("last_count_path") == 3 and e.get_stat("last_scan_path") == 3
        assert np.array_equal(e.query(rows), direct)
        assert np.array_equal(direct, truth_counts(oracle, reads, k, kmers))
        for fp in (2, 4):                                         # still refused for long engines
            with pytest.raises(KdfError):
                e.set_option("force_path", fp)
        e.set_option("force_path", 1)                             # the direct kernels, whatever the option says
        e.count_filtered(st)
        e.scan(st)
        assert e.get_stat("last_count_path") == 0 and e.get_stat("last_scan_path") == 0
        e.set_option("force_path", 0)
        e.set_option("long_sieve", 0)
        e.count_filtered(st)
        e.scan(st)
        assert e.get_stat("last_count_path") == 0 and e.get_stat("last_scan_path") == 0


# ---------------------------------------------------------------------------------------------------------------------
# every W, both ends of the top word
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (65, 95, 97, 129, 161, 201))
def test_every_width_counts_and_hits(k, oracle):
    rng = np.random.default_rng(100 + k)
    reads = mixed_reads(rng, k)
    foreign = mixed_reads(rng, k, 24)                              # another genome
    own = kmers_of(oracle, reads, k)
    filt = [c for c in own if rng.random() < 0.5] + kmers_of(oracle, foreign, k)
    filt = [filt[i] for i in rng.permutation(len(filt))]
    rows = rows_of(filt, k, oracle)
    st = ReadStream.from_strings(reads)
    want = truth_counts(oracle, reads, k, filt)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        e.set_option("long_sieve", 1)                              # before the filter: built by load_filter
        e.load_filter(rows)
        e.count_filtered(st)
        assert e.get_stat("last_count_path") == 3 and e.get_stat("last_sieve_in_lds") == 1
        assert np.array_equal(e.query(rows), want)
        _, distinct, windows = e.stats()
        assert distinct == len(filt) and windows == n_windows(oracle, reads, k)
        keys, _, cnt = e.export_ge(0)
        order = sorted(range(len(filt)), key=lambda i: int_of_row(rows[i]))
        assert np.array_equal(keys, rows[order]) and np.array_equal(cnt, want[order])
        got1, win1 = count_if(e, st, rows, 1, form=1, tag=f"k={k}")
        got0, win0 = count_if(e, st, rows, 0, tag=f"k={k}")
        assert np.array_equal(got0, want) and np.array_equal(got1, want) and win0 == win1 == windows
        # the scan of the counted filter: hits are the filter keys the reads hold
        probe = foreign[:8] + reads[:40] + mixed_reads(rng, k, 12)
        pst = ReadStream.from_strings(probe)
        hits, dist = scan_both(e, pst, form=1, tag=f"k={k}")
        present = {c for c, v in zip(filt, want) if v}
        check_py_hits(oracle, pst, probe, k, present, hits, dist, f"k={k}")


# ---------------------------------------------------------------------------------------------------------------------
# both forms, a saturated sieve
# ---------------------------------------------------------------------------------------------------------------------

FORMS = {                   # reads of the filter (150 bp, ~50 keys each at k = 101), sieve_bits, in LDS
    "lds": (300, 0, 1),
    "l2": (400, 32, 0),
    "l2def": (1400, 0, 0),
    "sat1": (450, 1, 1),
    "sat2": (450, 2, 1),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_forms_and_saturated_sieve(form, oracle):
    k = 101
    n_idx, bits, in_lds = FORMS[form]
    rng = np.random.default_rng(sum(map(ord, form)))
    G1, G2 = genome(rng, 2_000_000), genome(rng, 200_000)
    idx = rand_reads(rng, n_idx, 150, 150, n_frac=0.0, genome=G1)
    filt = kmers_of(oracle, idx, k)
    if form == "lds":
        assert len(filt) <= 65536
    elif form == "l2":
        assert len(filt) > 16384
    elif form == "l2def":
        assert len(filt) > 65536
    else:
        assert len(filt) > 20000
    rows = rows_of(filt, k, oracle)
    other = rand_reads(rng, 300, 100, 200, n_frac=0.005, genome=G2)
    probe = other if form.startswith("sat") else other[:150] + idx[::7]
    st = ReadStream.from_strings(probe)
    want = truth_counts(oracle, probe, k, filt)
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        if bits:
            e.set_option("sieve_bits", bits)
        e.set_option("long_sieve", 1)
        e.load_filter(rows)
        got1, win1 = count_if(e, st, rows, 1, form=in_lds, tag=form)
        got0, win0 = count_if(e, st, rows, 0, tag=form)
        assert np.array_equal(got1, want) and np.array_equal(got0, want), form
        assert win0 == win1 == n_windows(oracle, probe, k), form
        if form.startswith("sat"):
            assert not want.any()                                  # the table rejects every survivor
        count_if(e, ReadStream.from_strings(idx[::3]), rows, 1, form=in_lds, tag=form)    # counts to scan for
        hits, _ = scan_both(e, st, form=in_lds, tag=form)
        assert bool(hits.any()) == (not form.startswith("sat")), form


# ---------------------------------------------------------------------------------------------------------------------
# survivor-path boundaries
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ("all", "one", "few", "ragged", "empty"))
def test_survivor_boundaries(case, oracle):
    k = 101
    rng = np.random.default_rng(sum(map(ord, case)))
    G = genome(rng, 300_000)
    n_reads = {"ragged": 1400}.get(case, 300)
    probe = rand_reads(rng, n_reads, 150, 150, n_frac=0.002, genome=G)
    if case == "empty":
        filt, probe = kmers_of(oracle, probe[:20], k), []
    elif case == "all":
        filt = kmers_of(oracle, probe, k)                          # every valid window survives
    elif case == "one":
        filt = kmers_of(oracle, [probe[150][20:20 + k]], k)
    elif case == "few":
        filt = kmers_of(oracle, [probe[7][:k + 11], probe[290][30:30 + k + 17]], k)      # 30 hits (and hardly a false survivor: 30 keys in 2^16 bits)
        assert len(filt) < 64
    else:
        filt = kmers_of(oracle, probe[::50], k)
    rows = rows_of(filt, k, oracle)
    st = ReadStream.from_strings(probe)
    if case == "ragged":                                           # neither form's workgroup divides the tiles
        n_tiles = (st.n_bases + 63) // 64
        assert n_tiles > 2048 and n_tiles % 256 and n_tiles % 512
    want = truth_counts(oracle, probe, k, filt)
    for form, bits in ((1, 0), (0, l2_bits(len(filt)))):
        with KmerEngine(k, capacity_hint=1 << 10) as e:
            e.set_option("sieve_bits", bits)
            e.set_option("long_sieve", 1)
            e.load_filter(rows)
            tag = f"{case} form {form}"
            if case == "empty":
                e.count_filtered(st)
                hits, dist = e.scan(st)
                assert e.stats()[2] == 0 and not e.query(rows).any() and not hits.any() and len(dist) == 0, tag
                continue
            got1, win1 = count_if(e, st, rows, 1, form=form, tag=tag)
            got0, win0 = count_if(e, st, rows, 0, tag=tag)
            assert np.array_equal(got1, want) and np.array_equal(got0, want), tag
            assert win1 == win0 == n_windows(oracle, probe, k), tag
            hits, dist = scan_both(e, st, form=form, tag=tag)
            assert int(np.unpackbits(hits.view(np.uint8)).sum()) == int(want.sum()), tag


# ---------------------------------------------------------------------------------------------------------------------
# the LDS form's tile loop: several rounds per thread, the last one partly past the stream
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (101, 201))
def test_lds_form_several_rounds(k, oracle):
    """debug_flags 8192 caps the LDS form's grid at two workgroups (1024 tiles a round), so a stream of a few thousand
    tiles takes several rounds and ends inside one: hits, validity and keys of a round must not leak into the next,
    and the windows of all rounds add up."""
    rng = np.random.default_rng(k + 5)
    G = genome(rng, 300_000)
    L = k + 49
    probe = rand_reads(rng, 1400 * 150 // L, L, L, n_frac=0.002, genome=G)
    filt = kmers_of(oracle, probe[::9], k)
    rows = rows_of(filt, k, oracle)
    st = ReadStream.from_strings(probe)
    n_tiles = (st.n_bases + 63) // 64
    assert n_tiles > 3 * 1024 and n_tiles % 1024
    want = truth_counts(oracle, probe, k, filt)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        e.set_option("debug_flags", 8192)
        e.set_option("long_sieve", 1)
        e.load_filter(rows)
        got1, win1 = count_if(e, st, rows, 1, form=1, tag=f"k={k}")
        assert e.get_stat("last_sieve_rounds") == (n_tiles + 1023) // 1024
        got0, win0 = count_if(e, st, rows, 0, tag=f"k={k}")
        assert np.array_equal(got1, want) and np.array_equal(got0, want)
        assert win1 == win0 == n_windows(oracle, probe, k)
        count_if(e, ReadStream.from_strings(probe[::2]), rows, 1, form=1)          # counts to scan for: not every key hits
        hits, dist = scan_both(e, st, form=1, tag=f"k={k}")
        assert e.get_stat("last_sieve_rounds") == (n_tiles + 1023) // 1024
        present = set(oracle.py_count(probe[::2], k)) & set(filt)
        check_py_hits(oracle, st, probe, k, present, hits, dist, f"k={k}")


def test_lds_form_rounds_at_full_grid():
    """A device-resident stream of 60 M positions: more tiles than the device holds threads of the LDS form, so the grid
    is the full one and every thread walks at least two tiles.  Truth: the direct kernels on the same engine."""
    import torch
    from kmer_denovo_filter_amd.reads import stream_words
    from kmer_denovo_filter_amd.synth import synth_stream
    k = 101
    ds = synth_stream(400_000, 150, genome_len=2_000_000, seed=5, device="cuda:0")
    torch.cuda.synchronize()
    P, M, N = ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases
    with KmerEngine(k, capacity_hint=1 << 12) as e0:                # the filter: the k-mers of the first 40 reads
        e0.count_dev(P, M, 40 * 151)
        rows, _, _ = e0.export_ge(0)
    assert 1000 < len(rows) <= 2000
    _, mw = stream_words(N)
    out = {}
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        e.load_filter(rows)
        for ls in (1, 0):
            e.set_option("long_sieve", ls)
            e.reset_counts()
            e.count_filtered_dev(P, M, N)
            assert e.get_stat("last_count_path") == (3 if ls else 0)
            if ls:
                assert e.get_stat("last_sieve_in_lds") == 1 and e.get_stat("last_sieve_rounds") >= 2
            cnt, windows = e.query(rows), e.stats()[2]
            dh = torch.full((mw,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            e.scan_dev(P, M, N, dh.data_ptr())
            e.synchronize()
            assert e.get_stat("last_scan_path") == (3 if ls else 0)
            if ls:
                assert e.get_stat("last_sieve_in_lds") == 1 and e.get_stat("last_sieve_rounds") >= 2
            out[ls] = cnt, windows, dh.cpu().numpy()
    assert np.array_equal(out[1][0], out[0][0]) and out[1][1] == out[0][1] > 0
    assert np.array_equal(out[1][2], out[0][2])
    assert out[1][0].min() >= 1 and int(out[1][0].sum()) > 3 * len(rows)         # hits all along the stream (every k-mer ~10 times)
    nt = (N + 63) // 64
    assert (out[1][2][nt:] == -1).all() and (out[1][2][nt // 2:nt] != 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# index sources of the scan, staleness
# ---------------------------------------------------------------------------------------------------------------------

def _index(O, e, src, rng, k, idx_reads):
    """load the index of the scan -> the set of canonical k-mers stored with count > 0"""
    d = O.py_count(idx_reads, k)
    kmers = sorted(d)
    rows = rows_of(kmers, k, O)
    cnt = np.array([d[c] for c in kmers], np.uint32)
    if src == "a":
        sel = rng.random(len(kmers)) < 0.5
        filt = [c for c, s in zip(kmers, sel) if s]
        e.load_filter(rows[sel])
        own = idx_reads[::2]
        e.count_filtered(ReadStream.from_strings(own))
        t = O.py_count(own, k, set(filt))
        return {c for c in filt if t[c]}
    if src == "b":
        c2 = cnt.copy()
        c2[rng.random(len(c2)) < 0.3] = 0
        e.add_pairs(rows, None, c2)
        return {c for c, v in zip(kmers, c2) if v}
    if src == "c":
        e.count(ReadStream.from_strings(idx_reads))
        return set(kmers)
    e.add_pairs(rows)                                              # d: every key with count 0
    return set()


@pytest.mark.parametrize("src", ("a", "b", "c", "d"))
def test_scan_index_sources(src, oracle):
    k = 101
    rng = np.random.default_rng(ord(src))
    G1, G2 = genome(rng, 100_000), genome(rng, 100_000)
    idx_reads = rand_reads(rng, 200, 120, 200, n_frac=0.003, genome=G1)
    probe = idx_reads[::3] + rand_reads(rng, 100, k - 2, 200, n_frac=0.01, genome=G2) + ["", "N" * (k + 2)]
    st = ReadStream.from_strings(probe)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        e.set_option("long_sieve", 1)
        present = _index(oracle, e, src, rng, k, idx_reads)
        hits, dist = e.scan(st)                                    # first use: the sieve comes from the table (b, c, d) or the filter (a)
        assert e.get_stat("last_scan_path") == 3
        check_py_hits(oracle, st, probe, k, present, hits, dist, src)
        assert bool(hits.any()) == (src != "d")
        h2, d2 = scan_both(e, st, tag=src)
        assert np.array_equal(h2, hits) and np.array_equal(d2, dist)


@pytest.mark.parametrize("change", ("add", "count", "reset", "reserve", "clear", "toggle"))
def test_scan_after_state_change(change, oracle):
    k = 101
    rng = np.random.default_rng(sum(map(ord, change)))
    G1, G2 = genome(rng, 100_000), genome(rng, 100_000)
    idx_reads = rand_reads(rng, 200, 120, 200, n_frac=0.003, genome=G1)
    more = rand_reads(rng, 120, 120, 200, n_frac=0.003, genome=G2)          # keys the index does not hold yet
    probe = idx_reads[::3] + more[:60]
    st = ReadStream.from_strings(probe)
    d = oracle.py_count(idx_reads, k)
    md = oracle.py_count(more, k)
    mk = sorted(md)
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        e.set_option("long_sieve", 1)
        if change == "reset":
            kmers = sorted(d)
            e.load_filter(rows_of(kmers, k, oracle))
            e.count_filtered(ReadStream.from_strings(idx_reads))
        else:
            e.count(ReadStream.from_strings(idx_reads))
        present = set(d)
        hits, dist = e.scan(st)
        assert e.get_stat("last_scan_path") == 3
        check_py_hits(oracle, st, probe, k, present, hits, dist, change + " (first scan)")
        if change == "add":                                       # the new keys must hit: the first scan's sieve is stale
            e.add_pairs(rows_of(mk, k, oracle), None, np.array([md[c] for c in mk], np.uint32))
            present |= set(mk)
        elif change == "count":
            e.count(ReadStream.from_strings(more))
            present |= set(mk)
        elif change == "reset":                                   # every count 0: nothing hits
            e.reset_counts()
            present = set()
        elif change == "reserve":                                 # a rehash keeps the stored forms, and the sieve
            cap0, distinct, _ = e.stats()
            e.reserve(4 * distinct)
            assert e.stats()[0] > cap0
        elif change == "clear":                                   # the old keys no longer hit
            e.clear()
            e.add_pairs(rows_of(mk, k, oracle), None, np.array([md[c] for c in mk], np.uint32))
            present = set(mk)
        else:
            e.set_option("long_sieve", 0)
            e.count(ReadStream.from_strings(more))                # keys join while there is no sieve
            present |= set(mk)
            e.set_option("long_sieve", 1)
        hits, dist = e.scan(st)
        assert e.get_stat("last_scan_path") == 3
        check_py_hits(oracle, st, probe, k, present, hits, dist, change + " (second scan)")
        h2, _ = scan_both(e, st, tag=change)                      # ... and the direct kernel's mask on the same state
        assert np.array_equal(h2, hits)


# ---------------------------------------------------------------------------------------------------------------------
# the end of the stream
# ---------------------------------------------------------------------------------------------------------------------

def _dirty(reads, rng):
    """(packed, mask, n, codes): the stream of the reads without its last separator in exactly kdf_stream_words(n)
    words, every position at or past n a VALID random base"""
    c = np.concatenate([np.frombuffer((r + "N").encode(), np.uint8) for r in reads])     # one separator after every read
    inv = c == ord("N")
    codes = np.select([c == ord(x) for x in "CGT"], [1, 2, 3], 0)
    n = len(codes) - 1
    T = (n + 63) // 64
    pw, mw = 2 * T + 4, T + 2
    P = pw * 32
    c = rng.integers(0, 4, P).astype(np.uint64)
    m = np.zeros(P, bool)
    c[:n] = codes[:n]
    m[:n] = inv[:n]
    packed = np.bitwise_or.reduce(c.reshape(pw, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1)
    mask = np.packbits(m, bitorder="little").view(np.uint64)
    return packed, mask, n, c


@pytest.mark.parametrize("k", (101, 201))
@pytest.mark.parametrize("rem", (0, 1, 63))
def test_dirty_words_past_n_bases(k, rem, oracle):
    import torch
    from kmer_denovo_filter_amd.reads import stream_words
    rng = np.random.default_rng(k * 64 + rem)
    G = genome(rng, 100_000)
    reads = [r.upper() for r in rand_reads(rng, 40, k + 20, k + 120, n_frac=0.0, genome=G)]
    used = sum(len(r) + 1 for r in reads)
    L = k + 5 + (rem - (used + k + 5)) % 64                         # the last read ends on the stream's last base
    s0 = int(rng.integers(0, len(G) - L))
    reads.append("".join("ACGT"[c] for c in G[s0:s0 + L]))
    packed, mask, n, c = _dirty(reads, rng)
    assert n % 64 == rem and (len(packed), len(mask)) == stream_words(n)
    # the filter / index holds what a kernel that trusts the words at and past n_bases would find there
    tail = "".join("ACGT"[int(x)] for x in c[n - k + 1:])
    phantom = kmers_of(oracle, [tail], k)
    own = kmers_of(oracle, reads, k)
    assert len(phantom) >= 64 and not set(phantom) & set(own)
    filt = own[::2] + phantom
    rows = rows_of(filt, k, oracle)
    want = truth_counts(oracle, reads, k, filt)
    dp = torch.from_numpy(packed.view(np.int64).copy()).cuda()
    dm = torch.from_numpy(mask.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    nt = (n + 63) // 64
    for form, bits in ((1, 0), (0, l2_bits(len(filt)))):
        tag = f"k={k} rem={rem} form {form}"
        with KmerEngine(k, capacity_hint=1 << 10) as e:
            e.set_option("sieve_bits", bits)
            e.set_option("long_sieve", 1)
            e.load_filter(rows)
            e.count_filtered_dev(dp.data_ptr(), dm.data_ptr(), n)
            assert e.get_stat("last_count_path") == 3 and e.get_stat("last_sieve_in_lds") == form, tag
            assert np.array_equal(e.query(rows), want), tag + ": count --if"
            assert e.stats()[2] == n_windows(oracle, reads, k), tag + ": windows"
        with KmerEngine(k, capacity_hint=1 << 10) as e:
            e.set_option("sieve_bits", bits)
            e.set_option("long_sieve", 1)
            e.add_pairs(rows, None, np.ones(len(rows), np.uint32))           # the phantom keys too are stored with a count
            masks = []
            for ls in (1, 0):
                e.set_option("long_sieve", ls)
                dh = torch.full((len(mask),), -1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                e.scan_dev(dp.data_ptr(), dm.data_ptr(), n, dh.data_ptr())
                e.synchronize()
                assert e.get_stat("last_scan_path") == (3 if ls else 0), tag
                if ls:
                    assert e.get_stat("last_sieve_in_lds") == form, tag
                got = dh.cpu().numpy().view(np.uint64)
                assert (got[nt:] == ~np.uint64(0)).all(), tag + ": wrote past its tiles"
                masks.append(got[:nt].copy())
            assert np.array_equal(masks[0], masks[1]), tag + ": scan differs from the direct kernel"
            offs, off = [0], 0
            for r in reads:
                off += len(r) + 1
                offs.append(off)
            present = set(filt)
            for r, (pos, _) in enumerate(py_hits(oracle, reads, k, present)):
                assert hit_positions(masks[0], offs[r], offs[r + 1] - 1).tolist() == pos, tag + f": read {r}"
            assert int(np.unpackbits(masks[0].view(np.uint8)).sum()) == int(want.sum()), tag + ": a hit outside the reads"


# ---------------------------------------------------------------------------------------------------------------------
# the other entry points
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def entry(oracle):
    k = 101
    rng = np.random.default_rng(77)
    G = genome(rng, 100_000)
    reads = rand_reads(rng, 300, 100, 200, n_frac=0.003, genome=G)
    filt = kmers_of(oracle, reads[::2], k)
    return dict(k=k, reads=reads, filt=filt, rows=rows_of(filt, k, oracle), st=ReadStream.from_strings(reads),
                want=truth_counts(oracle, reads, k, filt), windows=n_windows(oracle, reads, k))


def test_host_forms(entry):
    with KmerEngine(entry["k"], capacity_hint=1 << 10) as e:
        e.set_option("long_sieve", 1)
        e.load_filter(entry["rows"])
        e.count_filtered(entry["st"])                              # kdf_count_reads_filtered
        assert e.get_stat("last_count_path") == 3
        assert np.array_equal(e.query(entry["rows"]), entry["want"]) and e.stats()[2] == entry["windows"]
        hits, dist = e.scan(entry["st"])                           # kdf_scan_reads
        assert e.get_stat("last_scan_path") == 3
        e.set_option("long_sieve", 0)
        h0, d0 = e.scan(entry["st"])
        assert np.array_equal(hits, h0) and np.array_equal(dist, d0) and hits.any()


def test_count_uploaded_filtered(entry):
    with KmerEngine(entry["k"], capacity_hint=1 << 10) as e:
        e.set_option("long_sieve", 1)
        e.load_filter(entry["rows"])
        e.upload_async(0, entry["st"])
        e.count_uploaded(0, filtered=True)
        assert e.get_stat("last_count_path") == 3
        assert np.array_equal(e.query(entry["rows"]), entry["want"]) and e.stats()[2] == entry["windows"]


def test_read_hits_rows(entry):
    with KmerEngine(entry["k"], capacity_hint=1 << 10) as e:
        e.set_option("long_sieve", 1)
        e.count(ReadStream.from_strings(entry["reads"][::2]))
        rows1, bits1 = e.read_hits(entry["st"], want_bits=True)
        assert e.get_stat("last_scan_path") == 3
        e.set_option("long_sieve", 0)
        rows0, bits0 = e.read_hits(entry["st"], want_bits=True)
        assert e.get_stat("last_scan_path") == 0
        assert np.array_equal(rows1, rows0) and np.array_equal(bits1, bits0) and rows1.any()


def test_spool_replay_and_read_hits(entry):
    from kmer_denovo_filter_amd.spool import ReadSpool
    half = len(entry["reads"]) // 2
    with ReadSpool(0, 1 << 28, 0) as sp, KmerEngine(entry["k"], capacity_hint=1 << 10) as e:
        sp.keep_reads = True
        sp.set_option("segment_positions", 1 << 16)               # (two appends of ~22 000 positions: one segment)
        sp.append(ReadStream.from_strings(entry["reads"][:half]))
        sp.append(ReadStream.from_strings(entry["reads"][half:]))
        e.set_option("long_sieve", 1)
        e.load_filter(entry["rows"])
        sp.replay(e, ReadSpool.COUNT_FILTERED)
        assert e.get_stat("last_count_path") == 3
        assert np.array_equal(e.query(entry["rows"]), entry["want"]) and e.stats()[2] == entry["windows"]
        rows1 = sp.read_hits(e)
        assert e.get_stat("last_scan_path") == 3
        e.set_option("long_sieve", 0)
        rows0 = sp.read_hits(e)
        assert e.get_stat("last_scan_path") == 0
        assert np.array_equal(rows1, rows0) and rows1.any()


# ---------------------------------------------------------------------------------------------------------------------
# the mirrors pick the option up from the environment
# ---------------------------------------------------------------------------------------------------------------------

def _chain_stages(tmp, k, cand_fa, paths):
    """parent filter and Module 3 of the mini trio -> (mother's counts, proband-unique set, the Module 3 tuple)"""
    from conftest import GIAB
    from kmer_denovo_filter_amd import jf_io
    from kmer_denovo_filter_amd.core import bam_scanner
    from kmer_denovo_filter_amd.core.jellyfish_wrappers import _build_proband_jf_index
    from kmer_denovo_filter_amd.discovery.pipeline import _count_parent_jellyfish, _filter_parents_discovery
    from kmer_denovo_filter_amd.kmer_fasta import read_kmer_fasta_keys
    from kmer_denovo_filter_amd.reads import keys_to_kmers
    close = KmerEngine.close

    def recording_close(self):
        if getattr(self, "_h", None):
            paths.append((self.get_stat("last_count_path"), self.get_stat("last_scan_path")))
        close(self)

    KmerEngine.close = recording_close
    try:
        mother, father = os.path.join(GIAB, "HG004_mother.bam"), os.path.join(GIAB, "HG003_father.bam")
        mjf = _count_parent_jellyfish(mother, None, cand_fa, k, os.path.join(tmp, "mother"), 4)
        _, mkeys, _, mcnt = jf_io.read_index(mjf, expect_k=k)
        mcounts = dict(zip(keys_to_kmers(mkeys, None, k), mcnt.tolist()))
        n3, pu_fa = _filter_parents_discovery(mother, father, None, cand_fa, k, 4, tmp, 0)
        pu = set(keys_to_kmers(read_kmer_fasta_keys(pu_fa, k)[0], None, k))
        assert n3 == len(pu) > 0
        pjf = _build_proband_jf_index(pu_fa, k, tmp, n3)
        bam_scanner._init_scan_worker(pjf, k, 1)
        m3 = bam_scanner.scan_bam_module3(os.path.join(GIAB, "HG002_child.bam"))
        bam_scanner._worker_engine.close()
    finally:
        KmerEngine.close = close
    return mcounts, pu, m3


def test_chain_under_env(tmp_path, monkeypatch):
    from conftest import GIAB
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_kmers_discovery
    k = 75
    monkeypatch.delenv("KDF_LONG_SIEVE", raising=False)
    base = str(tmp_path / "child")
    os.makedirs(base)
    cand_fa, n = _extract_child_kmers_discovery(os.path.join(GIAB, "HG002_child.bam"), None, k, 3, 4, base)
    assert n > 0
    out = {}
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("KDF_LONG_SIEVE", env)
        tmp = str(tmp_path / f"env{env}")
        os.makedirs(tmp)
        paths = []
        out[env] = _chain_stages(tmp, k, cand_fa, paths), paths
    (m0, pu0, t0), p0 = out[None]
    (m1, pu1, t1), p1 = out["1"]
    assert m0 == m1 and pu0 == pu1
    assert t0 == t1
    assert all(p == (0, 0) for p in p0), p0
    assert any(c == 3 for c, _ in p1) and any(s == 3 for _, s in p1), p1
