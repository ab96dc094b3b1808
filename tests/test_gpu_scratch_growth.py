"""The engine's grow-only device scratch at a regrow and at the reuse after one.

One long-lived engine per k takes a stream of ~300 positions, then one of ~100 000, then ~300 again, through every host
form that stages something on the device: the large stream needs 25 KB of packed words and 12.5 KB of mask words, well
past the first allocation (first size x 1.125 + 4096 bytes), so every staging buffer is freed and allocated again while
the engine lives, and the third stream runs in the regrown buffers.  Key arrays go 100 -> 50 000 -> 100 keys.  The two
upload slots and a spool's host-tier staging and replay buffers go through the same sizes.

All host forms of an engine stage in ONE arena that each call lays out anew, so the walk also takes the forms with many
items through it: the reads are ungapped copies of genome stretches, which makes their alignment known (one ``M``
operation at the genome offset) -- hits in reference coordinates, the coverage list, the hit keys, a dozen SNVs placed on
the genome for the variant windows and their evidence, the host join and the histogram.  A last case alternates a call of
many small items with a call of one large item, so that the same arena bytes serve different items in consecutive calls.

Every result is compared with the pure-Python truths of this directory (``depth_truth``, ``hits_truth``,
``prefilter_model``, ``sketch_model``, ``coverage_model``, ``variants_model``, ``join_truth``; canonical keys by the
oracle's string rules) -- never with the same call on a fresh engine."""
import numpy as np
import pytest

import coverage_model as CM
import depth_truth as DT
import hits_truth as HT
import join_truth as JT
import kmer_truth as KT
import prefilter_model as PM
import sketch_model as SK
import variants_model as VM

pytestmark = pytest.mark.gpu

ERR_STATE = 6
SIZES = (300, 100_000, 300)           # stream positions
N_KEYS = (100, 50_000, 100)           # keys of the query / add_pairs calls
PF_LOG2, SK_LOG2 = 16, 12
N_SNV = 12


class _Batch:
    """reads, their stream, and what the models need of them (computed once)"""
    def __init__(self, rng, genome, k, positions, n_keys):
        from kmer_denovo_filter_amd import ReadStream
        reads, starts, n = [], [], 0
        while n < positions:
            L = int(rng.integers(k + 5, k + 90))
            a = int(rng.integers(0, len(genome) - L))
            starts.append(a)
            r = list(genome[a:a + L])
            for j in range(L):
                x = rng.random()
                if x < 0.01:
                    r[j] = "ACGT"[int(rng.integers(0, 4))]
                elif x < 0.012:
                    r[j] = "N"
            reads.append("".join(r))
            n += L + 1
        reads.append(reads[0])                                      # (so that even a small batch holds k-mers seen twice)
        starts.append(starts[0])
        n += len(reads[0]) + 1
        self.reads = reads
        self.stream = ReadStream.from_strings(reads)
        assert self.stream.n_bases == n and np.array_equal(self.stream.offsets, DT.offsets_of(reads))
        self.keys = DT.keys_of_reads(reads, k)
        self.counts = {}
        for ks in self.keys:
            for _, v in ks:
                self.counts[v] = self.counts.get(v, 0) + 1
        # keys for query / add_pairs: the stream's own (at most 3 in 5 of the array), then keys no stream holds
        own = sorted(self.counts)[:n_keys * 3 // 5]
        absent = set()
        while len(own) + len(absent) < n_keys:
            v = int.from_bytes(rng.bytes(32), "little") % (1 << (2 * k))
            if v not in self.counts:
                absent.add(v)
        self.qkeys = own + sorted(absent)
        self.qcounts = (np.arange(n_keys) % 5).astype(np.uint32)      # (a 0 stores the key with count 0)
        # the alignment of the reads: ungapped, at their genome offset
        self.span = len(genome)
        self.ref_start = np.array(starts, np.int64)
        self.cigar = CM.cigar_words([(0, len(r)) for r in reads])
        self.cigar_offsets = np.arange(len(reads) + 1, dtype=np.int64)
        offs = DT.offsets_of(reads)
        self.key_at = {int(offs[r]) + i: v for r, ks in enumerate(self.keys) for i, v in ks}      # stream position -> key
        # SNVs on the genome, each under the middle of some read: the read's own base (its windows support the ALT) or another
        snv = []
        for r in rng.choice(len(reads), N_SNV, replace=len(reads) < N_SNV).tolist():
            at = len(reads[r]) // 2
            base = reads[r][at] if reads[r][at] in "ACGT" and len(snv) % 3 else "ACGT"[len(snv) % 4]
            snv.append((starts[r] + at, 1, 1, base.encode()))
        snv.sort(key=lambda x: x[0])
        self.var = {"packed": self.stream.packed, "invalid": self.stream.invalid, "n_bases": n, "offsets": self.stream.offsets,
                    "ref_start": self.ref_start, "cigar": self.cigar, "cigar_offsets": self.cigar_offsets,
                    "var_pos": np.array([x[0] for x in snv], np.int64), "var_span": np.ones(N_SNV, np.uint32),
                    "var_ref_len": np.ones(N_SNV, np.uint32), "alt": b"".join(x[3] for x in snv),
                    "alt_offsets": np.arange(N_SNV + 1, dtype=np.int64)}
        self.windows = VM.variant_windows(self.var, k)
        assert len(self.windows[0]) >= N_SNV and 0 < int(self.windows[2].sum()) < len(self.windows[0])


@pytest.fixture(scope="module", params=[31, 63, 65])
def case(request):
    k = request.param
    rng = np.random.default_rng(100 + k)
    genome = "".join(rng.choice(list("ACGT"), 40_000))
    batches = [_Batch(rng, genome, k, n, m) for n, m in zip(SIZES, N_KEYS)]
    # bytes of packed words: the large stream's are past what the small one's allocation left room for
    assert batches[1].stream.n_bases / 4 > batches[0].stream.n_bases / 4 * 1.125 + 4096 + 64
    return k, batches


def _key_args(k, keys):
    if k > 63:
        return (KT.rows(keys, (2 * k + 63) // 64),)
    return KT.lohi(keys)


def _table(e, k, min_count=0):
    """the engine's dump as {key int: count}"""
    lo, hi, cnt = e.export_ge(min_count)
    keys = [KT.int_of_row(r) for r in lo] if k > 63 else [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())]
    out = dict(zip(keys, cnt.tolist()))
    assert len(out) == len(keys)
    return out


def _add(table, counts):
    for v, c in counts.items():
        table[v] = table.get(v, 0) + c


def _ints(k, keys):
    """the keys of an export or a join (``(lo, hi)`` or the rows of long keys) as ints"""
    return [KT.int_of_row(r) for r in keys] if k > 63 else [int(a) | (int(c) << 64) for a, c in zip(keys[0].tolist(), keys[1].tolist())]


def _variant_windows(e, b):
    v = b.var
    return e.variant_windows(b.stream, v["ref_start"], v["cigar"], v["cigar_offsets"], v["var_pos"], v["var_span"], v["var_ref_len"],
                             v["alt"], v["alt_offsets"])


def _same(got, want, who):
    assert len(got) == len(want), who
    for g, w in zip(got, want):
        assert np.array_equal(g, w), who


def _host_forms(e, o, k, b, who):
    s, reads, keys = b.stream, b.reads, b.keys
    n_windows = sum(b.counts.values())
    # count, export, stats
    e.clear()
    e.count(s)
    T = dict(b.counts)
    assert _table(e, k) == T, who
    assert e.stats()[1:] == (len(T), n_windows), who
    # query and add_pairs with this step's key array
    qa = _key_args(k, b.qkeys)
    assert np.array_equal(e.query(*qa), [T.get(v, 0) for v in b.qkeys]), who
    e.add_pairs(qa[0], qa[1] if k <= 63 else None, b.qcounts)
    for v, c in zip(b.qkeys, b.qcounts.tolist()):
        T[v] = T.get(v, 0) + c
    assert np.array_equal(e.query(*qa), [T[v] for v in b.qkeys]), who
    assert e.count_ge(1) == sum(1 for c in T.values() if c >= 1), who
    # the histogram, and the host join against a second engine that is given this engine's own table (the engine itself is
    # refused as `other`): every key meets its own count there
    cnts = np.array(list(T.values()), np.int64)
    assert np.array_equal(e.histogram(3), np.append(np.bincount(cnts[cnts <= 3], minlength=4), (cnts > 3).sum())), who
    lo, hi, cnt = e.export_ge(0)
    o.clear()
    o.add_pairs(lo, hi if k <= 63 else None, cnt)
    jk, jc, joc = e.export_join(o, 1, None, 2, None)
    want_j = JT.join(list(T), list(T.values()), list(T), list(T.values()), 1, None, 2, None)
    assert (_ints(k, jk), jc.tolist(), joc.tolist()) == want_j and len(want_j[0]) > 0, who
    # window counts, read depth, read hits with the mask, the hit list
    want_c, want_v, offs = DT.profile(reads, k, T, keys)
    got_c, got_v = e.window_counts(s, want_valid=True)
    assert np.array_equal(got_c, want_c) and np.array_equal(DT.bits(got_v, s.n_bases), want_v), who
    assert np.array_equal(e.read_depth(s, 1), DT.depth_rows(reads, k, T, 1, keys)), who
    want_rows, per_read = HT.read_hits(reads, k, T, keys)
    got_rows, bits = e.read_hits(s, want_bits=True)
    assert np.array_equal(got_rows, want_rows) and want_rows[:, 0].sum() > 0, who
    assert np.array_equal(bits, HT.mask_words(reads, per_read, len(bits))), who
    pos, rd = e.hit_list(bits, s.n_bases, offs)
    want_pos, want_rd = HT.hit_list(reads, per_read)
    assert np.array_equal(pos.astype(np.int64), want_pos) and np.array_equal(rd, want_rd), who
    # hits in reference coordinates, added to accumulators that are not zero; the list of the covered positions; the hit keys
    kc, rc = (np.arange(b.span) % 7).astype(np.uint32), (np.arange(b.span) % 3).astype(np.uint32)
    want_kc, want_rc = kc.copy(), rc.copy()
    e.hit_coverage(bits, s.n_bases, offs, b.ref_start, b.cigar, b.cigar_offsets, kc, rc)
    CM.hit_coverage(bits, s.n_bases, k, offs, b.ref_start, b.cigar, b.cigar_offsets, want_kc, want_rc)
    assert np.array_equal(kc, want_kc) and np.array_equal(rc, want_rc) and int(rc.sum()) > int((np.arange(b.span) % 3).sum()), who
    _same(e.coverage_list(kc, rc, 100, b.span - 200, 3), CM.coverage_list(want_kc, want_rc, 100, b.span - 200, 3), who)
    assert [KT.int_of_row(r) for r in e.hit_keys(s, pos)] == [b.key_at[p] for p in want_pos.tolist()], who
    # the windows that span the SNVs, their keys, and the evidence of the table for them
    _same(_variant_windows(e, b), b.windows, who)
    pair_var, pair_flags, entry_pos, entry_pair = b.windows[1:]
    rows = e.hit_keys(s, entry_pos)
    ekeys = [b.key_at[p] for p in entry_pos.tolist()]
    assert [KT.int_of_row(r) for r in rows] == ekeys, who
    _same(e.variant_evidence(rows, entry_pair, pair_var, pair_flags, N_SNV), VM.variant_evidence(ekeys, entry_pair, pair_var, pair_flags, N_SNV, T), who)
    # count --if against half of the stream's keys and a few it does not hold
    filt = sorted(b.counts)[::2] + b.qkeys[-5:]
    fa = _key_args(k, filt)
    e.load_filter(*fa)
    e.count_filtered(s)
    assert np.array_equal(e.query(*fa), [b.counts.get(v, 0) for v in filt]), who
    assert e.stats()[1:] == (len(filt), n_windows), who
    # prefilter tally, then the armed count
    e.clear()
    e.prefilter_begin(2, PF_LOG2)
    e.prefilter_add(s)
    e.prefilter_arm()
    e.count(s)
    admitted, by_value = PM.model(b.counts, k, PF_LOG2, 2)
    assert _table(e, k) == admitted and e.prefilter_fill() == by_value, who
    assert 0 < len(admitted) and (len(b.counts) < 1000 or len(admitted) < len(b.counts)), who
    e.prefilter_drop()
    # sketch
    e.sketch_begin(SK_LOG2)
    e.sketch_add(s)
    assert np.array_equal(e.sketch_registers(), SK.registers_of_keys(b.counts.keys(), k, SK_LOG2)), who
    e.sketch_drop()


def _upload_slots(e, k, small, large, small2):
    from kmer_denovo_filter_amd._native import KdfError
    e.clear()
    e.upload_async(0, small.stream)
    e.upload_async(1, large.stream)
    e.count_uploaded(0)
    e.upload_async(0, large.stream)               # slot 0 regrows while its count may still be reading the old buffers
    e.count_uploaded(1)
    e.count_uploaded(0)
    T = dict(small.counts)
    _add(T, large.counts)
    _add(T, large.counts)
    assert _table(e, k) == T
    # a sketch keeps the slot's batch, a count consumes it
    e.sketch_begin(SK_LOG2)
    e.upload_async(1, small2.stream)              # (in the regrown slot)
    e.sketch_add_uploaded(1)
    e.count_uploaded(1)
    with pytest.raises(KdfError) as ei:
        e.count_uploaded(1)
    assert ei.value.code == ERR_STATE
    _add(T, small2.counts)
    assert np.array_equal(e.sketch_registers(), SK.registers_of_keys(small2.counts.keys(), k, SK_LOG2))
    e.sketch_drop()
    assert _table(e, k) == T
    assert e.stats()[2] == sum(T.values())


def test_one_engine_through_small_large_small(case):
    from kmer_denovo_filter_amd import KmerEngine
    k, batches = case
    with KmerEngine(k, capacity_hint=1 << 12) as e, KmerEngine(k, capacity_hint=1 << 12) as o:
        for i, b in enumerate(batches):
            _host_forms(e, o, k, b, f"k={k} stream {i} ({b.stream.n_bases} positions)")
        _upload_slots(e, k, *batches)


def test_many_small_items_after_one_large_item_and_back(case):
    """``variant_windows`` registers 18 items (the stream, the offsets, ten inputs, five outputs), ``export_ge`` one large
    one beside two smaller: alternated on one engine, in both orders, every item of a call lies on bytes that the call before
    it used for something else."""
    from kmer_denovo_filter_amd import KmerEngine
    k, batches = case
    small, large = batches[0], batches[1]
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        e.count(large.stream)
        for i in range(2):
            who = f"k={k} round {i}"
            assert _table(e, k) == large.counts, who                   # one large item ...
            _same(_variant_windows(e, small), small.windows, who)      # ... then many small ones ...
            _same(_variant_windows(e, large), large.windows, who)
            assert _table(e, k, 2) == {v: c for v, c in large.counts.items() if c >= 2}, who      # ... and back


def test_host_tier_spool_through_small_large_small(case):
    """No HBM budget: every segment is in pinned host memory, so appends pass through the spool's device staging and the
    per-read replays through its replay buffers -- both regrow at the large batch."""
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.spool import ReadSpool
    k, batches = case
    with ReadSpool(0, 0, 1 << 30) as sp, KmerEngine(k, capacity_hint=1 << 12) as e:
        sp.set_option("segment_positions", 1 << 12)
        for b in batches:
            sp.append(b.stream, keep_reads=True)
        assert (sp.stat("segments"), sp.stat("hbm_bytes"), sp.stat("overflowed")) == (3, 0, 0) and sp.stat("host_bytes") > 0
        assert sp.n_reads == sum(len(b.reads) for b in batches)
        e.count(batches[0].stream)
        e.count(batches[1].stream)
        T = dict(batches[0].counts)
        _add(T, batches[1].counts)
        want_hits = np.concatenate([HT.read_hits(b.reads, k, T, b.keys)[0] for b in batches])
        want_depth = np.concatenate([DT.depth_rows(b.reads, k, T, 1, b.keys) for b in batches])
        assert want_hits[:, 0].sum() > 0
        for _ in range(2):                                          # the second replay runs in the buffers the first left
            assert np.array_equal(sp.read_hits(e), want_hits)
            assert np.array_equal(sp.read_depth(e, 1), want_depth)
