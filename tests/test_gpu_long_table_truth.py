"""The long-key table (odd k 65..201) under CHOSEN hashes, against tests/long_truth.py.

Random keys never share the 64-bit stored form h, so with them the middle-word compares of kdf_try_add_long /
kdf_find_long never decide, the lower passes of the W-word sort never decide, probe runs stay short, and the owner,
slice and sieve rules never meet their boundaries.  Here the keys are written down: groups that share h and the top word
and differ in ONE middle word, probe runs that wrap inside a bucket, a bucket filled to its last slot, hashes on both
sides of every owner / slice boundary, absent probes that pass the sieve and land on an occupied home slot, and rows
that only a lower sort pass can order.  Every comparison is exact; capacity and bucket_bits are read from the engine."""
import collections

import numpy as np
import pytest

import long_truth as T
from kmer_denovo_filter_amd import KmerEngine, ReadStream
from kmer_denovo_filter_amd._native import KdfError, KDF_ERR_TABLE_FULL
from kmer_denovo_filter_amd.reads import stream_words
from test_gpu_long_ranks import GUARD, dump_by_owner
from test_gpu_long_sieve import l2_bits

pytestmark = pytest.mark.gpu

KS = (65, 95, 127, 159, 191, 201)            # W = 3, 3, 4, 5, 6, 7; top words of 2, 62, 62, 62, 62, 18 bits
GROUP_SIZES = (2, 3, 65, 300)
DUMP_PARTS = (1, 3, 64)
FORMS = ("direct", "lds", "l2")              # the direct kernels; the sieve copied into LDS; the sieve read from L2


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------

def up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def log2(n):
    assert n > 0 and n & (n - 1) == 0
    return n.bit_length() - 1


def geometry(e):
    """(log2 of the capacity, bucket_bits) as the engine reports them"""
    return log2(e.stats()[0]), e.get_stat("bucket_bits")


def as_dict(rows, cnt):
    d = {tuple(r): int(c) for r, c in zip(np.asarray(rows).tolist(), np.asarray(cnt).tolist())}
    assert len(d) == len(cnt), "a key is listed twice"
    return d


def check_table(e, rows, cnt, absent, tag=""):
    """The table holds exactly `rows` with `cnt`: query, the sorted dump, the dump by owner, and the key counter."""
    rows, cnt = np.asarray(rows, np.uint64), np.asarray(cnt, np.uint32)
    got = e.query(rows)
    bad = np.nonzero(got != cnt)[0]
    assert bad.size == 0, (f"{tag}: query of stored row {bad[0]} (h={int(T.long_hash(rows[bad[:1]])[0]):#x}) gives "
                           f"{got[bad[0]]}, not {cnt[bad[0]]}")
    if len(absent):
        got = e.query(absent)
        bad = np.nonzero(got)[0]
        assert bad.size == 0, (f"{tag}: absent row {bad[0]} (h={int(T.long_hash(absent[bad[:1]])[0]):#x}) is found "
                               f"with count {got[bad[0]]}")
    want_rows, want_cnt = T.sort_rows(rows, cnt)
    keys, _, c = e.export_ge(0)
    assert np.array_equal(keys, want_rows) and np.array_equal(c, want_cnt), f"{tag}: export_ge(0)"
    want = as_dict(rows, cnt)
    own_h = T.long_hash(rows)
    for parts in DUMP_PARTS:
        n, counts, _, segs = dump_by_owner(e, parts, 0)
        assert n == len(rows), f"{tag}: dump over {parts} parts lists {n} entries"
        seen = {}
        for p, (r, c) in enumerate(segs):
            if len(c):
                assert (T.owner(T.long_hash(r), parts) == p).all(), f"{tag}: part {p} of {parts} holds another owner's key"
            seen.update(as_dict(r, c))
        assert seen == want, f"{tag}: dump over {parts} parts"
        assert counts == np.bincount(T.owner(own_h, parts).astype(np.int64), minlength=parts).tolist()
    assert e.stats()[1] == len(rows), f"{tag}: distinct"


def kmer_reads(rows, k, reps):
    """Each row as a read of exactly k bases, every other one as its reverse complement, read i given reps[i] times."""
    out = []
    for i, (row, c) in enumerate(zip(rows, reps)):
        s = T.row_to_kmer(row, k)
        out += [T.revcomp_str(s) if i & 1 else s] * int(c)
    return out


def collision_groups(k, rng, canonical=True, sizes=GROUP_SIZES):
    """Groups of rows with ONE hash and ONE top word that differ in exactly one middle word (each j in 1 .. W-2), one
    group that shares the hash and every middle word and differs in the top word only, and one that shares every upper
    word and the home slot (of any table of up to 2^20 slots) and differs in w0, hence in the hash, only."""
    W, tb = T.W_of(k), T.top_width(k)
    groups = []
    for j in range(1, W - 1):
        for n in sizes:
            h = int(T._rand64(rng, 1)[0])
            g = T.rows_with_hash(h, k, n, rng, share=("middle", j), canonical=canonical)
            assert (T.long_hash(g) == np.uint64(h)).all() and len(set(g[:, W - 1].tolist())) == 1
            assert len(set(g[:, j].tolist())) == n
            groups.append(g)
    n = 2 if tb == 2 else 30
    h = int(T._rand64(rng, 1)[0])
    groups.append(T.rows_with_hash(h, k, n, rng, share="middles", canonical=canonical))
    top20 = int(rng.integers(0, 1 << 20))
    g = T.rows_with_hash(lambda m: T.hash_with(rng, m, top_bits=top20, nbits=20), k, 30, rng, share="upper", canonical=canonical)
    assert len(np.unique(g[:, 1:], axis=0)) == 1 and len(set(T.home(T.long_hash(g), 20).tolist())) == 1
    groups.append(g)
    return groups


def split(groups):
    """(even members, odd members) of every group"""
    return np.concatenate([g[::2] for g in groups]), np.concatenate([g[1::2] for g in groups])


def set_counts(e, rows, cnt):
    import torch
    dk, dc = up(rows), up(np.asarray(cnt, np.uint32))
    torch.cuda.synchronize()
    e.set_counts_w_dev(dk.data_ptr(), dc.data_ptr(), len(rows))


def run_block(e, k, stored, absent, rng, filter_mode, pads=None, tag=""):
    """Every check of the collision block on engine e: `stored` goes in (add_pairs with distinct counts, or load_filter +
    count_filtered of a stream that also holds every absent row), `absent` -- keys chosen to collide with them -- must
    stay out until they are added.  pads: further rows stored with the first step (filter mode: they size the table).
    -> (rows, counts) the table holds in the end."""
    n = len(stored)
    pads = np.zeros((0, T.W_of(k)), np.uint64) if pads is None else pads
    if filter_mode:
        cs = (1 + np.arange(n) % 3).astype(np.uint32)
        e.load_filter(np.concatenate([stored, pads]))
        reads = kmer_reads(stored, k, cs) + kmer_reads(absent, k, 1 + np.arange(len(absent)) % 2)
        e.count_filtered(ReadStream.from_strings(reads))
        assert e.stats()[2] == len(reads), f"{tag}: windows"
        pc = np.zeros(len(pads), np.uint32)
    else:
        cs = (1 + rng.permutation(n)).astype(np.uint32)           # distinct counts
        pc = (1000 + np.arange(len(pads))).astype(np.uint32)
        e.add_pairs(np.concatenate([stored, pads]), None, np.concatenate([cs, pc]))
    have, hc = np.concatenate([stored, pads]), np.concatenate([cs, pc])
    check_table(e, have, hc, absent, tag + ": even members stored")
    # set_counts on the stored members sets exactly those
    new = (5000 + rng.permutation(n)).astype(np.uint32)
    set_counts(e, stored, new)
    hc = np.concatenate([new, pc])
    check_table(e, have, hc, absent, tag + ": after set_counts")
    # ... and a call that includes an absent collider raises and changes nothing
    with pytest.raises(KdfError, match="not stored"):
        set_counts(e, np.concatenate([stored[:3], absent]), np.concatenate([new[:3], np.full(len(absent), 9, np.uint32)]))
    check_table(e, have, hc, absent, tag + ": after the refused set_counts")
    # the odd members join
    ca = (20000 + rng.permutation(len(absent))).astype(np.uint32)
    e.add_pairs(absent, None, ca)
    have, hc = np.concatenate([have, absent]), np.concatenate([hc, ca])
    check_table(e, have, hc, np.zeros((0, T.W_of(k)), np.uint64), tag + ": all members stored")
    return have, hc


# ---------------------------------------------------------------------------------------------------------------------
# a. collision groups
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filter_mode", (False, True), ids=("pairs", "filter"))
@pytest.mark.parametrize("k", KS)
def test_collision_groups(k, filter_mode):
    rng = np.random.default_rng(k)
    stored, absent = split(collision_groups(k, rng))
    with KmerEngine(k, capacity_hint=1) as e:
        run_block(e, k, stored, absent, rng, filter_mode, tag=f"k={k}")


# ---------------------------------------------------------------------------------------------------------------------
# b. the same groups through the read stream
# ---------------------------------------------------------------------------------------------------------------------

def stream_truth(reads, k, index):
    """Per read: the canonical key of every window, and from the index {key: count} the hit offsets, the distinct hit
    keys, and the count of every window (absent = 0)."""
    out = []
    for s in reads:
        keys = T.window_keys(s, k)
        cnt = [index.get(v, 0) for v in keys]
        out.append((keys, cnt))
    return out


def hit_bitmap(st, truth, n_words):
    bits = np.zeros(n_words * 64, dtype=bool)
    for r, (_, cnt) in enumerate(truth):
        for i, c in enumerate(cnt):
            if c:
                bits[int(st.offsets[r]) + i] = True
    return np.packbits(bits, bitorder="little").view(np.uint64)


def engine_for_form(k, form, n_keys):
    e = KmerEngine(k, capacity_hint=1)
    if form == "l2":
        e.set_option("sieve_bits", l2_bits(n_keys))
    e.set_option("long_sieve", 0 if form == "direct" else 1)
    return e


def check_form(e, form, what):
    """the kernel, and the form of it, that answered the last scan / count --if"""
    assert e.get_stat("last_scan_path" if what == "scan" else "last_count_path") == (0 if form == "direct" else 3)
    if form != "direct":
        assert e.get_stat("last_sieve_in_lds") == (1 if form == "lds" else 0)


def reads_around(rows, k, rng, n=4, flank=23):
    """a few longer reads with a crafted k-mer in the middle"""
    out = []
    for row in rows[:n]:
        a, b = ("".join(rng.choice(list("ACGT"), flank)) for _ in range(2))
        out.append(a + T.row_to_kmer(row, k) + b)
    return out


@pytest.mark.parametrize("k", KS)
def test_collision_groups_counted_from_reads(k):
    rng = np.random.default_rng(1000 + k)
    groups = collision_groups(k, rng)
    rows = np.concatenate(groups)
    reps = 1 + np.arange(len(rows)) % 3
    reads = kmer_reads(rows, k, reps) + reads_around(rows[::37], k, rng)
    want = collections.Counter(v for s in reads for v in T.window_keys(s, k))
    W = T.W_of(k)
    want_rows = T.rows_of_ints(sorted(want), W)
    want_cnt = np.array([want[v] for v in sorted(want)], np.uint32)
    with KmerEngine(k, capacity_hint=1) as e:
        e.count(ReadStream.from_strings(reads))
        keys, _, cnt = e.export_ge(0)
        assert np.array_equal(keys, want_rows) and np.array_equal(cnt, want_cnt)
        assert e.stats()[1:] == (len(want), sum(want.values()))
        assert np.array_equal(e.query(rows), np.array([want[T.row_to_int(r)] for r in rows], np.uint32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", KS)
def test_collision_groups_probed_by_reads(k, form):
    rng = np.random.default_rng(2000 + k)
    groups = collision_groups(k, rng)
    stored, absent = split(groups)
    cs = (1 + rng.permutation(len(stored))).astype(np.uint32)
    index = {T.row_to_int(r): int(c) for r, c in zip(stored, cs)}
    members = np.concatenate(groups)
    big = next(g for g in groups if len(g) == 65)
    two = T.row_to_kmer(big[0], k) + T.revcomp_str(T.row_to_kmer(big[2], k))       # two stored members of one group
    probe = kmer_reads(members, k, np.ones(len(members), int)) + reads_around(stored[::41], k, rng) \
        + reads_around(absent[::41], k, rng) + [two]
    st = ReadStream.from_strings(probe)
    truth = stream_truth(probe, k, index)
    n_words = stream_words(st.n_bases)[1]
    want_bits = hit_bitmap(st, truth, n_words)
    want_hits = np.array([sum(1 for c in cnt if c) for _, cnt in truth], np.uint32)
    want_dist = np.array([len({v for v, c in zip(keys, cnt) if c}) for keys, cnt in truth], np.uint32)
    assert want_dist[-1] == 2 and want_hits[-1] == 2
    with engine_for_form(k, form, len(stored)) as e:
        e.add_pairs(stored, None, cs)
        hits, dist = e.scan(st)
        check_form(e, form, "scan")
        assert np.array_equal(hits[:n_words], want_bits), "scan: hit words"
        assert np.array_equal(dist, want_dist), "scan: distinct"
        rh, bits = e.read_hits(st, want_bits=True)
        assert np.array_equal(bits[:n_words], want_bits) and np.array_equal(rh[:, 0], want_hits) and np.array_equal(rh[:, 1], want_dist)
        if form == "direct":                                       # (these two take no sieve)
            wc = e.window_counts(st)
            want_wc = np.zeros(st.n_bases, np.uint32)
            for r, (_, cnt) in enumerate(truth):
                want_wc[int(st.offsets[r]):int(st.offsets[r]) + len(cnt)] = cnt
            assert np.array_equal(wc, want_wc), "window_counts"
            rd = e.read_depth(st, 0)
            want_rd = np.array([[len(c), sum(1 for x in c if x), sum(1 for x in c if x == 0), min(c), max(c), sum(c)]
                                for _, c in truth], np.uint64)
            assert np.array_equal(rd, want_rd), "read_depth"
        check_table(e, stored, cs, absent, f"k={k} {form}: after the probes")
    # count --if: the colliders' reads count nothing
    mult = collections.Counter(v for keys, _ in truth for v in keys)
    with engine_for_form(k, form, len(stored)) as e:
        e.load_filter(stored)
        e.count_filtered(st)
        check_form(e, form, "count")
        want_c = np.array([mult[T.row_to_int(r)] for r in stored], np.uint32)
        assert want_c.min() >= 1
        assert e.stats()[2] == sum(mult.values())
        check_table(e, stored, want_c, absent, f"k={k} {form}: count --if")


# ---------------------------------------------------------------------------------------------------------------------
# c. crowded geometry
# ---------------------------------------------------------------------------------------------------------------------

def crowded_hashes(rng, log2cap, bucket_bits, bkt, n=300, last=40):
    """n distinct hashes whose home slots are the last `last` slots of bucket bkt of a table of 2^log2cap slots"""
    slots = (bkt << bucket_bits) + (1 << bucket_bits) - last + np.arange(n) % last
    h = T.hash_with(rng, n, top_bits=slots, nbits=log2cap)
    assert len(set(h.tolist())) == n and np.array_equal(T.home(h, log2cap), slots.astype(np.uint64))
    return h


@pytest.mark.parametrize("filter_mode", (False, True), ids=("pairs", "filter"))
@pytest.mark.parametrize("log2cap,where", ((10, "last"), (11, "last"), (12, "first"), (12, "last")))
@pytest.mark.parametrize("k", KS)
def test_crowded_bucket_end(k, log2cap, where, filter_mode):
    """2^10 and 2^11 slots are a single bucket, whose last slots are the table's own; 2^12 slots are two buckets."""
    rng = np.random.default_rng(3000 + 16 * k + log2cap)
    n_filter = (1 << (log2cap - 2)) + 64         # filter keys that get 2^log2cap slots (and leave room for the odd members)
    with KmerEngine(k, capacity_hint=1) as e:
        if not filter_mode:
            e.reserve(1 << (log2cap - 1))
        else:
            e.load_filter(T.random_rows(rng, k, n_filter))          # (the geometry this many filter keys get)
        lc, bb = geometry(e)
        assert lc == log2cap and bb == min(log2cap, 11)
        bkt = 0 if where == "first" else (1 << (lc - bb)) - 1
        h = crowded_hashes(rng, lc, bb, bkt)
        rows = T.rows_with_hash(h, k, len(h), rng, canonical=True)
        stored, absent = rows[::2], rows[1::2]
        pads = T.rows_with_hash(T._rand64(rng, n_filter - len(stored)), k, n_filter - len(stored), rng) if filter_mode else None
        have, hc = run_block(e, k, stored, absent, rng, filter_mode, pads=pads, tag=f"k={k} 2^{lc} {where}")
        assert geometry(e)[0] == lc
        # grow: the rehash reads stored forms, and the homes gain bits
        more = T.random_rows(rng, k, (1 << lc) + 1 - len(have))   # capacity doubles twice
        e.add_pairs(more, None, np.full(len(more), 7, np.uint32))
        assert geometry(e)[0] == lc + 2
        check_table(e, np.concatenate([have, more]), np.concatenate([hc, np.full(len(more), 7, np.uint32)]),
                    np.zeros((0, T.W_of(k)), np.uint64), f"k={k} 2^{lc} {where}: grown")


# ---------------------------------------------------------------------------------------------------------------------
# d. a bucket filled to its last slot
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_exactly_full_bucket(k):
    rng = np.random.default_rng(4000 + k)
    W = T.W_of(k)
    with KmerEngine(k, capacity_hint=1) as e:
        e.reserve(1 << 13)
        lc, bb = geometry(e)
        assert lc == 14 and bb < lc
        bkt = (1 << (lc - bb)) - 2
        n = 1 << bb

        def in_bucket(m):
            h = T.hash_with(rng, m, top_bits=bkt, nbits=lc - bb)
            assert (T.bucket(h, lc, bb) == bkt).all()
            return h

        h = in_bucket(n)
        rows = T.rows_with_hash(h, k, n, rng, canonical=True)
        cs = (1 + rng.permutation(n)).astype(np.uint32)
        e.add_pairs(rows, None, cs)                                # fills the bucket: every probe run ends on a match
        assert geometry(e) == (lc, bb)
        assert e.stats()[1] == n and np.array_equal(e.query(rows), cs)
        # absent keys of that bucket find no empty slot: the probe count ends the search
        coll = T.rows_with_hash(h[:200], k, 200, rng, share="top", canonical=True, top=rows[:200, W - 1])
        other = T.rows_with_hash(in_bucket(1000), k, 1000, rng, canonical=True)
        absent = np.concatenate([coll, other])
        assert not (e.query(absent)).any()
        probe = kmer_reads(np.concatenate([rows[:300], absent]), k, np.ones(300 + len(absent), int))
        st = ReadStream.from_strings(probe)
        rh = e.read_hits(st)
        assert rh[:300].tolist() == [[1, 1]] * 300 and not rh[300:].any()
        hits, dist = e.scan(st)
        assert dist[:300].tolist() == [1] * 300 and not dist[300:].any()
        assert int(sum(bin(int(x)).count("1") for x in hits)) == 300
        # one key more does not fit
        with pytest.raises(KdfError) as ei:
            e.add_pairs(other[:1], None, np.array([1], np.uint32))
        assert ei.value.code == KDF_ERR_TABLE_FULL
        e.clear()
        reads = kmer_reads(other[:50], k, 1 + np.arange(50) % 3) + reads_around(other[50:54], k, rng)
        want = collections.Counter(v for s in reads for v in T.window_keys(s, k))
        e.count(ReadStream.from_strings(reads))
        keys, _, cnt = e.export_ge(0)
        assert np.array_equal(keys, T.rows_of_ints(sorted(want), W))
        assert np.array_equal(cnt, np.array([want[v] for v in sorted(want)], np.uint32))
        assert e.stats()[1:] == (len(want), sum(want.values()))


# ---------------------------------------------------------------------------------------------------------------------
# e. owner and slice boundaries
# ---------------------------------------------------------------------------------------------------------------------

def boundary_values(parts_list):
    """per parts: the first 16-bit value of every part and the value before it; 0 and 65535"""
    vs = {0, 65535}
    for parts in parts_list:
        for j in range(1, parts):
            v = -(-j * 65536 // parts)
            assert (v * parts) >> 16 == j and ((v - 1) * parts) >> 16 == j - 1
            vs |= {v, v - 1}
    return np.array(sorted(vs), np.uint64)


@pytest.mark.parametrize("k", KS)
def test_owner_boundaries(k):
    rng = np.random.default_rng(5000 + k)
    parts_list = (2, 3, 5, 7, 64)
    vs = boundary_values(parts_list)
    h = np.concatenate([T.hash_with(rng, len(vs), owner16=vs, fill=0), T.hash_with(rng, len(vs), owner16=vs, fill=1)])
    assert h[0] == 0 and h[-1] == np.uint64(T.M64)
    rows = T.rows_with_hash(h, k, len(h), rng)
    cs = (1 + np.arange(len(rows))).astype(np.uint32)
    with KmerEngine(k, capacity_hint=1) as e:
        e.add_pairs(rows, None, cs)
        want = as_dict(rows, cs)
        for parts in parts_list:
            own = T.owner(h, parts)
            assert set(own.tolist()) == set(range(parts))
            n, counts, _, segs = dump_by_owner(e, parts, 0)
            assert n == len(rows) and counts == np.bincount(own.astype(np.int64), minlength=parts).tolist()
            seen = {}
            for p, (r, c) in enumerate(segs):
                assert set(map(tuple, r.tolist())) == set(map(tuple, rows[own == p].tolist())), f"part {p} of {parts}"
                seen.update(as_dict(r, c))
            assert seen == want


@pytest.mark.parametrize("k", KS)
def test_slice_boundaries(k):
    rng = np.random.default_rng(6000 + k)
    W = T.W_of(k)
    vs = boundary_values((2, 3, 5))
    h = np.concatenate([T.hash_with(rng, len(vs), slice16=vs, fill=0), T.hash_with(rng, len(vs), slice16=vs, fill=1)])
    rows = T.rows_with_hash(h, k, len(h), rng, canonical=True)
    reps = 1 + np.arange(len(rows)) % 3
    st = ReadStream.from_strings(kmer_reads(rows, k, reps))
    with KmerEngine(k, capacity_hint=1) as e:
        for key_parts in (2, 3, 5):
            sl = T.slice_of(h, key_parts)
            assert set(sl.tolist()) == set(range(key_parts))
            total = 0
            for part in range(key_parts):
                e.clear()
                e.set_option("key_parts", key_parts)
                e.set_option("key_part", part)
                e.count(st)
                want_rows, want_cnt = T.sort_rows(rows[sl == part], reps[sl == part].astype(np.uint32))
                keys, _, cnt = e.export_ge(0)
                assert np.array_equal(keys, want_rows) and np.array_equal(cnt, want_cnt), f"slice {part} of {key_parts}"
                total += len(cnt)
            assert total == len(rows)                              # the slices partition the set
        e.set_option("key_part", 0)
        e.set_option("key_parts", 1)


# ---------------------------------------------------------------------------------------------------------------------
# f. absent probes that pass the sieve
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ("lds", "l2"))
@pytest.mark.parametrize("k", KS)
def test_sieve_survivors_miss(k, form):
    rng = np.random.default_rng(7000 + k)
    W = T.W_of(k)
    n_pairs = 32
    n = 2 * n_pairs
    words = T.sieve_words(n, l2_bits(n) if form == "l2" else 32)
    assert (words > 8192) == (form == "l2")
    # (T.sieve_words restates the engine's sizing rule -- no stat tells the real word count.  Should the engine size its
    # sieve otherwise, part of the probes below would no longer survive it and the test would pass with less power: the
    # "all survive" assertion below holds against the truth's sieve only.)
    lw = log2(words)
    low_n = 12 + lw                                                # the hash bits the sieve reads
    # stored keys in pairs (a, b) of one sieve word with four different bits
    word = rng.permutation(words)[:n_pairs]
    bits = np.array([rng.permutation(64)[:4] for _ in range(n_pairs)])
    low_a = (word << 12) | (bits[:, 1] << 6) | bits[:, 0]
    low_b = (word << 12) | (bits[:, 3] << 6) | bits[:, 2]
    h_st = np.concatenate([T.hash_with(rng, n_pairs, low22=low_a, low_nbits=low_n), T.hash_with(rng, n_pairs, low22=low_b, low_nbits=low_n)])
    stored = T.rows_with_hash(h_st, k, n, rng, canonical=True)
    # absent probes that the sieve lets through, per stored key a: its own low bits; one bit of a and one of b; twice a's first bit
    lows = np.concatenate([low_a, (word << 12) | (bits[:, 3] << 6) | bits[:, 0], (word << 12) | (bits[:, 0] << 6) | bits[:, 0]])
    of = np.concatenate([np.arange(n_pairs)] * 3)                   # the stored key (a) each probe is aimed at
    with engine_for_form(k, form, n) as e:
        e.load_filter(stored)
        lc, _ = geometry(e)
        wmask = words - 1
        sv = np.zeros(words, np.uint64)                             # the sieve of the stored keys, by the truth
        w, b1, b2 = T.sieve_word_bits(h_st, wmask)
        np.bitwise_or.at(sv, w.astype(np.int64), (np.uint64(1) << b1) | (np.uint64(1) << b2))
        # once on the stored key's home slot with its top word, once elsewhere
        h_home = T.hash_with(rng, len(lows), top_bits=T.home(h_st[of], lc), nbits=lc, low22=lows, low_nbits=low_n)
        h_away = T.hash_with(rng, len(lows), low22=lows, low_nbits=low_n)
        p_home = T.rows_with_hash(h_home, k, len(lows), rng, share="top", canonical=True, top=stored[of, W - 1])
        p_away = T.rows_with_hash(h_away, k, len(lows), rng, canonical=True)
        probes = np.concatenate([p_home, p_away])
        hp = T.long_hash(probes)
        w, b1, b2 = T.sieve_word_bits(hp, wmask)
        assert (((sv[w.astype(np.int64)] >> b1) & (sv[w.astype(np.int64)] >> b2) & np.uint64(1)) == 1).all()   # all survive
        assert np.array_equal(T.home(hp[:len(lows)], lc), T.home(h_st[of], lc)) and (p_home[:, W - 1] == stored[of, W - 1]).all()
        assert not set(map(tuple, probes.tolist())) & set(map(tuple, stored.tolist()))
        reps = 1 + np.arange(n) % 3
        reads = kmer_reads(stored, k, reps) + kmer_reads(probes, k, np.ones(len(probes), int))
        st = ReadStream.from_strings(reads)
        e.count_filtered(st)
        check_form(e, form, "count")
        assert e.stats()[2] == len(reads)
        check_table(e, stored, reps.astype(np.uint32), probes, f"k={k} {form}: count --if")
        hits, dist = e.scan(st)
        check_form(e, form, "scan")
        n_st = int(reps.sum())
        assert dist[:n_st].tolist() == [1] * n_st and not dist[n_st:].any()
        want_bits = np.zeros(len(hits) * 64, bool)
        want_bits[np.asarray(st.offsets[:n_st], np.int64)] = True
        assert np.array_equal(hits, np.packbits(want_bits, bitorder="little").view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------
# g. the W-word sort
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_sorted_dump_decided_by_every_word(k):
    import torch
    rng = np.random.default_rng(8000 + k)
    W, tb = T.W_of(k), T.top_width(k)
    fam = []
    for j in range(W):
        r = T.random_rows(rng, k, 200)
        r[:, j + 1:] = r[0, j + 1:]                                # equal in every word above j
        flips = (0, tb - 1) if j == W - 1 else (0, 31, 32, 63)
        pairs = r[:len(flips)].copy()
        for i, b in enumerate(flips):
            pairs[i, j] ^= np.uint64(1 << b)
        fam += [r, pairs]
    rows = np.unique(np.concatenate(fam), axis=0)
    rows = rows[rng.permutation(len(rows))]
    assert T.valid_rows(rows, k).all() and len(rows) > 200 * W
    cs = rng.integers(0, 4, len(rows)).astype(np.uint32)
    with KmerEngine(k, capacity_hint=1) as e:
        e.add_pairs(rows, None, cs)
        for mc in (0, 2):
            want_rows, want_cnt = T.sort_rows(rows[cs >= mc], cs[cs >= mc])
            keys, _, cnt = e.export_ge(mc)
            assert np.array_equal(keys, want_rows) and np.array_equal(cnt, want_cnt), f"export_ge({mc})"
            m = len(want_cnt)
            dk = torch.full((m * W * 8 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            dc = torch.full((m * 4 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            got = e.export_ge_dev(mc, dk.data_ptr(), None, dc.data_ptr(), m, sorted_=True)
            torch.cuda.synchronize()
            hk, hc = dk.cpu().numpy(), dc.cpu().numpy()
            assert got == m and (hk[m * W * 8:] == 0xA5).all() and (hc[m * 4:] == 0xA5).all()
            assert np.array_equal(hk[:m * W * 8].view(np.uint64).reshape(m, W), want_rows), f"export_ge_dev({mc}, sorted)"
            assert np.array_equal(hc[:m * 4].view(np.uint32), want_cnt)
