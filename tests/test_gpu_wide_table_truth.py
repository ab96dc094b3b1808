"""The wide-key table (33 <= k <= 63) under CHOSEN full hashes, against tests/merge_truth.py and tests/kmer_truth.py.

A wide key is stored as (h, hi) with h = mix64(lo ^ rot_hi(hi)); unlike a narrow key's, that h is no bijection of the key:
any hi1 != hi2 with lo2 = lo1 ^ rot_hi(hi1) ^ rot_hi(hi2) share all 64 bits of h.  Random keys never do, so with them the
`chi == khi` / `clo == klo` compares of kdf_find_wide / kdf_try_add_wide, the "another key with the same 64-bit hash: probe
on" branches of kernel C (straight-line path and kb_probe_wide_once), of km_probe_wide_once and of the heavy-bucket
kernels, and the branches for a hash word that equals the empty marker never decide.  Here the keys are written down:
groups of 2, 3, 65 and 300 keys with ONE hash (merge_truth.collision_group), their mirror -- one hi, one home slot,
different h (merge_truth.keys_sharing_hi) -- a bucket filled to its last slot by one hash, and the canonical key whose
hash IS the empty marker, through every path that stores, counts, probes, dumps, merges or joins.  Every comparison is
exact; capacity and bucket_bits are read from the engine; every expectation comes from the construction (one read per
occurrence, exactly k bases) or from kmer_truth, never from another call into the engine; device output buffers are
longer than needed and pre-filled with a canary."""
import numpy as np
import pytest

import join_truth as J
import kmer_truth as KT
import merge_truth as MT

pytestmark = pytest.mark.gpu

KS = (33, 41, 47, 63)
GROUP_SIZES = (300, 65, 3, 2)                # (the big one first: its members get the small multiplicities below)
U32_MAX = MT.U32_MAX
GUARD = 256
CANARY64 = np.uint64(0xA5A5A5A5A5A5A5A5)
CANARY32 = np.uint32(0xA5A5A5A5)
BINNED = [(2, flags, defer) for flags in (0, 8) for defer in (0, 1)]          # debug_flags 8: kernel C's plain probe loop
COUNT_PATHS = [(1, 0, 0)] + BINNED
PATH_IDS = [f"path{p}-flags{f}-defer{d}" for p, f, d in COUNT_PATHS]


# ---------------------------------------------------------------------------------------------------------------------
# keys, reads, truths
# ---------------------------------------------------------------------------------------------------------------------

def rand64(rng):
    return int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2))


def group_sizes(k, canonical):
    """k = 33 has four keys per hash, and not every one of them is canonical"""
    cap = (3 if canonical else 4) if k == 33 else max(GROUP_SIZES)
    return [min(n, cap) for n in GROUP_SIZES]


def one_group(k, n, rng, canonical):
    """(h, lo, hi): n keys with one hash.  A hash under which too few keys are canonical (k = 33) is drawn again."""
    for _ in range(500):
        h = rand64(rng)
        try:
            return (h,) + MT.collision_group(h, n, k, rng, canonical=canonical)
        except AssertionError:
            assert k == 33
    raise AssertionError(f"k={k}: no hash with {n} keys")


def make_groups(k, rng, canonical):
    groups = [one_group(k, n, rng, canonical) for n in group_sizes(k, canonical)]
    for h, lo, hi in groups:
        assert (MT.key_hash(lo, hi) == np.uint64(h)).all() and len(set(hi.tolist())) == len(hi)
    assert len({g[0] for g in groups}) == len(groups)
    return groups


def cat(parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def split(groups, held_back=1):
    """(present, absent) members: the first `held_back` of every group are absent -- same h, other hi"""
    return cat([(lo[held_back:], hi[held_back:]) for _, lo, hi in groups]), cat([(lo[:held_back], hi[:held_back]) for _, lo, hi in groups])


def halves(groups):
    return cat([(lo[::2], hi[::2]) for _, lo, hi in groups]), cat([(lo[1::2], hi[1::2]) for _, lo, hi in groups])


def pads(k, n, rng, canonical=True):
    return MT.keys_with_hash(0, 0, n, k, rng, canonical=canonical)


def kmer_reads(lo, hi, k, reps):
    """One read per occurrence, exactly k bases, every other KEY as its reverse complement."""
    out = []
    for i, (a, b, c) in enumerate(zip(lo.tolist(), hi.tolist(), np.asarray(reps).tolist())):
        s = MT.kmer_string(a, b, k)
        out += [MT.revcomp_string(s) if i & 1 else s] * int(c)
    return out


def stream(reads):
    from kmer_denovo_filter_amd import ReadStream
    return ReadStream.from_strings(reads)


def spelled(lo, hi, k):
    """the construction pinned to kmer_truth: every key is canonical, and its read (either strand) counts under it"""
    want = {a | (b << 64): 1 for a, b in zip(lo.tolist(), hi.tolist())}
    assert len(want) == len(lo) and KT.count_truth(kmer_reads(lo, hi, k, np.ones(len(lo), int)), k) == want


def by_key(lo, hi, cnt):
    """(lo, hi, cnt) in ascending (hi, lo) order, counts as uint32"""
    order = np.lexsort((lo, hi))
    return lo[order], hi[order], np.asarray(cnt)[order].astype(np.uint32)


def summed(parts):
    """the saturating key-by-key sum of (lo, hi, cnt) parts, ascending"""
    return MT.merge(parts)


def up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def geometry(e):
    return e.get_stat("log2cap"), e.get_stat("bucket_bits")


def engine(k, hint=1 << 12, path=0, flags=0, defer=None, **options):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=hint)
    if path:
        e.set_option("force_path", path)
    if flags:
        e.set_option("debug_flags", flags)
    if defer is not None:
        e.set_option("defer", defer)
    for name, v in options.items():
        e.set_option(name, v)
    return e


def dump_dev(e, min_count, n_expect, sorted_):
    """kdf_export_ge_dev into canary buffers of n_expect + GUARD entries -> (lo, hi, cnt) as written"""
    import torch
    room = n_expect + GUARD
    lo = torch.full((room,), int(CANARY64.view(np.int64)), dtype=torch.int64, device="cuda")
    hi = lo.clone()
    cnt = torch.full((room,), int(CANARY32.view(np.int32)), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = e.export_ge_dev(min_count, lo.data_ptr(), hi.data_ptr(), cnt.data_ptr(), room, sorted_=sorted_)
    e.synchronize()
    torch.cuda.synchronize()
    hl, hh, hc = lo.cpu().numpy().view(np.uint64), hi.cpu().numpy().view(np.uint64), cnt.cpu().numpy().view(np.uint32)
    assert n <= room and (hl[n:] == CANARY64).all() and (hh[n:] == CANARY64).all() and (hc[n:] == CANARY32).all(), "entries past the reported size were written"
    return hl[:n], hh[:n], hc[:n]


def same(got, want, tag):
    assert len(got[0]) == len(want[0]), f"{tag}: {len(got[0])} entries, the truth has {len(want[0])}"
    for g, w, name in zip(got, want, ("lo", "hi", "count")):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{tag}: {name} differs at entry {bad[0]} (of {bad.size}): {int(g[bad[0]]):#x}, truth {int(w[bad[0]]):#x}"


def check_table(e, truth, absent=None, tag=""):
    """The table holds exactly `truth` = (lo, hi, cnt): query of present and absent keys, the dump in ascending (hi, lo)
    order (host form and device form), count_ge, stats()[1] and the histogram."""
    lo, hi, cnt = by_key(*truth)
    got = e.query(lo, hi)
    bad = np.nonzero(got != cnt)[0]
    assert bad.size == 0, (f"{tag}: query of stored key {bad[0]} (h={int(MT.key_hash(lo[bad[:1]], hi[bad[:1]])[0]):#x}, hi={int(hi[bad[0]]):#x}) "
                           f"gives {got[bad[0]]}, not {cnt[bad[0]]} ({bad.size} keys differ)")
    if absent is not None and len(absent[0]):
        got = e.query(*absent)
        bad = np.nonzero(got)[0]
        assert bad.size == 0, f"{tag}: absent key {bad[0]} (hi={int(absent[1][bad[0]]):#x}) is found with count {got[bad[0]]}"
    same(e.export_ge(0), (lo, hi, cnt), tag + ": export_ge(0)")
    same(dump_dev(e, 0, len(lo), True), (lo, hi, cnt), tag + ": export_ge_dev(0, sorted)")
    m = cnt >= 2
    same(by_key(*dump_dev(e, 2, int(m.sum()), False)), (lo[m], hi[m], cnt[m]), tag + ": export_ge_dev(2)")
    for mc in (0, 1, 2, 3, U32_MAX):
        assert e.count_ge(mc) == int((cnt >= mc).sum()), f"{tag}: count_ge({mc})"
    assert e.stats()[1] == len(lo), f"{tag}: distinct"
    high = 700
    want_bins = np.bincount(np.minimum(cnt.astype(np.int64), high + 1), minlength=high + 2).astype(np.uint64)
    assert np.array_equal(e.histogram(high), want_bins), f"{tag}: histogram"


def set_counts(e, lo, hi, cnt):
    import torch
    dl, dh, dc = up(lo), up(hi), up(np.asarray(cnt, np.uint32))
    torch.cuda.synchronize()
    e.set_counts_dev(dl.data_ptr(), dh.data_ptr(), dc.data_ptr(), len(lo))


def merge_call(e, segs):
    """kdf_add_pairs_multi_dev of numpy segments (lo, hi, cnt), one call"""
    import torch
    keep, args = [], []
    for lo, hi, cnt in segs:
        t = (up(lo), up(hi), up(np.asarray(cnt, np.uint32)))
        keep.append(t)
        args.append((t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(lo)))
    torch.cuda.synchronize()
    e.add_pairs_multi_dev(args)
    e.synchronize()


def in_bucket_order(seg, e):
    lc, bb = geometry(e)
    lo, hi, cnt = seg
    order = np.argsort(MT.bucket(MT.key_hash(lo, hi), lc, bb), kind="stable")
    return lo[order], hi[order], np.asarray(cnt)[order]


# ---------------------------------------------------------------------------------------------------------------------
# 1. stored groups, insert and filter mode
# ---------------------------------------------------------------------------------------------------------------------

def stored_block(e, k, present, absent, pad, cnt_p, cnt_pad, rng, tag):
    """every check on a table that holds `present` + `pad`; -> the counts it holds afterwards"""
    lo, hi = cat([present, pad])
    cnt = np.concatenate([cnt_p, cnt_pad]).astype(np.uint32)
    check_table(e, (lo, hi, cnt), absent, tag)
    new = (5000 + rng.permutation(len(present[0]))).astype(np.uint32)      # set_counts on the present members sets exactly those
    set_counts(e, present[0], present[1], new)
    cnt = np.concatenate([new, cnt_pad]).astype(np.uint32)
    check_table(e, (lo, hi, cnt), absent, tag + ": after set_counts")
    from kmer_denovo_filter_amd._native import KdfError
    with pytest.raises(KdfError, match="not stored"):                     # an absent member of a stored hash is refused
        set_counts(e, np.concatenate([present[0][:3], absent[0][:1]]), np.concatenate([present[1][:3], absent[1][:1]]),
                   np.concatenate([new[:3], [9]]))
    check_table(e, (lo, hi, cnt), absent, tag + ": after the refused set_counts")
    return new


@pytest.mark.parametrize("filter_mode", (False, True), ids=("pairs", "filter"))
@pytest.mark.parametrize("k", KS)
def test_stored_groups(k, filter_mode):
    rng = np.random.default_rng(100 + k)
    groups = make_groups(k, rng, canonical=filter_mode)
    present, absent = split(groups)
    pad = pads(k, 300, rng, canonical=filter_mode)
    n = len(present[0])
    tag = f"k={k} {'filter' if filter_mode else 'pairs'}"
    with engine(k, hint=1) as e:
        if filter_mode:
            spelled(*cat([present, absent]), k)
            reps = 1 + np.arange(n) % 5
            e.load_filter(*cat([present, pad]))
            reads = kmer_reads(*present, k, reps) + kmer_reads(*absent, k, 1 + np.arange(len(absent[0])) % 2)
            e.count_filtered(stream(reads))
            assert e.stats()[2] == len(reads), f"{tag}: windows"
            cnt_p, cnt_pad = reps, np.zeros(len(pad[0]), np.uint32)
        else:
            cnt_p = (1 + rng.permutation(n)).astype(np.uint32)          # distinct counts, some 0, one saturated
            cnt_p[::7] = 0
            cnt_p[1] = U32_MAX
            cnt_pad = (1000 + np.arange(len(pad[0]))).astype(np.uint32)
            e.add_pairs(*cat([present, pad]), np.concatenate([cnt_p, cnt_pad]))
        cnt_p = stored_block(e, k, present, absent, pad, cnt_p, cnt_pad, rng, tag)
        # the table grows: the rehash re-inserts the stored (h, hi) pairs
        lc = geometry(e)[0]
        e.reserve(4 << lc)
        assert geometry(e)[0] > lc, f"{tag}: reserve did not rehash"
        cnt_p = stored_block(e, k, present, absent, pad, cnt_p, cnt_pad, rng, tag + " grown")
        # the held-back members join: every group whole
        ca = (20000 + np.arange(len(absent[0]))).astype(np.uint32)
        e.add_pairs(*absent, ca)
        check_table(e, (*cat([present, pad, absent]), np.concatenate([cnt_p, cnt_pad, ca])), None, tag + ": all members stored")


# ---------------------------------------------------------------------------------------------------------------------
# 2. groups counted from reads, every count path
# ---------------------------------------------------------------------------------------------------------------------

def counted_keys(k, rng, n_pads=150):
    """(groups, (lo, hi) of every key -- members first, the big group first -- and multiplicities 1, 2, 3, ...)"""
    groups = make_groups(k, rng, canonical=True)
    lo, hi = cat([(g[1], g[2]) for g in groups] + [pads(k, n_pads, rng)])
    assert len({(a, b) for a, b in zip(lo.tolist(), hi.tolist())}) == len(lo)
    spelled(lo, hi, k)
    return groups, (lo, hi), 1 + np.arange(len(lo))


def witness(e, path):
    assert e.last_count_path() == ("direct" if path == 1 else "binned")
    if path == 2:
        assert e.get_stat("replayed_buckets") == 0, "a bucket was replayed: kernel C did not do the work"
        assert geometry(e)[0] > geometry(e)[1]


@pytest.mark.parametrize("path,flags,defer", COUNT_PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("k", KS)
def test_groups_counted_from_reads(k, path, flags, defer):
    rng = np.random.default_rng(200 + k)
    groups, (lo, hi), mult = counted_keys(k, rng)
    absent = pads(k, 50, rng)
    tag = f"k={k} path={path} flags={flags} defer={defer}"
    st_all = stream(kmer_reads(lo, hi, k, mult))
    windows = int(mult.sum())
    # (a) into an empty table
    with engine(k, path=path, flags=flags, defer=defer) as e:
        e.count(st_all)
        witness(e, path)
        check_table(e, (lo, hi, mult), absent, tag + ": empty table")
        assert e.stats()[2] == windows
        witness(e, path)
    # (b) into a live table that already holds half of each group
    (elo, ehi), _ = halves(groups)
    c0 = (7000 + np.arange(len(elo))).astype(np.uint32)
    c0[0], c0[1] = U32_MAX, U32_MAX - 1                                  # saturated, and saturating under the reads
    with engine(k, path=path, flags=flags, defer=defer) as e:
        e.add_pairs(elo, ehi, c0)
        e.count(st_all)
        witness(e, path)
        check_table(e, summed([(lo, hi, mult), (elo, ehi, c0)]), absent, tag + ": live table")
        witness(e, path)
    # (c) two passes that hold different members of every group (and the pads in both)
    m1 = np.arange(len(lo)) % 2 == 0
    m2 = ~m1
    m1[-150:] = True
    m2[-150:] = True
    with engine(k, path=path, flags=flags, defer=defer) as e:
        e.count(stream(kmer_reads(lo[m1], hi[m1], k, mult[m1])))
        e.count(stream(kmer_reads(lo[m2], hi[m2], k, mult[m2])))
        if path == 2 and defer:
            assert e.get_stat("pending_passes") == 2, f"{tag}: the passes are not pending"
        witness(e, path)
        check_table(e, summed([(lo[m1], hi[m1], mult[m1]), (lo[m2], hi[m2], mult[m2])]), absent, tag + ": two passes")
        assert e.get_stat("pending_passes") == 0 and e.stats()[2] == int(mult[m1].sum() + mult[m2].sum())
        witness(e, path)


# ---------------------------------------------------------------------------------------------------------------------
# 3. count --if
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", (1, 2, 4), ids=("direct", "binned", "sieve"))
@pytest.mark.parametrize("k", KS)
def test_count_filtered_groups(k, path):
    """The filter holds the even members of every group, the reads spell all of them: an odd member shares h with a stored
    key (it passes the sieve, it finds its h in the slice) and must count nothing, neither for itself nor for another key."""
    rng = np.random.default_rng(300 + k)
    groups, (lo, hi), mult = counted_keys(k, rng)
    (flo, fhi), (olo, ohi) = halves(groups)
    plo, phi = lo[-150:], hi[-150:]
    filt = cat([(flo, fhi), (plo[::2], phi[::2])])
    want = KT.count_truth(kmer_reads(lo, hi, k, np.ones(len(lo), int)), k, [a | (b << 64) for a, b in zip(filt[0].tolist(), filt[1].tolist())])
    in_filter = np.array([(a | (b << 64)) in want for a, b in zip(lo.tolist(), hi.tolist())])
    assert in_filter.sum() == len(filt[0]) == len(want)                 # (the truth's filter rule is the construction's)
    cnt = {a | (b << 64): int(c) for a, b, c in zip(lo[in_filter].tolist(), hi[in_filter].tolist(), mult[in_filter].tolist())}
    fcnt = np.array([cnt[a | (b << 64)] for a, b in zip(filt[0].tolist(), filt[1].tolist())], np.uint32)
    st = stream(kmer_reads(lo, hi, k, mult))
    with engine(k, hint=1 << 12) as e:
        e.load_filter(*filt)
        e.reserve(1 << 12)
        assert geometry(e)[0] > geometry(e)[1]
        e.set_option("force_path", path)
        e.count_filtered(st)
        assert e.last_count_path() == {1: "direct", 2: "binned", 4: "sieve"}[path]
        check_table(e, (*filt, fcnt), cat([(olo, ohi), (plo[1::2], phi[1::2])]), f"k={k} count --if path {path}")
        assert e.stats()[2] == int(mult.sum())
        e.count_filtered(st)                                            # and once more into the counts
        check_table(e, (*filt, 2 * fcnt), (olo, ohi), f"k={k} count --if path {path}, second batch")


# ---------------------------------------------------------------------------------------------------------------------
# 4. probes
# ---------------------------------------------------------------------------------------------------------------------

FORMS = {"direct": (300, None), "lds": (300, None), "sat": (21_000, 1), "l2": (17_000, 32), "l2def": (66_000, None)}   # pads stored, sieve_bits


def window_truth(reads, k, index):
    """per read: the stored count of every valid window's canonical key (absent or stored with 0: 0), by position"""
    from oracle import oracle as O
    out = []
    for s in reads:
        S, run, row = s.upper(), 0, []
        for j, ch in enumerate(S):
            run = run + 1 if ch in "ACGT" else 0
            if run >= k:
                row.append((j - k + 1, KT.key_int(O.canonicalize(S[j - k + 1:j + 1]))))
        out.append([(i, v, index.get(v, 0)) for i, v in row])
    return out


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("k", KS)
def test_groups_probed_by_reads(k, form):
    """A is stored with a count, B with count 0, C is absent; all three share one h."""
    from kmer_denovo_filter_amd.reads import stream_words
    rng = np.random.default_rng(400 + k)
    groups = make_groups(k, rng, canonical=True)
    A, B, C = [], [], []
    for _, lo, hi in groups:
        third = max(1, len(lo) // 3)
        A.append((lo[:third], hi[:third]))
        B.append((lo[third:2 * third], hi[third:2 * third]))
        C.append((lo[2 * third:], hi[2 * third:]))
    A, B, C = cat(A), cat(B), cat(C)
    assert len(A[0]) and len(B[0]) and len(C[0])
    n_pads, sieve_bits = FORMS[form]
    pad = pads(k, n_pads, rng, canonical=False)
    ca = (1 + np.arange(len(A[0]))).astype(np.uint32)
    index = {a | (b << 64): int(c) for a, b, c in zip(A[0].tolist(), A[1].tolist(), ca.tolist())}
    members = cat([A, B, C])
    spelled(*members, k)
    fl = lambda n: "".join(rng.choice(list("ACGT"), n))                 # noqa: E731
    s = lambda keys, i: MT.kmer_string(int(keys[0][i]), int(keys[1][i]), k)   # noqa: E731
    reads = kmer_reads(*members, k, np.ones(len(members[0]), int))
    for i in range(min(4, len(A[0]), len(B[0]), len(C[0]))):           # overlapping inside longer reads, both strands
        reads += [fl(11) + s(A, i) + s(B, i) + fl(7), s(C, i) + MT.revcomp_string(s(A, i)) + "N" + s(A, i)[1:],
                  fl(5) + MT.revcomp_string(s(B, i)) + s(C, i) + s(A, i) + s(A, i), s(A, i)[:-1], s(A, i).lower()]
    st = stream(reads)
    wt = window_truth(reads, k, index)
    hits_truth, dist_truth = KT.scan_truth(reads, k, index)
    assert [[i for i, _, c in row if c] for row in wt] == hits_truth    # (two readings of one rule)
    n_words = stream_words(st.n_bases)[1]
    want_bits = KT.hit_words(st.offsets, hits_truth, n_words)
    want_hits = np.array([len(p) for p in hits_truth], np.uint32)
    assert int(want_hits.sum()) >= len(A[0]) and int(dist_truth.max()) == 1 and int(want_hits.max()) >= 2   # A counted once however often it is hit
    with engine(k, hint=1 << 12, path=1 if form == "direct" else 0) as e:
        if sieve_bits is not None:
            e.set_option("sieve_bits", sieve_bits)
        e.add_pairs(*cat([A, B, pad]), np.concatenate([ca, np.zeros(len(B[0]), np.uint32), np.ones(n_pads, np.uint32)]))
        hits, dist = e.scan(st)
        assert e.get_stat("last_scan_path") == (0 if form == "direct" else 3)
        if form in ("lds", "l2", "l2def"):
            assert e.get_stat("last_sieve_in_lds") == (1 if form == "lds" else 0)
        assert np.array_equal(hits[:n_words], want_bits), f"k={k} {form}: hit words"
        assert np.array_equal(dist, dist_truth), f"k={k} {form}: distinct per read"
        rh, bits = e.read_hits(st, want_bits=True)
        assert np.array_equal(bits[:n_words], want_bits) and np.array_equal(rh[:, 0], want_hits) and np.array_equal(rh[:, 1], dist_truth)
        wc = e.window_counts(st)
        want_wc = np.zeros(st.n_bases, np.uint32)
        for r, row in enumerate(wt):
            for i, _, c in row:
                want_wc[int(st.offsets[r]) + i] = c
        assert np.array_equal(wc, want_wc), f"k={k} {form}: window_counts"
        rd = e.read_depth(st, 0)
        want_rd = np.array([[len(row), sum(1 for x in row if x[2]), sum(1 for x in row if x[2] == 0), min([x[2] for x in row] or [0]),
                             max([x[2] for x in row] or [0]), sum(x[2] for x in row)] for row in wt], np.uint64)
        assert np.array_equal(rd, want_rd), f"k={k} {form}: read_depth"
        pos = e.hit_list(hits, st.n_bases)
        want_keys = [v for r, row in enumerate(wt) for i, v, c in row if c]
        want_pos = [int(st.offsets[r]) + i for r, row in enumerate(wt) for i, v, c in row if c]
        assert pos.tolist() == want_pos
        hk = e.hit_keys(st, pos)
        assert [int(a) | (int(b) << 64) for a, b in hk.tolist()] == want_keys and set(want_keys) <= set(index)
        assert not e.query(*C).any() and not e.query(*B).any() and np.array_equal(e.query(*A), ca)


# ---------------------------------------------------------------------------------------------------------------------
# 5. dumps that leave from kernel C
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_dumps_out_of_kernel_c(k):
    rng = np.random.default_rng(500 + k)
    groups, (lo, hi), mult = counted_keys(k, rng)
    m1 = np.arange(len(lo)) % 3 != 0
    st1, st2 = stream(kmer_reads(lo[m1], hi[m1], k, mult[m1])), stream(kmer_reads(lo, hi, k, mult))
    both = summed([(lo[m1], hi[m1], mult[m1]), (lo, hi, mult)])
    # the fused dump: one pass applied, one pending when the dump comes -- into a live table
    for mc in (1, 400):
        with engine(k, hint=1 << 14, path=2, fused_dump=1) as e:
            e.count(st1)
            assert e.count_ge(1) == int(m1.sum())
            e.count(st2)
            assert e.get_stat("pending_passes") == 1
            keep = both[2] >= mc
            same(dump_dev(e, mc, int(keep.sum()), True), (both[0][keep], both[1][keep], both[2][keep]), f"k={k}: fused dump -L {mc}")
            assert e.get_stat("fused_dumps") == 1 and e.get_stat("pending_passes") == 0 and e.get_stat("replayed_buckets") == 0
            check_table(e, both, None, f"k={k}: the table after the fused dump")
    # count-then-dump: clear -> count -> dump writes the dump out of kernel C and leaves the table unwritten
    with engine(k, hint=1 << 14, path=2, fused_dump=1, lazy_table=1) as e:
        e.clear()
        e.count(st2)
        same(by_key(*dump_dev(e, 2, len(lo) - 1, False)), by_key(lo[1:], hi[1:], mult[1:]), f"k={k}: dump-only flush")
        assert (e.get_stat("dump_only_flushes"), e.get_stat("materialisations"), e.get_stat("fused_dumps")) == (1, 0, 1)
        check_table(e, (lo, hi, mult), None, f"k={k}: the table after the dump-only flush")
        assert e.get_stat("materialisations") == 1 and e.get_stat("replayed_buckets") == 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. the key whose hash word is the empty marker
# ---------------------------------------------------------------------------------------------------------------------

def empty_hash_key(k, rng):
    lo, hi = MT.collision_group(MT.EMPTY, 1, k, rng, canonical=True)
    assert int(MT.key_hash(lo, hi)[0]) == MT.EMPTY and int(lo[0]) == int(MT.unmix64(MT.EMPTY)) ^ int(MT.rot_hi(hi[0]))
    return lo, hi


def empty_case(k, seed):
    """(the key, all keys = the key + pads, multiplicities, the stream that spells them)"""
    rng = np.random.default_rng(seed + k)
    key = empty_hash_key(k, rng)
    lo, hi = cat([key, pads(k, 200, rng)])
    spelled(lo, hi, k)
    mult = 5 + np.arange(len(lo))
    return key, (lo, hi), mult, stream(kmer_reads(lo, hi, k, mult))


@pytest.mark.parametrize("k", (33, 47, 63))
def test_empty_marker_hash_stored_and_counted(k):
    key, (lo, hi), mult, st = empty_case(k, 600)
    absent = pads(k, 50, np.random.default_rng(k))
    with engine(k, hint=1) as e:                                        # add_pairs, query, export: lo comes back from (~0, hi)
        e.add_pairs(lo, hi, mult.astype(np.uint32))
        check_table(e, (lo, hi, mult), absent, f"k={k}: add_pairs")
        glo, ghi, _ = e.export_ge(0)
        want_lo = np.uint64(int(MT.unmix64(MT.EMPTY)) ^ int(MT.rot_hi(key[1][0])))
        assert int(((ghi == key[1][0]) & (glo == want_lo)).sum()) == 1
    with engine(k, path=1) as e:                                        # a direct count
        e.count(st)
        assert e.last_count_path() == "direct"
        check_table(e, (lo, hi, mult), absent, f"k={k}: direct count")
    for flags in (0, 8):
        with engine(k, path=2, flags=flags) as e:                       # binned, the key enters as a stream window: its bucket is replayed
            e.count(st)
            assert e.last_count_path() == "binned"
            check_table(e, (lo, hi, mult), absent, f"k={k}: binned count, flags {flags}")
            assert e.get_stat("replayed_buckets") >= 1
        with engine(k, path=2, flags=flags) as e:                       # ... and already stored when kernel C loads its bucket
            e.add_pairs(*key, np.array([9], np.uint32))
            e.count(st)
            assert e.last_count_path() == "binned"
            check_table(e, summed([(lo, hi, mult), (*key, [9])]), absent, f"k={k}: binned count into a table that holds the key, flags {flags}")
            assert e.get_stat("replayed_buckets") >= 1
    with engine(k, hint=1 << 14, path=2, fused_dump=1, lazy_table=1) as e:            # count-then-dump falls back and is still exact
        e.clear()
        e.count(st)
        same(by_key(*dump_dev(e, 1, len(lo), False)), by_key(lo, hi, mult), f"k={k}: count-then-dump")
        assert e.get_stat("dump_only_flushes") == 0 and e.get_stat("replayed_buckets") >= 1
        check_table(e, (lo, hi, mult), absent, f"k={k}: the table after count-then-dump")


@pytest.mark.parametrize("k", (33, 47, 63))
def test_empty_marker_hash_merged_and_joined(k):
    key, (lo, hi), mult, _ = empty_case(k, 650)
    c = mult.astype(np.uint32)
    with engine(k, hint=1 << 12, merge_min_pairs=1) as e:
        segs = [(lo, hi, c), (lo[:50], hi[:50], c[:50]), (lo[::3], hi[::3], np.full(len(lo[::3]), 0x60000000, np.uint32))]
        merge_call(e, [in_bucket_order(s, e) for s in segs])
        assert e.get_stat("last_merge_path") == 1
        truth = summed(segs)
        check_table(e, truth, None, f"k={k}: merge into a fresh table")
        merge_call(e, [in_bucket_order(s, e) for s in segs[:2]])        # and into the live one
        truth = summed([truth] + segs[:2])
        check_table(e, truth, None, f"k={k}: merge into a live table")
        assert int(e.query(*key)[0]) == min(U32_MAX, 4 * 5 + 0x60000000)
    # the join: A holds the key and the pads, B the key and every other pad
    ka = J.keys_of(lo, hi)
    kb, cb = ka[::2], (3 + np.arange(len(ka[::2])) % 4).tolist()
    with engine(k, hint=1) as a, engine(k, hint=1) as b:
        a.add_pairs(lo, hi, c)
        b.add_pairs(lo[::2], hi[::2], np.array(cb, np.uint32))
        for bounds in ((1, None, 0, 0), (1, None, 1, None), (5, 5, 3, 3), (0, None, 0, None)):
            want = J.join(ka, c.tolist(), kb, cb, *bounds)
            keys, cnt, oc = a.export_join(b, *bounds)
            assert (J.keys_of(keys[0], keys[1]), cnt.tolist(), oc.tolist()) == want, f"k={k} join {bounds}"
            assert a.count_join(b, *bounds) == len(want[0])
        assert J.join(ka, c.tolist(), kb, cb, 5, 5, 3, 3)[0] == [ka[0]]  # (the key itself, selected by both of its counts)


@pytest.mark.parametrize("k", (33, 47, 63))
def test_empty_marker_hash_in_a_binned_count_filtered(k):
    """count --if on the binned path with the key in the filter and in the reads: what the direct path gives, which is the
    truth's.  Kernel C cannot hold a stored hash word equal to the empty marker in its slice and flags the bucket; filter
    mode replays a flagged bucket through the direct filtered probe, as insert mode replays one through the direct insert."""
    key, (lo, hi), mult, st = empty_case(k, 680)
    sel = np.arange(len(lo)) % 2 == 0                                   # the key and every other pad
    filt = (lo[sel], hi[sel])
    want = KT.count_truth(kmer_reads(lo, hi, k, np.ones(len(lo), int)), k, [a | (b << 64) for a, b in zip(filt[0].tolist(), filt[1].tolist())])
    assert set(want) == {a | (b << 64) for a, b in zip(filt[0].tolist(), filt[1].tolist())} and int(key[0][0]) | (int(key[1][0]) << 64) in want
    got = {}
    for path in (1, 2):
        with engine(k, hint=1 << 12) as e:
            e.load_filter(*filt)
            e.reserve(1 << 12)
            assert geometry(e)[0] > geometry(e)[1]
            e.set_option("force_path", path)
            e.count_filtered(st)
            assert e.last_count_path() == ("direct" if path == 1 else "binned")
            check_table(e, (*filt, mult[sel]), (lo[~sel], hi[~sel]), f"k={k}: count --if path {path}")
            assert e.stats()[2] == int(mult.sum())
            e.count_filtered(st)
            check_table(e, (*filt, 2 * mult[sel]), (lo[~sel], hi[~sel]), f"k={k}: count --if path {path}, second batch")
            got[path] = e.export_ge(0)
    same(got[2], got[1], f"k={k}: binned against direct")


# ---------------------------------------------------------------------------------------------------------------------
# 7. a bucket filled to its last slot by one hash
# ---------------------------------------------------------------------------------------------------------------------

def store(e, how, lo, hi, cnt, k):
    """B keys into engine e by one of the four ways"""
    if how == "pairs":
        e.add_pairs(lo, hi, cnt.astype(np.uint32))
    elif how == "merge":
        e.set_option("merge_min_pairs", 1)
        merge_call(e, [(lo, hi, cnt)])
    else:
        e.set_option("force_path", 1 if how == "direct" else 2)
        e.count(stream(kmer_reads(lo, hi, k, cnt)))
        e.flush()


@pytest.mark.parametrize("k", (41, 63))
def test_a_bucket_filled_by_one_hash(k):
    from kmer_denovo_filter_amd._native import KDF_ERR_TABLE_FULL, KdfError
    rng = np.random.default_rng(700 + k)
    with engine(k, hint=1 << 12) as e:
        lc, bb = geometry(e)
        assert lc > bb
        B = 1 << bb
        h = rand64(rng)
        lo, hi = MT.collision_group(h, B + 1, k, rng, canonical=True)
        absent = pads(k, 50, rng)
        cnt = 1 + np.arange(B) % 3
        for how in ("pairs", "direct", "binned", "merge"):
            e.clear()
            store(e, how, lo[:B], hi[:B], cnt, k)                      # every probe run is B long and wraps
            assert geometry(e)[1] == bb
            check_table(e, (lo[:B], hi[:B], cnt), (np.concatenate([lo[B:], absent[0]]), np.concatenate([hi[B:], absent[1]])), f"k={k} {how}: B keys of one hash")
        for how in ("pairs", "direct", "binned", "merge"):            # one key more fits nowhere: a designed error, no hang
            e.clear()
            with pytest.raises(KdfError) as ei:
                store(e, how, lo, hi, np.ones(B + 1, int), k)
            assert ei.value.code == KDF_ERR_TABLE_FULL, f"k={k} {how}: {ei.value}"
            if how == "binned":
                assert geometry(e)[0] > lc                              # (it grew the table, replayed, and the bucket was still full)
        e.clear()
        e.set_option("force_path", 0)
        plo, phi = pads(k, 100, rng)
        mult = 1 + np.arange(100)
        e.count(stream(kmer_reads(plo, phi, k, mult)))
        check_table(e, (plo, phi, mult), (lo[:50], hi[:50]), f"k={k}: after clear()")


# ---------------------------------------------------------------------------------------------------------------------
# 8. same hi, different lo, one home slot
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ("pairs", "direct", "binned", "merge"))
@pytest.mark.parametrize("k", (33, 47))
def test_one_hi_one_home_slot(k, how):
    rng = np.random.default_rng(800 + k)
    lo, hi = MT.keys_sharing_hi(int(rng.integers(0, 1 << 20)), 20, 60, k, rng, canonical=True)
    h = MT.key_hash(lo, hi)
    assert len(set(hi.tolist())) == 1 and len(set(h.tolist())) == 60 and len(set(MT.home(h, 20).tolist())) == 1
    spelled(lo, hi, k)
    plo, phi = pads(k, 200, rng)
    present, absent = (lo[:40], hi[:40]), (lo[40:], hi[40:])
    klo, khi = cat([present, (plo, phi)])
    mult = 1 + np.arange(len(klo))
    with engine(k, hint=1 << 12) as e:
        store(e, how, klo, khi, mult, k)
        check_table(e, (klo, khi, mult), absent, f"k={k} {how}")
        store(e, how, *absent, 500 + np.arange(20), k)                  # the others join, into the live table
        check_table(e, (*cat([(klo, khi), absent]), np.concatenate([mult, 500 + np.arange(20)])), None, f"k={k} {how}: all members")


# ---------------------------------------------------------------------------------------------------------------------
# 9. two heavy keys with one hash
# ---------------------------------------------------------------------------------------------------------------------

def test_two_heavy_keys_with_one_hash():
    """Two members of one group, 45 000 reads each, and 10 000 reads of pads: one bucket holds nine tenths of a skewed
    pass and is left to kb_heavy_slice_kernel / kb_heavy_combine_kernel, whose private tables and fold compare (h, hi)."""
    k = 47
    rng = np.random.default_rng(900)
    _, glo, ghi = one_group(k, 3, rng, canonical=True)
    plo, phi = pads(k, 2000, rng)
    lo, hi = cat([(glo[:2], ghi[:2]), (plo, phi)])
    mult = np.concatenate([[45_000, 44_999], np.full(2000, 5)])
    reads = kmer_reads(lo, hi, k, mult)
    assert len(reads) <= 100_000
    reads = [reads[i] for i in rng.permutation(len(reads))]
    st = stream(reads)
    with engine(k, hint=1 << 22, path=2) as e:
        e.count(st)                                                     # the engine has now seen a skewed pass
        e.clear()
        e.count(st)
        check_table(e, (lo, hi, mult), (glo[2:], ghi[2:]), "two heavy keys")
        assert e.get_stat("heavy_buckets") > 0, "no bucket was split: the test does not reach the heavy-bucket kernels"
