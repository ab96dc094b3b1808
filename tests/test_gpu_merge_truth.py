"""The eight kernels of csrc/kdf_merge.h (the multi-GPU count for k <= 63) on ONE GPU against tests/merge_truth.py:
the dump grouped by owner rank (kdf_export_parts_dev, kdf_export_parts_packed_dev) and the owners' merge of what the
source ranks send (kdf_add_pairs_multi_dev).  Tables are filled with kdf_add_pairs_dev from chosen keys -- no reads --
so every expectation is the truth's, never another dump of the engine.  Every comparison is exact equality; every
output buffer is longer than needed and pre-filled with a canary."""
import numpy as np
import pytest

import merge_truth as T

pytestmark = pytest.mark.gpu

KS = (31, 63)
PARTS = (1, 2, 3, 5, 6, 7, 8, 17, 64)
SENDER_LOG2CAP = 28                          # the smallest table the owner-ordered dump takes
GUARD = 512                                  # entries (plain dump) / bytes (packed dump) behind every output buffer
CANARY = 0xA5
CANARY64 = np.uint64(0xA5A5A5A5A5A5A5A5)
CANARY32 = np.uint32(0xA5A5A5A5)
U32_MAX = T.U32_MAX


# ---- plumbing ---------------------------------------------------------------------------------------------------------

def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda")


def fill(e, lo, hi, cnt):
    """kdf_add_pairs_dev of one array of pairs (cnt None: NULL counts)."""
    import torch
    if len(lo) == 0:
        return
    dlo, dhi = to_dev(lo), (to_dev(hi) if hi is not None else None)
    dc = to_dev(np.asarray(cnt, dtype=np.uint32)) if cnt is not None else None
    torch.cuda.synchronize()
    e.add_pairs_dev(dlo.data_ptr(), dhi.data_ptr() if dhi is not None else None, dc.data_ptr() if dc is not None else None, len(lo))
    e.synchronize()


def at_least(truth, min_count):
    lo, hi, cnt = truth
    m = cnt >= np.uint32(min_count) if min_count else np.ones(len(cnt), bool)
    return lo[m], (hi[m] if hi is not None else None), cnt[m]


def same_pairs(got, want):
    g, w = T.sorted_triples(*got), T.sorted_triples(*want)
    assert len(g[0]) == len(w[0]), f"{len(g[0])} pairs, the truth has {len(w[0])}"
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[2], w[2]) and (w[1] is None or np.array_equal(g[1], w[1]))


def dump_plain(e, parts, min_count, n_expect, cap=None):
    """kdf_export_parts_dev into canary buffers of n_expect + GUARD entries -> (n, counts, lo, hi, cnt)."""
    import torch
    room = n_expect + GUARD
    cap = room - GUARD if cap is None else cap
    lo = torch.full((room,), int(CANARY64.view(np.int64)), dtype=torch.int64, device="cuda")
    hi = lo.clone() if e.wide else None
    cnt = torch.full((room,), int(CANARY32.view(np.int32)), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = None
    try:
        n, counts = e.export_parts_dev(min_count, parts, lo.data_ptr(), hi.data_ptr() if hi is not None else None, cnt.data_ptr(), cap)
    finally:
        e.synchronize()
        torch.cuda.synchronize()
        end = cap if n is None else n
        hl = lo.cpu().numpy().view(np.uint64)
        hh = hi.cpu().numpy().view(np.uint64) if hi is not None else None
        hc = cnt.cpu().numpy().view(np.uint32)
        assert (hl[end:] == CANARY64).all() and (hc[end:] == CANARY32).all() and (hh is None or (hh[end:] == CANARY64).all()), \
            "entries past the reported size (or past cap) were written"
    return n, counts, hl[:n], (hh[:n] if hh is not None else None), hc[:n]


def dump_packed(e, parts, min_count, n_expect, cap_bytes=None):
    """kdf_export_parts_packed_dev into a canary buffer -> (n, counts, offs, [(lo, hi, cnt) per part])."""
    import torch
    esz = 20 if e.wide else 12
    room = n_expect * esz + 8 * parts + GUARD
    cap_bytes = room - GUARD if cap_bytes is None else cap_bytes
    buf = torch.full((room,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs = None
    try:
        n, counts, offs = e.export_parts_packed_dev(min_count, parts, buf.data_ptr(), cap_bytes)
    finally:
        e.synchronize()
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        end = cap_bytes if offs is None else offs[parts]
        assert (host[end:] == CANARY).all(), "bytes past part_bytes_out[parts] (or past cap_bytes) were written"
    segs = []
    for p in range(parts):
        a, m = offs[p], counts[p]
        lo = host[a:a + 8 * m].view(np.uint64).copy()
        a += 8 * m
        hi = None
        if e.wide:                                                     # the counts come after hi
            hi = host[a:a + 8 * m].view(np.uint64).copy()
            a += 8 * m
        segs.append((lo, hi, host[a:a + 4 * m].view(np.uint32).copy()))
    return n, counts, offs, segs


def describe_descent(h, i, log2cap):
    blk = lambda x: int(x) >> (64 - (log2cap - 12))
    return (f"dump entry {i} has hash {int(h[i]):#018x} (home block {blk(h[i])}, home slot {int(h[i]) >> (64 - log2cap)}) "
            f"behind entry {i - 1} of home block {blk(h[i - 1])}; the next entry's home block is {blk(h[min(i + 1, len(h) - 1)])}")


def check_dump(e, parts, min_count, truth, log2cap=SENDER_LOG2CAP):
    """Both dumps of the table against the truth (lo, hi, cnt): multiset, per-part counts, owners, order, packed layout."""
    want = at_least(truth, min_count)
    wn = len(want[0])
    wown = T.owner(T.key_hash(want[0], want[1]), parts).astype(np.int64)
    wcounts = np.bincount(wown, minlength=parts).tolist()
    n, counts, lo, hi, cnt = dump_plain(e, parts, min_count, wn)
    tag = f"parts={parts} min_count={min_count}"
    assert n == wn == sum(counts), tag
    same_pairs((lo, hi, cnt), want)
    assert counts == wcounts, tag
    h = T.key_hash(lo, hi)
    own = T.owner(h, parts).astype(np.int64)
    part_of = np.repeat(np.arange(parts), counts)
    wrong = np.nonzero(own != part_of)[0]
    pre = T.order_key(h, log2cap)
    down = np.nonzero(pre[1:] < pre[:-1])[0]
    said = []                                                          # both findings in one message
    if wrong.size:
        i = int(wrong[0])
        said.append(f"{wrong.size} entries lie in another owner's part; first: entry {i} of owner {own[i]}, hash {int(h[i]):#018x}, "
                    f"home slot {int(h[i]) >> (64 - log2cap)}, lies in part {part_of[i]}")
    if down.size:
        said.append(f"the dump is not in hash order at {down.size} places; first: {describe_descent(h, int(down[0]) + 1, log2cap)}")
    assert not said, f"{tag}: " + "; ".join(said)
    # the packed dump: per part the same triples, starts on multiples of 8, the last offset = the bytes used
    pn, pcounts, offs, segs = dump_packed(e, parts, min_count, wn)
    esz = 20 if e.wide else 12
    assert pn == wn and pcounts == wcounts and len(offs) == parts + 1 and offs[0] == 0, tag
    a = 0
    for p in range(parts):
        assert offs[p] % 8 == 0 and offs[p + 1] - offs[p] == (counts[p] * esz + 7) // 8 * 8, tag
        same_pairs(segs[p], (lo[a:a + counts[p]], hi[a:a + counts[p]] if hi is not None else None, cnt[a:a + counts[p]]))
        a += counts[p]
    plo = np.concatenate([s[0] for s in segs])
    phi = np.concatenate([s[1] for s in segs]) if e.wide else None
    ppre = T.order_key(T.key_hash(plo, phi), log2cap)
    assert np.all(ppre[1:] >= ppre[:-1]), f"{tag}: the packed dump is not in hash order"
    return counts


def grid(e, truth, min_counts):
    for parts in PARTS:
        for mc in min_counts:
            check_dump(e, parts, mc, truth)


def random_keys(rng, k, n):
    return T.keys_with_hash(0, 0, n, k, rng)


@pytest.fixture(scope="module")
def senders():
    """One 2^28-slot engine per width, cleared between the cases; [k, 'big']: the same with big buckets forced."""
    from kmer_denovo_filter_amd import KmerEngine
    made = {}

    def get(k, big=False):
        key = (k, big)
        if key not in made:
            e = KmerEngine(k, capacity_hint=1 << 27)
            if big:
                e.set_option("big_bucket_log2cap", SENDER_LOG2CAP)
            made[key] = e
        e = made[key]
        e.clear()
        assert e.get_stat("log2cap") == SENDER_LOG2CAP and e.get_stat("hash_shift") == 0
        return e
    yield get
    for e in made.values():
        e.close()


def owner_engine(k, hint, world=None, hash_shift=None, big=None):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.distributed import EngineOps
    e = KmerEngine(k, capacity_hint=hint)
    if big is not None:
        e.set_option("big_bucket_log2cap", big)
    if world is not None:
        EngineOps(e, torch.device("cuda:0")).prepare_owner(world)
    if hash_shift is not None:
        e.set_option("hash_shift", hash_shift)
    e.set_option("merge_min_pairs", 1)
    return e


def geometry(e):
    return e.get_stat("log2cap"), e.get_stat("bucket_bits"), e.get_stat("hash_shift")


def in_bucket_order(seg, geo):
    """The segment's pairs grouped by the truth's bucket of a table of this geometry, ascending; inside a bucket the
    order stays as drawn."""
    lo, hi, cnt = seg
    order = np.argsort(T.bucket(T.key_hash(lo, hi), *geo), kind="stable")
    return lo[order], (hi[order] if hi is not None else None), (cnt[order] if cnt is not None else None)


def merge_call(e, segs):
    """kdf_add_pairs_multi_dev of numpy segments (lo, hi, cnt or None), one call."""
    import torch
    keep, args = [], []
    for lo, hi, cnt in segs:
        dlo, dhi = to_dev(lo), (to_dev(hi) if hi is not None else None)
        dc = to_dev(np.asarray(cnt, dtype=np.uint32)) if cnt is not None else None
        keep.append((dlo, dhi, dc))
        args.append((dlo.data_ptr(), dhi.data_ptr() if dhi is not None else None, dc.data_ptr() if dc is not None else None, len(lo)))
    torch.cuda.synchronize()
    e.add_pairs_multi_dev(args)
    e.synchronize()


def check_table(e, truth, absent=None):
    """The whole table against the truth: the full dump, stats, query of every present key and of absent ones."""
    lo, hi, cnt = truth
    got = e.export_ge(0)
    same_pairs((got[0], got[1] if e.wide else None, got[2]), truth)
    assert e.stats()[1] == len(lo)
    if len(lo):
        assert np.array_equal(e.query(lo, hi), cnt)
    if absent is not None:
        tl, th, tc = T.merge([truth, (absent[0], absent[1], None)])
        assert len(tl) == len(lo) + len(absent[0]), "an 'absent' key is in the truth"
        assert not e.query(absent[0], absent[1]).any()


# ---- the dump ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_dump_of_a_random_table(k, senders):
    rng = np.random.default_rng(10 + k)
    lo, hi = random_keys(rng, k, 60_001)
    cnt = rng.integers(0, 6, len(lo)).astype(np.uint32)                # zero counts among them
    cnt[:3] = (U32_MAX, U32_MAX - 1, 0x60000000)
    e = senders(k)
    fill(e, lo, hi, cnt)
    truth = T.merge([(lo, hi, cnt)])
    assert len(truth[0]) == len(lo)
    grid(e, truth, (0, 1, 2, U32_MAX))
    fill(e, lo[:1], None if hi is None else hi[:1], [9])               # stays saturated
    check_dump(e, 3, 3, truth)


@pytest.mark.parametrize("k", KS)
def test_dump_of_empty_one_key_and_one_part_tables(k, senders):
    rng = np.random.default_rng(20 + k)
    e = senders(k)                                                     # empty since clear(): the deferred clear
    empty = T.merge([])
    if k > 32:
        empty = (empty[0], np.zeros(0, np.uint64), empty[2])
    grid(e, empty, (0, 1))
    lo, hi = random_keys(rng, k, 1)                                    # one key
    fill(e, lo, hi, [2])
    grid(e, T.merge([(lo, hi, [2])]), (0, 1, 2, 3))
    e = senders(k)
    # every key under eight neighbouring 16-bit hash prefixes (eight 4096-slot blocks) that no boundary of PARTS
    # separates: one part holds them all whatever `parts` is, the others are empty
    tops = np.uint64(43691) + rng.integers(0, 8, 4800, dtype=np.uint64)
    assert all(len(set(T.owner(np.arange(43691, 43699, dtype=np.uint64) << np.uint64(48), p).tolist())) == 1 for p in PARTS)
    lo, hi = T.keys_with_hash(tops, 16, 4800, k, rng)
    cnt = rng.integers(1, 4, len(lo)).astype(np.uint32)
    fill(e, lo, hi, cnt)
    truth = T.merge([(lo, hi, cnt)])
    for parts in PARTS:
        for mc in (0, 1, 2, 4):
            counts = check_dump(e, parts, mc, truth)
            assert sum(1 for c in counts if c) <= 1


@pytest.mark.parametrize("k", KS)
def test_dump_of_zero_count_keys(k, senders):
    rng = np.random.default_rng(30 + k)
    lo, hi = random_keys(rng, k, 20_003)
    e = senders(k)
    fill(e, lo, hi, None)                                              # NULL counts: plain insertion
    zero = np.zeros(len(lo), np.uint32)
    truth = T.merge([(lo, hi, zero)])
    for parts in (1, 3, 8, 64):
        assert sum(check_dump(e, parts, 0, truth)) == len(lo)          # min_count 0 keeps them
        assert sum(check_dump(e, parts, 1, truth)) == 0                # 1 drops them
    one = np.zeros(len(lo), np.uint32)
    one[::3] = 1
    fill(e, lo[::3], None if hi is None else hi[::3], one[::3])
    truth = T.merge([(lo, hi, one)])
    grid(e, truth, (0, 1))


@pytest.mark.parametrize("k", KS)
def test_dump_of_a_filter_mode_table(k):
    """count --if on a 2^28-slot table: the filter's keys with the counts of the reads, absent ones with 0."""
    import kmer_truth as KT
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    rng = np.random.default_rng(40 + k)
    genome = "".join(rng.choice(list("ACGT"), 4000))
    reads = [genome[s:s + 150] for s in rng.integers(0, len(genome) - 150, 120)]
    other = "".join(rng.choice(list("ACGT"), 1500))
    seen = KT.count_truth(reads, k)
    filt = sorted(set(list(seen)[::2]) | set(KT.count_truth([other], k)))          # half of the reads' keys, and keys no read has
    want = KT.count_truth(reads, k, filt)
    full = {v: want.get(v, 0) for v in filt}
    lo = np.array([v & T.M64 for v in filt], dtype=np.uint64)
    hi = np.array([v >> 64 for v in filt], dtype=np.uint64) if k > 32 else None
    cnt = np.array([full[v] for v in filt], dtype=np.uint32)
    assert T.is_canonical(lo[:50], None if hi is None else hi[:50], k).all() and (cnt == 0).any() and (cnt > 1).any()
    with KmerEngine(k, capacity_hint=1 << 10) as e:
        e.load_filter(lo, hi)
        e.reserve(1 << 27)
        assert e.get_stat("log2cap") == SENDER_LOG2CAP
        e.count_filtered(ReadStream.from_strings(reads))
        e.synchronize()
        grid(e, T.merge([(lo, hi, cnt)]), (0, 1, 2))


@pytest.mark.parametrize("k", KS)
def test_short_buffers_and_bad_parts_are_refused(k, senders):
    from kmer_denovo_filter_amd._native import KDF_ERR_INVALID, KdfError
    rng = np.random.default_rng(50 + k)
    lo, hi = random_keys(rng, k, 9001)
    cnt = rng.integers(1, 5, len(lo)).astype(np.uint32)
    e = senders(k)
    fill(e, lo, hi, cnt)
    n = len(lo)
    for parts in (1, 3, 64):
        with pytest.raises(KdfError) as ex:
            dump_plain(e, parts, 0, n, cap=n - 1)                      # one entry short; the canary check runs in dump_plain
        assert ex.value.code == KDF_ERR_INVALID
        need = dump_packed(e, parts, 0, n)[2][parts]
        with pytest.raises(KdfError) as ex:
            dump_packed(e, parts, 0, n, cap_bytes=need - 1)            # one byte short
        assert ex.value.code == KDF_ERR_INVALID
        assert dump_packed(e, parts, 0, n, cap_bytes=need)[0] == n     # exactly enough
        assert dump_plain(e, parts, 0, n, cap=n)[0] == n
    for parts in (0, 65):
        with pytest.raises(KdfError) as ex:
            dump_plain(e, parts, 0, n)
        assert ex.value.code == KDF_ERR_INVALID
        with pytest.raises(KdfError) as ex:
            dump_packed(e, parts, 0, n)
        assert ex.value.code == KDF_ERR_INVALID
    check_dump(e, 3, 0, T.merge([(lo, hi, cnt)]))                      # the refusals left the table as it was


def crowd(rng, k, slot, n, log2cap=SENDER_LOG2CAP, width=100):
    """n keys whose home slots are the `width` slots before `slot` (n > width: the probe runs spill past `slot`)."""
    homes = rng.integers(slot - width, slot, n, dtype=np.uint64)
    return T.keys_with_hash(homes, log2cap, n, k, rng)


def join(sets):
    lo = np.concatenate([s[0] for s in sets])
    hi = np.concatenate([s[1] for s in sets]) if sets[0][1] is not None else None
    return lo, hi


@pytest.mark.parametrize("k", KS)
def test_dump_with_crowded_owner_boundaries(k, senders):
    """Probe runs that spill and wrap at every owner boundary of parts 3, 5 and 7.  With default buckets a boundary is
    a bucket boundary, so a run wraps to its own bucket's start and stays inside its 4096-slot block."""
    rng = np.random.default_rng(60 + k)
    e = senders(k)
    assert e.get_stat("bucket_bits") == (12 if k <= 32 else 11)
    sets = []
    for parts in (3, 5, 7):
        for p in range(1, parts):
            slot = -(-p * 65536 // parts) << (SENDER_LOG2CAP - 16)     # the first slot of owner p
            sets.append(crowd(rng, k, slot, 300))
            sets.append(crowd(rng, k, slot + 100, 300))
    lo, hi = join(sets)
    cnt = rng.integers(0, 4, len(lo)).astype(np.uint32)
    fill(e, lo, hi, cnt)
    truth = T.merge([(lo, hi, cnt)])
    assert len(truth[0]) == len(lo)
    for parts in (3, 5, 7, 8):
        for mc in (0, 2):
            check_dump(e, parts, mc, truth)


@pytest.mark.parametrize("k", KS)
def test_dump_of_a_big_bucket_table(k, senders):
    """Buckets of two dump blocks (k <= 32: 8192 slots under big_bucket_log2cap): an entry homed in one block of its
    bucket can lie in the other -- spilled over the middle, or wrapped from the bucket's end to its start -- and must
    still be dumped under its own hash prefix and to its own owner.  The bucket that holds 16-bit prefix 43691 is cut
    in half by the boundary between owners 1 and 2 of parts = 3.  k = 63 is the control: 4096-slot buckets, one block."""
    rng = np.random.default_rng(70 + k)
    e = senders(k, big=True)
    bb = e.get_stat("bucket_bits")
    assert bb == (13 if k <= 32 else 12)
    B = 1 << bb
    cut = (43691 << (SENDER_LOG2CAP - 16)) >> bb                       # the bucket the parts = 3 boundary falls into
    assert k > 32 or (cut << bb) + B // 2 == 43691 << (SENDER_LOG2CAP - 16)
    buckets = [0, 1, cut, (1 << (SENDER_LOG2CAP - bb)) - 1] + rng.integers(2, 1 << (SENDER_LOG2CAP - bb - 1), 6).tolist() \
        + rng.integers(1 << (SENDER_LOG2CAP - bb - 1), (1 << (SENDER_LOG2CAP - bb)) - 1, 6).tolist()
    sets = []
    for b in buckets:
        sets.append(crowd(rng, k, b * B + B // 2, 300))                # spills over the middle of the bucket
        sets.append(crowd(rng, k, b * B + B, 300))                     # wraps to the bucket's start
    lo, hi = join(sets)
    cnt = rng.integers(1, 4, len(lo)).astype(np.uint32)
    fill(e, lo, hi, cnt)
    assert geometry(e) == (SENDER_LOG2CAP, bb, 0)
    truth = T.merge([(lo, hi, cnt)])
    for parts in (3, 1, 2, 7, 8, 64):
        for mc in (0, 2):
            check_dump(e, parts, mc, truth)
    # what two owners make of the parts = 2 dump: the LDS bucket merge, and the truth
    n, counts, offs, segs = dump_packed(e, 2, 0, len(lo))
    got = []
    for r in range(2):
        own = owner_engine(k, 1 << 16, world=2)
        try:
            merge_call(own, [segs[r]])
            assert own.get_stat("last_merge_path") == 1, "a hash-ordered dump must take the LDS bucket merge"
            mine = T.owner(T.key_hash(truth[0], truth[1]), 2) == r
            check_table(own, (truth[0][mine], truth[1][mine] if truth[1] is not None else None, truth[2][mine]))
            got.append(int(mine.sum()))
        finally:
            own.close()
    assert sum(got) == len(lo) and min(got) > 0


# ---- the owner's merge ------------------------------------------------------------------------------------------------

SEG_COUNTS = (1, 2, 3, 8, 63, 64, 65)
LENGTHS = (2311, 1, 255, 0, 256, 257, 1777, 3001)


def build_segments(rng, k, S, geo):
    """S differing segments for a table of geometry `geo` (as drawn, not yet in bucket order) and a key no segment has.
    Keys in every non-empty segment ('common'), among them one alone in its bucket; keys in one segment only; keys
    twice in one segment; counts 0, 1, and values whose sum saturates only over three segments or lands on
    2^32 - 2 and 2^32 - 1 exactly."""
    lengths = []
    for s in range(S):
        n = LENGTHS[s % len(LENGTHS)]
        if s >= len(LENGTHS) or (n == 0 and S > 8):
            n = 300 + 7 * s if n in (0, 1) else n + s                  # unequal lengths; a zero length at S = 8 only
        lengths.append(n)
    assert len(set(lengths)) == S
    ulo, uhi = random_keys(rng, k, 6000)
    ub = T.bucket(T.key_hash(ulo, uhi), *geo)
    nb = 1 << (geo[0] - geo[1])
    keep = np.ones(len(ulo), bool)
    if nb > 1:                                                          # the lone key: nothing else of the universe in its bucket
        keep = ub != ub[0]
        keep[0] = True
    ulo, uhi = ulo[keep], (uhi[keep] if uhi is not None else None)
    n_common = 20
    absent = (ulo[-50:], uhi[-50:] if uhi is not None else None)
    pool = np.arange(n_common, len(ulo) - 50)
    full = [s for s in range(S) if lengths[s] >= 255]                  # segments that hold every common key
    m = len(full)
    segs = []
    for s in range(S):
        n = lengths[s]
        if n == 0:
            idx = np.zeros(0, np.int64)
        elif n == 1:
            idx = np.array([0])                                        # the lone key
        else:
            rest = rng.choice(pool, n - n_common - 5, replace=False)
            idx = np.concatenate([np.arange(n_common), rest, rest[:5]])          # five keys twice in this segment
        cnt = rng.choice(np.array([0, 1, 1, 2, 3, 5, 0x60000000], np.uint32), len(idx)).astype(np.uint32)
        if n >= 255:
            j = full.index(s)
            cnt[0] = 1                                                 # the lone key: one from everybody
            cnt[1] = (U32_MAX - 1) - (m - 1) if j == 0 else 1          # lands on 2^32 - 2
            cnt[2] = U32_MAX - (m - 1) if j == 0 else 1                # lands on 2^32 - 1 without passing it
            cnt[3] = 0x60000000 if j < 3 else 0                        # saturates with the third segment only
            cnt[4] = 0                                                 # present with count 0
            cnt[5] = U32_MAX if j == m - 1 else 1                      # saturated by one segment, then added to
        elif n == 1:
            cnt[0] = 1
        perm = rng.permutation(len(idx))
        idx, cnt = idx[perm], cnt[perm]
        segs.append((ulo[idx], uhi[idx] if uhi is not None else None, cnt))
    return segs, absent


@pytest.mark.parametrize("S", SEG_COUNTS)
@pytest.mark.parametrize("k", KS)
def test_merge_of_differing_segments(k, S):
    rng = np.random.default_rng(1000 * k + S)
    total_max = S * 3100
    e = owner_engine(k, total_max)
    try:
        geo = geometry(e)
        segs, absent = build_segments(rng, k, S, geo)
        truth = T.merge(segs)
        assert sum(len(s[0]) for s in segs) <= total_max
        merge_call(e, [in_bucket_order(s, geo) for s in segs])
        assert geometry(e) == geo
        nonempty = sum(1 for s in segs if len(s[0]))
        assert e.get_stat("last_merge_path") == (1 if nonempty <= 64 else 2)
        check_table(e, truth, absent)
        if S >= 3:
            assert {0, U32_MAX - 1, U32_MAX} <= set(truth[2].tolist())  # the sums the case is about did occur
    finally:
        e.close()


@pytest.mark.parametrize("k", KS)
def test_merge_into_cleared_live_and_growing_tables(k):
    rng = np.random.default_rng(200 + k)
    # (a) a table only clear()ed: the merge is the deferred clear.  Junk in every bucket first; the segments then
    #     reach only the buckets of the lower half of the hash space, so the other half is cleared without a pair.
    e = owner_engine(k, 1 << 15)
    try:
        geo = geometry(e)
        assert geo[0] == 16
        jlo, jhi = random_keys(rng, k, 20_000)
        fill(e, jlo, jhi, np.full(len(jlo), 7, np.uint32))
        assert e.stats()[1] == len(jlo) and len(np.unique(T.bucket(T.key_hash(jlo, jhi), *geo))) == 1 << (geo[0] - geo[1])
        e.clear()
        lo, hi = T.keys_with_hash(0, 1, 9000, k, rng)
        segs = [(lo[:5000], None if hi is None else hi[:5000], rng.integers(0, 9, 5000).astype(np.uint32)),
                (lo[3000:], None if hi is None else hi[3000:], rng.integers(0, 9, 6000).astype(np.uint32))]
        merge_call(e, [in_bucket_order(s, geo) for s in segs])
        assert geometry(e) == geo and e.get_stat("last_merge_path") == 1
        truth = T.merge(segs)
        check_table(e, truth, (jlo[:2000], None if jhi is None else jhi[:2000]))
        # (b) the table is live now: more segments, keys in common with what it holds and new ones
        nlo, nhi = random_keys(rng, k, 4000)
        segs2 = [(np.concatenate([lo[2000:4500], nlo[:2500]]), None if hi is None else np.concatenate([hi[2000:4500], nhi[:2500]]),
                  rng.integers(0, 9, 5000).astype(np.uint32)),
                 (nlo[1000:], None if nhi is None else nhi[1000:], np.full(3000, 0x60000000, np.uint32)),
                 (nlo[1000:3000], None if nhi is None else nhi[1000:3000], np.full(2000, 0x60000000, np.uint32)),
                 (nlo[500:2500], None if nhi is None else nhi[500:2500], np.full(2000, 0x60000000, np.uint32))]
        merge_call(e, [in_bucket_order(s, geo) for s in segs2])
        assert geometry(e) == geo and e.get_stat("last_merge_path") == 1
        truth = T.merge([truth] + segs2)
        assert (truth[2] == U32_MAX).any()
        check_table(e, truth)
    finally:
        e.close()
    # (c) the merge itself forces the growth: the rehash runs first, the segments are in the grown table's order
    e = owner_engine(k, 1 << 9)
    try:
        assert e.get_stat("log2cap") == 10
        olo, ohi = random_keys(rng, k, 400)
        old = (olo, ohi, rng.integers(1, 5, 400).astype(np.uint32))
        fill(e, *old)
        lo, hi = random_keys(rng, k, 6000)
        segs = [(np.concatenate([olo[:200], lo[:4000]]), None if hi is None else np.concatenate([ohi[:200], hi[:4000]]),
                 rng.integers(0, 5, 4200).astype(np.uint32)),
                (lo[2000:], None if hi is None else hi[2000:], rng.integers(0, 5, 4000).astype(np.uint32))]
        grown = 15                                                      # cap_log2_for(400 + 8200): 2^15 slots
        geo = (grown, 12 if k <= 32 else 11, 0)
        merge_call(e, [in_bucket_order(s, geo) for s in segs])
        assert geometry(e) == geo and e.get_stat("last_merge_path") == 1
        check_table(e, T.merge([old] + segs))
    finally:
        e.close()


@pytest.mark.parametrize("k", KS)
def test_merge_paths_have_witnesses_and_one_result(k):
    rng = np.random.default_rng(300 + k)
    lo, hi = random_keys(rng, k, 5000)
    sl = lambda a, b: (lo[a:b], None if hi is None else hi[a:b], rng.integers(0, 5, b - a).astype(np.uint32))

    def run(segs, path, setup=None, ordered=True):
        e = owner_engine(k, 1 << 15)
        try:
            geo = geometry(e)
            if setup:
                setup(e)
            merge_call(e, [in_bucket_order(s, geo) if ordered else s for s in segs])
            assert e.get_stat("last_merge_path") == path
            check_table(e, T.merge(segs))
        finally:
            e.close()
    three = [sl(0, 3000), sl(2000, 5000), sl(1000, 1300)]
    run(three, 1)                                                                   # grouped segments
    run(three, 2, ordered=False)                                                    # as drawn: not grouped
    run([sl(60 * s, 60 * s + 200) for s in range(65)], 2)                           # 65 segments
    run([sl(60 * s, 60 * s + 200) for s in range(64)], 1)                           # 64 still fit
    total = sum(len(s[0]) for s in three)
    run(three, 2, setup=lambda e: e.set_option("merge_min_pairs", total + 1))       # a total below merge_min_pairs
    run(three, 1, setup=lambda e: e.set_option("merge_min_pairs", total))
    null = (lo[2500:3500], None if hi is None else hi[2500:3500], None)            # NULL counts: its keys gain 0
    run([three[0], null, three[1]], 2)


SEAMS = (1, 63, 64, 65, 255, 256, 257)


@pytest.mark.parametrize("k", KS)
def test_bounds_kernel_seams(k):
    """km_bounds_kernel compares every pair's bucket with its predecessor's; lane 0 of a wave and thread 0 of a
    workgroup fetch the predecessor by another route than the other lanes.  One descending step at index i must be
    seen wherever it falls (path 2), and ascending bucket changes at exactly those indices must be taken (path 1)."""
    rng = np.random.default_rng(400 + k)
    n = 1003
    seams = SEAMS + (n - 1,)
    e = owner_engine(k, 1 << 16)
    try:
        geo = geometry(e)
        nbits = geo[0] - geo[1]
        nb = 1 << nbits
        assert geo[0] == 17 and nb >= 32
        cases = []
        for i in seams:                                                # ascending but for ONE descending step at i
            seq = np.concatenate([np.sort(rng.integers(nb // 2, nb, i)), np.sort(rng.integers(0, nb // 2, n - i))])
            cases.append((seq, 2))
        seq = np.zeros(n, np.int64)                                    # ascending, the bucket changes at the seams exactly
        for i in seams:
            seq[i:] += 3
        cases.append((seq, 1))
        seq = np.sort(rng.integers(0, nb, n))                          # control: ascending at random places
        cases.append((seq, 1))
        for seq, path in cases:
            lo, hi = T.keys_with_hash(seq.astype(np.uint64), nbits, n, k, rng)
            assert np.array_equal(T.bucket(T.key_hash(lo, hi), *geo).astype(np.int64), seq)
            cnt = rng.integers(0, 5, n).astype(np.uint32)
            e.clear()
            merge_call(e, [(lo, hi, cnt)])
            assert e.get_stat("last_merge_path") == path, f"steps {np.nonzero(np.diff(seq))[0] + 1}"
            check_table(e, T.merge([(lo, hi, cnt)]))
            merge_call(e, [(lo, hi, cnt)])                             # and into the live table
            assert e.get_stat("last_merge_path") == path
            check_table(e, T.merge([(lo, hi, cnt)] * 2))
    finally:
        e.close()


@pytest.mark.parametrize("log2cap", (10, 12, 13, 15, 17))
@pytest.mark.parametrize("k", KS)
def test_merge_geometry(k, log2cap):
    """One bucket (2^10, 2^12 narrow), a bucket count that is a multiple of 8 (the XCD swizzle) and one that is not,
    each at hash_shift 0, 1 and 3: the owner's keys then share their top hash bits."""
    rng = np.random.default_rng(500 + 32 * k + log2cap)
    for hs in (0, 1, 3):
        e = owner_engine(k, 1 << (log2cap - 1), hash_shift=hs)
        try:
            geo = geometry(e)
            assert geo == (log2cap, min(log2cap, 12 if k <= 32 else 11), hs)
            total = 1 << (log2cap - 1)                                  # as many pairs as keep the table at this size
            nkeys = total * 2 // 5
            lo, hi = T.keys_with_hash((1 << hs) - 1, hs, nkeys, k, rng)
            a, b = nkeys * 3 // 4, nkeys // 4
            segs = [(lo[:a], None if hi is None else hi[:a], rng.integers(0, 5, a).astype(np.uint32)),
                    (lo[b:], None if hi is None else hi[b:], rng.integers(0, 5, nkeys - b).astype(np.uint32)),
                    (lo[b:a], None if hi is None else hi[b:a], np.full(a - b, 0x60000000, np.uint32))]
            assert sum(len(s[0]) for s in segs) <= total
            merge_call(e, [in_bucket_order(s, geo) for s in segs])
            assert geometry(e) == geo and e.get_stat("last_merge_path") == 1
            truth = T.merge(segs)
            check_table(e, truth)
            merge_call(e, [in_bucket_order(segs[2], geo)] * 2)          # live: the third 0x60000000 saturates
            truth = T.merge([truth, segs[2], segs[2]])
            assert (truth[2] == U32_MAX).any()
            check_table(e, truth)
        finally:
            e.close()


@pytest.mark.parametrize("k", KS)
def test_merge_with_big_buckets_on_a_small_table(k):
    """Big buckets forced on a small owner table: more than 64 KB of dynamic LDS per workgroup.  Two engines in one
    process, each raising the kernel's limit for itself."""
    rng = np.random.default_rng(600 + k)
    for round_ in range(2):
        e = owner_engine(k, 1 << 14, big=10)
        try:
            geo = geometry(e)
            assert geo == (15, 13 if k <= 32 else 12, 0)
            assert ((8 if k <= 32 else 16) + 4) << geo[1] > 65536
            lo, hi = random_keys(rng, k, 7000)
            segs = [(lo[:5000], None if hi is None else hi[:5000], rng.integers(0, 5, 5000).astype(np.uint32)),
                    (lo[2000:], None if hi is None else hi[2000:], rng.integers(0, 5, 5000).astype(np.uint32))]
            merge_call(e, [in_bucket_order(s, geo) for s in segs])
            assert geometry(e) == geo and e.get_stat("last_merge_path") == 1
            check_table(e, T.merge(segs))
            merge_call(e, [in_bucket_order(segs[0], geo)])
            assert e.get_stat("last_merge_path") == 1
            check_table(e, T.merge(segs + [segs[0]]))
        finally:
            e.close()


@pytest.mark.parametrize("k", KS)
def test_an_overfull_bucket_is_table_full_and_clear_recovers(k):
    from kmer_denovo_filter_amd._native import KDF_ERR_TABLE_FULL, KdfError
    rng = np.random.default_rng(700 + k)
    e = owner_engine(k, 1 << 13)
    try:
        geo = geometry(e)
        assert geo[0] == 14
        B = 1 << geo[1]
        lo, hi = T.keys_with_hash(1, geo[0] - geo[1], B + 100, k, rng)          # B + 100 distinct keys of bucket 1
        assert B + 100 <= 1 << 13
        with pytest.raises(KdfError) as ex:
            merge_call(e, [(lo, hi, np.ones(len(lo), np.uint32))])
        assert ex.value.code == KDF_ERR_TABLE_FULL
        assert geometry(e) == geo
        e.clear()
        klo, khi = random_keys(rng, k, 3000)
        segs = [(klo[:2000], None if khi is None else khi[:2000], rng.integers(0, 5, 2000).astype(np.uint32)),
                (klo[1000:], None if khi is None else khi[1000:], rng.integers(0, 5, 2000).astype(np.uint32))]
        merge_call(e, [in_bucket_order(s, geo) for s in segs])
        assert e.get_stat("last_merge_path") == 1
        check_table(e, T.merge(segs), (lo[:500], None if hi is None else hi[:500]))
    finally:
        e.close()


@pytest.mark.parametrize("k", (47, 63))
def test_keys_that_share_all_64_hash_bits(k, senders):
    """Wide keys are stored as (h, hi), and different keys can share h (merge_truth.collision_group): groups of 2, 3 and
    65 such keys have one owner, one order key and one home slot whatever `parts` and the table are, and only hi tells
    them apart -- in the dump's compaction, and in the merge kernels' probe (km_probe_wide_once) and claim."""
    rng = np.random.default_rng(900 + k)
    groups = []
    for n in (2, 3, 65):
        h = int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + 1
        groups.append(T.collision_group(h, n + 1, k, rng))
        assert (T.key_hash(*groups[-1]) == np.uint64(h)).all()
    # the mirror: 40 keys with ONE hi whose hashes differ below their top 28 bits -- one home slot here and in the owner
    # tables, one owner; only the stored hash word tells them apart
    groups.append(T.keys_sharing_hi(int(rng.integers(0, 1 << 28)), 28, 41, k, rng))
    assert len(set(groups[-1][1].tolist())) == 1 and len(set(T.home(T.key_hash(*groups[-1]), 28).tolist())) == 1
    held = join([(g[0][:1], g[1][:1]) for g in groups])                 # one member of each group is never stored
    mlo, mhi = join([(g[0][1:], g[1][1:]) for g in groups])
    plo, phi = random_keys(rng, k, 3000)
    lo, hi = np.concatenate([mlo, plo]), np.concatenate([mhi, phi])
    cnt = (1 + np.arange(len(lo)) % 250).astype(np.uint32)              # the members: 1, 2, 3, ...
    cnt[::11] = 0
    cnt[1] = U32_MAX
    e = senders(k)
    fill(e, lo, hi, cnt)
    truth = T.merge([(lo, hi, cnt)])
    assert len(truth[0]) == len(lo) and not e.query(*held).any()
    for parts in (1, 3, 7, 64):
        assert all(len(set(T.owner(T.key_hash(*g), parts).tolist())) == 1 for g in groups)
        for mc in (0, 1, 3):
            check_dump(e, parts, mc, truth)
    # the owner's merge: segments that hold different members of each group and repeat some
    m = len(mlo)
    pick = lambda idx, pad: (np.concatenate([mlo[idx], plo[pad]]), np.concatenate([mhi[idx], phi[pad]]))   # noqa: E731
    idx = np.arange(m)
    parts_ = [pick(idx[idx % 2 == 0], slice(0, 1500)), pick(idx[idx % 2 == 1], slice(1000, 2500)),
              pick(np.concatenate([idx[idx % 3 == 0], idx[idx % 3 == 0][:7]]), slice(2400, 3000))]            # seven members twice in one segment
    segs = [(a, b, (1 + (np.arange(len(a)) * (s + 3)) % 97).astype(np.uint32)) for s, (a, b) in enumerate(parts_)]
    segs[2][2][:5] = 0x60000000
    own = owner_engine(k, 1 << 13)
    try:
        geo = geometry(own)
        merge_call(own, [in_bucket_order(s, geo) for s in segs])
        assert geometry(own) == geo and own.get_stat("last_merge_path") == 1
        fresh = T.merge(segs)
        check_table(own, fresh, held)
        more = [(segs[1][0], segs[1][1], np.full(len(segs[1][0]), 0x60000000, np.uint32)), segs[2], segs[0]]
        merge_call(own, [in_bucket_order(s, geo) for s in more])        # into the live table
        assert geometry(own) == geo and own.get_stat("last_merge_path") == 1
        live = T.merge([fresh] + more)
        assert (live[2] == U32_MAX).any()
        check_table(own, live, held)
        merge_call(own, [segs[0]])                                       # as drawn, not grouped: the atomic kernel
        assert own.get_stat("last_merge_path") == 2
        check_table(own, T.merge([live, segs[0]]), held)
    finally:
        own.close()


@pytest.mark.parametrize("world", (2, 3, 4))
@pytest.mark.parametrize("k", KS)
def test_a_whole_exchange_on_one_gpu(k, world, senders):
    """`world` sender tables with differing, overlapping key sets, each dumped packed by owner; owner r merges segment r
    of every sender as it lies in the packed buffers, in one call."""
    import torch
    rng = np.random.default_rng(800 + 8 * k + world)
    ulo, uhi = random_keys(rng, k, 30_000)
    sent, bufs = [], []
    e = None
    for s in range(world):
        e = senders(k)
        pick = rng.random(len(ulo)) < 0.6
        pick[:10] = True                                                # some keys every sender has
        lo, hi = ulo[pick], (uhi[pick] if uhi is not None else None)
        cnt = rng.choice(np.array([0, 1, 2, 3, 0x60000000], np.uint32), len(lo)).astype(np.uint32)
        fill(e, lo, hi, cnt)
        sent.append((lo, hi, cnt))
        cap = len(lo) * (20 if k > 32 else 12) + 8 * world
        buf = torch.full((cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n, counts, offs = e.export_parts_packed_dev(0, world, buf.data_ptr(), cap)
        e.synchronize()
        assert n == len(lo) and bool((buf[offs[world]:] == CANARY).all())
        bufs.append((buf, counts, offs))
    truth = T.merge(sent)
    town = T.owner(T.key_hash(truth[0], truth[1]), world)
    KW = 2 if k > 32 else 1
    held = 0
    for r in range(world):
        own = owner_engine(k, 1 << 15, world=world)
        try:
            args = []
            for buf, counts, offs in bufs:
                p, m = buf.data_ptr() + offs[r], counts[r]
                args.append((p, p + 8 * m if KW == 2 else None, p + 8 * m * KW, m))
            own.add_pairs_multi_dev(args)
            own.synchronize()
            if world & (world - 1) == 0:
                assert own.get_stat("last_merge_path") == 1
            mine = town == r
            check_table(own, (truth[0][mine], truth[1][mine] if truth[1] is not None else None, truth[2][mine]))
            held += own.stats()[1]
        finally:
            own.close()
    assert held == len(truth[0])                                        # every key in exactly one owner
