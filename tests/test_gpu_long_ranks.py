"""Long k-mers across ranks on the GPU, one process: the dump grouped by owner rank (kdf_export_parts_w_packed_dev)
against export_ge of the same table and distributed.owner_of_w, kdf_set_counts_w_dev against query, and the owner
exchange between engines of one process (the wire format without a process group).  Equality is exact."""
import numpy as np
import pytest

from kmer_denovo_filter_amd import KmerEngine, ReadStream
from kmer_denovo_filter_amd._native import KdfError

pytestmark = pytest.mark.gpu

KS = (65, 97, 129, 161, 201)                 # W = 3, 4, 5, 6, 7
PARTS = (1, 2, 3, 8, 64)
MIN_COUNTS = (0, 1, 3)
GUARD = 256                                  # bytes behind every output buffer, checked after every call
U32_MAX = 0xFFFFFFFF


def W_of(k):
    return (2 * k + 63) // 64


def random_rows(rng, k, n):
    """n distinct random key rows of a k-mer engine (the top word holds 2k - 64 (W - 1) bits)."""
    W = W_of(k)
    rows = rng.integers(0, 1 << 63, (n, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, W), dtype=np.uint64)
    rows[:, W - 1] &= np.uint64((1 << (2 * k - 64 * (W - 1))) - 1)
    return np.unique(rows, axis=0)


def random_reads(rng, k, n=40):
    genome = "".join(rng.choice(list("ACGT"), 3000))
    out = []
    for _ in range(n):
        L = int(rng.integers(k, k + 120))
        s = int(rng.integers(0, len(genome) - L))
        out.append(genome[s:s + L])
    return out


def sorted_pairs(rows, cnt):
    """(rows, counts) in ascending (row, count) order -- a multiset in canonical form."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    assert rows.ndim == 2 and len(rows) == len(cnt)
    order = np.lexsort((cnt,) + tuple(rows[:, j] for j in range(rows.shape[1])))
    return rows[order], np.asarray(cnt, dtype=np.uint32)[order]


def dump_by_owner(e, parts, min_count, cap_bytes=None):
    """Call the entry point into a guarded buffer; -> (n, counts, offsets, [(rows, counts) per part])."""
    import torch
    W = e.key_words
    esz = 8 * W + 4
    if cap_bytes is None:
        cap_bytes = e.count_ge(min_count) * esz + 8 * parts
    buf = torch.full((cap_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        n, counts, offs = e.export_parts_w_packed_dev(min_count, parts, buf.data_ptr(), cap_bytes)
    finally:
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[cap_bytes:] == 0xA5).all(), "bytes at or past cap_bytes were written"
    segs = []
    for p in range(parts):
        a, m = offs[p], counts[p]
        rows = host[a:a + 8 * W * m].view(np.uint64).reshape(m, W)
        cnt = host[a + 8 * W * m:a + esz * m].view(np.uint32)
        segs.append((rows.copy(), cnt.copy()))
    return n, counts, offs, segs


def check_dump(e, parts, min_count):
    import torch
    from kmer_denovo_filter_amd.distributed import owner_of_w
    W = e.key_words
    esz = 8 * W + 4
    want_rows, _, want_cnt = e.export_ge(min_count)
    n, counts, offs, segs = dump_by_owner(e, parts, min_count)
    assert n == len(want_cnt) == sum(counts)
    assert len(counts) == parts and len(offs) == parts + 1 and offs[0] == 0
    for p in range(parts):
        assert offs[p] % 8 == 0 and offs[p + 1] - offs[p] == (counts[p] * esz + 7) // 8 * 8
    assert offs[parts] % 8 == 0
    for p, (rows, cnt) in enumerate(segs):
        if len(cnt):
            own = owner_of_w(torch.from_numpy(rows.view(np.int64)), parts)
            assert bool((own == p).all()), f"part {p} holds another owner's key"
    got_rows = np.concatenate([r for r, _ in segs]) if n else np.zeros((0, W), np.uint64)
    got_cnt = np.concatenate([c for _, c in segs]) if n else np.zeros(0, np.uint32)
    gr, gc = sorted_pairs(got_rows, got_cnt)
    wr, wc = sorted_pairs(want_rows, want_cnt)
    assert np.array_equal(gr, wr) and np.array_equal(gc, wc)
    return counts


def grid(e):
    for parts in PARTS:
        for mc in MIN_COUNTS:
            check_dump(e, parts, mc)


@pytest.mark.parametrize("k", KS)
def test_smallest_grown_and_empty_tables(k):
    rng = np.random.default_rng(k)
    rows = random_rows(rng, k, 3001)                               # not a multiple of 64
    cnt = rng.integers(0, 6, len(rows)).astype(np.uint32)          # some keys stored with count 0
    cnt[0] = U32_MAX                                               # a saturated count
    with KmerEngine(k, capacity_hint=1) as e:
        grid(e)                                                    # empty
        small = 301
        e.add_pairs(rows[:small], None, cnt[:small])
        cap0 = e.stats()[0]
        assert cap0 == 1 << 10                                     # the smallest table a tiny hint gives
        grid(e)
        e.add_pairs(rows[:1], None, np.array([7], np.uint32))      # stays saturated
        e.add_pairs(rows[small:], None, cnt[small:])
        cap1, distinct, _ = e.stats()
        assert cap1 > cap0 and distinct == len(rows)               # the table has grown
        grid(e)
        r64, _, c64 = e.export_ge(U32_MAX)
        assert len(c64) == 1 and np.array_equal(r64[0], rows[0])
        _, _, _, segs = dump_by_owner(e, 8, U32_MAX)
        assert sorted(c for _, cs in segs for c in cs.tolist()) == [U32_MAX]


@pytest.mark.parametrize("k", KS)
def test_key_slice_filter_mode_and_prefilter(k):
    rng = np.random.default_rng(1000 + k)
    reads = random_reads(rng, k)
    stream = ReadStream.from_strings(reads + reads[:10])           # some windows seen twice and more
    with KmerEngine(k, capacity_hint=1 << 12) as e:                # key_parts = 4, slice 2 active
        e.set_option("key_parts", 4)
        e.set_option("key_part", 2)
        e.count(stream)
        _, distinct, _ = e.stats()
        assert 0 < distinct
        all_rows = None
        with KmerEngine(k, capacity_hint=1 << 12) as full:
            full.count(stream)
            all_rows, _, all_cnt = full.export_ge(0)
        assert distinct < len(all_rows)                            # a slice, not the whole key space
        grid(e)
    with KmerEngine(k, capacity_hint=1 << 12) as e:                # filter mode: every other key, counted against the reads
        e.load_filter(all_rows[::2])
        grid(e)                                                    # every count 0
        e.count_filtered(stream)
        assert e.count_ge(1) == len(all_rows[::2])
        grid(e)
    with KmerEngine(k, capacity_hint=1 << 12) as e:                # a prefilter armed: it dumps what the table holds
        e.prefilter_begin(2, 16)
        e.prefilter_add(stream)
        e.prefilter_arm()
        e.count(stream)
        assert 0 < e.stats()[1] < len(all_rows)
        grid(e)
        e.prefilter_drop()


@pytest.mark.parametrize("k", (65, 201))
def test_empty_parts_and_single_owner(k):
    import torch
    from kmer_denovo_filter_amd.distributed import owner_of_w
    rng = np.random.default_rng(2000 + k)
    rows = random_rows(rng, k, 4000)
    with KmerEngine(k, capacity_hint=1) as e:                      # 40 keys over 64 parts: some parts are empty
        e.add_pairs(rows[:40], None, np.arange(1, 41, dtype=np.uint32))
        counts = check_dump(e, 64, 0)
        assert counts.count(0) >= 24 and sum(counts) == 40
        check_dump(e, 64, 3)
    own = owner_of_w(torch.from_numpy(rows.view(np.int64)), 8).numpy()
    mine = rows[own == 5]                                          # keys picked so that all belong to one owner
    assert len(mine) > 300
    with KmerEngine(k, capacity_hint=1) as e:
        e.add_pairs(mine, None, np.full(len(mine), 2, np.uint32))
        counts = check_dump(e, 8, 1)
        assert counts == [0] * 5 + [len(mine)] + [0] * 2
        check_dump(e, 8, 3)                                        # nothing to dump


def test_too_small_buffer_and_refusals():
    k = 129
    rng = np.random.default_rng(5)
    rows = random_rows(rng, k, 1000)
    esz = 8 * W_of(k) + 4
    with KmerEngine(k, capacity_hint=1) as e:
        e.add_pairs(rows, None, np.full(len(rows), 1, np.uint32))
        _, _, offs, _ = dump_by_owner(e, 3, 0)
        need = offs[3]
        with pytest.raises(KdfError, match=str(need)):             # one entry short: the message names the bytes needed
            dump_by_owner(e, 3, 0, cap_bytes=need - esz)           # (and the guard behind cap_bytes is intact)
        dump_by_owner(e, 3, 0, cap_bytes=need)                     # exactly enough
        for parts in (0, 65):
            with pytest.raises(KdfError, match="parts"):
                dump_by_owner(e, parts, 0, cap_bytes=need)
        with pytest.raises(KdfError):                              # the (lo, hi) dumps keep refusing long engines
            e.export_parts_packed_dev(0, 2, None, 0)
        with pytest.raises(KdfError):
            e.set_option("hash_shift", 1)
    with KmerEngine(31, capacity_hint=1 << 10) as e:               # a k = 31 engine is refused
        with pytest.raises(KdfError, match="65"):
            e.export_parts_w_packed_dev(0, 2, None, 0)
        with pytest.raises(KdfError, match="65"):
            e.set_counts_w_dev(None, None, 1)


@pytest.mark.parametrize("k", KS)
def test_set_counts_w(k):
    import torch
    W = W_of(k)
    rng = np.random.default_rng(3000 + k)
    rows = random_rows(rng, k, 2500)
    present, absent = rows[:2001], rows[2001:]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()
    for filter_mode in (False, True):
        with KmerEngine(k, capacity_hint=1) as e:
            if filter_mode:
                e.load_filter(present)
            else:
                e.add_pairs(present, None, np.full(len(present), 3, np.uint32))
            distinct = e.stats()[1]
            new = rng.integers(0, 1 << 32, len(present), dtype=np.uint64).astype(np.uint32)
            new[:3] = (0, U32_MAX, 1 << 31)
            perm = rng.permutation(len(present))
            dk, dc = up(present[perm]), up(new[perm])
            torch.cuda.synchronize()
            e.set_counts_w_dev(dk.data_ptr(), dc.data_ptr(), len(present))
            assert np.array_equal(e.query(present), new)           # query_w returns the new counts
            assert e.stats()[1] == distinct
            before = sorted_pairs(*e.export_ge(0)[::2])
            bad = present[:5].copy()
            bad[:, W - 1] |= np.uint64(1 << (2 * k - 64 * (W - 1)))   # a bit at 2k - 64 (W - 1): no k-mer
            other = np.concatenate([absent, bad])
            dk2, dc2 = up(other), up(np.full(len(other), 9, np.uint32))
            torch.cuda.synchronize()
            with pytest.raises(KdfError, match="not stored"):
                e.set_counts_w_dev(dk2.data_ptr(), dc2.data_ptr(), len(other))
            after = sorted_pairs(*e.export_ge(0)[::2])             # absent rows and bad top words change nothing
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
            assert e.stats()[1] == distinct
            assert (e.query(absent) == 0).all()
            e.set_counts_w_dev(dk.data_ptr(), dc.data_ptr(), 0)    # n = 0: nothing


@pytest.mark.parametrize("k,R", [(75, 2), (201, 3)])
def test_exchange_between_engines_of_one_process(k, R):
    """R local tables dumped by owner, segment (s -> r) added to owner r: the owners' dumps are disjoint and together
    the key-by-key (saturating) sum of the local dumps.  Through EngineOps, as OwnerPartitionedCount.exchange does it."""
    import torch
    from kmer_denovo_filter_amd.distributed import EngineOps, owner_of_w
    W = W_of(k)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4000 + k)
    pool = random_rows(rng, k, 3000)
    locals_, owners = [], []
    try:
        want = {}
        for s in range(R):
            e = KmerEngine(k, capacity_hint=1)
            locals_.append(e)
            pick = rng.random(len(pool)) < 0.6
            pick[0] = True
            cnt = rng.integers(1, 50, len(pool)).astype(np.uint32)
            cnt[0] = 0xC0000000                                    # sums past 2^32 - 1 saturate on the owner
            e.add_pairs(pool[pick], None, cnt[pick])
            for row, c in zip(pool[pick].tolist(), cnt[pick].tolist()):
                want[tuple(row)] = min(want.get(tuple(row), 0) + c, U32_MAX)
        for r in range(R):
            owners.append(KmerEngine(k, capacity_hint=1))
        oops = [EngineOps(o, dev) for o in owners]
        for o in oops:
            o.prepare_owner(R)                                     # nothing for long keys (hash_shift stays refused)
        for s in range(R):
            buf, counts, offs = EngineOps(locals_[s], dev).export_packed_by_owner(R)
            assert sum(counts) == locals_[s].stats()[1]
            for r in range(R):
                n, a = counts[r], offs[r]
                if n:
                    rows = buf[a:a + 8 * W * n].view(torch.int64).view(n, W)
                    cnt = buf[a + 8 * W * n:a + (8 * W + 4) * n].view(torch.int32)
                    oops[r].add_pairs_segments([(rows, None, cnt)])
        got = {}
        for r, o in enumerate(owners):
            rows, _, cnt = o.export_ge(0)
            if len(cnt):
                assert bool((owner_of_w(torch.from_numpy(rows.view(np.int64)), R) == r).all())
            d = {tuple(row): c for row, c in zip(rows.tolist(), cnt.tolist())}
            assert not (set(d) & set(got)), "two owners hold the same key"
            got.update(d)
        assert got == want and want[tuple(pool[0].tolist())] == U32_MAX
    finally:
        for e in locals_ + owners:
            e.close()
