"""Reads in a spool (include/kdf.h "Reads in a spool"): the offsets kept beside the segments against the numpy model entry
for entry, the per-read replays against the same entry points batch by batch, the gap rule at a join of two batches,
select_reads, the device pointers of a segment, mode and refusals, and the plain replays left as they were."""
import numpy as np
import pytest
import torch

import spool_model as M
import spool_reads_model as R

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_NOMEM, ERR_STATE = 1, 3, 6
SEG = 1 << 12


def _engine(k, hint=1 << 14):
    from kmer_denovo_filter_amd import KmerEngine
    return KmerEngine(k, capacity_hint=hint)


def _spool(hbm=1 << 30, host=0, segment_positions=SEG, chunk=None):
    from kmer_denovo_filter_amd.spool import ReadSpool
    sp = ReadSpool(0, hbm, host)
    sp.set_option("segment_positions", segment_positions)
    if chunk:
        sp.set_option("offsets_chunk", chunk)
    return sp


def _stream(b):
    from kmer_denovo_filter_amd.reads import ReadStream
    return ReadStream(b[0], b[1], b[2], b[3])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _fill(sp, batches, **kw):
    for p, m, n, o in batches:
        sp.append(p, m, n, offsets=o, **kw)
    return sp


def _err(call):
    from kmer_denovo_filter_amd._native import KdfError
    with pytest.raises(KdfError) as ei:
        call()
    return ei.value


STATS = ("segments", "batches", "positions", "bases", "hbm_bytes", "host_bytes", "overflowed", "reads", "keeps_reads", "offset_bytes")


def _stats(sp):
    return [sp.stat(s) for s in STATS]


# ------------------------------------------------------------------ batches

def _genome_batches(k, seed=5):
    """Eight small batches of reads cut from one 3000-base genome (so k-mers repeat between batches), 1 % substitutions,
    a few invalid bases.  Read lengths include 0 (no stream position), 1, k - 1, k and one longer than a tile; the batch
    lengths cover n_bases % 64 in {0, 1, 63}; one batch is a single read; one is longer than the segment."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, 3000)

    def read(n):
        a = int(rng.integers(0, len(genome) - n))
        g = genome[a:a + n].copy()
        err = rng.random(n) < 0.01
        g[err] = (g[err] + 1) % 4
        if n > 5 and rng.random() < 0.2:
            g[int(rng.integers(0, n))] = 4
        return g

    def some(count):
        return [read(int(rng.integers(k + 5, k + 70))) for _ in range(count)]

    long_read = max(k + 40, 200)
    batches = [
        R.make_batch(rng, [read(1), None, read(k - 1)] + some(4) + [None, read(k)], rem=0),
        R.make_batch(rng, [read(long_read)], rem=63),                                       # one read
        R.make_batch(rng, some(5) + [None, None] + some(2), rem=1),
        R.make_batch(rng, [None] + some(3 + SEG // (k + 30)), rem=0),                       # above the segment size
        R.make_batch(rng, some(3), rem=63),
        R.make_batch(rng, some(2) + [None], rem=1),
        R.make_batch(rng, some(40), rem=1),
        R.make_batch(rng, some(38), rem=63),
    ]
    assert batches[3][2] > SEG and batches[1][3].tolist() == [0, batches[1][2]]
    assert sorted({b[2] % 64 for b in batches}) == [0, 1, 63]
    for p, m, n, o in batches:
        assert (len(p), len(m)) == M.stream_words(n) and o[0] == 0 and o[-1] == n
    return batches


@pytest.fixture(scope="module", params=[31, 63, 101])
def case(request):
    return request.param, _genome_batches(request.param)


@pytest.fixture(scope="module")
def case31():
    return 31, _genome_batches(31)


# ------------------------------------------------------------------ 1. layout

@pytest.mark.parametrize("form", ["append", "append_dev", "append_uploaded"])
@pytest.mark.parametrize("tier", ["hbm", "host"])
def test_offsets_layout_against_the_model(case31, form, tier):
    k, batches = case31
    rng = np.random.default_rng(1)
    empty = R.make_batch(rng, [])
    assert empty[2] == 0 and len(empty[3]) == 1
    batches = batches[:2] + [empty] + batches[2:]
    want_seg = M.segments([b[:3] for b in batches], SEG)
    want_off = R.segment_offsets(batches, SEG)
    assert len(want_seg) >= 4 and any(len(o) - 1 > 9 for o, _, _ in want_off)
    hbm, host = ((1 << 30, 0) if tier == "hbm" else (0, 1 << 30))
    # offsets_chunk 4: the arrays grow while the segments fill
    with _spool(hbm, host, chunk=4) as sp:
        assert sp.stat("keeps_reads") == 0
        if form == "append":
            _fill(sp, batches)
        elif form == "append_dev":
            side = torch.cuda.Stream()
            for j, (p, m, n, o) in enumerate(batches):
                dp, dm, do = _dev(p), _dev(m), _dev(o)
                torch.cuda.synchronize()
                sp.append_dev(dp.data_ptr(), dm.data_ptr(), n, side.cuda_stream if j % 2 else 0, d_offsets=do.data_ptr(), n_reads=len(o) - 1)
                torch.cuda.synchronize()
        else:
            with _engine(k) as eng:
                for j, b in enumerate(batches):
                    eng.upload_async(j & 1, _stream(b))
                    o = b[3].copy()
                    sp.append_uploaded(eng, j & 1, offsets=o)
                    o[:] = -7                                       # the caller's array is its own again at once
                    eng.count_uploaded(j & 1)
                assert eng.stats()[2] > 0
        n_reads = sum(len(b[3]) - 1 for b in batches)
        assert sp.stat("keeps_reads") == 1 and sp.stat("reads") == sp.n_reads == n_reads
        assert sp.stat("batches") == len(batches) - 1 and sp.stat("segments") == len(want_seg)
        ob = sp.stat("offset_bytes")
        assert ob >= 8 * (n_reads + len(want_seg)) and ob % 32 == 0
        seg_bytes = sum((2 * (w[2] // 64) + 4 + w[2] // 64 + 2) * 8 for w in want_seg)
        if tier == "hbm":
            # a segment is sized by segment_positions or by the one batch above it
            assert sp.stat("host_bytes") == 0 and sp.stat("hbm_bytes") - ob >= seg_bytes
        else:
            assert sp.stat("hbm_bytes") == 0 and sp.stat("host_bytes") - ob >= seg_bytes
        for i, ((wp, wm, wn), (wo, wfirst, wnr)) in enumerate(zip(want_seg, want_off)):
            gp, gm, gn = sp.read_segment(i)
            assert gn == wn
            np.testing.assert_array_equal(gp, wp)
            np.testing.assert_array_equal(gm, wm)
            go, gfirst, gnr = sp.read_offsets(i)
            assert (gfirst, gnr) == (wfirst, wnr)
            np.testing.assert_array_equal(go, wo)


# ------------------------------------------------------------------ 2. replay equals batch by batch

def _compare(sp, eng, batches):
    want = np.concatenate([eng.read_hits(_stream(b)) for b in batches])
    got = sp.read_hits(eng)
    assert got.shape == want.shape and got.dtype == np.uint32
    np.testing.assert_array_equal(got, want)
    for low_max in (0, 2):
        want_d = np.concatenate([eng.read_depth(_stream(b), low_max) for b in batches])
        got_d = sp.read_depth(eng, low_max)
        assert got_d.shape == want_d.shape and got_d.dtype == np.uint64
        np.testing.assert_array_equal(got_d, want_d)
    np.testing.assert_array_equal(got[:, 0].astype(np.uint64), want_d[:, 1])       # hits == present
    return want


@pytest.mark.parametrize("tier", ["hbm", "host"])
def test_replay_equals_batch_by_batch(case, tier):
    k, batches = case
    hbm, host = ((1 << 30, 0) if tier == "hbm" else (0, 1 << 30))
    with _spool(hbm, host) as sp, _engine(k) as eng:
        _fill(sp, batches)
        assert sp.stat("segments") >= 4 and (sp.stat("hbm_bytes") == 0) == (tier == "host")
        # insert mode
        for j in (0, 3):
            eng.count(_stream(batches[j]))
        rows = _compare(sp, eng, batches)
        assert rows[:, 1].max() >= 2 and (rows[:, 1] == 0).any() and (rows[:, 0] >= rows[:, 1]).all()
        lo, hi, cnt = eng.export_ge(0)
        # key_parts = 2: the hits of the slice the table holds
        eng.clear(); eng.set_option("key_parts", 2); eng.set_option("key_part", 1)
        for j in (0, 3):
            eng.count(_stream(batches[j]))
        part = _compare(sp, eng, batches)
        assert 0 < part[:, 0].sum() < rows[:, 0].sum()
        eng.set_option("key_parts", 0)
        # a loaded filter, most of its keys never seen again: stored with count 0, no hit
        eng.clear()
        eng.load_filter(lo, hi)
        eng.count_filtered(_stream(batches[4]))
        flt = _compare(sp, eng, batches)
        assert 0 < flt[:, 0].sum() < rows[:, 0].sum()
        assert sp.stat("replays") == 9


# ------------------------------------------------------------------ 3. the gap rule

def test_no_hit_or_window_crosses_the_join_of_two_batches():
    k = 31
    rng = np.random.default_rng(8)
    g = rng.integers(0, 4, 147).astype(np.uint8)
    first = rng.integers(0, 4, 60).astype(np.uint8)
    # batch A: a read and its separator (61 positions), then 67 valid bases up to position 127 and NO separator
    ca = np.concatenate([first, [0], g[:67]]).astype(np.uint8)
    ia = np.zeros(128, bool); ia[60] = True
    a = M.pack(ca, ia, rng) + (128, np.array([0, 61, 128], np.int64))
    # batch B starts on valid bases that continue A's last read in the genome
    cb = np.concatenate([g[67:], [0]]).astype(np.uint8)
    ib = np.zeros(81, bool); ib[80] = True
    b = M.pack(cb, ib, rng) + (81, np.array([0, 81], np.int64))
    whole = M.pack(g, np.zeros(147, bool)) + (147, np.array([0, 147], np.int64))
    with _spool() as sp, _engine(k) as eng:
        eng.count(_stream(whole))                                   # every window of the genome is in the table
        _fill(sp, [a, b])
        assert sp.stat("segments") == 1 and sp.stat("positions") == 64 * 5
        offs, first_read, n_reads = sp.read_offsets(0)
        assert offs.tolist() == [0, 61, 192, 273] and (first_read, n_reads) == (0, 3)
        alone = [eng.read_hits(_stream(x)) for x in (a, b)]
        assert alone[0][1].tolist() == [37, 37] and alone[1][0].tolist() == [50, 50]
        rows = sp.read_hits(eng)
        np.testing.assert_array_equal(rows, np.concatenate(alone))
        depth = sp.read_depth(eng)
        np.testing.assert_array_equal(depth, np.concatenate([eng.read_depth(_stream(x)) for x in (a, b)]))
        assert depth[:, 0].tolist()[1:] == [37, 50]                 # valid windows: none runs over the join
        # the hit bits of the segment itself: A's last read hits at 61 .. 97, B's read at 192 .. 241, nothing between
        dp, dm, n, do, _, _ = sp.segment_dev(0)
        bits = torch.zeros(n // 64 + 2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.scan_dev(dp, dm, n, bits.data_ptr())
        eng.synchronize()
        pos = np.flatnonzero(np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:n])
        assert pos[pos >= 61].tolist() == list(range(61, 98)) + list(range(192, 242))


# ------------------------------------------------------------------ 4. select_reads

@pytest.fixture(scope="module")
def many_reads():
    """2600 reads of 35 .. 50 bases in 13 batches: more than two 1024-row blocks, two segments of 2^16 positions.  Half
    the reads are random, the others come from the genome whose first 1500 bases fill the table; one in five of those is
    k genome bases from that part followed by random ones, a read with exactly one hit, so that min_distinct 1 and 2
    select different lists."""
    k = 31
    rng = np.random.default_rng(21)
    genome = rng.integers(0, 4, 4000)
    batches, table = [], []
    for j in range(13):
        reads = []
        for _ in range(200):
            n = int(rng.integers(35, 51))
            a = int(rng.integers(0, len(genome) - n))
            if rng.random() < 0.5:
                reads.append(rng.integers(0, 4, n))
            elif rng.random() < 0.2:
                a = int(rng.integers(0, 1500 - k))
                reads.append(np.concatenate([genome[a:a + k], rng.integers(0, 4, n - k)]))
            else:
                reads.append(genome[a:a + n].copy())
        batches.append(R.make_batch(rng, reads))
    table = R.make_batch(rng, [genome[:1500]])
    return k, batches, table


def test_select_reads(many_reads):
    k, batches, table = many_reads
    with _spool(segment_positions=1 << 16) as sp, _engine(k) as eng:
        _fill(sp, batches)
        eng.count(_stream(table))
        assert sp.stat("segments") == 2 and sp.n_reads == 2600
        firsts = [sp.read_offsets(i)[1] for i in range(2)]
        assert firsts[0] == 0 and firsts[1] % 1024 != 0 and firsts[1] > 1024
        rows = sp.read_hits(eng)
        np.testing.assert_array_equal(rows, np.concatenate([eng.read_hits(_stream(b)) for b in batches]))
        top = int(rows[:, 1].max())
        assert top >= 3
        for m in (1, 2, top + 1):
            want = np.flatnonzero(rows[:, 1] >= m)
            got = sp.select_reads(eng, m)
            assert got.dtype == np.int64
            np.testing.assert_array_equal(got, want)
        assert 0 < len(np.flatnonzero(rows[:, 1] >= 2)) < len(np.flatnonzero(rows[:, 1] >= 1)) < 2600
        assert len(sp.select_reads(eng, top + 1)) == 0
        np.testing.assert_array_equal(sp.select_reads(eng, 0), np.arange(2600))
        # the raw call: a buffer one entry too small, and rows that are only 8-byte aligned
        want = np.flatnonzero(rows[:, 1] >= 1)
        buf = torch.zeros(2601, dtype=torch.int64, device="cuda")
        buf[1:] = _dev(rows.reshape(-1).view(np.uint64))
        out = torch.full((len(want) + 1,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        aligned = buf[1:].clone()
        torch.cuda.synchronize()
        assert aligned.data_ptr() % 16 == 0
        for d_rows in (buf[1:].data_ptr(), aligned.data_ptr()):
            out.fill_(-1)
            torch.cuda.synchronize()
            rc, n = sp.select_reads_dev(d_rows, 1, out.data_ptr(), len(want) - 1)
            assert rc == ERR_INVALID and n == len(want)
            got = out.cpu().numpy()
            np.testing.assert_array_equal(got[:len(want) - 1], want[:-1])
            assert got[len(want) - 1:].tolist() == [-1, -1]           # at most cap entries are written
            rc, n = sp.select_reads_dev(d_rows, 1, out.data_ptr(), len(want))
            assert rc == 0 and n == len(want)
            np.testing.assert_array_equal(out.cpu().numpy()[:n], want)
        assert buf[1:].data_ptr() % 16 == 8


def test_ordinals_ride_along(case31):
    k, batches = case31
    with _spool() as sp:
        base = 0
        for p, m, n, o in batches:
            nr = len(o) - 1
            sp.append(p, m, n, offsets=o, ordinals=np.arange(base, base + nr, dtype=np.uint64) * 3)
            base += nr
        np.testing.assert_array_equal(sp.ordinals, np.arange(sp.n_reads, dtype=np.uint64) * 3)
        sp.append(*batches[0][:3], offsets=batches[0][3])           # one append without: no ordinals any more
        assert sp.ordinals is None
        sp.clear()
        assert len(sp.ordinals) == 0 and sp.n_reads == 0


# ------------------------------------------------------------------ 5. segment_dev

def test_segment_dev_runs_the_dev_entry_points_in_place(case31):
    k, batches = case31
    want_seg = M.segments([b[:3] for b in batches], SEG)
    want_off = R.segment_offsets(batches, SEG)
    with _spool() as sp, _engine(k) as eng:
        _fill(sp, batches)
        eng.count(_stream(batches[0])); eng.count(_stream(batches[3]))
        total = 0
        for i, ((wp, wm, wn), (wo, wfirst, wnr)) in enumerate(zip(want_seg, want_off)):
            dp, dm, n, do, first, nr = sp.segment_dev(i)
            assert (n, first, nr) == (wn, wfirst, wnr) and do
            from kmer_denovo_filter_amd.reads import ReadStream
            bits_want, _ = eng.scan(ReadStream(wp, wm, wn, wo), want_distinct=False)
            pos_want, reads_want = eng.hit_list(bits_want, wn, wo)
            bits = torch.zeros(len(wm), dtype=torch.int64, device="cuda")
            dpos = torch.zeros(max(len(pos_want), 1), dtype=torch.int64, device="cuda")
            drd = torch.zeros(max(len(pos_want), 1), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            eng.scan_dev(dp, dm, n, bits.data_ptr())
            got = eng.hit_list_dev(bits.data_ptr(), n, do, nr, dpos.data_ptr(), drd.data_ptr(), len(pos_want))
            eng.synchronize()
            assert got == len(pos_want)
            np.testing.assert_array_equal(dpos.cpu().numpy()[:got].view(np.uint64), pos_want)
            np.testing.assert_array_equal(drd.cpu().numpy()[:got], reads_want)
            assert (reads_want >= 0).all()                          # every hit lies in a read of its segment
            total += got
        assert total > 100
    with _spool(0, 1 << 30) as sp:
        _fill(sp, batches[:2])
        e = _err(lambda: sp.segment_dev(0))
        assert e.code == ERR_STATE and "kdf_spool_read_segment" in str(e)
    with _spool() as sp:                                            # a spool without reads: no offsets pointer
        sp.append(*batches[0][:3])
        dp, dm, n, do, first, nr = sp.segment_dev(0)
        assert dp and dm and n == 64 * (batches[0][2] // 64 + 1) and do is None and (first, nr) == (0, 0)
        assert _err(lambda: sp.read_offsets(0)).code == ERR_STATE


# ------------------------------------------------------------------ 6. state and errors

def test_mode_offsets_checks_and_refusals(case31):
    k, batches = case31
    p, m, n, o = batches[0]
    with _spool() as sp, _engine(k) as eng:
        # an empty spool: every replay is fine and writes nothing
        assert sp.read_hits(eng).shape == (0, 2) and sp.read_depth(eng).shape == (0, 6) and len(sp.select_reads(eng)) == 0
        sp.append(M.pack(np.zeros(0, np.uint8), np.zeros(0, bool))[0], M.pack(np.zeros(0, np.uint8), np.zeros(0, bool))[1], 0,
                  offsets=np.zeros(1, np.int64))                    # nothing stored, nothing decided
        assert _stats(sp) == [0] * len(STATS)
        # every offsets violation is refused before anything happens
        before = _stats(sp)
        bad = [o + 1, np.concatenate([o[:-1], [n - 1]]), np.concatenate([o[:-1], [n + 1]]),
               np.concatenate([o[:2], [o[1] - 1], o[3:]])]
        assert bad[3][2] < bad[3][1]
        for off in bad:
            assert _err(lambda: sp.append(p, m, n, offsets=off)).code == ERR_INVALID
            eng.upload_async(0, _stream(batches[0]))
            assert _err(lambda: sp.append_uploaded(eng, 0, offsets=off)).code == ERR_INVALID
            eng.count_uploaded(0)
        lib = sp._lib
        from ctypes import c_void_p
        vp = lambda a: a.ctypes.data_as(c_void_p)
        assert lib.kdf_spool_append_reads(sp._h, vp(p), vp(m), n, vp(o), -1) == ERR_INVALID
        assert lib.kdf_spool_append_reads(sp._h, vp(p), vp(m), n, vp(o), 0) == ERR_INVALID     # positions in no read
        # reads in a batch of no positions: refused in every form
        zeros = np.zeros(3, np.int64)
        dz = _dev(zeros)
        torch.cuda.synchronize()
        assert lib.kdf_spool_append_reads(sp._h, vp(p), vp(m), 0, vp(zeros), 2) == ERR_INVALID
        assert lib.kdf_spool_append_reads_dev(sp._h, None, None, None, 0, c_void_p(dz.data_ptr()), 2) == ERR_INVALID
        eng.upload_async(0, _stream(R.make_batch(np.random.default_rng(3), [])))
        assert _err(lambda: sp.append_uploaded(eng, 0, offsets=zeros)).code == ERR_INVALID
        eng.count_uploaded(0)
        assert _stats(sp) == before
        # the first append decides
        sp.append(p, m, n, offsets=o)
        after = _stats(sp)
        e = _err(lambda: sp.append(p, m, n))
        assert e.code == ERR_STATE
        eng.upload_async(1, _stream(batches[0]))
        assert _err(lambda: sp.append_uploaded(eng, 1)).code == ERR_STATE
        eng.count_uploaded(1)
        d = _dev(p)
        torch.cuda.synchronize()
        assert _err(lambda: sp.append_dev(d.data_ptr(), d.data_ptr(), 8)).code == ERR_STATE
        assert _stats(sp) == after
        sp.clear()
        sp.append(p, m, n)                                          # ... and after clear it decides again
        assert sp.stat("keeps_reads") == 0 and sp.stat("offset_bytes") == 0
        assert _err(lambda: sp.append(p, m, n, offsets=o)).code == ERR_STATE
        # a spool without reads refuses the per-read replays
        for call in (lambda: sp.read_hits(eng), lambda: sp.read_depth(eng), lambda: sp.select_reads(eng)):
            assert _err(call).code == ERR_STATE
    # an overflowed spool: the budget holds one segment and the offsets array its first batch sized, and no more
    seg_bytes = (2 * (SEG // 64) + 4 + SEG // 64 + 2) * 8
    with _spool(chunk=16) as probe:
        probe.append(*batches[1][:3], offsets=batches[1][3])
        ob = probe.stat("offset_bytes")
        assert probe.stat("hbm_bytes") == seg_bytes + ob and 16 <= ob < 4096
    rng = np.random.default_rng(2)
    tiny = R.make_batch(rng, [rng.integers(0, 4, 1) for _ in range(ob // 8)])   # more reads than entries are left
    assert batches[1][2] + tiny[2] + 128 < SEG
    with _spool(seg_bytes + ob, 0, chunk=16) as sp, _engine(k) as eng:
        sp.append(*batches[1][:3], offsets=batches[1][3])
        held = _stats(sp)
        e = _err(lambda: sp.append(*tiny[:3], offsets=tiny[3]))
        assert e.code == ERR_NOMEM and "read offsets" in str(e)
        assert sp.stat("overflowed") == 1 and [a for a, name in zip(_stats(sp), STATS) if name != "overflowed"] == \
            [a for a, name in zip(held, STATS) if name != "overflowed"]
        assert sp.stat("reads") == 1 and sp.stat("batches") == 1 and sp.stat("segments") == 1
        for call in (lambda: sp.read_hits(eng), lambda: sp.read_depth(eng)):
            e = _err(call)
            assert e.code == ERR_STATE and "overflowed" in str(e)
        assert _err(lambda: sp.append(*batches[1][:3], offsets=batches[1][3])).code == ERR_STATE
        offs, first, nr = sp.read_offsets(0)                        # what is stored stays readable
        assert offs.tolist() == batches[1][3].tolist() and (first, nr) == (0, 1)


def test_a_new_segment_goes_to_the_tier_that_holds_its_offsets_too(case31):
    """An HBM budget that holds one segment but not its first offsets array: the segment goes to the host tier, as one
    that does not fit would; the spool does not overflow while the host budget has room."""
    k, batches = case31
    seg_bytes = (2 * (SEG // 64) + 4 + SEG // 64 + 2) * 8
    with _spool(seg_bytes + 8, 1 << 30, chunk=16) as sp, _engine(k) as eng:
        _fill(sp, batches[:2])
        assert sp.stat("overflowed") == 0 and sp.stat("hbm_bytes") == 0
        assert sp.stat("host_bytes") == seg_bytes + sp.stat("offset_bytes") and sp.stat("offset_bytes") >= 16 * 8
        eng.count(_stream(batches[0]))
        np.testing.assert_array_equal(sp.read_hits(eng), np.concatenate([eng.read_hits(_stream(b)) for b in batches[:2]]))
    with _spool(seg_bytes + 8, 1 << 30) as sp:                      # ... and a spool without reads still takes HBM first
        sp.append(*batches[0][:3])
        assert sp.stat("hbm_bytes") == seg_bytes and sp.stat("host_bytes") == 0


def test_replay_refuses_an_engine_on_another_device(case31):
    k, batches = case31
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs: an engine on another device than the spool's cannot be made on one")
    from kmer_denovo_filter_amd import KmerEngine
    p, m, n, o = batches[0]
    with _spool() as sp, KmerEngine(k, capacity_hint=1 << 10, device=1) as other:
        sp.append(p, m, n, offsets=o)
        assert _err(lambda: sp.read_hits(other)).code == ERR_INVALID
        assert _err(lambda: sp.read_depth(other)).code == ERR_INVALID


# ------------------------------------------------------------------ 7. nothing else moved

def test_plain_replays_do_not_see_the_offsets(case31):
    k, batches = case31

    def state(eng):
        lo, hi, cnt = eng.export_ge(0)
        return [np.asarray(lo), np.asarray(cnt)], eng.stats()[1:]

    with _spool() as plain, _spool() as kept, _engine(k) as a, _engine(k) as b:
        for p, m, n, o in batches:
            plain.append(p, m, n)
            kept.append(p, m, n, offsets=o)
        assert plain.stat("offset_bytes") == 0 and plain.stat("reads") == 0 and kept.stat("reads") > 0
        for i in range(plain.stat("segments")):
            for x, y in zip(plain.read_segment(i), kept.read_segment(i)):
                np.testing.assert_array_equal(x, y)
        assert plain.stat("hbm_bytes") == kept.stat("hbm_bytes") - kept.stat("offset_bytes")
        plain.replay(a, 0); kept.replay(b, 0)
        (ka, sa), (kb, sb) = state(a), state(b)
        assert sa == sb and sa[1] > 0
        for x, y in zip(ka, kb):
            np.testing.assert_array_equal(x, y)
        keep = ka[1] >= 2
        for e, sp in ((a, plain), (b, kept)):
            e.clear(); e.load_filter(ka[0][keep], None)
            sp.replay(e, 1)
        (fa, sa), (fb, sb) = state(a), state(b)
        assert sa == sb
        for x, y in zip(fa, fb):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(fa[1], ka[1][keep])
        for e, sp in ((a, plain), (b, kept)):
            e.clear(); e.prefilter_begin(2, 16)
            sp.replay(e, 2)
        np.testing.assert_array_equal(a.prefilter_export(), b.prefilter_export())
        assert a.get_stat("prefilter_windows") == b.get_stat("prefilter_windows") > 0
