"""The device BAM feeder on the GPU: BGZF inflate (kdf_bgzf_inflate_dev), the batch decoder (kdf_bamdev_decode_dev) and
the consumer (reads.stream_bam_device, KDF_DEVICE_FEEDER=1).  Every check is exact equality against zlib or against the
host reader over the same parts of the same file."""
import os
import struct

import numpy as np
import pytest

import bamdev_cases as bc
from conftest import GIAB

pytestmark = pytest.mark.gpu

KDF_ERR_IO = 5
SAMPLES = ("HG002_child", "HG003_father", "HG004_mother")


def _engine(k=31, hint=1 << 18):
    from kmer_denovo_filter_amd import KmerEngine
    return KmerEngine(k, capacity_hint=hint)


def _dev(a, dtype=np.uint8):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


# ---- a. inflate -------------------------------------------------------------------------------------------------------------
def _inflate(eng, items, slack=0):
    """items: [(payload, isize)] -> (inflated bytes per block, device statuses); the blocks' outputs lie back to back"""
    import torch
    from kmer_denovo_filter_amd.reads import BGZF_BLOCK_DTYPE
    blocks = np.zeros(len(items), BGZF_BLOCK_DTYPE)
    comp, co, oo = b"", 0, 0
    for i, (p, isize) in enumerate(items):
        blocks[i] = (co, oo, 1000 * (i + 1), len(p), isize)
        comp += p; co += len(p); oo += isize
    d_comp, d_blocks = _dev(np.frombuffer(comp + b"\0", np.uint8)), _dev(blocks)
    d_out = torch.full((oo + slack + 1,), 0xA5, dtype=torch.uint8, device="cuda")
    d_st = torch.full((len(items),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.bgzf_inflate_dev(d_comp.data_ptr(), d_blocks.data_ptr(), len(items), d_out.data_ptr(), oo + slack, d_st.data_ptr())
    out = d_out.cpu().numpy()
    assert (out[oo:] == 0xA5).all()                                  # nothing is written behind the last block
    return [out[int(b["out_off"]):int(b["out_off"]) + int(b["isize"])].tobytes() for b in blocks], d_st.cpu().numpy()


def test_inflate_valid_blocks_equal_zlib_without_fallback():
    vs = bc.valid_payloads()
    with _engine() as eng:
        got, st = _inflate(eng, [(p, len(d)) for _, p, d in vs], slack=100)
        for (label, _, d), g, s in zip(vs, got, st):
            assert s == 0 and g == d, label
        assert eng.get_stat("bamdev_fallback_blocks") == 0


@pytest.fixture(scope="module")
def corrupt_list(tmp_path_factory):
    """The fixed list -- and the CPU program's word, under sanitizers, that the decoder rejects each cleanly."""
    tmp = tmp_path_factory.mktemp("inflate_check")
    cs = bc.corrupt_payloads()
    res, _, pr = bc.run_inflate_check(bc.build_inflate_check(tmp), [(p, n, None) for _, p, n in cs], tmp)
    assert pr.returncode == 0 and not pr.stderr.strip() and all(s != 0 for s, _ in res)
    return cs, [s for s, _ in res]


def test_corrupt_blocks_get_a_status_and_fail_as_io_errors(corrupt_list):
    from kmer_denovo_filter_amd._native import KdfError
    cs, cpu_status = corrupt_list
    _, good, data = bc.valid_payloads()[2]
    with _engine() as eng:
        for (label, p, isize), want in zip(cs, cpu_status):
            with pytest.raises(KdfError) as ei:                       # zlib rejects these too
                _inflate(eng, [(good, len(data)), (p, isize), (good, len(data))])
            assert ei.value.code == KDF_ERR_IO and "file offset 2000" in str(ei.value), label
            assert f"device status {want}" in str(ei.value), label    # the same verdict as the decoder on the CPU
        assert eng.get_stat("bamdev_fallback_blocks") == 0
        got, st = _inflate(eng, [(good, len(data))])                  # the engine is none the worse
        assert got[0] == data and st[0] == 0


def _check_equal_zlib(eng, cases, slack=0):
    """cases: [(label, payload, zlib's bytes)], decoded in one call: status 0 and zlib's bytes for each"""
    got, st = _inflate(eng, [(p, len(d)) for _, p, d in cases], slack=slack)
    for i, ((label, _, d), g, s) in enumerate(zip(cases, got, st)):
        assert s == 0 and g == d, (i, label, int(s))


def test_inflate_handmade_blocks_equal_zlib_without_fallback():
    """Legal DEFLATE that zlib's encoder never writes (bamdev_cases.handmade_payloads): the device decoder rejects none"""
    hs = bc.handmade_payloads()
    with _engine() as eng:
        _check_equal_zlib(eng, hs, slack=100)
        assert eng.get_stat("bamdev_fallback_blocks") == 0


def test_lanes_see_the_bytes_other_lanes_stored_at_every_distance():
    """What csrc/kdf_inflate.h rests its one GPU-specific assumption on: a lane's load sees the earlier store of another
    lane of its wave with no fence instruction.  Matches at every distance 1..130 (and around 192 and 256), shorter than,
    as long as and longer than the distance, and chains of matches that each copy what the match before stored."""
    hs = [c for c in bc.handmade_payloads() if c[0].startswith(("every-distance", "match-chains"))]
    assert sum(c[0].startswith("every-distance") for c in hs) >= 5 and sum(c[0].startswith("match-chains") for c in hs) == 4
    with _engine() as eng:
        _check_equal_zlib(eng, hs)
        assert eng.get_stat("bamdev_fallback_blocks") == 0


def test_inflate_mutants_zlib_accepts_equal_zlib():
    """The first 512 mutants of the CPU test's corpus that zlib accepts: still legal streams, nobody's encoder's"""
    ms = []
    for p, _, want in bc.mutants():
        if want is not None:
            ms.append((len(ms), p, want))
            if len(ms) == 512:
                break
    assert len(ms) == 512
    with _engine() as eng:
        _check_equal_zlib(eng, ms)
        assert eng.get_stat("bamdev_fallback_blocks") == 0


@pytest.mark.parametrize("n", (1, 3, 4, 5, 257))
def test_inflate_batches_that_fill_workgroups_unevenly(n):
    """Four waves of a workgroup hold four table sets: neighbouring waves decode different block types, and the last
    workgroup is partly empty."""
    hs = bc.handmade_payloads()
    batch = [hs[(7 * n + i) % len(hs)] for i in range(n)]
    with _engine() as eng:
        _check_equal_zlib(eng, batch)
        assert eng.get_stat("bamdev_fallback_blocks") == 0


def test_corrupt_blocks_among_valid_ones_in_one_batch(corrupt_list):
    from kmer_denovo_filter_amd._native import KdfError
    cs, cpu_status = corrupt_list
    hs = bc.handmade_payloads()
    items = [(cs[(i // 4) % len(cs)][1], cs[(i // 4) % len(cs)][2]) if i % 4 == 3 else (hs[i % len(hs)][1], len(hs[i % len(hs)][2]))
             for i in range(4 * len(cs) + 2)]
    with _engine() as eng:
        with pytest.raises(KdfError) as ei:
            _inflate(eng, items)
        assert ei.value.code == KDF_ERR_IO and "file offset 4000 " in str(ei.value)         # block 3: the first bad one
        assert f"device status {cpu_status[0]}" in str(ei.value)
        assert eng.get_stat("bamdev_fallback_blocks") == 0
        _check_equal_zlib(eng, hs[:9])                                   # the engine is none the worse
        assert eng.get_stat("bamdev_fallback_blocks") == 0


def test_host_inflate_option_walks_the_patch_path():
    """No block zlib wrote is rejected by the device decoder, so the zlib fallback is reached through the option that
    sends every block there: the patched bytes are zlib's, and the stat counts the blocks."""
    vs = bc.valid_payloads()
    with _engine() as eng:
        eng.set_option("bamdev_host_inflate", 1)
        got, _ = _inflate(eng, [(p, len(d)) for _, p, d in vs])
        assert got == [d for _, _, d in vs]
        assert eng.get_stat("bamdev_fallback_blocks") == sum(1 for _, _, d in vs if d)


def test_table_entry_that_does_not_fit_is_refused():
    """A block table entry whose output would pass out_cap (or that states more than 64 KB) is not decoded."""
    import torch
    from kmer_denovo_filter_amd._native import KdfError
    from kmer_denovo_filter_amd.reads import BGZF_BLOCK_DTYPE
    _, p, d = bc.valid_payloads()[2]
    with _engine() as eng:
        for out_off, isize, cap in ((0, len(d), len(d) - 1), (8, len(d), len(d)), (0, 70_000, 80_000)):
            blocks = np.zeros(1, BGZF_BLOCK_DTYPE)
            blocks[0] = (0, out_off, 0, len(p), isize)
            d_comp, d_blocks = _dev(np.frombuffer(p, np.uint8)), _dev(blocks)
            d_out = torch.full((90_000,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            with pytest.raises(KdfError) as ei:
                eng.bgzf_inflate_dev(d_comp.data_ptr(), d_blocks.data_ptr(), 1, d_out.data_ptr(), cap)
            assert ei.value.code == 1 and "does not fit" in str(ei.value)
            assert (d_out.cpu().numpy() == 0xA5).all()


# ---- b-d. whole files -------------------------------------------------------------------------------------------------------
def host_reads(path, flag_off, collapse, parts):
    from kmer_denovo_filter_amd.reads import bam_reader
    out = []
    for p in range(parts):
        with bam_reader(path, flag_off, collapse, max_bases=1 << 24, max_reads=1 << 18, part=p, parts=parts) as rd:
            for st in rd:
                out += bc.stream_reads(st)
    return out


def device_reads(eng, path, flag_off, collapse, parts, subrange_bytes, comp_cap=1 << 24, tail_blocks=0, stats=None):
    """Every batch of every part through bamdev_decode_dev.  Each batch's stream is held, word for word, against the host
    packer's stream of the same reads; unfinished sub-ranges are replayed alone with a longer tail.  -> the reads."""
    import torch
    from kmer_denovo_filter_amd import reads as R
    out = []

    def decode(b):
        cap_bases, cap_reads = R.decode_capacity(b.inflated_bytes)
        pw, mw = R.stream_words(cap_bases)
        dp = torch.full((pw,), 0x5555555555555555, dtype=torch.int64, device="cuda")
        dm = torch.full((mw,), 0x3333333333333333, dtype=torch.int64, device="cuda")
        do = torch.full((cap_reads + 1,), -7, dtype=torch.int64, device="cuda")
        dc, db, ds = _dev(np.append(b.comp, np.uint8(0))), _dev(b.blocks), _dev(b.subs)
        torch.cuda.synchronize()
        nb, nr, status = eng.bamdev_decode_dev(dc.data_ptr(), db.data_ptr(), len(b.blocks), ds.data_ptr(), len(b.subs), flag_off, collapse,
                                               dp.data_ptr(), dm.data_ptr(), cap_bases, do.data_ptr(), cap_reads)
        eng.synchronize()
        upw, umw = R.stream_words(nb)
        packed, invalid = dp.cpu().numpy().view(np.uint64), dm.cpu().numpy().view(np.uint64)
        offs = do.cpu().numpy()[:nr + 1]
        assert offs[0] == 0 and offs[-1] == nb and (np.diff(offs) >= 1).all()
        assert (packed[upw:] == 0x5555555555555555).all() and (invalid[umw:] == 0x3333333333333333).all()    # nothing beyond the stream's words
        st = R.ReadStream(packed[:upw], invalid[:umw], nb, offs)
        rs = bc.stream_reads(st)
        want = R.ReadStream.from_strings(rs)                          # the host packer's layout of the same reads
        assert want.n_bases == nb
        np.testing.assert_array_equal(st.packed, want.packed[:upw])
        np.testing.assert_array_equal(st.invalid, want.invalid[:umw])
        np.testing.assert_array_equal(offs, want.offsets)
        bad = np.flatnonzero(status != R.SUB_DONE)
        assert (status[bad] == R.SUB_UNFINISHED).all()
        return rs, (int(bad[0]) if len(bad) else len(b.subs))

    for p in range(parts):
        with R.bam_raw_reader(path, flag_off, collapse, p, parts, subrange_bytes, comp_cap, tail_blocks) as rd:
            for b in rd:
                rs, taken = decode(b)
                out += rs
                if stats is not None:
                    stats["batches"] = stats.get("batches", 0) + 1
                for sub in range(b.first_sub + taken, b.first_sub + len(b.subs)):
                    tail = 8
                    while True:
                        if stats is not None:
                            stats["replays"] = stats.get("replays", 0) + 1
                        with R.bam_raw_reader(path, flag_off, collapse, p, parts, subrange_bytes, comp_cap) as rp:
                            rp.seek(sub)
                            rs, t = decode(rp.next_into(np.empty(comp_cap, np.uint8), tail_blocks=tail, max_subs=1))
                        if t == 1:
                            out += rs
                            break
                        tail *= 4
    return out


@pytest.fixture(scope="module")
def giab_host():
    from kmer_denovo_filter_amd import reads as R
    return {(s, c): host_reads(os.path.join(GIAB, s + ".bam"), R.FLAG_OFF_SAMTOOLS_FASTA if c else R.FLAG_OFF_MODULE3, c, 1)
            for s in SAMPLES for c in (True, False)}


@pytest.mark.parametrize("sample", SAMPLES)
@pytest.mark.parametrize("parts", (1, 3))
@pytest.mark.parametrize("collapse", (True, False), ids=("collapse", "module3"))
def test_decode_giab_matches_the_host_reader(sample, parts, collapse, giab_host):
    from kmer_denovo_filter_amd import reads as R
    path = os.path.join(GIAB, sample + ".bam")
    flag_off = R.FLAG_OFF_SAMTOOLS_FASTA if collapse else R.FLAG_OFF_MODULE3
    want = host_reads(path, flag_off, collapse, parts) if parts > 1 else giab_host[(sample, collapse)]
    assert want == giab_host[(sample, collapse)]
    stats = {}
    with _engine() as eng:
        got = device_reads(eng, path, flag_off, collapse, parts, 100_000, comp_cap=330_000, stats=stats)
        assert eng.get_stat("bamdev_fallback_blocks") == 0
    assert stats["batches"] >= 2 * parts                             # the batch limit forces several batches per part
    assert got == want


def _edge_bam(tmp_path, extra_before=b""):
    """A few hundred records that hit the walker's and the packer's edges; the BGZF cuts are chosen, not regular."""
    rng = np.random.default_rng(11)
    seq = lambda n, alphabet="ACGT": "".join(rng.choice(list(alphabet), n))
    recs = []
    for n in (31, 32, 33, 63, 64, 65, 0, 1, 2, 7):                    # reads begin at every alignment of the 64-bit words
        recs.append(bc.bam_record(f"len{n}", 0, seq(n)))
    recs.append(bc.bam_record("iupac", 0, "ACGTN=MRSVWYHKDBNACGT"))
    for i in range(40):
        name = f"run{i:03d}"
        recs.append(bc.bam_record(name, 0x100 | 0x40, seq(40 + i), qual=False))     # a secondary (kept under 0x500? no: 0x100 is off in both)
        recs.append(bc.bam_record(name, 0x40, seq(41 + i), qual=False))             # READ1 without qualities ...
        recs.append(bc.bam_record(name, 0x800 | 0x40, seq(50), qual=True))          # (supplementary: off under 0xD00, kept under 0x500)
        recs.append(bc.bam_record(name, 0x40, seq(42 + i), qual=True))              # ... loses to the one with them
        recs.append(bc.bam_record(name, 0x80, seq(43 + i)))                         # READ2
        recs.append(bc.bam_record(name, 0x400 | 0x80, seq(44)))                     # a duplicate inside the run: off
        recs.append(bc.bam_record(name, 0, seq(45 + (i & 1))))                      # "other" comes last in the file, first in the stream
        recs.append(bc.bam_record(name, 0xC0, seq(9)))                              # READ1 | READ2 is "other" too: the first wins the tie
    recs.append(bc.bam_record("long", 0, seq(100_000)))                             # 150 KB of record: three BGZF blocks
    for i in range(60):
        recs.append(bc.bam_record(f"tail{i:03d}", 0, seq(20 + i, "ACGTN")))
    data = bc.bam_header()
    starts = []
    for r in recs:
        starts.append(len(data)); data += r
    cuts = set(range(1500, len(data), 1500))
    cuts.add(starts[5] + 2)                                          # a 4-byte length field that straddles a block boundary
    cuts.add(starts[30] + 1)
    cuts = {c for c in cuts if not (starts[-61] < c < starts[-60])} | {starts[-61] + 60_000, starts[-61] + 120_000}
    path = str(tmp_path / "edges.bam")
    with open(path, "wb") as f:
        edges = [0] + sorted(cuts) + [len(data)]
        for i in range(len(edges) - 1):
            piece = data[edges[i]:edges[i + 1]]
            f.write(bc.bgzf_block(bc.deflate(piece, 1 + i % 9), len(piece), 0, extra_before))
            if i in (3, 17):
                f.write(bc.bgzf_block(bc.deflate(b""), 0, 0, extra_before))         # empty blocks in mid-file
        f.write(bc.BGZF_EOF)
    return path


@pytest.mark.parametrize("collapse", (True, False), ids=("collapse", "module3"))
def test_edge_records_and_cuts(tmp_path, collapse):
    from kmer_denovo_filter_amd import reads as R
    path = _edge_bam(tmp_path)
    flag_off = R.FLAG_OFF_SAMTOOLS_FASTA if collapse else R.FLAG_OFF_MODULE3
    want = host_reads(path, flag_off, collapse, 1)
    assert len(want) > 150 and max(map(len, want)) == 100_000
    if collapse:                                                      # the emit order inside a run: other, READ1, READ2
        i = want.index(next(w for w in want if len(w) in (45, 46)))
        assert [len(w) for w in want[i:i + 3]] == [45, 42, 43]
    with _engine() as eng:
        assert device_reads(eng, path, flag_off, collapse, 1, 1 << 20) == want
        stats = {}
        # sub-ranges of 2 KB of file: runs straddle the cuts, many sub-ranges are empty, the long read covers dozens
        assert device_reads(eng, path, flag_off, collapse, 2, 2000, stats=stats) == want
        assert eng.get_stat("bamdev_fallback_blocks") == 0


@pytest.mark.parametrize("collapse", (True, False), ids=("collapse", "module3"))
def test_walks_that_run_off_the_batch_are_replayed(tmp_path, collapse):
    """Blocks of 120 bytes, batches of 3 KB with a tail of ONE block: every record spans several blocks, so the walk of
    a batch's last sub-range runs off its bytes and is planned again with a longer tail.  No read is lost or doubled."""
    from kmer_denovo_filter_amd import reads as R
    path = bc.synthetic_bam(tmp_path, n_runs=60, block=120)
    flag_off = R.FLAG_OFF_SAMTOOLS_FASTA if collapse else R.FLAG_OFF_MODULE3
    want = host_reads(path, flag_off, collapse, 1)
    stats = {}
    with _engine() as eng:
        assert device_reads(eng, path, flag_off, collapse, 1, 800, comp_cap=3000, tail_blocks=1, stats=stats) == want
    assert stats["replays"] > 0 and stats["batches"] > 3


def test_decode_patches_rejected_blocks_and_walks_again(tmp_path):
    """The decode driver's own fallback: with every block sent to zlib the first walk runs over bytes the patch then
    replaces, and the second walk and scan overwrite its statuses and totals.  Same reads as the host reader, batch by batch
    the host packer's words, replays included."""
    from kmer_denovo_filter_amd import reads as R
    path = bc.synthetic_bam(tmp_path, n_runs=80, block=400)
    want = host_reads(path, R.FLAG_OFF_SAMTOOLS_FASTA, True, 1)
    stats = {}
    with _engine() as eng:
        eng.set_option("bamdev_host_inflate", 1)
        got = device_reads(eng, path, R.FLAG_OFF_SAMTOOLS_FASTA, True, 2, 3000, comp_cap=5000, tail_blocks=1, stats=stats)
        assert eng.get_stat("bamdev_fallback_blocks") > 20
    assert stats["batches"] > 2
    assert got == want


def test_extra_subfield_in_front_of_bc(tmp_path):
    """BGZF blocks whose gzip extra field carries another subfield ahead of BC: the planner's table comes from the general
    XLEN parsing, and the device inflates the payload it points at."""
    from kmer_denovo_filter_amd import reads as R
    path = _edge_bam(tmp_path, extra_before=b"XY\x03\x00abc")
    want = host_reads(path, R.FLAG_OFF_SAMTOOLS_FASTA, True, 1)
    with _engine() as eng:
        assert device_reads(eng, path, R.FLAG_OFF_SAMTOOLS_FASTA, True, 1, 50_000) == want


def test_corrupt_record_is_an_io_error(tmp_path):
    from kmer_denovo_filter_amd import reads as R
    from kmer_denovo_filter_amd._native import KdfError
    good = bc.bam_record("ok", 0, "ACGTACGT")
    bad = bytearray(bc.bam_record("bad", 0, "ACGTACGT"))
    struct.pack_into("<i", bad, 4 + 16, 1000)                        # l_seq beyond block_size
    path = str(tmp_path / "bad.bam")
    bc.write_bgzf(path, bc.bam_header() + good * 5 + bytes(bad) + good * 5)
    with _engine() as eng:
        with pytest.raises(KdfError) as ei:
            device_reads(eng, path, R.FLAG_OFF_SAMTOOLS_FASTA, False, 1, 1 << 20)
        assert ei.value.code == KDF_ERR_IO


# ---- the consumer -----------------------------------------------------------------------------------------------------------
BAM = os.path.join(GIAB, "HG002_child.bam")
PARTS = [(0, 2), (1, 2)]


def _host_pass(eng, parts=PARTS, **kw):
    from kmer_denovo_filter_amd.reads import bam_reader, sketch_batches_overlapped, stream_batches_overlapped
    rds = [bam_reader(BAM, max_bases=1 << 22, max_reads=1 << 18, part=p, parts=n) for p, n in parts]
    try:
        if kw.pop("sketch", False):
            return sketch_batches_overlapped(eng, rds, **kw)
        return stream_batches_overlapped(eng, rds, kw.pop("filtered", False), **kw)
    finally:
        for rd in rds:
            rd.close()


def _device_pass(eng, parts=PARTS, **kw):
    from kmer_denovo_filter_amd import reads as R
    n = R.stream_bam_device(eng, BAM, parts, subrange_bytes=150_000, comp_cap=400_000, **kw)
    assert R.LAST_FEEDER["path"] == "device" and R.LAST_FEEDER["batches"] >= 4 and R.LAST_FEEDER["fallback_blocks"] == 0
    return n


def _table(eng):
    out = eng.export_ge(0)
    keys = np.asarray(out[0])
    cnt = np.asarray(out[-1])
    if keys.ndim == 1:
        hi = np.asarray(out[1]) if out[1] is not None else np.zeros_like(keys)
        o = np.lexsort((keys, hi))
        return keys[o], hi[o], cnt[o]
    o = np.lexsort(keys.T[::-1])
    return keys[o], cnt[o]


@pytest.mark.parametrize("k", (31, 101))
def test_count_gives_the_host_feeders_table(k):
    with _engine(k) as dev, _engine(k) as host:
        assert _device_pass(dev) == _host_pass(host) > 0
        assert dev.stats() == host.stats()
        for a, b in zip(_table(dev), _table(host)):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("k", (31, 101))
def test_count_if_tally_and_sketch_agree_with_the_host_feeder(k):
    with _engine(k) as src:
        _host_pass(src)
        filt = src.export_ge(3)
    keys = filt[:-1] if k <= 64 else filt[:1]
    with _engine(k) as dev, _engine(k) as host:
        for e in (dev, host):
            e.load_filter(*keys)
        assert _device_pass(dev, filtered=True) == _host_pass(host, filtered=True)
        for a, b in zip(_table(dev), _table(host)):
            np.testing.assert_array_equal(a, b)
    with _engine(k) as dev, _engine(k) as host:
        for e in (dev, host):
            e.prefilter_begin(3, 20)
        _device_pass(dev, tally=True); _host_pass(host, tally=True)
        np.testing.assert_array_equal(dev.prefilter_export(), host.prefilter_export())
        assert dev.get_stat("prefilter_windows") == host.get_stat("prefilter_windows") > 0
    with _engine(k) as dev, _engine(k) as host:
        for e in (dev, host):
            e.sketch_begin(12)
        _device_pass(dev, sketch=True); _host_pass(host, sketch=True)
        np.testing.assert_array_equal(dev.sketch_registers(), host.sketch_registers())


def _spool_reads(sp):
    """The reads of a spool, trailing invalid positions dropped: a spool pads every batch to a tile boundary and keeps only
    the reads' starts, so the padding behind a batch's last read reads as invalid positions of that read -- and the two
    feeders cut their batches at different reads."""
    from kmer_denovo_filter_amd.reads import ReadStream
    out = []
    for i in range(sp.stat("segments")):
        packed, invalid, n = sp.read_segment(i)
        offs, _, _ = sp.read_offsets(i)
        out += [r.rstrip("N") for r in bc.stream_reads(ReadStream(packed, invalid, n, offs))]
    return out


def test_spool_with_reads_holds_the_same_reads():
    from kmer_denovo_filter_amd.spool import ReadSpool
    with ReadSpool(0, 1 << 30, 0) as a, ReadSpool(0, 1 << 30, 0) as b, _engine() as dev, _engine() as host:
        a.keep_reads = b.keep_reads = True
        one = [(0, 1)]                                               # one part: the batches of both feeders arrive in file order
        n = _device_pass(dev, one, spool=a)
        assert n == _host_pass(host, one, spool=b) == a.n_reads == b.n_reads
        assert _spool_reads(a) == _spool_reads(b)
        assert dev.stats() == host.stats()


def test_discovery_chain_under_the_device_feeder(tmp_path, monkeypatch):
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as jw
    from kmer_denovo_filter_amd.discovery.pipeline import (
        _extract_child_kmers_discovery, _filter_parents_discovery, _subtract_reference_kmers)
    from kmer_denovo_filter_amd.kmer_fasta import read_kmer_fasta_keys

    def chain(tmp):
        os.makedirs(tmp)
        fa, n = _extract_child_kmers_discovery(BAM, None, 31, 3, 4, tmp)
        k1 = np.sort(read_kmer_fasta_keys(fa, 31)[0])
        fa2, n2 = _subtract_reference_kmers(os.path.join(GIAB, "mini_ref.fa.k31.jf"), fa, tmp)
        k2 = np.sort(read_kmer_fasta_keys(fa2, 31)[0])
        n3, fa3 = _filter_parents_discovery(os.path.join(GIAB, "HG004_mother.bam"), os.path.join(GIAB, "HG003_father.bam"), None, fa2, 31, 4, tmp, 0)
        return (n, n2, n3), (k1, k2, np.sort(read_kmer_fasta_keys(fa3, 31)[0]))

    monkeypatch.delenv("KDF_DEVICE_FEEDER", raising=False)
    counts_h, sets_h = chain(str(tmp_path / "host"))
    assert jw.LAST_FEEDER == {"path": "host"}
    monkeypatch.setenv("KDF_DEVICE_FEEDER", "1")
    monkeypatch.setenv("KDF_FEEDER_SUBRANGE_MB", "0.125")
    counts_d, sets_d = chain(str(tmp_path / "device"))
    assert jw.LAST_FEEDER["path"] == "device" and jw.LAST_FEEDER["fallback_blocks"] == 0
    assert counts_d == counts_h == (51125, 6679, 630)
    for a, b in zip(sets_d, sets_h):
        np.testing.assert_array_equal(a, b)
