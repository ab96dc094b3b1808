"""The device FASTQ feeder on the GPU (include/kdf.h "device FASTQ feeder"): kdf_fastq_pack against the model of the header's
rule (tests/fastq_stream_model.py, which the CPU test pins to ``ReadStream.from_strings`` on the same case list), word for
word -- the words behind n_bases and the bytes around the buffers included -- in one call, in chunks and in its refusals;
then through ``reads.stream_fastq_device`` against ``engine.count(ReadStream.from_strings(reads))``, the filtered count,
the tally, the sketch and a spool with read offsets.  The largest text is the random case of about 150 KB."""
import gzip

import numpy as np
import pytest

import fastq_stream_model as M

pytestmark = pytest.mark.gpu

T = M.TILE
FILL64 = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD_WORDS = 8                                          # 64 bytes behind every buffer
KDF_ERR_INVALID, KDF_ERR_IO = 1, 5
CASES = M.cases()
GOOD = [c for c in CASES if c.bad is None]
BAD = [c for c in CASES if c.bad is not None]
SMALL = [c for c in GOOD if len(c.text) <= 256]
LARGE = [c for c in GOOD if len(c.text) > 256]


def ids(cases):
    return [c.name for c in cases]


def quals_of(case):
    """min_qual: off, '!' (no quality of the cases is below it), a value that splits the case's qualities, 255"""
    q = np.frombuffer(b"".join(q for _, q in case.reads), np.uint8)
    return (0, 33, int(np.sort(q)[len(q) // 2]) if len(q) else 50, 255)


@pytest.fixture(scope="module")
def eng():
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(31, capacity_hint=1 << 10)            # (any engine packs any FASTQ)
    yield e
    e.close()


class Out:
    """what one call wrote: the words of the stream, the offsets, and that nothing else was touched"""


def dev_text(text: bytes, shift: int = 0):
    """the text on the device, ``shift`` bytes behind a 16-byte boundary -> (pointer, tensor to keep)"""
    import torch
    buf = torch.full((len(text) + 48,), 0x0A, dtype=torch.uint8, device="cuda")      # (line ends around it: a read outside shows)
    base = (-buf.data_ptr()) % 16 + 16 + shift
    if len(text):
        buf[base:base + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    return buf.data_ptr() + base, buf


def call(eng, text, final, state, min_qual=0, shift=0, cap_bases=None, cap_reads=None, want_offsets=True, expect_error=None):
    """kdf_fastq_pack (device memory) into buffers pre-filled with 0xA5 -> Out"""
    import torch
    from kmer_denovo_filter_amd._native import FastqFormatError, KdfError
    from kmer_denovo_filter_amd.reads import stream_words
    if cap_bases is None:
        cap_bases = len(text) // 2
    if cap_reads is None:
        cap_reads = len(text) // 4
    pw, mw = stream_words(cap_bases)
    fill = int(FILL64.view(np.int64))
    packed = torch.full((pw + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda")
    invalid = torch.full((mw + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda")
    offs = torch.full((cap_reads + 1 + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda")
    ptr, keep = dev_text(text, shift)
    torch.cuda.synchronize()                                 # (torch filled the buffers on ITS stream; the engine launches on its own)
    before = state.copy()
    o = Out()
    o.error = o.bad = None
    try:
        o.n_bases, o.n_reads, o.consumed = eng.fastq_pack_dev(
            ptr if len(text) else None, len(text), final, state, packed.data_ptr(), invalid.data_ptr(), cap_bases,
            offs.data_ptr() if want_offsets else None, cap_reads if want_offsets else 0, min_qual)
    except KdfError as ex:
        assert expect_error is not None and ex.code == expect_error, ex
        o.error = ex.code
        if isinstance(ex, FastqFormatError):
            o.bad = (ex.offset, ex.rule)
    else:
        assert expect_error is None
    torch.cuda.synchronize()
    hp, hm, ho = (x.cpu().numpy().view(np.uint64) for x in (packed, invalid, offs))
    assert (hp[pw:] == FILL64).all() and (hm[mw:] == FILL64).all() and (ho[cap_reads + 1:] == FILL64).all(), "guard bytes were written"
    if o.error is not None:                                  # refused: nothing written, state unchanged
        assert (hp == FILL64).all() and (hm == FILL64).all() and (ho == FILL64).all()
        assert (state.records, state.positions, state.bytes) == (before.records, before.positions, before.bytes)
        return o
    if not final and o.consumed == 0:                        # no complete record: emits nothing, writes nothing
        assert (o.n_bases, o.n_reads) == (0, 0)
        assert (hp == FILL64).all() and (hm == FILL64).all() and (ho == FILL64).all()
        o.packed, o.invalid, o.offsets = None, None, np.zeros(1, np.int64)
        return o
    uw, um = stream_words(o.n_bases)
    assert (hp[uw:pw] == FILL64).all() and (hm[um:mw] == FILL64).all(), "words behind kdf_stream_words(n_bases) were written"
    o.packed, o.invalid = hp[:uw].copy(), hm[:um].copy()
    if want_offsets:
        assert (ho[o.n_reads + 1:] == FILL64).all()
        o.offsets = ho[:o.n_reads + 1].view(np.int64).copy()
    else:
        assert (ho == FILL64).all()
        o.offsets = None
    return o


def same_as_model(o, codes, offsets):
    assert o.n_bases == len(codes) and o.n_reads == len(offsets) - 1
    if o.packed is None:
        assert len(codes) == 0
        return
    packed, invalid = M.to_words(codes)
    assert (o.packed == packed).all(), np.flatnonzero(o.packed != packed)[:4]
    assert (o.invalid == invalid).all(), np.flatnonzero(o.invalid != invalid)[:4]
    if o.offsets is not None:
        assert (o.offsets == offsets).all()


def key(st):
    return (st.records, st.positions, st.bytes)


# ---- 1. one final call ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", GOOD, ids=ids(GOOD))
def test_one_final_call(eng, case):
    from kmer_denovo_filter_amd._native import FastqState
    for mq in quals_of(case):
        codes, offsets = M.pack_file(case.text, mq)
        for shift, want_offsets in ((0, True), (1, True), (15, True), (0, False), (15, False)):
            st = FastqState()
            o = call(eng, case.text, True, st, mq, shift=shift, want_offsets=want_offsets)
            assert o.consumed == len(case.text)
            same_as_model(o, codes, offsets)
            assert key(st) == (len(offsets) - 1, len(codes), len(case.text))


@pytest.mark.parametrize("case", GOOD, ids=ids(GOOD))
def test_host_form_equals_the_device_form(eng, case):
    from kmer_denovo_filter_amd._native import FastqState
    for mq in quals_of(case)[::2]:
        codes, offsets = M.pack_file(case.text, mq)
        st = FastqState(3, 5, 7)
        stream, used = eng.fastq_pack(case.text, True, st, min_qual=mq)
        packed, invalid = M.to_words(codes)
        assert used == len(case.text) and stream.n_bases == len(codes) and key(st) == (3 + len(offsets) - 1, 5 + len(codes), 7 + used)
        assert (stream.packed == packed).all() and (stream.invalid == invalid).all() and (stream.offsets == offsets).all()
    if len(case.text) > 8:                                   # a call that is not the last, through the host form
        cut = len(case.text) * 2 // 3
        codes, offsets, consumed = M.pack_chunk(case.text[:cut], False)
        stream, used = eng.fastq_pack(case.text[:cut], False, FastqState())
        assert used == consumed and stream.n_bases == len(codes) and (stream.offsets == offsets).all()
        assert (stream.packed == M.to_words(codes)[0]).all() and (stream.invalid == M.to_words(codes)[1]).all()


# ---- 2. chunks ------------------------------------------------------------------------------------------------------

def run_cuts(eng, text, cuts, mq=0):
    """the calls of M.pack_cuts on the device, each compared with the model's: words, offsets, consumed, the state's totals"""
    from kmer_denovo_filter_amd._native import FastqState
    calls = M.pack_cuts(text, cuts, mq)
    st = FastqState()
    for i, (codes, offsets, consumed, after, chunk) in enumerate(calls):
        o = call(eng, chunk, i == len(calls) - 1, st, mq)
        assert o.consumed == consumed, (i, cuts)
        same_as_model(o, codes, offsets)
        assert key(st) == after.key(), (i, cuts)
    return calls


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_every_cut_in_two_calls(eng, case):
    whole = M.pack_file(case.text)[0]
    for cut in range(len(case.text) + 1):
        calls = run_cuts(eng, case.text, [cut])
        assert (np.concatenate([c[0] for c in calls]) == whole).all()        # (what the device calls were just held to)


@pytest.mark.parametrize("case", LARGE, ids=ids(LARGE))
def test_random_cuts_in_three_calls(eng, case):
    rng = np.random.default_rng(len(case.text))
    mid = quals_of(case)[2]
    for rep in range(32):
        cuts = sorted(rng.integers(0, len(case.text) + 1, 2).tolist())
        run_cuts(eng, case.text, cuts, mid if rep & 1 else 0)
    for cuts in ([T - 1, T], [T, T + 1], [2 * T, 2 * T + 1]):                # at the tile edges
        run_cuts(eng, case.text, [c for c in cuts if c <= len(case.text)])


def test_no_complete_record_writes_nothing(eng):
    from kmer_denovo_filter_amd._native import FastqState
    text = next(c for c in GOOD if c.name == "one_read_of_10k").text
    for cut in (1, 7, T, 10010, len(text) - 1):              # (the last: every line but the quality's end)
        st = FastqState(1, 2, 3)
        o = call(eng, text[:cut], False, st)
        assert (o.n_bases, o.n_reads, o.consumed) == (0, 0, 0) and o.packed is None and key(st) == (1, 2, 3)
    o = call(eng, b"", False, FastqState())                  # and so does an empty call that is not the last
    assert (o.n_bases, o.n_reads, o.consumed) == (0, 0, 0) and o.packed is None
    o = call(eng, text, False, FastqState())                 # the whole record, terminated: taken
    assert o.consumed == len(text) and o.n_reads == 1


# ---- 3. refusals ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", BAD, ids=ids(BAD))
def test_format_errors(eng, case):
    from kmer_denovo_filter_amd._native import FastqState
    for rep, (mq, shift) in enumerate(((0, 0), (40, 3), (0, 15))):       # three calls: the same record and rule every time
        st = FastqState(9, 8, 7)
        o = call(eng, case.text, True, st, mq, shift=shift, expect_error=KDF_ERR_IO)
        assert o.bad == case.bad, (rep, o.bad)
    try:                                                     # a call that is not the last examines the whole records only
        codes, offsets, consumed = M.pack_chunk(case.text, False)
    except M.FormatError as ex:
        assert call(eng, case.text, False, FastqState(), expect_error=KDF_ERR_IO).bad == (ex.offset, ex.rule) == case.bad
    else:
        assert case.bad[1] == M.TRUNCATED or case.name == "truncated_and_bad_header"
        o = call(eng, case.text, False, FastqState())
        assert o.consumed == consumed
        same_as_model(o, codes, offsets)


def test_an_incomplete_bad_record_is_left_to_the_last_call(eng):
    from kmer_denovo_filter_amd._native import FastqState
    good = next(c for c in GOOD if c.name == "crlf").text
    o = call(eng, good + b"oops\nAC\n+\n", False, FastqState())
    assert o.consumed == len(good) and o.n_reads == 3
    o = call(eng, b"oops\nAC\n+\n", True, FastqState(), expect_error=KDF_ERR_IO)
    assert o.bad == (0, M.BAD_HEADER)


def test_capacity_refusals(eng):
    from kmer_denovo_filter_amd._native import FastqState
    case = next(c for c in GOOD if c.name == "random_short_crlf")
    codes, offsets = M.pack_file(case.text)
    n_reads = len(offsets) - 1
    call(eng, case.text, True, FastqState(), cap_bases=len(codes) - 1, expect_error=KDF_ERR_INVALID)
    call(eng, case.text, True, FastqState(), cap_reads=n_reads - 1, expect_error=KDF_ERR_INVALID)
    call(eng, case.text, True, FastqState(), cap_bases=n_reads - 1, want_offsets=False, expect_error=KDF_ERR_INVALID)
    same_as_model(call(eng, case.text, True, FastqState(), cap_bases=len(codes), cap_reads=n_reads), codes, offsets)      # exactly enough
    same_as_model(call(eng, case.text, True, FastqState(), cap_reads=0, want_offsets=False), codes, offsets)             # no offsets: cap_reads does not count
    # more records than cap_reads is tested before the format, more positions than cap_bases behind it
    bad = next(c for c in BAD if c.name == "two_bad_records_far_apart")
    call(eng, bad.text, True, FastqState(), cap_reads=10, expect_error=KDF_ERR_INVALID)
    assert call(eng, bad.text, True, FastqState(), cap_bases=200, cap_reads=200, expect_error=KDF_ERR_IO).bad == bad.bad


def test_argument_refusals(eng):
    from kmer_denovo_filter_amd._native import FastqState
    text = GOOD[0].text
    call(eng, text, True, FastqState(), min_qual=256, expect_error=KDF_ERR_INVALID)
    # a text of line ends only, and one with more records than a well-formed text of its size can hold
    o = call(eng, b"\n" * 1000, True, FastqState())
    assert (o.n_bases, o.n_reads, o.consumed) == (0, 0, 1000)
    assert call(eng, b"\n" * 1000 + b"x", True, FastqState(), expect_error=KDF_ERR_IO).bad == (0, M.BAD_HEADER)
    assert call(eng, b"@\n\n+\n\n" * 3 + b"\n" * 1000 + b"x\n", False, FastqState(), expect_error=KDF_ERR_IO).bad == (18, M.BAD_HEADER)


def test_profile_stats(eng):
    from kmer_denovo_filter_amd._native import FastqState
    eng.profile(True)
    try:
        call(eng, next(c for c in GOOD if c.name == "random_150k").text, True, FastqState())
        assert eng.get_stat("fastqfeed_passes") == 1 and eng.get_stat("fastqfeed_us") > 0
    finally:
        eng.profile(False)


# ---- 4. through the engine ------------------------------------------------------------------------------------------

def _engine_reads():
    """2 000 seeded reads of 40 .. 221 bp with N runs and lower case, and their qualities"""
    lengths = np.random.default_rng(2024).integers(40, 222, 2000).tolist()
    return M.reads_of(lengths, 5000)


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    reads = _engine_reads()
    text = M.fq(reads)
    assert 500_000 < len(text) < 700_000
    d = tmp_path_factory.mktemp("fastq")
    path = str(d / "sample.fastq")
    with open(path, "wb") as f:
        f.write(text)
    return path, reads, text, d


def table_of(e):
    out = e.export_ge(0)
    keys, cnt = np.asarray(out[0]), np.asarray(out[-1])
    if keys.ndim == 1:
        hi = np.asarray(out[1]) if out[1] is not None else np.zeros_like(keys)
        o = np.lexsort((keys, hi))
        return keys[o].tolist(), hi[o].tolist(), cnt[o].tolist()
    o = np.lexsort(keys.T[::-1])
    return keys[o].tolist(), cnt[o].tolist()


def host_stream(reads, mq=0):
    from kmer_denovo_filter_amd.reads import ReadStream
    return ReadStream.from_strings([M.masked(s, q, mq) for s, q in reads])


@pytest.mark.parametrize("k", [31, 63, 101])
def test_count_equals_the_host_stream(sample, k):
    from kmer_denovo_filter_amd import KmerEngine, reads as R
    path, reads, text, _ = sample
    with KmerEngine(k, capacity_hint=1 << 19) as host:
        host.count(host_stream(reads))
        want = table_of(host)
    assert len(want[0]) > 10_000
    for chunk in (4 << 10, 64 << 10):
        with KmerEngine(k, capacity_hint=1 << 19) as dev:
            n = R.stream_fastq_device(dev, path, chunk_bytes=chunk)
            info = R.LAST_FASTQ_FEEDER
            assert n == len(reads) == info["records"] and info["bytes"] == len(text) and info["chunks"] == -(-len(text) // chunk)
            assert info["positions"] == sum(len(s) + 1 for s, _ in reads) and info["path"] == "device" and not info["compressed"]
            assert table_of(dev) == want, (k, chunk)


def test_min_qual_equals_the_masked_host_stream(sample):
    from kmer_denovo_filter_amd import KmerEngine, reads as R
    path, reads, _, _ = sample
    mq = 35                                                  # '!' and '"' of '!' .. 'I': one base in twenty, so that whole windows survive
    with KmerEngine(31, capacity_hint=1 << 19) as host, KmerEngine(31, capacity_hint=1 << 19) as dev:
        host.count(host_stream(reads, mq))
        R.stream_fastq_device(dev, path, min_qual=mq, chunk_bytes=64 << 10)
        assert R.LAST_FASTQ_FEEDER["min_qual"] == mq
        assert table_of(dev) == table_of(host) and len(table_of(host)[0]) > 1000
        host.clear()
        host.count(host_stream(reads))
        assert len(table_of(host)[0]) > 2 * len(table_of(dev)[0])            # (the mask took most windows)


def test_filtered_tally_and_sketch_equal_their_calls_on_the_host_stream(sample):
    from kmer_denovo_filter_amd import KmerEngine, reads as R
    path, reads, _, _ = sample
    stream = host_stream(reads)
    k = 31
    with KmerEngine(k, capacity_hint=1 << 19) as src:
        src.count(host_stream(reads[::3]))
        filt = src.export_ge(1)[:-1]
    with KmerEngine(k, capacity_hint=1 << 19) as dev, KmerEngine(k, capacity_hint=1 << 19) as host:
        for e in (dev, host):
            e.load_filter(*filt)
        host.count_filtered(stream)
        R.stream_fastq_device(dev, path, filtered=True, chunk_bytes=64 << 10)
        assert table_of(dev) == table_of(host) and sum(table_of(host)[-1]) > 0
    with KmerEngine(k, capacity_hint=1 << 19) as dev, KmerEngine(k, capacity_hint=1 << 19) as host:
        for e in (dev, host):
            e.prefilter_begin(3, 20)
        host.prefilter_add(stream)
        R.stream_fastq_device(dev, path, tally=True, chunk_bytes=64 << 10)
        np.testing.assert_array_equal(dev.prefilter_export(), host.prefilter_export())
        assert dev.get_stat("prefilter_windows") == host.get_stat("prefilter_windows") > 0
    with KmerEngine(k, capacity_hint=1 << 19) as dev, KmerEngine(k, capacity_hint=1 << 19) as host:
        for e in (dev, host):
            e.sketch_begin(12)
        host.sketch_add(stream)
        R.stream_fastq_device(dev, path, sketch=True, chunk_bytes=64 << 10)
        np.testing.assert_array_equal(dev.sketch_registers(), host.sketch_registers())


def test_spool_with_reads_gives_the_read_hits_of_the_host_stream(sample):
    from kmer_denovo_filter_amd import KmerEngine, reads as R
    from kmer_denovo_filter_amd.spool import ReadSpool
    path, reads, _, _ = sample
    stream = host_stream(reads)
    with KmerEngine(31, capacity_hint=1 << 19) as probe, KmerEngine(31, capacity_hint=1 << 19) as dev, ReadSpool(0, 1 << 30, 0) as sp:
        probe.count(host_stream(reads[::5]))
        sp.keep_reads = True
        n = R.stream_fastq_device(dev, path, spool=sp, chunk_bytes=64 << 10)
        assert n == sp.n_reads == len(reads) and not sp.stat("overflowed")
        assert R.LAST_FASTQ_FEEDER["chunks"] > 4 and sp.stat("segments") >= 1        # (several appends; how the spool cuts its segments is its own affair)
        want = probe.read_hits(stream)
        np.testing.assert_array_equal(sp.read_hits(probe), want)
        assert int(want[:, 0].sum()) > 0 and int((want[:, 0] == 0).sum()) > 0


def test_gzip_members_and_file_lists(sample):
    from kmer_denovo_filter_amd import KmerEngine, reads as R
    path, reads, text, d = sample
    cut = text.index(b"\n@r1000\n") + 1
    one, two, r1, r2 = str(d / "one.fastq.gz"), str(d / "two.fq.gz"), str(d / "R1.fq"), str(d / "R2.fastq")
    with gzip.open(one, "wb", compresslevel=1) as f:
        f.write(text)
    with gzip.open(two, "wb", compresslevel=1) as f:
        f.write(text[:cut + 100])                            # (a member boundary inside a record)
    with gzip.open(two, "ab", compresslevel=1) as f:
        f.write(text[cut + 100:])
    with open(r1, "wb") as f:
        f.write(text[:cut])
    with open(r2, "wb") as f:
        f.write(text[cut:-1])                                # (and no final newline)
    with KmerEngine(31, capacity_hint=1 << 19) as e:
        R.stream_fastq_device(e, path, chunk_bytes=64 << 10)
        want = table_of(e)
        for p, files, compressed in ((one, 1, True), (two, 1, True), ([r1, r2], 2, False), (r1 + "," + r2, 2, False)):
            e.clear()
            assert R.stream_fastq_device(e, p, chunk_bytes=64 << 10) == len(reads)
            assert R.LAST_FASTQ_FEEDER["files"] == files and R.LAST_FASTQ_FEEDER["compressed"] == compressed
            assert table_of(e) == want, p


def test_a_chunk_below_the_longest_record_raises(sample, monkeypatch):
    from kmer_denovo_filter_amd import KmerEngine, reads as R
    path = sample[0]
    with KmerEngine(31, capacity_hint=1 << 12) as e:
        with pytest.raises(ValueError, match="KDF_FASTQ_FEED_MB"):
            R.stream_fastq_device(e, path, chunk_bytes=64)
        monkeypatch.setenv("KDF_FASTQ_FEED_MB", str(64 / (1 << 20)))
        with pytest.raises(ValueError, match="KDF_FASTQ_FEED_MB"):
            R.stream_fastq_device(e, path)
        e.count(host_stream(_engine_reads()[:3]))            # the engine is back on its own stream and usable
        assert e.count_ge(1) > 0


def test_a_bad_record_names_its_offset_in_the_file(sample):
    from kmer_denovo_filter_amd import KmerEngine, reads as R
    from kmer_denovo_filter_amd._native import FastqFormatError
    path, reads, text, d = sample
    cut = text.index(b"\n@r1500\n") + 1
    bad = str(d / "bad.fq")
    with open(bad, "wb") as f:
        f.write(text[:cut] + b"@x\nACGT\n+\nIII\n" + text[cut:])
    with KmerEngine(31, capacity_hint=1 << 19) as e:
        with pytest.raises(FastqFormatError) as ei:
            R.stream_fastq_device(e, bad, chunk_bytes=8 << 10)
        assert (ei.value.offset, ei.value.rule, ei.value.code) == (cut, M.LENGTH, KDF_ERR_IO)
