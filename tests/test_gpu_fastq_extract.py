"""kdf_fq_extract on the GPU (include/kdf.h "FASTQ record extract") against the model written from the header
(tests/fastq_extract_model.py), byte for byte: both ``mem`` forms over the feeder's case list, every keep pattern, final and
not, text and output at every alignment, outputs that end on and around a granule and a tile, the final call's completions,
the sentinels around everything the call may write, every refusal with nothing written, a text cut into chunks, and two
runs that must agree.  The largest text is one read of 70 000 bases."""
import ctypes
from ctypes import byref, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

import fastq_extract_model as X
import fastq_stream_model as M

pytestmark = pytest.mark.gpu

T = M.TILE
FILL = 0xA5
GUARD = 64                                               # sentinel bytes in front of and behind the output
KDF_ERR_INVALID, KDF_ERR_IO = 1, 5
HOST, DEVICE = 0, 1
CASES = M.cases()
GOOD = [c for c in CASES if c.bad is None]
BAD = [c for c in CASES if c.bad is not None]


def ids(cases):
    return [c.name for c in cases]


@pytest.fixture(scope="module")
def eng():
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(31, capacity_hint=1 << 10)            # (any engine extracts from any FASTQ)
    yield e
    e.close()


def patterns(n, seed=0):
    """keep patterns over n records: none, all, first only, last only, every other, seeded random"""
    rng = np.random.default_rng(1000 + seed + n)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[:1] = 1
    last[-1:] = 7                                        # (any nonzero byte keeps)
    return {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "first": first, "last": last,
            "every_other": (np.arange(n) % 2 == 1).astype(np.uint8) * 255, "random": (rng.random(n) < 0.4).astype(np.uint8)}


class Res:
    pass


def call(eng, mem, text, final, keep, tshift=0, oshift=0, want_offsets=True, cap_out=None, n_reads=None, null_keep=False, n_bytes=None):
    """kdf_fq_extract through the library, text ``tshift`` and the output ``oshift`` bytes behind a 16-byte boundary,
    every buffer filled with 0xA5 and checked: nothing in front of ``out``, nothing behind ``out_bytes``, nothing behind
    entry ``n_kept + 1`` of the offsets, and nothing at all after a refusal or a call that emits nothing."""
    import torch
    from kmer_denovo_filter_amd import _native
    text = bytes(text)
    keep = np.ascontiguousarray(keep, np.uint8)
    nr = len(keep) if n_reads is None else n_reads
    cap = len(text) + 2 if cap_out is None else cap_out
    n_out, n_off = GUARD + 16 + 16 + cap + GUARD, (nr + 1 + 8)
    h_text = np.full(len(text) + 64, 0x0A, np.uint8)     # (line ends around the text: a read outside it shows)
    if mem == DEVICE:
        d_text = torch.full((len(text) + 64,), 0x0A, dtype=torch.uint8, device="cuda")
        d_out = torch.full((n_out,), FILL, dtype=torch.uint8, device="cuda")
        d_off = torch.full((n_off,), -1, dtype=torch.int64, device="cuda")
        d_keep = torch.from_numpy(np.concatenate([keep, np.zeros(1, np.uint8)])).cuda()
        tb = (-d_text.data_ptr()) % 16 + 16 + tshift
        ob = (-d_out.data_ptr()) % 16 + GUARD + oshift
        if len(text):
            d_text[tb:tb + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
        p_text, p_out, p_off, p_keep = d_text.data_ptr() + tb, d_out.data_ptr() + ob, d_off.data_ptr(), d_keep.data_ptr()
        torch.cuda.synchronize()                         # (torch filled the buffers on ITS stream; the engine launches on its own)
    else:
        h_out = np.full(n_out, FILL, np.uint8)
        h_off = np.full(n_off, -1, np.int64)
        h_keep = np.concatenate([keep, np.zeros(1, np.uint8)])
        tb = (-h_text.ctypes.data) % 16 + 16 + tshift
        ob = (-h_out.ctypes.data) % 16 + GUARD + oshift
        h_text[tb:tb + len(text)] = np.frombuffer(text, np.uint8)
        p_text, p_out, p_off, p_keep = h_text.ctypes.data + tb, h_out.ctypes.data + ob, h_off.ctypes.data, h_keep.ctypes.data
    out_bytes, n_kept, used, bad, rule = c_uint64(9), c_uint64(9), c_uint64(9), c_uint64(9), c_uint32(9)
    rc = eng._lib.kdf_fq_extract(eng._h, mem, c_void_p(p_text) if len(text) else None, len(text) if n_bytes is None else n_bytes, int(final),
                                    None if null_keep or (nr == 0 and n_reads is None) else c_void_p(p_keep), nr, c_void_p(p_out), cap,
                                    c_void_p(p_off) if want_offsets else None, byref(out_bytes), byref(n_kept), byref(used), byref(bad), byref(rule))
    if mem == DEVICE:
        torch.cuda.synchronize()
        h_out, h_off = d_out.cpu().numpy(), d_off.cpu().numpy()
    r = Res()
    r.rc, r.out_bytes, r.n_kept, r.consumed, r.bad = rc, out_bytes.value, n_kept.value, used.value, (bad.value, rule.value)
    assert (h_out[:ob] == FILL).all() and (h_out[ob + r.out_bytes:] == FILL).all(), "bytes outside out[0 .. out_bytes) were written"
    if rc != 0:
        assert (r.out_bytes, r.n_kept, r.consumed) == (0, 0, 0) and (h_off == -1).all(), "a refused call wrote something"
        if rc != KDF_ERR_IO:
            assert r.bad == (2 ** 64 - 1, 0)
        return r
    assert r.bad == (2 ** 64 - 1, 0)
    r.out = h_out[ob:ob + r.out_bytes].tobytes()
    if want_offsets and not (r.consumed == 0 and not final) and len(text):
        assert (h_off[r.n_kept + 1:] == -1).all(), "entries behind n_kept + 1 of the offsets were written"
        r.offsets = h_off[:r.n_kept + 1].tolist()
    else:
        assert (h_off == -1).all()
        r.offsets = None
    return r


def same_as_model(r, text, final, keep):
    out, offs, consumed = X.extract_chunk(text, final, list(keep))
    assert r.rc == 0
    assert (r.out_bytes, r.n_kept, r.consumed) == (len(out), len(offs) - 1, consumed)
    assert r.out == out, next(i for i in range(len(out)) if r.out[i] != out[i])
    if r.offsets is not None:
        assert r.offsets == offs
    assert r.out_bytes <= r.consumed + 2


def n_records(text, final):
    return len(X.records_of(text, final)[0]) if len(text) else 0


# ---- 1. the case list, every pattern, both mem forms, final and not ------------------------------------------------------

@pytest.mark.parametrize("mem", (DEVICE, HOST), ids=("device", "host"))
@pytest.mark.parametrize("case", GOOD, ids=ids(GOOD))
def test_cases_every_pattern(eng, case, mem):
    big = len(case.text) > 20000
    for final in (True, False):
        n = n_records(case.text, final)
        for i, (name, keep) in enumerate(patterns(n).items()):
            if big and mem == HOST and name not in ("random", "all"):
                continue
            r = call(eng, mem, case.text, final, keep, tshift=(3 * i + 1) % 16, oshift=(5 * i + 2) % 16, want_offsets=i % 2 == 0)
            same_as_model(r, case.text, final, keep)


# ---- 2. alignment: the text and the output at every skew --------------------------------------------------------------------

def test_every_skew_of_text_and_output(eng):
    reads = M.reads_of((40, 0, 33, 17, 64, 1, 90), 21)
    text = M.fq(reads, header=lambda i: b"@read%d/1 a comment" % i, plus=lambda i: b"+" if i % 2 else b"+read%d" % i)
    keep = np.array([1, 1, 0, 1, 0, 1, 1], np.uint8)
    want = X.extract_chunk(text, True, list(keep))[0]
    for ts in range(16):
        r = call(eng, DEVICE, text, True, keep, tshift=ts, oshift=(ts * 7) % 16)
        assert r.out == want
    for os_ in range(16):
        r = call(eng, DEVICE, text, True, keep, tshift=5, oshift=os_)
        assert r.out == want
        r = call(eng, HOST, text, True, keep, tshift=os_, oshift=15 - os_)
        assert r.out == want


# ---- 3. outputs that end on and around a granule and a tile -----------------------------------------------------------------

def sized(total, n_kept):
    """a text whose records 1, 3, 5 ... (n_kept of them, between dropped neighbours) take exactly ``total`` bytes"""
    s = 150 if total > 400 else 3
    plain = 2 * s + 6 + 2                                    # header "@k" + a digit is not used: headers are "@" + pad
    reads, headers = [], []
    for i in range(2 * n_kept + 1):
        reads.append((M.seq(s, 50 + i), M.qual(s, 50 + i)))
        headers.append(b"@" + b"d" * (i % 5))
    kept = list(range(1, 2 * n_kept, 2))
    for i in kept[:-1]:
        headers[i] = b"@kk"
    rest = total - (len(kept) - 1) * plain
    assert rest >= 2 * s + 6
    headers[kept[-1]] = b"@" + b"p" * (rest - 2 * s - 6)
    text = M.fq(reads, header=lambda i: headers[i])
    keep = np.zeros(len(reads), np.uint8)
    keep[kept] = 1
    return text, keep


@pytest.mark.parametrize("total", [b + d for b in (16, T, 2 * T) for d in (-1, 0, 1)])
def test_output_sizes_around_granule_and_tile(eng, total):
    text, keep = sized(total, 1 if total < 400 else 12)
    for oshift in (0, 1, 15):
        r = call(eng, DEVICE, text, True, keep, tshift=9, oshift=oshift)
        same_as_model(r, text, True, keep)
        assert r.out_bytes == total
    same_as_model(call(eng, HOST, text, False, keep), text, False, keep)


def test_empty_record_between_dropped_neighbours(eng):
    reads = M.reads_of((150, 0, 150, 150, 0, 0, 150), 31)
    text = M.fq(reads, header=lambda i: b"@")                # the empty records take 6 bytes: "@\n\n+\n\n"
    for keep in ([0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0], [0, 1, 0, 0, 1, 1, 0], [1, 1, 0, 0, 0, 1, 1]):
        for final in (True, False):
            r = call(eng, DEVICE, text, final, keep, tshift=7, oshift=3)
            same_as_model(r, text, final, keep)
            assert r.out_bytes >= 6 * sum(keep)
    r = call(eng, DEVICE, text, True, [0, 1, 0, 0, 0, 0, 0])
    assert r.out == b"@\n\n+\n\n" and r.offsets == [0, 6]


def test_one_read_of_70k_spans_many_output_tiles(eng):
    reads = M.reads_of((100, 70000, 120, 80), 41)
    text = M.fq(reads)
    for keep in ([0, 1, 0, 0], [1, 1, 0, 1], [0, 1, 1, 0]):
        r = call(eng, DEVICE, text, True, keep, tshift=11, oshift=6)
        same_as_model(r, text, True, keep)
    assert r.out_bytes > 30 * T
    same_as_model(call(eng, HOST, text, False, [0, 1, 0, 1]), text, False, [0, 1, 0, 1])


# ---- 4. the final call's completions ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", (DEVICE, HOST), ids=("device", "host"))
def test_final_completions(eng, mem):
    head = b"@a\nACGT\n+\nIIII\n"
    want = {
        head + b"@b\nAC\n+x\nII": head + b"@b\nAC\n+x\nII\n",                       # the text's end closes the last line
        head + b"@b\nAC\n+\nII\r": head + b"@b\nAC\n+\nII\n",                       # ... and a trailing CR without a LF goes
        head + b"@b\nAC\n+\nII\r\r\n": head + b"@b\nAC\n+\nII\r\r\n",               # through the first LF, verbatim
        head + b"@b\nAC\n+\nII\n\n\r\n\n": head + b"@b\nAC\n+\nII\n",               # trailing blank lines are dropped
        head + b"@b\r\nAC\r\n+\r\nII\r\n\r\n": head + b"@b\r\nAC\r\n+\r\nII\r\n",
        head + b"@b\n\n+": head + b"@b\n\n+\n\n",                                   # three lines, no bases: both line ends supplied
        head + b"@b\n\n+\n": head + b"@b\n\n+\n\n",
        head + b"@b\n\n+\n\n": head + b"@b\n\n+\n\n",
        head + b"@b\n\n+\n\n\n\n": head + b"@b\n\n+\n\n",
        head + b"@b\r\n\r\n+z\r\n": head + b"@b\r\n\r\n+z\r\n\n",
        b"@\n\n+": b"@\n\n+\n\n",
    }
    for text, out in want.items():
        n = n_records(text, True)
        assert X.extract_chunk(text, True, [1] * n)[0] == out                       # (the model reads the header the same way)
        r = call(eng, mem, text, True, [1] * n, tshift=13, oshift=1)
        same_as_model(r, text, True, [1] * n)
        assert r.out == out and r.consumed == len(text) and r.out_bytes <= len(text) + 2
        last_only = [0] * (n - 1) + [1]
        same_as_model(call(eng, mem, text, True, last_only, oshift=15), text, True, last_only)
    for text in (b"", b"\n\r\n\n"):                                                 # no records
        for final in (True, False):
            r = call(eng, mem, text, final, [])
            assert (r.rc, r.out_bytes, r.n_kept) == (0, 0, 0) and r.consumed == (len(text) if final else 0)


# ---- 5. refusals: nothing is written -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", (DEVICE, HOST), ids=("device", "host"))
@pytest.mark.parametrize("case", BAD, ids=ids(BAD))
def test_format_errors(eng, case, mem):
    # the format comes first: whatever the flags and their number
    for nr in (0, 1, 3):
        r = call(eng, mem, case.text, True, [1] * nr, tshift=2, oshift=9)
        assert r.rc == KDF_ERR_IO and r.bad == case.bad
    try:
        recs, _ = X.records_of(case.text, False)
    except X.FormatError as ex:
        r = call(eng, mem, case.text, False, [1])
        assert r.rc == KDF_ERR_IO and r.bad == (ex.offset, ex.rule)
    else:                                                    # the bad record is not whole yet: the call takes the records before it
        same_as_model(call(eng, mem, case.text, False, [1] * len(recs)), case.text, False, [1] * len(recs))


@pytest.mark.parametrize("mem", (DEVICE, HOST), ids=("device", "host"))
def test_argument_refusals(eng, mem):
    reads = M.reads_of((30, 0, 45, 12), 51)
    text = M.fq(reads)
    keep = [1, 0, 1, 1]
    need = len(X.extract_chunk(text, True, keep)[0])
    for nr in (3, 5):                                        # n_reads off by one in either direction
        r = call(eng, mem, text, True, [1] * nr)
        assert r.rc == KDF_ERR_INVALID and b"4 records" in eng._lib.kdf_last_error(eng._h)
    r = call(eng, mem, text, True, keep, cap_out=need - 1)   # one byte short
    assert r.rc == KDF_ERR_INVALID
    same_as_model(call(eng, mem, text, True, keep, cap_out=need), text, True, keep)
    assert call(eng, mem, text, True, keep, null_keep=True).rc == KDF_ERR_INVALID
    assert call(eng, 2, text, True, keep).rc == KDF_ERR_INVALID
    assert call(eng, -1, text, True, keep).rc == KDF_ERR_INVALID
    assert call(eng, mem, text, True, keep, n_bytes=2 ** 31 + 1).rc == KDF_ERR_INVALID
    assert call(eng, mem, b"", True, [1], n_reads=1).rc == KDF_ERR_INVALID         # no text, one flag
    r = call(eng, mem, text[:20], False, [])                 # no complete record: nothing
    assert (r.rc, r.out_bytes, r.n_kept, r.consumed) == (0, 0, 0, 0)
    assert call(eng, mem, text[:20], False, [1]).rc == KDF_ERR_INVALID


def test_more_records_than_a_well_formed_text_holds(eng):
    """a text of line ends has more four-line records than the scratch is sized for: one of the first is bad, and reported"""
    for keep in ([], [1] * 5):
        r = call(eng, DEVICE, b"\n" * 1000 + b"x", True, keep)
        assert r.rc == KDF_ERR_IO and r.bad == (0, M.BAD_HEADER)
        r = call(eng, DEVICE, b"@\n\n+\n\n" * 3 + b"\n" * 1000 + b"x\n", False, keep)
        assert r.rc == KDF_ERR_IO and r.bad == (18, M.BAD_HEADER)
    r = call(eng, DEVICE, b"\n" * 1000, True, [])
    assert (r.rc, r.out_bytes, r.n_kept, r.consumed) == (0, 0, 0, 1000)


def test_engine_methods_raise_and_return(eng):
    from kmer_denovo_filter_amd._native import FastqFormatError, KdfError
    reads = M.reads_of((30, 0, 45, 12), 52)
    text = M.fq(reads, eol=b"\r\n")
    keep = np.array([0, 1, 1, 0], np.uint8)
    out, offs, consumed = X.extract_chunk(text, True, list(keep))
    got, got_offs, used = eng.fastq_extract(text, True, keep, want_offsets=True)
    assert (got, got_offs.tolist(), used) == (out, offs, consumed)
    assert eng.fastq_extract(text, True, keep) == (out, consumed)
    bad = [c for c in BAD if c.name == "bad_plus"][0]
    with pytest.raises(FastqFormatError) as ei:
        eng.fastq_extract(bad.text, True, [1, 1])
    assert (ei.value.offset, ei.value.rule) == bad.bad
    with pytest.raises(KdfError):
        eng.fastq_extract(text, True, keep[:3])
    p0 = eng.get_stat("fastqextract_passes")
    eng.profile(True)
    try:
        eng.fastq_extract(text, True, keep)
        assert eng.get_stat("fastqextract_passes") == p0 + 1 and eng.get_stat("fastqextract_us") > 0
    finally:
        eng.profile(False)


# ---- 6. chunks ------------------------------------------------------------------------------------------------------------------

def test_chunks_concatenate_to_the_whole(eng):
    rng = np.random.default_rng(61)
    reads = M.reads_of(rng.integers(0, 200, 300).tolist(), 61)
    text = M.fq(reads, header=lambda i: b"@r%d %s" % (i, b"x" * (i % 23)), final_newline=False, tail=b"\r\n\n")
    keep = (rng.random(len(reads)) < 0.3).astype(np.uint8)
    whole = X.extract_chunk(text, True, list(keep))[0]
    assert 0 < len(whole) < len(text)
    for trial in range(3):
        cuts = sorted(set(np.random.default_rng(70 + trial).integers(1, len(text), 9).tolist()))
        parts, left, done = [], b"", 0
        bounds = [0, *cuts, len(text)]
        for i in range(len(bounds) - 1):
            chunk, final = left + text[bounds[i]:bounds[i + 1]], i == len(bounds) - 2
            n = n_records(chunk, final)
            r = call(eng, DEVICE, chunk, final, keep[done:done + n], tshift=(len(left) + i) % 16, oshift=(3 * i) % 16)
            same_as_model(r, chunk, final, keep[done:done + n])
            parts.append(r.out)
            done += n
            left = chunk[r.consumed:]
        assert done == len(reads) and left == b"" and b"".join(parts) == whole


def test_two_runs_give_identical_bytes(eng):
    case = [c for c in GOOD if c.name == "random_150k"][0]
    keep = patterns(len(case.reads), 5)["random"]
    a = call(eng, DEVICE, case.text, True, keep, tshift=3, oshift=12)
    b = call(eng, DEVICE, case.text, True, keep, tshift=3, oshift=12)
    assert a.out == b.out and a.offsets == b.offsets and len(a.out) > 8 * T
