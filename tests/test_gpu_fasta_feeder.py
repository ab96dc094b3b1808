"""The device FASTA feeder on the GPU (include/kdf.h "device FASTA feeder"): kdf_fasta_pack_dev against the host reader's
single batch and against the numpy model of the header's rule (tests/fasta_stream_model.py, which the CPU test pins to
the host reader and the oracle on the same case list), word for word -- the words behind n_bases and the bytes around
the buffers included -- then through ``count_dev`` against the host path's table and the oracle's, and through
``reads.stream_fasta_device`` and the KDF_DEVICE_FASTA_FEEDER switch.  The largest text is the long random case (~150 KB)."""
import gzip
import os

import numpy as np
import pytest

import fasta_stream_model as M

pytestmark = pytest.mark.gpu

T = 4096                                                 # KDF_FASTA_TILE_BYTES (test_abi_fasta_feeder.py holds it to the header)
FILL = 0xA5
FILL64 = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD_WORDS = 8                                          # 64 bytes behind kdf_stream_words(cap_bases)
KDF_ERR_INVALID = 1
NAMED = b">ab\r\nAC\r\r\nG\n>c\nT\n"                     # CR LF, CR CR LF, two headers: every cut of it is taken
CASES = M.cases() + [("named_cuts", NAMED)]
IDS = [name for name, _ in CASES]
SMALL = [(n, t) for n, t in CASES if len(t) <= 256]
LARGE = [(n, t) for n, t in CASES if len(t) > 256]


@pytest.fixture(scope="module")
def eng():
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(31, capacity_hint=1 << 10)            # (any engine packs any FASTA)
    yield e
    e.close()


# ---- one call, with everything around its buffers checked -----------------------------------------------------------

class Out:
    """what one call wrote: the words of the stream, the offsets, and that nothing else was touched"""


def dev_text(text: bytes, shift: int = 0):
    """the text on the device, ``shift`` bytes behind a 16-byte boundary -> (pointer, tensor to keep)"""
    import torch
    buf = torch.full((len(text) + 48,), 0x3E, dtype=torch.uint8, device="cuda")      # ('>' around it: a read outside shows)
    base = (-buf.data_ptr()) % 16 + 16 + shift
    if len(text):
        buf[base:base + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    return buf.data_ptr() + base, buf


def dev_stream(codes):
    """a model stream as device words -> (packed tensor, mask tensor)"""
    import torch
    p, m = M.to_words(codes)
    return torch.from_numpy(p.view(np.int64)).cuda(), torch.from_numpy(m.view(np.int64)).cuda()


def call(eng, text, final, state, prev=None, carry=0, shift=0, cap_bases=None, cap_reads=None, want_offsets=True, expect_error=False):
    """kdf_fasta_pack_dev into buffers pre-filled with 0xA5 -> Out.  prev: (packed tensor, mask tensor, n_bases)"""
    import torch
    from kmer_denovo_filter_amd._native import KdfError
    from kmer_denovo_filter_amd.reads import stream_words
    if cap_bases is None:
        cap_bases = len(text) + carry + 1
    if cap_reads is None:
        cap_reads = len(text) // 2 + 2
    pw, mw = stream_words(cap_bases)
    fill = int(FILL64.view(np.int64))
    packed = torch.full((pw + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda")
    invalid = torch.full((mw + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda")
    offs = torch.full((cap_reads + 1 + GUARD_WORDS,), fill, dtype=torch.int64, device="cuda")
    ptr, keep = dev_text(text, shift)
    torch.cuda.synchronize()                                 # (torch filled the buffers on ITS stream; the engine launches on its own)
    before = state.copy()
    o = Out()
    o.error = None
    try:
        o.n_bases, o.n_reads, o.consumed = eng.fasta_pack_dev(
            ptr if len(text) else None, len(text), final, state, packed.data_ptr(), invalid.data_ptr(), cap_bases,
            offs.data_ptr() if want_offsets else None, cap_reads if want_offsets else 0,
            prev[0].data_ptr() if prev else None, prev[1].data_ptr() if prev else None, prev[2] if prev else 0, carry)
    except KdfError as ex:
        assert expect_error, ex
        o.error = ex.code
    else:
        assert not expect_error
    torch.cuda.synchronize()
    o.tensors = (packed, invalid)
    hp, hm, ho = (x.cpu().numpy().view(np.uint64) for x in (packed, invalid, offs))
    assert (hp[pw:] == FILL64).all() and (hm[mw:] == FILL64).all() and (ho[cap_reads + 1:] == FILL64).all(), "guard bytes were written"
    if o.error is not None:                                  # refused: nothing written, state unchanged
        assert (hp == FILL64).all() and (hm == FILL64).all() and (ho == FILL64).all()
        assert (state.flags, state.records, state.positions) == (before.flags, before.records, before.positions)
        return o
    if len(text) == 0 and not final:                         # emits nothing, writes nothing
        assert (o.n_bases, o.n_reads, o.consumed) == (0, 0, 0)
        assert (hp == FILL64).all() and (hm == FILL64).all() and (ho == FILL64).all()
        o.packed, o.invalid, o.offsets = hp[:0], hm[:0], np.zeros(1, np.int64)
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
    """the call's words are those of the model's stream, with the tail of the host reader's finish()"""
    assert o.n_bases == len(codes)
    packed, invalid = M.to_words(codes)
    assert (o.packed == packed).all(), np.flatnonzero(o.packed != packed)[:4]
    assert (o.invalid == invalid).all(), np.flatnonzero(o.invalid != invalid)[:4]
    assert o.n_reads == len(offsets) - 1
    if o.offsets is not None:
        assert (o.offsets == offsets).all()


def model_state(st):
    return M.State(st.flags, st.records, st.positions)


def host_batch(tmp_path, text, k=31):
    from kmer_denovo_filter_amd.reads import fasta_reader
    p = str(tmp_path / "case.fa")
    with open(p, "wb") as f:
        f.write(text)
    return list(fasta_reader(p, k, max_bases=1 << 22, max_reads=1 << 16))


def final_chunk_is_the_host_batch(eng, tmp_path, text, shifts=(0,)):
    from kmer_denovo_filter_amd._native import FastaState
    codes, offsets = M.pack_file(text)
    batches = host_batch(tmp_path, text)
    assert len(batches) == (1 if len(offsets) > 1 else 0)
    for shift in shifts:
        st = FastaState()
        o = call(eng, text, True, st, shift=shift)
        assert o.consumed == len(text)
        same_as_model(o, codes, offsets)
        assert model_state(st) == M.State(0, len(offsets) - 1, len(codes))
        if batches:
            b = batches[0]
            assert o.n_bases == b.n_bases and o.n_reads == len(b.offsets) - 1
            assert (o.packed == b.packed).all() and (o.invalid == b.invalid).all() and (o.offsets == b.offsets).all()
        else:
            assert o.n_bases == 0 and o.n_reads == 0


# ---- 1. one final chunk ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,text", CASES, ids=IDS)
def test_one_final_chunk(eng, tmp_path, name, text):
    final_chunk_is_the_host_batch(eng, tmp_path, text, shifts=(0, 1, 7, 15))


def test_without_offsets(eng):
    from kmer_denovo_filter_amd._native import FastaState
    text = dict(CASES)["random_w60_crlf"]
    codes, offsets = M.pack_file(text)
    o = call(eng, text, True, FastaState(), want_offsets=False)
    same_as_model(o, codes, offsets)


# ---- 2. chunk invariance --------------------------------------------------------------------------------------------

def run_cuts(eng, text, cuts, carry=0):
    """the calls of M.pack_cuts on the device, each compared with the model's: words, offsets, consumed, state"""
    from kmer_denovo_filter_amd._native import FastaState
    calls = M.pack_cuts(text, cuts, carry)
    st, prev = FastaState(), None
    for i, (codes, offsets, consumed, after, chunk) in enumerate(calls):
        final = i == len(calls) - 1
        if codes is None:                                        # a chunk of CR only that is not the last
            o = call(eng, chunk, final, st, prev=prev, carry=carry, expect_error=True)
            assert o.error == KDF_ERR_INVALID
            continue
        o = call(eng, chunk, final, st, prev=prev, carry=carry)
        assert o.consumed == consumed
        assert model_state(st) == after, (i, chunk)
        if len(chunk) or final:
            same_as_model(o, codes, offsets)
            prev = (*o.tensors, o.n_bases)
    return calls


@pytest.mark.parametrize("name,text", SMALL, ids=[n for n, _ in SMALL])
def test_every_cut_in_two_chunks(eng, name, text):
    for cut in range(len(text) + 1):
        run_cuts(eng, text, [cut])


@pytest.mark.parametrize("name,text", LARGE, ids=[n for n, _ in LARGE])
def test_random_cut_sets(eng, name, text):
    rng = np.random.default_rng(len(text))
    for rep in range(3):
        cuts = sorted(rng.integers(0, len(text) + 1, int(rng.integers(2, 9))).tolist())
        run_cuts(eng, text, cuts)


def test_a_chunk_of_cr_only(eng):
    from kmer_denovo_filter_amd._native import FastaState
    calls = run_cuts(eng, NAMED, [7, 8])                         # ">ab\r\nAC" | "\r" | "\r\nG..."
    assert calls[1][0] is None
    o = call(eng, b"\r\r\r", False, FastaState(), expect_error=True)
    assert o.error == KDF_ERR_INVALID


# ---- 3. tile edges --------------------------------------------------------------------------------------------------

def seq(n, seed=0):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()


def wrapped(s, width, eol=b"\n"):
    return b"".join(s[a:a + width] + eol for a in range(0, len(s), width))


def sized(size, seed):
    """a multi-FASTA of exactly ``size`` bytes"""
    text = b""
    r = 0
    while len(text) < size:
        text += b">rec%d\n" % r + wrapped(seq(700 + 13 * r, seed + r), 60)
        r += 1
    return text[:size]


TILE_TEXTS = {
    "T-1": sized(T - 1, 1), "T": sized(T, 2), "T+1": sized(T + 1, 3), "2T+1": sized(2 * T + 1, 4),
    "header_straddles": b">a\n" + wrapped(seq(T - 3 - 50 - 66, 5), 60) + b">" + b"h" * 100 + b"\n" + wrapped(seq(300, 6), 60),
    "header_two_tiles": b">a\nACGT\n>" + b"x>y " * (T // 2 + 100) + b"\nACGTN\n>z\nAC\n",
    "cr_ends_tile": b">a\r\n" + seq(T - 5, 7) + b"\r\n" + wrapped(seq(200, 8), 60, b"\r\n"),
    "line_three_tiles": b">s\n" + seq(3 * T + 77, 9),
    "word_sizes": b"".join(b">r%d\n" % n + seq(n, n) + b"\n" for n in (31, 32, 33, 63, 64, 65)) * 40,
    "no_line_start": b">a\n" + seq(T - 3 + 100, 10) + b"N" * T + seq(50, 11) + b"\n>b\nAC",
}


def test_tile_texts_are_what_they_say():
    assert [len(TILE_TEXTS[n]) for n in ("T-1", "T", "T+1", "2T+1")] == [T - 1, T, T + 1, 2 * T + 1]
    t = TILE_TEXTS["header_straddles"]
    a = t.index(b">h")
    assert a < T < a + 100
    t = TILE_TEXTS["cr_ends_tile"]
    assert t[T - 1:T + 1] == b"\r\n"
    assert b"\n" not in TILE_TEXTS["line_three_tiles"][3:] and b"\n" not in TILE_TEXTS["no_line_start"][T:2 * T]
    assert len(TILE_TEXTS["word_sizes"]) > 2 * T


@pytest.mark.parametrize("name", list(TILE_TEXTS))
def test_tile_edges(eng, tmp_path, name):
    text = TILE_TEXTS[name]
    final_chunk_is_the_host_batch(eng, tmp_path, text, shifts=(0, 7))
    for cuts in ([T], [T - 1], [T + 1, 2 * T], [len(text) // 3]):
        run_cuts(eng, text, [c for c in cuts if c <= len(text)])


# ---- 4. carry and counting ------------------------------------------------------------------------------------------

def table_of(e):
    lo, hi, cnt = e.export_ge(0)
    if e.long:
        keys = [sum(int(x) << (64 * j) for j, x in enumerate(row)) for row in lo]
    else:
        keys = [int(a) | ((int(b) << 64) if hi is not None else 0) for a, b in zip(lo, hi if hi is not None else lo)]
    return keys, cnt.tolist()


def count_chunked(e, text, chunk, k):
    """the file through fasta_pack_dev in chunks of ``chunk`` bytes with carry = k - 1, each stream counted -> carries seen"""
    from kmer_denovo_filter_amd._native import FastaState
    st, prev, left, carries = FastaState(), None, b"", []
    for a in range(0, max(len(text), 1), chunk):
        piece = left + text[a:a + chunk]
        final = a + chunk >= len(text)
        open_before = bool(st.flags & M.IN_RECORD)
        o = call(e, piece, final, st, prev=prev, carry=k - 1)
        left = piece[o.consumed:]
        carries.append(min(k - 1, prev[2]) if (prev and open_before) else 0)
        if o.n_bases:
            e.count_dev(o.tensors[0].data_ptr(), o.tensors[1].data_ptr(), o.n_bases)
        prev = (*o.tensors, o.n_bases)
    e.synchronize()
    return carries


def host_table(e, tmp_path, text, k):
    from kmer_denovo_filter_amd.reads import fasta_reader
    p = str(tmp_path / "host.fa")
    with open(p, "wb") as f:
        f.write(text)
    e.clear()
    with fasta_reader(p, k, max_bases=1 << 22) as rd:
        for b in rd:
            e.count(b)
    return table_of(e)


def oracle_table(oracle, records, k):
    if k <= 63:
        lo, hi, cnt = oracle.OracleTable(k).count_reads(records).export_ge(0)
        return [int(a) | (int(b) << 64) for a, b in zip(lo, hi)], cnt.tolist()
    items = sorted((oracle.kmer_to_int(s), c) for s, c in oracle.py_count(records, k).items())     # the long tests' truth
    return [v for v, _ in items], [c for _, c in items]


@pytest.fixture(scope="module")
def mini_ref(giab):
    with open(os.path.join(giab, "mini_ref.fa"), "rb") as f:
        return f.read()


@pytest.mark.parametrize("k", [5, 31, 63, 101])
def test_carry_and_count(tmp_path, oracle, mini_ref, giab, k):
    from kmer_denovo_filter_amd import KmerEngine
    records = [s for _, s in oracle.read_fasta(os.path.join(giab, "mini_ref.fa"))]
    truth = oracle_table(oracle, records, k)
    with KmerEngine(k, capacity_hint=1 << 16) as e:
        want = host_table(e, tmp_path, mini_ref, k)
        assert want == truth
        for chunk in (1000, 4099):
            e.clear()
            carries = count_chunked(e, mini_ref, chunk, k)
            assert any(carries)
            assert table_of(e) == want, (k, chunk)


def test_carry_corner_cases(tmp_path):
    """a chunk that ends exactly at a record's end (the carry crosses the separator: no window gained or lost), and a
    previous stream shorter than k - 1"""
    from kmer_denovo_filter_amd import KmerEngine
    k = 31
    a, b, c = seq(80, 21), seq(12, 22), seq(90, 23)
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        text = b">a\n" + a + b"\n>b\n" + c + b"\n"
        want = host_table(e, tmp_path, text, k)
        e.clear()
        carries = count_chunked(e, text, len(b">a\n" + a + b"\n"), k)       # chunk 2 begins with '>': its separator follows the carry
        assert carries[:2] == [0, k - 1] and table_of(e) == want
        text = b">s\n" + b + a + c + b"\n"
        want = host_table(e, tmp_path, text, k)
        e.clear()
        carries = count_chunked(e, text, 3 + len(b), k)                      # the first stream holds 12 < k - 1 positions
        assert carries[:2] == [0, len(b)] and table_of(e) == want
        assert len(want[0]) == len(b + a + c) - k + 1


# ---- 5. errors ------------------------------------------------------------------------------------------------------

def test_refusals(eng):
    from kmer_denovo_filter_amd._native import FastaState
    text = dict(CASES)["random_w61_lf"]
    codes, offsets = M.pack_file(text)
    o = call(eng, text, True, FastaState(), cap_bases=len(codes) - 1, expect_error=True)
    assert o.error == KDF_ERR_INVALID
    o = call(eng, text, True, FastaState(), cap_reads=len(offsets) - 2, expect_error=True)
    assert o.error == KDF_ERR_INVALID
    same_as_model(call(eng, text, True, FastaState(), cap_bases=len(codes), cap_reads=len(offsets) - 1), codes, offsets)   # exactly enough
    same_as_model(call(eng, text, True, FastaState(), cap_reads=0, want_offsets=False), codes, offsets)                   # no offsets: cap_reads does not count


def test_equal_prev_and_output_are_refused(eng):
    import torch
    from kmer_denovo_filter_amd._native import FastaState, KdfError
    from kmer_denovo_filter_amd.reads import stream_words
    text = b">a\nACGT\n"
    pw, mw = stream_words(64)
    packed = torch.full((pw,), 7, dtype=torch.int64, device="cuda")
    invalid = torch.full((mw,), 7, dtype=torch.int64, device="cuda")
    other = torch.full((pw,), 7, dtype=torch.int64, device="cuda")
    ptr, keep = dev_text(text)
    for pp, pm in ((packed, other), (other, invalid), (packed, invalid)):
        st = FastaState(M.IN_RECORD, 0, 1, 5)
        with pytest.raises(KdfError) as ei:
            eng.fasta_pack_dev(ptr, len(text), True, st, packed.data_ptr(), invalid.data_ptr(), 64, None, 0, pp.data_ptr(), pm.data_ptr(), 5, 4)
        assert ei.value.code == KDF_ERR_INVALID
        assert (st.flags, st.records, st.positions) == (M.IN_RECORD, 1, 5)
        torch.cuda.synchronize()
        assert bool((packed == 7).all()) and bool((invalid == 7).all())


def test_empty_calls(eng):
    from kmer_denovo_filter_amd._native import FastaState
    st = FastaState(M.IN_RECORD | M.MID_LINE, 0, 3, 40)
    o = call(eng, b"", False, st)                                    # nothing
    assert (st.flags, st.records, st.positions) == (M.IN_RECORD | M.MID_LINE, 3, 40)
    prev_codes = np.array([0, 1, 2, 3, 4, 1], np.uint8)
    p, m = dev_stream(prev_codes)
    o = call(eng, b"", True, st, prev=(p, m, len(prev_codes)), carry=4)     # closes the record behind the carry
    same_as_model(o, np.array([2, 3, 4, 1, 4], np.uint8), np.array([0, 5]))
    assert (st.flags, st.records, st.positions) == (0, 3, 41)
    st = FastaState()
    o = call(eng, b"", True, st)                                     # no record was open
    same_as_model(o, np.zeros(0, np.uint8), np.array([0]))
    assert (st.flags, st.records, st.positions) == (0, 0, 0)


def test_host_form(eng):
    from kmer_denovo_filter_amd._native import FastaState
    text = dict(CASES)["random_w60_crlf"]
    calls = M.pack_cuts(text, [len(text) // 2], carry=30)
    st, prev = FastaState(), None
    for i, (codes, offsets, consumed, after, chunk) in enumerate(calls):
        stream, used = eng.fasta_pack(chunk, i == 1, st, prev=prev, carry=30)
        packed, invalid = M.to_words(codes)
        assert used == consumed and stream.n_bases == len(codes) and model_state(st) == after
        assert (stream.packed == packed).all() and (stream.invalid == invalid).all() and (stream.offsets == offsets).all()
        prev = stream


def test_profile_stats(eng):
    from kmer_denovo_filter_amd._native import FastaState
    eng.profile(True)
    try:
        call(eng, dict(CASES)["mini_ref"], True, FastaState())
        assert eng.get_stat("fastafeed_passes") == 1 and eng.get_stat("fastafeed_us") > 0
    finally:
        eng.profile(False)


# ---- 6. wrapper and switch ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("compressed", [False, True], ids=["plain", "gzip"])
def test_stream_fasta_device(tmp_path, giab, mini_ref, compressed):
    from kmer_denovo_filter_amd import KmerEngine, reads
    path = os.path.join(giab, "mini_ref.fa")
    if compressed:
        path = str(tmp_path / "mini_ref.fa.gz")
        with gzip.open(path, "wb") as f:
            f.write(mini_ref[:20000])
        with gzip.open(path, "ab") as f:                             # a second member
            f.write(mini_ref[20000:])
    k = 31
    with KmerEngine(k, capacity_hint=1 << 16) as e:
        want = host_table(e, tmp_path, mini_ref, k)
        e.clear()
        n = reads.stream_fasta_device(e, path, k, chunk_bytes=4096)
        info = reads.LAST_FASTA_FEEDER
        assert n == mini_ref.count(b"\n>") + 1 == 24
        assert info["path"] == "device" and info["compressed"] == compressed and info["bytes"] == len(mini_ref)
        assert info["chunks"] == -(-len(mini_ref) // 4096) and info["carries"] >= info["chunks"] - 1
        assert table_of(e) == want


def _index_bytes(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("k", [31, 75])
def test_switch_ensure_ref_jf(tmp_path, monkeypatch, mini_ref, k):
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as JW
    monkeypatch.setenv("KDF_FASTA_FEED_MB", str(8192 / (1 << 20)))
    out = {}
    for mode in ("host", "device"):
        d = tmp_path / mode
        d.mkdir()
        ref = str(d / "ref.fa")
        with open(ref, "wb") as f:
            f.write(mini_ref)
        if mode == "device":
            monkeypatch.setenv("KDF_DEVICE_FASTA_FEEDER", "1")
        else:
            monkeypatch.delenv("KDF_DEVICE_FASTA_FEEDER", raising=False)
        monkeypatch.chdir(d)
        jf = JW._ensure_ref_jf("ref.fa", k, 4)
        out[mode] = _index_bytes(jf)
        assert JW.LAST_FASTA_FEEDER["path"] == mode
    assert JW.LAST_FASTA_FEEDER["chunks"] > 1
    assert out["host"] == out["device"] and len(out["host"]) > 1000


def test_switch_build_proband_jf_index(tmp_path, monkeypatch):
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as JW
    k = 31
    kmers = [seq(k, 100 + i) for i in range(500)]
    fa = str(tmp_path / "proband_unique.fa")
    with open(fa, "wb") as f:
        f.write(b"".join(b">%d\n%s\n" % (i, s) for i, s in enumerate(kmers)))
    out = {}
    d = tmp_path / "index"                                           # (the index records its own path: one place for both)
    d.mkdir()
    for mode in ("host", "device"):
        if mode == "device":
            monkeypatch.setenv("KDF_DEVICE_FASTA_FEEDER", "1")
        else:
            monkeypatch.delenv("KDF_DEVICE_FASTA_FEEDER", raising=False)
        jf = JW._build_proband_jf_index(fa, k, str(d), n_proband_unique=len(kmers))
        out[mode] = _index_bytes(jf)
        os.remove(jf)
        assert JW.LAST_FASTA_FEEDER["path"] == mode
    assert out["host"] == out["device"] and len(out["host"]) > 1000
