"""The k-mer FASTA codec on the device (include/kdf.h "k-mer FASTA codec"): kdf_format_kmers*, kdf_parse_kmer_fasta* and
the two wrappers of kmer_fasta.py, byte for byte against the host codec (``write_kmer_fasta``, ``read_kmer_fasta_keys``,
``keys.to_ascii``) and, where records do not start at 0, against a plain Python loop.  The largest case is 100 003 keys."""
import os
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [1, 5, 31, 32, 33, 47, 63, 65, 101, 201]           # bases on both sides of every word boundary
NS = [0, 1, 9, 10, 11, 100, 1001, 100_003]
FIRSTS = [0, 7, 99_990, 9_999_999_990]
FASTA, ROWS = 0, 1
GUARD = 64
FILL = 0xA5
GARBAGE = -0x0123456789ABCDEF
KDF_ERR_INVALID, KDF_ERR_IO = 1, 5


@pytest.fixture(scope="module")
def eng():
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(31, capacity_hint=1 << 10)            # (the codec's k is the call's, not the engine's)
    yield e
    e.close()


# ---- keys and truths ------------------------------------------------------------------------------------------------

def make_words(k, n, pattern, seed=0):
    """(W, n) uint64 key words with nothing above bit 2k: random, all A, all T, or alternating words"""
    from kmer_denovo_filter_amd import keys
    W = keys.n_words(k)
    if pattern == "random":
        w = np.random.default_rng(1000 * k + n + seed).integers(0, 1 << 64, (W, n), dtype=np.uint64)
    elif pattern == "A":
        w = np.zeros((W, n), np.uint64)
    elif pattern == "T":
        w = np.full((W, n), 0xFFFFFFFFFFFFFFFF, np.uint64)
    else:                                                # words of ...GTGT / ...TGTG in turn, the other way in every other key
        w = np.empty((W, n), np.uint64)
        for j in range(W):
            w[j, 0::2] = 0xBBBBBBBBBBBBBBBB if j % 2 == 0 else 0xEEEEEEEEEEEEEEEE
            w[j, 1::2] = 0xEEEEEEEEEEEEEEEE if j % 2 == 0 else 0xBBBBBBBBBBBBBBBB
    top = 2 * k - 64 * (W - 1)
    if top < 64:
        w[W - 1] &= np.uint64((1 << top) - 1)
    return w


def pair(words):
    from kmer_denovo_filter_amd import keys
    return keys.to_pair(words, zero_hi=False)


def host_fasta(tmp_path, words, k):
    """the host codec's file of these keys, as bytes (no sidecar)"""
    from kmer_denovo_filter_amd import kmer_fasta
    p = str(tmp_path / "host.fa")
    kmer_fasta.write_kmer_fasta(p, *pair(words), k, sidecar=False)
    with open(p, "rb") as f:
        return f.read()


def loop_fasta(words, k, first):
    from kmer_denovo_filter_amd import keys
    seqs = keys.to_ascii(words, k)
    return "".join(f">{first + i}\n{seqs[i].tobytes().decode()}\n" for i in range(len(seqs))).encode()


def host_keys(tmp_path, text, k, canonical):
    """``read_kmer_fasta_keys`` of a file that holds ``text``, no sidecar on disk"""
    from kmer_denovo_filter_amd import kmer_fasta
    p = str(tmp_path / "in.fa")
    with open(p, "wb") as f:
        f.write(text)
    assert not os.path.exists(p + ".kdfkeys.npz")
    return kmer_fasta.read_kmer_fasta_keys(p, k, canonical)


def same_keys(got, want, k):
    """two (lo, hi) pairs in the callers' form hold the same keys in the same order"""
    from kmer_denovo_filter_amd import keys
    a, b = np.asarray(keys.from_pair(*got, k)), np.asarray(keys.from_pair(*want, k))
    return a.shape == b.shape and (a == b).all()


# ---- device calls ---------------------------------------------------------------------------------------------------

def dev_keys(words):
    """device tensors of the callers' form -> (pointers (lo, hi), the tensors to keep alive)"""
    import torch
    lo, hi = pair(words)
    t = [None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in (lo, hi)]
    return tuple(0 if x is None or x.numel() == 0 else x.data_ptr() for x in t), t


def format_raw(eng, ptrs, n, k, layout, first, byte_first, byte_count, d_out):
    return eng._lib.kdf_format_kmers_dev(eng._h, c_void_p(ptrs[0]) if ptrs[0] else None, c_void_p(ptrs[1]) if ptrs[1] else None, n, k,
                                         layout, first, byte_first, byte_count, c_void_p(d_out) if d_out else None)


def format_windows(eng, words, k, layout, first, sizes, shift=0):
    """The text cut into windows of ``sizes`` bytes in turn (cyclic; a ragged last one), every window written behind its
    own guard bytes in one device buffer; ``shift``: the windows' output pointers are that far off a multiple of 16.
    -> the concatenation; asserts that every guard is intact."""
    import torch
    n = words.shape[1]
    ptrs, keep = dev_keys(words)
    total = eng.kmer_text_bytes(k, layout, first, n)
    wins, a, i = [], 0, 0
    while a < total:
        m = min(sizes[i % len(sizes)], total - a)
        wins.append((a, m))
        a, i = a + m, i + 1
    slot = [GUARD + shift + (m + 15) // 16 * 16 + GUARD for _, m in wins]
    offs = np.concatenate([[0], np.cumsum(slot)]).astype(np.int64)
    buf = torch.full((int(offs[-1]) + 16,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for (a, m), o in zip(wins, offs[:-1]):
        assert format_raw(eng, ptrs, n, k, layout, first, a, m, buf.data_ptr() + int(o) + GUARD + shift) == 0
    eng.synchronize()
    host = buf.cpu().numpy()
    out = []
    for (a, m), o, s in zip(wins, offs[:-1], slot):
        o = int(o)
        out.append(host[o + GUARD + shift:o + GUARD + shift + m].tobytes())
        assert (host[o:o + GUARD + shift] == FILL).all() and (host[o + GUARD + shift + m:o + s] == FILL).all(), f"window [{a}, +{m}): a guard byte was written"
    assert (host[int(offs[-1]):] == FILL).all()
    return b"".join(out)


def format_whole(eng, words, k, layout, first=0):
    total = eng.kmer_text_bytes(k, layout, first, words.shape[1])
    return format_windows(eng, words, k, layout, first, [max(total, 16)])


def parse_raw(eng, text, k, canonical, final, cap=None):
    """kdf_parse_kmer_fasta_dev over ``text`` -> (rc, n_out, consumed, bad_offset, (lo, hi) of the first min(cap, n_out)
    rows); asserts that nothing behind those rows was written.  cap None: room for every line; cap 0: NULL outputs."""
    import torch
    from kmer_denovo_filter_amd import keys
    W = keys.n_words(k)
    t = np.frombuffer(bytes(text), np.uint8)
    if cap is None:
        cap = len(t) // (k + 1) + 1
    d_t = torch.from_numpy(t.copy()).cuda() if len(t) else None
    shape = (cap + 2, W) if W > 2 else (cap + 2,)
    d_lo = torch.full(shape, GARBAGE, dtype=torch.int64, device="cuda")
    d_hi = torch.full((cap + 2,), GARBAGE, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n, consumed, bad = c_uint64(0), c_uint64(0), c_uint64(0)
    rc = eng._lib.kdf_parse_kmer_fasta_dev(eng._h, c_void_p(d_t.data_ptr()) if d_t is not None else None, len(t), k, int(canonical), int(final),
                                           c_void_p(d_lo.data_ptr()) if cap else None, c_void_p(d_hi.data_ptr()) if cap and W == 2 else None,
                                           cap, byref(n), byref(consumed), byref(bad))
    eng.synchronize()
    lo, hi = d_lo.cpu().numpy(), d_hi.cpu().numpy()
    w = min(cap, n.value) if rc in (0, KDF_ERR_INVALID) else cap
    assert (lo[w:] == GARBAGE).all() and (hi[w if W == 2 else 0:] == GARBAGE).all(), "a write past the first min(cap, n_out) rows"
    return rc, n.value, consumed.value, bad.value, (lo[:w].view(np.uint64), hi[:w].view(np.uint64) if W == 2 else None)


def parse_ok(eng, text, k, canonical=True, final=True):
    rc, n, consumed, bad, got = parse_raw(eng, text, k, canonical, final)
    assert rc == 0 and bad == 2 ** 64 - 1 and n == len(got[0])
    return got, consumed


# ---- format -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_format_and_round_trip(eng, tmp_path, k):
    """both layouts of every n and key pattern against the host codec, and the text parsed back into the keys"""
    from kmer_denovo_filter_amd import keys
    for n in NS:
        for pattern in (("random",) if n > 1001 else ("random", "A", "T", "alt")):
            words = make_words(k, n, pattern)
            want = host_fasta(tmp_path, words, k)
            assert eng.kmer_text_bytes(k, FASTA, 0, n) == len(want)
            got = format_whole(eng, words, k, FASTA)
            assert got == want, (k, n, pattern)
            assert format_whole(eng, words, k, ROWS) == keys.to_ascii(words, k).tobytes(), (k, n, pattern)
            # the round trip: the forward keys are the keys, the canonical ones the host reader's
            back, consumed = parse_ok(eng, got, k, canonical=False)
            assert consumed == len(got) and same_keys(back, pair(words), k), (k, n, pattern)
            if n <= 1001:
                back, _ = parse_ok(eng, got, k, canonical=True)
                assert same_keys(back, host_keys(tmp_path, got, k, True), k), (k, n, pattern)


@pytest.mark.parametrize("k", KS)
def test_format_first_index(eng, k):
    for first in FIRSTS:
        for n in (1, 25, 2000):                          # 99 990 + 25 and 9 999 999 990 + 25 gain a digit on the way
            words = make_words(k, n, "random", seed=first % 97)
            want = loop_fasta(words, k, first)
            assert eng.kmer_text_bytes(k, FASTA, first, n) == len(want)
            assert format_whole(eng, words, k, FASTA, first) == want, (k, first, n)


# ---- windows ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,n,first,sizes", [
    (31, 1001, 0, [16]), (31, 1001, 0, [48]), (31, 1001, 99_990, [16]), (1, 1001, 0, [16]), (5, 300, 9_999_999_990, [48, 16]),
    (33, 700, 95, [48]), (63, 500, 0, [16, 4096]), (65, 400, 0, [48]), (201, 300, 99_990, [16, 48]),
    (31, 100_003, 0, [4096]), (31, 100_003, 0, [65_536 + 16]), (47, 20_000, 99_990, [4096, 65_536 + 16, 16, 48]),
    (101, 20_000, 0, [65_536 + 16, 4096]), (32, 5000, 7, [4096]),
])
def test_windows(eng, k, n, first, sizes):
    words = make_words(k, n, "random")
    want = loop_fasta(words, k, first)
    assert format_windows(eng, words, k, FASTA, first, sizes) == want
    if n <= 5000:
        from kmer_denovo_filter_amd import keys
        assert format_windows(eng, words, k, ROWS, 0, sizes) == keys.to_ascii(words, k).tobytes()


@pytest.mark.parametrize("k", [31, 47, 101])
def test_windows_into_unaligned_buffers(eng, k):
    words = make_words(k, 777, "random")
    want = loop_fasta(words, k, 95)
    for shift in (1, 8, 15):
        assert format_windows(eng, words, k, FASTA, 95, [4096, 48], shift=shift) == want


def test_format_refusals_write_nothing(eng):
    import torch
    k, n = 31, 100
    words = make_words(k, n, "random")
    ptrs, keep = dev_keys(words)
    total = eng.kmer_text_bytes(k, FASTA, 0, n)
    buf = torch.full((total + 4096,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = buf.data_ptr() + GUARD
    for byte_first, byte_count in ((8, 16), (1, 1), (17, 0), (0, total + 1), (16, total - 15), (total // 16 * 16 + 16, 0), (total // 16 * 16 + 16, 1),
                                   (2 ** 63, 16)):
        assert format_raw(eng, ptrs, n, k, FASTA, 0, byte_first, byte_count, out) == KDF_ERR_INVALID, (byte_first, byte_count)
    for kk, layout, first, nn in ((64, FASTA, 0, n), (66, FASTA, 0, n), (0, FASTA, 0, n), (31, 2, 0, n), (31, FASTA, 2 ** 63 - 50, n)):
        assert format_raw(eng, ptrs, nn, kk, layout, first, 0, 16, out) == KDF_ERR_INVALID, (kk, layout, first)
    # nothing to do is no error: an empty window (also at the very end), no keys
    assert format_raw(eng, ptrs, n, k, FASTA, 0, 16, 0, out) == 0
    assert format_raw(eng, ptrs, n, k, ROWS, 0, n * k // 16 * 16, 0, out) == 0
    assert format_raw(eng, (0, 0), 0, k, FASTA, 0, 0, 0, 0) == 0
    eng.synchronize()
    assert (buf.cpu().numpy() == FILL).all()
    with pytest.raises(Exception):
        eng.format_kmers_dev(ptrs[0], None, n, k, FASTA, 0, 8, 16, out)


@pytest.mark.parametrize("k", [5, 31, 33, 63, 65, 201])
def test_host_form_equals_device_form(eng, k):
    from kmer_denovo_filter_amd import keys
    words = make_words(k, 1500, "random")
    lo, hi = pair(words)
    want = loop_fasta(words, k, 99_990)
    assert eng.format_kmers(lo, hi, k, FASTA, 99_990).tobytes() == want
    assert eng.format_kmers(lo, hi, k, FASTA, 99_990, 4096, 1000).tobytes() == want[4096:5096]
    assert eng.format_kmers(lo, hi, k, ROWS).tobytes() == keys.to_ascii(words, k).tobytes()
    assert len(eng.format_kmers(lo[:0], None if hi is None else hi[:0], k)) == 0
    # ... and of the parse
    got = eng.parse_kmer_fasta(want, k, canonical=False)
    assert got[2] == len(want) and same_keys(got[:2], (lo, hi), k)
    dev, consumed = parse_ok(eng, want, k, canonical=True)
    got = eng.parse_kmer_fasta(np.frombuffer(want, np.uint8), k)
    assert same_keys(got[:2], dev, k)
    lo0, hi0, c0 = eng.parse_kmer_fasta(b"", k)
    assert len(lo0) == 0 and c0 == 0


def test_profile_stats(eng):
    words = make_words(31, 100, "random")
    eng.profile(True)
    try:
        p0 = eng.get_stat("kmerfasta_passes")
        text = format_whole(eng, words, 31, FASTA)
        parse_ok(eng, text, 31)
        assert eng.get_stat("kmerfasta_passes") == p0 + 2 and eng.get_stat("kmerfasta_us") > 0
    finally:
        eng.profile(False)


# ---- parse ------------------------------------------------------------------------------------------------------------

def revcomp(seq: bytes) -> bytes:
    return seq.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def variants(words, k):
    """the same records dressed differently: (name, text)"""
    from kmer_denovo_filter_amd import keys
    seqs = [s.tobytes() for s in keys.to_ascii(words, k)]
    lf = b"".join(b">%d\n%s\n" % (i, s) for i, s in enumerate(seqs))
    return [
        ("lf", lf),
        ("crlf", lf.replace(b"\n", b"\r\n")),
        ("lower", lf.lower()),
        ("mixed case", b"".join(b">%d\n%s\n" % (i, bytes(c | 0x20 if (i + j) % 3 == 0 else c for j, c in enumerate(s))) for i, s in enumerate(seqs))),
        ("no final newline", lf[:-1]),
        ("crlf, no final newline", lf.replace(b"\n", b"\r\n")[:-2]),
        ("crlf, ends in cr", lf.replace(b"\n", b"\r\n")[:-1]),
        ("blank lines", b"\n\n" + lf.replace(b"\n>", b"\n\n\r\n>") + b"\n\r\n\n"),
        ("no headers", b"".join(s + b"\n" for s in seqs)),
        ("long headers", b"".join(b">" + b"x" * 5000 + b" %d\n%s\n" % (i, s) for i, s in enumerate(seqs[:40]))),
        ("reverse complements", b"".join(b">%d\n%s\n" % (i, revcomp(s)) for i, s in enumerate(seqs))),
    ]


@pytest.mark.parametrize("k", [1, 5, 31, 32, 33, 63, 65, 101, 201])
def test_parse_equals_host_reader(eng, tmp_path, k):
    words = make_words(k, 300, "random")
    for name, text in variants(words, k):
        for canonical in (True, False):
            want = host_keys(tmp_path, text, k, canonical)
            got, consumed = parse_ok(eng, text, k, canonical)
            assert consumed == len(text) and same_keys(got, want, k), (k, name, canonical)


@pytest.mark.parametrize("text", [b"", b"\n", b"\r\n", b">only a header", b">a\n>b\n", b">a\r\n>b\r\n\r\n", b">" + b"h" * 5000 + b"\n>" + b"g" * 9000, b"\r"])
def test_parse_files_without_keys(eng, tmp_path, text):
    for k in (31, 65):
        want = host_keys(tmp_path, text, k, True)
        got, consumed = parse_ok(eng, text, k)
        assert len(want[0]) == 0 and len(got[0]) == 0 and consumed == len(text)


@pytest.mark.parametrize("k", [2, 4, 32, 34, 62])
def test_parse_even_k_palindromes(eng, tmp_path, k):
    """a k-mer that is its own reverse complement: the tie of the canonical minimum is the same key"""
    rng = np.random.default_rng(k)
    half = ["ACGT"[i] for i in rng.integers(0, 4, k // 2)]
    pal = ("".join(half)).encode()
    pal = pal + revcomp(pal)
    assert revcomp(pal) == pal and len(pal) == k
    other = bytes(rng.choice(list(b"ACGT"), k).tolist())
    text = b">0\n" + pal + b"\n>1\n" + other + b"\n>2\n" + pal.lower() + b"\n"
    for canonical in (True, False):
        got, _ = parse_ok(eng, text, k, canonical)
        assert same_keys(got, host_keys(tmp_path, text, k, canonical), k)
    fwd, _ = parse_ok(eng, text, k, False)
    can, _ = parse_ok(eng, text, k, True)
    assert fwd[0][0] == can[0][0] == can[0][2]


@pytest.mark.parametrize("k", [31, 47, 101])
def test_parse_cap_and_sizing(eng, k):
    words = make_words(k, 500, "random")
    text = loop_fasta(words, k, 0)
    rc, n, consumed, bad, _ = parse_raw(eng, text, k, False, True, cap=0)          # the sizing call
    assert (rc, n, consumed) == (KDF_ERR_INVALID, 500, len(text))
    assert eng.parse_kmer_fasta_dev(0, 0, k, False, True, None, None, 0) == (0, 0)
    for cap in (1, 255, 499):
        rc, n, consumed, bad, got = parse_raw(eng, text, k, False, True, cap=cap)  # (parse_raw: nothing behind row cap was written)
        assert (rc, n, consumed) == (KDF_ERR_INVALID, 500, len(text))
        assert same_keys(got, pair(words[:, :cap]), k)
    rc, n, consumed, bad, got = parse_raw(eng, text, k, False, True, cap=500)
    assert rc == 0 and same_keys(got, pair(words), k)
    # a sizing call through the Python face
    import torch
    d = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    assert eng.parse_kmer_fasta_dev(d.data_ptr(), len(text), k, True, True, None, None, 0) == (500, len(text))


# ---- chunks -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,name", [(31, "lf"), (31, "crlf"), (5, "crlf"), (47, "blank lines"), (65, "crlf"), (31, "long headers"), (201, "lf")])
def test_parse_cut_at_every_offset(eng, k, name):
    """the file handed over in two chunks, cut at every offset of 200 bytes around a record: inside a header, inside a
    sequence, between '\\r' and '\\n'"""
    words = make_words(k, 60, "random")
    text = dict(variants(words, k))[name]
    whole, _ = parse_ok(eng, text, k)
    c0 = text.index(b"\n>", len(text) // 3) - 40                     # 40 bytes before the end of a sequence line
    for cut in range(c0, c0 + 200):
        first, consumed = parse_ok(eng, text[:cut], k, final=False)
        assert consumed == text.rfind(b"\n", 0, cut) + 1, cut
        rest, consumed2 = parse_ok(eng, text[consumed:], k, final=True)
        assert consumed2 == len(text) - consumed
        joined = tuple(None if a is None else np.concatenate([a, b]) for a, b in zip(first, rest))
        assert same_keys(joined, whole, k), cut


def feed(eng, text, k, chunk, canonical=True):
    """the wrapper's loop over the C call with a buffer of ``chunk`` bytes: the tail in front of the next chunk, a header
    longer than the buffer skipped without growing it"""
    parts, buf, pos, in_header = [], b"", 0, False
    while True:
        take = text[pos:pos + chunk - len(buf)]
        pos += len(take)
        buf += take
        eof = pos >= len(text)
        if in_header:
            j = buf.find(b"\n")
            if j < 0:
                buf = b""
                if eof:
                    break
                continue
            buf, in_header = buf[j + 1:], False
            if not eof:
                continue
        got, consumed = parse_ok(eng, buf, k, canonical, final=eof)
        parts.append(got)
        if eof:
            break
        if consumed == 0 and len(buf) == chunk:
            assert buf[:1] == b">"
            buf, in_header = b"", True
            continue
        buf = buf[consumed:]
    return tuple(None if p[0] is None else np.concatenate(p) for p in zip(*parts))


@pytest.mark.parametrize("k,name,chunk", [(31, "lf", 64), (31, "crlf", 100), (31, "long headers", 1000), (31, "long headers", 5003),
                                          (65, "long headers", 4096), (5, "blank lines", 16), (101, "crlf", 300)])
def test_parse_in_small_chunks(eng, k, name, chunk):
    words = make_words(k, 60, "random")
    text = dict(variants(words, k))[name]
    whole, _ = parse_ok(eng, text, k)
    assert same_keys(feed(eng, text, k, chunk), whole, k)


def test_parse_chunk_without_newline(eng):
    for text in (b">" + b"h" * 300, b"ACGT" * 100, b"\rACGT"):
        rc, n, consumed, bad, _ = parse_raw(eng, text, 31, True, False)
        assert (rc, n, consumed, bad) == (0, 0, 0, 2 ** 64 - 1), text[:8]


# ---- errors -----------------------------------------------------------------------------------------------------------

def scan_bad(text, k, final):
    """(offset, rule) of the first bad line of a chunk, by the rule of ``read_kmer_fasta_keys``; None: every line is fine"""
    if final and text and not text.endswith(b"\n"):
        text += b"\n"
    pos = 0
    while True:
        e = text.find(b"\n", pos)
        if e < 0:
            return None
        line = text[pos:e]
        if line.endswith(b"\r"):
            line = line[:-1]
        if line and not line.startswith(b">"):
            if len(line) != k:
                return pos, "length"
            if any(c not in b"ACGTacgt" for c in line):
                return pos, "base"
        pos = e + 1


ERROR_K = [5, 31, 33, 65]


@pytest.mark.parametrize("k", ERROR_K)
def test_parse_errors(eng, tmp_path, k):
    from kmer_denovo_filter_amd import kmer_fasta
    words = make_words(k, 400, "random")
    good = loop_fasta(words, k, 0)
    lines = good.split(b"\n")                              # 2 i: header, 2 i + 1: sequence of record i

    def with_line(i, new, sep=b"\n"):
        x = list(lines)
        x[2 * i + 1] = new
        return sep.join(x)

    s = lines[2 * 123 + 1]
    cases = {
        "short": with_line(123, s[:-1]), "long": with_line(123, s + b"A"), "N": with_line(123, s[:k // 2] + b"N" + s[k // 2 + 1:]),
        "short crlf": with_line(123, s[:-1], b"\r\n"), "long crlf": with_line(123, s + b"C", b"\r\n"),
        "cr in the line": with_line(123, s[:k // 2] + b"\r" + s[k // 2 + 1:]), "k bytes ending in cr": with_line(123, s[:-1] + b"\r"),
        "two lines in one": with_line(123, s + s), "space": with_line(123, s[:-1] + b" "), "nul": with_line(123, b"\0" + s[1:]),
        "first line": with_line(0, s[:-1]), "last line": with_line(399, s + b"G"),
        "base then length": with_line(7, b"N" + s[1:]).replace(lines[2 * 300 + 1], lines[2 * 300 + 1] + b"T"),
        "length then base": with_line(7, s[1:]).replace(lines[2 * 300 + 1], b"n" + lines[2 * 300 + 1][1:]),
        "two in one tile": with_line(200, b"N" + s[1:]).replace(lines[2 * 201 + 1], lines[2 * 201 + 1][:-1]),
    }
    for name, text in cases.items():
        want = scan_bad(text, k, True)
        assert want is not None, name
        rc, n, consumed, bad, _ = parse_raw(eng, text, k, True, True)
        assert rc == KDF_ERR_IO and bad == want[0], (k, name, bad, want)
        msg = eng._lib.kdf_last_error(eng._h).decode()
        assert ("non-ACGT" in msg) == (want[1] == "base") and (f"length != k={k}" in msg) == (want[1] == "length"), (name, msg)
        with pytest.raises(ValueError) as ei:
            eng.parse_kmer_fasta(text, k)
        assert ei.value.offset == want[0] and ei.value.rule == want[1]
        # the same report in the sizing call, and whatever the first chunk's end
        rc, n, consumed, bad, _ = parse_raw(eng, text, k, True, True, cap=0)
        assert rc == KDF_ERR_IO and bad == want[0]
        cut = want[0] + 3 * k + 40
        if cut < len(text):
            rc, n, consumed, bad, _ = parse_raw(eng, text[:cut], k, True, False)
            assert rc == KDF_ERR_IO and bad == want[0], (k, name)
    # the wrapper raises where the host function does, with its words (one bad line: the first is the only one)
    for name in ("short", "long", "N", "short crlf", "cr in the line", "k bytes ending in cr", "first line", "last line", "nul"):
        p = str(tmp_path / "bad.fa")
        with open(p, "wb") as f:
            f.write(cases[name])
        with pytest.raises(ValueError) as host:
            kmer_fasta.read_kmer_fasta_keys(p, k)
        with pytest.raises(ValueError) as dev:
            kmer_fasta.read_kmer_fasta_keys_device(p, k)
        assert str(dev.value) == str(host.value), name


@pytest.mark.parametrize("k", ERROR_K)
def test_parse_last_line_cut_short(eng, k):
    words = make_words(k, 50, "random")
    good = loop_fasta(words, k, 0)
    for drop in (2, k // 2 + 1, k):                        # the last line keeps k - 1 bases, about half of them, one base ... and no '\n'
        text = good[:len(good) - drop]
        rc, n, consumed, bad, got = parse_raw(eng, text, k, False, False)          # not the last chunk: the line is not looked at
        assert (rc, n, bad) == (0, 49, 2 ** 64 - 1) and consumed == text.rfind(b"\n") + 1
        assert same_keys(got, pair(words[:, :49]), k)
        rc, n, consumed, bad, _ = parse_raw(eng, text, k, False, True)             # the last chunk: it is too short
        assert rc == KDF_ERR_IO and bad == text.rfind(b"\n") + 1 == scan_bad(text, k, True)[0]
    # an unfinished line with a bad base in it is no error either until it ends
    text = good[:-4] + b"N"
    rc, n, consumed, bad, _ = parse_raw(eng, text, k, False, False)
    assert (rc, n, bad) == (0, 49, 2 ** 64 - 1)


# ---- the wrappers -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,n", [(31, 0), (31, 1), (31, 100_003), (47, 30_000), (101, 20_000), (5, 100_003)])
def test_wrappers_equal_the_host_codec(eng, tmp_path, monkeypatch, k, n):
    """the file and the sidecar of write_kmer_fasta_device are write_kmer_fasta's, through several windows; the device
    reader gives the host reader's keys with and without the sidecar"""
    import torch
    from kmer_denovo_filter_amd import devkeys, kmer_fasta
    monkeypatch.setenv("KDF_FASTA_CHUNK_MB", "1")
    words = make_words(k, n, "random")
    lo, hi = pair(words)
    host_path, dev_path = str(tmp_path / "host.fa"), str(tmp_path / "dev.fa")
    kmer_fasta.write_kmer_fasta(host_path, lo, hi, k)
    dlo, dhi = devkeys.from_host(lo, hi, wide=33 <= k <= 63)
    assert kmer_fasta.write_kmer_fasta_device(dev_path, dlo, dhi, k, engine=eng) == n
    assert kmer_fasta.LAST_FASTA_CODEC == "device"
    assert open(dev_path, "rb").read() == open(host_path, "rb").read()
    a, b = np.load(host_path + ".kdfkeys.npz"), np.load(dev_path + ".kdfkeys.npz")
    for f in ("lo", "hi", "k"):
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and (a[f] == b[f]).all(), f
    st = os.stat(dev_path)
    assert int(b["size"]) == st.st_size and int(b["mtime_ns"]) == st.st_mtime_ns
    got = kmer_fasta.read_kmer_fasta_keys_device(dev_path, k)
    assert kmer_fasta.LAST_FASTA_CODEC == "sidecar"
    for canonical in (True, False):
        os.path.exists(dev_path + ".kdfkeys.npz") and os.remove(dev_path + ".kdfkeys.npz")
        want = kmer_fasta.read_kmer_fasta_keys(dev_path, k, canonical)
        got = kmer_fasta.read_kmer_fasta_keys_device(dev_path, k, canonical)       # (the codec's own engine)
        assert kmer_fasta.LAST_FASTA_CODEC == "device"
        assert got[0].is_cuda and got[0].dtype == torch.int64 and (got[1] is None) == (not 33 <= k <= 63)
        assert same_keys(devkeys.to_host(*got), want, k)
    # records numbered from elsewhere, no sidecar
    if 0 < n <= 30_000:
        kmer_fasta.write_kmer_fasta_device(dev_path, dlo, dhi, k, engine=eng, first_index=99_990, sidecar=False)
        assert open(dev_path, "rb").read() == loop_fasta(words, k, 99_990) and not os.path.exists(dev_path + ".kdfkeys.npz")


def test_reader_with_small_windows(eng, tmp_path, monkeypatch):
    """windows shorter than a header: the reader skips the header without growing its buffers"""
    from kmer_denovo_filter_amd import devkeys, kmer_fasta
    k = 31
    words = make_words(k, 60, "random")
    for name, win in (("long headers", 4096), ("long headers", 1 << 16), ("crlf", 4096), ("blank lines", 4096)):
        text = dict(variants(words, k))[name]
        p = str(tmp_path / "small.fa")
        with open(p, "wb") as f:
            f.write(text)
        want = kmer_fasta.read_kmer_fasta_keys(p, k)
        monkeypatch.setattr(kmer_fasta, "_window_bytes", lambda: win)
        got = kmer_fasta.read_kmer_fasta_keys_device(p, k, engine=eng)
        monkeypatch.undo()
        assert same_keys(devkeys.to_host(*got), want, k), (name, win)
    # a sequence line longer than a window is a line of the wrong length
    p = str(tmp_path / "longline.fa")
    with open(p, "wb") as f:
        f.write(b">0\n" + b"ACGT" * 2000 + b"\n")
    monkeypatch.setattr(kmer_fasta, "_window_bytes", lambda: 4096)
    with pytest.raises(ValueError, match="length != k=31"):
        kmer_fasta.read_kmer_fasta_keys_device(p, k, engine=eng)
