"""The index record codec on the device (include/kdf.h "index record codec"): kdf_index_encode, kdf_index_decode,
kdf_jf_positions, kdf_jf_order and the device writers and loaders of jf_io.py, against the host codec -- the body
``jf_io.write_index`` writes, ``jf_io._decode``, ``jf_io.jf_positions``, ``keys.order`` -- and, for tiny n, a
``struct.pack`` loop.  The largest case is 100 003 records."""
import os
import struct
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

KS = [1, 4, 5, 31, 32, 33, 47, 63, 65, 101, 201]         # R = 5 5 6 12 12 13 16 20 21 30 55: below, at and across 16; W = 1 .. 7
NS = [0, 1, 2, 3, 15, 16, 17, 255, 256, 257, 1001, 100_003]
CBS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16]
JF_KS = [1, 15, 31, 32, 33, 47, 63]
HOST, DEVICE = 0, 1
MEMS = [pytest.param(HOST, id="host"), pytest.param(DEVICE, id="device")]
GUARD = 64
FILL = 0xA5
KDF_ERR_INVALID, KDF_ERR_IO = 1, 5
FIXTURE = os.path.join(ROOT, "tests", "golden", "giab", "mini_ref.fa.k31.jf")
P = lambda x: c_void_p(x) if x else None                 # noqa: E731


@pytest.fixture(scope="module")
def eng():
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(31, capacity_hint=1 << 10)            # (the codec's k is the call's, not the engine's)
    yield e
    e.close()


# ---- keys, counts and truths ----------------------------------------------------------------------------------------

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
    else:
        w = np.empty((W, n), np.uint64)
        for j in range(W):
            w[j, 0::2] = 0xBBBBBBBBBBBBBBBB if j % 2 == 0 else 0xEEEEEEEEEEEEEEEE
            w[j, 1::2] = 0xEEEEEEEEEEEEEEEE if j % 2 == 0 else 0xBBBBBBBBBBBBBBBB
    top = 2 * k - 64 * (W - 1)
    if top < 64:
        w[W - 1] &= np.uint64((1 << top) - 1)
    return w


def make_counts(n, seed=0):
    """uint32 counts: random, with 0, 1 and 2^32 - 1 among them"""
    c = np.random.default_rng(77 + n + seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    c[0::7], c[1::7], c[2::7] = 0, 1, 0xFFFFFFFF
    return c


def pair(words):
    from kmer_denovo_filter_amd import keys
    return keys.to_pair(words, zero_hi=False)


def host_body(tmp_path, words, counts, k, perm=None):
    """the record area of the file ``jf_io.write_index`` writes for these records (in the order of ``perm``)"""
    from kmer_denovo_filter_amd import jf_io
    if perm is not None:
        words, counts = words[:, perm], None if counts is None else counts[perm]
    if counts is None:
        counts = np.zeros(words.shape[1], np.uint32)
    p = str(tmp_path / "host.jf")
    jf_io.write_index(p, k, *pair(words), counts)
    _, off = jf_io.read_header(p)
    with open(p, "rb") as f:
        return f.read()[off:]


def loop_body(words, counts, k, perm=None):
    kb = (2 * k + 7) // 8
    out = []
    for e in range(words.shape[1]):
        i = e if perm is None else int(perm[e])
        v = sum(int(words[j, i]) << (64 * j) for j in range(words.shape[0]))
        out.append(v.to_bytes(words.shape[0] * 8, "little")[:kb] + struct.pack("<I", 0 if counts is None else int(counts[i])))
    return b"".join(out)


# ---- buffers in either memory kind ----------------------------------------------------------------------------------

class Mem:
    """arrays in host or device memory by the call's ``mem``; pointers 16-byte aligned plus an offset"""

    def __init__(self, mem):
        self.mem, self.keep = mem, []

    def put(self, a, offset=0, before=0, after=0, rng=None):
        """the array's bytes at ``offset`` past a 16-aligned address with ``before`` / ``after`` dirty bytes around -> pointer (0: None or empty)"""
        import torch
        if a is None or a.size == 0 and not (before or after):
            return 0
        raw = np.ascontiguousarray(a).view(np.uint8).ravel()
        lead = 16 * ((before + 15) // 16) + offset
        dirty = (rng or np.random.default_rng(5)).integers(1, 256, lead + len(raw) + after + 32, dtype=np.uint8)
        dirty[lead:lead + len(raw)] = raw
        if self.mem == DEVICE:
            t = torch.from_numpy(dirty).cuda()
            base = t.data_ptr()
        else:
            t = np.empty(len(dirty) + 16, np.uint8)
            shift = (-t.ctypes.data) % 16
            t[shift:shift + len(dirty)] = dirty
            base = t.ctypes.data + shift
        assert base % 16 == 0
        self.keep.append(t)
        return base + lead

    def out(self, nbytes, offset=0):
        """a buffer of ``nbytes`` at ``offset`` past a 16-aligned address between guards -> (pointer, reader): reader() gives the
        bytes and asserts the guards"""
        import torch
        total = GUARD + 16 + nbytes + GUARD + 16
        if self.mem == DEVICE:
            t = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
            base, shift = t.data_ptr(), 0
        else:
            t = np.full(total + 16, FILL, np.uint8)
            shift = (-t.ctypes.data) % 16
            base = t.ctypes.data + shift
        assert base % 16 == 0
        at = GUARD + offset
        self.keep.append(t)

        def read(what="output"):
            host = t.cpu().numpy() if self.mem == DEVICE else t
            host = host[shift:shift + total]
            assert (host[:at] == FILL).all() and (host[at + nbytes:] == FILL).all(), f"{what}: a guard byte was written"
            return host[at:at + nbytes].copy()
        return base + at, read


def key_ptrs(M, words):
    lo, hi = pair(words)
    return M.put(lo), M.put(hi)


def encode_raw(eng, mem, lo, hi, counts, perm, n, k, byte_first, byte_count, out):
    return eng._lib.kdf_index_encode(eng._h, mem, P(lo), P(hi), P(counts), P(perm), n, k, byte_first, byte_count, P(out))


def encode_windows(eng, mem, words, counts, perm, k, wins, offset=0):
    """every window (byte_first, byte_count) into its own guarded buffer at ``offset`` past a 16-aligned address -> list of bytes"""
    import torch
    M = Mem(mem)
    n = words.shape[1]
    lo, hi = key_ptrs(M, words)
    c = M.put(counts)
    pm = M.put(None if perm is None else np.asarray(perm, np.uint32))
    outs = [M.out(m, offset) for _, m in wins]
    if mem == DEVICE:
        torch.cuda.synchronize()
    for (a, m), (ptr, _) in zip(wins, outs):
        assert encode_raw(eng, mem, lo, hi, c, pm, n, k, a, m, ptr) == 0, (k, n, a, m)
    eng.synchronize()
    return [read(f"k={k} n={n} window [{a}, +{m}) offset {offset}").tobytes() for (a, m), (_, read) in zip(wins, outs)]


# ---- encode ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("k", KS)
def test_encode_equals_the_host_body(eng, tmp_path, k, mem):
    R = eng.index_record_bytes(k)
    assert R == (2 * k + 7) // 8 + 4
    rng = np.random.default_rng(k)
    for n in NS:
        for pattern in (["random", "A", "T", "alt"] if n <= 1001 else ["random"]):
            words, counts = make_words(k, n, pattern), make_counts(n)
            want = host_body(tmp_path, words, counts, k)
            total = n * R
            assert len(want) == total
            if n <= 17:
                assert want == loop_body(words, counts, k)
            wins = [(0, total)]
            if n <= 17:                                  # every split at a multiple of 16
                wins += [w for s in range(0, total + 1, 16) for w in ((0, s), (s, total - s))]
            elif pattern == "random":                    # windows that start and end inside records
                for _ in range(6):
                    a = 16 * int(rng.integers(0, total // 16))
                    wins.append((a, int(rng.integers(1, min(total - a, 9000) + 1))))
            got = encode_windows(eng, mem, words, counts, None, k, wins)
            for (a, m), g in zip(wins, got):
                assert g == want[a:a + m], f"k={k} n={n} {pattern} window [{a}, +{m})"


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("k", KS)
def test_encode_unaligned_output_null_counts_and_perm(eng, tmp_path, k, mem):
    R = eng.index_record_bytes(k)
    rng = np.random.default_rng(100 + k)
    for n in (3, 17, 257, 1001):
        words, counts = make_words(k, n, "random", seed=1), make_counts(n, seed=1)
        total = n * R
        want = host_body(tmp_path, words, counts, k)
        wins = [(0, total), (16, total - 16 - 1), (total // 32 * 16, total - total // 32 * 16)]
        wins = [(a, m) for a, m in wins if m > 0]
        for offset in (0, 1, 8):
            for (a, m), g in zip(wins, encode_windows(eng, mem, words, counts, None, k, wins, offset)):
                assert g == want[a:a + m], f"k={k} n={n} offset {offset} window [{a}, +{m})"
        zero = host_body(tmp_path, words, None, k)
        assert encode_windows(eng, mem, words, None, None, k, [(0, total)])[0] == zero
        for name, perm in (("identity", np.arange(n)), ("reversed", np.arange(n)[::-1]), ("random", rng.permutation(n))):
            wantp = host_body(tmp_path, words, counts, k, perm)
            if n <= 17:
                assert wantp == loop_body(words, counts, k, perm)
            wp = [(0, total), (16 * (total // 48), total - 16 * (total // 48) - 3)]
            for (a, m), g in zip(wp, encode_windows(eng, mem, words, counts, perm, k, wp, offset=1 if name == "random" else 0)):
                assert g == wantp[a:a + m], f"k={k} n={n} perm {name} window [{a}, +{m})"


@pytest.mark.parametrize("k", [5, 31, 63, 101])
def test_encode_largest_case_through_a_permutation(eng, tmp_path, k):
    n = 100_003
    words, counts = make_words(k, n, "random", seed=2), make_counts(n, seed=2)
    perm = np.random.default_rng(k).permutation(n)
    want = host_body(tmp_path, words, counts, k, perm)
    total = len(want)
    wins = [(0, total), (total // 32 * 16, 70_001)]
    for (a, m), g in zip(wins, encode_windows(eng, DEVICE, words, counts, perm, k, wins)):
        assert g == want[a:a + m]


@pytest.mark.parametrize("mem", MEMS)
def test_encode_refusals_leave_the_output_untouched(eng, mem):
    n, k = 100, 31
    words, counts = make_words(k, n, "random"), make_counts(n)
    R = eng.index_record_bytes(k)
    M = Mem(mem)
    lo, hi = key_ptrs(M, words)
    c, pm = M.put(counts), M.put(np.arange(n, dtype=np.uint32))
    out, read = M.out(n * R)
    cases = [
        ("byte_first % 16", dict(byte_first=8, byte_count=16)),
        ("window past the body", dict(byte_first=0, byte_count=n * R + 1)),
        ("window begins past the body", dict(byte_first=(n * R + 15) // 16 * 16 + 16, byte_count=0)),
        ("k = 0", dict(k=0)), ("k = 64", dict(k=64)), ("k = 66", dict(k=66)), ("k = 202", dict(k=202)),
        ("mem", dict(mem=2)),
        ("n * R >= 2^63", dict(n=(1 << 63) // R + 1)),
        ("perm and n >= 2^32", dict(n=1 << 32, perm=pm)),
    ]
    for what, over in cases:
        a = dict(mem=mem, lo=lo, hi=hi, counts=c, perm=0, n=n, k=k, byte_first=0, byte_count=16, out=out)
        a.update(over)
        assert encode_raw(eng, **a) == KDF_ERR_INVALID, what
        assert eng._lib.kdf_last_error(eng._h)
    eng.synchronize()
    assert (read("refusals") == FILL).all()
    assert encode_raw(eng, mem, lo, hi, c, 0, n, k, 16, 0, out) == 0 and encode_raw(eng, mem, 0, 0, 0, 0, 0, k, 0, 0, 0) == 0
    eng.synchronize()
    assert (read("empty windows") == FILL).all()
    assert encode_raw(eng, mem, lo, hi, c, 0, ((1 << 63) - 1) // R, k, 0, 0, out) == 0


# ---- decode ---------------------------------------------------------------------------------------------------------

def make_records(words, k, cb, seed=0):
    """structured records (k: kb bytes, c: cb bytes) of the keys with counts that straddle 2^32 - 1; cb > 8: zero and non-zero tails"""
    from kmer_denovo_filter_amd import keys
    n = words.shape[1]
    kb = (2 * k + 7) // 8
    rng = np.random.default_rng(31 * k + cb + n + seed)
    c64 = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    edge = np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF, 0x100000000, 0x100000001, 0xFFFFFFFFFFFFFFFF, 0x1FFFFFFFF], np.uint64)
    pick = rng.integers(0, 3, n)
    c64 = np.where(pick == 0, edge[rng.integers(0, len(edge), n)], np.where(pick == 1, c64 >> np.uint64(32), c64))
    cbytes = np.zeros((n, 16), np.uint8)
    cbytes[:, :8] = c64.view(np.uint8).reshape(n, 8)
    tail = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    tail[rng.random(n) < 0.6] = 0
    lone = rng.random(n) < 0.2                           # a single set byte, the record's very last one
    tail[lone] = 0
    cbytes[:, 8:] = tail
    if cb > 8:
        cbytes[lone, cb - 1] = 1
    data = np.zeros(n, np.dtype([("k", "u1", (kb,)), ("c", "u1", (cb,))]))
    data["k"] = keys.to_bytes(words, k)
    data["c"] = cbytes[:, :cb]
    return data


def decode_raw(eng, mem, data, k, cb, offset=0, want_hi=None, want_counts=True, seed=0):
    """kdf_index_decode over the records at ``offset`` past a 16-aligned address, dirty bytes around them -> (rc, bad, lo, hi or
    None, counts or None) as host arrays of exactly n rows; asserts the output guards"""
    from kmer_denovo_filter_amd import keys
    n, W = len(data), keys.n_words(k)
    M = Mem(mem)
    src = M.put(data, offset, before=48, after=48, rng=np.random.default_rng(seed + offset)) if n else 0
    want_hi = W == 2 if want_hi is None else want_hi
    lo, rlo = M.out(n * 8 * (W if W > 2 else 1))
    hi, rhi = M.out(n * 8) if want_hi else (0, None)
    cnt, rcnt = M.out(n * 4) if want_counts else (0, None)
    bad = c_uint64(123)
    if mem == DEVICE:
        import torch
        torch.cuda.synchronize()
    rc = eng._lib.kdf_index_decode(eng._h, mem, P(src), n, k, cb, P(lo), P(hi), P(cnt), byref(bad))
    glo = rlo("lo").view(np.uint64)
    return (rc, bad.value, glo.reshape(n, W) if W > 2 else glo, rhi("hi").view(np.uint64) if rhi else None,
            rcnt("counts").view(np.uint32) if rcnt else None)


def check_decoded(got, data, k, cb, what):
    from kmer_denovo_filter_amd import jf_io
    kb = (2 * k + 7) // 8
    lo, hi, counts = jf_io._decode(data, kb, cb)
    _, _, glo, ghi, gcnt = got
    assert np.array_equal(glo, np.asarray(lo, np.uint64).reshape(glo.shape)), f"{what}: lo"
    if ghi is not None:
        assert np.array_equal(ghi, np.zeros(len(data), np.uint64) if hi is None else hi), f"{what}: hi"
    if gcnt is not None:
        assert np.array_equal(gcnt, counts), f"{what}: counts"


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("k", KS)
def test_decode_equals_the_host_rule(eng, k, mem):
    for cb in CBS:
        for i, n in enumerate(NS):
            if n == 100_003 and cb not in (4, 9):
                continue
            data = make_records(make_words(k, n, "random" if n > 3 else "T"), k, cb)
            offset = (5 * i + cb) % 16
            got = decode_raw(eng, mem, data, k, cb, offset)
            assert got[:2] == (0, 0xFFFFFFFFFFFFFFFF), (k, cb, n, got[:2])
            check_decoded(got, data, k, cb, f"k={k} cb={cb} n={n} offset {offset}")
    for pattern in ("A", "T", "alt"):
        data = make_records(make_words(k, 257, pattern), k, 4)
        check_decoded(decode_raw(eng, mem, data, k, 4, 3), data, k, 4, f"k={k} {pattern}")


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("k", KS)
def test_decode_at_every_offset_and_with_null_outputs(eng, k, mem):
    for cb in (4, 9):
        data = make_records(make_words(k, 257, "random", seed=3), k, cb, seed=3)
        for offset in range(16):
            got = decode_raw(eng, mem, data, k, cb, offset)
            assert got[0] == 0
            check_decoded(got, data, k, cb, f"k={k} cb={cb} offset {offset}")
    data = make_records(make_words(k, 300, "random", seed=4), k, 4)
    got = decode_raw(eng, mem, data, k, 4, 7, want_counts=False)
    assert got[0] == 0 and got[4] is None
    check_decoded(got, data, k, 4, "no counts")
    if k <= 32:                                          # hi is optional: NULL, or filled with zeros
        got = decode_raw(eng, mem, data, k, 4, 9, want_hi=True)
        assert got[0] == 0 and not got[3].any()
        check_decoded(got, data, k, 4, "hi given at k <= 32")


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("k", [k for k in KS if 2 * k % 8])          # (k = 4 and 32 fill their key bytes: no such bit exists)
def test_decode_reports_the_first_bad_record(eng, k, mem):
    kb = (2 * k + 7) // 8
    for n in (1, 257, 1001):
        for spots in ([0], [n // 2], [n - 1], [n // 3, n - 1], [0, n // 2]):
            for bit in (2 * k, 8 * kb - 1):
                data = make_records(make_words(k, n, "random", seed=5), k, 4)
                for s in set(spots):
                    data["k"][s, bit // 8] |= np.uint8(1 << (bit % 8))
                runs = [decode_raw(eng, mem, data, k, 4, 5) for _ in range(2)]
                for got in runs:
                    assert got[:2] == (KDF_ERR_IO, min(spots)), (k, n, spots, bit, got[:2])
                    check_decoded(got, data, k, 4, f"k={k} n={n} bad {spots}: rows as read")
                assert b"record" in eng._lib.kdf_last_error(eng._h)


@pytest.mark.parametrize("mem", MEMS)
def test_decode_refusals(eng, mem):
    data = make_records(make_words(31, 10, "random"), 31, 4)
    M = Mem(mem)
    src = M.put(data)
    lo, rlo = M.out(80)
    bad = c_uint64(5)
    call = lambda **o: eng._lib.kdf_index_decode(eng._h, o.get("mem", mem), P(src), 10, o.get("k", 31), o.get("cb", 4), P(o.get("lo", lo)), None, None, byref(bad))  # noqa: E731
    for over in (dict(k=0), dict(k=64), dict(k=66), dict(k=202), dict(cb=0), dict(cb=17), dict(mem=3), dict(lo=0), dict(k=47)):
        assert call(**over) == KDF_ERR_INVALID, over
        assert bad.value == 0xFFFFFFFFFFFFFFFF
    eng.synchronize()
    assert (rlo() == FILL).all()
    assert eng._lib.kdf_index_decode(eng._h, mem, None, 0, 31, 4, None, None, None, None) == 0


@pytest.mark.parametrize("k", KS)
def test_round_trip_through_the_python_face(eng, k):
    from kmer_denovo_filter_amd.engine import IndexRecordError
    for n in (0, 1, 17, 1001):
        words, counts = make_words(k, n, "random", seed=6), make_counts(n, seed=6)
        lo, hi = pair(words)
        body = eng.index_encode(lo, hi, counts, k)
        assert body.dtype == np.uint8 and len(body) == n * eng.index_record_bytes(k)
        glo, ghi, gcnt = eng.index_decode(body, k)
        assert np.array_equal(glo, lo) and np.array_equal(gcnt, counts) and (ghi is None if hi is None else np.array_equal(ghi, hi))
        if n:
            perm = np.random.default_rng(n).permutation(n)
            glo, ghi, gcnt = eng.index_decode(eng.index_encode(lo, hi, counts, k, perm=perm).tobytes(), k)
            assert np.array_equal(glo, lo[perm]) and np.array_equal(gcnt, counts[perm])
            part = eng.index_encode(lo, hi, counts, k, byte_first=16 * (len(body) // 32), byte_count=min(40, len(body) - 16 * (len(body) // 32)))
            assert part.tobytes() == body.tobytes()[16 * (len(body) // 32):][:40]
    with pytest.raises(ValueError):
        eng.index_decode(b"\0" * 7, 31)
    if 2 * k % 8:
        body = eng.index_encode(*pair(make_words(k, 9, "random")), None, k)
        body[4 * eng.index_record_bytes(k) + (2 * k) // 8] |= 1 << (2 * k % 8)
        with pytest.raises(IndexRecordError) as ei:
            eng.index_decode(body, k)
        assert ei.value.record == 4


# ---- positions and order --------------------------------------------------------------------------------------------

def distinct_words(k, n, seed=0):
    """(W, m) distinct keys, m = min(n, 4^k)"""
    if n == 0:
        return make_words(k, 0, "random")
    w = make_words(k, min(2 * n, 1 << 18), "random", seed=seed)
    rows = np.unique(w.T, axis=0)
    rng = np.random.default_rng(seed + k)
    return np.ascontiguousarray(rows[rng.permutation(len(rows))[:n]].T)


def column_sets(k):
    from kmer_denovo_filter_amd import jf_io
    sets = [(jf_io.jf_make_matrix(2 * k, r), 1 << r) for r in (10, 40)]
    if k == 31:
        hd, _ = jf_io.read_header(FIXTURE)
        assert hd["matrix1"]["r"] == 27 and hd["key_len"] == 62
        sets.append((hd["matrix1"]["columns"], hd["size"]))
    return sets


def host_positions(cols, size, words, k):
    from kmer_denovo_filter_amd import jf_io
    return jf_io.jf_positions(cols, 2 * k, *pair(words)) & np.uint64(size - 1)


def positions_raw(eng, mem, words, k, cols, size):
    M = Mem(mem)
    n = words.shape[1]
    lo, hi = key_ptrs(M, words)
    out, read = M.out(n * 8)
    c = np.ascontiguousarray([int(x) for x in cols], dtype=np.uint64)
    if mem == DEVICE:
        import torch
        torch.cuda.synchronize()
    rc = eng._lib.kdf_jf_positions(eng._h, mem, P(lo), P(hi), n, k, c.ctypes.data_as(eng._lib.kdf_jf_positions.argtypes[6]), size, P(out))
    eng.synchronize()
    return rc, read("positions").view(np.uint64)


def order_raw(eng, mem, words, k, cols, size):
    M = Mem(mem)
    n = words.shape[1]
    lo, hi = key_ptrs(M, words)
    out, read = M.out(n * 4)
    c = np.ascontiguousarray([int(x) for x in cols], dtype=np.uint64)
    if mem == DEVICE:
        import torch
        torch.cuda.synchronize()
    rc = eng._lib.kdf_jf_order(eng._h, mem, P(lo), P(hi), n, k, c.ctypes.data_as(eng._lib.kdf_jf_order.argtypes[6]), size, P(out))
    return rc, read("order").view(np.uint32)


@pytest.mark.parametrize("mem", MEMS)
@pytest.mark.parametrize("k", JF_KS)
def test_positions_and_order_equal_the_host_rule(eng, k, mem):
    from kmer_denovo_filter_amd import keys
    for cols, size in column_sets(k):
        for n in (0, 1, 3, 257, 1001, 100_003):
            words = distinct_words(k, n, seed=n)
            want = host_positions(cols, size, words, k)
            rc, pos = positions_raw(eng, mem, words, k, cols, size)
            assert rc == 0 and np.array_equal(pos, want), (k, size, n)
            rc, perm = order_raw(eng, mem, words, k, cols, size)
            assert rc == 0 and np.array_equal(perm, keys.order(words, want).astype(np.uint32)), (k, size, n)
    words = distinct_words(k, 500)
    cols, size = column_sets(k)[0]
    assert np.array_equal(eng.jf_positions(*pair(words), k, cols, size), host_positions(cols, size, words, k))


def test_order_breaks_position_ties_by_key(eng):
    from kmer_denovo_filter_amd import keys
    for k in (31, 47):
        cols, size = column_sets(k)[0]
        words = distinct_words(k, 100_003, seed=9)
        pos = host_positions(cols, size, words, k)
        words = np.ascontiguousarray(words[:, pos < 3])
        pos = host_positions(cols, size, words, k)
        n = words.shape[1]
        assert 100 < n and len(np.unique(pos)) <= 3 and np.bincount(pos.astype(np.int64)).max() > 30      # many keys per position
        for mem in (HOST, DEVICE):
            rc, perm = order_raw(eng, mem, words, k, cols, size)
            assert rc == 0 and np.array_equal(perm, keys.order(words, pos).astype(np.uint32))


@pytest.mark.parametrize("mem", MEMS)
def test_jf_refusals(eng, mem):
    from kmer_denovo_filter_amd import jf_io
    words = distinct_words(31, 10)
    cols = jf_io.jf_make_matrix(62, 10)
    for k, size in ((0, 1024), (64, 1024), (65, 1024), (31, 1000), (31, 0)):
        c = (list(cols) * 3)[:max(2 * k, 1)]
        assert positions_raw(eng, mem, words, k, c, size)[0] == KDF_ERR_INVALID, (k, size)
        assert order_raw(eng, mem, words, k, c, size)[0] == KDF_ERR_INVALID, (k, size)
    assert eng._lib.kdf_jf_positions(eng._h, mem, None, None, 5, 31, None, 1024, None) == KDF_ERR_INVALID
    assert eng._lib.kdf_jf_order(eng._h, 7, None, None, 0, 31, None, 1024, None) == KDF_ERR_INVALID


# ---- files ----------------------------------------------------------------------------------------------------------

def to_device(words, counts):
    import torch
    from kmer_denovo_filter_amd import devkeys
    lo, hi = pair(words)
    dlo, dhi = devkeys.from_host(lo, hi, words.shape[0] == 2)
    return dlo, dhi, torch.from_numpy(np.ascontiguousarray(counts).view(np.int32)).cuda()


def sorted_words(k, n, seed=0):
    from kmer_denovo_filter_amd import keys
    w = distinct_words(k, n, seed)
    return np.ascontiguousarray(w[:, keys.order(w)])


def test_fixture_rewritten_on_the_device_is_the_fixture(eng, tmp_path):
    """the 45 275 records of the real Jellyfish file, shuffled and written under its own header: the host writer's file byte for
    byte, and the fixture's records byte for byte (the host writer spaces the JSON text differently, the fields are equal)"""
    from kmer_denovo_filter_amd import jf_io
    k, lo, hi, cnt = jf_io.read_index(FIXTURE)
    assert (k, len(lo)) == (31, 45275)
    header, off = jf_io.read_header(FIXTURE)
    perm = np.random.default_rng(3).permutation(len(lo))
    words = lo[perm][None, :]
    host, dev = str(tmp_path / "host.jf"), str(tmp_path / "dev.jf")
    jf_io.write_jellyfish_index(host, 31, lo[perm], None, cnt[perm], header=header)
    jf_io.write_jellyfish_index_device(dev, 31, *to_device(words, cnt[perm]), header=header)
    assert jf_io.LAST_INDEX_CODEC == "device" and not os.path.exists(dev + ".tmp")
    raw = open(dev, "rb").read()
    assert raw == open(host, "rb").read()
    h2, off2 = jf_io.read_header(dev)
    assert h2 == header and raw[off2:] == open(FIXTURE, "rb").read()[off:]


@pytest.mark.parametrize("k", [15, 31, 47, 63])
def test_jellyfish_writer_equals_the_host_writer(tmp_path, k):
    from kmer_denovo_filter_amd import jf_io
    for n in (0, 1, 5000):
        words = distinct_words(k, n, seed=11)
        counts = make_counts(words.shape[1])
        host, dev = str(tmp_path / "host.jf"), str(tmp_path / "dev.jf")
        jf_io.write_jellyfish_index(host, k, *pair(words), counts, cmdline=["t"])
        jf_io.write_jellyfish_index_device(dev, k, *to_device(words, counts), cmdline=["t"])
        assert open(dev, "rb").read() == open(host, "rb").read(), (k, n)
    with pytest.raises(ValueError):
        jf_io.write_jellyfish_index_device(str(tmp_path / "x.jf"), 65, None, None, None)


@pytest.mark.parametrize("k", [31, 47, 63, 101])
def test_write_index_device_equals_write_index(tmp_path, monkeypatch, k):
    from kmer_denovo_filter_amd import jf_io
    monkeypatch.setenv("KDF_INDEX_CHUNK_MB", "1")          # the body of the largest case takes several windows
    for n in (0, 1, 100_003):
        words = sorted_words(k, n, seed=12)
        counts = make_counts(words.shape[1])
        assert n < 100_003 or words.shape[1] * ((2 * k + 7) // 8 + 4) > 1 << 20
        host, dev = str(tmp_path / "host.jf"), str(tmp_path / "dev.jf")
        jf_io.write_index(host, k, *pair(words), counts, cmdline=["a", "b"])
        jf_io.write_index_device(dev, k, *to_device(words, counts), cmdline=["a", "b"])
        assert jf_io.LAST_INDEX_CODEC == "device" and not os.path.exists(dev + ".tmp")
        assert open(dev, "rb").read() == open(host, "rb").read(), (k, n)
        rk, dlo, dhi, dcnt = jf_io.read_index_device(dev)
        assert rk == k and np.array_equal(dcnt.cpu().numpy().view(np.uint32), counts)
        glo = dlo.cpu().numpy().view(np.uint64)
        lo, hi = pair(words)
        assert np.array_equal(glo, lo) and (dhi is None if hi is None else np.array_equal(dhi.cpu().numpy().view(np.uint64), hi))


def table_of(engine):
    """sorted (key rows, counts) of everything the engine's table holds"""
    from kmer_denovo_filter_amd import keys
    lo, hi, cnt = engine.export_ge(0)
    words = np.asarray(keys.from_pair(lo, hi, engine.k))
    o = keys.order(words)
    return np.ascontiguousarray(words[:, o]), cnt[o]


def load_both(path, k, monkeypatch, part=0, parts=1):
    from kmer_denovo_filter_amd import KmerEngine, jf_io
    out = []
    for device in (False, True):
        with KmerEngine(k, capacity_hint=1 << 12) as e:
            if device:
                n = jf_io.load_index_into_device(e, path, expect_k=k, part=part, parts=parts)
            else:
                monkeypatch.delenv("KDF_DEVICE_INDEX", raising=False)
                n = jf_io.load_index_into(e, path, expect_k=k, part=part, parts=parts)
            assert jf_io.LAST_INDEX_CODEC == ("device" if device else "host")
            out.append((n, *table_of(e)))
    (n0, w0, c0), (n1, w1, c1) = out
    assert n0 == n1 and np.array_equal(w0, w1) and np.array_equal(c0, c1)
    return n1, w1, c1


def write_raw_index(path, k, words, counts64, cb, fmt="kdf/sorted"):
    """an index file written by hand: any counter_len"""
    from kmer_denovo_filter_amd import jf_io, keys
    n = words.shape[1]
    hd = {"alignment": 8, "canonical": True, "cmdline": [], "counter_len": cb, "format": fmt, "key_len": 2 * k, "size": n}
    data = np.zeros(n, np.dtype([("k", "u1", ((2 * k + 7) // 8,)), ("c", "u1", (cb,))]))
    data["k"] = keys.to_bytes(words, k)
    data["c"] = np.asarray(counts64, "<u8").view(np.uint8).reshape(n, 8)[:, :cb] if cb <= 8 else np.pad(np.asarray(counts64, "<u8").view(np.uint8).reshape(n, 8), ((0, 0), (0, cb - 8)))
    with open(path, "wb") as f:
        f.write(jf_io._header_bytes(hd))
        data.tofile(f)
    return data


@pytest.mark.parametrize("k", [31, 47, 101])
def test_load_index_into_device_equals_the_host_loader(tmp_path, monkeypatch, k):
    from kmer_denovo_filter_amd import jf_io
    monkeypatch.setenv("KDF_INDEX_CHUNK_MB", "1")
    words = sorted_words(k, 100_003, seed=13)
    n = words.shape[1]
    counts = make_counts(n)
    path = str(tmp_path / "idx.jf")
    jf_io.write_index(path, k, *pair(words), counts)
    got_n, w, c = load_both(path, k, monkeypatch)
    assert got_n == n and np.array_equal(w, words) and np.array_equal(c, counts)
    shares = [load_both(path, k, monkeypatch, part=p, parts=3) for p in range(3)]
    assert all(s[0] == n for s in shares) and sum(s[1].shape[1] for s in shares) == n
    allw, allc = np.concatenate([s[1] for s in shares], axis=1), np.concatenate([s[2] for s in shares])
    assert np.array_equal(allw, words) and np.array_equal(allc, counts)          # (the shares are consecutive runs of a sorted file)
    # the switch sends load_index_into to the device loader
    from kmer_denovo_filter_amd import KmerEngine
    monkeypatch.setenv("KDF_DEVICE_INDEX", "1")
    jf_io.LAST_INDEX_CODEC = None
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        assert jf_io.load_index_into(e, path) == n and jf_io.LAST_INDEX_CODEC == "device"
        w2, c2 = table_of(e)
    assert np.array_equal(w2, words) and np.array_equal(c2, counts)


def test_load_other_counter_lengths_formats_and_an_empty_index(tmp_path, monkeypatch):
    from kmer_denovo_filter_amd import KmerEngine, jf_io
    from kmer_denovo_filter_amd.engine import IndexRecordError
    k = 31
    words = sorted_words(k, 3001, seed=14)
    n = words.shape[1]
    rng = np.random.default_rng(8)
    for cb, c64 in ((8, rng.integers(0, 1 << 34, n, dtype=np.uint64)), (2, rng.integers(0, 1 << 16, n, dtype=np.uint64)),
                    (12, rng.integers(0, 1 << 33, n, dtype=np.uint64))):
        path = str(tmp_path / f"cb{cb}.jf")
        write_raw_index(path, k, words, c64, cb)
        got_n, w, c = load_both(path, k, monkeypatch)
        assert got_n == n and np.array_equal(w, words) and np.array_equal(c, np.minimum(c64, 0xFFFFFFFF).astype(np.uint32))
    got_n, w, c = load_both(FIXTURE, 31, monkeypatch)      # binary/sorted: the real Jellyfish file
    fk, flo, _, fcnt = jf_io.read_index(FIXTURE)
    o = np.argsort(flo)
    assert got_n == 45275 and np.array_equal(w[0], flo[o]) and np.array_equal(c, fcnt[o])
    empty = str(tmp_path / "empty.jf")
    jf_io.write_index(empty, k, np.zeros(0, np.uint64), None, np.zeros(0, np.uint32))
    assert load_both(empty, k, monkeypatch)[0] == 0
    rk, dlo, dhi, dcnt = jf_io.read_index_device(empty)
    assert (rk, len(dlo), dhi, len(dcnt)) == (31, 0, None, 0)
    # a record whose key has a bit at 2k: the device loader names it, the host loader does not look
    bad = str(tmp_path / "bad.jf")
    data = write_raw_index(bad, k, words, np.ones(n, np.uint64), 4)
    data["k"][2222, 7] |= 0x40
    _, off = jf_io.read_header(bad)
    with open(bad, "r+b") as f:
        f.seek(off)
        data.tofile(f)
    monkeypatch.setenv("KDF_INDEX_CHUNK_MB", "1")
    with KmerEngine(k, capacity_hint=1 << 12) as e:
        with pytest.raises(IndexRecordError, match="record 2222") as ei:
            jf_io.load_index_into_device(e, bad)
        assert ei.value.record == 2222 and "bad.jf" in str(ei.value)
        with pytest.raises(IndexRecordError, match="record 2222"):           # (a share that starts behind record 0)
            jf_io.load_index_into_device(e, bad, part=1, parts=2)
        assert jf_io.load_index_into_device(e, bad, part=0, parts=2) == n
    with KmerEngine(33, capacity_hint=1 << 10) as e:
        with pytest.raises(ValueError):
            jf_io.load_index_into_device(e, bad)


def test_profile_stats(eng):
    eng.profile(True)
    p0 = eng.get_stat("indexcodec_passes")
    words, counts = make_words(31, 1001, "random"), make_counts(1001)
    body = eng.index_encode(*pair(words), counts, 31)
    eng.index_decode(body, 31)
    assert eng.get_stat("indexcodec_passes") == p0 + 2 and eng.get_stat("indexcodec_us") > 0
    eng.profile(False)
