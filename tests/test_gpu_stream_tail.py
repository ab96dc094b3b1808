"""Every entry point that takes a read stream, against streams whose words at and past ``n_bases`` are DIRTY.

The contract (include/kdf.h, "Read streams"): a position >= n_bases is invalid whatever the caller's buffers hold there
-- the bits of the last mask word past n_bases % 64, the 2 padding mask words and 4 padding packed words of
``kdf_stream_words``, the bases of the last packed words -- and the buffers need be no longer than ``kdf_stream_words``
says.  So the same stream with the same n_bases must give the same table, filter counts and hit bits on every path,
whether the producer padded it cleanly, with ``torch.zeros``, or handed over a prefix of a longer stream.

Fillings of everything at or past n_bases (the device tensors always have exactly ``kdf_stream_words(n_bases)`` words):

  clean    mask ones, packed zeros (what synth.py and the host forms produce): the control
  zeros    mask 0, packed 0: the phantom windows are poly-A runs
  live     mask 0, random bases: every phantom window is a fresh key
  prefix   the words of a longer stream of more reads, as they lie (the ``midread`` stream is cut inside a read)

Stream ends: n_bases % 64 in {0, 1, 31, 32, 33, 63} with the last read ending at n_bases - 1 (no separator inside
n_bases), a read that ends k - 1 positions before a tile edge, n_bases < k, n_bases == k, a cut in the middle of a read,
and two streams of a few thousand tiles whose last tile is alone in its slab of 128 / 256 tiles (``big_own``) or shares
it (``big_shared``): the slab-sort and sieve kernels walk slabs with persistent workgroups.

Truth: ``stream_truth.count_truth`` over the CPU words (k <= 63), ``kmer_truth.count_truth`` over the read strings cut
at n_bases (long k).  Before the GPU is touched every case asserts that the truth of the dirty words equals the truth
of the clean words, so no expectation depends on the filling.  Filters and scan indexes hold the PHANTOM keys -- the
poly-A k-mer and every window that could be formed from the dirty words at or past n_bases - k + 1 -- so a kernel that
trusts those words produces a count or a hit bit, not a miss that looks right.

Every case asserts a witness stat for the path its row names; a row collects the failures of all its streams and
fillings and reports them together.  The file prints its wall time when it is done."""
import time

import numpy as np
import pytest
import torch

import kmer_truth as KT
import stream_truth as ST
from test_stream_truth import pack

pytestmark = pytest.mark.gpu

FILLINGS = ("clean", "zeros", "live", "prefix")
REMS = (0, 1, 31, 32, 33, 63)
BIG_OWN_TILES, BIG_SHARED_TILES = 256 * 12 + 1, 256 * 10 + 70
_LUT = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _LUT[ord(_c)] = _i
    _LUT[ord(_c.lower())] = _i


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\n[stream tail] wall time of tests/test_gpu_stream_tail.py: {time.perf_counter() - t0:.1f} s", flush=True)


# ---------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------

def layout(reads):
    """(codes uint8, invalid bool) of the stream of ``reads``: one invalid separator position after every read"""
    parts = []
    for r in reads:
        parts.append(_LUT[np.frombuffer(r.encode(), np.uint8)])
        parts.append(np.array([4], np.uint8))
    c = np.concatenate(parts)
    return np.where(c == 4, 0, c).astype(np.uint8), c == 4


def words(codes, inv, n, filling, seed):
    """(packed, mask) uint64 arrays of exactly kdf_stream_words(n) words: positions < n from (codes, inv), the rest by
    ``filling``"""
    T = (n + 63) // 64
    pw, mw = 2 * T + 4, T + 2
    P = pw * 32
    assert P == mw * 64
    c = np.zeros(P, np.uint64)
    m = np.ones(P, bool)
    c[:n] = codes[:n]
    m[:n] = inv[:n]
    if filling == "zeros":
        m[n:] = False
    elif filling == "live":
        m[n:] = False
        c[n:] = np.random.default_rng(seed).integers(0, 4, P - n)
    elif filling == "prefix":
        ext = min(P, len(codes))
        c[n:ext] = codes[n:ext]
        m[n:ext] = inv[n:ext]
    else:
        assert filling == "clean"
    packed = np.bitwise_or.reduce(c.reshape(pw, 32) << (2 * np.arange(32, dtype=np.uint64)), axis=1)
    mask = np.packbits(m, bitorder="little").view(np.uint64)
    return packed, mask


def cpu(w):
    return torch.from_numpy(w.view(np.int64).copy())


def cut_reads(reads, n):
    """the read strings of the stream's first n positions (the read that n cuts ends there)"""
    out, off = [], 0
    for r in reads:
        if off >= n:
            break
        out.append(r[:n - off])
        off += len(r) + 1
    return out


class Stream:
    def __init__(self, name, reads, n, seed):
        self.name, self.n, self.seed = name, n, seed
        rng = np.random.default_rng(seed)
        self.reads = reads + [_rd(rng, 100, clean=True) for _ in range(3)]    # what a longer stream goes on with
        self.codes, self.inv = layout(self.reads)
        assert n < len(self.codes) - 200
        self.cut = cut_reads(self.reads, n)
        self._w = {}

    def words(self, filling):
        if filling not in self._w:
            self._w[filling] = words(self.codes, self.inv, self.n, filling, self.seed + 1)
        return self._w[filling]

    def offsets(self):
        return np.cumsum([0] + [len(r) + 1 for r in self.cut])


def _rd(rng, L, clean=False):
    r = rng.choice(list("ACGT"), L)
    if not clean and L:
        r[rng.random(L) < 0.01] = "N"
    return "".join(r)


def _ending(rng, k, want_mod):
    """a few reads, then a last read without N that ends at n - 1 with n % 64 == want_mod"""
    reads = [_rd(rng, int(rng.integers(20, 150))) for _ in range(5)]
    base = sum(len(r) + 1 for r in reads)
    L = k + 5 + ((want_mod - base - k - 5) % 64)
    reads.append(_rd(rng, L, clean=True))
    assert (base + L) % 64 == want_mod % 64
    return reads, base + L


def _big(rng, k, tiles):
    genome = _rd(rng, 60000, clean=True)
    n = 64 * (tiles - 1) + 17
    reads, base = [], 0
    while n - base > 400:
        s = int(rng.integers(0, len(genome) - 150))
        r = list(genome[s:s + 150])
        if rng.random() < 0.3:
            r[int(rng.integers(0, 150))] = "N"
        reads.append("".join(r))
        base += 151
    reads.append(_rd(rng, n - base, clean=True))
    return reads, n


_STREAMS = {}


def streams(k):
    """the stream ends of the module docstring for one k (built once)"""
    if k in _STREAMS:
        return _STREAMS[k]
    rng = np.random.default_rng(1000 + k)
    out = []
    for rem in REMS:
        reads, n = _ending(rng, k, rem)
        out.append(Stream(f"rem{rem}", reads, n, 100 * k + rem))
    reads, n = _ending(rng, k, -(k - 1))                        # the last read ends k - 1 positions before a tile edge
    assert (n + k - 1) % 64 == 0
    out.append(Stream("edge", reads, n, 100 * k + 64))
    out.append(Stream("below_k", [_rd(rng, k + 30, clean=True)], k - 1, 100 * k + 65))
    out.append(Stream("exactly_k", [_rd(rng, k + 30, clean=True)], k, 100 * k + 66))
    reads, n = _ending(rng, k, 5)
    out.append(Stream("midread", reads[:-1] + [reads[-1] + _rd(rng, k + 70, clean=True)], n, 100 * k + 67))
    for name, tiles in (("big_own", BIG_OWN_TILES), ("big_shared", BIG_SHARED_TILES)):
        reads, n = _big(rng, k, tiles)
        assert (n + 63) // 64 == tiles
        out.append(Stream(name, reads, n, 100 * k + tiles % 97))
    assert out[-2].n // 64 % 256 == 0 and 0 < out[-1].n // 64 % 128 < 127
    _STREAMS[k] = out
    return out


def second_batch(k):
    """the batch that follows in the two-batch rows: it STARTS with valid bases, so a first batch whose tail leaked into
    it would form windows across the two"""
    rng = np.random.default_rng(77)
    reads = [_rd(rng, 260, clean=True), _rd(rng, 90)]
    return Stream("second", reads, 261 + 90, 9000 + k)


# ---------------------------------------------------------------------------------------------------------------------
# truth (CPU) and its precondition: the same for every filling
# ---------------------------------------------------------------------------------------------------------------------

_TRUTH = {}


def truth(k, s):
    """k <= 63: (lo, hi, counts, windows) CPU tensors; long k: ({key: count}, windows).  Asserts, for every filling,
    that the dirty words have the truth of the clean ones and decode to the same positions below n_bases."""
    key = (k, s.name, s.seed)
    if key in _TRUTH:
        return _TRUTH[key]
    P, M = s.words("clean")
    clean = (cpu(P), cpu(M), s.n)
    ref = ST.decode(clean, 0, s.n)
    if k <= 63:
        t = ST.count_truth(clean, k)
    else:
        d = KT.count_truth(s.cut, k)
        t = (d, sum(d.values()))
    for f in FILLINGS[1:]:
        P2, M2 = s.words(f)
        dirty = (cpu(P2), cpu(M2), s.n)
        got = ST.decode(dirty, 0, s.n)
        assert torch.equal(got[0][~got[1]], ref[0][~ref[1]]) and torch.equal(got[1], ref[1]), f"{s.name}/{f}: the words differ below n_bases"
        if k <= 63:
            t2 = ST.count_truth(dirty, k)
            assert all(torch.equal(a, b) for a, b in zip(t[:3], t2[:3])) and t[3] == t2[3], f"{s.name}/{f}: the truth depends on the filling"
    if s.name == "rem33":                                       # the helper against the suite's own packer, once per k
        p0, m0, n0 = pack(s.reads)
        w = words(s.codes, s.inv, n0, "clean", 0)
        assert torch.equal(cpu(w[0])[:p0.numel()], p0) and torch.equal(cpu(w[1])[:m0.numel()], m0)
    _TRUTH[key] = t
    return t


def tail_strings(P, M, n):
    """the strings a kernel that trusts every word could read from position max(n - k - 64, 0) .. on: the dirty words
    decoded to the end of the buffers, cut at invalid positions"""
    n_ext = M.size * 64
    a = max(n - 300, 0)
    codes, inv = ST.decode((cpu(P), cpu(M), n_ext), a, n_ext)
    s = "".join("N" if i else "ACGT"[c] for c, i in zip(codes.tolist(), inv.tolist()))
    return [x for x in s.split("N") if x]


def phantom_keys(k, s, filling):
    """{key} of every window of tail_strings, the poly-A k-mer included: a superset of the phantom windows"""
    P, M = s.words(filling)
    keys = set(KT.count_truth(tail_strings(P, M, s.n), k))
    keys.add(0)
    return keys


def lohi_t(keys):
    lo, hi = KT.lohi(sorted(keys))
    return cpu(lo), cpu(hi)


def distinct_keys(parts):
    """ascending distinct (lo, hi) of several (lo, hi) tensors"""
    ones = [(lo, hi, torch.ones_like(lo)) for lo, hi in parts]
    lo, hi, _ = ST.accumulate(ones)
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------------
# engine helpers
# ---------------------------------------------------------------------------------------------------------------------

def dev(s, filling):
    """the stream on the device: tensors of exactly kdf_stream_words(n_bases) words"""
    from kmer_denovo_filter_amd.reads import stream_words
    P, M = s.words(filling)
    assert (P.size, M.size) == stream_words(s.n)
    dp, dm = cpu(P).cuda(), cpu(M).cuda()
    torch.cuda.synchronize()
    return dp, dm


def new_engine(k, hint=1 << 16, **opts):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=hint)
    for name, v in opts.items():
        e.set_option(name, v)
    return e


def table(e):
    """(sorted dump as CPU tensors or {key: count}, distinct, windows) of a (flushed by stats) engine"""
    _, distinct, windows = e.stats()
    n = e.count_ge(0)
    cap = max(n, 1)
    cnt = torch.zeros(cap, dtype=torch.int32, device="cuda")
    if e.long:
        keys = torch.zeros((cap, e.key_words), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        got = e.export_ge_dev(0, keys.data_ptr(), None, cnt.data_ptr(), cap, sorted_=True)
        e.synchronize()
        assert got == n
        rows = keys.cpu().numpy().view(np.uint64)[:n]
        ks = [KT.int_of_row(r) for r in rows]
        assert ks == sorted(ks)
        return dict(zip(ks, (cnt.cpu().numpy().view(np.uint32)[:n]).tolist())), distinct, windows
    lo = torch.zeros(cap, dtype=torch.int64, device="cuda")
    hi = torch.zeros(cap, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    got = e.export_ge_dev(0, lo.data_ptr(), hi.data_ptr() if e.wide else None, cnt.data_ptr(), cap, sorted_=True)
    e.synchronize()
    assert got == n
    return (lo[:n].cpu(), hi[:n].cpu(), (cnt[:n].to(torch.int64) & 0xFFFFFFFF).cpu()), distinct, windows


def table_diff(e, t):
    """None when the engine's table is the truth ``t``, or what differs"""
    got, distinct, windows = table(e)
    if e.long:
        d, w = t
        if got != d:
            extra = len(set(got) - set(d))
            return f"dump: {len(got)} keys ({extra} not in the truth), truth {len(d)}; windows {windows} / {w}"
        if (distinct, windows) != (len(d), w):
            return f"stats: distinct {distinct} / {len(d)}, windows {windows} / {w}"
        return None
    if got[0].numel() != t[0].numel() or not all(torch.equal(a, b) for a, b in zip(got, t[:3])):
        return f"dump: {got[0].numel()} keys summing {int(got[2].sum())}, truth {t[0].numel()} keys summing {int(t[2].sum())}; windows {windows} / {t[3]}"
    if (distinct, windows) != (t[0].numel(), t[3]):
        return f"stats: distinct {distinct} / {t[0].numel()}, windows {windows} / {t[3]}"
    return None


def count_dev(e, d, n):
    e.count_dev(d[0].data_ptr(), d[1].data_ptr(), n)


def report(bad):
    assert not bad, f"{len(bad)} failing (stream/filling): " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# kdf_count_reads_dev
# ---------------------------------------------------------------------------------------------------------------------

def _count_once(k, row, s, filling):
    """one dirty stream through the path ``row`` names -> what differs from the truth, or None.  The witness of the
    path is asserted: a case that did not reach its kernel is a failure of the test."""
    d = dev(s, filling)
    nt = (s.n + 63) // 64
    tag = f"{row} k={k} {s.name}/{filling}"
    if row == "pending":
        e = new_engine(k)
    elif row in ("direct", "long"):
        e = new_engine(k, force_path=1)
    elif row == "binned":
        e = new_engine(k, force_path=2)
    elif row == "auto":
        e = new_engine(k, l1_direct_positions=1)
    else:
        assert row == "passes"
        e = new_engine(k, l1_direct_positions=1, binned_max_positions=64 * max(nt - 1, 1))
    with e:
        if row in ("binned", "auto", "passes"):
            assert e.get_stat("log2cap") > e.get_stat("bucket_bits"), tag + ": a single bucket, nothing to partition"
        count_dev(e, d, s.n)
        if row == "pending":
            assert e.get_stat("pending_positions") > 0 and e.get_stat("pending_passes") == 0 and e.get_stat("binned_passes") == 0, tag
        elif row in ("direct", "long"):
            assert e.last_count_path() == "direct" and e.get_stat("binned_passes") == 0 and e.get_stat("pending_positions") == 0, tag
        elif row == "binned":
            assert e.last_count_path() == "binned" and e.get_stat("binned_passes") >= 1, tag
        else:
            # partitioned where it lies, at the call: the passes wait in the ring, nothing waits in the pending STREAM
            # (pending_positions counts both: one tile-rounded position per partitioned position)
            want_passes = 2 if row == "passes" and nt >= 2 else 1
            assert e.get_stat("binned_passes") == want_passes and e.get_stat("pending_passes") == want_passes, tag
            assert e.get_stat("pending_positions") == nt * 64, tag
            e.flush()
            assert e.get_stat("pending_positions") == 0 and e.get_stat("pending_passes") == 0, tag
        return table_diff(e, truth(k, s))


COUNT_ROWS = ([("pending", k) for k in (15, 31, 32, 33, 47, 63)] + [("direct", k) for k in (15, 31, 32, 33, 47, 63)]
              + [("binned", k) for k in (31, 63)] + [("auto", k) for k in (31, 63)] + [("passes", k) for k in (31, 47)]
              + [("long", k) for k in (65, 101, 201)])


@pytest.mark.parametrize("row,k", COUNT_ROWS, ids=[f"{r}-k{k}" for r, k in COUNT_ROWS])
def test_count_dev(row, k):
    bad = []
    for s in streams(k):
        truth(k, s)                                             # (the precondition, before the GPU is touched)
        for f in FILLINGS:
            why = _count_once(k, row, s, f)
            if why:
                bad.append(f"{s.name}/{f}: {why}")
    report(bad)


@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("defer", [1, 0])
@pytest.mark.parametrize("path", ["pending", "binned"])
def test_two_dirty_batches_into_one_table(k, defer, path):
    """Two dirty batches into one table: the first batch's tail must not leak into the second (the pending stream
    concatenates batches tile aligned; the second batch starts with valid bases)."""
    b = second_batch(k)
    tb = truth(k, b)
    bad = []
    for s in streams(k):
        ta = truth(k, s)
        both = ST.accumulate([ta, tb]) + (ta[3] + tb[3],)
        for f in FILLINGS:
            da, db = dev(s, f), dev(b, f)
            tag = f"two batches {path} defer={defer} k={k} {s.name}/{f}"
            with new_engine(k, defer=defer, **({"force_path": 2} if path == "binned" else {})) as e:
                count_dev(e, da, s.n)
                if not defer:
                    assert e.get_stat("pending_positions") == 0 and e.get_stat("defer") == 0, tag
                count_dev(e, db, b.n)
                if defer:
                    assert e.get_stat("pending_positions") >= s.n + b.n, tag
                    assert e.get_stat("pending_passes") == (2 if path == "binned" else 0), tag
                    e.flush()
                else:
                    assert e.last_count_path() == ("binned" if path == "binned" else "direct"), tag
                assert e.get_stat("pending_positions") == 0, tag
                why = table_diff(e, both)
            if why:
                bad.append(f"{s.name}/{f}: {why}")
    report(bad)


@pytest.mark.parametrize("path", ["direct", "binned"])
def test_key_parts_union_equals_truth(path):
    """key_parts 3: the union of the three slices' tables is the truth, their windows add up to the truth's"""
    k = 31
    bad = []
    for s in streams(k):
        t = truth(k, s)
        for f in FILLINGS:
            d = dev(s, f)
            parts, windows = [], 0
            for part in range(3):
                with new_engine(k, force_path=1 if path == "direct" else 2, key_parts=3, key_part=part) as e:
                    count_dev(e, d, s.n)
                    assert e.last_count_path() == path, f"key_parts {path} {s.name}/{f}"
                    got, _, w = table(e)
                parts.append(got)
                windows += w
            got = ST.accumulate(parts)
            if windows != t[3] or not all(a.numel() == b.numel() and torch.equal(a, b) for a, b in zip(got, t[:3])):
                bad.append(f"{s.name}/{f}: {got[0].numel()} keys / {windows} windows, truth {t[0].numel()} / {t[3]}")
    report(bad)


# ---------------------------------------------------------------------------------------------------------------------
# kdf_count_reads_filtered_dev
# ---------------------------------------------------------------------------------------------------------------------

_FILLER = {}


def filler_keys(k):
    """20 000 more filter keys (a random sequence's own), for the rows that need a filter or a table of some size"""
    if k not in _FILLER:
        rng = np.random.default_rng(5 + k)
        codes, inv = layout([_rd(rng, 20000 + k, clean=True)])
        P, M = words(codes, inv, len(codes), "clean", 0)
        t = ST.count_truth((cpu(P), cpu(M), len(codes)), k)
        _FILLER[k] = (t[0], t[1])
    return _FILLER[k]


def filter_for(k, s, filling, row):
    """(filter keys, expected count of each) -- the stream's own keys (at most 40 000 of them), the phantom keys of this
    filling and, where the row needs size, the filler"""
    t = truth(k, s)
    ph = phantom_keys(k, s, filling)
    if k > 63:
        keys = sorted(set(t[0]) | ph)
        return keys, np.array([t[0].get(v, 0) for v in keys], np.uint32)
    parts = [(t[0][:40000], t[1][:40000]), lohi_t(ph)]
    if row in ("sieve_l2", "binned_if"):
        parts.append(filler_keys(k))
    flo, fhi = distinct_keys(parts)
    return (flo, fhi), ST.filtered_truth(t, (flo, fhi)).numpy().astype(np.uint32)


def _filtered_once(k, row, defer, s, filling):
    d = dev(s, filling)
    keys, want = filter_for(k, s, filling, row)
    tag = f"{row} defer={defer} k={k} {s.name}/{filling}"
    opts = {"sieve_lds": {}, "sieve_l2": {"sieve_bits": 32}, "binned_if": {"force_path": 2}, "direct_if": {"force_path": 1}}[row]
    with new_engine(k, defer=defer, **opts) as e:
        if e.long:
            rows = KT.rows(keys, e.key_words)
            e.load_filter(rows)
            nkeys = len(keys)
        else:
            lo, hi = keys[0].numpy().view(np.uint64), keys[1].numpy().view(np.uint64)
            e.load_filter(lo, hi if e.wide else None)
            nkeys = len(lo)
        # the sieve's geometry, by the method of tests/test_gpu_scan_paths.py: default sizing keeps it in LDS up to
        # 65 536 keys; 32 bits per key leave LDS above 16 384 keys
        if row == "sieve_lds":
            assert nkeys <= 65536, tag
        elif row == "sieve_l2":
            assert nkeys > 16384, tag
        elif row == "binned_if":
            assert e.get_stat("log2cap") > e.get_stat("bucket_bits"), tag
        e.count_filtered_dev(d[0].data_ptr(), d[1].data_ptr(), s.n)
        if row.startswith("sieve"):
            assert e.last_count_path() == "sieve", tag
        elif row == "direct_if":
            assert e.last_count_path() == "direct" and e.get_stat("binned_passes") == 0, tag
        else:
            assert e.last_count_path() == "binned" and e.get_stat("binned_passes") == 1, tag
            assert e.get_stat("pending_passes") == (1 if defer else 0), tag
        got = e.query(rows) if e.long else e.query(lo, hi if e.wide else None)
        assert e.get_stat("pending_passes") == 0
    if not np.array_equal(got, want):
        wrong = np.flatnonzero(got != want)
        return f"{len(wrong)} of {len(want)} filter keys differ (sum {int(got.sum())}, truth {int(want.sum())})"
    return None


FILTER_ROWS = ([("sieve_lds", k, 1) for k in (21, 31, 47)] + [("sieve_l2", 31, 1)] + [("binned_if", k, d) for k in (31, 55) for d in (1, 0)]
               + [("direct_if", k, 1) for k in (31, 63, 101)])


@pytest.mark.parametrize("row,k,defer", FILTER_ROWS, ids=[f"{r}-k{k}-defer{d}" for r, k, d in FILTER_ROWS])
def test_count_filtered_dev(row, k, defer):
    bad = []
    for s in streams(k):
        truth(k, s)
        for f in FILLINGS:
            why = _filtered_once(k, row, defer, s, f)
            if why:
                bad.append(f"{s.name}/{f}: {why}")
    report(bad)


# ---------------------------------------------------------------------------------------------------------------------
# kdf_scan_reads_dev
# ---------------------------------------------------------------------------------------------------------------------

_HITS = {}


def expected_hits(k, s):
    """the hit words of the stream against its OWN keys, every third of them (ascending order) stored with count 0: a
    window hits iff it lies wholly below n_bases, is valid and its key has a count > 0.  (The phantom keys join the
    index with count 1 only where the stream does not hold them, so they change no expected bit.)"""
    key = (k, s.name, s.seed)
    if key in _HITS:
        return _HITS[key]
    t = truth(k, s)
    nt = (s.n + 63) // 64
    if k > 63:
        index = {v: (0 if i % 3 == 0 else 1) for i, v in enumerate(sorted(t[0]))}
        hits, _ = KT.scan_truth(s.cut, k, index)
        want = KT.hit_words(s.offsets(), hits, nt)
    else:
        bits = np.zeros(nt * 64, bool)
        if s.n >= k:
            P, M = s.words("clean")
            wlo, whi, ok = ST.windows(*ST.decode((cpu(P), cpu(M), s.n), 0, s.n), k)
            pos = torch.ones_like(t[0], dtype=torch.bool)
            pos[::3] = False
            bits[:s.n - k + 1] = (ok & ST.member(t[0][pos], t[1][pos], wlo, whi)).numpy()
        want = np.packbits(bits, bitorder="little").view(np.uint64)
    _HITS[key] = want
    return want


def scan_index(k, s, filling):
    """(keys, counts, expected hit words): the index holds the stream's keys -- every third with count 0 -- and the
    phantom keys of this filling with count 1"""
    t = truth(k, s)
    ph = phantom_keys(k, s, filling)
    want = expected_hits(k, s)
    if k > 63:
        index = {v: (0 if i % 3 == 0 else 1) for i, v in enumerate(sorted(t[0]))}
        for v in ph:
            index.setdefault(v, 1)
        keys = sorted(index)
        return keys, np.array([index[v] for v in keys], np.uint32), want
    own_cnt = torch.ones_like(t[0])
    own_cnt[::3] = 0
    plo, phi = lohi_t(ph)
    new = ~ST.member(t[0], t[1], plo, phi)
    lo, hi, cnt = ST.sort_keys(torch.cat([t[0], plo[new]]), torch.cat([t[1], phi[new]]), torch.cat([own_cnt, torch.ones_like(plo[new])]))
    return (lo, hi), cnt.numpy().astype(np.uint32), want


SCAN_ROWS = [("sieve", 31), ("sieve", 63), ("direct", 31), ("direct", 63), ("long", 101)]


@pytest.mark.parametrize("row,k", SCAN_ROWS, ids=[f"{r}-k{k}" for r, k in SCAN_ROWS])
def test_scan_dev(row, k):
    """hit words 0 .. ceil(n_bases / 64) - 1, bit for bit: no bit at a position > n_bases - k"""
    bad = []
    for s in streams(k):
        truth(k, s)
        nt = (s.n + 63) // 64
        for f in FILLINGS:
            keys, counts, want = scan_index(k, s, f)
            d = dev(s, f)
            tag = f"scan {row} k={k} {s.name}/{f}"
            with new_engine(k, **({} if row == "sieve" else {"force_path": 1})) as e:
                if e.long:
                    e.add_pairs(KT.rows(keys, e.key_words), None, counts)
                else:
                    e.add_pairs(keys[0].numpy().view(np.uint64), keys[1].numpy().view(np.uint64) if e.wide else None, counts)
                dh = torch.full((d[1].numel(),), -1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                e.scan_dev(d[0].data_ptr(), d[1].data_ptr(), s.n, dh.data_ptr())
                e.synchronize()
                assert e.get_stat("last_scan_path") == (3 if row == "sieve" else 0), tag
            got = dh.cpu().numpy().view(np.uint64)[:nt]
            if not np.array_equal(got, want):
                extra = int(np.unpackbits((got & ~want).view(np.uint8)).sum())
                bad.append(f"{s.name}/{f}: {int((got != want).sum())} hit words differ ({extra} bits the truth does not have)")
    report(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the host forms (control): caller arrays of ceil(n / 32) and ceil(n / 64) words, dirty past n_bases
# ---------------------------------------------------------------------------------------------------------------------

def host_stream(s, filling):
    from kmer_denovo_filter_amd import ReadStream
    P, M = s.words(filling)
    return ReadStream(P[:(s.n + 31) // 32].copy(), M[:(s.n + 63) // 64].copy(), s.n, s.offsets().astype(np.int64))


@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("form", ["count", "upload", "scan"])
def test_host_forms(k, form):
    bad = []
    for s in streams(k):
        t = truth(k, s)
        for f in FILLINGS:
            st = host_stream(s, f)
            with new_engine(k) as e:
                if form == "count":
                    e.count(st)
                    assert e.get_stat("pending_positions") > 0
                    why = table_diff(e, t)
                elif form == "upload":
                    e.upload_async(0, st)
                    e.count_uploaded(0)
                    assert e.get_stat("pending_positions") > 0
                    why = table_diff(e, t)
                else:
                    keys, counts, want = scan_index(k, s, f)
                    e.add_pairs(keys[0].numpy().view(np.uint64), keys[1].numpy().view(np.uint64) if e.wide else None, counts)
                    hits, _ = e.scan(st, want_distinct=False)
                    assert e.get_stat("last_scan_path") == 3
                    nt = (s.n + 63) // 64
                    why = None if np.array_equal(hits[:nt], want) and not hits[nt:].any() else f"{int((hits[:nt] != want).sum())} hit words differ"
            if why:
                bad.append(f"{s.name}/{f}: {why}")
    report(bad)
