"""The table join (include/kdf.h "Table join"; csrc/kdf_join.h) against tests/join_truth.py.

Shapes: a 20 kbp random genome; table A is counted from 2 000 reads of k + 69 bases (100 bp at k = 31) drawn with
repeats over the whole genome, a tenth of them with one substitution (counts spread over 1..20, the error k-mers sit
at 1); table B from 1 000 reads over the overlapping half [5 000, 15 000) with its own error reads.  The model is fed
from ``export_ge(0)`` of both engines and is computed on the host; every comparison is exact."""
import functools
from ctypes import byref, c_uint64, c_void_p

import numpy as np
import pytest

import join_truth as J
import long_truth as T
import merge_truth as MT

pytestmark = pytest.mark.gpu

MAX = None                                                # an upper bound that bounds nothing
KS = (15, 31, 33, 47, 63, 65, 101, 201)
BOUNDS = ((1, MAX, 0, 0), (3, MAX, 0, 0), (3, 10, 1, MAX), (2, 2, 5, 7), (0, MAX, 0, MAX))
SENT = -7
GUARD = 64


# ---------------------------------------------------------------------------------------------------------------------
# streams and tables
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reads(which, k, n_reads=None):
    """which: "a" the whole genome, "b" its middle half; -> tuple of read strings"""
    g = np.random.default_rng(5).integers(0, 4, 20_000)
    rng = np.random.default_rng({"a": 11, "b": 23}[which])
    lo, hi = (0, 20_000) if which == "a" else (5_000, 15_000)
    n = n_reads or (2_000 if which == "a" else 1_000)
    L = k + 69
    starts = rng.integers(lo, hi - L, n)
    out = []
    for i, s in enumerate(starts.tolist()):
        r = g[s:s + L].copy()
        if i % 10 == 0:                                               # an error read: one substitution
            p = int(rng.integers(0, L))
            r[p] = (r[p] + 1 + int(rng.integers(0, 3))) & 3
        if i & 1:                                                     # the other strand
            r = (3 - r)[::-1]
        out.append("".join("ACGT"[b] for b in r))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _stream(which, k, n_reads=None):
    from kmer_denovo_filter_amd import ReadStream
    return ReadStream.from_strings(_reads(which, k, n_reads))


def _counted(k, which, hint=1 << 15, n_reads=None, **options):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=hint)
    for name, v in options.items():
        e.set_option(name, v)
    e.count(_stream(which, k, n_reads))
    return e


def _from_pairs(k, keys, cnt, hint=1, **options):
    """an engine holding the listed entries (keys: join_truth keys)"""
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=hint)
    for name, v in options.items():
        e.set_option(name, v)
    lo, hi = _arrays(k, keys)
    e.add_pairs(lo, hi, np.asarray(cnt, np.uint32))
    return e


def _arrays(k, keys):
    """join_truth keys -> what the engine's host forms take"""
    if k > 63:
        return np.array(keys, np.uint64).reshape(len(keys), T.W_of(k)), None
    if k > 32:
        return np.array([x[0] for x in keys], np.uint64), np.array([x[1] for x in keys], np.uint64)
    return np.array(keys, np.uint64), None


def _table(e):
    """(keys, counts) of everything the engine stores, as the model takes them"""
    lo, hi, cnt = e.export_ge(0)
    return J.keys_of(lo, hi if (e.wide and not e.long) else None), cnt.tolist()


def _got(e, other, b):
    keys, cnt, oc = e.export_join(other, *b)
    k = J.keys_of(keys) if e.long else J.keys_of(keys[0], keys[1] if e.wide else None)
    return k, cnt.tolist(), oc.tolist()


def _want(ta, tb, b):
    return J.join(ta[0], ta[1], None if tb is None else tb[0], None if tb is None else tb[1], *b)


def _check(e, other, ta, tb, bounds, tag=""):
    for b in bounds:
        want = _want(ta, tb, b)
        assert _got(e, other, b) == want, f"{tag} bounds {b}"
        assert e.count_join(other, *b) == len(want[0]), f"{tag} bounds {b}: count_join"


def _raw(e, other, b, cap, sorted_=0, with_cnt=True, with_ocnt=True):
    """kdf_export_join[_w]_dev into sentinel-filled buffers with GUARD words behind `cap`
    -> (rc, n, keys (cap + GUARD[, W]), hi or None, cnt or None, ocnt or None) on the host"""
    import torch
    W = e.key_words if e.long else 1
    lo = torch.full(((cap + GUARD) * W,), SENT, dtype=torch.int64, device="cuda:0")
    hi = torch.full((cap + GUARD,), SENT, dtype=torch.int64, device="cuda:0") if (e.wide and not e.long) else None
    cnt = torch.full((cap + GUARD,), SENT, dtype=torch.int32, device="cuda:0") if with_cnt else None
    oc = torch.full((cap + GUARD,), SENT, dtype=torch.int32, device="cuda:0") if with_ocnt else None
    torch.cuda.synchronize()
    ub = lambda v: 0xFFFFFFFF if v is None else int(v)                # noqa: E731
    p = lambda t: c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    n = c_uint64(0)
    args = (e._h, other._h if other is not None else None, int(b[0]), ub(b[1]), int(b[2]), ub(b[3]))
    if e.long:
        rc = e._lib.kdf_export_join_w_dev(*args, p(lo), p(cnt), p(oc), int(cap), int(sorted_), byref(n))
    else:
        rc = e._lib.kdf_export_join_dev(*args, p(lo), p(hi), p(cnt), p(oc), int(cap), int(sorted_), byref(n))
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()          # noqa: E731
    keys = host(lo)
    return rc, int(n.value), keys.reshape(-1, W) if e.long else keys, host(hi), host(cnt), host(oc)


def _raw_entries(e, res, n):
    """the first n entries of a raw export as [(key, count, other count)]"""
    _, _, lo, hi, cnt, oc = res
    keys = J.keys_of(lo[:n].view(np.uint64)) if e.long else J.keys_of(lo[:n].view(np.uint64), None if hi is None else hi[:n].view(np.uint64))
    return list(zip(keys, cnt[:n].view(np.uint32).tolist(), oc[:n].view(np.uint32).tolist()))


# ---------------------------------------------------------------------------------------------------------------------
# truth: every width, every bound set
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_truth(k):
    from kmer_denovo_filter_amd import KmerEngine
    with _counted(k, "a") as a, _counted(k, "b") as b:
        ta, tb = _table(a), _table(b)
        assert max(ta[1]) >= 12 and min(ta[1]) == 1 and len(set(ta[0]) & set(tb[0])) > 1000
        assert len(_want(ta, tb, (2, 2, 5, 7))[0]) > 0 and len(_want(ta, tb, (3, 10, 1, MAX))[0]) > 100
        _check(a, b, ta, tb, BOUNDS[:4], f"k={k}")
        _check(a, None, ta, None, ((0, 2, 0, 0), (0, 2, 5, 7)), f"k={k} other=None")
        # A in filter mode: half of A's keys and half of B's as the filter, counted over A's stream -- B's own keys
        # are never seen and stay stored with count 0
        in_a = set(ta[0])
        fk = ta[0][::2] + [x for x in tb[0][::2] if x not in in_a]
        with KmerEngine(k, capacity_hint=len(fk)) as f:
            f.load_filter(*_arrays(k, fk))
            f.count_filtered(_stream("a", k))
            tf = _table(f)
            assert sorted(tf[0], key=J.key_order) == sorted(fk, key=J.key_order) and tf[1].count(0) > 100
            _check(f, b, tf, tb, (BOUNDS[4], (0, 0, 1, MAX), (0, 0, 0, 0)), f"k={k} filter mode")
            _check(f, None, tf, None, ((0, 2, 0, 0),), f"k={k} filter mode, other=None")
            # ... and as the table that is probed: a key stored there with count 0 reads as absent
            _check(a, f, ta, tf, ((1, MAX, 0, 0), (1, MAX, 1, MAX)), f"k={k} filter as other")


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------

GEO_BOUNDS = ((1, MAX, 0, 0), (3, 10, 1, MAX), (0, MAX, 0, MAX))


@pytest.fixture(scope="module")
def base31():
    """the two tables at k = 31 as the model takes them, computed once"""
    with _counted(31, "a") as a, _counted(31, "b") as b:
        ta, tb = _table(a), _table(b)
    return ta, tb


@pytest.mark.parametrize("k", (31, 63, 65))
def test_small_and_large_tables(k):
    """A of 2^10 slots (narrow keys: half of one workgroup's 2^11, two waves lie past the end; wide and long keys: one
    workgroup of 2^10), A of 2^16 (32 or 64 workgroups); a B of 2^10 against an A of 2^16 and the reverse."""
    with _counted(k, "a") as a16, _counted(k, "b") as b16:
        ta, tb = _table(a16), _table(b16)
        assert a16.stats()[0] >= 1 << 16 and b16.stats()[0] >= 1 << 15
        # 300 entries of each, 150 of them shared
        ca, cb = dict(zip(*ta)), dict(zip(*tb))
        shared = [x for x in ta[0] if x in cb][:150]
        ka = shared + [x for x in ta[0] if x not in cb][:150]
        kb = shared + [x for x in tb[0] if x not in ca][:150]
        with _from_pairs(k, ka, [ca[x] for x in ka]) as a10, _from_pairs(k, kb, [cb[x] for x in kb]) as b10:
            assert a10.stats()[0] == 1 << 10 and b10.stats()[0] == 1 << 10
            t10a, t10b = _table(a10), _table(b10)
            _check(a10, b16, t10a, tb, GEO_BOUNDS, f"k={k} A 2^10, B large")
            _check(a16, b10, ta, t10b, GEO_BOUNDS, f"k={k} A large, B 2^10")
            _check(a10, b10, t10a, t10b, GEO_BOUNDS, f"k={k} both 2^10")
            _check(a10, None, t10a, None, ((0, 2, 0, 0),), f"k={k} A 2^10, no B")


def test_b_after_growth_and_big_buckets(base31):
    ta, tb = base31
    with _counted(31, "a") as a:
        with _counted(31, "b", hint=1) as grown:                      # created with 2^10 slots, rehashed while counting
            assert grown.stats()[0] > 1 << 10
            assert _table(grown) == tb
            _check(a, grown, ta, tb, GEO_BOUNDS, "B after growth")
        with _counted(31, "b") as plain, _counted(31, "b", big_bucket_log2cap=10) as big:
            assert big.get_stat("bucket_bits") == plain.get_stat("bucket_bits") + 1
            assert _table(big) == tb
            _check(a, big, ta, tb, GEO_BOUNDS, "B with big buckets")
            _check(big, a, tb, ta, GEO_BOUNDS, "A with big buckets")


def test_owner_table_with_hash_shift(base31):
    """B is rank 1's owner table of four (hash_shift = 2): it holds the keys whose hash begins with the bits 01, and its
    home slot drops those bits"""
    ta, tb = base31
    h = MT.key_hash(np.array(tb[0], np.uint64))
    own = (h >> np.uint64(62)) == np.uint64(1)
    kb = [x for x, o in zip(tb[0], own.tolist()) if o]
    cb = [c for c, o in zip(tb[1], own.tolist()) if o]
    assert 1000 < len(kb) < len(tb[0])
    with _counted(31, "a") as a, _from_pairs(31, kb, cb, hint=len(kb), hash_shift=2) as owner:
        assert owner.get_stat("hash_shift") == 2
        tob = _table(owner)
        assert tob == (kb, cb)
        _check(a, owner, ta, tob, GEO_BOUNDS, "B an owner table")
        _check(owner, a, tob, ta, GEO_BOUNDS, "A an owner table")


@pytest.mark.parametrize("k", (31, 65))
def test_key_parts_union(k):
    with _counted(k, "a") as a, _counted(k, "b") as b:
        ta, tb = _table(a), _table(b)
    from kmer_denovo_filter_amd import KmerEngine
    with KmerEngine(k, capacity_hint=1 << 15) as s, _counted(k, "b") as b:
        s.set_option("key_parts", 3)
        for bounds in ((1, MAX, 0, 0), (3, 10, 1, MAX)):
            union, sizes = [], []
            for part in range(3):
                s.clear(); s.set_option("key_part", part)
                s.count(_stream("a", k))
                got = _got(s, b, bounds)
                assert s.count_join(b, *bounds) == len(got[0])
                sizes.append(len(got[0]))
                union += list(zip(*got))
            assert min(sizes) > 0
            union.sort(key=lambda e: J.key_order(e[0]))
            assert union == list(zip(*_want(ta, tb, bounds))), f"k={k} {bounds}"


# ---------------------------------------------------------------------------------------------------------------------
# keys that share a hash or a home slot
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (95, 201))                  # W = 3 and 7
def test_full_hash_collisions_long(k):
    rng = np.random.default_rng(k)
    W = T.W_of(k)
    groups = []
    for j in range(1, W - 1):                                         # one hash, one top word, middle word j differs
        groups.append(T.rows_with_hash(int(T._rand64(rng, 1)[0]), k, 9, rng, share=("middle", j)))
    groups.append(T.rows_with_hash(int(T._rand64(rng, 1)[0]), k, 9, rng, share="middles"))   # ... the top word differs
    pads = T.random_rows(rng, k, 200)
    for g in groups:
        assert len(set(T.long_hash(g).tolist())) == 1
    rows_a = np.concatenate(groups + [pads])
    missing = [g[int(rng.integers(0, len(g)))] for g in groups]       # one member of each group is not in B
    miss = {tuple(r) for r in np.array(missing).tolist()}
    ka = J.keys_of(rows_a)
    kb = [x for x in ka if x not in miss]
    ca = (1 + np.arange(len(ka)) % 7).tolist()
    cb = (1 + np.arange(len(kb)) % 5).tolist()
    with _from_pairs(k, ka, ca) as a, _from_pairs(k, kb, cb) as b:
        ta, tb = _table(a), _table(b)
        got = _got(a, b, (1, MAX, 0, 0))
        assert set(got[0]) == miss and len(got[0]) == len(miss)
        _check(a, b, ta, tb, ((1, MAX, 0, 0), (1, MAX, 1, MAX), (2, 4, 2, 3)), f"k={k}")
        _check(b, a, tb, ta, ((1, MAX, 0, 0), (1, MAX, 1, MAX)), f"k={k} reversed")


@pytest.mark.parametrize("k", (33, 47, 63))
def test_full_hash_collisions_wide(k):
    """The wide twin: two groups per k whose members share all 64 bits of the stored hash word and differ in hi only
    (k = 33: the four keys a hash has; else nine); B lacks one member of each, which A's probe of B must report absent
    although B holds its h."""
    rng = np.random.default_rng(k)
    n = 4 if k == 33 else 9
    groups = [MT.collision_group(int(T._rand64(rng, 1)[0]), n, k, rng) for _ in range(2)]
    for lo, hi in groups:
        assert len(set(MT.key_hash(lo, hi).tolist())) == 1 and len(set(hi.tolist())) == n
    plo, phi = MT.keys_with_hash(0, 0, 200, k, rng)
    lo = np.concatenate([g[0] for g in groups] + [plo])
    hi = np.concatenate([g[1] for g in groups] + [phi])
    ka = J.keys_of(lo, hi)
    assert len(set(ka)) == len(ka)
    miss = {ka[i * n + int(rng.integers(0, n))] for i in range(2)}     # one member of each group is not in B
    kb = [x for x in ka if x not in miss]
    ca = (1 + np.arange(len(ka)) % 7).tolist()
    cb = (1 + np.arange(len(kb)) % 5).tolist()
    with _from_pairs(k, ka, ca) as a, _from_pairs(k, kb, cb) as b:
        ta, tb = _table(a), _table(b)
        assert sorted(ta[0], key=J.key_order) == sorted(ka, key=J.key_order) and dict(zip(*ta)) == dict(zip(ka, ca))
        assert dict(zip(*tb)) == dict(zip(kb, cb))
        got = _got(a, b, (1, MAX, 0, 0))
        assert set(got[0]) == miss and len(got[0]) == len(miss)
        _check(a, b, ta, tb, ((1, MAX, 0, 0), (1, MAX, 1, MAX), (2, 4, 2, 3)), f"k={k}")
        _check(b, a, tb, ta, ((1, MAX, 0, 0), (1, MAX, 1, MAX)), f"k={k} reversed")


def test_shared_home_slot_wide():
    """k = 63: 40 keys whose hashes share the top 20 bits (one home slot in any table of up to 2^20 slots) and differ in
    hi; B lacks every fourth"""
    rng = np.random.default_rng(63)
    lo, hi = MT.keys_with_hash(int(rng.integers(0, 1 << 20)), 20, 40, 63, rng)
    plo, phi = MT.keys_with_hash(0, 0, 200, 63, rng)
    ka = J.keys_of(np.concatenate([lo, plo]), np.concatenate([hi, phi]))
    assert len(set(ka)) == len(ka) and len(set(hi.tolist())) == 40
    miss = set(ka[:40:4])
    kb = [x for x in ka if x not in miss]
    with _from_pairs(63, ka, (1 + np.arange(len(ka)) % 7).tolist()) as a, _from_pairs(63, kb, (1 + np.arange(len(kb)) % 5).tolist()) as b:
        ta, tb = _table(a), _table(b)
        got = _got(a, b, (1, MAX, 0, 0))
        assert set(got[0]) == miss and len(got[0]) == len(miss)
        _check(a, b, ta, tb, ((1, MAX, 0, 0), (1, MAX, 1, MAX), (2, 4, 2, 3)), "k=63")


# ---------------------------------------------------------------------------------------------------------------------
# state
# ---------------------------------------------------------------------------------------------------------------------

def _dev_stream(which, k):
    import torch
    st = _stream(which, k)
    return (torch.from_numpy(st.packed.view(np.int64)).cuda(), torch.from_numpy(st.invalid.view(np.int64)).cuda(), st.n_bases)


@pytest.mark.parametrize("k", (31, 63, 65))
def test_pending_state(k):
    """count_dev leaves its work pending (and the table of a cleared engine unwritten): the join applies it first, on
    either engine"""
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    da, db = _dev_stream("a", k), _dev_stream("b", k)
    torch.cuda.synchronize()
    bounds = ((1, MAX, 0, 0), (3, 10, 1, MAX))

    def engines(mode):
        a, b = KmerEngine(k, capacity_hint=1 << 15), KmerEngine(k, capacity_hint=1 << 15)
        for e, d in ((a, da), (b, db)):
            if mode == "direct":
                e.set_option("force_path", 1)
            e.clear()
            e.count_dev(d[0].data_ptr(), d[1].data_ptr(), d[2])
            if mode == "flushed":
                e.flush()
        return a, b

    results = {}
    for mode in ("pending", "flushed", "direct"):
        a, b = engines(mode)
        with a, b:
            results[mode] = [_got(a, b, x) for x in bounds] + [a.count_join(b, *x) for x in bounds]
            if mode == "pending":
                a2, b2 = engines(mode)
                with a2, b2:                                          # count_join as the first reader, and B as the one joined
                    assert [a2.count_join(b2, *x) for x in bounds] == results[mode][2:]
                    rev = [_got(b2, a2, x) for x in bounds]
            ta, tb = _table(a), _table(b)
            assert [_want(ta, tb, x) for x in bounds] == results[mode][:2], mode
            lo, hi, cnt = a.export_ge(1)                              # a later dump of A
            assert (J.keys_of(lo, hi if (a.wide and not a.long) else None), cnt.tolist()) == J.join(ta[0], ta[1], None, None, 1, MAX)[:2]
            if mode == "pending":
                assert rev == [_want(tb, ta, x) for x in bounds]
    assert results["pending"] == results["flushed"] == results["direct"]


@pytest.mark.parametrize("k", (31, 65))
def test_nothing_is_modified(k):
    with _counted(k, "a") as a, _counted(k, "b") as b:
        def state():
            return [(_table(e), e.stats(), e.count_stats()) for e in (a, b)]
        before = state()
        for bounds in BOUNDS:
            a.count_join(b, *bounds); a.export_join(b, *bounds)
        _raw(a, b, (1, MAX, 0, MAX), 10)                              # (refused for its size: still nothing changes)
        a.export_join(None, 0, 2)
        assert state() == before


def test_filter_in_b_keeps_its_sieve(base31):
    from kmer_denovo_filter_amd import KmerEngine
    ta, tb = base31
    with _counted(31, "a") as a, KmerEngine(31, capacity_hint=len(tb[0])) as f:
        f.set_option("force_path", 4)                                 # count --if through the sieve or not at all
        f.load_filter(*_arrays(31, tb[0]))
        f.count_filtered(_stream("b", 31))
        assert f.last_count_path() == "sieve"
        tf = _table(f)
        assert tf == tb                                               # the filter is B's key set: B's counts
        _check(a, f, ta, tf, ((1, MAX, 0, 0), (3, 10, 1, MAX)), "filter in B")
        _check(f, a, tf, ta, ((0, MAX, 0, 0),), "filter in A")
        f.reset_counts()
        f.count_filtered(_stream("b", 31))
        assert f.last_count_path() == "sieve" and _table(f) == tf


# ---------------------------------------------------------------------------------------------------------------------
# capacity, order, errors, profile
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (31, 63, 65))
def test_capacity_and_order(k):
    from kmer_denovo_filter_amd._native import KDF_ERR_INVALID
    b = (2, MAX, 0, MAX)
    with _counted(k, "a") as a, _counted(k, "b") as o:
        want = list(zip(*_want(_table(a), _table(o), b)))
        n = len(want)
        assert n > 5000 and a.count_join(o, *b) == n
        # one entry too few: refused, sized, nothing behind cap
        res = _raw(a, o, b, n - 1)
        assert res[0] == KDF_ERR_INVALID and res[1] == n
        assert b"room for" in a._lib.kdf_last_error(a._h)
        for arr in res[2:]:
            assert arr is None or (arr[n - 1:] == SENT).all()
        got = _raw_entries(a, res, n - 1)
        assert len(set(e[0] for e in got)) == n - 1 and set(got) <= set(want)
        # unsorted: the same entries in some order
        res = _raw(a, o, b, n)
        assert res[:2] == (0, n)
        for arr in res[2:]:
            assert arr is None or (arr[n:] == SENT).all()
        assert sorted(_raw_entries(a, res, n), key=lambda e: J.key_order(e[0])) == want
        # sorted: ascending keys, both count columns with them
        res = _raw(a, o, b, n, sorted_=1)
        assert res[:2] == (0, n) and _raw_entries(a, res, n) == want
        for arr in res[2:]:
            assert arr is None or (arr[n:] == SENT).all()
        # NULL count pointers, each and both, sorted and not
        keys_only = [e[0] for e in want]
        for srt in (0, 1):
            for wc, wo in ((False, True), (True, False), (False, False)):
                res = _raw(a, o, b, n, sorted_=srt, with_cnt=wc, with_ocnt=wo)
                assert res[:2] == (0, n)
                lo, hi = res[2][:n].view(np.uint64), None if res[3] is None else res[3][:n].view(np.uint64)
                keys = J.keys_of(lo) if a.long else J.keys_of(lo, hi)
                assert (keys if srt else sorted(keys, key=J.key_order)) == keys_only
                if srt and wc:
                    assert res[4][:n].view(np.uint32).tolist() == [e[1] for e in want]
                if srt and wo:
                    assert res[5][:n].view(np.uint32).tolist() == [e[2] for e in want]
        # cap = 0 with no buffers at all: the size alone
        nn = c_uint64(0)
        args = (a._h, o._h, 2, 0xFFFFFFFF, 0, 0xFFFFFFFF)
        rc = (a._lib.kdf_export_join_w_dev(*args, None, None, None, 0, 0, byref(nn)) if a.long
              else a._lib.kdf_export_join_dev(*args, None, None, None, None, 0, 0, byref(nn)))
        assert rc == KDF_ERR_INVALID and nn.value == n


def test_argument_errors():
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd._native import KDF_ERR_INVALID, KdfError
    with _counted(31, "a", n_reads=50) as a, _counted(31, "b", n_reads=50) as b, KmerEngine(33) as w, KmerEngine(65) as lg, KmerEngine(67) as lg2:
        a.profile(True)
        a.count_join(b)
        passes = a.get_stat("join_passes")
        assert passes == 1
        for fn in (lambda: a.count_join(a), lambda: a.export_join(a)):
            with pytest.raises(KdfError, match="itself") as ei:
                fn()
            assert ei.value.code == KDF_ERR_INVALID
        for other in (w, lg):
            with pytest.raises(KdfError, match="differ in k") as ei:
                a.count_join(other)
            assert ei.value.code == KDF_ERR_INVALID
        with pytest.raises(KdfError, match="differ in k"):
            lg.export_join(lg2)
        with pytest.raises(KdfError, match="min_count 3 > max_count 2") as ei:
            a.count_join(b, 3, 2)
        assert ei.value.code == KDF_ERR_INVALID
        with pytest.raises(KdfError, match="min_count 3 > max_count 2"):
            a.export_join(None, 3, 2)
        with pytest.raises(KdfError, match="other_min 5 > other_max 4") as ei:
            a.export_join(b, 1, None, 5, 4)
        assert ei.value.code == KDF_ERR_INVALID
        assert a.count_join(None, 1, None, 5, 4) == a.count_ge(1)     # without B the other bounds are not looked at
        # the wrong key form is refused by name
        n = c_uint64(0)
        rc = a._lib.kdf_export_join_dev(lg._h, None, 1, 2, 0, 0, None, None, None, None, 0, 0, byref(n))
        assert rc == KDF_ERR_INVALID and b"kdf_export_join_w_dev" in a._lib.kdf_last_error(lg._h)
        rc = a._lib.kdf_export_join(lg._h, None, 1, 2, 0, 0, None, None, None, None, 0, byref(n))
        assert rc == KDF_ERR_INVALID and b"kdf_export_join_w" in a._lib.kdf_last_error(lg._h)
        for name in ("kdf_export_join_w_dev", "kdf_export_join_w"):
            tail = (0, 0, byref(n)) if name.endswith("_dev") else (0, byref(n))
            rc = getattr(a._lib, name)(a._h, None, 1, 2, 0, 0, None, None, None, *tail)
            assert rc == KDF_ERR_INVALID and b"(lo, hi) form" in a._lib.kdf_last_error(a._h)
        assert a.get_stat("join_passes") == passes + 1                # (the join without B); every refusal came before a launch


def test_profile():
    with _counted(31, "a") as a, _counted(31, "b") as b:
        assert a.get_stat("join_passes") == 0 and a.get_stat("join_us") == 0
        a.count_join(b)                                               # not profiled: not timed
        assert a.get_stat("join_passes") == 0
        a.profile(True)
        a.count_join(b)
        assert a.get_stat("join_passes") == 1 and a.get_stat("join_us") > 0
        a.export_join(b)                     # count_join sizes the arrays, the host form then writes in one pass
        assert a.get_stat("join_passes") == 3
        n = c_uint64(0)                      # a cap that says nothing about the size: the host form counts first (and refuses)
        assert a._lib.kdf_export_join(a._h, b._h, 1, 0xFFFFFFFF, 0, 0, None, None, None, None, 0, byref(n)) != 0 and n.value == a.count_join(b)
        assert a.get_stat("join_passes") == 5
        assert b.get_stat("join_passes") == 0


def test_dump_join_device_tensors():
    """devkeys.dump_join: ascending device keys, sized by count_join, every key form"""
    from kmer_denovo_filter_amd import devkeys
    for k in (31, 63, 65):
        with _counted(k, "a") as a, _counted(k, "b") as b:
            want = _want(_table(a), _table(b), (3, MAX, 0, 0))[0]
            lo, hi = devkeys.dump_join(a, b, 3, other_max=0)
            assert (hi is None) == (k <= 32 or k > 63)
            lo_h = lo.cpu().numpy().view(np.uint64)
            got = J.keys_of(lo_h) if k > 63 else J.keys_of(lo_h, None if hi is None else hi.cpu().numpy().view(np.uint64))
            assert got == want and len(want) > 100
            lo, hi = devkeys.dump_join(a, None, 0, 2)
            assert lo.shape[0] == a.count_join(None, 0, 2) == len(_want(_table(a), None, (0, 2, 0, 0))[0])
            lo, hi = devkeys.dump_join(a, b, 2, 2, 1000, 2000)        # nothing selected
            assert lo.shape[0] == 0
