"""kdf_variant_windows / kdf_variant_evidence on the GPU against the plain-Python model of tests/variants_model.py
(written from include/kdf.h).  Cases come from the generator the CPU test checks against the host helpers: about 300
reads and 40 variants, runs of equal positions included.  The reference of a k is computed once and shared."""
import types

import numpy as np
import pytest
import torch

import kmer_truth as KT
import variants_model as VM
from test_gpu_depth import cuda_words, new_engine

pytestmark = pytest.mark.gpu

KS = [5, 31, 33, 63, 75]
GUARD = 32
KDF_ERR_INVALID = 1
_COMP = str.maketrans("ACGT", "TGCA")
_CASES = {}


def case_of(k):
    """(case, the model's answer) for k, made once"""
    if k not in _CASES:
        case = VM.random_case(9100 + k, n_reads=300, n_var=40, min_baseq=20, lo=max(20, k - 6), hi=max(60, k + 70))
        _CASES[k] = (case, VM.variant_windows(case, k))
    return _CASES[k]


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(k):
        if k not in made:
            made[k] = new_engine(k, hint=1 << 12)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def stream(case):
    return types.SimpleNamespace(packed=case["packed"], invalid=case["invalid"], n_bases=case["n_bases"], offsets=case["offsets"])


def host_form(e, case, n_bases=None, **caps):
    q = case["qual"] is not None and case["min_baseq"] > 0
    return e.variant_windows(stream(case), case["ref_start"], case["cigar"], case["cigar_offsets"], case["var_pos"], case["var_span"],
                             case["var_ref_len"], case["alt"], case["alt_offsets"], case["qual"] if q else None,
                             case["qual_offsets"] if q else None, case["min_baseq"], n_bases=n_bases, **caps)


def dev(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    if a.nbytes == 0:
        a = np.zeros(1, dt)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def guarded(n, dt):
    """n elements of dt between two guard regions of 0x5A bytes -> (tensor, pointer to the first element)"""
    sz = np.dtype(dt).itemsize
    t = torch.full(((n + 2 * GUARD) * sz,), 0x5A, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + GUARD * sz


def unguard(t, n, dt, written):
    sz = np.dtype(dt).itemsize
    a = t.cpu().numpy()
    assert (a[:GUARD * sz] == 0x5A).all() and (a[(GUARD + written) * sz:] == 0x5A).all(), "a write outside the first `written` elements"
    return a[GUARD * sz:(GUARD + n) * sz].view(dt).copy()


def device_form(e, case, pair_cap=None, entry_cap=None, n_bases=None, buffers=None):
    """variant_windows_dev into guarded outputs -> (n_pairs, n_entries, the five arrays cut to min(count, cap))"""
    nb = case["n_bases"] if n_bases is None else n_bases
    dp, dm = buffers if buffers is not None else (cuda_words(case["packed"]), cuda_words(case["invalid"]))
    q = case["qual"] is not None and case["min_baseq"] > 0
    ins = [dev(case["offsets"], np.int64), dev(case["ref_start"], np.int64), dev(case["cigar"], np.uint32), dev(case["cigar_offsets"], np.int64),
           dev(case["qual"] if q else [], np.uint8), dev(case["qual_offsets"] if q else [], np.int64), dev(case["var_pos"], np.int64),
           dev(case["var_span"], np.uint32), dev(case["var_ref_len"], np.uint32), dev(np.frombuffer(case["alt"], np.uint8), np.uint8),
           dev(case["alt_offsets"], np.int64)]
    do, drs, dcg, dco, dq, dqo, dvp, dvs, dvr, dal, dao = (t.data_ptr() for t in ins)
    args = (dp.data_ptr(), dm.data_ptr(), nb, do, len(case["offsets"]) - 1, drs, dcg, len(case["cigar"]), dco, dq if q else None,
            len(case["qual"]) if q else 0, dqo if q else None, case["min_baseq"], dvp, dvs, dvr, len(case["var_pos"]), dal, len(case["alt"]), dao)
    torch.cuda.synchronize()
    if pair_cap is None or entry_cap is None:
        pair_cap, entry_cap = e.variant_windows_dev(*args, None, None, None, 0, None, None, 0)            # the sizing call
    dts = (np.int64, np.uint32, np.uint8, np.uint64, np.uint64)
    caps = (pair_cap, pair_cap, pair_cap, entry_cap, entry_cap)
    outs = [guarded(c, dt) for c, dt in zip(caps, dts)]
    torch.cuda.synchronize()
    n_pairs, n_ent = e.variant_windows_dev(*args, outs[0][1], outs[1][1], outs[2][1], pair_cap, outs[3][1], outs[4][1], entry_cap, check=False)
    e.synchronize()
    got = [unguard(t, min(c, n), dt, min(c, n)) for (t, _p), c, dt, n in zip(outs, caps, dts, (n_pairs,) * 3 + (n_ent,) * 2)]
    return n_pairs, n_ent, got


def same(got, want, what):
    for g, w, name in zip(got, want, ("pair_read", "pair_var", "pair_flags", "entry_pos", "entry_pair")):
        assert g.dtype == w.dtype and np.array_equal(g, w), f"{what}: {name} differs (first at {np.flatnonzero(g[:len(w)] != w[:len(g)])[:5]}, lengths {len(g)} / {len(w)})"


@pytest.mark.parametrize("k", KS)
def test_host_and_device_forms_equal_the_model(engines, k):
    e = engines(k)
    case, want = case_of(k)
    assert len(want[0]) > 40 and 0 < want[2].sum() < len(want[2]) and len(want[3]) > len(want[0])
    runs = np.diff(case["var_pos"]) == 0
    assert runs.any() and len(set(want[1].tolist())) > 10
    same(host_form(e, case), want, "host form")
    n_pairs, n_ent, got = device_form(e, case)
    assert (n_pairs, n_ent) == (len(want[0]), len(want[3]))
    same(got, want, "device form")
    n_pairs, n_ent, again = device_form(e, case)
    same(again, got, "second run")
    # without the quality rule there are more entries, and the same with min_baseq = 0 or without the arrays
    noq = dict(case, min_baseq=0)
    want0 = VM.variant_windows(noq, k)
    assert len(want0[3]) > len(want[3])
    same(host_form(e, noq), want0, "host form, min_baseq 0")
    same(device_form(e, dict(case, qual=None, qual_offsets=None))[2], want0, "device form, no qualities")


def sub_case(case, a, b):
    return VM.pack_case(case["reads"][a:b], case["variants"], case["min_baseq"])


@pytest.mark.parametrize("k", [5, 33, 75])
def test_one_call_equals_three_calls(engines, k):
    e = engines(k)
    case, want = case_of(k)
    n = len(case["reads"])
    parts, n_pairs = [[] for _ in range(5)], 0
    for a, b in ((0, 97), (97, 98), (98, n)):
        sub = sub_case(case, a, b)
        assert np.array_equal(sub["var_pos"], case["var_pos"])
        _np, _ne, got = device_form(e, sub)
        pr, pv, pf, ep, epair = got
        # back to the whole case's read indices and stream positions
        ep = ep + np.uint64(int(case["offsets"][a])) if len(ep) else ep
        for lst, x in zip(parts, (pr + a, pv, pf, ep, epair + np.uint64(n_pairs))):
            lst.append(x)
        n_pairs += len(pr)
    same([np.concatenate(x) for x in parts], want, "three calls")


def test_caps_and_the_sizing_call(engines):
    e = engines(31)
    case, want = case_of(31)
    P, E = len(want[0]), len(want[3])
    for pc, ec in ((P, E - 1), (P - 1, E), (P // 2, E // 3), (0, E), (P, 0)):
        n_pairs, n_ent, got = device_form(e, case, pair_cap=pc, entry_cap=ec)      # (the guards: nothing past the caps)
        assert (n_pairs, n_ent) == (P, E)
        same(got, [w[:c] for w, c in zip(want, (pc, pc, pc, ec, ec))], f"caps {pc}, {ec}")
        with pytest.raises(RuntimeError):
            host_form(e, case, pair_cap=pc, entry_cap=ec)
    same(host_form(e, case, pair_cap=P + 5, entry_cap=E + 9), want, "roomy caps")
    # nothing to do: KDF_OK and both counts set to 0
    from ctypes import byref, c_uint64
    a, b = c_uint64(7), c_uint64(7)
    rc = e._lib.kdf_variant_windows_dev(e._h, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, None, None, None, 0, None, 0, None,
                                        None, None, None, 0, None, None, 0, byref(a), byref(b))
    assert rc == 0 and (a.value, b.value) == (0, 0)


def test_empty_shapes(engines):
    e = engines(5)
    case, _ = case_of(5)
    none = VM.pack_case([], case["variants"])
    for c in (none, VM.pack_case(case["reads"][:5], []), dict(case, n_bases=0)):
        got = host_form(e, c, n_bases=c["n_bases"])
        assert all(len(x) == 0 for x in got)
        n_pairs, n_ent, _ = device_form(e, c, n_bases=c["n_bases"])
        assert (n_pairs, n_ent) == (0, 0)
    empty_cigars = VM.pack_case([(s, [], rs, q) for s, _ops, rs, q in case["reads"][:20]], case["variants"])
    assert all(len(x) == 0 for x in host_form(e, empty_cigars))
    assert device_form(e, empty_cigars)[:2] == (0, 0)
    # variants that no read reaches
    far = VM.pack_case(case["reads"][:20], [(10 ** 9 + i, 1, 1, b"A") for i in range(4)])
    assert device_form(e, far)[:2] == (0, 0) and all(len(x) == 0 for x in host_form(e, far))


def test_a_long_read_with_200_operations(engines):
    k = 31
    e = engines(k)
    rng = np.random.default_rng(4242)
    ops = []
    while len(ops) < 199:
        ops += [(0, int(rng.integers(30, 60))), (int(rng.choice([1, 2, 3, 1, 2])), int(rng.integers(1, 9)))]
    ops = ops[:199] + [(0, 30)]
    qlen = sum(ln for op, ln in ops if op in (0, 1))
    assert len(ops) == 200 and 4000 < qlen <= 5000
    seq = "".join(rng.choice(list("ACGT"), 5000))             # longer than the CIGAR consumes: the tail aligns nowhere
    q = rng.integers(25, 41, 5000).astype(np.uint8)
    q[rng.random(5000) < 0.01] = 3
    short = VM.random_read(rng, lo=40, hi=80)
    reads = [short[:2] + (50,) + short[3:], (seq, ops, 100, q), short[:2] + (2500,) + short[3:]]
    rtot = VM.walk(ops)[2]
    variants = VM.variants_for(rng, [reads[1]], 60)
    variants += [(100 + rtot - 1, 1, 1, b"A"), (100 + rtot, 1, 1, b"A"), (100, 3, 1, seq[:3].encode())]
    case = VM.pack_case(reads, variants, 20)
    want = VM.variant_windows(case, k)
    assert (want[0] == 1).sum() > 30 and want[2].sum() > 3
    same(host_form(e, case), want, "host form")
    same(device_form(e, case)[2], want, "device form")


@pytest.mark.parametrize("k", [5, 33])
def test_a_prefix_with_dirty_words_past_n_bases(engines, k):
    from test_gpu_read_hits import dirty_buffers
    e = engines(k)
    case, want = case_of(k)
    r = int(want[0][len(want[0]) // 2])                      # cut inside a read that has entries
    inside = want[3][want[0][want[4].astype(np.int64)] == r].astype(np.int64)
    n_cut = int(inside.min()) + k + (int(inside.max()) - int(inside.min())) // 2
    cut = VM.variant_windows(case, k, n_bases=n_cut)
    assert 0 < len(cut[3]) < len(want[3]) and int(cut[3].max()) + k <= n_cut
    for mask_fill in (0, 1):                                 # past n_cut: every mask bit clear (would read as valid bases), or set
        bufs = dirty_buffers(stream(case), n_cut, mask_fill)
        same(device_form(e, case, n_bases=n_cut, buffers=bufs)[2], cut, f"prefix, mask fill {mask_fill}")
    same(host_form(e, case, n_bases=n_cut), cut, "host form, prefix")


# ---- evidence ---------------------------------------------------------------------------------------------------------------

def entry_keys(case, k, got):
    """the canonical key of every entry, as an integer, from the read strings"""
    pr, _pv, _pf, ep, epair = got
    out = []
    for p, i in zip(ep.tolist(), epair.tolist()):
        r = int(pr[int(i)])
        s = int(p) - int(case["offsets"][r])
        w = case["reads"][r][0].upper()[s:s + k]
        out.append(min(KT.key_int(w), KT.key_int(w[::-1].translate(_COMP))))
    return out


def device_evidence(e, rows, entry_pair, pair_var, pair_flags, n_var):
    dk, dep, dpv, dpf = dev(rows, np.uint64), dev(entry_pair, np.uint64), dev(pair_var, np.uint32), dev(pair_flags, np.uint8)
    tp, pp = guarded(len(pair_var) * 2, np.uint32)
    tv, pv_ = guarded(n_var * 8, np.uint64)
    torch.cuda.synchronize()
    e.variant_evidence_dev(dk.data_ptr(), dep.data_ptr(), len(entry_pair), dpv.data_ptr(), dpf.data_ptr(), len(pair_var), n_var, pp, pv_)
    e.synchronize()
    return (unguard(tp, len(pair_var) * 2, np.uint32, len(pair_var) * 2).reshape(-1, 2),
            unguard(tv, n_var * 8, np.uint64, n_var * 8).reshape(-1, 8))


def two_batches_reversed(case, k, want):
    """the entries and pairs of the case as two batches (reads split in two), concatenated second batch first and each
    batch's pairs in reversed order: pairs come in no order of variants, entries stay grouped by pair"""
    pr, pv, pf, ep, epair = want
    keys = np.asarray(entry_keys(case, k, want), dtype=object)
    half = len(case["reads"]) // 2
    order = np.concatenate((np.flatnonzero(pr >= half)[::-1], np.flatnonzero(pr < half)[::-1]))
    new_of = np.empty(len(pr), np.int64)
    new_of[order] = np.arange(len(pr))
    eorder = np.concatenate([np.flatnonzero(epair == np.uint64(i)) for i in order])
    return list(keys[eorder]), new_of[epair[eorder].astype(np.int64)].astype(np.uint64), pv[order], pf[order]


@pytest.mark.parametrize("mode", ["insert", "filter"])
@pytest.mark.parametrize("k", KS)
def test_evidence_equals_the_model(k, mode):
    case, want = case_of(k)
    rng = np.random.default_rng(600 + k)
    keys, entry_pair, pair_var, pair_flags = two_batches_reversed(case, k, want)
    n_var = len(case["var_pos"])
    distinct = sorted(set(keys))
    stored = [v for v in distinct if rng.random() < 0.5]
    with new_engine(k, hint=1 << 12) as e:
        W = e.key_words
        args = lambda ks: (KT.rows(ks, W),) if e.long else (KT.lohi(ks)[0], KT.lohi(ks)[1] if e.wide else None)
        if mode == "insert":
            counts = {v: 0 if rng.random() < 0.1 else int(rng.integers(1, 2000)) for v in stored}     # (some stored with count 0)
            cnt = np.asarray([counts[v] for v in stored], np.uint32)
            if e.long:
                e.add_pairs(KT.rows(stored, W), None, cnt)
            else:
                e.add_pairs(*args(stored), cnt)
        else:
            from kmer_denovo_filter_amd import ReadStream
            e.load_filter(*args(stored))
            some, more = [s for s, *_ in case["reads"][::3]], [s for s, *_ in case["reads"][::2]]
            if k < 8:                                                            # (so few keys that 250 reads hold them all)
                some, more = some[:6], more[:3]
            e.count_filtered(ReadStream.from_strings(some))
            e.count_filtered(ReadStream.from_strings(more))                      # (every sixth read twice; a third never:
            counts = KT.count_truth(some + more, k, filt=stored)                 #  keys of the filter with count 0)
        assert any(counts.get(v, 0) == 0 for v in stored) and any(counts.get(v, 0) > 1 for v in stored)
        # out-of-range indices: an entry of no pair, a pair of no variant (its entries count nowhere)
        keys = keys + [keys[0], keys[1]]
        entry_pair = np.concatenate((entry_pair, np.asarray([len(pair_var) + 3, len(pair_var)], np.uint64)))
        pair_var = np.concatenate((pair_var, np.asarray([n_var], np.uint32)))
        pair_flags = np.concatenate((pair_flags, np.asarray([1], np.uint8)))
        wp, wv = VM.variant_evidence(keys, entry_pair, pair_var, pair_flags, n_var, counts)
        assert (wp[:, 1] > 0).any() and (wp[:, 1] == 0).any() and (wv[:, 0] > 0).any() and (wv[:, 4] > 0).any()
        assert (wv[:, 4] < wv[:, 0]).any() and (wv[:, 2] < wv[:, 3]).any()
        rows = KT.rows(keys, W)
        hp, hv = e.variant_evidence(rows, entry_pair, pair_var, pair_flags, n_var)
        assert np.array_equal(hp, wp), f"host form: pair rows differ at {np.flatnonzero((hp != wp).any(axis=1))[:5]}"
        assert np.array_equal(hv, wv), f"host form: variant rows differ at {np.flatnonzero((hv != wv).any(axis=1))[:5]}"
        before = e.count_ge(0), e.count_ge(1)
        dp_, dv_ = device_evidence(e, rows, entry_pair, pair_var, pair_flags, n_var)
        assert np.array_equal(dp_, wp) and np.array_equal(dv_, wv), "device form"
        assert (e.count_ge(0), e.count_ge(1)) == before                           # the table is only read
        # a key row of all ones is no key; no entries at all: zero rows
        ones = rows.copy()
        ones[:] = ~np.uint64(0)
        op_, ov_ = device_evidence(e, ones, entry_pair, pair_var, pair_flags, n_var)
        assert np.array_equal(op_[:, 0], wp[:, 0]) and np.array_equal(op_[:, 1], wp[:, 0]) and not ov_.any()
        zp, zv = e.variant_evidence(np.zeros((0, W), np.uint64), np.zeros(0, np.uint64), pair_var, pair_flags, n_var)
        assert zp.shape == (len(pair_var), 2) and not zp.any() and not zv.any()


def test_windows_then_keys_then_evidence_on_the_device(engines):
    """the chain the driver runs: entry positions -> hit_keys -> evidence, against keys cut from the read strings"""
    k = 33
    case, want = case_of(k)
    ints = entry_keys(case, k, want)
    with new_engine(k, hint=1 << 12) as e:
        rows = e.hit_keys(stream(case), want[3])
        assert np.array_equal(rows, KT.rows(ints, e.key_words))
        e.profile(True)
        before = e.get_stat("variants_passes")
        device_form(e, case)
        device_evidence(e, rows, want[4], want[1], want[2], len(case["var_pos"]))
        assert e.get_stat("variants_passes") >= before + 3 and e.get_stat("variants_us") > 0
        e.profile(False)


def test_evidence_refuses_what_does_not_fit_63_bits():
    with new_engine(5, hint=1 << 10) as e:
        e.add_pairs(np.asarray([1, 2, 3], np.uint64), None, np.asarray([1, 1, 1], np.uint32))
        rows, ep = np.asarray([[1]], np.uint64), np.zeros(1, np.uint64)
        t = torch.zeros(64, dtype=torch.int64, device="cuda")                    # (refused before anything is written)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="63 bits"):
            e.variant_evidence_dev(t.data_ptr(), t.data_ptr(), 1, t.data_ptr(), t.data_ptr(), 1, 1 << 54, t.data_ptr(), t.data_ptr())
        e.synchronize()
        assert not t.cpu().numpy().any()
        assert e.variant_evidence(rows, ep, np.zeros(1, np.uint32), np.zeros(1, np.uint8), 1)[1][0, :4].tolist() == [1, 1, 1, 1]


# ---- refusals of the host form -----------------------------------------------------------------------------------------------

def test_host_form_refusals(engines):
    e = engines(5)
    case, want = case_of(5)
    small = VM.pack_case(case["reads"][:12], case["variants"][:8], 20)

    def refused(**change):
        with pytest.raises(RuntimeError):
            host_form(e, dict(small, **change))
    bad = small["offsets"].copy(); bad[3] = bad[2] - 1
    refused(offsets=bad)
    bad = small["offsets"].copy(); bad[0] = -1
    refused(offsets=bad)
    for name, total in (("cigar_offsets", len(small["cigar"])), ("alt_offsets", len(small["alt"])), ("qual_offsets", len(small["qual"]))):
        o = small[name]
        first = o.copy(); first[0] = 1
        down = o.copy(); down[2] = down[3] + 1
        end = o.copy(); end[-1] = total + 1
        for b in (first, down, end):
            refused(**{name: b})
    vp = small["var_pos"].copy(); vp[4] = vp[3] - 1
    refused(var_pos=vp)
    from ctypes import byref, c_uint64
    a, b = c_uint64(0), c_uint64(0)
    rc = e._lib.kdf_variant_windows(e._h, None, None, 0, None, -1, None, None, 0, None, None, 0, None, 0, None, None, None, 0, None, 0, None,
                                    None, None, None, 0, None, None, 0, byref(a), byref(b))
    assert rc == KDF_ERR_INVALID
    rc = e._lib.kdf_variant_windows_dev(e._h, None, None, 0, None, -1, None, None, 0, None, None, 0, None, 0, None, None, None, 0, None, 0, None,
                                        None, None, None, 0, None, None, 0, byref(a), byref(b))
    assert rc == KDF_ERR_INVALID
    same(host_form(e, small), VM.variant_windows(small, 5), "after the refusals")
