"""The read spool on the device (include/kdf.h "read spool"): segment words against the numpy model bit for bit, replay
against the same batches given to the engine one by one, tiers, overflow and refusals, and the discovery chain with
``KDF_SPOOL=1``."""
import os

import numpy as np
import pytest
import torch

import spool_model as M
from conftest import GIAB

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_NOMEM, ERR_STATE = 1, 3, 6


def _engine(k, hint=1 << 16):
    from kmer_denovo_filter_amd import KmerEngine
    return KmerEngine(k, capacity_hint=hint)


def _spool(hbm=1 << 30, host=0, segment_positions=None):
    from kmer_denovo_filter_amd.spool import ReadSpool
    sp = ReadSpool(0, hbm, host)
    if segment_positions:
        sp.set_option("segment_positions", segment_positions)
    return sp


def _stream(packed, invalid, n):
    from kmer_denovo_filter_amd.reads import ReadStream
    return ReadStream(packed, invalid, n, np.zeros(1, np.int64))


def _dev(a):
    return torch.from_numpy(a.view(np.int64)).cuda()


def _segments(sp):
    return [sp.read_segment(i) for i in range(sp.stat("segments"))]


def _same_segments(sp, want):
    got = _segments(sp)
    assert len(got) == len(want)
    for (gp, gm, gn), (wp, wm, wn) in zip(got, want):
        assert gn == wn
        np.testing.assert_array_equal(gp, wp)
        np.testing.assert_array_equal(gm, wm)


# ------------------------------------------------------------------ 1. layout

LENGTHS = [0, 1, 63, 64, 65, 127, 128, 4095, 4096, 300001, 700, 64 * 7, 1500, 31]


@pytest.fixture(scope="module")
def dirty_batches():
    """random bases, ~2 % invalid positions, random bits at and past n_bases; arrays of exactly stream_words(n)"""
    rng = np.random.default_rng(11)
    out = []
    for n in LENGTHS:
        out.append(M.pack(rng.integers(0, 4, n).astype(np.uint8), rng.random(n) < 0.02, rng) + (n,))
        assert (len(out[-1][0]), len(out[-1][1])) == M.stream_words(n)
    return out, M.segments(out, 1 << 12)


@pytest.mark.parametrize("form", ["append", "append_dev", "append_uploaded"])
def test_layout_bit_for_bit_against_the_model(dirty_batches, form):
    batches, want = dirty_batches
    assert len(want) >= 5 and max(w[2] for w in want) == 64 * (300001 // 64 + 1)
    with _spool(segment_positions=1 << 12) as sp:
        if form == "append":
            for p, m, n in batches:
                sp.append(p, m, n)
        elif form == "append_dev":
            side = torch.cuda.Stream()
            for j, (p, m, n) in enumerate(batches):
                dp, dm = _dev(p), _dev(m)
                torch.cuda.synchronize()
                # (8-byte aligned only, every other batch: the kernel's two-load path; and two streams in turn)
                if j % 2:
                    dp = torch.cat([dp.new_zeros(1), dp])[1:]
                    torch.cuda.synchronize()
                sp.append_dev(dp.data_ptr(), dm.data_ptr(), n, side.cuda_stream if j % 3 == 0 else 0)
                torch.cuda.synchronize()
        else:
            with _engine(31) as eng:
                for j, (p, m, n) in enumerate(batches):
                    eng.upload_async(j & 1, _stream(p, m, n))
                    sp.append_uploaded(eng, j & 1)
                    eng.count_uploaded(j & 1)                      # the slot kept its batch
                assert eng.stats()[2] > 0
        assert sp.stat("batches") == len([b for b in batches if b[2]]) and sp.stat("bases") == sum(LENGTHS)
        assert sp.stat("positions") == sum(w[2] for w in want)
        assert sp.stat("hbm_bytes") > 0 and sp.stat("host_bytes") == 0 and sp.stat("overflowed") == 0
        _same_segments(sp, want)


# ------------------------------------------------------------------ 2. replay equals direct

def _cut_batches(k, seed=3):
    """~3000 ragged reads (0.3 % substitutions, a few N) over a small genome as ONE stream, cut into about ten ragged
    batches at arbitrary positions, so a batch may cut a read.  One batch has a length that is a multiple of 64 and ends
    in the middle of a read, inside a run of k valid bases: the first bases of the next batch would complete valid
    k-mers with its last bases, and without the padding tile a spool would count them.  Every batch is packed into arrays
    of exactly stream_words(n) words with random bits at and past n."""
    from kmer_denovo_filter_amd.reads import ReadStream
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, 20000)
    reads = []
    for _ in range(3000):
        n = int(rng.integers(max(k + 10, 40), 151))
        a = int(rng.integers(0, len(genome) - n))
        g = genome[a:a + n].copy()
        err = rng.random(n) < 0.003
        g[err] = (g[err] + 1) % 4
        r = np.array(list("ACGT"))[g]
        if rng.random() < 0.05:
            r[int(rng.integers(0, n))] = "N"
        reads.append("".join(r))
    st = ReadStream.from_strings(reads)
    codes, inv = M.unpack(st.packed, st.invalid, st.n_bases)
    edges = sorted({0, st.n_bases} | {int(x) for x in rng.integers(1000, st.n_bases - 1000, 9)})
    start = edges[2]
    end = next(j for j in range(start + 64 * 100, st.n_bases, 64) if not inv[j - k // 2:j - k // 2 + k].any())
    edges = sorted({e for e in edges if not start < e <= end + 200} | {end})
    batches = [M.pack(codes[a:b], inv[a:b], rng) + (b - a,) for a, b in zip(edges[:-1], edges[1:])]
    assert any(n % 64 == 0 for _, _, n in batches) and len(batches) >= 6
    return batches


@pytest.fixture(scope="module", params=[31, 63, 101])
def replay_case(request):
    return request.param, _cut_batches(request.param)


def _dump(eng):
    lo, hi, cnt = eng.export_ge(0)
    return [np.asarray(lo), None if hi is None else np.asarray(hi), np.asarray(cnt)]


def _same_engine_state(a, b):
    da, db = _dump(a), _dump(b)
    for x, y in zip(da, db):
        if x is None:
            assert y is None
        else:
            np.testing.assert_array_equal(x, y)
    assert a.stats()[1:] == b.stats()[1:]
    return da


def _fill(sp, batches):
    for p, m, n in batches:
        sp.append(p, m, n)
    return sp


def _direct(eng, batches, how="count"):
    for p, m, n in batches:
        getattr(eng, how)(_stream(p, m, n))


def _check_all_modes(k, batches, sp):
    with _engine(k) as a, _engine(k) as b, _engine(k) as c:
        # mode 0, and the same spool into a second engine
        _direct(a, batches)
        sp.replay(b, sp.COUNT)
        sp.replay(c, sp.COUNT)
        full = _same_engine_state(a, b)
        _same_engine_state(a, c)
        assert a.stats()[2] > 0 and len(full[2]) > 1000 and sp.stat("replays") >= 2
        # a window that ran from the 64-multiple batch into the next would show here: every engine must agree with the
        # sum of the batches counted ALONE
        total = 0
        for p, m, n in batches:
            c.clear()
            c.count(_stream(p, m, n))
            total += c.stats()[2]
        assert total == a.stats()[2]
        # mode 0 under key_parts = 3, slice by slice
        a.set_option("key_parts", 3); b.set_option("key_parts", 3)
        n_keys = 0
        for part in range(3):
            for e in (a, b):
                e.clear(); e.set_option("key_part", part)
            _direct(a, batches)
            sp.replay(b, sp.COUNT)
            n_keys += len(_same_engine_state(a, b)[2])
        assert n_keys == len(full[2])
        a.set_option("key_parts", 0); b.set_option("key_parts", 0)
        # mode 1 on a loaded filter: the keys seen at least twice
        keep = full[2] >= 2
        flt = (full[0][keep], None if full[1] is None else full[1][keep])
        for e in (a, b):
            e.clear(); e.load_filter(*flt)
        _direct(a, batches, "count_filtered")
        sp.replay(b, sp.COUNT_FILTERED)
        got = _same_engine_state(a, b)
        np.testing.assert_array_equal(got[2], full[2][keep])
        # mode 2: the sieve words, then armed and gated
        for e in (a, b):
            e.clear(); e.prefilter_begin(2, 20)
        _direct(a, batches, "prefilter_add")
        sp.replay(b, sp.TALLY)
        np.testing.assert_array_equal(a.prefilter_export(), b.prefilter_export())
        assert list(a.prefilter_fill()) == list(b.prefilter_fill())
        assert a.get_stat("prefilter_windows") == b.get_stat("prefilter_windows") > 0
        for e in (a, b):
            e.prefilter_arm()
        _direct(a, batches)
        sp.replay(b, sp.COUNT)
        gated = _same_engine_state(a, b)
        assert 0 < len(gated[2]) < len(full[2])
    return full


def test_replay_equals_direct(replay_case):
    k, batches = replay_case
    with _spool(segment_positions=1 << 16) as sp:
        _fill(sp, batches)
        assert sp.stat("segments") >= 4
        before = _segments(sp)
        _check_all_modes(k, batches, sp)
        _same_segments(sp, before)                                  # a replay does not change the spool


# ------------------------------------------------------------------ 3. tiers

@pytest.fixture(scope="module")
def tier_batches():
    k, batches = 31, _cut_batches(31, seed=9)
    small = []
    for p, m, n in batches:                                         # no batch above one segment: all segments the same size
        codes, inv = M.unpack(p, m, n)
        for a in range(0, n, 40000):
            small.append(M.pack(codes[a:a + 40000], inv[a:a + 40000]) + (len(codes[a:a + 40000]),))
    return k, small


SEG_BYTES = (2 * 1024 + 4 + 1024 + 2) * 8                           # a segment of 2^16 positions


@pytest.mark.parametrize("hbm, host", [(0, 1 << 30), (SEG_BYTES + 100, 1 << 30)])
def test_tiers(tier_batches, hbm, host):
    k, batches = tier_batches
    with _spool(hbm, host, segment_positions=1 << 16) as sp:
        _fill(sp, batches)
        nseg = sp.stat("segments")
        assert nseg >= 4
        assert sp.stat("hbm_bytes") == (SEG_BYTES if hbm else 0)
        assert sp.stat("host_bytes") == (nseg - (1 if hbm else 0)) * SEG_BYTES
        _same_segments(sp, M.segments(batches, 1 << 16))
        _check_all_modes(k, batches, sp)


def test_host_tier_filled_from_device_buffers_and_upload_slots(tier_batches):
    k, batches = tier_batches
    want = M.segments(batches, 1 << 16)
    with _spool(0, 1 << 30, segment_positions=1 << 16) as sp, _engine(k) as eng, _engine(k) as ref:
        eng.prefilter_begin(2, 16)
        for j, (p, m, n) in enumerate(batches):
            if j % 2:
                dp, dm = _dev(p), _dev(m)
                torch.cuda.synchronize()
                sp.append_dev(dp.data_ptr(), dm.data_ptr(), n)
                torch.cuda.synchronize()
            else:
                eng.upload_async(0, _stream(p, m, n))
                sp.append_uploaded(eng, 0)
                eng.prefilter_add_uploaded(0)
        _same_segments(sp, want)
        eng.prefilter_drop()
        sp.replay(eng, sp.COUNT)
        _direct(ref, batches)
        _same_engine_state(ref, eng)


# ------------------------------------------------------------------ 4. overflow and state

def test_overflow_and_clear(tier_batches):
    from kmer_denovo_filter_amd._native import KdfError
    k, batches = tier_batches
    with _spool(SEG_BYTES, 0, segment_positions=1 << 16) as sp, _engine(k) as eng:
        eng.count(_stream(*batches[0]))
        before = (_dump(eng), eng.stats())
        stored = []
        with pytest.raises(KdfError) as ei:
            for b in batches:
                sp.append(*b)
                stored.append(b)
        assert ei.value.code == ERR_NOMEM and 0 < len(stored) < len(batches)
        assert sp.stat("overflowed") == 1 and sp.stat("segments") == 1 and sp.stat("batches") == len(stored)
        with pytest.raises(KdfError) as ei:
            sp.append(*batches[0])
        assert ei.value.code == ERR_STATE and "overflowed" in str(ei.value)
        with pytest.raises(KdfError) as ei:
            sp.replay(eng, sp.COUNT)
        assert ei.value.code == ERR_STATE
        after = (_dump(eng), eng.stats())
        for x, y in zip(before[0], after[0]):
            assert (x is None and y is None) or np.array_equal(x, y)
        assert before[1] == after[1]
        _same_segments(sp, M.segments(stored, 1 << 16))             # what is stored stays readable
        sp.clear()
        assert [sp.stat(s) for s in ("overflowed", "segments", "batches", "bases", "hbm_bytes")] == [0] * 5
        sp.append(*batches[0])
        eng.clear()
        sp.replay(eng, sp.COUNT)
        for x, y in zip(before[0], _dump(eng)):
            assert (x is None and y is None) or np.array_equal(x, y)


def test_refusals(tier_batches):
    from kmer_denovo_filter_amd._native import KdfError
    k, batches = tier_batches
    with _spool(1 << 30, 1 << 30, segment_positions=1 << 16) as sp, _engine(k) as eng, _engine(k) as other:
        # above 2^31 positions: refused by the argument check, before any allocation (the pointers are never read)
        tiny = torch.zeros(16, dtype=torch.int64, device="cuda")
        for call in (lambda: sp.append_dev(tiny.data_ptr(), tiny.data_ptr(), (1 << 31) + 1),
                     lambda: sp.append(np.zeros(8, np.uint64), np.zeros(8, np.uint64), (1 << 31) + 1)):
            with pytest.raises(KdfError) as ei:
                call()
            assert ei.value.code == ERR_INVALID
        assert sp.stat("segments") == 0 and sp.stat("hbm_bytes") == 0 and sp.stat("host_bytes") == 0
        with pytest.raises(KdfError) as ei:
            sp.set_option("segment_positions", 1 << 11)
        assert ei.value.code == ERR_INVALID
        with pytest.raises(KdfError) as ei:
            sp.append_uploaded(eng, 0)                              # nothing uploaded
        assert ei.value.code == ERR_STATE
        _fill(sp, batches[:3])
        held = _segments(sp)
        # the engine's own rule, with its own message: a plain count while the prefilter is tallying
        eng.prefilter_begin(2, 16)
        with pytest.raises(KdfError) as ei:
            sp.replay(eng, sp.COUNT)
        assert ei.value.code == ERR_STATE and "tallying" in str(ei.value) and "segment 0" in str(ei.value)
        assert eng.get_stat("prefilter_windows") == 0
        eng.prefilter_drop()
        with pytest.raises(KdfError) as ei:
            sp.replay(eng, sp.COUNT_FILTERED)                       # count --if without a filter
        assert ei.value.code == ERR_STATE and "filter" in str(ei.value)
        with pytest.raises(KdfError) as ei:
            sp.replay(eng, 3)
        assert ei.value.code == ERR_INVALID
        assert eng.stats()[1:] == (0, 0)
        _same_segments(sp, held)                                    # the spool is intact ...
        sp.replay(eng, sp.COUNT)                                    # ... and usable
        _direct(other, batches[:3])
        _same_engine_state(other, eng)
    # a host-tier replay needs the upload slots: one that holds a caller's batch refuses it, nothing is replayed
    with _spool(0, 1 << 30, segment_positions=1 << 16) as sp, _engine(k) as eng:
        _fill(sp, batches[:3])
        eng.upload_async(1, _stream(*batches[0]))
        with pytest.raises(KdfError) as ei:
            sp.replay(eng, sp.COUNT)
        assert ei.value.code == ERR_STATE and "slot 1" in str(ei.value)
        assert eng.stats()[1:] == (0, 0)
        eng.count_uploaded(1)                                       # the caller's batch is still there
        assert eng.stats()[2] > 0


def test_spool_and_engine_on_different_devices():
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd._native import KdfError
    from kmer_denovo_filter_amd.spool import ReadSpool
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    with ReadSpool(1, 1 << 20, 0) as sp, KmerEngine(31, capacity_hint=1 << 10, device=0) as eng:
        with pytest.raises(KdfError) as ei:
            sp.replay(eng, 0)
        assert ei.value.code == ERR_INVALID


def test_profile_times_the_append_kernel(tier_batches):
    _, batches = tier_batches
    with _spool(1 << 30, 0) as sp:
        sp.set_option("profile", 1)
        _fill(sp, batches[:4])
        assert sp.stat("append_passes") == 4 and sp.stat("append_us") > 0


# ------------------------------------------------------------------ 5. the chain

def _child(tmp, monkeypatch, env):
    from kmer_denovo_filter_amd.core import jellyfish_wrappers as W
    from kmer_denovo_filter_amd.discovery import pipeline as P
    for name in ("KDF_KEY_PARTS", "KDF_PREFILTER", "KDF_SPOOL", "KDF_SPOOL_HBM_GB", "KDF_SPOOL_HOST_GB"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    opened = []
    real = W.bam_reader
    monkeypatch.setattr(W, "bam_reader", lambda *a, **kw: (opened.append(1), real(*a, **kw))[1])
    os.makedirs(tmp, exist_ok=True)
    fa, n = P._extract_child_kmers_discovery(os.path.join(GIAB, "HG002_child.bam"), None, 31, 3, 4, tmp)
    monkeypatch.setattr(W, "bam_reader", real)
    return open(fa, "rb").read(), n, len(opened), dict(P.LAST_CHILD_SPOOL), dict(P.LAST_CHILD_COUNT)


@pytest.mark.parametrize("env, passes, mode", [({"KDF_KEY_PARTS": "3"}, 3, "plain"), ({"KDF_PREFILTER": "1"}, 2, "two_pass")])
def test_chain_with_the_spool_reads_the_bam_once(tmp_path, monkeypatch, env, passes, mode):
    plain, n, opened, sp0, cnt0 = _child(str(tmp_path / "a"), monkeypatch, env)
    assert n == 51125 and cnt0["mode"] == mode
    assert sp0 == {"used": False, "segments": 0, "positions": 0, "hbm_bytes": 0, "host_bytes": 0, "overflowed": False, "bam_passes": passes}
    spooled, n1, opened1, sp1, cnt1 = _child(str(tmp_path / "b"), monkeypatch, dict(env, KDF_SPOOL="1"))
    assert spooled == plain and n1 == n and cnt1 == cnt0           # LAST_CHILD_COUNT keeps its exact keys
    assert sp1["used"] and not sp1["overflowed"] and sp1["bam_passes"] == 1
    assert sp1["segments"] >= 1 and sp1["positions"] > 0 and sp1["hbm_bytes"] > 0 and sp1["host_bytes"] == 0
    assert opened1 >= 1 and opened == passes * opened1             # one round of reader openings instead of `passes`


def test_chain_falls_back_when_the_spool_overflows(tmp_path, monkeypatch):
    plain, n, opened, _, _ = _child(str(tmp_path / "a"), monkeypatch, {"KDF_KEY_PARTS": "3"})
    again, n1, opened1, sp1, _ = _child(str(tmp_path / "b"), monkeypatch, {"KDF_KEY_PARTS": "3", "KDF_SPOOL": "1", "KDF_SPOOL_HBM_GB": "0"})
    assert again == plain and n1 == n == 51125
    assert sp1["used"] and sp1["overflowed"] and sp1["bam_passes"] == 3 and opened1 == opened
