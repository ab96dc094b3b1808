"""Two-pass counting (include/kdf.h "two-pass counting") on the GPU: the table of a gated count holds exactly the keys
the sieve MODEL admits, with their full counts.

T = an engine-independent truth of the reads (``kmer_truth.count_truth`` at fixture size, ``stream_truth`` for packed
streams); M = ``prefilter_model``: cell(key) by the rule of kdf.h, value = min(sum of T over the cell, 3), admitted iff
value >= L.  Every test states equalities; none measures."""
import json
import math
import os

import numpy as np
import pytest

import kmer_truth as KT
import prefilter_model as PM
import stream_truth as ST
from conftest import GIAB, GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL_K = (15, 31, 32, 33, 47, 63, 75, 101, 201)


def new_engine(k, hint=1 << 16):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    torch.cuda.empty_cache()
    return KmerEngine(k, capacity_hint=hint)


def stream_of(reads):
    from kmer_denovo_filter_amd.reads import ReadStream
    return ReadStream.from_strings(reads)


def dump_dict(e, m=0):
    """{key int: count} of the entries with count >= m"""
    lo, hi, cnt = e.export_ge(m)
    if e.long:
        return {KT.int_of_row(r): int(c) for r, c in zip(lo, cnt)}
    return {int(a) | (int(b) << 64): int(c) for a, b, c in zip(lo, hi, cnt)}


def plain_engine(k, streams, hint=1 << 16):
    e = new_engine(k, hint)
    for s in streams:
        e.count(s)
    return e


def assert_exact(e, T, k, s, L, plain, what):
    """conditions 1 and 2 of the issue for a gated engine `e` against the truth T and a plain engine of the same reads"""
    admitted, by_value = PM.model(T, k, s, L)
    got = dump_dict(e, 0)
    assert len(got) == len(admitted), f"{what}: {len(got)} keys stored, the model admits {len(admitted)} of {len(T)}"
    assert got == admitted, f"{what}: the stored (key, count) set is not the model's"
    for m in (L, L + 1, 5, 100):
        assert dump_dict(e, m) == dump_dict(plain, m), f"{what}: dump -L {m} differs from the plain count's"
    hg, hp = e.histogram(300), plain.histogram(300)
    assert np.array_equal(hg[L:], hp[L:]), f"{what}: histogram bins from {L} up differ from the plain count's"
    assert e.prefilter_fill() == by_value, f"{what}: prefilter_fill"
    cap, distinct, windows = e.stats()
    assert distinct == len(admitted), f"{what}: distinct"
    assert windows == sum(admitted.values()), f"{what}: windows must count admitted windows only"
    assert e.get_stat("prefilter_windows") == sum(T.values()), f"{what}: prefilter_windows"


def reads_for(k, seed, n=160):
    rng = np.random.default_rng(seed)
    return KT.random_reads(rng, k, n, max_len=max(400, 3 * k))


# ---------------------------------------------------------------------------------------------------------------------
# condition 3: every key width, both L, every path and form
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", ALL_K)
@pytest.mark.parametrize("L", (2, 3))
def test_every_key_width(k, L):
    reads = reads_for(k, 7 * k + L)
    T = KT.count_truth(reads, k)
    assert any(c < L for c in T.values()) and any(c >= L for c in T.values())
    st = stream_of(reads)
    plain = plain_engine(k, [st])
    assert dump_dict(plain, 0) == T                                 # (the truth and the plain engine agree to begin with)
    e = new_engine(k)
    e.prefilter_begin(L, 16).prefilter_add(st).prefilter_arm()
    assert [e.get_stat(n) for n in ("prefilter_state", "prefilter_min_count", "prefilter_log2_cells", "prefilter_bytes")] == [2, L, 16, 1 << 15]
    e.count(st)
    assert_exact(e, T, k, 16, L, plain, f"k={k} L={L}")
    # drop, then a plain count on the same engine equals a fresh engine's
    e.prefilter_drop()
    assert e.get_stat("prefilter_state") == 0
    e.clear()
    e.count(st)
    assert dump_dict(e, 0) == T
    e.close(); plain.close()


@pytest.mark.parametrize("k", (31, 47))
@pytest.mark.parametrize("force_path", (0, 1, 2))
@pytest.mark.parametrize("defer", (0, 1))
def test_paths_and_deferral(k, force_path, defer):
    L = 3 if force_path != 1 else 2
    reads = reads_for(k, 100 + k, n=400)
    T = KT.count_truth(reads, k)
    st = stream_of(reads)
    plain = plain_engine(k, [st])
    e = new_engine(k, 1 << 17)
    e.set_option("force_path", force_path); e.set_option("defer", defer)
    e.prefilter_begin(L, 17).prefilter_add(st).prefilter_arm()
    e.count(st)
    if force_path == 2:
        assert e.last_count_path() == "binned"
    if force_path == 1:
        assert e.last_count_path() == "direct"
    assert_exact(e, T, k, 17, L, plain, f"k={k} force_path={force_path} defer={defer}")
    e.close(); plain.close()


@pytest.mark.parametrize("k,binned_pending", ((31, False), (31, True), (63, False), (63, True), (75, False)))
def test_many_small_batches_in_the_pending_stream(k, binned_pending):
    """the gate runs when the pending stream is partitioned / counted, not per call (long keys have no binned pipeline
    and no pending stream: their batches are gated one by one)"""
    L = 3
    reads = reads_for(k, 200 + k, n=300)
    T = KT.count_truth(reads, k)
    batches = [stream_of(reads[i:i + 7]) for i in range(0, len(reads), 7)]
    plain = plain_engine(k, batches)
    e = new_engine(k, 1 << 17)
    if binned_pending:                                              # the flush of the pending stream takes the binned pipeline
        e.set_option("binned_min_positions", 0); e.set_option("binned_bytes_per_position", 1 << 40)
    e.prefilter_begin(L, 16)
    for b in batches:
        e.prefilter_add(b)
    e.prefilter_arm()
    for b in batches:
        e.count(b)
    if k <= 63:
        assert e.get_stat("pending_positions") > 0                 # nothing has been applied yet
    assert_exact(e, T, k, 16, L, plain, f"k={k} pending stream, binned={binned_pending}")
    if k <= 63:
        assert e.last_count_path() == ("binned" if binned_pending else "direct")
    e.close(); plain.close()


def _dev_buffers(st):
    import torch
    p = torch.from_numpy(st.packed.view(np.int64).copy()).to(DEV)
    m = torch.from_numpy(st.invalid.view(np.int64).copy()).to(DEV)
    torch.cuda.synchronize()
    return p, m


@pytest.mark.parametrize("k", (31, 47, 101))
@pytest.mark.parametrize("tally_form,count_form", (("host", "dev"), ("dev", "slot"), ("slot", "host")))
def test_host_device_and_upload_slot_forms(k, tally_form, count_form):
    L = 2
    reads = reads_for(k, 300 + k, n=200)
    T = KT.count_truth(reads, k)
    halves = [stream_of(reads[:100]), stream_of(reads[100:])]
    plain = plain_engine(k, halves)
    e = new_engine(k)
    keep = []

    def feed(form, tally):
        for i, st in enumerate(halves):
            if form == "host":
                e.prefilter_add(st) if tally else e.count(st)
            elif form == "dev":
                p, m = _dev_buffers(st); keep.append((p, m))
                (e.prefilter_add_dev if tally else e.count_dev)(p.data_ptr(), m.data_ptr(), st.n_bases)
            else:
                e.upload_async(i & 1, st)
                e.prefilter_add_uploaded(i & 1) if tally else e.count_uploaded(i & 1)
    e.prefilter_begin(L, 16)
    feed(tally_form, True)
    e.prefilter_arm()
    feed(count_form, False)
    assert_exact(e, T, k, 16, L, plain, f"k={k} tally={tally_form} count={count_form}")
    e.close(); plain.close()


@pytest.mark.parametrize("k", (31, 63))
@pytest.mark.parametrize("force_path", (1, 2))
def test_batches_that_cut_reads_with_dirty_words_past_n_bases(k, force_path):
    """Both passes take the stream as two device batches: a PREFIX that ends in the middle of a read, its words at and
    past n_bases overwritten with garbage, and the rest from a tile boundary on.  The truth of each piece is
    stream_truth's (positions at or past n_bases are invalid), summed."""
    import torch
    L = 3
    reads = reads_for(k, 400 + k, n=300)
    st = stream_of(reads)
    N = st.n_bases
    cut = (N // 2) | 37                                             # not a tile boundary; lands inside a read or on a separator
    p, m = _dev_buffers(st)
    # piece 1: a copy of the words stream_words(cut) sizes, dirty from position `cut` on
    pw, mw = 2 * ((cut + 63) // 64) + 4, (cut + 63) // 64 + 2
    g = torch.Generator(device=DEV); g.manual_seed(k)
    p1, m1 = p[:pw].clone(), m[:mw].clone()
    junk_p = torch.randint(-(1 << 62), 1 << 62, (pw,), dtype=torch.int64, device=DEV, generator=g)
    junk_m = torch.randint(-(1 << 62), 1 << 62, (mw,), dtype=torch.int64, device=DEV, generator=g)
    wp, wm = cut // 32, cut // 64
    p1[wp + 1:] = junk_p[wp + 1:]
    p1[wp] = (p1[wp] & ((1 << (2 * (cut % 32))) - 1)) | (junk_p[wp] & ~((1 << (2 * (cut % 32))) - 1))
    m1[wm + 1:] = junk_m[wm + 1:]
    m1[wm] = m1[wm] & ((1 << (cut % 64)) - 1)                      # the mask bits past `cut` read VALID: the worst dirt
    t0 = cut // 64
    p2, m2 = p[2 * t0:].clone(), m[t0:].clone()
    n2 = N - 64 * t0
    torch.cuda.synchronize()
    pieces = [(p1, m1, cut), (p2, m2, n2)]
    parts = [ST.count_truth(pc, k)[:3] for pc in pieces]
    tlo, thi, tcnt = ST.accumulate(parts)
    T = {int(a) & PM.M64 | (int(b) << 64): int(c) for a, b, c in zip(tlo.cpu().numpy().view(np.uint64), thi.cpu().numpy(), tcnt.cpu().numpy())}
    plain = new_engine(k, 1 << 17)
    for a, b, n in pieces:
        plain.count_dev(a.data_ptr(), b.data_ptr(), n)
    assert dump_dict(plain, 0) == T
    e = new_engine(k, 1 << 17)
    e.set_option("force_path", force_path)
    e.prefilter_begin(L, 16)
    for a, b, n in pieces:
        e.prefilter_add_dev(a.data_ptr(), b.data_ptr(), n)
    e.prefilter_arm()
    for a, b, n in pieces:
        e.count_dev(a.data_ptr(), b.data_ptr(), n)
    assert_exact(e, T, k, 16, L, plain, f"k={k} force_path={force_path} cut stream")
    e.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# condition 4 (a tiny sieve: the degenerate end) and growth of the table while armed
# ---------------------------------------------------------------------------------------------------------------------

def _many_keys(k, seed):
    rng = np.random.default_rng(seed)
    genome = "".join(rng.choice(list("ACGT"), 400_000))
    return KT.random_reads(rng, k, 4800, genome=genome, max_len=1500)


@pytest.mark.parametrize("k,force_path,hint", ((31, 0, 1024), (31, 2, 1 << 14), (47, 1, 1024), (75, 0, 1024)))
def test_tiny_sieve_and_growth_while_armed(k, force_path, hint):
    L = 3
    reads = _many_keys(k, 500 + k)
    T = KT.count_truth(reads, k)
    assert len(T) > 250_000
    admitted, by_value = PM.model(T, k, 16, L)
    assert by_value[3] > 0.75 * (1 << 16) and len(admitted) > 0.85 * len(T)     # most cells read 3: nearly every key is admitted
    st = stream_of(reads)
    plain = plain_engine(k, [st])
    e = new_engine(k, hint)
    cap0 = e.stats()[0]
    e.set_option("force_path", force_path)
    e.prefilter_begin(L, 16).prefilter_add(st).prefilter_arm()
    e.count(st)
    assert_exact(e, T, k, 16, L, plain, f"k={k} tiny sieve force_path={force_path}")
    assert e.stats()[0] > cap0                                      # the table grew while armed
    e.close(); plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# condition 5: the state machine
# ---------------------------------------------------------------------------------------------------------------------

def _refused(code, fn, *a):
    from kmer_denovo_filter_amd._native import KdfError
    with pytest.raises(KdfError) as ei:
        fn(*a)
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


@pytest.mark.parametrize("k", (31, 47, 75))
def test_state_machine(k):
    from kmer_denovo_filter_amd import _native
    INVALID, STATE = _native.KDF_ERR_INVALID, _native.KDF_ERR_STATE
    reads = reads_for(k, 600 + k, n=120)
    T = KT.count_truth(reads, k)
    st = stream_of(reads)
    e = new_engine(k)
    e.count(st)
    before = dump_dict(e, 0)
    assert before == T

    def untouched(state):
        assert e.get_stat("prefilter_state") == state
        assert dump_dict(e, 0) == before

    # off: nothing but begin
    for fn, a in ((e.prefilter_add, (st,)), (e.prefilter_arm, ()), (e.prefilter_drop, ()), (e.prefilter_fill, ()), (e.prefilter_add_uploaded, (0,))):
        _refused(STATE, fn, *a)
    for L in (0, 1, 4, 7):
        assert "2 or 3" in _refused(INVALID, e.prefilter_begin, L, 16)
    for s in (1, 15, 39, 64):
        _refused(INVALID, e.prefilter_begin, 3, s)
    untouched(0)
    # refused together, either order
    e.set_option("key_parts", 4)
    assert "key_parts" in _refused(STATE, e.prefilter_begin, 3, 16)
    e.set_option("key_parts", 0)
    if k <= 63:
        e2 = new_engine(k)
        e2.set_option("hash_shift", 2)
        assert "hash_shift" in _refused(STATE, e2.prefilter_begin, 3, 16)
        assert e2.get_stat("prefilter_state") == 0
        e2.close()
    untouched(0)
    # tallying
    e.prefilter_begin(3, 0)
    assert e.get_stat("prefilter_log2_cells") == 19                 # ceil(log2(8 x the capacity hint of 2^16))
    assert "drop" in _refused(STATE, e.prefilter_begin, 3, 16)
    assert "tallying" in _refused(STATE, e.count, st)
    p, m = _dev_buffers(st)
    _refused(STATE, e.count_dev, p.data_ptr(), m.data_ptr(), st.n_bases)
    e.upload_async(0, st)
    _refused(STATE, e.count_uploaded, 0)
    assert "key_parts" in _refused(STATE, e.set_option, "key_parts", 2)
    if k <= 63:
        assert "hash_shift" in _refused(STATE, e.set_option, "hash_shift", 1)
    untouched(1)
    e.prefilter_add_uploaded(0)                                     # (the refused count left the slot's batch in place)
    assert e.get_stat("prefilter_windows") == sum(T.values())
    # queries, dumps, histogram, scan and add_pairs are not affected
    assert e.count_ge(0) == len(T) and int(e.histogram(10).sum()) == len(T)
    e.scan(st, want_distinct=False)
    # armed
    e.prefilter_arm()
    for fn, a in ((e.prefilter_add, (st,)), (e.prefilter_arm, ()), (e.prefilter_begin, (3, 16)), (e.prefilter_add_uploaded, (0,))):
        _refused(STATE, fn, *a)
    assert "key_parts" in _refused(STATE, e.set_option, "key_parts", 2)
    untouched(2)
    # clear empties the table and leaves the prefilter armed
    e.clear()
    assert e.get_stat("prefilter_state") == 2 and e.count_ge(0) == 0
    e.count(st)
    assert dump_dict(e, 0) == PM.model(T, k, 19, 3)[0]
    # drop: counts are ungated again; a plain count equals a fresh engine's
    e.prefilter_drop()
    e.clear()
    e.count(st)
    assert dump_dict(e, 0) == T
    e.close()


def test_profile_times_the_tally_kernel():
    k = 31
    st = stream_of(reads_for(k, 700, n=100))
    e = new_engine(k)
    e.profile(True)
    e.prefilter_begin(3, 16).prefilter_add(st).prefilter_add(st)
    assert e.get_stat("prefilter_passes") == 2 and e.get_stat("prefilter_us") > 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# conditions 6 and 7: packed streams, the model in torch on the device
# ---------------------------------------------------------------------------------------------------------------------

def _assert_stream_exact(ds, k, L, log2_cells, hint, force_path=0):
    """tally + arm + count of a device stream against stream_truth and the torch model: every stored key and count"""
    import torch
    lo, hi, cnt, n_valid = ST.count_truth(ds, k)
    n = lo.numel()
    s = log2_cells if log2_cells else min(38, max(16, math.ceil(math.log2(8 * hint))))
    keep, by_value = PM.model_torch(lo, hi, cnt, k, s, L)
    want = (lo[keep], hi[keep], cnt[keep])
    n_adm = int(keep.sum())
    ge = {m: ST.rows_ge((lo, hi, cnt), m) for m in (L, L + 1, 5, 100)}
    del keep
    torch.cuda.empty_cache()
    e = new_engine(k, hint)
    e.set_option("force_path", force_path)
    e.prefilter_begin(L, log2_cells)
    assert e.get_stat("prefilter_log2_cells") == s
    e.prefilter_add_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
    e.prefilter_arm()
    e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
    cap, distinct, windows = e.stats()
    print(f"[prefilter] k={k} L={L} cells=2^{s} distinct(T)={n} model stores {n_adm} ({n_adm / n:.3f}); engine stores {distinct}; "
          f"fill={e.prefilter_fill()} table slots={cap}", flush=True)
    return e, (lo, hi, cnt, n_valid), want, n_adm, by_value, ge


def _sorted_dump(e, m, n):
    import torch
    dlo = torch.empty(max(n, 1), dtype=torch.int64, device=DEV)
    dhi = torch.empty(max(n, 1), dtype=torch.int64, device=DEV) if e.wide else None
    dc = torch.empty(max(n, 1), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    got = e.export_ge_dev(m, dlo.data_ptr(), dhi.data_ptr() if e.wide else None, dc.data_ptr(), n, sorted_=True)
    e.synchronize()
    assert got == n
    return dlo[:n], (dhi[:n] if e.wide else torch.zeros(n, dtype=torch.int64, device=DEV)), dc[:n].to(torch.int64) & 0xFFFFFFFF


def _check_stream_engine(e, T, want, n_adm, by_value, ge, L, what):
    import torch
    cap, distinct, windows = e.stats()
    assert distinct == n_adm, f"{what}: {distinct} keys stored, the model admits {n_adm}"
    assert e.count_ge(0) == n_adm
    got = _sorted_dump(e, 0, n_adm)
    for name, g, w in zip(("lo", "hi", "counts"), got, want):
        assert torch.equal(g, w), f"{what}: {name} of the stored set differs from the model's in {int((g != w).sum())} rows"
    assert windows == int(want[2].sum()), f"{what}: windows"
    del got
    for m, rows in ge.items():                                      # dump -L m of the plain count IS the truth's rows with count >= m
        assert e.count_ge(m) == rows[0].numel(), f"{what}: count_ge({m})"
        g = _sorted_dump(e, m, rows[0].numel())
        for a, b in zip(g, rows):
            assert torch.equal(a, b), f"{what}: dump -L {m}"
    assert e.prefilter_fill() == by_value, f"{what}: prefilter_fill"
    assert e.get_stat("prefilter_windows") == T[3], f"{what}: prefilter_windows"


def test_worth_having_15x_reads_with_errors():
    """Condition 6, the cap that keeps the suite from passing on a sieve that admits everything: 15x reads of a 2 Mbp
    genome with 0.5 % substitutions, k = 31, L = 3, 8 cells per distinct key.  About 70 % of the distinct keys are error
    k-mers seen once or twice, and with m >= 8 n cells at most 1 - exp(-n / m) <= 11.8 % of them share a cell at all: the
    model stores under half of the distinct keys.  FIRST the model's own ratio (the input's fault if that fails), then
    the engine against the model, key by key."""
    import torch
    from kmer_denovo_filter_amd.synth import synth_stream
    k, L = 31, 3
    ds = synth_stream(200_000, 150, 2_000_000, seed=61, device=DEV, sub_rate=0.005)
    torch.cuda.synchronize()
    n = ST.count_truth(ds, k)[0].numel()
    s = math.ceil(math.log2(8 * n))
    e, T, want, n_adm, by_value, ge = _assert_stream_exact(ds, k, L, s, 1 << 20)
    assert n_adm <= 0.5 * n, f"the model itself stores {n_adm} of {n} distinct keys: the input was badly chosen"
    assert e.stats()[1] == n_adm
    _check_stream_engine(e, T, want, n_adm, by_value, ge, L, "15x reads")
    e.close()


def test_full_size_bench_batch_every_key():
    """Condition 7: the bench batch (10 M x 150 bp, k = 31), L = 3, the engine's own choice of cells: every stored key and
    count against stream_truth and the model; the plain and the gated `dump -L 3` equal."""
    import torch
    from kmer_denovo_filter_amd.synth import synth_stream
    k, L = 31, 3
    ds = synth_stream(10_000_000, 150, 100_000_000, seed=20260417, device=DEV, genome_seed=20260417)
    torch.cuda.synchronize()
    e, T, want, n_adm, by_value, ge = _assert_stream_exact(ds, k, L, 0, 1 << 27)
    assert T[3] == 1_163_397_354
    _check_stream_engine(e, T, want, n_adm, by_value, ge, L, "bench batch")
    e.close()
    del want
    torch.cuda.empty_cache()
    plain = new_engine(k, 1 << 28)
    plain.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)
    rows = ge[L]
    got = _sorted_dump(plain, L, rows[0].numel())
    for a, b in zip(got, rows):
        assert torch.equal(a, b)
    plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# condition 8: the mirror, opt-in
# ---------------------------------------------------------------------------------------------------------------------

def test_mini_trio_child_with_the_prefilter(oracle, trio_reads, tmp_path, monkeypatch, caplog):
    import logging
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_kmers_discovery
    from kmer_denovo_filter_amd.kmer_fasta import read_kmer_fasta_keys
    m = json.load(open(os.path.join(GOLDEN, "example_output_discovery", "giab_discovery.metrics.json")))
    monkeypatch.setenv("KDF_PREFILTER", "1")
    with caplog.at_level(logging.INFO):
        fa, n = _extract_child_kmers_discovery(os.path.join(GIAB, "HG002_child.bam"), None, 31, 3, 4, str(tmp_path))
    assert "two passes" in caplog.text                              # the two-pass count ran, and said what it stored
    assert n == m["child_candidate_kmers"] == 51125
    lo, _ = read_kmer_fasta_keys(fa, 31)
    want = oracle.OracleTable(31).count_reads(trio_reads["child"]).export_ge(3)[0]
    np.testing.assert_array_equal(np.sort(lo), want)


def test_mini_trio_child_long_k_with_the_prefilter(oracle, trio_reads, tmp_path, monkeypatch):
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_kmers_discovery
    from kmer_denovo_filter_amd.kmer_fasta import read_kmer_fasta_keys
    from kmer_denovo_filter_amd.reads import keys_to_kmers
    k = 75
    monkeypatch.setenv("KDF_PREFILTER", "1")
    fa, n = _extract_child_kmers_discovery(os.path.join(GIAB, "HG002_child.bam"), None, k, 3, 4, str(tmp_path))
    want = {c for c, v in oracle.py_count(trio_reads["child"], k).items() if v >= 3}
    got = set(keys_to_kmers(read_kmer_fasta_keys(fa, k)[0], None, k))
    assert n == len(got) == len(want) and got == want
