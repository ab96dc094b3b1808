"""Merging counting sieves on the GPU (include/kdf.h "two-pass counting": several ranks; csrc/kdf_prefilter.h
``kdf_pf_merge_kernel``).

1. the kernel against ``prefilter_merge_model`` (numpy), word for word: garbage segments, odd starts and lengths,
   1 to 64 segments, sum and replace;
2. the split-stream property: the merged sieves of P engines that tallied disjoint read sets ARE the sieve of one
   engine that tallied all reads;
3. end to end on one GPU: shard engines gated by the merged sieve, their dumps summed, equal a single-engine two-pass
   count bit for bit;
4. state / argument errors and stats.
Every test states equalities; none measures."""
import numpy as np
import pytest

import prefilter_merge_model as MM

pytestmark = pytest.mark.gpu

S = 16
N_WORDS = 1 << (S - 4)
SLICES = ((0, 4096), (1, 3), (1, 4094), (4095, 1), (7, 0), (2, 1))


def new_engine(k, hint=1 << 16):
    import torch
    from kmer_denovo_filter_amd import KmerEngine
    torch.cuda.empty_cache()
    return KmerEngine(k, capacity_hint=hint)


def shard_streams(k, parts, n_reads=3000, genome_len=60_000):
    """`parts` disjoint read sets over ONE small genome (about 7x coverage in all: many cells reach 2 and 3)"""
    from kmer_denovo_filter_amd.synth import synth_stream
    import torch
    out = [synth_stream(n_reads // parts, read_len=150, genome_len=genome_len, seed=100 * k + p, genome_seed=k, sub_rate=0.01)
           for p in range(parts)]
    torch.cuda.synchronize()
    return out


def tally(e, ds):
    e.prefilter_add_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)


def count(e, ds):
    e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), ds.n_bases)


def err_code(fn):
    from kmer_denovo_filter_amd._native import KdfError
    with pytest.raises(KdfError) as ei:
        fn()
    return ei.value.code


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the model
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tallied():
    """(engine k = 31 with a tallied sieve of 4096 words, that sieve)"""
    e = new_engine(31)
    e.prefilter_begin(2, S)
    for ds in shard_streams(31, 1, n_reads=300, genome_len=20_000):
        tally(e, ds)
    base = e.prefilter_export()
    assert len(base) == N_WORDS == e.prefilter_words()
    f = MM.fill(base)
    assert MM.valid_codes(base) and min(f) > 0 and f == e.prefilter_fill()    # cells of every value: the sieve is not empty
    yield e, base
    e.close()


def segments(nseg, n, seed, dense):
    """dense: uniformly random words (bit 3 set, non-thermometer codes, every cell saturates under many segments);
    sparse: few planes set per segment, so that sums below 3 survive 64 segments too"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nseg):
        w = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        if not dense:
            for _ in range(2 + int(np.log2(nseg))):
                w &= rng.integers(0, 1 << 64, n, dtype=np.uint64)
            w |= rng.integers(0, 1 << 64, n, dtype=np.uint64) & np.uint64(0x8888888888888888)   # bit 3 carries nothing
        out.append(w)
    return out


@pytest.mark.parametrize("dense", (True, False))
@pytest.mark.parametrize("replace", (False, True))
@pytest.mark.parametrize("nseg", (1, 2, 3, 64))
def test_kernel_against_model(tallied, nseg, replace, dense):
    e, base = tallied
    for first, n in SLICES:
        e.prefilter_merge([base], 0, replace=True)                 # back to the tallied sieve (valid codes: replace is the identity)
        np.testing.assert_array_equal(e.prefilter_export(), base)
        segs = segments(nseg, n, 1000 * nseg + 10 * first + n, dense)
        expect = MM.merge_slice(base, first, segs, replace)
        e.prefilter_merge(segs, first, replace=replace)
        got = e.prefilter_export()
        np.testing.assert_array_equal(got[first:first + n], expect[first:first + n], err_msg=f"slice ({first}, {n})")
        np.testing.assert_array_equal(got, expect, err_msg=f"words outside ({first}, {n}) changed")
        assert MM.valid_codes(got)
        np.testing.assert_array_equal(e.prefilter_export(first, n), expect[first:first + n])
        assert e.prefilter_fill() == MM.fill(expect)
    if not dense and not replace:
        assert 0 < MM.fill(expect)[1] + MM.fill(expect)[2]          # (the sparse case did keep sums below 3)


def test_device_segments_at_any_word(tallied):
    """the device form: segments that start at odd words of their buffers, whatever the parity of the slice's start"""
    import torch
    e, base = tallied
    rng = np.random.default_rng(5)
    for first, n, shift in ((0, 4096, 1), (1, 4094, 0), (1, 4094, 1), (2, 1001, 1), (3, 1000, 0)):
        e.prefilter_merge([base], 0, replace=True)
        segs = [rng.integers(0, 1 << 64, n, dtype=np.uint64) & rng.integers(0, 1 << 64, n, dtype=np.uint64) for _ in range(3)]
        bufs = [torch.zeros(n + 2, dtype=torch.int64, device="cuda") for _ in segs]
        for b, s in zip(bufs, segs):
            b[shift:shift + n] = torch.from_numpy(s.view(np.int64)).cuda()
        torch.cuda.synchronize()
        e.prefilter_merge_dev([b.data_ptr() + 8 * shift for b in bufs], first, n)
        e.synchronize()
        out = torch.empty(N_WORDS, dtype=torch.int64, device="cuda")
        e.prefilter_export_dev(out.data_ptr(), 0, N_WORDS)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), MM.merge_slice(base, first, segs, False))


# ---------------------------------------------------------------------------------------------------------------------
# 2. split streams
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (31, 63, 101))
@pytest.mark.parametrize("parts", (2, 3))
def test_merged_sieves_of_split_reads_are_the_sieve_of_all_reads(k, parts):
    import torch
    s = 18
    shards = shard_streams(k, parts)
    whole = new_engine(k)
    whole.prefilter_begin(3, s)
    engines = []
    for ds in shards:
        tally(whole, ds)
        e = new_engine(k)
        e.prefilter_begin(3, s)
        tally(e, ds)
        engines.append(e)
    expect = whole.prefilter_export()
    f = MM.fill(expect)
    assert f[2] > 1000 and f[3] > 1000 and f == whole.prefilter_fill()
    n = engines[0].prefilter_words()
    assert n == 1 << (s - 4)
    own = engines[0].prefilter_export()
    assert not np.array_equal(own, expect)                          # a shard's own tallies under-count
    # device to device: the other engines' exports, merged into engine 0 in ONE call
    bufs = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in engines[1:]]
    for b, e in zip(bufs, engines[1:]):
        e.prefilter_export_dev(b.data_ptr(), 0, n)
    windows = engines[0].get_stat("prefilter_windows")
    engines[0].prefilter_merge_dev([b.data_ptr() for b in bufs], 0, n)
    got = engines[0].prefilter_export()
    np.testing.assert_array_equal(got, expect)
    assert engines[0].prefilter_fill() == whole.prefilter_fill()
    assert engines[0].get_stat("prefilter_windows") == windows      # "windows this engine tallied"
    assert sum(e.get_stat("prefilter_windows") for e in engines) == whole.get_stat("prefilter_windows")
    # the model agrees with the kernel on real sieves too
    np.testing.assert_array_equal(MM.merge(own, [b.cpu().numpy().view(np.uint64) for b in bufs]), expect)
    for e in engines + [whole]:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. end to end on one GPU
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,L", ((31, 3), (101, 2)))
def test_gated_shards_sum_to_the_single_engine_two_pass_count(k, L):
    s, parts = 18, 3
    shards = shard_streams(k, parts)
    engines = []
    for ds in shards:
        e = new_engine(k)
        e.prefilter_begin(L, s)
        tally(e, ds)
        engines.append(e)
    exports = [e.prefilter_export() for e in engines]
    for i, e in enumerate(engines):                                  # every shard engine ends with the merged sieve
        e.prefilter_merge([x for j, x in enumerate(exports) if j != i])
    for e in engines[1:]:
        np.testing.assert_array_equal(e.prefilter_export(), engines[0].prefilter_export())
    total = new_engine(k)
    for e, ds in zip(engines, shards):
        e.prefilter_arm()
        count(e, ds)
        lo, hi, cnt = e.export_ge(0)
        total.add_pairs(lo, hi, cnt)
    single = new_engine(k)
    single.prefilter_begin(L, s)
    for ds in shards:
        tally(single, ds)
    single.prefilter_arm()
    plain = new_engine(k)
    for ds in shards:
        count(single, ds)
        count(plain, ds)
    for m, ref in ((0, single), (L, plain), (L + 2, plain)):
        got, exp = total.export_ge(m), ref.export_ge(m)
        assert len(got[0]) == len(exp[0]) > 0
        for a, b in zip(got, exp):
            if a is None or b is None:
                assert a is None and b is None
            else:
                np.testing.assert_array_equal(a, b, err_msg=f"export_ge({m})")
    assert len(single.export_ge(0)[0]) < len(plain.export_ge(0)[0])  # the gate did keep keys out
    for e in engines + [total, single, plain]:
        e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. errors and stats
# ---------------------------------------------------------------------------------------------------------------------

def test_state_and_argument_errors():
    import torch
    from kmer_denovo_filter_amd import _native
    STATE, INVALID = _native.KDF_ERR_STATE, _native.KDF_ERR_INVALID
    e = new_engine(31)
    seg = np.full(8, 0x7777777777777777, dtype=np.uint64)
    dseg = torch.from_numpy(seg.view(np.int64)).cuda()
    # off
    assert err_code(lambda: e.prefilter_merge([seg])) == STATE
    assert err_code(lambda: e.prefilter_merge_dev([dseg.data_ptr()], 0, 8)) == STATE
    assert err_code(lambda: e.prefilter_export()) == STATE
    assert err_code(lambda: e.prefilter_export(0, 8)) == STATE
    assert err_code(lambda: e.prefilter_export_dev(dseg.data_ptr(), 0, 8)) == STATE
    assert err_code(lambda: e.prefilter_words()) == STATE
    # tallying: argument errors write nothing
    e.prefilter_begin(2, S)
    for ds in shard_streams(31, 1, n_reads=200, genome_len=20_000):
        tally(e, ds)
    before = e.prefilter_export()
    assert err_code(lambda: e.prefilter_merge([seg], N_WORDS - 7)) == INVALID         # reaches one word past the end
    assert err_code(lambda: e.prefilter_merge([seg], N_WORDS + 1)) == INVALID
    assert err_code(lambda: e.prefilter_merge([seg], (1 << 64) - 4)) == INVALID       # first + n wraps
    assert err_code(lambda: e.prefilter_export(N_WORDS - 7, 8)) == INVALID
    assert err_code(lambda: e.prefilter_merge_dev([], 0, 8)) == INVALID               # nseg 0
    assert err_code(lambda: e.prefilter_merge_dev([dseg.data_ptr()] * 65, 0, 8)) == INVALID
    assert err_code(lambda: e.prefilter_merge_dev([dseg.data_ptr(), 0], 0, 8)) == INVALID   # a NULL segment
    np.testing.assert_array_equal(e.prefilter_export(), before)
    e.prefilter_merge([seg[:0]], 7)                                                   # n_words == 0: OK, nothing written
    e.prefilter_merge_dev([dseg.data_ptr()], N_WORDS, 0)
    assert len(e.prefilter_export(N_WORDS, 0)) == 0
    np.testing.assert_array_equal(e.prefilter_export(), before)
    # armed: export works, merge does not
    e.prefilter_arm()
    np.testing.assert_array_equal(e.prefilter_export(), before)
    assert err_code(lambda: e.prefilter_merge([seg])) == STATE
    assert err_code(lambda: e.prefilter_merge_dev([dseg.data_ptr()], 0, 8)) == STATE
    np.testing.assert_array_equal(e.prefilter_export(), before)
    e.prefilter_drop()
    assert err_code(lambda: e.prefilter_export()) == STATE
    e.close()


def test_stats():
    e = new_engine(31)
    e.profile(True)
    e.prefilter_begin(3, S)
    for ds in shard_streams(31, 1, n_reads=200, genome_len=20_000):
        tally(e, ds)
    windows = e.get_stat("prefilter_windows")
    assert windows > 0 and e.get_stat("prefilter_merged_words") == 0 and e.get_stat("prefilter_merge_passes") == 0
    seg = np.full(100, 0x1111111111111111, dtype=np.uint64)
    e.prefilter_merge([seg, seg], 5)
    e.prefilter_merge([seg[:3]], 0, replace=True)
    assert e.get_stat("prefilter_windows") == windows
    assert e.get_stat("prefilter_merged_words") == 103
    assert e.get_stat("prefilter_merge_passes") == 2 and e.get_stat("prefilter_merge_us") >= 0
    e.prefilter_drop()
    e.prefilter_begin(3, S)
    assert e.get_stat("prefilter_merged_words") == 0                # counted since kdf_prefilter_begin
    e.close()
