"""The pipelined piece sort (``kb_piecesort_pipe_kernel``, csrc/kdf_binned.h) at the edges of its pipeline.  A piece is five
iterations in the kernel: offsets requested, run table, gather, histogram + scan one piece ahead, rank + scatter +
write-out; three barriers per iteration.  Every case counts the same stream(s) three times and compares the sorted
``(key, count)`` dumps entry by entry, and ``stats()``:

* the binned path with the pipelined kernel (``force_path`` 2);
* the binned path with the one-piece-per-workgroup kernel (``debug_flags`` 64: ``kb_sort_piece``, the independent form);
* the direct path (``force_path`` 1).

Geometry, read back through ``get_stat`` where a case depends on it (kb_make_plan): a table of at most 2^8 buckets has
no coarse bits, and a fresh engine (one window per position assumed) then makes every slab a group -- a piece per slab;
2^9 .. 2^16 buckets: 8 fine bits (``nf`` 256), beyond: 9 (``nf`` 512).  A slab is 16 384 stream positions (k = 31) or
8 192 (k = 63); a workgroup per CU walks pairs (group, coarse bin) j0, j0 + nj, ...

* ``test_fresh_engine_piece_per_slab``: ~2 M positions, first pass of a fresh engine, no coarse bits: one piece per slab
  (125 / 249 pieces, nearly full), spread over the workgroups -- most take one piece or none.  (A group of one slab
  exists only without coarse bits, so these pieces are whole slabs; tiny pieces by the hundred come from the big table
  below, deep walks from the second pass.)
* ``test_second_pass_large_groups``: the same engine after a flush, now with the measured density, counts 45 000 or
  130 000 reads into a table with coarse bits: groups of several slabs, nearly full pieces, 400 .. 2 500 pairs over
  the workgroups: 1 .. 5 and more pieces each, with fill and drain.
* ``test_fewer_slabs_than_stages``: 1, 2 and 3 slabs.
* ``test_many_empty_coarse_bins``: a few thousand windows of ~40 distinct keys into a table with 2^8 and more coarse
  bins and 9 fine bits: empty pairs inside every workgroup's walk, pieces of a few dozen entries.
* ``test_short_pieces_every_parity``: two tiny passes without a flush between them, each one piece of fewer than 1 024
  entries; the first has an even or odd number of windows, so the second starts at an even or odd ring position, and
  has an even or odd length itself (k = 63: the hi words of an odd piece start on an odd word).
* ``test_short_pieces_512_fine_bins``: ~200 000 positions into the big table: hundreds of pieces of a few hundred
  entries, of both parities, one behind the other in the ring.
* ``test_skewed_pairs_overflow``: a third of the reads are one homopolymer: its coarse bin holds several pieces per
  group -- the first by the pipelined kernel, the others by ``kb_piecesort_more_kernel`` after it.

The order of the entries inside a fine run is unspecified and nothing here depends on it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [31, 63]
SMALL, LARGE = 1 << 17, 1 << 21
BIG = {31: 1 << 29, 63: 1 << 28}                                  # 2^17 buckets and more: 9 fine bits
SLAB = {31: 16384, 63: 8192}
MODES = ("pipe", "one_piece", "direct")
ACGT = np.frombuffer(b"ACGT", np.uint8)


@functools.lru_cache(maxsize=None)
def _synth(n_reads, genome_len, seed):
    """a device stream of 150 bp reads without substitutions (few distinct keys: no table grows), some N"""
    import torch
    from kmer_denovo_filter_amd.synth import synth_stream
    ds = synth_stream(n_reads, 150, genome_len, seed=seed, device="cuda:0", sub_rate=0.0, n_rate=0.001)
    torch.cuda.synchronize()
    return ds


@functools.lru_cache(maxsize=None)
def _strings(reads):
    from kmer_denovo_filter_amd import ReadStream
    return ReadStream.from_strings(list(reads))


def _reads(seed, n, genome_len=30_000, length=150, homopolymer_every=0):
    rng = np.random.default_rng(seed)
    genome = ACGT[rng.integers(0, 4, genome_len)]
    out = []
    for i in range(n):
        a = int(rng.integers(0, genome_len - length + 1))
        out.append(b"A" * length if homopolymer_every and i % homopolymer_every == 0 else genome[a:a + length].tobytes())
    return tuple(out)


def _count(e, s):
    if hasattr(s, "read_len"):                                    # synth.DeviceStream
        e.count_dev(s.packed.data_ptr(), s.invalid.data_ptr(), s.n_bases)
    else:
        e.count(s)


def _run(k, hint, mode, passes, flush_between):
    """dump, stats and (c1, c2) per pass of one engine that counts `passes` one after the other"""
    from kmer_denovo_filter_amd import KmerEngine
    with KmerEngine(k, capacity_hint=hint) as e:
        e.set_option("force_path", 1 if mode == "direct" else 2)
        if mode == "one_piece":
            e.set_option("debug_flags", 64)
        geo = []
        for i, s in enumerate(passes):
            if i and flush_between:
                e.flush()
            _count(e, s)
            assert e.last_count_path() == ("direct" if mode == "direct" else "binned")
            if mode != "direct":
                geo.append((e.get_stat("c1"), e.get_stat("c2")))
        if mode != "direct" and not flush_between:
            assert e.get_stat("pending_passes") == len(passes)
        lo, hi, cnt = e.export_ge(0)
        return (lo, hi, cnt), e.stats(), geo


def _three_ways(k, hint, passes, flush_between=True):
    """the three runs agree; returns the pipelined run's stats and geometry"""
    got = {m: _run(k, hint, m, passes, flush_between) for m in MODES}
    (lo, hi, cnt), stats, geo = got["pipe"]
    assert len(lo) > 0 and stats[1] == len(lo) and stats[2] == int(cnt.astype(np.uint64).sum())
    for m in MODES[1:]:
        (l2, h2, c2), st2, g2 = got[m]
        print(f"k={k} {m}: {len(l2)} keys, stats {st2}, geometry {g2} (pipelined: {len(lo)} keys, {stats}, {geo})")
        np.testing.assert_array_equal(l2, lo, err_msg=m)
        np.testing.assert_array_equal(c2, cnt, err_msg=m)
        if k > 32:
            np.testing.assert_array_equal(h2, hi, err_msg=m)
        assert st2 == stats, (m, st2, stats)
    assert got["one_piece"][2] == geo
    return stats, geo


@pytest.mark.parametrize("k", KS)
def test_fresh_engine_piece_per_slab(k):
    s = _synth(13_500, 30_000, 11)                                # 2.04 M positions
    assert s.n_bases > 100 * SLAB[k] and s.n_bases % SLAB[k] != 0
    stats, geo = _three_ways(k, SMALL, [s])
    assert geo[0][0] == 0 and geo[0][1] <= 8                       # no coarse bits: group = 1 slab on a fresh engine


@pytest.mark.parametrize("reads", [45_000, 130_000])
@pytest.mark.parametrize("k", KS)
def test_second_pass_large_groups(k, reads):
    first, second = _synth(13_500, 30_000, 11), _synth(reads, 200_000, 12)
    assert first.n_bases >= 1 << 20                                # enough for the engine to take its density from
    stats, geo = _three_ways(k, LARGE, [first, second])
    assert geo[1][0] >= 1 and geo[1][1] == 8                       # coarse bins: groups of several slabs; nf = 256


@pytest.mark.parametrize("slabs", [1, 2, 3])
@pytest.mark.parametrize("k", KS)
def test_fewer_slabs_than_stages(k, slabs):
    n = int((slabs - 0.4) * SLAB[k]) // 151
    s = _strings(_reads(20 + slabs, n))
    assert -(-s.n_bases // SLAB[k]) == slabs
    stats, geo = _three_ways(k, SMALL, [s])
    assert geo[0][0] == 0


@pytest.mark.parametrize("k", KS)
def test_many_empty_coarse_bins(k):
    reads = _reads(31, 60, genome_len=k + 40, length=k + 40)       # 60 copies of one short sequence: 41 distinct windows
    stats, geo = _three_ways(k, BIG[k], [_strings(reads)])
    assert geo[0][0] >= 8 and geo[0][1] == 9                       # 256 coarse bins and more, nf = 512
    assert stats[1] <= 41 and 2000 <= stats[2] <= 4000             # far fewer keys than bins: most pairs are empty


@pytest.mark.parametrize("second_odd", [0, 1], ids=["even-length", "odd-length"])
@pytest.mark.parametrize("first_odd", [0, 1], ids=["even-start", "odd-start"])
@pytest.mark.parametrize("k", KS)
def test_short_pieces_every_parity(k, first_odd, second_odd):
    def tiny(seed, odd):                                          # no N: 5 (150 - k + 1) windows, one more with a read of k bases
        return _reads(seed, 5) + (_reads(seed + 1, 1, length=k) if odd else ())
    a, b = tiny(40, first_odd), tiny(42, second_odd)
    wa, wb = 5 * (150 - k + 1) + first_odd, 5 * (150 - k + 1) + second_odd
    assert wa % 2 == first_odd and wb % 2 == second_odd and wb < 1024
    stats, geo = _three_ways(k, SMALL, [_strings(a), _strings(b)], flush_between=False)
    assert geo[1][0] == 0                                          # one bin: each pass is one piece, the second behind the first
    assert stats[2] == wa + wb


@pytest.mark.parametrize("k", KS)
def test_short_pieces_512_fine_bins(k):
    s = _strings(_reads(50, 1300))                                # 196 300 positions
    stats, geo = _three_ways(k, BIG[k], [s])
    assert geo[0][1] == 9
    assert stats[2] // (1 << geo[0][0]) < 1024                     # the average piece


@pytest.mark.parametrize("k", KS)
def test_skewed_pairs_overflow(k):
    s = _strings(_reads(60, 2400, homopolymer_every=3))           # 362 400 positions, a third of them one key
    stats, geo = _three_ways(k, 1 << 24, [s])
    c1 = geo[0][0]
    assert c1 >= 2
    # the homopolymer's windows alone are more than a piece: a fresh engine's group is 0.98 * 2^c1 slabs (or the whole
    # stream), a third of its reads are that key, (150 - k + 1) windows per 151 positions, all in one coarse bin, and a
    # piece holds as many entries as a slab has positions
    group = min(int(0.98 * (1 << c1)), s.n_bases // SLAB[k])
    assert group * (150 - k + 1) / (3 * 151) > 1.5
