"""``kdf_destroy`` with everything alive: every buffer of an engine frees itself when the engine goes (csrc/kdf_devbuf.h,
DESIGN.md 4), so three engines are destroyed in the middle of their work -- no flush, no drop, no synchronise from the
caller -- and a fresh engine in the same process must still count right.

One stream of 64 reads of 150 bp (a 3 kb genome, a few N, some lower case), split 48 + 16.  Alive at the destroy:

* engine 1: a partitioned pass pending in the ring and a small batch in the pending stream (k <= 63: ``l1_direct_positions``
  4096 sends the 48 reads to the ring and the 16 behind them to the pending stream; witnessed by ``pending_passes`` /
  ``pending_positions``), both upload slots filled and not consumed, a sketch that was fed, and the per-read scratch of a
  read-hits and a window-counts call.  k = 65 has no binned pipeline: its counts go straight to the table, the rest is
  the same.
* engine 2: a prefilter left tallying.
* engine 3: a loaded filter with a filtered count, so the sieve exists (k = 65: option ``long_sieve``); k <= 63 counts
  again with ``sieve_bins`` 1, so the bin-major sieve exists too (witnessed by ``last_count_path`` 5).

The assertion is that teardown of live state neither hangs nor faults nor disturbs the next engine: its dump with
``min_count`` 1 equals ``kmer_truth.count_truth`` key by key.  Free device memory is not looked at (the device is shared)."""
import functools

import numpy as np
import pytest

import kmer_truth as KT
from test_gpu_parity_basic import rand_reads

pytestmark = pytest.mark.gpu

HINT = 1 << 17                       # 2^18 slots: 32 / 64 buckets, so the binned pipeline is eligible


@functools.lru_cache(maxsize=None)
def _reads():
    rng = np.random.default_rng(20)
    return tuple(rand_reads(rng, 64, 150, 150, n_frac=0.002, genome=rng.integers(0, 4, 3000).astype(np.uint8)))


@functools.lru_cache(maxsize=None)
def _truth(k):
    return KT.count_truth(list(_reads()), k)


def _keys(k, ints):
    """the engine's key arguments for a list of canonical keys"""
    if k > 63:
        return (KT.rows(ints, (2 * k + 63) // 64),)
    lo, hi = KT.lohi(ints)
    return (lo, hi)


def _dump(e, k):
    keys, hi, cnt = e.export_ge(1)
    if k > 63:
        ints = [KT.int_of_row(r) for r in keys]
    else:
        ints = [int(l) | (int(h) << 64) for l, h in zip(keys, hi)]
    assert len(set(ints)) == len(ints)
    return dict(zip(ints, (int(c) for c in cnt)))


@pytest.mark.parametrize("k", [31, 63, 65])
def test_destroy_with_everything_alive(k):
    from kmer_denovo_filter_amd import KmerEngine, ReadStream
    reads = list(_reads())
    whole, big, small = ReadStream.from_strings(reads), ReadStream.from_strings(reads[:48]), ReadStream.from_strings(reads[48:])
    assert whole.n_bases == 64 * 151 and big.n_bases >= 4096 > small.n_bases       # (a read and its separator: 151 positions)
    truth = _truth(k)
    long = k > 63

    # ---- engine 1: pending passes, pending stream, upload slots, sketch, per-read scratch
    e1 = KmerEngine(k, capacity_hint=HINT)
    if not long:
        e1.set_option("binned_min_positions", 1)
        e1.set_option("l1_direct_positions", 4096)
    e1.sketch_begin(10)
    e1.count(big)
    rows = e1.read_hits(whole)                                   # (flushes: the table holds the 48 reads)
    assert int(rows[:48, 0].sum()) > 0
    counts = e1.window_counts(whole)
    assert int(counts.max()) >= 1
    e1.count(big)
    e1.count(small)
    if not long:
        assert e1.get_stat("pending_passes") == 1                # the 48 reads, partitioned and not applied
        assert e1.get_stat("pending_positions") >= whole.n_bases  # ... and the 16 behind them in the pending stream (the pass alone: 7296)
    e1.upload_async(0, small)
    e1.upload_async(1, big)
    e1.sketch_add(whole)

    # ---- engine 2: a prefilter left tallying
    e2 = KmerEngine(k, capacity_hint=HINT)
    e2.prefilter_begin(2, 16)
    e2.prefilter_add(whole)
    assert e2.get_stat("prefilter_state") == 1

    # ---- engine 3: a filter, its sieve(s) and a filtered count
    e3 = KmerEngine(k, capacity_hint=HINT)
    if long:
        e3.set_option("long_sieve", 1)
    e3.load_filter(*_keys(k, sorted(truth)[::2]))
    e3.count_filtered(whole)
    assert e3.get_stat("last_count_path") == 3                   # through the sieve
    if not long:
        e3.set_option("sieve_bins", 1)
        e3.count_filtered(whole)
        assert e3.get_stat("last_count_path") == 5               # through the bin-major sieve

    # ---- destroyed as they are
    for e in (e1, e2, e3):
        e.close()

    # ---- the next engine of the process
    with KmerEngine(k, capacity_hint=HINT) as e:
        e.count(whole)
        got = _dump(e, k)
    assert len(got) == len(truth)
    for key, c in truth.items():
        assert got.get(key) == c, f"k={k}: key {key:#x}"
