"""The direct count of ONE stream split over several launches: a small table makes ``direct_insert`` walk the stream in
chunks (each sized to the room left in the table) and double the table in between, so every chunk but the first starts
in the middle of the stream.  Each chunk must still end where the whole stream ends: the last one holds the tile with
the dirty words past ``n_bases``, and no chunk may count a window twice or skip one.

One stream per k of about 300 tiles of short reads with some N, sampled from a small genome with a few substitution
errors (most keys are seen several times, some once), n_bases % 64 == 33, in device buffers of exactly
``kdf_stream_words(n_bases)`` words with the "live" filling of test_gpu_stream_tail.py (mask 0 and random bases at and
past n_bases).  Counted with force_path=1 into an engine of capacity_hint 2^10 under profile(True), once plain and once
behind a prefilter tallied from the same stream with min_count 2.

Truth: ``stream_truth`` (k <= 63) / ``kmer_truth`` (long k) through test_gpu_stream_tail.truth; for the gated run the keys
seen at least twice, with their full counts.  The sieve is hashed, so that is only its model when no key seen once
shares a cell with another key: asserted from ``prefilter_model`` before the GPU is touched.  Witnesses: several stream
launches (profile_read) and a table that grew."""
import numpy as np
import pytest

import prefilter_model as PM
import test_gpu_stream_tail as TL

pytestmark = pytest.mark.gpu

KS = (31, 63, 101)
TILES = 300
LOG2_CELLS = 24
MIN_COUNT = 2
_CASES = {}


def case(k):
    """(stream, truth, truth of the keys seen at least twice) for one k, built once"""
    if k in _CASES:
        return _CASES[k]
    rng = np.random.default_rng(4100 + k)
    genome = TL._rd(rng, 2500, clean=True)
    reads, base = [], 0
    while base < 64 * (TILES - 8):
        L = int(rng.integers(k + 40, k + 250))
        a = int(rng.integers(0, len(genome) - L))
        r = np.array(list(genome[a:a + L]))
        x = rng.random(L)
        r[x < 0.003] = "N"
        sub = (x >= 0.003) & (x < 0.005)
        r[sub] = rng.choice(list("ACGT"), int(sub.sum()))
        reads.append("".join(r))
        base += L + 1
    L = k + 5 + ((33 - base - k - 5) % 64)                        # a last read without N that ends at n - 1
    reads.append(TL._rd(rng, L, clean=True))
    n = base + L
    assert n % 64 == 33 and TILES - 8 < (n + 63) // 64 <= TILES + 4
    s = TL.Stream(f"pieces{k}", reads, n, 4200 + k)
    t = TL.truth(k, s)
    if k <= 63:
        lo, hi, cnt, _ = t
        keep = cnt >= MIN_COUNT
        twice = (lo[keep], hi[keep], cnt[keep], int(cnt[keep].sum()))
        adm, _ = PM.model_np(lo.numpy().view(np.uint64), hi.numpy().view(np.uint64), cnt.numpy(), k, LOG2_CELLS, MIN_COUNT)
        assert np.array_equal(adm, keep.numpy()), "a key seen once shares its sieve cell: the model is not 'seen twice'"
        n_once = int((~keep).sum())
    else:
        d = {key: c for key, c in t[0].items() if c >= MIN_COUNT}
        twice = (d, sum(d.values()))
        assert PM.model(t[0], k, LOG2_CELLS, MIN_COUNT)[0] == d, "a key seen once shares its sieve cell: the model is not 'seen twice'"
        n_once = len(t[0]) - len(d)
    n_twice = twice[0].numel() if k <= 63 else len(twice[0])
    assert n_once >= 20 and n_twice >= 1500                      # the gate drops something and what it keeps outgrows 2^10 slots
    _CASES[k] = (s, t, twice)
    return _CASES[k]


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("k", KS)
def test_direct_count_in_several_launches(k, gated):
    s, t, twice = case(k)
    d = TL.dev(s, "live")
    with TL.new_engine(k, hint=1 << 10, force_path=1) as e:
        log2cap0 = e.get_stat("log2cap")
        if gated:
            e.prefilter_begin(MIN_COUNT, LOG2_CELLS)
            e.prefilter_add_dev(d[0].data_ptr(), d[1].data_ptr(), s.n)
            e.prefilter_arm()
        e.profile(True)
        TL.count_dev(e, d, s.n)
        assert e.last_count_path() == "direct"
        ms, launches, positions = e.profile_read()
        print(f"k={k} gated={gated}: {launches} launches, {positions} positions, log2cap {log2cap0} -> {e.get_stat('log2cap')}")
        assert launches >= 3, f"{launches} stream launches: the count was not split"
        why = TL.table_diff(e, twice if gated else t)             # the dump, then stats() distinct and windows
        assert why is None, why
        assert e.get_stat("log2cap") > log2cap0, "the table did not grow"
