"""What ``kdf_profile`` counts: one fixed sequence of calls on one engine and two spools, and the integers
``profile_read``, ``profile_stages`` and every ``*_passes`` stat must then return.  The times are only required to be
there (``>= 0``), to read the same twice, and to be 0 again after ``profile(False)``.

The expected integers, from the engine's own rules (k = 31, streams A and B of tA and tB tiles of 64 positions):

    launches   4   one per direct count (a table of 2^17 slots takes a stream this small in one launch: the direct path
                   cuts a stream where the table could pass load 0.8), one for the partition pass of the binned count
                   (its flush is timed but brings no positions of its own), one for the sieve count --if
    positions  64 * (tA + tB + tA + tB): direct A, direct B, binned A, sieve B -- whole tiles
    stage passes 1 the one partition pass; the flush only adds to stage 3's time
    prefilter 2, prefilter_merge 2, depth 2 (a per-read and a per-window call), hits 2 (a call that finds hits records
    two timed groups and still counts once), sketch 1, histo 2; spool: append 4 / offsets 0 without reads, 2 / 2 with
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 31
PASSES = {"prefilter_passes": 2, "prefilter_merge_passes": 2, "depth_passes": 2, "hits_passes": 2, "sketch_passes": 1,
          "histo_passes": 2}
TIMES = tuple(n.replace("_passes", "_us") for n in PASSES)


def _reads(rng, genome, n, length=150):
    out = []
    for _ in range(n):
        a = int(rng.integers(0, len(genome) - length))
        out.append("".join("ACGT"[c] for c in genome[a:a + length]))
    return out


def _stream(reads):
    from kmer_denovo_filter_amd import ReadStream
    return ReadStream.from_strings(reads)


def _work(e, A, B, other, keys):
    """the sequence of the docstring; the engine ends in insert mode, cleared, prefilter and sketch dropped"""
    e.reserve(1 << 16)                                               # (load_filter below sizes the table for its keys: back to
    e.set_option("force_path", 1)                                    # 2^17 slots, where a direct count of A or B is ONE launch)
    e.count(A)
    e.count(B)                                                       # two direct counts
    e.set_option("force_path", 2)
    e.count(A)                                                       # one partition pass, pending
    e.flush()                                                        # ... applied
    e.set_option("force_path", 0)
    e.read_depth(A, 1)
    e.window_counts(B)                                               # two depth passes
    rows = e.read_hits(A)
    none = e.read_hits(other)                                        # two hit reductions: with hits, without
    e.sketch_begin(10)
    e.sketch_add(A)
    e.sketch_drop()
    e.histogram(10)
    e.histogram(10)
    e.load_filter(keys[0], keys[1])
    e.count_filtered(B)                                              # the sieve kernel
    path = e.get_stat("last_count_path")
    e.clear()
    e.prefilter_begin(2, 16)
    e.prefilter_add(A)
    e.prefilter_add(B)
    seg = np.ones(64, np.uint64)
    e.prefilter_merge([seg], first=0)
    e.prefilter_merge([seg, seg], first=64)
    e.prefilter_drop()
    return rows, none, path


def _read_all(e):
    ms, launches, positions = e.profile_read()
    stage_ms, passes = e.profile_stages()
    stats = {n: e.get_stat(n) for n in tuple(PASSES) + TIMES}
    return ms, launches, positions, stage_ms, passes, stats


def test_engine_profile_counts_this_sequence():
    from kmer_denovo_filter_amd import KmerEngine
    rng = np.random.default_rng(11)
    genome = rng.integers(0, 4, 4000)
    A, B = _stream(_reads(rng, genome, 20)), _stream(_reads(rng, genome, 33))
    other = _stream(_reads(rng, rng.integers(0, 4, 3000), 10))      # another genome: none of its 31-mers is stored
    assert 2000 < A.n_bases < B.n_bases < 6000 and A.n_bases % 64 and B.n_bases % 64
    tA, tB = (A.n_bases + 63) // 64, (B.n_bases + 63) // 64
    with KmerEngine(K, capacity_hint=1 << 16) as e:
        e.count(A)
        lo, hi, _ = e.export_ge(1)
        e.clear()
        keys = (lo[::2].copy(), hi[::2].copy())
        assert e.get_stat("log2cap") > e.get_stat("bucket_bits")    # (the binned pipeline takes this table)

        # profiling off: nothing is recorded
        _work(e, A, B, other, keys)
        e.clear()
        got = _read_all(e)
        assert got[:3] == (0.0, 0, 0) and got[3] == [0.0] * 4 and got[4] == 0 and not any(got[5].values()), got

        e.profile(True)
        binned0 = e.get_stat("binned_passes")
        rows, none, path = _work(e, A, B, other, keys)
        assert rows[:, 0].sum() > 0 and none[:, 0].sum() == 0 and path == 3
        assert e.get_stat("binned_passes") == binned0 + 1
        ms, launches, positions, stage_ms, passes, stats = first = _read_all(e)
        print(f"launches={launches} positions={positions} stage_passes={passes} ms={ms:.4f} stage_ms={stage_ms} {stats}", flush=True)
        assert launches == 4
        assert positions == 64 * (tA + tB + tA + tB)
        assert passes == 1
        assert {n: stats[n] for n in PASSES} == PASSES
        assert ms > 0 and all(m >= 0 for m in stage_ms)
        assert all(stats[n] >= 0 for n in TIMES)
        assert _read_all(e) == first                                # collecting is idempotent

        e.profile(False)
        got = _read_all(e)
        assert got[:3] == (0.0, 0, 0) and got[3] == [0.0] * 4 and got[4] == 0 and not any(got[5].values()), got
        _work(e, A, B, other, keys)
        got = _read_all(e)
        assert got[:3] == (0.0, 0, 0) and got[3] == [0.0] * 4 and got[4] == 0 and not any(got[5].values()), got


def _spool_stats(sp):
    return {n: sp.stat(n) for n in ("append_passes", "offsets_passes", "append_us", "offsets_us")}


def test_spool_profile_counts_appends():
    """A spool's two timers: appends and offset rewrites.  Its totals are never reset: turning the option off stops the
    recording and keeps what was recorded."""
    from kmer_denovo_filter_amd.spool import ReadSpool
    rng = np.random.default_rng(12)
    genome = rng.integers(0, 4, 4000)
    batches = [_stream(_reads(rng, genome, n)) for n in (7, 20, 1, 12)]
    with ReadSpool(0, 1 << 28, 0) as plain, ReadSpool(0, 1 << 28, 0) as keeps:
        for sp in (plain, keeps):
            sp.set_option("segment_positions", 1 << 12)
        plain.append(batches[0], keep_reads=False)                  # off: not recorded
        assert _spool_stats(plain) == {"append_passes": 0, "offsets_passes": 0, "append_us": 0, "offsets_us": 0}
        plain.clear()
        plain.set_option("profile", 1)
        keeps.set_option("profile", 1)
        for b in batches:
            plain.append(b, keep_reads=False)
        for b in batches[:2]:
            keeps.append(b, keep_reads=True)
        assert plain.stat("keeps_reads") == 0 and keeps.stat("keeps_reads") == 1
        p, q = _spool_stats(plain), _spool_stats(keeps)
        print(f"plain={p} keeps={q}", flush=True)
        assert (p["append_passes"], p["offsets_passes"]) == (4, 0) and p["append_us"] >= 0 and p["offsets_us"] == 0
        assert (q["append_passes"], q["offsets_passes"]) == (2, 2) and q["append_us"] >= 0 and q["offsets_us"] >= 0
        assert _spool_stats(plain) == p and _spool_stats(keeps) == q
        for sp, want in ((plain, p), (keeps, q)):
            sp.set_option("profile", 0)
            assert _spool_stats(sp) == want
        plain.append(batches[0], keep_reads=False)
        keeps.append(batches[2], keep_reads=True)
        assert _spool_stats(plain) == p and _spool_stats(keeps) == q
