"""CPU tests of the lifetime test's own parts: the model (tests/engine_model.py) against independent truths on
straight scripts, and the generator (tests/engine_ops.py): deterministic, and every committed (seed, family) covers the
required call pairs and model-side preconditions -- so that the coverage the GPU test relies on cannot be missing for a
reason that lies in the generator."""
import numpy as np
import pytest
import torch

import depth_truth as DT
import engine_model as EM
import engine_ops as EO
import kmer_truth as KT
import prefilter_model as PM
import stream_truth as ST
from test_gpu_engine_lifetime import N_OPS, SEEDS

SAT = EM.SAT


def reads_for(k, seed, n=120):
    return KT.random_reads(np.random.default_rng(seed), k, n, max_len=max(200, k + 60))


def oracle_table(oracle, k, reads):
    lo, hi, cnt = oracle.OracleTable(k, 1 << 12).count_reads(reads).export_ge(0)
    return {int(a) | (int(b) << 64): int(c) for a, b, c in zip(lo.tolist(), hi.tolist(), cnt.tolist())}


@pytest.mark.parametrize("k", [21, 32, 33, 63])
def test_count_over_batches_equals_the_oracle(oracle, k):
    reads = reads_for(k, k)
    m = EM.EngineModel(k)
    for a in range(0, len(reads), 37):
        m.count(reads[a:a + 37])
    assert m.table == oracle_table(oracle, k, reads)
    assert m.windows == oracle.count_windows(reads, k) == sum(m.table.values())
    ks, cnt = m.export_ge(2)
    assert ks == sorted(ks) and all(m.table[v] >= 2 for v in ks) and m.count_ge(2) == len(ks)


@pytest.mark.parametrize("k", [65, 201])
def test_count_over_batches_equals_kmer_truth(k):
    reads = reads_for(k, k, 40)
    m = EM.EngineModel(k)
    m.count(reads[:15]); m.count(reads[15:])
    assert m.table == KT.count_truth(reads, k)


@pytest.mark.parametrize("k", [31, 47])
def test_count_filtered_equals_the_oracle(oracle, k):
    reads, other = reads_for(k, 1), reads_for(k, 2) + reads_for(k, 1)[:30]
    keys = sorted(oracle_table(oracle, k, reads))[::3]
    lo, hi = KT.lohi(keys)
    ot = oracle.OracleTable(k, 1 << 12).load_filter(lo, hi).count_reads_filtered(other)
    m = EM.EngineModel(k)
    m.count(reads)
    m.load_filter(keys)
    assert m.windows == 0 and set(m.table.values()) == {0} and m.filter_mode
    m.count_filtered(other)
    assert np.array_equal(m.query(keys), ot.query(lo, hi))
    assert m.windows == oracle.count_windows(other, k)
    assert len(m.table) == len(keys)                         # nothing inserted
    with pytest.raises(EM.Refused) as r:
        m.count(other)
    assert r.value.code == EM.ERR_STATE


@pytest.mark.parametrize("k,L", [(31, 2), (63, 3), (65, 2)])
def test_prefilter_life_equals_the_prefilter_model(k, L):
    reads = reads_for(k, 5, 60)
    truth = KT.count_truth(reads, k)
    admitted, by_value = PM.model(truth, k, 16, L)
    m = EM.EngineModel(k)
    m.prefilter_begin(L, 16)
    with pytest.raises(EM.Refused):
        m.count(reads)
    m.prefilter_add(reads[:20]); m.upload(1, reads[20:]); m.prefilter_add_uploaded(1)
    m.clear()                                                # leaves the prefilter as it is
    assert m.prefilter_fill() == by_value
    m.prefilter_arm()
    m.count(reads)
    assert m.table == admitted and m.windows == sum(admitted.values())
    m.prefilter_drop()
    m.count(reads[:5])
    assert m.windows == sum(admitted.values()) + sum(KT.count_truth(reads[:5], k).values())


@pytest.mark.parametrize("k", [31, 63, 127])
def test_key_parts_union_is_the_whole(k):
    reads = reads_for(k, 9, 60)
    truth = KT.count_truth(reads, k)
    m = EM.EngineModel(k)
    m.set_option("key_parts", 3)
    union, windows = {}, 0
    for part in range(3):
        m.clear(); m.set_option("key_part", part)
        m.count(reads)
        assert not set(m.table) & set(union)
        assert all(EM.slice_of_key(v, k, 3) == part for v in m.table)
        union.update(m.table); windows += m.windows
    assert union == truth and windows == sum(truth.values())
    m.set_option("key_part", 0); m.count(reads)              # no clear: the table holds the union of slices 2 and 0
    assert set(m.table) == {v for v in truth if EM.slice_of_key(v, k, 3) in (0, 2)}
    if k <= 63:                                              # any other partition of the key space gives the same whole
        lo, hi = KT.lohi(sorted(truth))
        s = ST.slice_of(torch.from_numpy(lo.view(np.int64)), torch.from_numpy(hi.view(np.int64)), k, 3)
        assert sum(int((s == p).sum()) for p in range(3)) == len(truth)


def test_saturation_and_repeated_keys():
    k = 21
    m = EM.EngineModel(k)
    key = KT.key_int("A" * k)
    m.add_pairs([key, 5, key, 7], [SAT - 6, 0, 2, SAT])       # a key twice in one call is summed
    assert m.table == {key: SAT - 4, 5: 0, 7: SAT}
    m.count(["A" * (k + 2)])                                 # 3 windows
    assert m.table[key] == SAT - 1 and m.windows == 3
    m.count(["a" * (k + 9)])                                 # 10 more: saturates
    assert m.table[key] == SAT and m.windows == 13
    m.add_pairs([9, 9], None)                                # None counts add 0
    assert m.table[9] == 0 and m.count_ge(0) == 4 and m.count_ge(1) == 2
    assert m.count_stats() == {"unique": 0, "distinct": 2, "total": 2 * SAT, "max_count": SAT}
    h = m.histogram(1)
    assert h.tolist() == [2, 0, 2]
    m.reset_counts()                                         # insert mode: keys kept, counts and windows 0
    assert set(m.table) == {key, 5, 7, 9} and not any(m.table.values()) and m.windows == 0 and not m.filter_mode
    m.load_filter([key]); m.add_pairs([11], [3])             # add_pairs works in filter mode and drops the sieve
    m.set_option("force_path", 4)
    with pytest.raises(EM.Refused) as r:
        m.count_filtered(["A" * k])
    assert r.value.code == EM.ERR_STATE and m.windows == 0
    m.set_option("force_path", 0); m.count_filtered(["A" * k, "ACGTN"])
    assert m.table == {key: 1, 11: 3} and m.windows == 1


def test_refusals_leave_the_model_untouched():
    m = EM.EngineModel(31)
    m.count(["ACGT" * 20]); m.upload(0, ["ACGT" * 20])
    before = (dict(m.table), m.windows, list(m.slots), m.force_path, m.hash_shift, m.pf_state)
    for call, code in [(lambda: m.count_filtered(["ACGT" * 20]), EM.ERR_STATE), (lambda: m.count_uploaded(1, False), EM.ERR_STATE),
                       (lambda: m.count_uploaded(0, True), EM.ERR_STATE), (m.prefilter_arm, EM.ERR_STATE), (m.prefilter_drop, EM.ERR_STATE),
                       (lambda: m.set_option("force_path", 3), EM.ERR_INVALID), (lambda: m.set_option("hash_shift", 1), EM.ERR_STATE),
                       (lambda: m.set_option("key_part", 1), EM.ERR_INVALID), (lambda: m.set_counts([12345], [1]), EM.ERR_INVALID)]:
        with pytest.raises(EM.Refused) as r:
            call()
        assert r.value.code == code
        assert before == (dict(m.table), m.windows, list(m.slots), m.force_path, m.hash_shift, m.pf_state)
    m.set_option("key_parts", 2)
    with pytest.raises(EM.Refused) as r:
        m.prefilter_begin(2, 16)
    assert r.value.code == EM.ERR_STATE and m.pf_state == EM.PF_OFF
    long = EM.EngineModel(65)
    for name, value in (("force_path", 2), ("force_path", 4), ("fused_dump", 1), ("hash_shift", 1)):
        with pytest.raises(EM.Refused) as r:
            long.set_option(name, value)
        assert r.value.code == EM.ERR_INVALID


@pytest.mark.parametrize("k", [31, 65])
def test_observers_equal_the_truths_called_directly(k):
    reads, probe = reads_for(k, 3, 50), reads_for(k, 4, 12) + [""]
    m = EM.EngineModel(k)
    m.count(reads)
    hits, distinct = KT.scan_truth(probe, k, m.table)
    offs = DT.offsets_of(probe)
    got_hits, got_distinct = m.scan(probe)
    assert np.array_equal(got_distinct, distinct)
    assert np.array_equal(got_hits, KT.hit_words(offs, hits, (int(offs[-1]) + 63) // 64 + 2))
    counts, valid = m.window_counts(probe)
    want = DT.profile(probe, k, m.table)
    assert np.array_equal(counts, want[0]) and np.array_equal(valid, want[1])
    assert np.array_equal(DT.bits(got_hits, len(counts)), counts != 0)      # the scan is one bit of the count profile
    assert np.array_equal(m.read_depth(probe, 1), DT.depth_rows(probe, k, m.table, 1))
    some = sorted(m.table)[:20]
    assert m.query(some + [some[0] ^ 1]).tolist()[:20] == [m.table[v] for v in some]


# ---- the generator ---------------------------------------------------------------------------------------------------

# (last mutator class, next call class): what every committed life must contain
REQUIRED_PAIRS = [
    ("clear", "count"), ("clear", "observe"), ("clear", "reserve"), ("clear", "prefilter"),
    ("count", "clear"), ("count", "load_filter"), ("count", "reset_counts"), ("count", "observe"), ("count", "add_pairs"),
    ("count", "option"), ("count", "upload"), ("count", "count"), ("count", "refused"),
    ("upload", "set_stream"), ("set_stream", "count"),
    ("add_pairs", "observe"), ("add_pairs", "add_pairs"),
    ("load_filter", "count_filtered"), ("load_filter", "add_pairs"), ("load_filter", "observe"), ("load_filter", "clear"),
    ("count_filtered", "reset_counts"), ("count_filtered", "clear"), ("count_filtered", "observe"), ("count_filtered", "count_filtered"),
    ("reset_counts", "count_filtered"), ("reset_counts", "count"), ("reset_counts", "observe"),
    ("reserve", "count"), ("option", "count"), ("option", "count_filtered"), ("option", "observe"), ("option", "option"),
    ("prefilter", "prefilter"), ("prefilter", "count"), ("prefilter", "clear"), ("prefilter", "observe"),
]
REQUIRED_PAIRS_SHORT = [          # k <= 63: the merge, set_counts, re-bucketing, the fused dump's orders
    ("clear", "option"), ("option", "add_pairs"), ("clear", "add_pairs"), ("count", "prefilter"), ("count", "reserve"),
    ("reserve", "observe"), ("set_counts", "count_filtered"), ("add_pairs", "option"), ("option", "clear"), ("load_filter", "set_counts"),
]

LIVES = [(f, s) for f in SEEDS for s in SEEDS[f]]
_cache = {}


def life(family, seed):
    if (family, seed) not in _cache:
        _cache[family, seed] = EO.generate(seed, family, N_OPS[family])
    return _cache[family, seed]


@pytest.mark.parametrize("family,seed", LIVES)
def test_generator_is_deterministic(family, seed):
    ops, cov = life(family, seed)
    ops2, cov2 = EO.generate(seed, family, N_OPS[family])
    assert len(ops) == len(ops2) and EO.digest(ops) == EO.digest(ops2) and cov == cov2
    assert ops[0]["k"] in EO.FAMILIES[family] and len(ops) - 1 >= N_OPS[family]


@pytest.mark.parametrize("family,seed", LIVES)
def test_life_covers_the_required_orders(family, seed):
    ops, cov = life(family, seed)
    short = family != "long"
    pairs = REQUIRED_PAIRS + (REQUIRED_PAIRS_SHORT if short else [])
    missing = [p for p in pairs if p not in cov["pairs"]]
    assert not missing, f"{family} seed {seed}: pairs {missing}"
    missing = [p for p in (EO.PRECONDITIONS if short else EO.LONG_PRECONDITIONS) if p not in cov["preconditions"]]
    assert not missing, f"{family} seed {seed}: preconditions {missing}"
    # every observer at the end of the life, refusals at a few per cent, each followed by an observer at some point
    tail = [o["kind"] for o in ops[-len(EO.OBSERVERS) - 1:] if o["op"] == "obs"]
    assert set(EO.OBSERVERS) <= set(tail)
    refused = [i for i, o in enumerate(ops) if o.get("refused")]
    assert 0.01 * len(ops) <= len(refused) <= 0.1 * len(ops), len(refused)
    assert all(ops[i + 1]["op"] == "obs" for i in refused)
    # count_uploaded refused while its slot HOLDS a batch (the batch must stay), and uploads out of pinned buffers
    m, kept = EM.EngineModel(ops[0]["k"]), 0
    for op in ops[1:]:
        kept += op["op"] == "count_uploaded" and op["refused"] and m.slots[op["slot"]] is not None
        EO.apply(m, op)
    assert kept >= 2, kept
    assert sum(1 for o in ops[1:] if o["op"] == "upload" and o["pinned"]) >= 3
    seq = ops[1:]
    i_up = [i for i, o in enumerate(seq) if o["op"] == "upload" and o["pinned"]]
    assert any(seq[i + 1]["op"] == "set_stream" and seq[i + 2]["op"] == "count_uploaded" for i in i_up if i + 2 < len(seq))
    names = {(o["op"], o.get("form")) for o in ops[1:]}
    for need in [("count", "host"), ("count", "dev"), ("count_uploaded", None), ("count_filtered", "host"), ("count_filtered", "dev"),
                 ("add_pairs", "host"), ("add_pairs", "dev"), ("load_filter", "host"), ("load_filter", "dev"),
                 ("set_stream", None), ("reserve", None), ("flush", None), ("reset_counts", None)] + ([("add_pairs", "multi"), ("set_counts", None)] if short else []):
        assert need in names, f"{family} seed {seed}: no {need}"
    assert {"pf_begin", "pf_add", "pf_arm", "pf_drop", "upload"} <= {o["op"] for o in ops[1:]}


def test_every_op_replays_on_a_fresh_model():
    """the records are self-contained: replaying them on a new model refuses exactly the ops marked refused"""
    ops, _ = life("narrow", SEEDS["narrow"][0])
    m = EM.EngineModel(ops[0]["k"])
    for op in ops[1:]:
        assert (EO.apply(m, op)[0] == "err") == op["refused"], EO.describe(op)
