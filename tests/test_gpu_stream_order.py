"""The stream-order contract of every device entry point of ``include/kdf.h``, observed with ``tests/stream_order.py``.

One table, ``CASES``: each case names the entry points it puts under contract conditions, the class the header gives the
call (``no_sync``: runs in stream order and does not synchronise; ``syncs``: synchronises the engine's stream and its
outputs are complete in stream order on return), the key widths it runs at and the function that builds inputs and
decoys, observes the result and compares it with the truth.  ``tests/test_stream_order_table.py`` proves on the CPU that
the table covers the header.

Every case runs its call twice on one engine in one state: the control run (host synchronisations around the call, true
inputs, nothing in flight) and the contract run (decoys in the buffers, the true inputs produced on the caller's stream
behind a measured delay, no host synchronisation before the call, the decoys put back right after it).  Control, contract
and the independent truth (``kmer_truth`` / ``depth_truth`` / ``hits_truth`` / the models, never the code under test) must
agree, and the call must have returned inside the delay window (``no_sync``) or after it (``syncs``)."""
import collections

import numpy as np
import pytest

import coverage_model as CM
import depth_truth as DT
import hits_truth as HT
import kmer_truth as KT
import merge_truth as MT
import prefilter_merge_model as PMM
import prefilter_model as PM
import regions_model as RM
import sketch_model as SkM
import spool_model as SM
import variants_model as VM
from stream_order import NO_SYNC, SYNCS, CallerStreams, Delay, StreamOrder, World, decoy_indices, decoy_like, decoy_offsets, pack_reads, random_reads, same

pytestmark = pytest.mark.gpu

KS = (31, 47, 65)              # one word, two words, three-word long keys
SHORT = (31, 47)
LOG2_CELLS = 20
SKETCH_P = 12


# ------------------------------------------------------------------------------------------------ truth, computed once

class Truth:
    """Everything the cases compare with, from the read strings alone (``depth_truth.keys_of_reads``: the oracle's string
    rules), for the true reads and -- keys only -- for the decoy reads."""

    def __init__(self, world, k):
        self.k, self.W = k, PM.key_words(k)
        self.read_keys = DT.keys_of_reads(world.reads, k)
        self.counts = dict(collections.Counter(v for ks in self.read_keys for _, v in ks))
        self.windows = sum(self.counts.values())
        self.keys = sorted(self.counts)
        self.decoy_keys = sorted({v for ks in DT.keys_of_reads(world.decoy_reads, k) for _, v in ks})
        assert not set(self.decoy_keys) & set(self.keys)
        self.solid = {v: c for v, c in self.counts.items() if c >= 2}        # the table / filter of the reading cases
        assert 1000 < len(self.solid) < len(self.counts)


_world = None
_truths = {}


def world():
    global _world
    if _world is None:
        _world = World(seed=20240607)
        assert 2e5 <= _world.n_bases <= 3e5
    return _world


def truth(k):
    if k not in _truths:
        _truths[k] = Truth(world(), k)
    return _truths[k]


@pytest.fixture(scope="module")
def delay():
    """One unit of the delay op, timed with HIP events."""
    return Delay()


@pytest.fixture(scope="module")
def report(delay):
    rows = []
    yield rows
    if rows:
        ts = [r[2] for r in rows if r[1] != "-"]
        print(f"\nstream-order: delay unit {delay.unit_ms:.4f} ms; {len(rows)} contract runs; t_call {min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f} ms")
        for label, cls, t_call, host, ms, early in rows:
            print(f"  {label:58s} {cls:8s} t_call {t_call * 1e3:8.3f} ms  call {host * 1e3:8.3f} ms  delay {ms:7.1f} ms  early {early}")


@pytest.fixture(scope="module")
def caller_streams(delay):
    """caller streams measured to run independently of one another"""
    cs = CallerStreams(delay)
    print(f"\nstream-order: {len(cs.streams)} caller streams measured independent of one another")
    return cs


@pytest.fixture()
def H(delay, caller_streams, report):
    h = StreamOrder(delay, caller_streams)
    yield h
    report.extend(h.records)


# ------------------------------------------------------------------------------------------------ helpers

def engine(H, k, hint=1 << 18, stream=None, **opts):
    from kmer_denovo_filter_amd import KmerEngine
    e = KmerEngine(k, capacity_hint=hint)
    for name, v in opts.items():
        e.set_option(name, v)
    e.set_stream(H.handle if stream is None else stream.cuda_stream)
    return e


def key_cols(keys, k):
    """canonical keys (Python ints) -> the arrays an engine for k takes: lo | lo, hi | (n, W) rows in the lo position"""
    if k <= 32:
        return {"lo": np.array(keys, dtype=np.uint64)}
    if k <= 63:
        lo, hi = KT.lohi(keys)
        return {"lo": lo, "hi": hi}
    return {"lo": KT.rows(keys, PM.key_words(k))}


def key_inputs(true_keys, decoy_keys, k):
    assert len(true_keys) == len(decoy_keys)
    t, d = key_cols(true_keys, k), key_cols(decoy_keys, k)
    return {n: (t[n], d[n]) for n in t}


def draw(pool, n, rng):
    return [pool[i] for i in rng.integers(0, len(pool), n)]


def ints_of(lo, hi, k):
    lo = np.asarray(lo, dtype=np.uint64)
    if k > 63:
        return [KT.int_of_row(r) for r in lo.reshape(-1, PM.key_words(k)).tolist()]
    if k <= 32 or hi is None:
        return [int(v) for v in lo.tolist()]
    return [int(l) | (int(h) << 64) for l, h in zip(lo.tolist(), np.asarray(hi, dtype=np.uint64).tolist())]


def table(e):
    """{key: count} of everything the engine's table holds (counts 0 included)"""
    lo, hi, cnt = e.export_ge(0)
    keys = ints_of(lo, hi, e.k)
    assert len(set(keys)) == len(keys)
    return dict(zip(keys, (int(c) for c in cnt.tolist())))


def load_table(e, counts):
    keys = sorted(counts)
    cols = key_cols(keys, e.k)
    e.add_pairs(cols["lo"], cols.get("hi"), np.array([counts[v] for v in keys], np.uint32))
    return keys


def load_filter(e, keys):
    cols = key_cols(sorted(keys), e.k)
    e.load_filter(cols["lo"], cols.get("hi"))


def both(H, engines, label, cls, setup, inputs, outputs, call, observe, want, producers=None):
    """control run, then a contract run on each of the two independent caller streams (``engines`` move with them), and
    the three-way agreement"""
    if H.expected is not None and not H.class_checked:           # the case's principal call: the table's class is the one enforced
        assert cls == H.expected, f"{label}: the table lists class {H.expected}, the case enforces {cls}"
        H.class_checked = True
    H.use(H.streams.pair[0], engines)
    setup()
    ctl = H.control(inputs, outputs, call)
    got_ctl = observe(ctl)
    same(got_ctl, want, f"{label}: control run vs truth")
    for i, stream in enumerate(H.streams.pair):
        H.use(stream, engines)
        setup()
        run = H.contract(inputs, outputs, call, ctl.host_s, producers=producers)
        got = observe(run)
        H.note(f"{label} S{i}", cls, ctl, run)
        broke = None
        try:
            H.check_class(label, cls, run)
        except AssertionError as e:          # report wrong data first: it is the graver finding
            broke = e
        same(got, want, f"{label}: contract run on caller stream {i} vs truth")
        same(got, got_ctl, f"{label}: contract run on caller stream {i} vs control run")
        if broke is not None:
            raise broke


def stream_call(method, w):
    return lambda p: method(p["packed"], p["invalid"], w.n_bases)


def bits_to_words(bits, n_words):
    b = np.zeros(n_words * 64, bool)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64)


def sieve_words(counts, k, s):
    """the words of a sieve that tallied ``counts``: thermometer nibbles of min(sum of the cell's sightings, 3)"""
    cells = np.zeros(1 << s, np.int64)
    for key, c in counts.items():
        cells[PM.cell_of(key, k, s)] += c
    code = np.array([0, 1, 3, 7], np.uint64)[np.minimum(cells, 3)]
    return (code.reshape(-1, 16) << (np.arange(16, dtype=np.uint64) * np.uint64(4))).sum(axis=1, dtype=np.uint64)


def hit_mask(w, T, index):
    rows, per_read = HT.read_hits(w.reads, T.k, index, keys=T.read_keys)
    return rows, per_read, HT.mask_words(w.reads, per_read, (w.n_bases + 63) // 64)


# ------------------------------------------------------------------------------------------------ stream consumers

def count_class(k, path="pending"):
    """kdf_count_reads_dev is deferred and does not synchronise where the batch goes to the pending stream or is
    partitioned; through the direct kernels (force_path 1, every long engine) the host learns the number of distinct keys
    after every chunk, to grow the table in time: those calls synchronise (include/kdf.h says so)."""
    return SYNCS if k > 63 or path == "direct" else NO_SYNC


COUNT_PATHS = {"pending": {}, "direct": {"force_path": 1}, "binned": {"force_path": 2}, "in_place": {"l1_direct_positions": 1 << 12}}


def case_count_dev(H, k, path):
    w, T = world(), truth(k)
    with engine(H, k, **COUNT_PATHS[path]) as e:
        # the table is read only after the decoys are back in place: whatever the call deferred is applied then
        both(H, [e], f"count_dev[{path}] k={k}", count_class(k, path), e.clear, w.stream_inputs(), {}, stream_call(e.count_dev, w),
             lambda run: (table(e), e.stats()[2]), (T.counts, T.windows))
        if path in ("binned", "in_place"):
            assert e.get_stat("binned_passes") >= 1
        if path == "direct":
            assert e.last_count_path() == "direct" and e.get_stat("binned_passes") == 0


def case_count_dev_lazy(H, k, path):
    """clear, count_dev, export_ge_dev served by the dump-only flush, then a query that materialises the table"""
    import torch
    w, T = world(), truth(k)
    cols = key_cols(T.keys, k)
    want_q = np.array([T.counts[v] for v in T.keys], np.uint32)
    with engine(H, k, **COUNT_PATHS[path]) as e:
        assert e.get_stat("lazy_table") == 1 and e.get_stat("fused_dump") == 1

        def observe(run):
            cap = len(T.keys) + 64
            with torch.cuda.stream(H.S):
                lo, hi, cnt = (torch.zeros(cap, dtype=torch.int64, device=H.dev) for _ in range(3))
            torch.cuda.synchronize()
            d0, m0 = e.get_stat("dump_only_flushes"), e.get_stat("materialisations")
            n = e.export_ge_dev(1, lo.data_ptr(), hi.data_ptr() if k > 32 else None, cnt.data_ptr(), cap, sorted_=True)
            assert e.get_stat("dump_only_flushes") == d0 + 1 and e.get_stat("materialisations") == m0
            with torch.cuda.stream(H.S):
                keys = ints_of(lo[:n].cpu().numpy().view(np.uint64), hi[:n].cpu().numpy().view(np.uint64), k)
                dump = dict(zip(keys, cnt.cpu().numpy().view(np.uint32)[:n].tolist()))
            q = e.query(cols["lo"], cols.get("hi"))
            assert e.get_stat("materialisations") == m0 + 1
            return dump, q, table(e)
        both(H, [e], f"count_dev[lazy {path}] k={k}", NO_SYNC, e.clear, w.stream_inputs(), {}, stream_call(e.count_dev, w), observe,
             (T.counts, want_q, T.counts))


FILTERED_PATHS = {"direct": {"force_path": 1}, "sieve": {"force_path": 4}, "bin_sieve": {"sieve_bins": 1}, "long_sieve": {"long_sieve": 1}}


def case_count_filtered_dev(H, k, path):
    from kmer_denovo_filter_amd._native import KdfError
    from kmer_denovo_filter_amd.engine import bin_sieve_geometry
    w, T = world(), truth(k)
    with engine(H, k, **FILTERED_PATHS[path]) as e:
        load_filter(e, T.solid)
        both(H, [e], f"count_filtered_dev[{path}] k={k}", CLASS["kdf_count_reads_filtered_dev"], e.reset_counts, w.stream_inputs(), {},
             stream_call(e.count_filtered_dev, w), lambda run: table(e), T.solid)
        took = e.get_stat("last_count_path")
        if path == "bin_sieve":
            try:
                bin_sieve_geometry(len(T.solid), T.W)
                accepted = True
            except KdfError:
                accepted = False
            assert (took == 5) == accepted
        else:
            assert took == {"direct": 0, "sieve": 3, "long_sieve": 3}[path]


def case_prefilter(H, k):
    """prefilter_add_dev, then arm, then the gated count_dev"""
    w, T = world(), truth(k)
    admitted, by_value = PM.model(T.counts, k, LOG2_CELLS, 2)
    assert 0 < len(admitted) < len(T.counts)
    with engine(H, k) as e:
        def begin():
            if e.get_stat("prefilter_state"):
                e.prefilter_drop()
            e.clear()
            e.prefilter_begin(2, LOG2_CELLS)
        both(H, [e], f"prefilter_add_dev k={k}", NO_SYNC, begin, w.stream_inputs(), {}, stream_call(e.prefilter_add_dev, w),
             lambda run: (e.prefilter_export(), e.prefilter_fill(), e.get_stat("prefilter_windows")),
             (sieve_words(T.counts, k, LOG2_CELLS), by_value, T.windows))
        e.prefilter_arm()
        both(H, [e], f"count_dev[armed prefilter] k={k}", count_class(k), e.clear, w.stream_inputs(), {}, stream_call(e.count_dev, w),
             lambda run: (table(e), e.stats()[2]), (admitted, sum(admitted.values())))


def case_sketch_add_dev(H, k):
    w, T = world(), truth(k)
    with engine(H, k) as e:
        def begin():
            if e.get_stat("sketch_state"):
                e.sketch_drop()
            e.sketch_begin(SKETCH_P)
        both(H, [e], f"sketch_add_dev k={k}", NO_SYNC, begin, w.stream_inputs(), {}, stream_call(e.sketch_add_dev, w),
             lambda run: (e.sketch_registers(), e.get_stat("sketch_windows")), (SkM.registers_of_keys(T.keys, k, SKETCH_P), T.windows))


def case_scan_dev(H, k, path):
    w, T = world(), truth(k)
    _, mw = SM.stream_words(w.n_bases)
    nw = (w.n_bases + 63) // 64
    opts = {"direct": {"force_path": 1}, "sieve": {}, "long_sieve": {"long_sieve": 1}}[path]
    with engine(H, k, **opts) as e:
        load_table(e, T.solid)
        both(H, [e], f"scan_dev[{path}] k={k}", NO_SYNC, lambda: None, w.stream_inputs(), {"hits": mw * 8},
             lambda p: e.scan_dev(p["packed"], p["invalid"], w.n_bases, p["hits"]),
             lambda run: run.read("hits", np.uint64, nw), hit_mask(w, T, T.solid)[2])
        assert e.get_stat("last_scan_path") == (0 if path == "direct" else 3)


def case_window_counts_dev(H, k):
    w, T = world(), truth(k)
    _, mw = SM.stream_words(w.n_bases)
    nw = (w.n_bases + 63) // 64
    counts, valid, _ = DT.profile(w.reads, k, T.solid, keys=T.read_keys)
    with engine(H, k) as e:
        load_table(e, T.solid)
        both(H, [e], f"window_counts_dev k={k}", NO_SYNC, lambda: None, w.stream_inputs(), {"counts": w.n_bases * 4, "valid": mw * 8},
             lambda p: e.window_counts_dev(p["packed"], p["invalid"], w.n_bases, p["counts"], p["valid"]),
             lambda run: (run.read("counts", np.uint32, w.n_bases), run.read("valid", np.uint64, nw)), (counts, bits_to_words(valid, nw)))


def case_read_depth_dev(H, k):
    w, T = world(), truth(k)
    nr = len(w.reads)
    with engine(H, k) as e:
        load_table(e, T.solid)
        both(H, [e], f"read_depth_dev k={k}", CLASS["kdf_read_depth_dev"], lambda: None, {**w.stream_inputs(), **w.offsets_input()}, {"rows": nr * 48},
             lambda p: e.read_depth_dev(p["packed"], p["invalid"], w.n_bases, p["offsets"], nr, 2, p["rows"]),
             lambda run: run.read("rows", np.uint64, nr * 6).reshape(nr, 6), DT.depth_rows(w.reads, k, T.solid, 2, keys=T.read_keys))


def case_hit_keys_dev(H, k):
    w, T = world(), truth(k)
    rng = np.random.default_rng(5)
    starts = [(int(w.offsets[r]) + i, v) for r, ks in enumerate(T.read_keys) for i, v in ks]
    pick = [starts[i] for i in rng.integers(0, len(starts), 5000)]
    pos = np.array([p for p, _ in pick], np.uint64)
    inputs = {"packed": (w.packed, w.d_packed), "positions": (pos, decoy_indices(len(pos), w.n_bases - k + 1, rng))}
    with engine(H, k) as e:
        both(H, [e], f"hit_keys_dev k={k}", NO_SYNC, lambda: None, inputs, {"keys": len(pos) * T.W * 8},
             lambda p: e.hit_keys_dev(p["packed"], w.n_bases, p["positions"], len(pos), p["keys"]),
             lambda run: run.read("keys", np.uint64, len(pos) * T.W).reshape(len(pos), T.W), KT.rows([v for _, v in pick], T.W))


# ------------------------------------------------------------------------------------------------ key-array consumers

def _pairs(T, k, rng, order):
    keys = list(T.keys)
    if order == "hash":            # ascending table hash: grouped by the buckets of a table of any size
        cols = key_cols(keys, k)
        keys = [keys[i] for i in np.argsort(MT.key_hash(cols["lo"], cols.get("hi")), kind="stable")]
    else:
        keys = [keys[i] for i in rng.permutation(len(keys))]
    cnt = np.array([T.counts[v] for v in keys], np.uint32)
    inputs = key_inputs(keys, draw(T.decoy_keys, len(keys), rng), k)
    inputs["counts"] = (cnt, rng.integers(1, 1000, len(cnt)).astype(np.uint32))
    return keys, inputs


def case_add_pairs_dev(H, k, path):
    T = truth(k)
    rng = np.random.default_rng(6)
    keys, inputs = _pairs(T, k, rng, "hash" if path == "lds" else "shuffled")
    with engine(H, k, **({} if k > 63 else {"merge_min_pairs": 1 if path == "lds" else 1 << 40})) as e:
        both(H, [e], f"add_pairs_dev[{path}] k={k}", CLASS["kdf_add_pairs_dev"], e.clear, inputs, {},
             lambda p: e.add_pairs_dev(p["lo"], p.get("hi"), p["counts"], len(keys)), lambda run: table(e), T.counts)
        if k <= 63:
            assert e.get_stat("last_merge_path") == (1 if path == "lds" else 2)


def _dumped_in_bucket_order(H, T, k):
    """the truth's keys in the order kdf_export_parts_dev writes them: a 2^28-slot table holding the truth, dumped with
    parts = 1 between host synchronisations"""
    import torch
    with engine(H, k, hint=BIG_HINT) as src:
        load_table(src, T.counts)
        cap = len(T.counts) + 64
        lo, hi, cnt = (torch.zeros(cap, dtype=torch.int64, device=H.dev) for _ in range(3))
        torch.cuda.synchronize()
        n, _ = src.export_parts_dev(0, 1, lo.data_ptr(), hi.data_ptr() if k > 32 else None, cnt.data_ptr(), cap)
        torch.cuda.synchronize()
        keys = ints_of(lo[:n].cpu().numpy().view(np.uint64), hi[:n].cpu().numpy().view(np.uint64), k)
    assert sorted(keys) == T.keys
    return keys


def case_add_pairs_multi_dev(H, k, order):
    """three segments that share keys: every key's count is split over the segments that hold it.  ``bucket_order``: the
    segments keep the order of a kdf_export_parts_dev dump (each bucket merged in LDS); ``shuffled``: global atomics"""
    T = truth(k)
    rng = np.random.default_rng(7)
    keys = _dumped_in_bucket_order(H, T, k) if order == "bucket_order" else _pairs(T, k, rng, "shuffled")[0]
    inputs, lens = {}, []
    for s in range(3):
        part = [v for j, v in enumerate(keys) if j % 3 == s or T.counts[v] >= 3]
        cnt = np.array([T.counts[v] if T.counts[v] < 3 else T.counts[v] // 3 + (s < T.counts[v] % 3) for v in part], np.uint32)
        for n, pair in key_inputs(part, draw(T.decoy_keys, len(part), rng), k).items():
            inputs[f"{n}{s}"] = pair
        inputs[f"counts{s}"] = (cnt, rng.integers(1, 1000, len(cnt)).astype(np.uint32))
        lens.append(len(part))
    with engine(H, k, merge_min_pairs=1) as e:
        both(H, [e], f"add_pairs_multi_dev[{order}] k={k}", CLASS["kdf_add_pairs_multi_dev"], e.clear, inputs, {},
             lambda p: e.add_pairs_multi_dev([(p[f"lo{s}"], p.get(f"hi{s}"), p[f"counts{s}"], lens[s]) for s in range(3)]),
             lambda run: table(e), T.counts)
        assert e.get_stat("last_merge_path") == (1 if order == "bucket_order" else 2)


def case_load_filter_dev(H, k):
    """the filter is loaded from HBM; what it holds shows in the count --if of the true reads that follows"""
    import torch
    w, T = world(), truth(k)
    rng = np.random.default_rng(8)
    stored = sorted(T.solid)
    keys = [stored[i] for i in rng.permutation(len(stored))]
    dp, dm = H.to_dev(w.packed), H.to_dev(w.invalid)

    def counted(run):
        torch.cuda.synchronize()
        e.count_filtered_dev(dp.data_ptr(), dm.data_ptr(), w.n_bases)
        return table(e)
    with engine(H, k) as e:
        both(H, [e], f"load_filter_dev k={k}", CLASS["kdf_load_filter_dev"], lambda: None, key_inputs(keys, draw(T.decoy_keys, len(keys), rng), k), {},
             lambda p: e.load_filter_dev(p["lo"], p.get("hi"), len(keys)), counted, T.solid)


def case_query_dev(H, k):
    T = truth(k)
    rng = np.random.default_rng(9)
    n = 20000
    ask = draw(T.keys, n // 2, rng) + draw(T.decoy_keys, n - n // 2, rng)
    ask = [ask[i] for i in rng.permutation(n)]
    other = draw(T.keys, n // 2, rng) + draw(T.decoy_keys, n - n // 2, rng)
    with engine(H, k) as e:
        load_table(e, T.solid)
        both(H, [e], f"query_dev k={k}", CLASS["kdf_query_dev"], lambda: None, key_inputs(ask, other, k), {"counts": n * 4},
             lambda p: e.query_dev(p["lo"], p.get("hi"), n, p["counts"]), lambda run: run.read("counts", np.uint32, n),
             np.array([T.solid.get(v, 0) for v in ask], np.uint32))


def case_set_counts_dev(H, k):
    """decoy keys are STORED keys too (another draw): a read out of order sets other counts, it is not refused"""
    T = truth(k)
    rng = np.random.default_rng(10)
    stored = sorted(T.solid)
    pick = [stored[i] for i in rng.permutation(len(stored))[:len(stored) // 2]]
    other = [stored[i] for i in rng.permutation(len(stored))[:len(pick)]]
    cnt = rng.integers(1, 1 << 20, len(pick)).astype(np.uint32)
    inputs = key_inputs(pick, other, k)
    inputs["counts"] = (cnt, rng.integers(1, 1 << 20, len(pick)).astype(np.uint32))
    want = {v: 0 for v in stored}
    want.update(zip(pick, (int(c) for c in cnt)))
    with engine(H, k) as e:
        load_filter(e, stored)
        call = (lambda p: e.set_counts_w_dev(p["lo"], p["counts"], len(pick))) if k > 63 else \
               (lambda p: e.set_counts_dev(p["lo"], p.get("hi"), p["counts"], len(pick)))
        both(H, [e], f"set_counts_dev k={k}", CLASS["kdf_set_counts_dev"], e.reset_counts, inputs, {}, call, lambda run: table(e), want)


def case_prefilter_merge_dev(H, k):
    rng = np.random.default_rng(11)
    s, first, n = 16, 256, 2048
    segs = [PMM.encode(rng.integers(0, 4, (n, 16))) for _ in range(4)]
    with engine(H, k) as e:
        def begin():
            if e.get_stat("prefilter_state"):
                e.prefilter_drop()
            e.prefilter_begin(2, s)
        want = np.zeros(1 << (s - 4), np.uint64)
        want[first:first + n] = PMM.merge(want[first:first + n], segs[:2])
        both(H, [e], f"prefilter_merge_dev k={k}", NO_SYNC, begin, {"seg0": (segs[0], segs[2]), "seg1": (segs[1], segs[3])}, {},
             lambda p: e.prefilter_merge_dev([p["seg0"], p["seg1"]], first, n), lambda run: e.prefilter_export(), want)


def case_format_kmers_dev(H, k):
    from oracle import oracle as O
    T = truth(k)
    rng = np.random.default_rng(12)
    keys = draw(T.keys, 3001, rng)
    text = "".join(f">{7 + i}\n{O.int_to_kmer(v, k)}\n" for i, v in enumerate(keys)).encode()
    with engine(H, 31) as e:                                          # (the key form follows the call's k, not the engine's)
        assert e.kmer_text_bytes(k, 0, 7, len(keys)) == len(text)
        both(H, [e], f"format_kmers_dev k={k}", NO_SYNC, lambda: None, key_inputs(keys, draw(T.decoy_keys, len(keys), rng), k), {"text": len(text)},
             lambda p: e.format_kmers_dev(p["lo"], p.get("hi"), len(keys), k, 0, 7, 0, len(text), p["text"]),
             lambda run: run.read("text", np.uint8, len(text)), np.frombuffer(text, np.uint8))


def _variant_case(seed, k):
    case = VM.random_case(seed, n_reads=300, n_var=60, lo=max(k + 10, 40), hi=k + 60)
    return case, VM.variant_windows(case, k)


def _window_keys(case, k, entry_pos):
    """canonical keys (Python ints) of listed windows of a packed case, by the string rules"""
    from oracle import oracle as O
    codes, _ = VM.stream_arrays(case["packed"], case["invalid"], case["n_bases"])
    s = "".join("ACGT"[int(c)] for c in codes)
    return [KT.key_int(O.canonicalize(s[int(p):int(p) + k])) for p in entry_pos]


def case_variant_evidence_dev(H, k):
    case, (pr, pv, pf, ep, epair) = _variant_case(21, k)
    other, (opr, opv, opf, oep, oepair) = _variant_case(22, k)
    assert len(ep) > 200 and len(pr) > 20
    rng = np.random.default_rng(13)
    W, n_var = PM.key_words(k), len(case["var_pos"])
    keys = _window_keys(case, k, ep)
    stored = {v: int(rng.integers(1, 50)) for v in set(keys) if rng.random() < 0.7}
    pool = _window_keys(other, k, oep)
    inputs = {"keys": (KT.rows(keys, W), KT.rows(draw(pool, len(keys), rng), W)),
              "entry_pair": (epair, decoy_indices(len(epair), len(pr), rng)),
              "pair_var": (pv, decoy_indices(len(pv), n_var, rng, np.uint32)),
              "pair_flags": (pf, rng.integers(0, 2, len(pf)).astype(np.uint8))}
    with engine(H, k) as e:
        load_table(e, stored)
        both(H, [e], f"variant_evidence_dev k={k}", NO_SYNC, lambda: None, inputs, {"pair_rows": len(pv) * 8, "var_rows": n_var * 64},
             lambda p: e.variant_evidence_dev(p["keys"], p["entry_pair"], len(ep), p["pair_var"], p["pair_flags"], len(pv), n_var, p["pair_rows"], p["var_rows"]),
             lambda run: (run.read("pair_rows", np.uint32, len(pv) * 2).reshape(-1, 2), run.read("var_rows", np.uint64, n_var * 8).reshape(-1, 8)),
             VM.variant_evidence(keys, epair, pv, pf, n_var, stored))


# ------------------------------------------------------------------------------------------------ synchronising entry points

def case_read_hits_dev(H, k):
    w, T = world(), truth(k)
    nr, nw = len(w.reads), (w.n_bases + 63) // 64
    rows, _, mask = hit_mask(w, T, T.solid)
    with engine(H, k) as e:
        load_table(e, T.solid)
        both(H, [e], f"read_hits_dev k={k}", SYNCS, lambda: None, {**w.stream_inputs(), **w.offsets_input()}, {"rows": nr * 8, "bits": (nw + 2) * 8},
             lambda p: e.read_hits_dev(p["packed"], p["invalid"], w.n_bases, p["offsets"], nr, p["bits"], p["rows"]),
             lambda run: (run.read("rows", np.uint32, nr * 2).reshape(nr, 2), run.read("bits", np.uint64, nw)), (rows, mask))


def case_hit_list_dev(H, k):
    w, T = world(), truth(k)
    rng = np.random.default_rng(14)
    _, per_read, mask = hit_mask(w, T, T.solid)
    pos, rd = HT.hit_list(w.reads, per_read)
    dbits = np.zeros(len(mask) * 64, bool)
    dbits[decoy_indices(len(pos), w.n_bases - k + 1, rng).astype(np.int64)] = True
    inputs = {"bits": (mask, np.packbits(dbits, bitorder="little").view(np.uint64)), **w.offsets_input()}
    cap = 2 * len(pos) + 64
    with engine(H, k) as e:
        def observe(run):
            n = run.ret
            return n, run.read("positions", np.uint64, n), run.read("reads", np.int64, n)
        both(H, [e], f"hit_list_dev k={k}", SYNCS, lambda: None, inputs, {"positions": cap * 8, "reads": cap * 8},
             lambda p: e.hit_list_dev(p["bits"], w.n_bases, p["offsets"], len(w.reads), p["positions"], p["reads"], cap), observe,
             (len(pos), pos.astype(np.uint64), rd))


def _coverage_inputs(w, T, rng):
    """the true reads aligned on a small reference with M / I / D / S CIGARs; a tenth of them skipped"""
    _, per_read, mask = hit_mask(w, T, T.solid)
    span = 8192
    cigar, co, rs = [], [0], []
    for r in w.reads:
        L = len(r)
        if L > 30 and rng.random() < 0.5:
            a, i, d = int(rng.integers(5, L // 3)), int(rng.integers(1, 5)), int(rng.integers(1, 5))
            ops = [(4, 3), (0, a), (1, i), (0, 5), (2, d), (0, L - 3 - a - i - 5)]
        else:
            ops = [(0, L)]
        cigar += CM.cigar_words(ops).tolist()
        co.append(len(cigar))
        rs.append(-1 if rng.random() < 0.1 else int(rng.integers(0, span)))          # (some run past span: dropped)
    return mask, span, np.array(rs, np.int64), np.array(cigar, np.uint32), np.array(co, np.int64)


def case_hit_coverage_dev(H, k):
    w, T = world(), truth(k)
    rng = np.random.default_rng(15)
    mask, span, rs, cigar, co = _coverage_inputs(w, T, rng)
    dmask = hit_mask(w, T, {v: 1 for v in draw(T.keys, 3000, rng)})[2]
    inputs = {"bits": (mask, dmask), **w.offsets_input(), "ref_start": (rs, rng.permutation(rs)), "cigar": (cigar, rng.permutation(cigar)),
              "cigar_offsets": (co, decoy_offsets(co, rng))}
    kc, rc = np.zeros(span, np.uint32), np.zeros(span, np.uint32)
    CM.hit_coverage(mask, w.n_bases, k, w.offsets, rs, cigar, co, kc, rc)
    assert rc.any()
    with engine(H, k) as e:
        both(H, [e], f"hit_coverage_dev k={k}", SYNCS, lambda: None, inputs, {"kmer_cov": (span * 4, 0), "read_cov": (span * 4, 0)},
             lambda p: e.hit_coverage_dev(p["bits"], w.n_bases, p["offsets"], len(w.reads), p["ref_start"], p["cigar"], len(cigar),
                                          p["cigar_offsets"], p["kmer_cov"], p["read_cov"], span),
             lambda run: (run.read("kmer_cov", np.uint32, span), run.read("read_cov", np.uint32, span)), (kc, rc))


def case_coverage_list_dev(H, k):
    rng = np.random.default_rng(16)
    span = 50000

    def cov():
        rc = np.where(rng.random(span) < 0.3, rng.integers(1, 6, span), 0).astype(np.uint32)
        return (rc * rng.integers(1, 20, span)).astype(np.uint32), rc
    (kc, rc), (dkc, drc) = cov(), cov()
    first, n = 100, span - 333
    want = CM.coverage_list(kc, rc, first, n, 2)
    cap = n
    with engine(H, k) as e:
        def observe(run):
            m = run.ret
            return m, run.read("pos", np.uint64, m), run.read("kmer", np.uint32, m), run.read("read", np.uint32, m)
        both(H, [e], f"coverage_list_dev k={k}", SYNCS, lambda: None, {"kmer_cov": (kc, dkc), "read_cov": (rc, drc)},
             {"pos": cap * 8, "kmer": cap * 4, "read": cap * 4},
             lambda p: e.coverage_list_dev(p["kmer_cov"], p["read_cov"], first, n, 2, p["pos"], p["kmer"], p["read"], cap), observe,
             (len(want[0]),) + tuple(want))


def case_variant_windows_dev(H, k):
    case, want = _variant_case(21, k)
    other, _ = _variant_case(22, k)
    rng = np.random.default_rng(17)
    n, nr, nv = case["n_bases"], len(case["offsets"]) - 1, len(case["var_pos"])
    pw, mw = SM.stream_words(n)

    def fit(a, m):
        """another case's array cut or cycled to m entries (values stay what a case holds)"""
        a = np.asarray(a)
        return np.resize(a, m) if len(a) else np.zeros(m, a.dtype)
    alt = np.frombuffer(case["alt"], np.uint8)
    dalt = rng.choice(np.frombuffer(b"ACGT", np.uint8), len(alt))
    dpacked, dinvalid, _, _ = pack_reads(random_reads(rng, np.diff(case["offsets"]) - 1))
    inputs = {"packed": (case["packed"][:pw], dpacked), "invalid": (case["invalid"][:mw], dinvalid),
              "offsets": (case["offsets"], decoy_offsets(case["offsets"], rng)),
              "ref_start": (case["ref_start"], rng.permutation(case["ref_start"])),
              "cigar": (case["cigar"], fit(other["cigar"], len(case["cigar"]))),
              "cigar_offsets": (case["cigar_offsets"], decoy_offsets(case["cigar_offsets"], rng)),
              "qual": (case["qual"], rng.integers(0, 41, len(case["qual"])).astype(np.uint8)),
              "qual_offsets": (case["qual_offsets"], decoy_offsets(case["qual_offsets"], rng)),
              "var_pos": (case["var_pos"], np.sort(rng.permutation(fit(other["var_pos"], nv)))),
              "var_span": (case["var_span"], fit(other["var_span"], nv)), "var_ref_len": (case["var_ref_len"], fit(other["var_ref_len"], nv)),
              "alt": (alt, dalt), "alt_offsets": (case["alt_offsets"], decoy_offsets(case["alt_offsets"], rng))}
    pc, ec = 2 * len(want[0]) + 256, 2 * len(want[3]) + 4096
    assert len(want[0]) > 20 and len(want[3]) > 200
    with engine(H, k) as e:
        def call(p):
            return e.variant_windows_dev(p["packed"], p["invalid"], n, p["offsets"], nr, p["ref_start"], p["cigar"], len(case["cigar"]),
                                         p["cigar_offsets"], p["qual"], len(case["qual"]), p["qual_offsets"], case["min_baseq"], p["var_pos"],
                                         p["var_span"], p["var_ref_len"], nv, p["alt"], len(alt), p["alt_offsets"], p["pair_read"],
                                         p["pair_var"], p["pair_flags"], pc, p["entry_pos"], p["entry_pair"], ec, check=False)

        def observe(run):
            a, b = run.ret
            assert a <= pc and b <= ec
            return (run.read("pair_read", np.int64, a), run.read("pair_var", np.uint32, a), run.read("pair_flags", np.uint8, a),
                    run.read("entry_pos", np.uint64, b), run.read("entry_pair", np.uint64, b))
        both(H, [e], f"variant_windows_dev k={k}", SYNCS, lambda: None, inputs,
             {"pair_read": pc * 8, "pair_var": pc * 4, "pair_flags": pc, "entry_pos": ec * 8, "entry_pair": ec * 8}, call, observe, tuple(want))


def case_cluster_intervals_dev(H, k):
    rng = np.random.default_rng(18)
    n = 30000

    def intervals():
        chrom = rng.integers(-1, 5, n).astype(np.int64)
        start = rng.integers(0, 3_000_000, n).astype(np.int64)
        return chrom, start, start + rng.integers(1, 400, n)
    (c, s, t), (dc, ds, dt) = intervals(), intervals()
    region_of, regions = RM.cluster_intervals(c, s, t, 150)
    cap = n
    with engine(H, k) as e:
        def observe(run):
            m = run.ret
            return m, run.read("region_of", np.int64, n), run.read("regions", np.int64, m * 4).reshape(m, 4)
        both(H, [e], f"cluster_intervals_dev k={k}", SYNCS, lambda: None, {"chrom": (c, dc), "start": (s, ds), "end": (t, dt)},
             {"region_of": n * 8, "regions": cap * 32},
             lambda p: e.cluster_intervals_dev(p["chrom"], p["start"], p["end"], n, 150, p["region_of"], p["regions"], cap), observe,
             (len(regions), region_of, regions))


def case_group_distinct_dev(H, k):
    T = truth(k)
    rng = np.random.default_rng(19)
    n, groups = 40000, 300
    rows = KT.rows(draw(T.keys[:2000], n, rng), T.W)
    drows = KT.rows(draw(T.decoy_keys[:2000], n, rng), T.W)
    g = rng.integers(-2, groups + 2, n).astype(np.int64)
    with engine(H, 31) as e:                                          # (words is independent of the engine's key width)
        both(H, [e], f"group_distinct_dev k={k}", SYNCS, lambda: None, {"group": (g, rng.integers(-2, groups + 2, n).astype(np.int64)), "keys": (rows, drows)},
             {"counts": groups * 8}, lambda p: e.group_distinct_dev(p["group"], p["keys"], T.W, n, groups, p["counts"]),
             lambda run: run.read("counts", np.uint64, groups), RM.group_distinct(g, rows, groups))


DUMPS = {"sorted": ({"force_path": 1}, 0, True), "unsorted": ({"force_path": 1}, 2, False), "fused": ({"force_path": 2}, 1, False)}


def case_export_ge_dev(H, k, form):
    """the table's input is the count_dev in front of the dump, its stream produced behind the delay"""
    w, T = world(), truth(k)
    opts, min_count, sorted_ = DUMPS[form]
    want = {v: c for v, c in T.counts.items() if c >= min_count}
    cap = len(want) + 64
    with engine(H, k, **({} if k > 63 else opts)) as e:
        def call(p):
            e.count_dev(p["packed"], p["invalid"], w.n_bases)
            return e.export_ge_dev(min_count, p["lo"], p["hi"] if 32 < k <= 63 else None, p["cnt"], cap, sorted_=sorted_)

        def observe(run):
            n = run.ret
            keys = ints_of(run.read("lo", np.uint64, n * (T.W if k > 63 else 1)), run.read("hi", np.uint64, n), k)
            if sorted_:
                assert keys == sorted(keys)
            return dict(zip(keys, run.read("cnt", np.uint32, n).tolist()))
        f0 = e.get_stat("fused_dumps") if k <= 63 else 0
        both(H, [e], f"export_ge_dev[{form}] k={k}", SYNCS, e.clear, w.stream_inputs(),
             {"lo": cap * 8 * (T.W if k > 63 else 1), "hi": cap * 8, "cnt": cap * 4}, call, observe, want)
        if form == "fused":
            assert e.get_stat("fused_dumps") == f0 + 3


def case_export_parts_w_packed_dev(H, k):
    """the long engines' owner dump (any table size) behind a count_dev whose stream is produced behind the delay"""
    import long_truth as LT
    w, T = world(), truth(k)
    parts = 3
    owners = LT.owner(LT.long_hash(KT.rows(T.keys, T.W)), parts)
    want = {v: (T.counts[v], int(o)) for v, o in zip(T.keys, owners.tolist())}
    assert len(set(owners.tolist())) == parts
    cap = len(T.keys) * (8 * T.W + 4) + 8 * parts + 64
    with engine(H, k) as e:
        def call(p):
            e.count_dev(p["packed"], p["invalid"], w.n_bases)
            return e.export_parts_w_packed_dev(1, parts, p["buf"], cap)

        def observe(run):
            n, counts, offs = run.ret
            assert n == sum(counts) and offs[parts] <= cap and all(o % 8 == 0 for o in offs)
            buf, got = run.read("buf", np.uint8), {}
            for part in range(parts):
                m, a = counts[part], offs[part]
                keys = buf[a:a + m * T.W * 8].view(np.uint64).reshape(m, T.W)
                cnt = buf[a + m * T.W * 8:a + m * T.W * 8 + m * 4].view(np.uint32)
                got.update((KT.int_of_row(r), (int(c), part)) for r, c in zip(keys.tolist(), cnt.tolist()))
            assert len(got) == n
            return got
        both(H, [e], f"export_parts_w_packed_dev k={k}", SYNCS, e.clear, w.stream_inputs(), {"buf": cap}, call, observe, want)


BIG_HINT = 1 << 27             # 2^28 slots: the smallest table the owner-ordered dump takes
PARTS = 3


def _owner_truth(T, k, counts, min_count):
    """{key: (count, owner)} of the entries with count >= min_count: owner(key) = ((hash >> 48) * parts) >> 16 (merge_truth)"""
    keys = sorted(v for v, c in counts.items() if c >= min_count)
    cols = key_cols(keys, k)
    owners = MT.owner(MT.key_hash(cols["lo"], cols.get("hi")), PARTS)
    assert len(set(owners.tolist())) == PARTS
    return {v: (counts[v], int(o)) for v, o in zip(keys, owners.tolist())}


def _hash_ordered(keys, k, log2cap):
    """is the list grouped by the top log2cap - 6 hash bits, ascending (the order the header gives the owner-ordered dump)?"""
    cols = key_cols(keys, k)
    pre = MT.order_key(MT.key_hash(cols["lo"], cols.get("hi")), log2cap)
    return bool(np.all(pre[1:] >= pre[:-1]))


def case_export_parts_dev(H, k, form):
    """the owner-ordered dump of a 2^28-slot table (its own kernels over merge scratch: count, scan, write) behind a
    count_dev whose stream is produced behind the delay; ``form``: separate arrays or the packed all-to-all layout"""
    w, T = world(), truth(k)
    want = _owner_truth(T, k, T.counts, 2)
    n_want = len(want)
    cap = n_want + 64
    cap_bytes = cap * (20 if k > 32 else 12) + 8 * PARTS
    with engine(H, k, hint=BIG_HINT) as e:
        assert e.get_stat("log2cap") == 28

        def call(p):
            e.count_dev(p["packed"], p["invalid"], w.n_bases)
            if form == "packed":
                return e.export_parts_packed_dev(2, PARTS, p["buf"], cap_bytes)
            return e.export_parts_dev(2, PARTS, p["lo"], p["hi"] if k > 32 else None, p["cnt"], cap)

        def observe(run):
            n, counts = run.ret[0], run.ret[1]
            assert n == sum(counts) <= cap
            if form == "packed":
                offs, buf = run.ret[2], run.read("buf", np.uint8)
                assert offs[PARTS] <= cap_bytes and all(o % 8 == 0 for o in offs)
                lo, hi, cnt = [], [], []
                for part in range(PARTS):
                    m, a = counts[part], offs[part]
                    lo.append(buf[a:a + 8 * m].view(np.uint64))
                    a += 8 * m
                    if k > 32:
                        hi.append(buf[a:a + 8 * m].view(np.uint64))
                        a += 8 * m
                    cnt.append(buf[a:a + 4 * m].view(np.uint32))
                lo, cnt = np.concatenate(lo), np.concatenate(cnt)
                hi = np.concatenate(hi) if k > 32 else None
            else:
                lo, hi, cnt = run.read("lo", np.uint64, n), run.read("hi", np.uint64, n) if k > 32 else None, run.read("cnt", np.uint32, n)
            keys = ints_of(lo, hi, k)
            assert _hash_ordered(keys, k, 28), "the dump is not in hash order"
            owner = np.repeat(np.arange(PARTS), counts).tolist()
            return dict(zip(keys, zip((int(c) for c in cnt.tolist()), owner)))
        outputs = {"buf": cap_bytes} if form == "packed" else {"lo": cap * 8, "hi": cap * 8, "cnt": cap * 4}
        both(H, [e], f"export_parts{'_packed' if form == 'packed' else ''}_dev k={k}", SYNCS, e.clear, w.stream_inputs(), outputs, call, observe, want)


def case_histogram_dev(H, k):
    w, T = world(), truth(k)
    high = 40
    bins = np.zeros(high + 2, np.uint64)
    for c in T.counts.values():
        bins[min(c, high + 1)] += 1
    with engine(H, k) as e:
        def call(p):
            e.count_dev(p["packed"], p["invalid"], w.n_bases)
            e.histogram_dev(high, p["bins"])
        both(H, [e], f"histogram_dev k={k}", SYNCS, e.clear, w.stream_inputs(), {"bins": (high + 2) * 8}, call,
             lambda run: run.read("bins", np.uint64, high + 2), bins)


def case_prefilter_export_dev(H, k):
    w, T = world(), truth(k)
    nwords = 1 << (LOG2_CELLS - 4)
    with engine(H, k) as e:
        def begin():
            if e.get_stat("prefilter_state"):
                e.prefilter_drop()
            e.prefilter_begin(3, LOG2_CELLS)

        def call(p):
            e.prefilter_add_dev(p["packed"], p["invalid"], w.n_bases)
            e.prefilter_export_dev(p["words"], 0, nwords)
        both(H, [e], f"prefilter_export_dev k={k}", SYNCS, begin, w.stream_inputs(), {"words": nwords * 8}, call,
             lambda run: run.read("words", np.uint64, nwords), sieve_words(T.counts, k, LOG2_CELLS))


def case_sketch_registers_dev(H, k):
    w, T = world(), truth(k)
    with engine(H, k) as e:
        def begin():
            if e.get_stat("sketch_state"):
                e.sketch_drop()
            e.sketch_begin(SKETCH_P)

        def call(p):
            e.sketch_add_dev(p["packed"], p["invalid"], w.n_bases)
            e.sketch_registers_dev(p["regs"])
        both(H, [e], f"sketch_registers_dev k={k}", SYNCS, begin, w.stream_inputs(), {"regs": 1 << SKETCH_P}, call,
             lambda run: run.read("regs", np.uint8, 1 << SKETCH_P), SkM.registers_of_keys(T.keys, k, SKETCH_P))


def case_parse_kmer_fasta_dev(H, k):
    from oracle import oracle as O
    T = truth(k)
    rng = np.random.default_rng(23)
    n = 4000

    def text_of(keys):
        return np.frombuffer("".join(f">{i}\n{O.int_to_kmer(v, k)}\n" for i, v in enumerate(keys)).encode(), np.uint8)
    keys, other = draw(T.keys, n, rng), draw(T.decoy_keys, n, rng)
    text = text_of(keys)
    want = key_cols(keys, k)
    with engine(H, 31) as e:
        def observe(run):
            assert run.ret == (n, len(text))
            got = {"lo": run.read("lo", np.uint64, n * (T.W if k > 63 else 1)).reshape(want["lo"].shape)}
            if 32 < k <= 63:
                got["hi"] = run.read("hi", np.uint64, n)
            return got
        both(H, [e], f"parse_kmer_fasta_dev k={k}", SYNCS, lambda: None, {"text": (text, text_of(other))}, {"lo": n * 8 * max(T.W if k > 63 else 1, 1), "hi": n * 8},
             lambda p: e.parse_kmer_fasta_dev(p["text"], len(text), k, True, True, p["lo"], p["hi"] if 32 < k <= 63 else None, n), observe, want)


def _fasta_text(rng, lengths):
    out = []
    for i, r in enumerate(random_reads(rng, lengths)):
        out.append(f">r{i:05d}\n")
        out += [r[a:a + 60] + "\n" for a in range(0, len(r), 60)]
    return "".join(out).encode()


def case_fasta_pack_dev(H, k):
    import fasta_stream_model as FM
    from kmer_denovo_filter_amd import _native
    rng = np.random.default_rng(24)
    lengths = rng.integers(100, 2000, 200)
    text, dtext = _fasta_text(rng, lengths), _fasta_text(rng, lengths[::-1])
    assert len(text) == len(dtext)
    codes, offs = FM.pack_file(text)
    n, nr = len(codes), len(offs) - 1
    cap_bases, cap_reads = len(text) + 1, len(text) // 2 + 2
    pw, mw = SM.stream_words(cap_bases)
    with engine(H, k) as e:
        def call(p):
            return e.fasta_pack_dev(p["text"], len(text), True, _native.FastaState(), p["packed"], p["invalid"], cap_bases, p["offsets"], cap_reads)

        def observe(run):
            assert run.ret == (n, nr, len(text))
            return FM.from_words(run.read("packed", np.uint64), run.read("invalid", np.uint64), n), run.read("offsets", np.int64, nr + 1)
        both(H, [e], f"fasta_pack_dev k={k}", SYNCS, lambda: None, {"text": (np.frombuffer(text, np.uint8), np.frombuffer(dtext, np.uint8))},
             {"packed": pw * 8, "invalid": mw * 8, "offsets": (cap_reads + 1) * 8}, call, observe, (np.asarray(codes, np.uint8), np.asarray(offs, np.int64)))


def _bam_pair(tmp, n_reads=1200):
    """two BAMs (tests/helpers.write_bam) of reads of the same names and lengths over different genomes: the same records
    byte for byte except for the sequences, so the same inflated layout, block count and sub-ranges -> (paths, reads)"""
    import os
    from helpers import write_bam
    rng = np.random.default_rng(27)
    reads = world().reads[:n_reads]
    other = random_reads(rng, [len(r) for r in reads])
    paths = []
    for tag, rs in (("true", reads), ("decoy", other)):
        paths.append(os.path.join(tmp, f"{tag}.bam"))
        write_bam(paths[-1], [("chr1", 1_000_000)], [{"name": f"r{i:06d}", "seq": r, "pos": 100 + i} for i, r in enumerate(rs)])
    return paths, reads


def _bgzf_blocks(path):
    """[(DEFLATE payload, isize)] of the non-empty BGZF blocks of a file, and the bytes they inflate to (python's gzip)"""
    import gzip
    import struct
    raw = open(path, "rb").read()
    items, at = [], 0
    while at < len(raw):
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        isize = struct.unpack_from("<I", raw, at + bsize - 4)[0]
        if isize:
            items.append((raw[at + 18:at + bsize - 8], isize))
        at += bsize
    return items, gzip.decompress(raw)


def _padded(a, n):
    out = np.zeros(n, np.uint8)
    out[:len(a)] = np.frombuffer(bytes(a), np.uint8) if not isinstance(a, np.ndarray) else a
    return out


def case_bgzf_inflate_dev(H, k):
    import tempfile
    from kmer_denovo_filter_amd.reads import BGZF_BLOCK_DTYPE
    with tempfile.TemporaryDirectory() as tmp:
        paths, _ = _bam_pair(tmp)
        (items, data), (ditems, _) = _bgzf_blocks(paths[0]), _bgzf_blocks(paths[1])
    assert len(items) == len(ditems) >= 3 and [i for _, i in items] == [i for _, i in ditems]

    def tables(its):
        blocks = np.zeros(len(its), BGZF_BLOCK_DTYPE)
        co = oo = 0
        for j, (p, isize) in enumerate(its):
            blocks[j] = (co, oo, 1000 * (j + 1), len(p), isize)
            co += len(p); oo += isize
        return b"".join(p for p, _ in its), blocks, oo
    (comp, blocks, total), (dcomp, dblocks, _) = tables(items), tables(ditems)
    room = max(len(comp), len(dcomp)) + 8
    inputs = {"comp": (_padded(comp, room), _padded(dcomp, room)), "blocks": (blocks, dblocks)}
    with engine(H, k) as e:
        f0 = e.get_stat("bamdev_fallback_blocks")
        both(H, [e], f"bgzf_inflate_dev k={k}", SYNCS, lambda: None, inputs, {"out": total, "status": len(items) * 4},
             lambda p: e.bgzf_inflate_dev(p["comp"], p["blocks"], len(items), p["out"], total, p["status"]),
             lambda run: (run.read("out", np.uint8, total), run.read("status", np.uint32, len(items))),
             (np.frombuffer(data, np.uint8), np.zeros(len(items), np.uint32)))
        assert e.get_stat("bamdev_fallback_blocks") == f0               # the device decoder took every block


def case_bamdev_decode_dev(H, k):
    import tempfile
    from kmer_denovo_filter_amd import reads as R
    with tempfile.TemporaryDirectory() as tmp:
        paths, reads = _bam_pair(tmp)
        batches_ = []
        for path in paths:
            with R.bam_raw_reader(path, 0xD00, False, 0, 1, 1 << 22, 1 << 22) as rd:
                got = list(rd)
            assert len(got) == 1
            batches_.append(got[0])
    b, d = batches_
    assert len(b.blocks) == len(d.blocks) >= 3 and len(b.subs) == len(d.subs) and b.inflated_bytes == d.inflated_bytes
    room = max(len(b.comp), len(d.comp)) + 8
    inputs = {"comp": (_padded(b.comp, room), _padded(d.comp, room)), "blocks": (b.blocks, d.blocks), "subs": (b.subs, d.subs)}
    cap_bases, cap_reads = R.decode_capacity(b.inflated_bytes)
    pw, mw = SM.stream_words(cap_bases)
    packed, invalid, n, offs = pack_reads(reads)
    codes, inv = SM.unpack(packed, invalid, n)
    with engine(H, k) as e:
        def call(p):
            return e.bamdev_decode_dev(p["comp"], p["blocks"], len(b.blocks), p["subs"], len(b.subs), 0xD00, False, p["packed"], p["invalid"],
                                       cap_bases, p["offsets"], cap_reads)

        def observe(run):
            nb, nr, status = run.ret
            c, i = SM.unpack(run.read("packed", np.uint64), run.read("invalid", np.uint64), nb)
            return nb, nr, status, np.where(i, 0, c).astype(np.uint8), i, run.read("offsets", np.int64, nr + 1)
        both(H, [e], f"bamdev_decode_dev k={k}", SYNCS, lambda: None, inputs, {"packed": pw * 8, "invalid": mw * 8, "offsets": (cap_reads + 1) * 8},
             call, observe, (n, len(reads), np.zeros(len(b.subs), np.uint32), np.where(inv, 0, codes).astype(np.uint8), inv, offs))


# ------------------------------------------------------------------------------------------------ two engines

def case_join(H, k):
    """h's join against an engine on ANOTHER caller stream with work in flight there: a count --if (stream order, does not
    synchronise, at every k) whose read stream is produced behind a delay on that stream, and no synchronisation before
    the join.  The header: other's stream is synchronised before the kernel is queued on h's stream.  (Deferred insert
    counts would not do: the flush that applies them ends in a host synchronisation of its own, and so does
    kdf_add_pairs_dev.)"""
    w, T = world(), truth(k)
    rng = np.random.default_rng(25)
    S2 = H.independent_stream()
    a_keys = [v for v in T.keys if rng.random() < 0.5] + draw(T.decoy_keys, 2000, rng)
    a_counts = dict(zip(a_keys, (int(c) for c in rng.integers(0, 6, len(a_keys)))))
    want = {v: (c, T.counts.get(v, 0)) for v, c in a_counts.items() if c >= 2 and 1 <= T.counts.get(v, 0) <= 2}
    assert len(want) > 100
    cap = len(want) + 64
    with engine(H, k) as a, engine(H, k, stream=S2) as o:
        load_table(a, a_counts)
        load_filter(o, T.keys)                                       # other holds every key of the reads, counted by the call below

        def call(p):
            o.count_filtered_dev(p["packed"], p["invalid"], w.n_bases)
            n = a.export_join_dev(o, 2, None, 1, 2, p["out_lo"], p["out_hi"] if 32 < k <= 63 else None, p["out_cnt"], p["out_other"], cap, sorted_=True)
            return n, a.count_join(o, 2, None, 1, 2)

        def observe(run):
            n, m = run.ret
            assert n == m
            keys = ints_of(run.read("out_lo", np.uint64, n * (T.W if k > 63 else 1)), run.read("out_hi", np.uint64, n), k)
            return dict(zip(keys, zip(run.read("out_cnt", np.uint32, n).tolist(), run.read("out_other", np.uint32, n).tolist())))
        inputs = w.stream_inputs()
        both(H, [a], f"export_join_dev / count_join k={k}", SYNCS, o.reset_counts, inputs,
             {"out_lo": cap * 8 * (T.W if k > 63 else 1), "out_hi": cap * 8, "out_cnt": cap * 4, "out_other": cap * 4}, call, observe, want,
             producers={n: S2 for n in inputs})


# ------------------------------------------------------------------------------------------------ upload slots

def _halves(k):
    """the true reads as two batches cut between reads, packed apart: (ReadStream-like triples, the reads of each)"""
    w = world()
    h = len(w.reads) // 2
    return [pack_reads(w.reads[:h]), pack_reads(w.reads[h:])]


def _pinned(batches):
    from kmer_denovo_filter_amd.reads import PinnedBatches, ReadStream
    pb = PinnedBatches(len(batches), max(b[2] for b in batches))
    out = []
    for (hp, hm), (p, m, n, offs) in zip(pb.batches, batches):
        hp[:len(p)] = p
        hm[:len(m)] = m
        out.append(ReadStream(hp, hm, n, offs))
    return pb, out


def _gate(H, ms, stream=None):
    """a delay on S (or ``stream``) and an event behind it: ``not gate.query()`` right after a call means it returned inside the window"""
    import torch
    stream = H.S if stream is None else stream
    with torch.cuda.stream(stream):
        H.delay.enqueue(ms)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def case_count_uploaded(H, k, move):
    """upload into slot 0, delay on S, count; the second batch goes into slot 0 AT ONCE (the copy stream must wait for
    use_done), count again.  ``move``: a set_stream to a second caller stream between upload and count."""
    import torch
    T = truth(k)
    pb, (b0, b1) = _pinned(_halves(k))
    S2 = H.independent_stream()
    try:
        with engine(H, k) as e:
            def sequence(contract, ms):
                e.set_stream(H.handle)
                e.clear()
                torch.cuda.synchronize()
                e.upload_async(0, b0)
                gate = _gate(H, ms) if contract else None
                if move:                             # (set_stream drains the old stream, its delay included: the window is S2's)
                    e.set_stream(S2.cuda_stream)
                    gate = _gate(H, ms, S2) if contract else None
                e.count_uploaded(0)
                e.upload_async(0, b1)
                early = None if gate is None else not gate.query()
                e.count_uploaded(0)                  # (the host waits for the slot's copy, and that copy for use_done)
                if not contract:
                    torch.cuda.synchronize()
                return early
            import time
            t0 = time.perf_counter()
            sequence(False, 0)
            t_call = time.perf_counter() - t0
            ctl = (table(e), e.stats()[2])
            ms = max(20.0, 4e3 * t_call)
            early = sequence(True, ms)
            got = (table(e), e.stats()[2])
            H.records.append((f"count_uploaded[{'moved' if move else 'same stream'}] k={k}", NO_SYNC, t_call, 0.0, ms, early))
            same(got, (T.counts, T.windows), "count_uploaded: contract run vs truth")
            same(ctl, (T.counts, T.windows), "count_uploaded: control run vs truth")
            assert H.expected == count_class(k)
            H.class_checked = True
            if H.expected == NO_SYNC:
                assert early is True, "kdf_count_uploaded / kdf_upload_reads_async: returned after the delay on the engine's stream had run"
            else:                                    # (the count itself synchronises: direct kernels)
                assert early is False
    finally:
        pb.close()


def case_tally_sketch_uploaded(H, k):
    """prefilter_add_uploaded takes the slot's batch, sketch_add_uploaded leaves it: sketch, tally, upload the next at once"""
    import torch
    T = truth(k)
    pb, (b0, b1) = _pinned(_halves(k))
    try:
        with engine(H, k) as e:
            def sequence(contract, ms):
                for state, drop in (("prefilter_state", e.prefilter_drop), ("sketch_state", e.sketch_drop)):
                    if e.get_stat(state):
                        drop()
                e.prefilter_begin(2, LOG2_CELLS)
                e.sketch_begin(SKETCH_P)
                torch.cuda.synchronize()
                e.upload_async(0, b0)
                gate = _gate(H, ms) if contract else None
                e.sketch_add_uploaded(0)
                e.prefilter_add_uploaded(0)
                e.upload_async(0, b1)
                early = None if gate is None else not gate.query()
                e.sketch_add_uploaded(0)             # (returns once the slot's copy is complete: that copy waits for use_done)
                e.prefilter_add_uploaded(0)
                if not contract:
                    torch.cuda.synchronize()
                return early
            import time
            t0 = time.perf_counter()
            sequence(False, 0)
            t_call = time.perf_counter() - t0
            ctl = (e.prefilter_export(), e.sketch_registers())
            ms = max(20.0, 4e3 * t_call)
            early = sequence(True, ms)
            got = (e.prefilter_export(), e.sketch_registers())
            H.records.append((f"prefilter_add_uploaded / sketch_add_uploaded k={k}", NO_SYNC, t_call, 0.0, ms, early))
            want = (sieve_words(T.counts, k, LOG2_CELLS), SkM.registers_of_keys(T.keys, k, SKETCH_P))
            same(got, want, "uploaded tally and sketch: contract run vs truth")
            same(ctl, want, "uploaded tally and sketch: control run vs truth")
            assert H.expected == NO_SYNC
            H.class_checked = True
            assert early is True, "kdf_prefilter_add_uploaded / kdf_sketch_add_uploaded: returned after the delay on the engine's stream had run"
    finally:
        pb.close()


# ------------------------------------------------------------------------------------------------ spool

SEG = 1 << 16
N_BATCHES = 6


class Batches:
    """the true reads cut into ragged batches between reads, each with a decoy batch of the same n_bases and read count"""

    def __init__(self):
        w = world()
        rng = np.random.default_rng(26)
        cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(100, len(w.reads) - 100), N_BATCHES - 1, replace=False)) + [len(w.reads)]
        self.reads = [w.reads[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        self.true = [pack_reads(r) for r in self.reads]
        self.decoy = [pack_reads(random_reads(rng, [len(x) for x in r][::-1])) for r in self.reads]
        assert all(t[2] == d[2] for t, d in zip(self.true, self.decoy))

    def inputs(self, j, offsets=False):
        t, d = self.true[j], self.decoy[j]
        out = {"packed": (t[0], d[0]), "invalid": (t[1], d[1])}
        if offsets:
            out["offsets"] = (t[3], d[3])
        return out

    def segments(self, upto=None):
        return SM.segments([(t[0], t[1], t[2]) for t in self.true[:upto]], SEG)


_batches = None


def batches():
    global _batches
    if _batches is None:
        _batches = Batches()
    return _batches


def batch_truth(k, upto):
    """{key: count} and the windows of the first ``upto`` batches (no window spans a batch: the batches are cut between reads)"""
    T, B = truth(k), batches()
    n_reads = sum(len(r) for r in B.reads[:upto])
    counts = dict(collections.Counter(v for ks in T.read_keys[:n_reads] for _, v in ks))
    return counts, sum(counts.values())


def spool(hbm=1 << 30, host=0):
    from kmer_denovo_filter_amd.spool import ReadSpool
    sp = ReadSpool(0, hbm, host)
    sp.set_option("segment_positions", SEG)
    return sp


def append_all(H, sp, streams, upto, first=0, offsets=False, t_call=0.0):
    """append_dev of batches [first, upto) in turn on ``streams``, every batch produced behind a delay on its stream, no
    host synchronisation between the appends -> the runs (their buffers stay alive with them)"""
    B = batches()
    runs = []
    for j in range(first, upto):
        s = streams[j % len(streams)]
        inputs = B.inputs(j, offsets)
        n, nr = B.true[j][2], len(B.reads[j])
        call = (lambda p, n=n, nr=nr, s=s: sp.append_dev(p["packed"], p["invalid"], n, s.cuda_stream, p["offsets"], nr)) if offsets else \
               (lambda p, n=n, s=s: sp.append_dev(p["packed"], p["invalid"], n, s.cuda_stream))
        runs.append(H.contract(inputs, {}, call, t_call, producers={name: s for name in inputs}))
    return runs


def segments_of(sp):
    return [sp.read_segment(i) for i in range(sp.stat("segments"))]


def same_segments(sp, want, what):
    got = segments_of(sp)
    same([(p, m, int(n)) for p, m, n in got], [(p, m, int(n)) for p, m, n in want], what)


def case_spool(H, k, tier):
    """appends produced behind delays on two caller streams in turn, then -- at once -- replays in every mode and the
    sketch into engines on a third stream, then one more append behind the replay"""
    import torch
    T, B = truth(k), batches()
    S1, S2 = H.independent_stream(), H.independent_stream()
    counts, windows = batch_truth(k, N_BATCHES - 1)
    solid = {v: c for v, c in counts.items() if c >= 2}
    want = ((counts, windows), solid, sieve_words(counts, k, LOG2_CELLS), SkM.registers_of_keys(sorted(counts), k, SKETCH_P))
    hbm, host = ((1 << 30), 0) if tier == "hbm" else (0, 1 << 30)
    # (the control fills a spool of its own, alive to the end: the contract run's segments are other memory, so a replay
    # that did not wait for the appends cannot find the control's bytes there)
    with spool(hbm, host) as spc, spool(hbm, host) as sp, engine(H, k) as e, engine(H, k) as ef, engine(H, k) as et:
        load_filter(ef, solid)
        et.prefilter_begin(2, LOG2_CELLS)
        e.sketch_begin(SKETCH_P)

        def reset():
            e.clear(); e.sketch_drop(); e.sketch_begin(SKETCH_P)
            ef.reset_counts()
            et.prefilter_drop(); et.prefilter_begin(2, LOG2_CELLS)

        def observe():
            return (table(e), e.stats()[2]), table(ef), et.prefilter_export(), e.sketch_registers()

        # control: the same sequence with host synchronisations around every step
        import time
        t_app = 0.0
        for j in range(N_BATCHES - 1):
            t0 = time.perf_counter()
            H.control(B.inputs(j), {}, lambda p, j=j: spc.append_dev(p["packed"], p["invalid"], B.true[j][2], S1.cuda_stream))
            t_app = max(t_app, time.perf_counter() - t0)
        t0 = time.perf_counter()
        spc.replay(ef, spc.COUNT_FILTERED); spc.replay(et, spc.TALLY); spc.sketch(e); spc.replay(e, spc.COUNT)
        torch.cuda.synchronize()
        t_rep = time.perf_counter() - t0
        same_segments(spc, B.segments(N_BATCHES - 1), "spool control: segments vs model")
        ctl = observe()
        # contract
        reset()
        runs = append_all(H, sp, (S1, S2), N_BATCHES - 1, t_call=max(t_app, t_rep))
        pending = lambda: not any(ev.query() for ev in runs[-1].produced)   # the last append's producer has not run yet
        sp.replay(ef, sp.COUNT_FILTERED)
        sp.replay(et, sp.TALLY)
        sp.sketch(e)
        early_light = pending()                      # modes 1 and 2 and the sketch call entry points that do not synchronise
        sp.replay(e, sp.COUNT)
        early_replay = pending()                     # mode 0 is as synchronous as the count it calls
        last = append_all(H, sp, (S1, S2), N_BATCHES, first=N_BATCHES - 1, t_call=t_app)      # behind the replays: must not be counted
        got = observe()
        for j, r in enumerate(runs + last):
            H.records.append((f"spool_append_dev[{tier}] batch {j} k={k}", NO_SYNC, t_app, r.host_s, r.delay_ms, r.early))
        H.records.append((f"spool_replay[{tier}] modes 1, 2, sketch k={k}", NO_SYNC if tier == "hbm" else SYNCS, t_rep, 0.0, runs[-1].delay_ms, early_light))
        H.records.append((f"spool_replay[{tier}] mode 0 k={k}", count_class(k) if tier == "hbm" else SYNCS, t_rep, 0.0, runs[-1].delay_ms, early_replay))
        same(got, want, f"spool[{tier}]: contract run vs truth")
        same(ctl, want, f"spool[{tier}]: control run vs truth")
        same_segments(sp, B.segments(N_BATCHES), f"spool[{tier}] contract: segments vs model")
        assert sp.stat("hbm_bytes" if tier == "host" else "host_bytes") == 0
        assert H.expected == (count_class(k) if tier == "hbm" else SYNCS)
        H.class_checked = True
        assert all(r.early for r in runs + last), "kdf_spool_append_dev: an append returned after its producer had run"
        if tier == "hbm":
            assert early_light, "kdf_spool_replay modes 1, 2 / kdf_spool_sketch (HBM tier): returned after the appends' producers had run"
            assert early_replay is (count_class(k) == NO_SYNC), "kdf_spool_replay mode 0 (HBM tier): not as synchronous as the count it calls"
        else:                                        # (the host waits for the last append: the uploads read host memory)
            assert early_light is False and early_replay is False
        del runs, last


def case_spool_reads(H, k):
    """the same with read offsets: read_hits, read_depth and select_reads of the spool, at once behind the appends"""
    import torch
    w, T, B = world(), truth(k), batches()
    S1, S2 = H.independent_stream(), H.independent_stream()
    nr = len(w.reads)
    rows, _, _ = hit_mask(w, T, T.solid)
    depth = DT.depth_rows(w.reads, k, T.solid, 2, keys=T.read_keys)
    sel = np.flatnonzero(rows[:, 1] >= 3).astype(np.int64)
    assert 0 < len(sel) < nr
    with spool() as spc, spool() as sp, engine(H, k) as e:           # (a spool of its own for the control: see case_spool)
        load_table(e, T.solid)

        def consume(sp, pending=None):
            with torch.cuda.stream(H.S):
                hits = torch.zeros(nr, dtype=torch.int64, device=H.dev)
                dep = torch.zeros(nr * 6, dtype=torch.int64, device=H.dev)
                out = torch.zeros(nr, dtype=torch.int64, device=H.dev)
            H.S.synchronize()
            sp.read_depth_dev(e, 2, dep.data_ptr())              # (does not synchronise: kdf_read_depth_dev per segment)
            early.append(None if pending is None else pending())
            sp.read_hits_dev(e, hits.data_ptr())
            e.synchronize()
            rc, n = sp.select_reads_dev(hits.data_ptr(), 3, out.data_ptr(), nr)
            assert rc == 0
            torch.cuda.synchronize()
            return (hits.cpu().numpy().view(np.uint32).reshape(nr, 2), dep.cpu().numpy().view(np.uint64).reshape(nr, 6), out[:n].cpu().numpy())
        import time
        early = []
        t0 = time.perf_counter()
        for j in range(N_BATCHES):
            H.control(B.inputs(j, True), {}, lambda p, j=j: spc.append_dev(p["packed"], p["invalid"], B.true[j][2], S1.cuda_stream, p["offsets"], len(B.reads[j])))
        ctl = consume(spc)
        t_all = time.perf_counter() - t0
        runs = append_all(H, sp, (S1, S2), N_BATCHES, offsets=True, t_call=t_all)
        got = consume(sp, lambda: not any(ev.query() for ev in runs[-1].produced))
        for j, r in enumerate(runs):
            H.records.append((f"spool_append_reads_dev batch {j} k={k}", NO_SYNC, t_all, r.host_s, r.delay_ms, r.early))
        H.records.append((f"spool_read_depth k={k}", NO_SYNC, t_all, 0.0, runs[-1].delay_ms, early[-1]))
        want = (rows, depth, sel)
        same(got, want, "spool reads: contract run vs truth")
        same(ctl, want, "spool reads: control run vs truth")
        assert sp.n_reads == nr
        assert H.expected == NO_SYNC
        H.class_checked = True
        assert all(r.early for r in runs), "kdf_spool_append_reads_dev: an append returned after its producer had run"
        assert early[-1] is True, "kdf_spool_read_depth: returned after the appends' producers had run"
        del runs


def case_spool_append_uploaded(H, k):
    """append_uploaded behind a delayed engine stream; the slot keeps its batch and is counted, the spool replays into another engine"""
    import torch
    T = truth(k)
    halves = _halves(k)
    pb, (b0, b1) = _pinned(halves)
    want_seg = SM.segments([(h[0], h[1], h[2]) for h in halves], SEG)
    try:
        with spool() as spc, spool() as spx, engine(H, k) as e, engine(H, k, stream=H.independent_stream()) as e2:
            def sequence(contract, ms):
                sp = spx if contract else spc             # (a spool of its own for the control: see case_spool)
                e.clear(); e2.clear()
                torch.cuda.synchronize()
                e.upload_async(0, b0)
                e.upload_async(1, b1)
                gate = _gate(H, ms) if contract else None
                sp.append_uploaded(e, 0)
                e.count_uploaded(0)
                sp.append_uploaded(e, 1)
                e.count_uploaded(1)
                sp.replay(e2, sp.COUNT)
                early = None if gate is None else not gate.query()
                if not contract:
                    torch.cuda.synchronize()
                return early
            import time
            t0 = time.perf_counter()
            sequence(False, 0)
            t_call = time.perf_counter() - t0
            ctl = (table(e), table(e2))
            same_segments(spc, want_seg, "append_uploaded control: segments vs model")
            ms = max(20.0, 4e3 * t_call)
            early = sequence(True, ms)
            got = (table(e), table(e2))
            H.records.append((f"spool_append_uploaded k={k}", NO_SYNC, t_call, 0.0, ms, early))
            same(got, (T.counts, T.counts), "append_uploaded: contract run vs truth")
            same(ctl, (T.counts, T.counts), "append_uploaded: control run vs truth")
            same_segments(spx, want_seg, "append_uploaded contract: segments vs model")
            assert H.expected == NO_SYNC
            H.class_checked = True
            assert early is True, "kdf_spool_append_uploaded / kdf_spool_replay: returned after the delay on the engine's stream had run"
    finally:
        pb.close()


# ------------------------------------------------------------------------------------------------ the table

# The class of the entry points whose ordering the header leaves unstated, decided by what the call must do (each is
# also named in its comment in include/kdf.h):
#   - calls that insert caller keys learn on the host whether a bucket overflowed (kdf_add_pairs*_dev, kdf_load_filter*_dev)
#     or whether a key was not stored (kdf_set_counts*_dev): they synchronise;
#   - kdf_query*_dev, kdf_count_reads_filtered_dev and kdf_read_depth_dev only queue work: stream order, no synchronisation.
CLASS = {
    "kdf_add_pairs_dev": SYNCS, "kdf_add_pairs_multi_dev": SYNCS, "kdf_load_filter_dev": SYNCS, "kdf_set_counts_dev": SYNCS,
    "kdf_query_dev": NO_SYNC, "kdf_count_reads_filtered_dev": NO_SYNC, "kdf_read_depth_dev": NO_SYNC,
}

Case = collections.namedtuple("Case", "name entry_points cls ks fn args")


def _c(name, entry_points, cls, ks, fn, *args):
    return Case(name, tuple(entry_points), cls, tuple(ks), fn, args)


CASES = [
    # stream consumers
    _c("count_dev[pending]", ["kdf_count_reads_dev"], NO_SYNC, SHORT, case_count_dev, "pending"),
    _c("count_dev[long keys]", ["kdf_count_reads_dev"], SYNCS, (65,), case_count_dev, "pending"),
    _c("count_dev[direct]", ["kdf_count_reads_dev"], SYNCS, KS, case_count_dev, "direct"),
    _c("count_dev[binned]", ["kdf_count_reads_dev"], NO_SYNC, SHORT, case_count_dev, "binned"),
    _c("count_dev[in_place]", ["kdf_count_reads_dev"], NO_SYNC, SHORT, case_count_dev, "in_place"),
    _c("count_dev[lazy binned]", ["kdf_count_reads_dev", "kdf_export_ge_dev"], NO_SYNC, SHORT, case_count_dev_lazy, "binned"),
    _c("count_dev[lazy in_place]", ["kdf_count_reads_dev", "kdf_export_ge_dev"], NO_SYNC, SHORT, case_count_dev_lazy, "in_place"),
    _c("count_filtered_dev[direct]", ["kdf_count_reads_filtered_dev"], CLASS["kdf_count_reads_filtered_dev"], KS, case_count_filtered_dev, "direct"),
    _c("count_filtered_dev[sieve]", ["kdf_count_reads_filtered_dev"], CLASS["kdf_count_reads_filtered_dev"], SHORT, case_count_filtered_dev, "sieve"),
    _c("count_filtered_dev[bin_sieve]", ["kdf_count_reads_filtered_dev"], CLASS["kdf_count_reads_filtered_dev"], SHORT, case_count_filtered_dev, "bin_sieve"),
    _c("count_filtered_dev[long_sieve]", ["kdf_count_reads_filtered_dev"], CLASS["kdf_count_reads_filtered_dev"], (65,), case_count_filtered_dev, "long_sieve"),
    _c("prefilter_add_dev (then arm and the gated count_dev, whose class is count_class(k))", ["kdf_prefilter_add_reads_dev", "kdf_count_reads_dev"], NO_SYNC, KS, case_prefilter),
    _c("sketch_add_dev", ["kdf_sketch_add_reads_dev"], NO_SYNC, KS, case_sketch_add_dev),
    _c("scan_dev[direct]", ["kdf_scan_reads_dev"], NO_SYNC, KS, case_scan_dev, "direct"),
    _c("scan_dev[sieve]", ["kdf_scan_reads_dev"], NO_SYNC, SHORT, case_scan_dev, "sieve"),
    _c("scan_dev[long_sieve]", ["kdf_scan_reads_dev"], NO_SYNC, (65,), case_scan_dev, "long_sieve"),
    _c("window_counts_dev", ["kdf_window_counts_dev"], NO_SYNC, KS, case_window_counts_dev),
    _c("read_depth_dev", ["kdf_read_depth_dev"], CLASS["kdf_read_depth_dev"], KS, case_read_depth_dev),
    _c("hit_keys_dev", ["kdf_hit_keys_dev"], NO_SYNC, KS, case_hit_keys_dev),
    # key-array consumers
    _c("add_pairs_dev[lds]", ["kdf_add_pairs_dev"], CLASS["kdf_add_pairs_dev"], SHORT, case_add_pairs_dev, "lds"),
    _c("add_pairs_dev[atomic]", ["kdf_add_pairs_dev", "kdf_add_pairs_w_dev"], CLASS["kdf_add_pairs_dev"], KS, case_add_pairs_dev, "atomic"),
    _c("add_pairs_multi_dev[bucket_order]", ["kdf_add_pairs_multi_dev", "kdf_export_parts_dev"], CLASS["kdf_add_pairs_multi_dev"], SHORT, case_add_pairs_multi_dev, "bucket_order"),
    _c("add_pairs_multi_dev[shuffled]", ["kdf_add_pairs_multi_dev"], CLASS["kdf_add_pairs_multi_dev"], SHORT, case_add_pairs_multi_dev, "shuffled"),
    _c("load_filter_dev", ["kdf_load_filter_dev", "kdf_load_filter_w_dev"], CLASS["kdf_load_filter_dev"], KS, case_load_filter_dev),
    _c("query_dev", ["kdf_query_dev", "kdf_query_w_dev"], CLASS["kdf_query_dev"], KS, case_query_dev),
    _c("set_counts_dev", ["kdf_set_counts_dev", "kdf_set_counts_w_dev"], CLASS["kdf_set_counts_dev"], KS, case_set_counts_dev),
    _c("prefilter_merge_dev", ["kdf_prefilter_merge_dev"], NO_SYNC, (31,), case_prefilter_merge_dev),
    _c("format_kmers_dev", ["kdf_format_kmers_dev"], NO_SYNC, KS, case_format_kmers_dev),
    _c("variant_evidence_dev", ["kdf_variant_evidence_dev"], NO_SYNC, KS, case_variant_evidence_dev),
    # synchronising entry points
    _c("read_hits_dev", ["kdf_read_hits_dev"], SYNCS, KS, case_read_hits_dev),
    _c("hit_list_dev", ["kdf_hit_list_dev"], SYNCS, (31,), case_hit_list_dev),
    _c("hit_coverage_dev", ["kdf_hit_coverage_dev"], SYNCS, (31,), case_hit_coverage_dev),
    _c("coverage_list_dev", ["kdf_coverage_list_dev"], SYNCS, (31,), case_coverage_list_dev),
    _c("variant_windows_dev", ["kdf_variant_windows_dev"], SYNCS, (31,), case_variant_windows_dev),
    _c("cluster_intervals_dev", ["kdf_cluster_intervals_dev"], SYNCS, (31,), case_cluster_intervals_dev),
    _c("group_distinct_dev", ["kdf_group_distinct_dev"], SYNCS, KS, case_group_distinct_dev),
    _c("export_ge_dev[sorted]", ["kdf_export_ge_dev", "kdf_export_ge_w_dev"], SYNCS, KS, case_export_ge_dev, "sorted"),
    _c("export_ge_dev[unsorted]", ["kdf_export_ge_dev", "kdf_export_ge_w_dev"], SYNCS, KS, case_export_ge_dev, "unsorted"),
    _c("export_ge_dev[fused]", ["kdf_export_ge_dev"], SYNCS, SHORT, case_export_ge_dev, "fused"),
    _c("export_parts_w_packed_dev", ["kdf_export_parts_w_packed_dev"], SYNCS, (65,), case_export_parts_w_packed_dev),
    _c("export_parts_dev", ["kdf_export_parts_dev"], SYNCS, SHORT, case_export_parts_dev, "arrays"),
    _c("export_parts_packed_dev", ["kdf_export_parts_packed_dev"], SYNCS, SHORT, case_export_parts_dev, "packed"),
    _c("histogram_dev", ["kdf_histogram_dev"], SYNCS, KS, case_histogram_dev),
    _c("prefilter_export_dev", ["kdf_prefilter_export_dev"], SYNCS, KS, case_prefilter_export_dev),
    _c("sketch_registers_dev", ["kdf_sketch_registers_dev"], SYNCS, KS, case_sketch_registers_dev),
    _c("parse_kmer_fasta_dev", ["kdf_parse_kmer_fasta_dev"], SYNCS, KS, case_parse_kmer_fasta_dev),
    _c("fasta_pack_dev", ["kdf_fasta_pack_dev"], SYNCS, (31,), case_fasta_pack_dev),
    _c("bgzf_inflate_dev", ["kdf_bgzf_inflate_dev"], SYNCS, (31,), case_bgzf_inflate_dev),
    _c("bamdev_decode_dev", ["kdf_bamdev_decode_dev"], SYNCS, (31,), case_bamdev_decode_dev),
    # two engines
    _c("export_join_dev / count_join", ["kdf_export_join_dev", "kdf_export_join_w_dev", "kdf_count_join"], SYNCS, KS, case_join),
    # upload slots
    _c("count_uploaded[same stream]", ["kdf_count_uploaded", "kdf_upload_reads_async"], NO_SYNC, SHORT, case_count_uploaded, False),
    _c("count_uploaded[same stream, long keys]", ["kdf_count_uploaded", "kdf_upload_reads_async"], SYNCS, (65,), case_count_uploaded, False),
    _c("count_uploaded[moved]", ["kdf_count_uploaded", "kdf_upload_reads_async"], NO_SYNC, (31,), case_count_uploaded, True),
    _c("tally and sketch uploaded", ["kdf_prefilter_add_uploaded", "kdf_sketch_add_uploaded"], NO_SYNC, KS, case_tally_sketch_uploaded),
    # spool
    _c("spool[hbm]", ["kdf_spool_append_dev", "kdf_spool_replay", "kdf_spool_sketch"], NO_SYNC, SHORT, case_spool, "hbm"),
    _c("spool[hbm, long keys]", ["kdf_spool_append_dev", "kdf_spool_replay", "kdf_spool_sketch"], SYNCS, (65,), case_spool, "hbm"),
    _c("spool[host]", ["kdf_spool_append_dev", "kdf_spool_replay", "kdf_spool_sketch"], SYNCS, (31,), case_spool, "host"),
    _c("spool reads", ["kdf_spool_append_reads_dev", "kdf_spool_read_hits", "kdf_spool_read_depth", "kdf_spool_select_reads"], NO_SYNC, (31, 65), case_spool_reads),
    _c("spool append_uploaded", ["kdf_spool_append_uploaded", "kdf_spool_replay"], NO_SYNC, (31,), case_spool_append_uploaded),
]

# Entry points of the header without a contract case, each with its reason.
EXCLUDED = {
    "kdf_spool_append_uploaded_reads": "kdf_spool_append_uploaded plus a host offsets array copied before return; the device side is kdf_spool_append_reads_dev's",
    "kdf_spool_segment_dev": "waits on the host for the last append and launches nothing",
}


def _params():
    for c in CASES:
        for k in c.ks:
            yield pytest.param(c, k, id=f"{c.name}-k{k}")


@pytest.mark.parametrize("case, k", list(_params()))
def test_stream_order(H, case, k):
    H.expected, H.class_checked = case.cls, False
    case.fn(H, k, *case.args)
    assert H.class_checked, "the case never compared its class with the table's"
