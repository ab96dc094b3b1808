"""Model-based lifetime test: a seeded sequence of API calls on ONE long-lived engine, compared call by call with the
plain-Python model (tests/engine_model.py, sequences from tests/engine_ops.py).

Every other GPU test creates an engine, feeds it by a fixed script, checks it and destroys it.  Here the ORDER of the
calls is what varies: count / count --if (host, device, uploaded), add_pairs and the multi-segment merge, set_counts,
load_filter, reset_counts, clear, reserve, flush, option changes in the middle of a life, prefilter cycles, set_stream,
API refusals -- and after every call whatever it returned (a value or a KdfError code) must equal the model's, bit for
bit.  ``kdf_get_stat`` witnesses, accumulated over the seeds of a family, assert that the hardware paths behind the
orders really ran (binned passes pending at a clear, the LDS merge, the sieve scan, the fused dump, a re-bucketed and a
grown live table, a flush that was the clear).  The named fixed scripts at the end write out by hand the orders the
seeds are aimed at, so that they stay covered whatever the seeds are.

Wall time on the MI355X, beside tests/test_gpu_fuzz.py from the same run: DESIGN.md section 6, the paragraph "One
engine, many calls in a drawn order".
"""
import numpy as np
import pytest

import engine_model as EM
import engine_ops as EO
import kmer_truth as KT
import depth_truth as DT

pytestmark = pytest.mark.gpu

SEEDS = {"narrow": (11, 22, 33), "wide": (11, 22, 33), "long": (11, 22, 33)}
N_OPS = {"narrow": 220, "wide": 220, "long": 200}
WITNESSES = {}          # family -> set of witness names, accumulated over its seeds (asserted by test_witnesses)

SHORT_WITNESSES = {"binned_passes grew", "pending_passes > 0 before clear", "pending_passes > 0 before load_filter",
                   "pending_passes > 0 before reset_counts", "last_count_path 0", "last_count_path 1", "last_count_path 3",
                   "last_merge_path 1", "last_merge_path 2", "last_scan_path 0", "last_scan_path 3", "fused_dumps grew",
                   "bucket_bits changed with distinct > 0", "log2cap grew with distinct > 0", "flushes grew on a cleared table"}
LONG_WITNESSES = {"last_count_path 0", "last_scan_path 0", "log2cap grew with distinct > 0"}


class Runner:
    """one engine + its model; ``run(op)`` performs an op on both and asserts that they agree"""

    def __init__(self, k, capacity_hint=1 << 16, tag="", witnesses=None):
        import torch
        from kmer_denovo_filter_amd import KmerEngine
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.k, self.tag = k, tag
        self.e = KmerEngine(k, capacity_hint=capacity_hint)
        self.m = EM.EngineModel(k)
        self.long, self.wide = self.e.long, self.e.wide
        self.W = self.e.key_words
        self.keep = []                       # device tensors handed to the engine, alive until it has synchronised
        self.pinned = None                   # reads.PinnedBatches: one page-locked buffer per upload slot
        self.m_slot_full = [False, False]    # a pinned buffer was handed to upload_async (cleared by a synchronise)
        self.prev_pending = 0                # stat pending_positions after the previous op
        self.stream = torch.cuda.Stream()
        self.log = []
        self.wit = witnesses if witnesses is not None else set()
        self.seen_distinct = 0               # the engine's last reported `distinct` (0 again after clear / load_filter)
        self.fresh = False                   # cleared, and nothing but count calls, option changes and flushes since
        self.stat = {n: self.e.get_stat(n) for n in ("log2cap", "bucket_bits", "flushes", "binned_passes", "fused_dumps")}

    def close(self):
        self.e.synchronize()
        self.keep.clear()
        self.e.close()
        if self.pinned is not None:
            self.pinned.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- arguments -----------------------------------------------------------------------------------------------------
    def t(self, a):
        """a numpy array of 64- or 32-bit words as a device tensor (kept alive)"""
        a = np.ascontiguousarray(a)
        view = {8: np.int64, 4: np.int32}[a.dtype.itemsize]
        x = self.torch.from_numpy(a.view(view).copy()).to(self.dev)
        self.keep.append(x)
        return x

    def zeros(self, n, dtype):
        x = self.torch.zeros(max(int(n), 1), dtype=dtype, device=self.dev)
        self.keep.append(x)
        return x

    def ready(self):
        self.torch.cuda.synchronize()        # the tensors were written on torch's stream: complete before the engine reads them

    def stream_of(self, reads):
        from kmer_denovo_filter_amd import ReadStream
        return ReadStream.from_strings(reads)

    PINNED_BASES = 1 << 19

    def pinned_stream(self, op):
        """the batch in the page-locked buffer of its slot: upload_async returns at once and the copy runs on the engine's
        copy stream, ordered against the count by the slot's events alone (also across a set_stream in between).  The
        buffer is not touched again before the slot's batch was taken or the engine has synchronised."""
        from kmer_denovo_filter_amd.reads import PinnedBatches, ReadStream
        s = self.stream_of(op["reads"])
        assert s.n_bases <= self.PINNED_BASES, s.n_bases
        if self.pinned is None:
            self.pinned = PinnedBatches(2, self.PINNED_BASES)
        slot = op["slot"]
        if self.m_slot_full[slot]:
            self.e.synchronize()                             # an earlier copy out of this buffer may still be in flight
        packed, invalid = self.pinned.batches[slot]
        packed[:len(s.packed)] = s.packed
        invalid[:len(s.invalid)] = s.invalid
        self.m_slot_full[slot] = True
        return ReadStream(packed[:len(s.packed)], invalid[:len(s.invalid)], s.n_bases, s.offsets)

    def dev_stream(self, reads):
        """torch buffers of exactly stream_words size"""
        s = self.stream_of(reads)
        p, i = self.t(s.packed), self.t(s.invalid)
        self.ready()
        return p.data_ptr(), i.data_ptr(), s.n_bases

    def key_arrays(self, keys):
        """-> (lo or rows, hi or None) numpy arrays in the engine's layout"""
        if self.long:
            return KT.rows(keys, self.W), None
        lo, hi = KT.lohi(keys)
        return lo, (hi if self.wide else None)

    def dev_keys(self, keys):
        lo, hi = self.key_arrays(keys)
        if not len(keys):
            return None, None
        tl = self.t(lo)
        th = self.t(hi) if hi is not None else None
        return tl.data_ptr(), (th.data_ptr() if th is not None else None)

    def keys_from(self, lo, hi):
        if self.long:
            return [KT.int_of_row(r) for r in lo]
        return [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), (hi if hi is not None else np.zeros(len(lo), np.uint64)).tolist())]

    # ---- the calls -----------------------------------------------------------------------------------------------------
    def call(self, op):
        e, n = self.e, op["op"]
        if n in ("count", "count_filtered", "pf_add"):
            host = {"count": e.count, "count_filtered": e.count_filtered, "pf_add": e.prefilter_add}[n]
            devf = {"count": e.count_dev, "count_filtered": e.count_filtered_dev, "pf_add": e.prefilter_add_dev}[n]
            if op["form"] == "host":
                host(self.stream_of(op["reads"]))
            else:
                devf(*self.dev_stream(op["reads"]))
        elif n == "upload":
            e.upload_async(op["slot"], self.pinned_stream(op) if op.get("pinned") else self.stream_of(op["reads"]))
        elif n == "count_uploaded":
            e.count_uploaded(op["slot"], op["filtered"])
        elif n == "pf_add_uploaded":
            e.prefilter_add_uploaded(op["slot"])
        elif n == "add_pairs":
            if op["form"] == "host":
                keys, counts = op["segs"][0]
                lo, hi = self.key_arrays(keys)
                e.add_pairs(lo, hi, None if counts is None else np.array(counts, np.uint32))
            elif op["form"] == "dev":
                keys, counts = op["segs"][0]
                dl, dh = self.dev_keys(keys)
                dc = self.t(np.array(counts, np.uint32)).data_ptr() if counts is not None and len(keys) else None
                self.ready()
                e.add_pairs_dev(dl, dh, dc, len(keys))
            else:
                segs = []
                for keys, counts in op["segs"]:
                    dl, dh = self.dev_keys(keys)
                    segs.append((dl, dh, self.t(np.array(counts, np.uint32)).data_ptr() if len(keys) else None, len(keys)))
                self.ready()
                e.add_pairs_multi_dev(segs)
        elif n == "set_counts":
            dl, dh = self.dev_keys(op["keys"])
            dc = self.t(np.array(op["counts"], np.uint32)).data_ptr()
            self.ready()
            e.set_counts_dev(dl, dh, dc, len(op["keys"]))
        elif n == "load_filter":
            if op["form"] == "host":
                lo, hi = self.key_arrays(op["keys"])
                e.load_filter(lo, hi)
            else:
                dl, dh = self.dev_keys(op["keys"])
                self.ready()
                e.load_filter_dev(dl, dh, len(op["keys"]))
        elif n in ("reset_counts", "clear", "flush"):
            getattr(e, n)()
        elif n == "reserve":
            e.reserve(op["n"])
        elif n == "option":
            e.set_option(op["name"], op["value"])
        elif n == "set_stream":
            e.set_stream(self.stream.cuda_stream if op["own"] else None)
        elif n == "pf_begin":
            e.prefilter_begin(op["L"], op["s"])
        elif n == "pf_arm":
            e.prefilter_arm()
        elif n == "pf_drop":
            e.prefilter_drop()
        else:
            assert n == "obs", n
            return self.observe(op)
        return None

    def observe(self, op):
        e, kind, torch = self.e, op["kind"], self.torch
        if kind == "stats":
            _, d, w = e.stats()
            self.seen_distinct = d
            return d, w
        if kind == "count_ge":
            return e.count_ge(op["m"])
        if kind == "export_ge":
            lo, hi, cnt = e.export_ge(op["m"])
            return self.keys_from(lo, hi), cnt
        if kind == "export_ge_dev":
            # (sized by the MODEL: a count_ge here would flush what is pending, and the fused dump is written by that flush)
            cap = self.m.count_ge(op["m"]) + 8
            dl = self.zeros(cap * (self.W if self.long else 1), torch.int64)
            dh = self.zeros(cap, torch.int64) if self.wide and not self.long else None
            dc = self.zeros(cap, torch.int32)
            self.ready()
            n = e.export_ge_dev(op["m"], dl.data_ptr(), dh.data_ptr() if dh is not None else None, dc.data_ptr(), cap, sorted_=op["sorted"])
            assert n <= cap, f"{n} entries for a buffer of {cap}"
            lo = dl.cpu().numpy().view(np.uint64)
            cnt = dc[:n].cpu().numpy().view(np.uint32)
            if self.long:
                keys = self.keys_from(lo[:n * self.W].reshape(n, self.W), None)
            else:
                keys = self.keys_from(lo[:n], dh[:n].cpu().numpy().view(np.uint64) if dh is not None else None)
            if not op["sorted"]:
                o = sorted(range(n), key=lambda i: keys[i])
                keys, cnt = [keys[i] for i in o], cnt[o] if n else cnt
            return keys, cnt
        if kind == "histogram":
            return e.histogram(op["high"])
        if kind == "histogram_dev":
            d = self.zeros(op["high"] + 2, torch.int64)
            self.ready()
            e.histogram_dev(op["high"], d.data_ptr())
            return d.cpu().numpy().view(np.uint64)[:op["high"] + 2]
        if kind == "count_stats":
            return e.count_stats()
        if kind == "query":
            lo, hi = self.key_arrays(op["keys"])
            return e.query(lo, hi)
        if kind == "pf_fill":
            return e.prefilter_fill()
        s = self.stream_of(op["reads"])
        if kind == "scan":
            return e.scan(s)
        if kind == "window_counts":
            counts, valid = e.window_counts(s, want_valid=True)
            return counts, DT.bits(valid, s.n_bases)
        assert kind == "read_depth", kind
        return e.read_depth(s, op["low_max"])

    # ---- one op on both sides --------------------------------------------------------------------------------------------
    def run(self, op):
        from kmer_denovo_filter_amd._native import KdfError
        e = self.e
        idx = len(self.log)
        self.log.append(EO.describe(op))
        cls = EO.op_class(op)
        if cls in ("clear", "load_filter", "reset_counts") and e.get_stat("pending_passes") > 0:
            self.wit.add(f"pending_passes > 0 before {cls}")
        if op["op"] == "option" and op["name"] == "big_bucket_log2cap":
            self.seen_distinct = e.stats()[1]                # (set_option flushes what is pending anyway)
        want = EO.apply(self.m, op)
        try:
            got = ("ok", self.call(op))
        except KdfError as ex:
            if ex.code == 2:                                  # KDF_ERR_HIP: the device is in doubt -- nothing more runs on it
                pytest.exit(f"{self.tag} k={self.k} op {idx} {self.log[-1]}: {ex}", returncode=3)
            got = ("err", ex.code)
        why = differ(want, got)
        if why:
            last = "\n    ".join(f"[{idx - len(self.log[-12:]) + 1 + i}] {l}" for i, l in enumerate(self.log[-12:]))
            raise AssertionError(f"{self.tag} k={self.k} op {idx} {self.log[-1]}: {why}\n  last ops:\n    {last}")
        self.witness(op, cls, got[0] == "ok")

    def witness(self, op, cls, ok):
        e, wit = self.e, self.wit
        now = {n: e.get_stat(n) for n in self.stat}
        if ok and cls in ("count", "count_filtered"):
            wit.add(f"last_count_path {e.get_stat('last_count_path')}")
        if ok and cls == "add_pairs" and sum(len(a) for a, _ in op["segs"]):
            wit.add(f"last_merge_path {e.get_stat('last_merge_path')}")
        if ok and cls == "observe" and op["kind"] == "scan":
            wit.add(f"last_scan_path {e.get_stat('last_scan_path')}")
        if now["binned_passes"] > self.stat["binned_passes"]:
            wit.add("binned_passes grew")
        if now["fused_dumps"] > self.stat["fused_dumps"]:
            wit.add("fused_dumps grew")
        if cls in ("clear", "load_filter") and ok:
            self.seen_distinct = 0
        if self.seen_distinct > 0 and now["bucket_bits"] != self.stat["bucket_bits"] and now["log2cap"] == self.stat["log2cap"]:
            wit.add("bucket_bits changed with distinct > 0")
        if self.seen_distinct > 0 and now["log2cap"] > self.stat["log2cap"]:
            wit.add("log2cap grew with distinct > 0")
        # `fresh` <=> the engine's table is still only LOGICALLY empty: kdf_clear came, and since then nothing has written
        # or materialized it.  Count calls keep it as long as their work stays pending (stream or ring); option changes,
        # flush, reserve and set_stream keep it when nothing was pending (they flush, and a flush through the direct
        # kernels memsets the table first); every reader and every other mutator ends it.  A kernel-C flush (stat
        # "flushes") that happens while `fresh` holds is the flush that WAS the clear (nonempty = 0): the witness.
        grew = now["flushes"] > self.stat["flushes"]
        if self.fresh and grew:
            wit.add("flushes grew on a cleared table")
        if cls == "clear" and ok:
            self.fresh = True
        elif grew:
            self.fresh = False
        elif cls == "count":                                  # still pending (stream or ring): the table is untouched
            self.fresh = self.fresh and e.get_stat("pending_positions") > 0
        elif cls in ("option", "flush", "reserve", "set_stream"):
            self.fresh = self.fresh and self.prev_pending == 0    # (something pending went through the direct kernels)
        elif cls != "upload":
            self.fresh = False                                # everything else materializes the table
        self.prev_pending = e.get_stat("pending_positions")
        self.stat = now
        if len(self.keep) > 64:
            e.synchronize()
            self.keep.clear()
            self.m_slot_full = [False, False]


def differ(want, got):
    """'' when a call's result equals the model's, else what differs"""
    if want[0] != got[0]:
        return f"model says {want[0]} {want[1] if want[0] == 'err' else ''}, engine {got[0]} {got[1] if got[0] == 'err' else ''}"
    a, b = want[1], got[1]
    if want[0] == "err":
        return "" if a == b else f"refused with code {b}, the model says {a}"
    return _diff(a, b)


def _diff(a, b):
    if a is None:
        return ""
    if isinstance(a, dict):
        return "" if a == b else f"model {a}, engine {b}"
    if isinstance(a, tuple):
        for i, (x, y) in enumerate(zip(a, b)):
            w = _diff(x, y)
            if w:
                return f"[{i}] {w}"
        return ""
    if isinstance(a, np.ndarray):
        b = np.asarray(b)
        if a.shape != b.shape:
            return f"model shape {a.shape}, engine {b.shape}"
        if a.dtype == bool:
            b = b.astype(bool)
        bad = np.nonzero(a.reshape(-1) != b.reshape(-1))[0]
        return "" if not len(bad) else f"{len(bad)} of {a.size} values differ, first at {int(bad[0])}: model {a.reshape(-1)[bad[0]]}, engine {b.reshape(-1)[bad[0]]}"
    if isinstance(a, list) and a and not isinstance(a[0], int):
        return _diff(tuple(a), tuple(b))
    if isinstance(a, list):
        b = list(b)
        if len(a) != len(b):
            return f"model {len(a)} entries, engine {len(b)}"
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                return f"entry {i}: model {x:#x}, engine {y:#x}"
        return ""
    return "" if a == b else f"model {a}, engine {b}"


def run_life(seed, family):
    ops, cov = EO.generate(seed, family, N_OPS[family])
    head = ops[0]
    wit = WITNESSES.setdefault(family, set())
    with Runner(head["k"], head["capacity_hint"], tag=f"seed {seed} family {family}", witnesses=wit) as r:
        for op in ops[1:]:
            r.run(op)
    return cov


@pytest.mark.parametrize("family,seed", [(f, s) for f in SEEDS for s in SEEDS[f]])
def test_life_matches_model(family, seed):
    run_life(seed, family)


@pytest.mark.parametrize("family", list(SEEDS))
def test_witnesses(family):
    """the hardware paths behind the model-side preconditions ran, over the seeds of the family (run after them)"""
    if family not in WITNESSES:                               # (selected alone: the lives have not run in this process)
        for seed in SEEDS[family]:
            run_life(seed, family)
    need = LONG_WITNESSES if family == "long" else SHORT_WITNESSES
    missing = sorted(need - WITNESSES[family])
    assert not missing, f"{family}: witnesses not seen over seeds {SEEDS[family]}: {missing}; seen {sorted(WITNESSES[family])}"


# ---------------------------------------------------------------------------------------------------------------------
# the orders the seeds are aimed at, written out by hand
# ---------------------------------------------------------------------------------------------------------------------

def script(k, kinds, seed=7, capacity_hint=1 << 8):
    """carry out a list of generator kinds (engine_ops._Gen.make) on a fresh engine, checking every call"""
    g = EO._Gen(seed, "narrow" if k <= 32 else "wide" if k <= 63 else "long")
    g.k, g.m = k, EM.EngineModel(k)
    g.long = k > 63
    with Runner(k, capacity_hint, tag=f"script k={k}") as r:
        for kind in kinds:
            op = dict(kind) if isinstance(kind, dict) else g.make(kind)
            assert op is not None, f"{kind} does not apply here"
            if op["op"] == "upload" and op["reads"] is None:
                op["reads"] = g.reads("some")
            g.emit(op)
            r.run(op)
        for kind in ("stats", "export_ge", "histogram", "count_stats"):
            op = g.observer(kind)
            g.emit(op)
            r.run(op)
        return r


def opt(name, value):
    return {"op": "option", "name": name, "value": value}


def dump(m=1, sorted_=True):
    return {"op": "obs", "kind": "export_ge_dev", "m": m, "sorted": sorted_}


@pytest.mark.parametrize("k", [31, 47])
def test_load_filter_at_another_size_and_at_the_same_size(k):
    """load_filter_core reallocates the table when the filter needs another size (no kdf_clear on that way) and clears
    lazily when it does not: both after a count whose clear was still lazy, both followed by histogram and count --if"""
    script(k, ["big_count", "obs:histogram", "clear", "load_filter", "obs:histogram", "count_filtered", "obs:export_ge", "clear",
               "load_filter_empty", "obs:histogram", "obs:export_ge", "clear", "reserve_big", "load_filter", "obs:histogram", "count_filtered"])


@pytest.mark.parametrize("k", [31, 47])
def test_clear_then_first_writer(k):
    """clear, then the LDS merge / a binned flush / reserve + count as the first writer of a table that was re-bucketed
    or grown since its last real write"""
    r = script(k, ["reserve_big", opt("force_path", 2), "big_count", "obs:export_ge", opt("big_bucket_log2cap", 10), "clear",
                   opt("merge_min_pairs", 1), "merge_sorted", "obs:export_ge", "clear", "big_count", "obs:export_ge", "clear",
                   {"op": "reserve", "n": 1 << 17}, "count", "obs:export_ge", opt("big_bucket_log2cap", 31), "clear", "merge_shuffled"])
    assert {"last_merge_path 1", "last_merge_path 2", "binned_passes grew", "flushes grew on a cleared table"} <= r.wit, sorted(r.wit)


@pytest.mark.parametrize("k", [21, 63, 65])
def test_clear_then_reader(k):
    """a reader right after clear has to materialize a table that is only logically empty"""
    kinds = []
    for obs in ("obs:export_ge", "obs:histogram", "obs:scan", "obs:window_counts", "obs:read_depth", "obs:export_ge_dev", "obs:query"):
        kinds += ["big_count", "clear", obs]
    script(k, kinds)


@pytest.mark.parametrize("k", [31, 65])
def test_set_stream_between_upload_and_count_and_with_an_armed_prefilter(k):
    script(k, ["upload", "set_stream", "count_uploaded", "obs:export_ge", "upload", "set_stream", "count_uploaded", "obs:export_ge",
               "pf_begin", "upload", "set_stream", "count_uploaded", "pf_add", "pf_arm", "set_stream", "count", "upload", "set_stream",
               "count_uploaded", "obs:export_ge", "obs:pf_fill", "set_stream", "pf_drop"])


@pytest.mark.parametrize("k", [31, 47])
def test_scan_sieve_follows_the_table(k):
    """a scan builds a sieve from an insert-mode table; add_pairs / count add keys, reset_counts zeroes them: every later
    scan must see the table as it is"""
    r = script(k, ["count", "obs:scan", "add_pairs", "obs:scan", "count", "obs:scan", "reset_counts", "obs:scan", "count", "obs:scan",
                   opt("force_path", 1), "obs:scan"])
    assert {"last_scan_path 0", "last_scan_path 3"} <= r.wit, sorted(r.wit)


@pytest.mark.parametrize("k", [31, 47])
def test_add_pairs_into_a_filter_then_count_filtered(k):
    """keys added to a loaded filter are counted by count --if on paths 0 and 2; path 4 (sieve only) is KDF_ERR_STATE until
    a scan has rebuilt the sieve"""
    r = script(k, ["big_count", "load_filter", "add_pairs", opt("force_path", 0), "count_filtered", "obs:query", opt("force_path", 2),
                   "count_filtered", "obs:export_ge", opt("force_path", 4), "count_filtered:refused", "obs:export_ge", "obs:scan",
                   "count_filtered", "obs:export_ge"])
    assert r.m.windows > 0


def test_hash_shift_only_on_an_empty_table():
    """refused while the table holds keys -- also keys whose counts were reset -- and taken after a clear that dropped
    pending work and after a load_filter of zero keys"""
    script(31, ["count", "reset_counts", opt("hash_shift", 1), "obs:stats", "load_filter_empty", opt("hash_shift", 1), "obs:stats",
                opt("hash_shift", 0), "clear", opt("force_path", 2), "big_count", "clear", opt("hash_shift", 2), "count", "obs:export_ge",
                opt("hash_shift", 0), "clear", opt("hash_shift", 0)])


@pytest.mark.parametrize("k", [31, 63, 127])
def test_key_part_changed_between_counts(k):
    """set_option flushes first: without a clear the table holds the union of the slices counted"""
    script(k, [opt("key_parts", 3), "count", opt("key_part", 1), "count", "obs:export_ge", opt("key_part", 2), "big_count", "obs:stats",
               opt("key_parts", 0), "count"])


@pytest.mark.parametrize("then", ["reserve", "big_bucket", "prefilter"])
def test_fused_dump_with_something_before_the_dump(then):
    """fused_dump on, passes pending, and a reserve / a re-bucketing / a prefilter_begin before the dump is asked for"""
    mid = {"reserve": [{"op": "reserve", "n": 1 << 18}], "big_bucket": [opt("big_bucket_log2cap", 10)], "prefilter": ["pf_begin", "pf_arm"]}[then]
    r = script(31, ["reserve_big", opt("force_path", 2), opt("fused_dump", 1), "big_count", dump(1), "big_count"] + mid +
               [dump(2, False), "big_count", dump(1)])
    assert "fused_dumps grew" in r.wit, sorted(r.wit)


# ---- reduced sequences of what the seeded lives found ------------------------------------------------------------------

@pytest.mark.parametrize("k", [32, 63, 65])
def test_reset_counts_in_insert_mode_keeps_the_keys_of_pending_counts(k):
    """found by seed 22 / narrow at op 5: reset_counts dropped the count work that was still pending, so in insert mode
    the keys of those batches never reached the table -- what the table held depended on whether a flush came first"""
    script(k, ["count", "obs:histogram", "big_count", "reset_counts", "obs:histogram", "count", "reset_counts", "count", "obs:export_ge"],
           capacity_hint=1 << 16)


@pytest.mark.parametrize("k", [31, 47, 65, 201])
def test_a_scan_does_not_move_windows(k):
    """found by the long seeds and the scan script: a scan through the direct kernel (force_path 1, every long engine)
    added its valid windows to kdf_stats' `windows`"""
    r = script(k, ["count", "obs:stats", opt("force_path", 1), "obs:scan", "obs:stats", "obs:window_counts", "obs:read_depth", "obs:stats",
                   opt("force_path", 0), "obs:scan", "obs:stats", "reset_counts", "obs:scan", "obs:stats"])
    assert "last_scan_path 0" in r.wit, sorted(r.wit)


@pytest.mark.parametrize("k", [31, 63, 65])
def test_a_refused_count_uploaded_keeps_the_batch(k):
    """found by reading: kdf_count_uploaded refused for the engine's mode used to consume the slot's batch, while the same
    call refused for a tallying prefilter kept it.  Every refusal here is followed by the successful count of the same
    slot (pinned uploads): count with a filter loaded, count --if without one, count while tallying, and for k <= 63 count
    --if under force_path 4 after add_pairs dropped the sieve"""
    up = lambda slot: {"op": "upload", "slot": slot, "reads": None, "pinned": True}
    cu = lambda slot, filtered: {"op": "count_uploaded", "slot": slot, "filtered": filtered}
    kinds = ["count", up(0), "load_filter_some", cu(0, False), "obs:stats", cu(0, True), "obs:export_ge", cu(0, True), "clear",
             up(1), cu(1, True), "obs:stats", cu(1, False), "obs:export_ge",
             "pf_begin", up(0), cu(0, False), "obs:pf_fill", {"op": "pf_add_uploaded", "slot": 0}, "obs:pf_fill", up(0), "pf_arm",
             cu(0, False), "obs:export_ge", "pf_drop"]
    if k <= 63:
        kinds += ["count", "load_filter_some", opt("force_path", 4), up(1), "add_pairs", cu(1, True), "obs:stats", "obs:scan", cu(1, True),
                  "obs:export_ge", opt("force_path", 0)]
    r = script(k, kinds)
    refused = [l for l in r.log if l.startswith("count_uploaded") and "refused=True" in l]
    assert len(refused) == (5 if k <= 63 else 4), r.log           # (one of them the empty slot after the batch was taken)
