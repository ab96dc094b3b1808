"""Seeded generator of API-call sequences for ONE long-lived engine (host only), and ``apply``: what the model says a
call must return.

``generate(seed, family, n_ops)`` -> (ops, coverage).  An op is a dict: ``{"op": name, ...concrete arguments}`` -- read
strings, key lists (Python ints), option values.  Everything is drawn with ``numpy.random.default_rng(seed)`` and by
consulting the ``EngineModel`` alone, so the sequence is the same wherever it is generated.  About a third of the
sequence comes from short MOTIFS (the orders tests/test_gpu_engine_lifetime.py aims at: a clear with work pending, a
merge into a cleared table, a scan around add_pairs, ...), drawn at random points of the life and carried out
against whatever state the life is in; the rest is drawn op by op from weights that depend on the model's mode.

``coverage`` = {"pairs": every (last mutator class, next call class) that occurred, "preconditions": which of
PRECONDITIONS occurred}; tests/test_engine_model.py asserts the required sets per committed seed.
"""
import numpy as np

import engine_model as EM
import kmer_truth as KT
import prefilter_model as PM
from oracle import oracle as O

FAMILIES = {"narrow": (21, 31, 32), "wide": (33, 47, 63), "long": (65, 127, 201)}
SAT = EM.SAT
IUPAC = "RYKMSWBDHV"

PRECONDITIONS = (
    "clear with a count since the last reader",
    "load_filter with a count since the last reader",
    "reset_counts with a count since the last reader",
    "count right after clear",
    "merge right after clear",
    "reserve right after clear",
    "scan after count",
    "scan after add_pairs into a filter table",
    "count_filtered after add_pairs into a filter table",
    "prefilter begun on an engine that has had a filter life",
    "big_bucket_log2cap changed with a non-empty model",
    "key_part changed between count calls without a clear",
)
LONG_PRECONDITIONS = tuple(p for p in PRECONDITIONS if not p.startswith(("merge", "big_bucket")))

OBSERVERS = ("stats", "count_ge", "export_ge", "export_ge_dev", "histogram", "histogram_dev", "count_stats", "query",
             "scan", "window_counts", "read_depth")


def op_class(op):
    """the class of a call in the coverage summary"""
    n = op["op"]
    if n == "obs":
        return "observe"
    if n == "count_uploaded":
        return "count_filtered" if op["filtered"] else "count"
    if n.startswith("pf_"):
        return "prefilter"
    return n


def apply(model, op):
    """Run one op on the model -> ("ok", value) or ("err", KDF_ERR_* code); a refused op leaves the model untouched."""
    try:
        return "ok", _apply(model, op)
    except EM.Refused as r:
        return "err", r.code


def _apply(m, op):
    n = op["op"]
    if n == "count":
        return m.count(op["reads"])
    if n == "count_filtered":
        return m.count_filtered(op["reads"])
    if n == "upload":
        return m.upload(op["slot"], op["reads"])
    if n == "count_uploaded":
        return m.count_uploaded(op["slot"], op["filtered"])
    if n == "add_pairs":
        for keys, counts in op["segs"]:
            m.add_pairs(keys, counts)
        return None
    if n == "set_counts":
        return m.set_counts(op["keys"], op["counts"])
    if n == "load_filter":
        return m.load_filter(op["keys"])
    if n in ("reset_counts", "clear"):
        return getattr(m, n)()
    if n in ("reserve", "flush", "set_stream"):
        return None
    if n == "option":
        return m.set_option(op["name"], op["value"])
    if n == "pf_begin":
        return m.prefilter_begin(op["L"], op["s"])
    if n == "pf_add":
        return m.prefilter_add(op["reads"])
    if n == "pf_add_uploaded":
        return m.prefilter_add_uploaded(op["slot"])
    if n == "pf_arm":
        return m.prefilter_arm()
    if n == "pf_drop":
        return m.prefilter_drop()
    assert n == "obs", n
    k = op["kind"]
    if k == "stats":
        return m.stats()
    if k == "count_ge":
        return m.count_ge(op["m"])
    if k in ("export_ge", "export_ge_dev"):
        return m.export_ge(op["m"])
    if k in ("histogram", "histogram_dev"):
        return m.histogram(op["high"])
    if k == "count_stats":
        return m.count_stats()
    if k == "query":
        return m.query(op["keys"])
    if k == "pf_fill":
        return m.prefilter_fill()
    if k == "scan":
        m.note_scan(op["reads"])
        return m.scan(op["reads"])
    if k == "window_counts":
        return m.window_counts(op["reads"])
    assert k == "read_depth", k
    return m.read_depth(op["reads"], op["low_max"])


def describe(op):
    """one line per op for assert messages: the name, argument SIZES and option values"""
    parts = []
    for key, v in op.items():
        if key == "op":
            continue
        if key == "reads":
            parts.append(f"reads={len(v)}/{sum(len(r) for r in v)}b")
        elif key == "keys":
            parts.append(f"keys={len(v)}")
        elif key == "counts":
            parts.append(f"counts={'None' if v is None else len(v)}")
        elif key == "segs":
            parts.append("segs=[" + ", ".join(f"{len(a)}{'' if c is not None else ' no counts'}" for a, c in v) + "]")
        else:
            parts.append(f"{key}={v}")
    return op["op"] + "(" + ", ".join(parts) + ")"


MOTIFS = {
    "all": [
        ["big_count", "clear", "count", "obs"],
        ["big_count", "reset_counts", "obs:export_ge"],
        ["big_count", "load_filter", "obs:export_ge", "count_filtered", "obs"],
        ["clear", "reserve", "count", "obs:export_ge"],
        ["clear", "obs:export_ge"], ["clear", "obs:histogram"], ["clear", "obs:scan"], ["clear", "obs:window_counts"],
        ["count", "upload:pinned", "set_stream", "count_uploaded", "obs:export_ge", "upload:pinned", "set_stream", "count_uploaded", "obs:export_ge"],
        ["count", "obs:scan", "add_pairs", "obs:scan"],
        ["count", "obs:scan", "count", "obs:scan"],
        ["count", "obs:scan", "reset_counts", "obs:scan", "count", "obs:scan"],
        ["load_filter", "add_pairs", "obs:scan", "add_pairs", "opt:force_path=0", "count_filtered", "obs:query"],
        ["load_filter", "count_filtered", "reset_counts", "count_filtered", "obs:export_ge"],
        ["load_filter", "count_filtered", "clear", "pf_begin", "pf_add", "pf_add", "pf_arm", "set_stream", "count", "count",
         "obs:export_ge", "set_stream", "pf_drop", "obs:stats"],
        ["opt:key_parts=3", "count", "opt:key_part=1", "count", "obs:export_ge", "opt:key_part=2", "count", "obs:export_ge",
         "opt:key_parts=0"],
        ["pf_begin", "pf_add", "clear", "pf_add", "pf_arm", "count", "obs:export_ge", "pf_drop"],
        ["count", "reset_counts", "count", "obs:export_ge"],
        ["count", "load_filter_empty", "obs:stats", "clear"],
        ["load_filter_some", "count_filtered", "count_filtered", "obs"],
        ["opt:defer=0", "opt:binned_min_positions=1024", "count", "obs", "opt:defer=1"],
        ["opt:force_path=1", "count", "obs:scan", "obs:stats", "opt:force_path=0"],
        ["count", "obs:stats", "reserve_huge", "obs:export_ge"],
        ["count", "count", "flush", "obs:stats"],
        ["upload:pinned", "load_filter_some", "count_uploaded:wrong", "count_uploaded", "obs:export_ge", "clear", "upload",
         "count_uploaded:wrong", "count_uploaded", "obs:export_ge"],
        ["pf_begin", "upload:pinned", "count_uploaded:tallying", "count_uploaded", "pf_arm", "obs:pf_fill", "pf_drop"],
        ["count", "refuse", "obs"], ["refuse"], ["refuse"], ["refuse"],
    ],
    "short": [     # k <= 63 only: the binned pipeline, the merge kernels, the sieve, owner tables
        ["reserve_big", "opt:force_path=2", "big_count", "clear", "big_count", "obs:export_ge", "opt:force_path=0"],
        ["reserve_big", "opt:force_path=2", "big_count", "load_filter", "obs:export_ge", "opt:force_path=0"],
        ["reserve_big", "opt:force_path=2", "big_count", "reset_counts", "obs:export_ge", "opt:force_path=0"],
        ["reserve_big", "opt:force_path=2", "opt:fused_dump=1", "big_count", "obs:export_ge_dev", "opt:fused_dump=0", "opt:force_path=0"],
        ["reserve_big", "opt:force_path=2", "opt:fused_dump=1", "big_count", "reserve", "obs:export_ge_dev", "opt:fused_dump=0", "opt:force_path=0"],
        ["reserve_big", "opt:force_path=2", "opt:fused_dump=1", "big_count", "opt:big_bucket_log2cap", "obs:export_ge_dev", "opt:fused_dump=0",
         "opt:force_path=0"],
        ["reserve_big", "opt:force_path=2", "opt:fused_dump=1", "big_count", "pf_begin", "obs:export_ge_dev", "pf_drop", "opt:fused_dump=0",
         "opt:force_path=0"],
        ["clear", "opt:merge_min_pairs=1", "merge_sorted", "obs:export_ge"],
        ["big_count", "opt:big_bucket_log2cap", "clear", "opt:merge_min_pairs=1", "merge_sorted", "obs:export_ge"],
        ["clear", "merge_shuffled", "obs:export_ge"],
        ["count", "opt:big_bucket_log2cap", "obs:export_ge"],
        ["load_filter", "add_pairs", "opt:force_path=2", "count_filtered", "obs:query", "opt:force_path=0"],
        ["load_filter", "add_pairs", "opt:force_path=4", "count_filtered", "obs:query", "opt:force_path=0"],
        ["load_filter_some", "opt:force_path=4", "upload:pinned", "add_pairs", "count_uploaded:refused", "obs:scan", "count_uploaded",
         "obs:export_ge", "opt:force_path=0"],
        ["load_filter", "opt:force_path=4", "count_filtered", "obs:export_ge", "opt:force_path=0"],
        ["load_filter_some", "set_counts", "count_filtered", "obs:export_ge"],
        ["count", "reset_counts", "opt:hash_shift", "obs:stats"],
        ["count", "load_filter_empty", "opt:hash_shift", "count_filtered", "obs:stats", "clear", "opt:hash_shift=0"],
        ["big_count", "clear", "opt:hash_shift", "count", "obs:export_ge", "clear", "opt:hash_shift=0"],
    ],
}


class _Gen:
    def __init__(self, seed, family):
        self.rng = np.random.default_rng(seed)
        self.family = family
        self.k = int(self.rng.choice(FAMILIES[family]))
        self.long = family == "long"
        self.m = EM.EngineModel(self.k)
        glen = 6000 if self.long else 30000
        self.genome = np.frombuffer("".join(self.rng.choice(list("ACGT"), glen)).encode(), np.uint8)
        self.capacity_hint = int(self.rng.choice([1, 1 << 8, 1 << 16]))
        self.ops = []
        self.pairs, self.pre = set(), set()
        self.last_mut = "create"
        self.prev_class = "create"
        self.counts_since_reader = 0
        self.last_count_slice = None          # (key_parts, key_part) of the last count call, None after a clear
        self.own_stream = False
        self.pairs_in_filter = False
        self.huge = 0
        self.queue, self.todo, self.rounds = [], [], 0

    # ---- arguments -----------------------------------------------------------------------------------------------------
    def reads(self, size=None):
        rng, k = self.rng, self.k
        if size is None:
            size = rng.choice(["one", "few", "some", "big"], p=[0.1, 0.35, 0.45, 0.1])
        n = {"one": 1, "few": int(rng.integers(2, 20)), "some": int(rng.integers(30, 300)),
             "big": int(rng.integers(150, 300)) if self.long else int(rng.integers(1500, 4000))}[size]
        max_len = k + 120 if self.long else 160
        out = []
        lens = rng.integers(max(1, k - 3), max_len, n)
        starts = rng.integers(0, len(self.genome) - max_len, n)
        flip = rng.random(n)
        for L, s, f in zip(lens.tolist(), starts.tolist(), flip.tolist()):
            r = self.genome[s:s + L].copy()
            if f < 0.3:                       # lower case, N and IUPAC codes in some reads
                x = rng.random(L)
                r[x < 0.05] |= 0x20
                r[x > 0.995] = ord("N")
                r[(x > 0.99) & (x <= 0.995)] = ord(IUPAC[int(rng.integers(0, len(IUPAC)))])
            s_ = r.tobytes().decode()
            out.append(O.reverse_complement(s_.upper()) if 0.3 <= f < 0.45 else s_)
        if rng.random() < 0.2:
            out += ["A" * int(rng.integers(k, k + 200))] * int(rng.integers(1, 12)) + ["ACGT" * 60] * int(rng.integers(0, 6))
        if rng.random() < 0.25:
            for _ in range(int(rng.integers(1, 4))):
                out.insert(int(rng.integers(0, len(out) + 1)), "")
        return out

    def probe_reads(self):
        n = int(self.rng.integers(1, 25))
        return self.reads("few")[:n] or ["ACGT" * 60]

    def stored(self, n):
        ks = list(self.m.table)
        if not ks or n <= 0:
            return []
        sel = self.rng.choice(len(ks), size=min(n, len(ks)), replace=False)
        return [ks[i] for i in sel.tolist()]

    def new_keys(self, n):
        out = []
        for _ in range(n):                                   # half of them k-mers of the genome: later reads meet them
            if self.rng.random() < 0.5:
                at = int(self.rng.integers(0, len(self.genome) - self.k))
                s = self.genome[at:at + self.k].tobytes().decode()
            else:
                s = "".join(self.rng.choice(list("ACGT"), self.k))
            out.append(KT.key_int(O.canonicalize(s)))
        return out

    def pair_counts(self, n):
        rng = self.rng
        x = rng.random()
        if x < 0.5:
            c = rng.integers(0, 6, n)
        elif x < 0.75:
            c = np.where(rng.random(n) < 0.3, SAT - rng.integers(0, 11, n), rng.integers(0, 4, n))
        else:
            c = np.zeros(n, np.int64)
        return [int(v) for v in c]

    def pairs_keys(self, n):
        n_st = int(self.rng.integers(0, n + 1))
        keys = self.stored(n_st) + self.new_keys(n - n_st)
        keys = list(dict.fromkeys(keys))
        if len(keys) > 1 and self.rng.random() < 0.4:                 # a key twice in one call
            keys += [keys[int(self.rng.integers(0, len(keys)))] for _ in range(int(self.rng.integers(1, 4)))]
        order = self.rng.permutation(len(keys))
        return [keys[i] for i in order.tolist()]

    def hash_order(self, keys, counts):
        h = [(PM.stored_form(key, self.k) << self.m.hash_shift) & PM.M64 for key in keys]
        o = sorted(range(len(keys)), key=lambda i: h[i])
        return [keys[i] for i in o], [counts[i] for i in o]

    # ---- one op of a kind; None when the kind does not apply to the current state ----------------------------------------
    def make(self, kind):
        rng, m = self.rng, self.m
        arg = None
        if ":" in kind:
            kind, arg = kind.split(":", 1)
        form3 = lambda: str(rng.choice(["host", "dev"]))
        if kind in ("count", "big_count"):
            if m.filter_mode or m.pf_state == EM.PF_TALLYING:
                return None
            return {"op": "count", "form": form3(), "reads": self.reads("big" if kind == "big_count" else None)}
        if kind == "count_filtered":
            if not m.filter_mode or (m.force_path == 4 and not m.sieve and arg != "refused"):
                return None
            return {"op": "count_filtered", "form": form3(), "reads": self.reads()}
        if kind == "upload":                                 # pinned: the copy is asynchronous, ordered by the slot's events alone
            return {"op": "upload", "slot": int(rng.integers(0, 2)), "reads": self.reads(rng.choice(["few", "some"])),
                    "pinned": arg == "pinned" or bool(rng.random() < 0.6)}
        if kind == "count_uploaded":
            full = [s for s in (0, 1) if m.slots[s] is not None]
            if not full:
                return None
            if arg == "wrong":                               # refused for the engine's state: the slot keeps its batch
                wrong = not m.filter_mode
                if not wrong and m.force_path == 4 and not m.sieve:
                    wrong = True                             # (filter mode, path 4, no sieve: the right mode is refused too)
                return {"op": "count_uploaded", "slot": full[0], "filtered": wrong}
            if m.pf_state == EM.PF_TALLYING and not m.filter_mode:
                if arg == "tallying":                        # an insert-mode count while tallying: refused, the batch stays
                    return {"op": "count_uploaded", "slot": full[0], "filtered": False}
                return {"op": "pf_add_uploaded", "slot": full[0]}
            if m.filter_mode and m.force_path == 4 and not m.sieve and arg != "refused":
                return None
            return {"op": "count_uploaded", "slot": full[0], "filtered": m.filter_mode}
        if kind in ("add_pairs", "merge_sorted", "merge_shuffled"):
            n = int(rng.choice([1, 5, 40, 400, 3000]))
            form = {"add_pairs": str(rng.choice(["host", "dev"] if self.long else ["host", "dev", "multi"])),
                    "merge_sorted": "multi", "merge_shuffled": "multi"}[kind]
            if form == "multi" and self.long:
                return None
            if form != "multi":
                keys = self.pairs_keys(n)
                return {"op": "add_pairs", "form": form, "segs": [(keys, None if rng.random() < 0.25 else self.pair_counts(len(keys)))]}
            ordered = kind == "merge_sorted" or (kind == "add_pairs" and rng.random() < 0.5)
            segs = []
            for _ in range(int(rng.integers(1, 5))):
                keys = self.pairs_keys(max(n, 40) if kind != "add_pairs" else n)
                counts = self.pair_counts(len(keys))
                segs.append(self.hash_order(keys, counts) if ordered else (keys, counts))
            return {"op": "add_pairs", "form": "multi", "ordered": ordered, "segs": segs}
        if kind == "set_counts":
            keys = self.stored(int(rng.integers(1, 200)))
            if not keys or self.long:
                return None
            return {"op": "set_counts", "keys": keys, "counts": self.pair_counts(len(keys))}
        if kind in ("load_filter", "load_filter_some", "load_filter_empty"):
            keys = []
            if kind == "load_filter_some" or (kind == "load_filter" and rng.random() > 0.1):
                keys = self.stored(int(rng.choice([3, 50, 800, 6000]))) + self.new_keys(int(rng.integers(kind == "load_filter_some", 30)))
            return {"op": "load_filter", "form": form3(), "keys": keys}
        if kind in ("reset_counts", "clear", "flush"):
            return {"op": kind}
        if kind in ("reserve", "reserve_big", "reserve_huge"):
            big = {"reserve_big": 1 << 15, "reserve_huge": (1 << 16) << (1 + 2 * min(self.huge, 2))}
            self.huge += kind == "reserve_huge"            # (each one larger than the last: a live table grows)
            return {"op": "reserve", "n": big[kind] if kind in big else int(rng.choice([1, 1000, 20000, 100000]))}
        if kind == "set_stream":
            self.own_stream = not self.own_stream
            return {"op": "set_stream", "own": self.own_stream}
        if kind == "opt":
            return self.option(arg)
        if kind == "pf_begin":
            if m.filter_mode or m.pf_state != EM.PF_OFF or m.key_parts > 1 or m.hash_shift:
                return None
            return {"op": "pf_begin", "L": int(rng.choice([2, 3])), "s": int(rng.choice([16, 17, 18]))}
        if kind == "pf_add":
            if m.pf_state != EM.PF_TALLYING:
                return None
            return {"op": "pf_add", "form": form3(), "reads": self.reads()}
        if kind in ("pf_arm", "pf_drop"):
            if (kind == "pf_arm" and m.pf_state != EM.PF_TALLYING) or (kind == "pf_drop" and m.pf_state == EM.PF_OFF):
                return None
            return {"op": kind}
        if kind == "refuse":
            return self.refusal()
        assert kind == "obs", kind
        return self.observer(arg)

    def option(self, arg):
        rng, m = self.rng, self.m
        if arg is None:
            names = ["force_path", "defer", "l1_positions", "l1_direct_positions", "binned_min_positions", "binned_max_positions",
                     "binned_bytes_per_position", "sieve_bits", "merge_min_pairs", "debug_flags", "big_bucket_log2cap", "fused_dump"]
            arg = str(rng.choice(names[:6] + ["debug_flags"] if self.long else names))     # (plain setters a long engine takes too)
        name, _, val = arg.partition("=")
        if val != "":
            value = int(val)
        elif name == "force_path":
            value = int(rng.choice([0, 1] if self.long else [0, 1, 2, 4] if m.filter_mode and m.sieve else [0, 1, 2]))
        elif name == "hash_shift":
            value = int(rng.integers(1, 4))
        else:
            value = int(rng.choice({"defer": [0, 1], "l1_positions": [1 << 12, 1 << 16, 1 << 30], "l1_direct_positions": [1 << 14, 1 << 18, 1 << 28],
                                    "binned_min_positions": [1 << 10, 1 << 22], "binned_max_positions": [4096, 65536, 1 << 31],
                                    "binned_bytes_per_position": [1, 70], "sieve_bits": [0, 8, 16, 32], "merge_min_pairs": [1, 1 << 16],
                                    "debug_flags": [0, 4096], "big_bucket_log2cap": [10, 14, 31], "fused_dump": [0, 1]}[name]))
        if self.long and name in ("hash_shift", "fused_dump", "big_bucket_log2cap", "merge_min_pairs", "sieve_bits") and value:
            return None
        if self.long and name == "force_path" and value in (2, 4):
            return None
        if name == "hash_shift" and value and m.pf_state != EM.PF_OFF:
            return None
        if name == "key_parts" and value > 1 and (m.pf_state != EM.PF_OFF):
            return None
        if name == "key_part" and value >= max(m.key_parts, 1):
            return None
        if name == "force_path" and value == 4 and not (m.filter_mode and m.sieve):
            return None
        return {"op": "option", "name": name, "value": value}

    def refusal(self):
        """an API refusal that returns before any device work, chosen among those the current state offers"""
        m, rng = self.m, self.rng
        can = ["option:force_path=3"]
        if m.filter_mode:
            can.append("count")
        else:
            can.append("count_filtered")
            if m.pf_state == EM.PF_TALLYING:
                can.append("count")
            if m.key_parts > 1 and m.pf_state == EM.PF_OFF:
                can.append("pf_begin")
        if m.pf_state == EM.PF_OFF:
            can.append("pf_arm")
        if m.table and not self.long and m.pf_state == EM.PF_OFF:
            can.append("option:hash_shift")
        empty = [s for s in (0, 1) if m.slots[s] is None]
        if empty:
            can.append("count_uploaded")
        full = [s for s in (0, 1) if m.slots[s] is not None]
        if full:
            can.append("count_uploaded:wrong")
        c = str(rng.choice(can))
        if c == "count":
            return {"op": "count", "form": str(rng.choice(["host", "dev"])), "reads": self.reads("few") + ["ACGT" * 60]}
        if c == "count_filtered":
            return {"op": "count_filtered", "form": str(rng.choice(["host", "dev"])), "reads": self.reads("few") + ["ACGT" * 60]}
        if c == "pf_begin":
            return {"op": "pf_begin", "L": 2, "s": 16}
        if c == "pf_arm":
            return {"op": "pf_arm"}
        if c == "count_uploaded":
            return {"op": "count_uploaded", "slot": empty[0], "filtered": m.filter_mode}
        if c == "count_uploaded:wrong":
            return self.make(c)
        if c == "option:hash_shift":
            return {"op": "option", "name": "hash_shift", "value": m.hash_shift + 1 if m.hash_shift < 3 else 0}
        return {"op": "option", "name": "force_path", "value": 3}

    def observer(self, kind=None):
        rng, m = self.rng, self.m
        if kind is None:
            kind = str(rng.choice(OBSERVERS))
            if m.pf_state != EM.PF_OFF and rng.random() < 0.15:
                kind = "pf_fill"
        op = {"op": "obs", "kind": kind}
        if kind == "count_ge":
            op["m"] = int(rng.choice([0, 1, 2, 3, 5, SAT]))
        elif kind == "export_ge":
            op["m"] = int(rng.choice([0, 0, 1, 2, 3]))
        elif kind == "export_ge_dev":
            op["m"] = int(rng.choice([0, 1, 1, 2, 3]))
            op["sorted"] = bool(rng.random() < 0.5)
        elif kind in ("histogram", "histogram_dev"):
            op["high"] = int(rng.choice([0, 1, 5, 100, 10000]))
        elif kind == "query":
            st = self.stored(int(rng.integers(0, 200)))
            bits = 2 * self.k
            near = [key ^ (1 << int(rng.integers(0, bits))) for key in st[:60]]
            keys = st + near + self.new_keys(int(rng.integers(1, 40)))
            op["keys"] = [keys[i] for i in rng.permutation(len(keys)).tolist()]
        elif kind in ("scan", "window_counts", "read_depth"):
            op["reads"] = self.probe_reads()
            if kind == "read_depth":
                op["low_max"] = int(rng.choice([0, 1, 3, SAT]))
        return op

    # ---- bookkeeping -----------------------------------------------------------------------------------------------------
    def emit(self, op):
        m = self.m
        cls = op_class(op)
        was_filter, was_nonempty, prev = m.filter_mode, bool(m.table), self.prev_class
        had_filter_life = m.had_filter_life
        res = apply(m, op)
        op["refused"] = res[0] == "err"
        self.ops.append(op)
        if op["refused"]:
            self.pairs.add((self.last_mut, "refused"))
            self.prev_class = "refused"
            return
        self.pairs.add((self.last_mut, cls))
        P = self.pre.add
        if cls in ("clear", "load_filter", "reset_counts") and self.counts_since_reader:
            P(f"{cls} with a count since the last reader")
        if cls == "count":
            if prev == "clear":
                P("count right after clear")
            now = (m.key_parts, m.key_part)
            if self.last_count_slice is not None and now != self.last_count_slice and now[0] > 1 and self.last_count_slice[0] == now[0]:
                P("key_part changed between count calls without a clear")
            self.last_count_slice = now
        if cls == "add_pairs" and op["form"] == "multi" and prev == "clear":
            P("merge right after clear")
        if cls == "reserve" and prev == "clear":
            P("reserve right after clear")
        if cls == "observe" and op["kind"] == "scan":
            if self.last_mut == "count":
                P("scan after count")
            if self.pairs_in_filter:
                P("scan after add_pairs into a filter table")
        if cls == "count_filtered" and self.pairs_in_filter:
            P("count_filtered after add_pairs into a filter table")
        if cls == "add_pairs" and m.filter_mode:
            self.pairs_in_filter = True                    # keys the loaded filter's sieve has not seen
        if cls in ("clear", "load_filter"):
            self.pairs_in_filter = False
        if op["op"] == "pf_begin" and had_filter_life:
            P("prefilter begun on an engine that has had a filter life")
        if op["op"] == "option" and op["name"] == "big_bucket_log2cap" and was_nonempty:
            P("big_bucket_log2cap changed with a non-empty model")
        if cls in ("count", "count_filtered"):
            self.counts_since_reader += 1
        elif cls not in ("upload",) and not (cls == "option" and op["name"] in ("debug_flags", "defer_max_bytes")):
            self.counts_since_reader = 0           # everything else reads, flushes or drops what is pending
        if cls in ("clear", "load_filter"):
            self.last_count_slice = None
        if cls != "observe":
            self.last_mut = cls
        self.prev_class = cls

    def step(self):
        rng, m = self.rng, self.m
        if not self.queue and rng.random() < 0.3:
            if not self.todo:                                 # every motif once, in a drawn order, before any comes again
                pool = MOTIFS["all"] + ([] if self.long else MOTIFS["short"])
                self.todo = [pool[i] for i in rng.permutation(len(pool)).tolist()]
                self.rounds += 1
            self.queue = list(self.todo.pop())
            if m.pf_state != EM.PF_OFF and not self.queue[0].startswith("pf_") and (m.pf_state == EM.PF_TALLYING or rng.random() < 0.7):
                self.queue.insert(0, "pf_drop")               # (most motifs count: a tallying prefilter would refuse them)
            if "pf_begin" in self.queue and m.pf_state == EM.PF_OFF:
                if m.hash_shift:
                    self.queue[:0] = ["clear", "opt:hash_shift=0"]
                if m.key_parts > 1:
                    self.queue.insert(0, "opt:key_parts=0")
            if m.filter_mode and self.queue[0] not in ("load_filter", "clear", "refuse"):
                self.queue.insert(0, "clear")                 # (... and so would a loaded filter)
        if self.queue:
            op = self.make(self.queue.pop(0))     # (opt:hash_shift: an empty model takes it, any other refuses it)
            if op is not None:
                self.emit(op)
                if op["refused"]:
                    self.emit(self.observer())                # every refusal is followed by an observer: nothing moved
            return
        if m.pf_state == EM.PF_TALLYING:
            kinds, w = ["pf_add", "upload", "count_uploaded", "pf_arm", "obs", "clear", "refuse", "set_stream", "pf_drop"], [5, 2, 2, 3, 2, 0.5, 1, 0.5, 0.5]
        elif m.filter_mode:
            kinds = ["count_filtered", "upload", "count_uploaded", "add_pairs", "set_counts", "load_filter", "reset_counts", "clear", "reserve",
                     "flush", "opt", "set_stream", "refuse", "obs"]
            w = [8, 2, 2, 3, 1.5, 2, 2, 2, 1, 1, 4, 1, 1.5, 3]
        else:
            kinds = ["count", "upload", "count_uploaded", "add_pairs", "set_counts", "load_filter", "reset_counts", "clear", "reserve", "flush",
                     "opt", "set_stream", "refuse", "obs", "pf_begin", "pf_drop", "opt:key_parts=3", "opt:key_parts=0", "opt:key_part=1"]
            w = [9, 2, 2, 3, 1, 1.5, 1.5, 2, 1.5, 1, 5, 1, 1.5, 3, 0.7, 1.5 if m.pf_state else 0, 0.3, 0.6 if m.key_parts else 0, 0.5 if m.key_parts else 0]
        w = np.array(w, float)
        op = self.make(str(rng.choice(kinds, p=w / w.sum())))
        if op is None:
            return
        self.emit(op)
        if op["refused"] or (op_class(op) != "observe" and rng.random() < 0.3):
            self.emit(self.observer())

    def finish(self):
        """every observer at the end of the life (the prefilter's too, when one is there)"""
        for kind in OBSERVERS + (("pf_fill",) if self.m.pf_state != EM.PF_OFF else ()):
            self.emit(self.observer(kind))


def generate(seed, family, n_ops):
    """-> (ops, coverage): ``n_ops`` calls and then every observer; the first op record holds k and the capacity hint"""
    g = _Gen(seed, family)
    while len(g.ops) < n_ops or g.rounds < 1 or (g.rounds == 1 and (g.todo or g.queue)):
        g.step()                                              # (at least n_ops calls, and every motif at least once)
    g.finish()
    head = {"k": g.k, "capacity_hint": g.capacity_hint, "seed": seed, "family": family}
    return [head] + g.ops, {"pairs": g.pairs, "preconditions": g.pre}


def digest(ops):
    """a short fingerprint of a sequence (names, sizes, option values and a hash of every argument)"""
    import hashlib
    h = hashlib.sha256()
    for op in ops:
        h.update(repr(sorted(op.items(), key=lambda kv: kv[0])).encode())
    return h.hexdigest()
