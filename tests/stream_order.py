"""The stream-order contract of the device entry points, made observable (a helper, not a conftest).

Every ``_dev`` entry point of ``include/kdf.h`` promises an order: its reads of the caller's buffers and its writes to them
happen in the order of the engine's stream, whether or not the call itself waits for the device.  With an idle stream that
promise cannot be seen to break -- a kernel queued on the wrong stream, a missing event wait or a pointer kept past the
call still finds the right bytes.  ``StreamOrder`` runs one call under the conditions the promise is made for:

1. every input buffer holds a DECOY (a well-formed other input of the same shape and dtype), every output a sentinel;
2. on the caller's stream ``S`` (a ``torch.cuda.Stream`` the engine was given with ``set_stream``, never the default
   stream: handle 0 means "the engine's own stream") a bounded delay of plain matmul launches is queued, behind it the
   copies that overwrite the decoys with the true inputs, behind those the event ``produced``;
3. the call is made with no host synchronisation in front of it;
4. as soon as it returns ``early = not produced.query()`` is noted and copies that put the decoys BACK are queued on ``S``:
   from then on the caller's buffers are dead, whatever the engine deferred must not read them again;
5. outputs are read on ``S``.

A call that read a buffer out of order saw a decoy and computes the answer for the decoy -- a wrong answer, never a wild
access: decoys are built by the functions below from in-range values only (reads, offsets that do not decrease and end
where the true ones end, positions and indices below their bounds, canonical keys), and those builders are unit-tested on
the CPU by ``tests/test_stream_order_table.py``.  Nothing here uses random bits for a value a kernel indexes with.

The delay is sized from measurements only: ``Delay`` times one unit with HIP events; a case's control run (the same call
on the same engine state between host synchronisations, true inputs, no delay) gives ``t_call`` and warms the call up;
the contract run queues ``max(20 ms, 4 x t_call)`` of delay.  Whether the window was real is asserted, not assumed: a call
of class ``no_sync`` must come back with ``early`` true (it returned while the producer had not run), one of class
``syncs`` with ``early`` false.  The window also has to be a window for work on OTHER streams: see ``CallerStreams``."""
import math
import time

import numpy as np

import spool_model as SM

NO_SYNC, SYNCS = "no_sync", "syncs"

FLOOR_MS = 20.0          # covers timer noise
MARGIN = 4.0             # over the only thing the window must outlast: the call's own host time
MAX_DELAY_MS = 1500.0    # bounded, whatever a control run measured
SENTINEL = 0x5A5A5A5A5A5A5A5A

_ACGT = np.frombuffer(b"ACGT", np.uint8)


# ------------------------------------------------------------------------------------------------ inputs and decoys (CPU)

def random_reads(rng, lengths, genome_len=6000, sub=0.003, n_rate=0.05):
    """Ragged reads over a small random genome: 0.3 % substitutions, one N in 5 % of the reads."""
    genome = rng.integers(0, 4, genome_len)
    reads = []
    for L in lengths:
        L = int(L)
        a = int(rng.integers(0, genome_len - L))
        g = genome[a:a + L].copy()
        err = rng.random(L) < sub
        g[err] = (g[err] + 1) % 4
        r = _ACGT[g].copy()
        if L and rng.random() < n_rate:
            r[int(rng.integers(0, L))] = ord("N")
        reads.append(r.tobytes().decode())
    return reads


def pack_reads(reads):
    """(packed, invalid, n_bases, offsets) of reads laid out as ``include/kdf.h`` "Read streams" has them: one invalid
    separator position behind every read, arrays of exactly the stream_words(n_bases) sizes (``spool_model.pack``)."""
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) + 1 for r in reads])
    n = int(offs[-1])
    codes = np.zeros(n, np.uint8)
    inv = np.ones(n, bool)
    lut = np.full(256, 255, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
        lut[ord(chr(c).lower())] = i
    for r, a in zip(reads, offs[:-1].tolist()):
        c = lut[np.frombuffer(r.encode(), np.uint8)]
        codes[a:a + len(r)] = np.where(c == 255, 0, c)
        inv[a:a + len(r)] = c == 255
    packed, invalid = SM.pack(codes, inv)
    return packed, invalid, n, offs


class World:
    """True reads and decoy reads: as many reads, the same total length (so the same n_bases and the same stream_words),
    another genome and the lengths in reverse order (so other offsets and, for k >= 31, no k-mer in common)."""

    def __init__(self, seed, n_reads=1800, min_len=40, max_len=221):
        rng = np.random.default_rng(seed)
        lengths = rng.integers(min_len, max_len, n_reads)
        self.reads = random_reads(rng, lengths)
        self.decoy_reads = random_reads(rng, lengths[::-1])
        self.packed, self.invalid, self.n_bases, self.offsets = pack_reads(self.reads)
        self.d_packed, self.d_invalid, dn, self.d_offsets = pack_reads(self.decoy_reads)
        assert dn == self.n_bases and not np.array_equal(self.offsets, self.d_offsets)

    def stream_inputs(self):
        return {"packed": (self.packed, self.d_packed), "invalid": (self.invalid, self.d_invalid)}

    def offsets_input(self):
        return {"offsets": (self.offsets, self.d_offsets)}


def decoy_offsets(offsets, rng):
    """Another offsets array of the same length: starts where the true one starts, does not decrease, ends at the same
    total -- and differs from it whenever there is room to."""
    o = np.asarray(offsets, np.int64)
    if len(o) <= 2:
        return o.copy()
    inner = np.sort(rng.integers(int(o[0]), int(o[-1]) + 1, len(o) - 2)).astype(np.int64)
    return np.concatenate([o[:1], inner, o[-1:]])


def decoy_indices(n, bound, rng, dtype=np.uint64):
    """n values in [0, bound): positions, group ids, pair indices."""
    return rng.integers(0, max(int(bound), 1), int(n)).astype(dtype)


def decoy_like(true, pool, rng):
    """len(true) rows drawn (with repetition when the pool is short) from ``pool``, an array of well-formed alternative
    values of the same dtype and row shape: keys out of another truth, counts, CIGAR words."""
    true, pool = np.asarray(true), np.asarray(pool)
    assert pool.dtype == true.dtype and pool.shape[1:] == true.shape[1:] and len(pool) > 0
    return pool[rng.integers(0, len(pool), len(true))].copy()


# ------------------------------------------------------------------------------------------------ the delay and the harness (GPU)

class Delay:
    """A bounded delay made of ordinary torch work: a chain of fp32 matmul launches on a scratch tensor."""

    N = 2048

    def __init__(self, device=0):
        import torch
        self.torch = torch
        dev = torch.device("cuda", device)
        self.a = torch.randn(self.N, self.N, device=dev) / math.sqrt(self.N)
        self.b = torch.empty_like(self.a)
        for _ in range(300):                         # (clocks up before the unit is timed: a cold unit is a long one)
            self._unit()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 100
        e0.record()
        for _ in range(reps):
            self._unit()
        e1.record()
        torch.cuda.synchronize(dev)
        self.unit_ms = e0.elapsed_time(e1) / reps
        assert self.unit_ms > 0

    def _unit(self):
        self.torch.mm(self.a, self.a, out=self.b)

    def enqueue(self, ms):
        """Queue at least ``ms`` milliseconds of work on the current stream -> the units queued."""
        n = int(math.ceil(min(ms, MAX_DELAY_MS) / self.unit_ms))
        for _ in range(n):
            self._unit()
        return n


class CallerStreams:
    """Caller streams that were MEASURED to run independently of one another.  A device multiplexes its streams onto a
    few hardware queues, and two streams that share a queue run in order whatever the program says: an engine that
    launched on a stream of its own would then be ordered behind the caller's delay by accident, and a missing wait could
    not show.  Which queue an engine's internal streams land on is not the harness's to choose, so every contract run is
    made on TWO caller streams that do not share a queue (``pair``): a stream of the engine's can share one with at most
    one of them.  Independence is a measurement: with a delay queued on ``a``, a small piece of work on ``b`` completes
    while the delay's event is still pending."""

    def __init__(self, delay, device=0, want=4, candidates=16):
        import torch
        self.torch, self.delay = torch, delay
        self.dev = torch.device("cuda", device)
        self._probe = torch.zeros(64, device=self.dev)
        self.streams = []
        for _ in range(candidates):
            s = torch.cuda.Stream(self.dev)
            if s.cuda_stream == 0 or any(s.cuda_stream == t.cuda_stream for t in self.streams):
                continue
            if all(self.independent(t, s) and self.independent(s, t) for t in self.streams):
                self.streams.append(s)
            if len(self.streams) == want:
                break
        assert len(self.streams) >= 2, "no two caller streams that run independently: the contract window cannot be made"

    def independent(self, a, b):
        torch = self.torch
        torch.cuda.synchronize(self.dev)
        with torch.cuda.stream(a):
            self.delay.enqueue(FLOOR_MS)
            ea = torch.cuda.Event()
            ea.record(a)
        with torch.cuda.stream(b):
            self._probe.add_(1.0)
            eb = torch.cuda.Event()
            eb.record(b)
        eb.synchronize()
        ok = not ea.query()
        torch.cuda.synchronize(self.dev)
        return ok

    @property
    def pair(self):
        return self.streams[:2]

    def other(self, i):
        """the i-th further stream measured independent of the pair and of the others, or None where the device gave fewer"""
        return self.streams[2 + i] if 2 + i < len(self.streams) else None


class Run:
    def __init__(self, harness, ret, early, host_s, delay_ms, outs, keep, produced=()):
        self.h, self.ret, self.early, self.host_s, self.delay_ms, self.outs, self._keep = harness, ret, early, host_s, delay_ms, outs, keep
        self.produced = list(produced)

    def read(self, name, dtype, count=None):
        """An output buffer as a host array, read on the caller's stream."""
        torch = self.h.torch
        with torch.cuda.stream(self.h.S):
            host = self.outs[name].cpu().numpy()
        a = host.view(np.uint8).view(dtype)
        return a.copy() if count is None else a[:int(count)].copy()


class StreamOrder:
    """One caller stream ``S`` and the two kinds of run on it.  ``inputs``: {name: (true, decoy)} host arrays of one shape
    and dtype; ``outputs``: {name: bytes} or {name: (bytes, fill word)}; ``call(ptr)``: the entry point, ``ptr[name]`` the
    raw device pointer of a buffer, its return value is kept in ``Run.ret``."""

    def __init__(self, delay, streams, device=0):
        import torch
        self.torch, self.delay, self.streams = torch, delay, streams
        self.dev = torch.device("cuda", device)
        self.S = streams.pair[0]
        assert all(s.cuda_stream != 0 for s in streams.streams), "a caller stream must not be the default stream"
        self.records = []
        self._others = 0
        self.expected, self.class_checked = None, True           # the class the table lists for the running case

    @property
    def handle(self):
        return self.S.cuda_stream

    def use(self, stream, engines=()):
        """make ``stream`` the caller stream and hand it to the engines"""
        self.S = stream
        for e in engines:
            e.set_stream(stream.cuda_stream)

    def independent_stream(self):
        """A further caller stream (a second engine's, the producers of a spool's appends), measured to run independently
        of the pair and of the ones handed out before.  A wait across two streams that share a hardware queue cannot be
        seen to be missing, so a device that has no such stream left is never passed over in silence: the case goes on
        with an unmeasured stream, and says so in a warning and in the records."""
        s = self.streams.other(self._others)
        self._others += 1
        if s is None:
            import warnings
            s = self.torch.cuda.Stream(self.dev)
            msg = (f"only {len(self.streams.streams)} independent caller streams on this device: stream {self._others + 2} of this case is "
                   f"unmeasured, the waits across it may be untested")
            warnings.warn(msg)
            self.records.append((msg, "-", 0.0, 0.0, 0.0, None))
        assert s.cuda_stream != 0
        return s

    def to_dev(self, a):
        """host array -> int64 device tensor that holds its bytes (padded to whole words; never empty)"""
        b = np.ascontiguousarray(a).view(np.uint8).ravel()
        words = max((len(b) + 7) // 8, 1)
        buf = np.zeros(words * 8, np.uint8)
        buf[:len(b)] = b
        return self.torch.from_numpy(buf.view(np.int64)).to(self.dev)

    def _outs(self, outputs):
        outs = {}
        for name, spec in outputs.items():
            nbytes, fill = spec if isinstance(spec, tuple) else (spec, SENTINEL)
            fill = fill - (1 << 64) if fill >= (1 << 63) else fill
            outs[name] = self.torch.full((max((int(nbytes) + 7) // 8, 1),), fill, dtype=self.torch.int64, device=self.dev)
        return outs

    @staticmethod
    def _check_pairs(inputs):
        for name, (t, d) in inputs.items():
            t, d = np.asarray(t), np.asarray(d)
            assert t.shape == d.shape and t.dtype == d.dtype, f"decoy of {name}: {d.dtype}{d.shape} for {t.dtype}{t.shape}"

    def control(self, inputs, outputs, call):
        """The call between host synchronisations, true inputs, nothing in flight: the reference behaviour, the warm-up
        and ``t_call`` (call and the synchronisation behind it: an upper bound of the call's host time)."""
        torch = self.torch
        self._check_pairs(inputs)
        live = {n: self.to_dev(t) for n, (t, _) in inputs.items()}
        outs = self._outs(outputs)
        ptr = {n: t.data_ptr() for n, t in {**live, **outs}.items()}
        torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        ret = call(ptr)
        torch.cuda.synchronize(self.dev)
        t1 = time.perf_counter()
        return Run(self, ret, None, t1 - t0, 0.0, outs, live)

    def contract(self, inputs, outputs, call, t_call, producers=None):
        """The call under contract conditions (module docstring).  ``producers``: {name: stream} for inputs that another
        caller stream than ``S`` produces (each gets its own delay)."""
        torch = self.torch
        self._check_pairs(inputs)
        true = {n: self.to_dev(t) for n, (t, _) in inputs.items()}
        decoy = {n: self.to_dev(d) for n, (_, d) in inputs.items()}
        live = {n: d.clone() for n, d in decoy.items()}
        outs = self._outs(outputs)
        ptr = {n: t.data_ptr() for n, t in {**live, **outs}.items()}
        delay_ms = min(max(FLOOR_MS, MARGIN * 1e3 * t_call), MAX_DELAY_MS)
        streams = {}
        for n in live:
            streams.setdefault((producers or {}).get(n, self.S), []).append(n)
        torch.cuda.synchronize(self.dev)
        produced = []
        for s, names in streams.items():
            with torch.cuda.stream(s):
                self.delay.enqueue(delay_ms)
                for n in names:
                    live[n].copy_(true[n], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(s)
                produced.append(ev)
        t0 = time.perf_counter()
        ret = call(ptr)
        t1 = time.perf_counter()
        early = not any(ev.query() for ev in produced) if produced else None
        for s, names in streams.items():
            with torch.cuda.stream(s):
                for n in names:
                    live[n].copy_(decoy[n], non_blocking=True)
        return Run(self, ret, early, t1 - t0, delay_ms, outs, (true, decoy, live), produced)

    def note(self, label, cls, ctl, run):
        self.records.append((label, cls, ctl.host_s, run.host_s, run.delay_ms, run.early))

    def check_class(self, label, cls, run):
        if cls == NO_SYNC:
            assert run.early is True, (
                f"{label}: documented as not synchronising, but the call returned after the producer had run "
                f"(host {run.host_s * 1e3:.2f} ms inside a delay of {run.delay_ms:.1f} ms): either the call synchronises "
                f"against its documentation or the window was not real")
        else:
            assert cls == SYNCS
            assert run.early is False, f"{label}: documented as synchronising, but it returned before the producer had run"


def same(got, want, what=""):
    """Deep equality of nested tuples / lists / dicts of numpy arrays and scalars, with a readable failure."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and got.keys() == want.keys(), f"{what}: keys differ ({len(got)} vs {len(want)})"
        bad = [k for k in want if not _eq(got[k], want[k])]
        assert not bad, f"{what}: {len(bad)} of {len(want)} entries differ, first {bad[0]!r}: {got[bad[0]]!r} != {want[bad[0]]!r}"
    elif isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), f"{what}: {len(got)} parts for {len(want)}"
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, f"{what}[{i}]")
    elif isinstance(want, np.ndarray):
        g = np.asarray(got)
        assert g.shape == want.shape, f"{what}: shape {g.shape} for {want.shape}"
        if not np.array_equal(g, want):
            at = np.flatnonzero(g.ravel() != want.ravel())
            raise AssertionError(f"{what}: {len(at)} of {want.size} values differ, first at {at[0]}: {g.ravel()[at[0]]} != {want.ravel()[at[0]]}")
    else:
        assert got == want, f"{what}: {got!r} != {want!r}"


def _eq(a, b):
    if isinstance(b, np.ndarray) or isinstance(a, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b
