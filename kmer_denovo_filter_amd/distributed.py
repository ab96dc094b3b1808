"""Multi-GPU layer: one process per GPU, ``torch.distributed`` (backend "nccl" ==
RCCL over xGMI on ROCm; "gloo" in the CPU tests).  The reference has no
distributed path at all (no NCCL/MPI call site; its only
parallelism is ``jellyfish -t`` and a per-contig process pool), so this follows
SURVEY.md section 8e rather than a reference file:

* ``ShardedFilterCount`` -- the ``count --if`` stages (parent filter
  discovery/pipeline.py:462-612, VCF Step 3 vcf/pipeline.py:1587-1609).  Reads
  are independent units: every rank holds the same filter table, counts its own
  shard of the read stream, and the per-key counts (queried in the SAME key
  order on every rank, so slot layouts need not agree) are merged with ONE
  all-reduce(sum).  No other collective touches the data path.

* ``OwnerPartitionedCount`` -- the full count stage (child counting,
  discovery/pipeline.py:69-268).  Every rank counts its read shard into a local
  table, dumps (key, count) pairs on the device, sends each pair to the rank
  that owns its key (one all-to-all; pre-aggregation bounds the traffic by the
  distinct k-mers per GPU, not by the windows) and the owner sums them.  After
  the exchange rank r holds the exact global count of every key it owns; the
  ``dump -L`` threshold is then rank-local and a scalar all-reduce gives the
  global number of survivors.  This is Jellyfish's ``merge`` (jellyfish_wrappers.py:335-366)
  done over xGMI.

  With the two-pass count (``prefilter_begin`` / ``tally_local`` / ``prefilter_merge``, kdf.h "two-pass counting")
  every rank first tallies its shard into a counting sieve; the sieves are merged with a saturating sum (a
  hand-made reduce-scatter + all-gather, the sum runs in ``kdf_pf_merge_kernel``) so that every rank holds the
  sieve of the WHOLE sample, and the local counts that follow store only the keys that sieve admits: smaller local
  tables and a smaller all-to-all, the same ``dump -L``.

Long k-mers (odd k from 65 to 201, keys as (n, W) rows with ``hi`` None) go through both classes too: owners come
from ``owner_of_w``, an entry on the wire is 8 W + 4 bytes, the engine dumps by owner at any table size
(``kdf_export_parts_w_packed_dev``) and the owner adds each received segment with one ``kdf_add_pairs_w_dev``.  The
mirrors take this only under ``KDF_LONG_RANKS=1``; it has run as several ranks on one GPU over gloo, never over RCCL.

Both classes are written against a tiny adapter (``TableOps``) so that the
sharding / exchange logic runs under gloo on CPU tensors in the tests, with the
oracle standing in for the table; on a GPU the adapter is ``EngineOps`` (the HIP
engine through raw device pointers).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

_U32_MAX = 0xFFFFFFFF


def _lsr(x: torch.Tensor, n: int) -> torch.Tensor:
    """Logical right shift of int64 bit patterns."""
    return (x >> n) & ((1 << (64 - n)) - 1)


def owner_of(lo: torch.Tensor, hi: Optional[torch.Tensor], world: int) -> torch.Tensor:
    """Owner rank of each key: ``((hash >> 48) * world) >> 16`` with the TABLE's hash
    (csrc/kdf_device.h ``kdf_hash``; int64 arithmetic wraps like uint64).  The top
    hash bits are the top bits of a key's home slot, so on every rank the keys of
    one owner sit in one contiguous slot range and the engine can dump them grouped
    by owner without a sort (``kdf_export_parts_dev``).  It depends on the key only
    -- not on any table's size."""
    x = lo
    if hi is not None:
        x = lo ^ ((hi << 37) | _lsr(hi, 27))
    h = (x ^ _lsr(x, 32)) * -0x604DE39AE16720DB           # KDF_MIX_MUL = 0x9FB21C651E98DF25 as int64
    return (_lsr(h, 48) * world) >> 16


_MIX_MUL = -0x604DE39AE16720DB                            # KDF_MIX_MUL = 0x9FB21C651E98DF25 as int64
_FOLD_ADD = 0x632BE59BD9B4E019                            # kdf_long_fold_step's constant


def _mix64(x: torch.Tensor) -> torch.Tensor:
    """csrc/kdf_device.h ``kdf_mix64`` on int64 bit patterns (int64 arithmetic wraps like uint64)."""
    return (x ^ _lsr(x, 32)) * _MIX_MUL


def long_hash(keys: torch.Tensor) -> torch.Tensor:
    """The stored form of long key rows, csrc/kdf_long.h ``kdf_long_hash``: ``keys`` is an (n, W) int64 tensor of key
    words (bit patterns), word 0 the least significant, W = 3..7."""
    f = torch.zeros(keys.shape[0], dtype=torch.int64, device=keys.device)
    for j in range(keys.shape[1] - 1, 0, -1):             # the fold runs from the top word down
        f = _mix64(f ^ keys[:, j]) + _FOLD_ADD
    return _mix64(keys[:, 0] ^ f)


def owner_of_w(keys: torch.Tensor, world: int) -> torch.Tensor:
    """Owner rank of each long key row: ``(((h >> 16) & 0xFFFF) * world) >> 16`` with h = ``long_hash(keys)``, world
    1..64 -- bits 16..31 of the table's hash, where ``owner_of`` takes the top 16.  The home slot is the TOP log2cap
    bits of h and the ``key_parts`` slice its LOW 16, so an owner's keys spread over the whole of an ordinary long table
    (no ``hash_shift``), whatever key slice is active; the engine groups its dump by this rule key by key
    (``kdf_export_parts_w_packed_dev``)."""
    if not 1 <= int(world) <= 64:
        raise ValueError(f"owner_of_w: world={world} outside 1..64")
    if keys.dim() != 2 or not 3 <= keys.shape[1] <= 7:
        raise ValueError(f"owner_of_w: keys must be (n, 3..7) rows of key words, got shape {tuple(keys.shape)}")
    return ((_lsr(long_hash(keys), 16) & 0xFFFF) * int(world)) >> 16


def _entry_bytes(wide: bool, key_words: int = 0) -> int:
    """Bytes of one (key, count) entry on the wire: 12 / 20 for (lo) / (lo, hi) keys, 8 W + 4 for rows of W words."""
    return 8 * key_words + 4 if key_words > 2 else (20 if wide else 12)


class TableOps:
    """What the distributed logic needs from a table (see EngineOps).  A table of long keys (``key_words`` = W >= 3)
    takes and returns its keys as (n, W) rows in the ``lo`` position with ``hi`` None."""
    wide: bool
    device: torch.device
    key_words: int = 0                                    # 3..7: long keys; anything else: (lo, hi)

    def clear(self): raise NotImplementedError
    def count_stream(self, packed: torch.Tensor, invalid: torch.Tensor, n_bases: int): raise NotImplementedError
    def count_stream_filtered(self, packed: torch.Tensor, invalid: torch.Tensor, n_bases: int): raise NotImplementedError
    def export_pairs(self, min_count: int) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]: raise NotImplementedError
    def add_pairs(self, lo: torch.Tensor, hi: Optional[torch.Tensor], cnt: torch.Tensor): raise NotImplementedError
    def query(self, lo: torch.Tensor, hi: Optional[torch.Tensor]) -> torch.Tensor: raise NotImplementedError
    def count_ge(self, min_count: int) -> int: raise NotImplementedError
    def stats(self) -> Tuple[int, int, int]: raise NotImplementedError
    def histogram(self, high: int) -> torch.Tensor: raise NotImplementedError   # int64[high + 2] on self.device
    def count_stats(self) -> dict: raise NotImplementedError

    # two-pass counting: the counting sieve of kdf.h.  Words travel as int64 tensors on self.device.
    def prefilter_begin(self, min_count: int, log2_cells: int): raise NotImplementedError
    def prefilter_tally_stream(self, packed: torch.Tensor, invalid: torch.Tensor, n_bases: int): raise NotImplementedError
    def prefilter_words(self) -> int: raise NotImplementedError
    def prefilter_export(self, first: int, n: int) -> torch.Tensor: raise NotImplementedError
    def prefilter_merge(self, first: int, segments: List[torch.Tensor], replace: bool = False): raise NotImplementedError
    def prefilter_arm(self): raise NotImplementedError
    def prefilter_drop(self): raise NotImplementedError
    def prefilter_windows(self) -> int: raise NotImplementedError            # windows THIS table tallied

    # distinct k-mer sketch (kdf.h "distinct k-mer sketch").  Registers travel as uint8 tensors on the CPU: 2^p bytes.
    def sketch_begin(self, log2_registers: int): raise NotImplementedError
    def sketch_add_stream(self, packed: torch.Tensor, invalid: torch.Tensor, n_bases: int): raise NotImplementedError
    def sketch_registers(self) -> torch.Tensor: raise NotImplementedError
    def sketch_merge(self, regs: torch.Tensor): raise NotImplementedError    # reg = max(own, regs)
    def sketch_estimate(self) -> float: raise NotImplementedError
    def sketch_drop(self): raise NotImplementedError

    def add_pairs_segments(self, segments):
        """Sum the segments [(lo, hi, cnt), ...] received from the source ranks (a table that can merge them
        in one pass overrides this)."""
        for lo, hi, cnt in segments:
            self.add_pairs(lo, hi, cnt)

    def prepare_owner(self, world: int):
        """Called once on the table that will hold the keys this rank OWNS out of ``world`` ranks."""


class EngineOps(TableOps):
    """TableOps over a KmerEngine; tensors are int64 / int32 views of the
    engine's uint64 / uint32 arrays in HBM."""

    def __init__(self, engine, device: torch.device):
        self.e = engine
        self.wide = engine.wide
        self.long = bool(getattr(engine, "long", False))
        self.key_words = int(engine.key_words) if self.long else 0
        self.device = device

    def clear(self):
        self.e.clear()

    def _sync(self):
        torch.cuda.current_stream(self.device).synchronize()

    def count_stream(self, packed, invalid, n_bases):
        self._sync()
        self.e.count_dev(packed.data_ptr(), invalid.data_ptr(), n_bases)

    def count_stream_filtered(self, packed, invalid, n_bases):
        self._sync()
        self.e.count_filtered_dev(packed.data_ptr(), invalid.data_ptr(), n_bases)

    def export_pairs(self, min_count):
        n = self.e.count_ge(min_count)
        lo = torch.empty((n, self.key_words) if self.long else n, dtype=torch.int64, device=self.device)
        hi = torch.empty(n, dtype=torch.int64, device=self.device) if self.wide and not self.long else None
        cnt = torch.empty(n, dtype=torch.int32, device=self.device)
        self._sync()
        if n:
            got = self.e.export_ge_dev(min_count, lo.data_ptr(), hi.data_ptr() if hi is not None else None,
                                       cnt.data_ptr(), n)
            assert got == n
        return lo, hi, cnt

    def export_pairs_by_owner(self, world: int):
        """(lo, hi, cnt, per-owner counts) already grouped by owner rank, or None when
        the table is too small for the engine's owner-ordered dump (and for long keys: they travel packed)."""
        if self.long or self.e.get_stat("log2cap") < 28 or world > 64 or self.e.get_stat("hash_shift"):
            return None
        _, distinct, _ = self.e.stats()
        lo = torch.empty(distinct, dtype=torch.int64, device=self.device)
        hi = torch.empty(distinct, dtype=torch.int64, device=self.device) if self.wide else None
        cnt = torch.empty(distinct, dtype=torch.int32, device=self.device)
        self._sync()
        n, counts = self.e.export_parts_dev(0, world, lo.data_ptr(), hi.data_ptr() if hi is not None else None,
                                            cnt.data_ptr(), distinct)
        self.e.synchronize()
        return lo[:n], (hi[:n] if hi is not None else None), cnt[:n], counts

    def export_packed_by_owner(self, world: int):
        """(send buffer uint8, per-owner pair counts, per-owner byte offsets [world + 1]): the owner-ordered dump written
        by the engine straight into the layout `OwnerPartitionedCount.exchange` sends -- no (lo, hi, cnt) temporaries, no
        packing copies.  None when the table cannot be dumped by owner (see export_pairs_by_owner).  A long engine groups
        its dump by `owner_of_w` key by key (``kdf_export_parts_w_packed_dev``), at any table size: never None."""
        if self.long:
            if not 1 <= world <= 64:
                raise ValueError(f"long keys: the owner exchange takes 1..64 ranks, not {world}")
            _, distinct, _ = self.e.stats()
            cap = distinct * _entry_bytes(False, self.key_words) + 8 * world + 8
            buf = torch.empty(cap, dtype=torch.uint8, device=self.device)
            self._sync()
            n, counts, offs = self.e.export_parts_w_packed_dev(0, world, buf.data_ptr(), cap)   # complete on return
            return buf[:offs[world]], counts, offs
        if self.e.get_stat("log2cap") < 28 or world > 64 or self.e.get_stat("hash_shift"):
            return None
        _, distinct, _ = self.e.stats()
        cap = distinct * (20 if self.wide else 12) + 8 * world + 8
        buf = torch.empty(cap, dtype=torch.uint8, device=self.device)
        self._sync()
        n, counts, offs = self.e.export_parts_packed_dev(0, world, buf.data_ptr(), cap)
        self.e.synchronize()
        return buf[:offs[world]], counts, offs

    def add_pairs(self, lo, hi, cnt):
        if lo.shape[0] == 0:
            return
        lo, cnt = lo.contiguous(), cnt.contiguous()
        hi = hi.contiguous() if hi is not None else None
        self._sync()
        self.e.add_pairs_dev(lo.data_ptr(), hi.data_ptr() if hi is not None else None, cnt.data_ptr(), lo.shape[0])
        self.e.synchronize()

    def add_pairs_segments(self, segments):
        """All source ranks' segments in ONE engine call: when they arrive in hash order (the engine's
        owner-ordered dump) every table bucket is merged in LDS and written once (csrc/kdf_merge.h).  Long keys: one
        ``kdf_add_pairs_w_dev`` call per segment."""
        if self.long:
            for lo, hi, cnt in segments:
                self.add_pairs(lo, hi, cnt)
            return
        segs = [(lo.contiguous(), hi.contiguous() if hi is not None else None, cnt.contiguous())
                for lo, hi, cnt in segments if lo.numel()]
        if not segs:
            return
        self._sync()
        self.e.add_pairs_multi_dev([(lo.data_ptr(), hi.data_ptr() if hi is not None else None, cnt.data_ptr(), lo.numel())
                                    for lo, hi, cnt in segs])
        self.e.synchronize()

    def prepare_owner(self, world: int):
        """An owner only ever sees keys whose top hash bits name it: its table drops floor(log2(world)) of them
        from the home slot (engine option ``hash_shift``), so the whole table is used and the senders' hash
        order is the table's bucket order.  (world not a power of two: the owner's keys cover
        2^floor(log2 world) / world of the table; ask for that much more capacity.)  Long keys: nothing to do -- their
        owner bits (`owner_of_w`) are not home-slot bits."""
        if self.long:
            return
        self.e.set_option("hash_shift", max(0, int(world).bit_length() - 1))

    def prefilter_begin(self, min_count, log2_cells):
        self.e.prefilter_begin(min_count, log2_cells)

    def prefilter_tally_stream(self, packed, invalid, n_bases):
        self._sync()
        self.e.prefilter_add_dev(packed.data_ptr(), invalid.data_ptr(), n_bases)

    def prefilter_words(self):
        return self.e.prefilter_words()

    def prefilter_export(self, first, n):
        out = torch.empty(int(n), dtype=torch.int64, device=self.device)
        if n:
            self._sync()
            self.e.prefilter_export_dev(out.data_ptr(), first, n)   # complete on return
        return out

    def prefilter_merge(self, first, segments, replace=False):
        """All segments (int64 tensors of one length in HBM) in ONE kernel launch (``kdf_pf_merge_kernel``)."""
        segs = [s.contiguous() for s in segments]
        if not segs or segs[0].numel() == 0:
            return
        self._sync()
        self.e.prefilter_merge_dev([s.data_ptr() for s in segs], first, segs[0].numel(), replace)
        self.e.synchronize()                                        # (the segments are the caller's again)

    def prefilter_arm(self):
        self.e.prefilter_arm()

    def prefilter_drop(self):
        self.e.prefilter_drop()

    def prefilter_windows(self):
        return self.e.get_stat("prefilter_windows")

    def sketch_begin(self, log2_registers):
        self.e.sketch_begin(log2_registers)

    def sketch_add_stream(self, packed, invalid, n_bases):
        self._sync()
        self.e.sketch_add_dev(packed.data_ptr(), invalid.data_ptr(), n_bases)

    def sketch_registers(self):
        return torch.from_numpy(self.e.sketch_registers())

    def sketch_merge(self, regs):
        self.e.sketch_merge(regs.cpu().numpy())

    def sketch_estimate(self):
        return self.e.sketch_estimate()

    def sketch_drop(self):
        self.e.sketch_drop()

    def query(self, lo, hi):
        n = lo.shape[0]                                              # (long keys: rows)
        out = torch.zeros(n, dtype=torch.int32, device=self.device)
        if n:
            lo = lo.contiguous()
            hi = hi.contiguous() if hi is not None else None
            self._sync()
            self.e.query_dev(lo.data_ptr(), hi.data_ptr() if hi is not None else None, n, out.data_ptr())
            self.e.synchronize()
        return out

    def count_ge(self, min_count):
        return self.e.count_ge(min_count)

    def stats(self):
        return self.e.stats()

    def histogram(self, high):
        """int64[high + 2] in HBM, written by ``kdf_histogram_dev`` (bin high + 1: counts above ``high``)."""
        bins = torch.empty(int(high) + 2, dtype=torch.int64, device=self.device)
        self._sync()
        self.e.histogram_dev(int(high), bins.data_ptr())           # synchronises the engine's stream
        return bins

    def count_stats(self):
        return self.e.count_stats()


def _u32(t: torch.Tensor) -> torch.Tensor:
    """int32 bit patterns -> non-negative int64 values."""
    return t.to(torch.int64) & _U32_MAX


class ShardedFilterCount:
    """count --if over a read stream sharded across ranks, merged by one all-reduce."""

    def __init__(self, ops: TableOps, group=None, stage_through_host: bool = False):
        self.ops = ops
        self.group = group
        self.host = stage_through_host
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.last_reduce_dtype = None

    def merged_counts(self, keys_lo: torch.Tensor, keys_hi: Optional[torch.Tensor]) -> torch.Tensor:
        """Global count of every filter key (same key order on every rank), saturating at
        2^32-1, as int64 values.  Call after each rank counted its own shard.  Long keys: ``keys_lo`` holds the
        (n, W) rows and ``keys_hi`` is None.

        The counts travel as ONE all-reduce(sum) of 4-byte words (the `ncclUint32` reduce of
        SURVEY.md section 8e): a scalar all-reduce(max) of the largest local count first
        proves that world x max < 2^31, i.e. that the sums stay inside the SIGNED 32-bit range
        the backends reduce in (a sum in [2^31, 2^32) would be signed overflow inside gloo's /
        RCCL's `+`).  Only when that fails (counts within a factor `world` of 2^31) the sum is
        taken in 8-byte words and clamped."""
        local32 = self.ops.query(keys_lo, keys_hi)                 # int32 bit patterns of uint32 counts
        if self.world == 1 or local32.numel() == 0:
            return _u32(local32)
        if self.host:
            local32 = local32.cpu()
        mx = _u32(local32).max().reshape(1)
        dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=self.group)
        if int(mx.item()) * self.world <= 0x7FFFFFFF:
            dist.all_reduce(local32, op=dist.ReduceOp.SUM, group=self.group)   # proven to stay below 2^31
            self.last_reduce_dtype = torch.int32
            out = _u32(local32)
        else:
            wide = _u32(local32)
            dist.all_reduce(wide, op=dist.ReduceOp.SUM, group=self.group)
            self.last_reduce_dtype = torch.int64
            out = torch.clamp(wide, max=_U32_MAX)
        return out.to(keys_lo.device) if self.host else out


def agree_max(value: int, group=None, stage_through_host: bool = False, device=None) -> int:
    """The largest of the ranks' integers (one scalar all-reduce(MAX)); ``value`` itself without a process group."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return int(value)
    t = torch.tensor([int(value)], dtype=torch.int64, device=torch.device("cpu") if stage_through_host or device is None else device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return int(t.item())


def sketch_merge_ranks(ops: TableOps, group=None, stage_through_host: bool = False) -> Tuple[float, float]:
    """Merge the ranks' distinct k-mer sketches (kdf.h "distinct k-mer sketch"): ONE all-reduce(MAX) over the uint8
    registers -- on CPU copies under ``stage_through_host`` -- and every rank takes the result with ``sketch_merge``, so
    every rank holds the registers of the whole sample.  Returns (local estimate, taken before the merge; global
    estimate)."""
    local = float(ops.sketch_estimate())
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return local, local
    regs = ops.sketch_registers().to(torch.device("cpu") if stage_through_host else ops.device).contiguous()
    dist.all_reduce(regs, op=dist.ReduceOp.MAX, group=group)
    ops.sketch_merge(regs.cpu())
    return local, float(ops.sketch_estimate())


def _round8(n: int) -> int:
    return (n + 7) & ~7


class OwnerPartitionedCount:
    """Full count over a sharded read stream: local count, owner-partitioned
    all-to-all of (key, count) pairs, owner-side sum."""

    def __init__(self, local_ops: TableOps, group=None, device=None, owner_ops: Optional[TableOps] = None,
                 make_owner_ops=None, stage_through_host: bool = False):
        """``stage_through_host``: run the collectives on CPU copies (a gloo group over GPU
        engines: rehearsals and tests on a box without one GPU per rank; RCCL takes the device
        tensors directly)."""
        self.host = stage_through_host
        self.local = local_ops
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.device = device if device is not None else local_ops.device
        if owner_ops is None and make_owner_ops is not None:
            owner_ops = make_owner_ops()
        if self.world > 1 and owner_ops is None:
            # summing the received pairs into the table that still holds the local partial counts would
            # count this rank's own keys twice and keep the keys it does not own
            raise ValueError("OwnerPartitionedCount: with more than one rank the owner-side table "
                             "(owner_ops or make_owner_ops) must be distinct from the local one")
        # with one rank the local table already is the global one
        self.owner = owner_ops if self.world > 1 else local_ops
        if self.world > 1 and hasattr(self.owner, "prepare_owner"):
            self.owner.prepare_owner(self.world)
        self._local_stats = (0, 0, 0)
        self.last_exchange_pairs = 0
        self.last_prefilter_rounds = 0

    def local_stats(self):
        """(capacity, distinct, windows) of this rank's LOCAL table.  Reading them applies what the count calls have
        deferred: ask after the last batch, not after every batch."""
        return self.local.stats()

    def exchange(self):
        """Move every locally counted (key, count) pair to its owner rank: one count exchange and ONE
        packed all-to-all (per destination a byte segment [lo words | hi words | counts], starts aligned to 8; long
        keys, rows of W words: [keys: n x W words, row-major | counts], 8 W + 4 bytes per entry, owners by `owner_of_w`)."""
        if self.world == 1:
            return
        packed = self.local.export_packed_by_owner(self.world) if hasattr(self.local, "export_packed_by_owner") else None
        wide = bool(getattr(self.local, "wide", False))
        kw = int(getattr(self.local, "key_words", 0) or 0)
        kw = kw if kw > 2 else 0
        esz = _entry_bytes(wide, kw)
        cdev = torch.device("cpu") if self.host else self.device
        if packed is not None:                       # the engine wrote the send buffer itself, owner by owner, in hash order
            send, s_list, offs = packed
            s_bytes = [offs[p + 1] - offs[p] for p in range(self.world)]
            send_counts = torch.tensor(s_list, dtype=torch.int64)
        else:
            grouped = self.local.export_pairs_by_owner(self.world) if hasattr(self.local, "export_pairs_by_owner") else None
            if grouped is not None:                  # the engine dumps owner by owner: nothing to sort
                lo, hi, cnt, counts = grouped
                send_counts = torch.tensor(counts, dtype=torch.int64)
            else:
                lo, hi, cnt = self.local.export_pairs(0)
                own = owner_of_w(lo, self.world) if kw else owner_of(lo, hi, self.world)
                order = torch.argsort(own, stable=True)
                lo, cnt = lo[order], cnt[order]
                hi = hi[order] if hi is not None else None
                send_counts = torch.bincount(own, minlength=self.world).to(torch.int64).cpu()
            wide = hi is not None
            esz = _entry_bytes(wide, kw)
            kwords = kw or 1                         # words of the first key block of a segment
            s_list = send_counts.tolist()
            s_bytes = [_round8(n * esz) for n in s_list]
            send = torch.empty(sum(s_bytes), dtype=torch.uint8, device=lo.device)
            off = a = 0
            for n, nb in zip(s_list, s_bytes):       # 2-3 contiguous device copies per destination
                if n:
                    send[off:off + 8 * kwords * n].view(torch.int64).copy_(lo[a:a + n].reshape(-1))
                    o2 = off + 8 * kwords * n
                    if hi is not None:
                        send[o2:o2 + 8 * n].view(torch.int64).copy_(hi[a:a + n])
                        o2 += 8 * n
                    send[o2:o2 + 4 * n].view(torch.int32).copy_(cnt[a:a + n])
                off += nb
                a += n
        sc = send_counts.to(cdev)
        rc = torch.empty_like(sc)
        dist.all_to_all_single(rc, sc, group=self.group)
        r_list: List[int] = rc.tolist()
        self.last_exchange_pairs = int(sum(s_list))
        r_bytes = [_round8(n * esz) for n in r_list]
        src = send.cpu() if self.host else send
        recv = torch.empty(sum(r_bytes), dtype=torch.uint8, device=src.device)
        dist.all_to_all_single(recv, src, output_split_sizes=r_bytes, input_split_sizes=s_bytes, group=self.group)
        if self.host:
            recv = recv.to(send.device)
        off = 0
        segments = []
        for n, nb in zip(r_list, r_bytes):           # the owner sums straight from the received segments, all sources at once
            if n:
                kwords = kw or 1
                rlo = recv[off:off + 8 * kwords * n].view(torch.int64)
                if kw:
                    rlo = rlo.view(n, kw)
                o2 = off + 8 * kwords * n
                rhi = None
                if wide and not kw:
                    rhi = recv[o2:o2 + 8 * n].view(torch.int64)
                    o2 += 8 * n
                segments.append((rlo, rhi, recv[o2:o2 + 4 * n].view(torch.int32)))
            off += nb
        if hasattr(self.owner, "add_pairs_segments"):
            self.owner.add_pairs_segments(segments)
        else:
            for seg in segments:
                self.owner.add_pairs(*seg)

    def clear(self):
        self.local.clear()
        if self.owner is not self.local:
            self.owner.clear()

    def count_local(self, packed, invalid, n_bases: int):
        """Count one more batch of this rank's read shard into its LOCAL table (no
        communication: a streamed sample is many such batches, then one merge)."""
        if isinstance(packed, int):
            raise TypeError("pass the stream tensors, not raw pointers")
        self.local.count_stream(packed, invalid, n_bases)

    # ---- two-pass counting over the ranks (kdf.h "two-pass counting": several ranks) ----------------------------------
    # prefilter_begin -> tally_local over every batch of the shard -> prefilter_merge (ends armed) -> count_local over
    # the same batches (gated by the engine) -> exchange / merge as always -> prefilter_drop.  The owner table never
    # has a prefilter.

    def _cdev(self):
        return torch.device("cpu") if self.host else self.device

    def all_ok(self, ok: bool) -> bool:
        """True iff ``ok`` on every rank (one scalar all-reduce): the ranks decide TOGETHER whether a step that can fail
        on one of them alone (a sieve or a table that does not fit its device) went through, before any of them enters
        the next collective."""
        if self.world == 1:
            return bool(ok)
        f = torch.tensor([1 if ok else 0], dtype=torch.int64, device=self._cdev())
        dist.all_reduce(f, op=dist.ReduceOp.MIN, group=self.group)
        return bool(f.item())

    def agree_log2_cells(self, log2_cells: int) -> int:
        """The largest of the ranks' proposals (all-reduce(max)): the merge needs sieves of one size."""
        if self.world == 1:
            return int(log2_cells)
        if not log2_cells:
            raise ValueError("OwnerPartitionedCount.prefilter_begin: with more than one rank log2_cells must be given "
                             "(the engine's own choice depends on each rank's capacity hint; the sieves must have one size)")
        t = torch.tensor([int(log2_cells)], dtype=torch.int64, device=self._cdev())
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return int(t.item())

    def prefilter_begin(self, min_count: int, log2_cells: int = 0) -> int:
        """Start pass 1 on the LOCAL table with the sieve size the ranks agree on; returns that log2_cells."""
        s = self.agree_log2_cells(log2_cells)
        self.local.prefilter_begin(int(min_count), s)
        return s

    def tally_local(self, packed, invalid, n_bases: int):
        """Tally one more batch of this rank's read shard into its sieve (no communication)."""
        if isinstance(packed, int):
            raise TypeError("pass the stream tensors, not raw pointers")
        self.local.prefilter_tally_stream(packed, invalid, n_bases)

    def prefilter_slices(self, n_words: int) -> List[int]:
        """world + 1 bounds: rank r merges sieve words [floor(r n / world), floor((r + 1) n / world))."""
        return [r * n_words // self.world for r in range(self.world + 1)]

    def prefilter_merge(self, chunk_words: Optional[int] = None):
        """Saturating sum of every rank's sieve into every rank's sieve, then arm.  A hand-made reduce-scatter +
        all-gather: every rank sends slice j to rank j (``all_to_all_single``), rank j merges the world - 1 received
        segments into its own slice with ONE ``prefilter_merge`` call, the merged slices are all-gathered and written
        with replace.  Per-rank traffic 2 x sieve bytes x (world - 1) / world, in rounds of at most ``chunk_words``
        words per peer (default: staging below 1 GB)."""
        if self.world > 1:
            n = self.local.prefilter_words()
            W, me = self.world, self.rank
            if chunk_words is None:
                chunk_words = max(2, (10 ** 9 // (8 * 3 * W)) & ~1)     # send + receive + gather buffers: 3 W chunk words
            chunk_words = max(1, int(chunk_words))
            b = self.prefilter_slices(n)
            longest = max(b[j + 1] - b[j] for j in range(W))
            cdev = self._cdev()
            self.last_prefilter_rounds = 0
            for off in range(0, longest, chunk_words):
                first = [min(b[j] + off, b[j + 1]) for j in range(W)]
                c = [min(chunk_words, b[j + 1] - first[j]) for j in range(W)]   # this round's piece of slice j (the last ones are ragged)
                # reduce-scatter: piece j goes to rank j
                s_split = [0 if j == me else c[j] for j in range(W)]
                r_split = [0 if j == me else c[me] for j in range(W)]
                send = torch.cat([self.local.prefilter_export(first[j], s_split[j]) for j in range(W)]).to(cdev)
                recv = torch.empty(sum(r_split), dtype=torch.int64, device=cdev)
                dist.all_to_all_single(recv, send, output_split_sizes=r_split, input_split_sizes=s_split, group=self.group)
                if c[me]:
                    recv = recv.to(self.device)
                    self.local.prefilter_merge(first[me], list(recv.split(c[me])), replace=False)
                # all-gather of the merged pieces (padded to the longest piece of the round)
                cmax = max(c)
                mine = torch.zeros(cmax, dtype=torch.int64, device=cdev)
                mine[:c[me]] = self.local.prefilter_export(first[me], c[me]).to(cdev)
                outs = [torch.empty_like(mine) for _ in range(W)]
                dist.all_gather(outs, mine, group=self.group)
                for j in range(W):
                    if j != me and c[j]:
                        self.local.prefilter_merge(first[j], [outs[j][:c[j]].to(self.device)], replace=True)
                self.last_prefilter_rounds += 1
        self.local.prefilter_arm()

    def prefilter_drop(self):
        self.local.prefilter_drop()

    def prefilter_windows(self) -> int:
        """Windows tallied by all ranks together: all-reduce(sum) of the ranks' ``prefilter_windows``."""
        t = torch.tensor([int(self.local.prefilter_windows())], dtype=torch.int64, device=self._cdev())
        if self.world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return int(t.item())

    # ---- distinct k-mer sketch over the ranks (kdf.h "distinct k-mer sketch") ------------------------------------------
    # sketch_begin -> sketch_local over every batch of the shard -> sketch_merge: a register is a max over windows, so the
    # element-wise max of the ranks' registers is the sketch of the whole sample, and every rank ends up holding it --
    # whatever the ranks size from it, they size alike.

    def sketch_begin(self, log2_registers: int = 0) -> int:
        """Start a sketch on the LOCAL table's engine with the register count the ranks agree on (the largest
        proposal; 0: the engine's default, 16); returns that log2_registers."""
        p = agree_max(int(log2_registers) or 16, self.group, self.host, self.device)
        self.local.sketch_begin(p)
        return p

    def sketch_local(self, packed, invalid, n_bases: int):
        """Sketch one more batch of this rank's read shard (no communication)."""
        if isinstance(packed, int):
            raise TypeError("pass the stream tensors, not raw pointers")
        self.local.sketch_add_stream(packed, invalid, n_bases)

    def sketch_merge(self) -> Tuple[float, float]:
        """ONE all-reduce(MAX) over the uint8 registers; every rank then holds the sample's registers.  Returns
        (local estimate, taken before the merge; global estimate)."""
        return sketch_merge_ranks(self.local, self.group, self.host)

    def merge(self, min_count: int = 1) -> int:
        """Exchange the local (key, count) pairs to their owners; returns the global
        number of keys with count >= min_count (``dump -L``)."""
        self.exchange()
        n = torch.tensor([self.owner.count_ge(min_count)], dtype=torch.int64, device="cpu" if self.host else self.device)
        if self.world > 1:
            dist.all_reduce(n, op=dist.ReduceOp.SUM, group=self.group)
        return int(n.item())

    def histogram(self, high: int = 10000) -> torch.Tensor:
        """Global count histogram (`jellyfish histo` of the merged table) as int64[high + 2]; call after
        ``exchange()``: every key then lives on exactly one owner, so the global bins are ONE all-reduce(sum) of
        the owners' bins.  With one rank it is the local table's."""
        bins = self.owner.histogram(int(high))
        if self.world > 1:
            red = bins.cpu() if self.host else bins
            dist.all_reduce(red, op=dist.ReduceOp.SUM, group=self.group)
            bins = red.to(bins.device) if self.host else red
        return bins

    def count_stats(self) -> dict:
        """Global `jellyfish stats` after ``exchange()``: unique / distinct / total by all-reduce(sum) of the
        owners' numbers, max_count by all-reduce(max)."""
        st = self.owner.count_stats()
        if self.world > 1:
            cdev = "cpu" if self.host else self.device
            sums = torch.tensor([st["unique"], st["distinct"], st["total"]], dtype=torch.int64, device=cdev)
            mx = torch.tensor([st["max_count"]], dtype=torch.int64, device=cdev)
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.group)
            dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=self.group)
            u, d, t = (int(x) for x in sums.tolist())
            st = {"unique": u, "distinct": d, "total": t, "max_count": int(mx.item())}
        return st

    def count_and_merge(self, packed, invalid, n_bases: int, min_count: int = 1) -> int:
        """clear -> count the local shard -> exchange -> global number of keys
        with count >= min_count."""
        self.clear()
        self.count_local(packed, invalid, n_bases)
        return self.merge(min_count)
