"""Drop-in mirror of the hot-path helpers of
``kmer_denovo_filter/discovery/pipeline.py`` (Modules 1-2):

    _extract_child_kmers_discovery   reference :69-268
    _subtract_reference_kmers        reference :271-319
    _count_parent_jellyfish          reference :322-459
    _filter_parents_discovery        reference :462-612

Same names, arguments, return values, intermediate files
(``child_candidates.fa`` -> ``child_non_ref_kmers.fa`` -> ``after_mother.fa`` ->
``proband_unique.fa``, each ``>{i}\\n{KMER}\\n``) and RuntimeError convention.
The orchestration above these helpers (run_discovery_pipeline, clustering,
writers) is out of scope and unchanged.
"""
from __future__ import annotations

import logging
import os
import time

import numpy as np

from .. import devkeys, dist_env, jf_io, keys
from .._native import KdfError
from ..core.jellyfish_wrappers import (
    _device,
    _engine_capacity_hint,
    _estimate_jf_hash_size,
    _sample_bytes,
    _format_elapsed,
    _format_file_size,
    _merge_filter_counts,
    _sketch_bam,
    _stream_bam,
)
from ..engine import mirror_engine
from ..kmer_fasta import (device_fasta, load_kmer_set, read_kmer_fasta_keys_device, remove_with_sidecar, store_kmer_set)
from ..reads import refuse_fastq

logger = logging.getLogger(__name__)


def _child_key_parts(child_bam, device=0, world=1, kmer_size=31):
    """Slices of the key space for the child count: ``KDF_KEY_PARTS`` when set, else from the BAM size and
    the free HBM.  Rule of thumb (30x human WGS: ~0.6 BAM bytes per base, ~0.14 distinct 31-mers per base with
    0.5 % errors): distinct ~ 0.23 x BAM bytes, table bytes ~ 12 x distinct / 0.6 ~ 4.6 x BAM bytes; the table
    may take 70 % of what is free (the rest is partition scratch and growth).  Long k-mers (odd 65..201): slots of
    8 W + 4 bytes instead of 12 (W = 3..7 key words, 28..60 bytes), so the estimate grows by that ratio.  Small
    inputs give 1."""
    env = os.environ.get("KDF_KEY_PARTS")
    if env:
        return max(1, int(env))
    need = _child_table_bytes(child_bam, world, kmer_size)
    return max(1, int(-(-need // max(1.0, 0.7 * _device_free_bytes(device)))))


def _device_free_bytes(device):
    from ctypes import byref, c_uint64
    from .. import _native
    free, total = c_uint64(0), c_uint64(0)
    _native.check(_native.load().kdf_device_memory(device, byref(free), byref(total)))
    return free.value


def _child_table_bytes(child_bam, world=1, kmer_size=31):
    """Table bytes the rule of thumb of _child_key_parts plans for the whole key space of one rank."""
    need = 4.6 * _sample_bytes(child_bam) / max(1, world)      # (several ranks: every rank holds its share of the keys twice -- local + owned)
    W = keys.key_words(kmer_size)
    if W > 2:
        need *= (8 * W + 4) / 12.0
    return need


# How the last child count of this process ran: {"mode": "plain" | "two_pass" | "two_pass_sharded", "L", "log2_cells",
# "world"} (L and log2_cells 0 without a prefilter).  For logs and tests; nothing reads it to decide anything.
LAST_CHILD_COUNT = None


# What the read spool of the last child count did: {"used" (KDF_SPOOL=1 and a spool was created), "segments", "positions",
# "hbm_bytes", "host_bytes", "overflowed", "bam_passes" (passes of THIS rank through the BAM feeder)}.  For logs and tests.
LAST_CHILD_SPOOL = None


# What the sketch-sized child count (KDF_SIZE_FROM_SKETCH=1) planned: {"log2_registers", "windows" (this rank's), "local_estimate",
# "global_estimate", "capacity_hint" (of the local engine, per key slice), "key_parts" (agreed by all ranks), "world"}; None
# when the mode is off.  LAST_CHILD_SKETCH_REGISTERS: the (merged) registers, uint8[2^p].  For logs and tests.
LAST_CHILD_SKETCH = None
LAST_CHILD_SKETCH_REGISTERS = None


# How the last _filter_parents_discovery took a parent's survivors: "query" (kdf_query_dev and a mask) or "join" (the table
# join under KDF_DEVICE_JOIN=1); None before the first.  For logs and tests; nothing reads it to decide anything.
LAST_PARENT_FILTER = None


def _sketch_margin(log2_registers):
    """What a table sized from the sketch's estimate adds to it: five standard errors of HyperLogLog (1.04 / sqrt(m):
    8.1 % at p = 12, 2.0 % at p = 16) plus 5 % for the classic estimator's bias between 2.5 m and 5 m (kdf.h)."""
    return 1.05 + 5 * 1.04 / float(1 << int(log2_registers)) ** 0.5


def _table_bytes(n_keys, kmer_size):
    """Bytes of the table kdf_create allocates for a capacity hint: 2^ceil(log2(2 n)) slots (at least 2^10) of 8 W + 4 bytes."""
    slots = max(1 << 10, 1 << (2 * max(int(n_keys), 1) - 1).bit_length())
    return slots * (8 * keys.key_words(kmer_size) + 4)


def _child_sketch_plan(passes, child_bam, ref_fasta, kmer_size, threads):
    """The sizing pass of KDF_SIZE_FROM_SKETCH=1: sketch every window of this rank's reads (kdf.h "distinct k-mer sketch") --
    on the pass that fills the read spool when there is one, as an extra pass over the BAM otherwise -- merge the ranks'
    sketches, and plan from the estimates: the local engine's capacity hint (the local estimate), the owner engine's (the
    global estimate x this rank's share of the key space, 1 / world) and the number of key slices, from the bytes of both
    tables and the HBM that is free now.  ``key_parts`` (``KDF_KEY_PARTS`` when set) is agreed with an all-reduce(MAX):
    every rank plans from its own free HBM, and ranks that disagreed would hang in mismatched collectives.  Returns
    (key_parts, local capacity hint, owner capacity hint) per slice."""
    global LAST_CHILD_SKETCH, LAST_CHILD_SKETCH_REGISTERS
    from ..distributed import agree_max
    world, rank, host = dist_env.world_rank()
    device = _device()
    dev = None
    if world > 1:
        import torch
        dev = torch.device("cuda", device)
    p = agree_max(int(os.environ.get("KDF_SKETCH_LOG2M") or 0) or 16, None, host, dev)
    with mirror_engine(kmer_size, capacity_hint=1, device=device) as sk:      # (its table stays empty: the sketch stores no key)
        sk.sketch_begin(p)
        if passes.spool is None:
            logger.info("Sizing the child count from a sketch without a read spool (KDF_SPOOL=1): an extra pass over the BAM")
        passes.run(sk, child_bam, ref_fasta, threads, sketch=True)
        windows = sk.get_stat("sketch_windows")
        if world > 1:
            from ..distributed import EngineOps, sketch_merge_ranks
            local_est, global_est = sketch_merge_ranks(EngineOps(sk, dev), None, host)
        else:
            local_est = global_est = sk.sketch_estimate()
        LAST_CHILD_SKETCH_REGISTERS = sk.sketch_registers()
        sk.sketch_drop()
    margin = _sketch_margin(p)
    local_keys = local_est * margin
    owner_keys = global_est / world * margin if world > 1 else 0.0
    env = os.environ.get("KDF_KEY_PARTS")
    if env:
        parts = max(1, int(env))
    else:
        room = 0.7 * _device_free_bytes(device)                  # (the rest: partition scratch and growth, as in _child_key_parts)
        parts = 1
        while parts < (1 << 16) and (_table_bytes(local_keys / parts, kmer_size)
                                     + (_table_bytes(owner_keys / parts, kmer_size) if world > 1 else 0)) > room:
            parts += 1
    parts = agree_max(parts, None, host, dev)
    local_cap = max(1, int(-(-local_keys // parts)))
    owner_cap = max(1, int(-(-owner_keys // parts)))
    LAST_CHILD_SKETCH = {"log2_registers": p, "windows": windows, "local_estimate": local_est, "global_estimate": global_est,
                         "capacity_hint": local_cap, "key_parts": parts, "world": world}
    logger.info("Child count sized from a sketch of 2^%d registers: %d windows, about %.0f distinct k-mers in this rank's reads, "
                "%.0f in all ranks' (%d); capacity hint %d (owner table %d), %d key slice(s)",
                p, windows, local_est, global_est, world, local_cap, owner_cap, parts)
    return parts, local_cap, owner_cap


class _ChildPasses:
    """The passes of one child count over the child BAM.  Without ``KDF_SPOOL=1`` every pass is ``_stream_bam``, as it
    always was.  With it the first pass also fills a read spool (kdf.h "read spool") and every later pass is a replay of
    the spool; a spool that overflows its budgets is logged and dropped, and the later passes stream the BAM again -- the
    counts are the same either way.  Budgets: ``KDF_SPOOL_HBM_GB`` (default: the HBM that is free now, minus
    ``reserve_bytes`` -- the table the slice planner plans for and the sieve -- never negative) and ``KDF_SPOOL_HOST_GB``
    (pinned host memory, default 0: nobody has measured what these hosts can pin)."""

    def __init__(self, device, reserve_bytes=0):
        self.spool, self.filled, self.bam_passes = None, False, 0
        self.info = {"used": False, "segments": 0, "positions": 0, "hbm_bytes": 0, "host_bytes": 0, "overflowed": False}
        if os.environ.get("KDF_SPOOL") != "1":
            return
        from ..spool import ReadSpool
        env = os.environ.get("KDF_SPOOL_HBM_GB")
        hbm = float(env) * 1e9 if env else _device_free_bytes(device) - reserve_bytes
        host = float(os.environ.get("KDF_SPOOL_HOST_GB") or 0) * 1e9
        self.spool = ReadSpool(device, max(0, int(hbm)), max(0, int(host)))
        self.info["used"] = True
        logger.info("Read spool on: up to %.1f GB of HBM and %.1f GB of pinned host memory", max(0.0, hbm) / 1e9, max(0.0, host) / 1e9)

    def _note(self):
        for name in ("segments", "positions", "hbm_bytes", "host_bytes"):
            self.info[name] = self.spool.stat(name)

    def run(self, eng, child_bam, ref_fasta, threads, tally=False, sketch=False):
        """One pass: count, or ``tally`` into the prefilter, or ``sketch`` (nothing is counted: the sizing pass)."""
        if self.spool is None:
            self.bam_passes += 1
            if sketch:
                return _sketch_bam(eng, child_bam, ref_fasta, threads)
            return _stream_bam(eng, child_bam, ref_fasta, threads, filtered=False, tally=tally)
        if self.filled:
            if sketch:
                return self.spool.sketch(eng)
            return self.spool.replay(eng, self.spool.TALLY if tally else self.spool.COUNT)
        self.bam_passes += 1
        if sketch:
            n = _sketch_bam(eng, child_bam, ref_fasta, threads, spool=self.spool)
        else:
            n = _stream_bam(eng, child_bam, ref_fasta, threads, filtered=False, tally=tally, spool=self.spool)
        self._note()
        if self.spool.stat("overflowed"):
            logger.info("Read spool overflowed after %d positions (%.1f GB of HBM, %.1f GB of host memory): dropped, the "
                        "remaining passes stream the BAM", self.info["positions"], self.info["hbm_bytes"] / 1e9, self.info["host_bytes"] / 1e9)
            self.info["overflowed"] = True
            self.spool.close()
            self.spool = None
        else:
            self.filled = True
            logger.info("Read spool holds the sample: %d positions in %d segments (%.1f GB of HBM, %.1f GB of host memory)",
                        self.info["positions"], self.info["segments"], self.info["hbm_bytes"] / 1e9, self.info["host_bytes"] / 1e9)
        return n

    def close(self):
        global LAST_CHILD_SPOOL
        if self.spool is not None:
            self.spool.close()
            self.spool = None
        LAST_CHILD_SPOOL = dict(self.info, bam_passes=self.bam_passes)


def _child_prefilter_min(min_child_count, world):
    """The L of the two-pass child count, or 0 when it is off: opt-in (``KDF_PREFILTER=1``) and a dump bound of at least
    2.  A cell of the sieve saturates at 3, so ``-L 5`` tallies with 3 and dumps with 5.  Several ranks: every rank
    tallies its share of the reads and the sieves are merged before any rank counts (_child_count_two_pass_sharded)."""
    if os.environ.get("KDF_PREFILTER") != "1" or min_child_count < 2:
        return 0
    return min(int(min_child_count), 3)


def _child_count_two_pass(child_bam, ref_fasta, kmer_size, min_child_count, threads, jf_hash_size, extract_start,
                          dump=None):
    """`jellyfish bc` + `count --bc` made exact: stream the BAM twice -- tally every window into the counting sieve, arm,
    count -- so that only k-mers whose cell was seen >= L times get a table slot, each with its full count; then
    ``dump -L min_child_count`` as usual, one slice.  Returns the candidates (device keys), or None when the sieve plus the
    table of the admitted keys do not fit the device (the caller then counts in key_parts slices without a prefilter)."""
    from .. import _native
    global LAST_CHILD_COUNT
    L = _child_prefilter_min(min_child_count, 1)
    hint = _engine_capacity_hint(jf_hash_size, child_bam)            # distinct k-mers expected, errors included
    log2_cells = min(38, max(16, (8 * max(int(hint), 1) - 1).bit_length()))
    with mirror_engine(kmer_size, capacity_hint=1 << 16, device=_device()) as eng:
        passes = _ChildPasses(eng.device, _child_table_bytes(child_bam, 1, kmer_size) + (1 << (log2_cells - 1)))
        try:
            eng.prefilter_begin(L, log2_cells)
            passes.run(eng, child_bam, ref_fasta, threads, tally=True)
            fill = eng.prefilter_fill()
            eng.prefilter_arm()
            eng.reserve(fill[L] + (fill[3] if L == 2 else 0) + 1)    # about one admitted key per cell that reads >= L
            passes.run(eng, child_bam, ref_fasta, threads)
            cap, distinct, windows = eng.stats()
        except KdfError as e:
            if e.code != _native.KDF_ERR_NOMEM:
                raise
            logger.info("Two-pass child count: a sieve of 2^%d cells plus the table of the admitted k-mers do not fit the device "
                        "(%s); counting in key-space slices without a prefilter", log2_cells, e)
            return None
        finally:
            passes.close()
        logger.info("Child k-mer counting complete (%s, two passes, L=%d, sieve 2^%d cells reading 0/1/2/3: %d/%d/%d/%d, "
                    "%d of %d windows admitted, %d distinct stored, table %d slots)", _format_elapsed(time.monotonic() - extract_start),
                    L, log2_cells, fill[0], fill[1], fill[2], fill[3], windows, eng.get_stat("prefilter_windows"), distinct, cap)
        logger.info("Dumping child k-mers with count >= %d…", min_child_count)
        dlo, dhi = (dump or devkeys.dump_ge)(eng, min_child_count, eng.device)
        LAST_CHILD_COUNT = {"mode": "two_pass", "L": L, "log2_cells": log2_cells, "world": 1}
        return devkeys.select([(dlo, dhi)])


def _child_count_two_pass_sharded(child_bam, ref_fasta, kmer_size, min_child_count, threads, jf_hash_size, extract_start):
    """The two-pass child count over several ranks (kdf.h "two-pass counting": several ranks).  Every rank tallies its
    BGZF ranges; the sieves are merged with a saturating sum, so every rank holds the sieve of the WHOLE sample and
    admits the same keys; every rank counts its ranges again, gated; then the owner exchange and ``dump -L`` on the
    owners as in the plain sharded count.  The owner engine never has a prefilter.  Returns the gathered candidates, or
    None -- ON EVERY RANK -- when the sieve or a table did not fit on ANY rank: a rank that runs out of memory must not
    leave the others waiting in a collective, so the ranks all-reduce an "it went through here" flag after every step
    that can fail locally and before the next collective."""
    import torch
    from .. import _native
    from ..distributed import EngineOps, OwnerPartitionedCount
    global LAST_CHILD_COUNT
    world, rank, host = dist_env.world_rank()
    L = _child_prefilter_min(min_child_count, world)
    hint = _engine_capacity_hint(jf_hash_size, child_bam)            # distinct k-mers expected in the WHOLE sample
    proposal = min(38, max(16, (8 * max(int(hint), 1) - 1).bit_length()))
    eng = owner_eng = passes = None
    try:
        eng = mirror_engine(kmer_size, capacity_hint=1 << 16, device=_device())
        owner_eng = mirror_engine(kmer_size, capacity_hint=1 << 16, device=eng.device)
        dev = torch.device("cuda", eng.device)
        merger = OwnerPartitionedCount(EngineOps(eng, dev), device=dev, owner_ops=EngineOps(owner_eng, dev), stage_through_host=host)
        log2_cells = merger.agree_log2_cells(proposal)
        # (every rank spools its own BGZF ranges: the reader of a pass is this rank's share of the file)
        passes = _ChildPasses(eng.device, _child_table_bytes(child_bam, world, kmer_size) + (1 << (log2_cells - 1)))
        state = {"why": None}

        def step(fn):
            """run a rank-local step; True iff it went through on EVERY rank"""
            ok = True
            try:
                fn()
            except KdfError as e:
                if e.code != _native.KDF_ERR_NOMEM:
                    raise
                ok, state["why"] = False, str(e)
            return merger.all_ok(ok)

        def give_up(what):
            logger.info("Two-pass child count over %d ranks: %s did not fit the device on %s (%s); counting in key-space "
                        "slices without a prefilter", world, what, "this rank" if state["why"] else "another rank", state["why"] or "-")
            return None

        def tally():
            eng.prefilter_begin(L, log2_cells)
            passes.run(eng, child_bam, ref_fasta, threads, tally=True)

        if not step(tally):
            return give_up("a sieve of 2^%d cells" % log2_cells)
        merger.prefilter_merge()                                     # ends armed: every rank holds the sieve of all reads
        fill = eng.prefilter_fill()                                  # (the same on every rank: the global fill)
        tallied = merger.prefilter_windows()
        st = {}

        def count():
            eng.reserve(fill[L] + (fill[3] if L == 2 else 0) + 1)    # at most about one admitted key per cell that reads >= L
            passes.run(eng, child_bam, ref_fasta, threads)
            st["stats"] = eng.stats()

        if not step(count):
            return give_up("the table of the admitted k-mers")
        cap, distinct, windows = st["stats"]
        logger.info("Child k-mer counting complete (%s, two passes over %d ranks, L=%d, sieve 2^%d cells reading 0/1/2/3: %d/%d/%d/%d "
                    "(all ranks), %d windows tallied by all ranks; this rank: %d windows admitted, %d distinct stored, table %d slots)",
                    _format_elapsed(time.monotonic() - extract_start), world, L, log2_cells, fill[0], fill[1], fill[2], fill[3],
                    tallied, windows, distinct, cap)
        logger.info("Dumping child k-mers with count >= %d…", min_child_count)
        if not step(merger.exchange):
            return give_up("an owner table")
        dlo, dhi = devkeys.dump_ge(owner_eng, min_child_count, eng.device)
        dlo, dhi = dist_env.all_gather_keys(dlo, dhi)               # every rank holds the whole candidate set
        LAST_CHILD_COUNT = {"mode": "two_pass_sharded", "L": L, "log2_cells": log2_cells, "world": world,
                            "exchange_pairs": merger.last_exchange_pairs}
        return devkeys.select([(dlo, dhi)])
    finally:
        if passes is not None:
            passes.close()
        for e in (owner_eng, eng):
            if e is not None:
                e.close()


def _count_and_dump_child(child_bam, ref_fasta, kmer_size, min_child_count, threads, jf_hash_size, dump=None):
    """The counting half of Module 1: count every canonical child k-mer (plain, in key slices, two-pass, sharded) and
    take what ``dump(eng, min_child_count, device)`` gives of every slice's table -- ``devkeys.dump_ge`` (None: looked up
    when it is called) for Module 1,
    a join against the reference for the fused stage (_extract_child_non_ref_kmers; one rank only: the sharded paths
    dump their owner tables with ``dump_ge``).  Returns (device key set, lo, hi, start of the last dump), ascending."""
    global LAST_CHILD_COUNT, LAST_CHILD_SKETCH, LAST_CHILD_SKETCH_REGISTERS
    LAST_CHILD_SKETCH = LAST_CHILD_SKETCH_REGISTERS = None
    if jf_hash_size is None:
        jf_hash_size = _estimate_jf_hash_size(child_bam, kmer_size, default="1G")
    logger.info("Extracting child k-mers from BAM (k=%d, jf hash size=%s)…", kmer_size, jf_hash_size)
    extract_start = time.monotonic()
    # A 30x human sample has ~10^10 distinct 31-mers (sequencing errors included): more than one table in
    # 288 GB of HBM holds.  KDF_KEY_PARTS = P counts the key space in P slices, one pass over the BAM each
    # (Jellyfish's answer to the same problem is to spill and merge hash files, jellyfish_wrappers.py:335-366).
    world, rank, host = dist_env.world_rank()
    parts = _child_key_parts(child_bam, _device(), world, kmer_size)
    owner_eng = merger = passes = None
    dump_start = time.monotonic()
    try:
        cand = None
        LAST_CHILD_COUNT = {"mode": "plain", "L": 0, "log2_cells": 0, "world": world}
        if _child_prefilter_min(min_child_count, world):
            if world == 1:
                cand = _child_count_two_pass(child_bam, ref_fasta, kmer_size, min_child_count, threads, jf_hash_size, extract_start, dump)
            else:
                cand = _child_count_two_pass_sharded(child_bam, ref_fasta, kmer_size, min_child_count, threads, jf_hash_size, extract_start)
        if cand is not None:
            lo, hi = devkeys.to_host(*cand)
        else:
            local_hint = max(1, _engine_capacity_hint(jf_hash_size, child_bam) // parts)
            local_cap, owner_cap = max(1, local_hint // world) if world > 1 else local_hint, max(1, local_hint // world)
            if os.environ.get("KDF_SIZE_FROM_SKETCH") == "1":
                # opt-in: tables and key slices sized from a distinct-count sketch of the reads, not from the BAM's size
                passes = _ChildPasses(_device(), _child_table_bytes(child_bam, world, kmer_size) / parts)
                parts, local_cap, owner_cap = _child_sketch_plan(passes, child_bam, ref_fasta, kmer_size, threads)
            with mirror_engine(kmer_size, capacity_hint=local_cap, device=_device()) as eng:
                if world > 1:
                    # one process per GPU: every rank counts its ranges of the BAM into a local table, one owner-partitioned
                    # exchange moves each (k-mer, count) pair to the rank that owns the k-mer, the owner sums -- and `dump -L`
                    # runs on the owners' tables (distributed.OwnerPartitionedCount; SURVEY.md section 8e "full count stage")
                    import torch
                    from ..distributed import EngineOps, OwnerPartitionedCount
                    dev = torch.device("cuda", eng.device)
                    owner_eng = mirror_engine(kmer_size, capacity_hint=owner_cap, device=eng.device)
                    merger = OwnerPartitionedCount(EngineOps(eng, dev), device=dev, owner_ops=EngineOps(owner_eng, dev), stage_through_host=host)
                dev_sets = []
                if parts > 1:
                    eng.set_option("key_parts", parts)
                # (slice 0 streams the BAM; with KDF_SPOOL=1 it also spools it and slices 1 .. P-1 replay the spool)
                if passes is None:
                    passes = _ChildPasses(eng.device, _child_table_bytes(child_bam, world, kmer_size) / parts)
                for part in range(parts):
                    if parts > 1:
                        eng.clear(); eng.set_option("key_part", part)
                        if owner_eng is not None:
                            owner_eng.clear()
                    passes.run(eng, child_bam, ref_fasta, threads)
                    cap, distinct, windows = eng.stats()
                    logger.info("Child k-mer counting complete (%s, slice %d of %d, %d windows, %d distinct, table %d slots)",
                                _format_elapsed(time.monotonic() - extract_start), part + 1, parts, windows, distinct, cap)
                    logger.info("Dumping child k-mers with count >= %d…", min_child_count)
                    dump_start = time.monotonic()
                    # the dump stays in HBM for the next stage (ascending keys: Jellyfish's dump order is not reproducible and
                    # nothing downstream relies on it, but the contract files are then the same bytes on every run)
                    if merger is None:
                        dlo, dhi = (dump or devkeys.dump_ge)(eng, min_child_count, eng.device)
                    else:
                        merger.exchange()
                        dlo, dhi = devkeys.dump_ge(owner_eng, min_child_count, eng.device)
                        dlo, dhi = dist_env.all_gather_keys(dlo, dhi)           # every rank holds the whole candidate set
                    dev_sets.append((dlo, dhi))
                cand = devkeys.select(dev_sets)
                lo, hi = devkeys.to_host(*cand)
    except KdfError as e:
        raise RuntimeError(f"jellyfish count (child) failed: {e}") from e
    finally:
        if passes is not None:
            passes.close()                                         # (synchronises the device: no replayed count still reads a segment)
        if owner_eng is not None:
            owner_eng.close()
    if world > 1:                                                  # (rank order of the gathered sets is not key order)
        import torch
        order = keys.order(keys.from_pair(lo, hi, kmer_size))
        lo, hi = lo[order], (hi[order] if hi is not None else None)   # (long keys: rows, no hi)
        cand = devkeys.select([cand], torch.from_numpy(order).to(cand[0].device))
    return cand, lo, hi, dump_start


def _extract_child_kmers_discovery(child_bam, ref_fasta, kmer_size, min_child_count, threads, tmpdir,
                                   jf_hash_size=None):
    """Module 1: count every canonical child k-mer, keep count >= min_child_count.

    Returns (child_candidates_fa, n_candidates)."""
    child_candidates_fa = os.path.join(tmpdir, "child_candidates.fa")
    cand, lo, hi, dump_start = _count_and_dump_child(child_bam, ref_fasta, kmer_size, min_child_count, threads, jf_hash_size)
    rank = dist_env.world_rank()[1]
    n_candidates = len(lo)
    if rank == 0:
        store_kmer_set(child_candidates_fa, kmer_size, cand, (lo, hi))
    dist_env.barrier()                                             # the file exists (and has its final size) on every rank
    devkeys.register(child_candidates_fa, *cand, kmer_size)
    logger.info("Child k-mer dump complete (%s, %d candidates, FASTA: %s)",
                _format_elapsed(time.monotonic() - dump_start), n_candidates,
                _format_file_size(child_candidates_fa))
    logger.info("Child candidate k-mers (count >= %d): %d", min_child_count, n_candidates)
    return child_candidates_fa, n_candidates


def _index_k(ref_jf):
    header, _ = jf_io.read_header(ref_jf)
    return int(header["key_len"]) // 2


def _subtract_reference_kmers(ref_jf, child_candidates_fa, tmpdir):
    """Keep the candidates whose count in the reference index is 0
    (``jellyfish query ref.jf -s candidates.fa`` + ``== "0"``).  Deletes the
    input FASTA.  Returns (child_non_ref_fa, n_non_ref)."""
    child_non_ref_fa = os.path.join(tmpdir, "child_non_ref_kmers.fa")
    try:
        k = _index_k(ref_jf)
        dev = devkeys.lookup(child_candidates_fa, k)             # the candidates are still in HBM when Module 1 ran here
        if dev is None and device_fasta():                       # (KDF_DEVICE_FASTA=1: parsed where it is used)
            dev = read_kmer_fasta_keys_device(child_candidates_fa, k, device=_device())
        elif dev is None:
            lo, hi = load_kmer_set(child_candidates_fa, k)
            dev = devkeys.from_host(lo, hi, k > 32) if len(lo) else None
        world, rank, host = dist_env.world_rank()
        if dev is not None and dev[0].numel():
            with mirror_engine(k, capacity_hint=max(jf_io.index_records(ref_jf) // world, 1), device=_device()) as eng:
                # memory-mapped, block by block (a human index is 30 GB); several ranks: every rank loads ITS share of the
                # index's records and answers for all candidates, one all-reduce(sum) gives `jellyfish query`'s counts
                jf_io.load_index_into(eng, ref_jf, part=rank, parts=world)
                if world == 1:
                    keep = devkeys.query(eng, dev[0], dev[1], eng.device) == 0
                else:
                    import torch
                    from ..distributed import EngineOps, ShardedFilterCount
                    keep = ShardedFilterCount(EngineOps(eng, torch.device("cuda", eng.device)), stage_through_host=host).merged_counts(dev[0], dev[1]) == 0
            dlo, dhi = devkeys.select([dev], keep)
            lo, hi = devkeys.to_host(dlo, dhi)
        else:
            dlo = dhi = None
            lo = hi = np.zeros(0, np.uint64)
    except (KdfError, ValueError, OSError) as e:
        raise RuntimeError(f"jellyfish query (ref subtraction) failed: {e}") from e
    n_non_ref = len(lo)
    dist_env.barrier()                                             # every rank has read what it needs of the input file
    if dist_env.is_root():
        store_kmer_set(child_non_ref_fa, k, (dlo, dhi) if dlo is not None else None, (lo, hi), _device())
        remove_with_sidecar(child_candidates_fa)
    dist_env.barrier()
    if dlo is not None:
        devkeys.register(child_non_ref_fa, dlo, dhi, k)
    devkeys.forget(child_candidates_fa)
    logger.info("Non-reference child k-mers after subtraction: %d", n_non_ref)
    return child_non_ref_fa, n_non_ref


def _extract_child_non_ref_kmers(child_bam, ref_fasta, ref_jf, kmer_size, min_child_count, threads, tmpdir,
                                 jf_hash_size=None):
    """Module 1 and the reference subtraction in one call (opt-in): the reference index is loaded into
    an engine first, the child is counted exactly as _extract_child_kmers_discovery counts it, and every slice's table
    is dumped by a join against the reference's (``devkeys.dump_join``: count >= min_child_count here, count 0 there)
    in place of ``dump -L``.  ``child_candidates.fa`` is never written; ``child_non_ref_kmers.fa`` is, with the bytes
    the two stages write.  Several ranks: the two stages run in turn.

    Returns (child_non_ref_fa, n_candidates, n_non_ref)."""
    world, rank, host = dist_env.world_rank()
    if world > 1:
        logger.info("Fused extract-and-subtract stage under %d ranks: running Module 1 and the reference subtraction in turn", world)
        cand_fa, n_candidates = _extract_child_kmers_discovery(child_bam, ref_fasta, kmer_size, min_child_count, threads, tmpdir,
                                                               jf_hash_size)
        child_non_ref_fa, n_non_ref = _subtract_reference_kmers(ref_jf, cand_fa, tmpdir)
        return child_non_ref_fa, n_candidates, n_non_ref
    child_non_ref_fa = os.path.join(tmpdir, "child_non_ref_kmers.fa")
    ref_eng = None
    try:
        try:
            k = _index_k(ref_jf)
            if k != int(kmer_size):
                raise ValueError(f"{ref_jf} is an index of {k}-mers, the child is counted at k={kmer_size}")
            # loaded BEFORE the child is planned: the slice planner and the spool budget read the HBM that is free then,
            # which no longer holds the reference table's bytes
            ref_eng = mirror_engine(k, capacity_hint=max(jf_io.index_records(ref_jf), 1), device=_device())
            jf_io.load_index_into(ref_eng, ref_jf)
            ref_eng.flush()
            logger.info("Reference index loaded for the join: %d k-mers, table %d slots", ref_eng.stats()[1], ref_eng.stats()[0])
        except (KdfError, ValueError, OSError) as e:
            raise RuntimeError(f"jellyfish query (ref subtraction) failed: {e}") from e
        seen = {"candidates": 0}

        def dump(eng, min_count, device):
            n = eng.count_ge(min_count)
            seen["candidates"] += n
            logger.info("Child candidate k-mers (count >= %d) in this table: %d; joining against the reference…", min_count, n)
            return devkeys.dump_join(eng, ref_eng, min_count, None, 0, 0, device)

        cand, lo, hi, dump_start = _count_and_dump_child(child_bam, ref_fasta, kmer_size, min_child_count, threads, jf_hash_size, dump)
    finally:
        if ref_eng is not None:
            ref_eng.close()
    n_candidates, n_non_ref = seen["candidates"], len(lo)
    store_kmer_set(child_non_ref_fa, kmer_size, cand, (lo, hi))
    devkeys.register(child_non_ref_fa, *cand, kmer_size)
    logger.info("Child k-mer join complete (%s, %d candidates, FASTA: %s)", _format_elapsed(time.monotonic() - dump_start),
                n_candidates, _format_file_size(child_non_ref_fa))
    logger.info("Non-reference child k-mers after subtraction: %d", n_non_ref)
    return child_non_ref_fa, n_candidates, n_non_ref


def _count_parent_jellyfish(parent_bam, ref_fasta, kmer_fasta, kmer_size, parent_dir, threads,
                            label="Parent", n_filter_kmers=None):
    """``samtools fasta | jellyfish count -C --if kmer_fasta`` -> index path.
    The index holds every filter k-mer (count 0 when never seen)."""
    os.makedirs(parent_dir, exist_ok=True)
    jf_output = os.path.join(parent_dir, "parent.jf")
    logger.info("%s: scanning BAM (%s): %s", label, _format_file_size(parent_bam), parent_bam)
    scan_start = time.monotonic()
    try:
        lo, hi = load_kmer_set(kmer_fasta, kmer_size, device=_device())
        logger.info("  BAM stream -> MI355X count --if (k=%d, threads=%d, filter_kmers=%d)",
                    kmer_size, threads, len(lo))
        with mirror_engine(kmer_size, capacity_hint=max(len(lo), 1), device=_device()) as eng:
            eng.load_filter(lo, hi)
            _stream_bam(eng, parent_bam, ref_fasta, threads, filtered=True)
            _merge_filter_counts(eng, lo, hi)                  # (several ranks: the sum of their shards' counts)
            if jf_io.device_index():                           # opt-in: the dump stays in HBM and the records are made there
                dump = devkeys.dump_ge_counts(eng, 0, _device())
            else:
                dump = eng.export_ge(0)
        if dist_env.is_root():
            (jf_io.write_index_device if jf_io.device_index() else jf_io.write_index)(
                jf_output, kmer_size, *dump, cmdline=["count", "-m", str(kmer_size), "-C", "--if", kmer_fasta, "-o", jf_output])
        dist_env.barrier()
    except (KdfError, ValueError, OSError) as e:
        raise RuntimeError(f"jellyfish count ({label}) failed: {e}") from e
    logger.info("  %s jellyfish counting complete (%s, index: %s)", label,
                _format_elapsed(time.monotonic() - scan_start), _format_file_size(jf_output))
    return jf_output


def _query_index(jf_path, lo, hi, k, what):
    """``jellyfish query jf -s kmers.fa``: counts in input order."""
    try:
        with mirror_engine(k, capacity_hint=max(jf_io.index_records(jf_path), 1)) as eng:
            jf_io.load_index_into(eng, jf_path, expect_k=k)
            return eng.query(lo, hi)
    except (KdfError, ValueError, OSError) as e:
        raise RuntimeError(f"jellyfish query ({what}) failed: {e}") from e


def _count_parent_on_device(parent_bam, ref_fasta, dlo, dhi, kmer_size, threads, label):
    """The counting half of _count_parent_jellyfish with the filter taken from HBM; returns the engine (the
    caller queries it and closes it: no ``parent.jf`` is written only to be read back)."""
    logger.info("%s: scanning BAM (%s): %s", label, _format_file_size(parent_bam), parent_bam)
    scan_start = time.monotonic()
    n = int(dlo.shape[0])                                      # (long keys: rows of W words)
    logger.info("  BAM stream -> MI355X count --if (k=%d, threads=%d, filter_kmers=%d)", kmer_size, threads, n)
    eng = mirror_engine(kmer_size, capacity_hint=max(n, 1), device=_device())
    try:
        eng.load_filter_dev(dlo.data_ptr(), dhi.data_ptr() if dhi is not None else None, n)
        _stream_bam(eng, parent_bam, ref_fasta, threads, filtered=True)
        _merge_filter_counts(eng, None, None, dlo, dhi)        # (several ranks: one all-reduce of the per-key counts)
    except Exception:
        eng.close()
        raise
    logger.info("  %s jellyfish counting complete (%s)", label, _format_elapsed(time.monotonic() - scan_start))
    return eng


def _filter_parents_discovery(mother_bam, father_bam, ref_fasta, child_non_ref_fa, kmer_size, threads, tmpdir,
                              parent_max_count=0):
    """Module 2: mother then father (on the survivors), keep
    ``count <= parent_max_count``.  Returns (n_proband_unique, path | None).

    The key set stays in HBM from stage to stage: it is the parent's ``--if`` filter (kdf_load_filter_dev), the
    engine that counted the parent answers the ``jellyfish query`` directly (kdf_query_dev), and the survivors
    are a device-side mask.  ``after_mother.fa`` and ``proband_unique.fa`` are written as the reference writes them."""
    try:
        dev = devkeys.lookup(child_non_ref_fa, kmer_size)
        if dev is None and device_fasta():
            dev = read_kmer_fasta_keys_device(child_non_ref_fa, kmer_size, device=_device())
        elif dev is None:
            lo, hi = load_kmer_set(child_non_ref_fa, kmer_size)
            if len(lo) == 0:
                return 0, None
            dev = devkeys.from_host(lo, hi, kmer_size > 32)
    except (KdfError, ValueError, OSError) as e:
        raise RuntimeError(f"jellyfish count (Mother) failed: {e}") from e
    dlo, dhi = dev
    devkeys.forget(child_non_ref_fa)                             # taken: the registry must not pin GBs of HBM for the life of the process
    n_input = int(dlo.shape[0])
    if n_input == 0:
        return 0, None
    logger.info("Filtering %d non-reference k-mers against parents…", n_input)

    global LAST_PARENT_FILTER
    device_join = os.environ.get("KDF_DEVICE_JOIN") == "1" and dist_env.world_rank()[0] == 1
    LAST_PARENT_FILTER = "join" if device_join else "query"

    def one_parent(bam, label, dlo, dhi):
        os.makedirs(os.path.join(tmpdir, label.lower()), exist_ok=True)
        try:
            eng = _count_parent_on_device(bam, ref_fasta, dlo, dhi, kmer_size, threads, label)
            try:
                if device_join:
                    # `dump -U parent_max_count` of the parent's table: it holds exactly the filter keys (never-seen ones with
                    # count 0), so the join without a second table is the survivors -- in ASCENDING key order, which is the
                    # input's order whenever the input is a stage's sorted dump; an input in another order (Module 1 in key
                    # slices, a FASTA written elsewhere) keeps its order only on the default path
                    return devkeys.select([devkeys.dump_join(eng, None, 0, parent_max_count, device=eng.device)])
                keep = devkeys.query(eng, dlo, dhi, eng.device) <= parent_max_count
            finally:
                eng.close()
        except (KdfError, ValueError, OSError) as e:
            raise RuntimeError(f"jellyfish count ({label}) failed: {e}") from e
        return devkeys.select([(dlo, dhi)], keep)

    dlo, dhi = one_parent(mother_bam, "Mother", dlo, dhi)
    after_mother_fa = os.path.join(tmpdir, "after_mother.fa")
    n_surviving = int(dlo.shape[0])
    if dist_env.is_root():                                         # (the contract files are written once; every rank holds the same sets)
        store_kmer_set(after_mother_fa, kmer_size, (dlo, dhi))
    logger.info("Mother: %d / %d non-ref k-mers found (count > %d), %d surviving",
                n_input - n_surviving, n_input, parent_max_count, n_surviving)
    if n_surviving == 0:
        return 0, None

    dlo, dhi = one_parent(father_bam, "Father", dlo, dhi)
    proband_unique_fa = os.path.join(tmpdir, "proband_unique.fa")
    n_proband = int(dlo.shape[0])
    if dist_env.is_root():
        store_kmer_set(proband_unique_fa, kmer_size, (dlo, dhi))
        remove_with_sidecar(after_mother_fa)
    dist_env.barrier()
    logger.info("Father: %d / %d surviving k-mers found (count > %d), %d proband-unique",
                n_surviving - n_proband, n_surviving, parent_max_count, n_proband)
    logger.info("Proband-unique k-mers (absent from both parents): %d / %d", n_proband, n_input)
    logger.info("Proband-unique FASTA: %s (%s)", proband_unique_fa, _format_file_size(proband_unique_fa))
    return n_proband, proband_unique_fa


def _write_informative_reads_discovery(child_bam, ref_fasta, proband_unique_kmers_or_path, kmer_size, output_bam,
                                       threads=4):
    """Child records carrying a proband-unique k-mer -> sorted, indexed BAM with
    ``dk:i:1`` on every record (reference :1979-2079).  Same selection: secondary
    and duplicate records skipped, unmapped and low-MAPQ ones kept, first record
    per (query name, is_supplementary).  The probe is the engine's scan kernel
    (the reference dispatches to ``jellyfish query`` or an Aho-Corasick automaton
    on the same three input kinds); the copy, sort and index are
    ``kdf_bam_write_subset`` instead of pysam / ``samtools sort`` / ``samtools index``.
    Returns the number of records written."""
    refuse_fastq(child_bam, "the informative-reads BAM of discovery mode")
    from ..core import bam_scanner
    from ..reads import bam_reader, write_bam_subset
    bam_scanner._init_scan_worker(proband_unique_kmers_or_path or set(), kmer_size)
    eng = bam_scanner._worker_engine
    ordinals, written = [], set()
    try:
        with bam_reader(child_bam, flag_off=bam_scanner.FLAG_OFF_MODULE3, collapse=False,
                        max_bases=bam_scanner.SCAN_BATCH_BASES, max_reads=1 << 20, threads=threads,
                        want_meta=True) as rd:
            for batch in rd:
                distinct, _hits_of = bam_scanner._scan_batch(eng, batch)      # (KDF_DEVICE_HITS=1: reduced on the device)
                for r in np.flatnonzero(distinct >= 1).tolist():
                    key = (batch.name(r), bool(int(batch.flags[r]) & 0x800))
                    if key not in written:
                        written.add(key)
                        ordinals.append(int(batch.ordinals[r]))
        n = write_bam_subset(child_bam, output_bam, ordinals, [b"dkC\x01"] * len(ordinals), sort_and_index=True,
                             threads=threads)
    except KdfError as e:
        raise RuntimeError(f"informative reads BAM failed: {e}") from e
    logger.info("Informative reads BAM written: %s (%d reads)", output_bam, n)
    return n


def _write_informative_reads_fastq(child_fastq, proband_unique_kmers, kmer_size, out_prefix, min_distinct_kmers_per_read=1,
                                   paired=None):
    """The alignment-free end of the chain for a child given as FASTQ: the records that carry at least
    ``min_distinct_kmers_per_read`` distinct proband-unique k-mers, written as FASTQ text, byte for byte
    (``reads.informative_fastq``: selection and extraction on the device).  ``child_fastq``: one path, a comma-separated
    list or a sequence of paths whose names say FASTQ -- anything else is refused by name.  ``proband_unique_kmers``: what
    the Module 3 paths take (a set of k-mers, a k-mer FASTA or an index), loaded into an engine the same way, at k <= 63 and
    odd k 65 .. 201.  ``paired``: as in ``informative_fastq`` (``None``: two files are a pair).  Writes
    ``{out_prefix}.fastq``, or ``{out_prefix}.R1.fastq`` / ``{out_prefix}.R2.fastq`` for a pair (several unpaired files:
    ``{out_prefix}.{i}.fastq``).  Returns the number of records written per file."""
    from .. import reads
    from ..core import bam_scanner
    files = reads.fastq_paths(child_fastq) if child_fastq is not None else []
    if not files or not reads.is_fastq_path(files):
        raise ValueError(f"the informative reads of a FASTQ child need FASTQ files (.fastq / .fq / .fastq.gz / .fq.gz): {child_fastq} is not")
    pair = len(files) == 2 if paired is None else bool(paired)
    if pair and len(files) != 2:
        raise ValueError(f"the informative reads of a FASTQ pair need two files (R1, R2): {child_fastq} names {len(files)}")
    if pair:
        outs = [f"{out_prefix}.R1.fastq", f"{out_prefix}.R2.fastq"]
    elif len(files) == 1:
        outs = [f"{out_prefix}.fastq"]
    else:
        outs = [f"{out_prefix}.{i + 1}.fastq" for i in range(len(files))]
    bam_scanner._init_scan_worker(proband_unique_kmers or set(), kmer_size)
    eng = bam_scanner._worker_engine
    try:
        res = reads.informative_fastq(eng, files, outs, min_distinct=min_distinct_kmers_per_read, paired=paired, min_qual=reads.fastq_min_qual())
    except KdfError as e:
        if isinstance(e, reads._native.FastqFormatError):
            raise
        raise RuntimeError(f"informative reads FASTQ failed: {e}") from e
    kept = [r["kept"] for r in res]
    logger.info("Informative reads FASTQ written: %s (%s of %s records)", ", ".join(outs), kept, [r["records"] for r in res])
    return kept
