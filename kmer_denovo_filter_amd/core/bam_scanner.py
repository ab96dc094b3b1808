"""Module 3 hot loop: mirror of the k-mer probing part of
``kmer_denovo_filter/core/bam_scanner.py`` (``_init_scan_worker`` :250-281,
``_scan_contig_for_hits`` JF branch :396-474).

The reference extracts every window of every read in Python, unions the k-mers
of 5000 reads and spawns one ``jellyfish query`` per batch.  Here a batch of
reads is one packed stream and ONE scan-kernel launch returns a hit bit per
window; reads are kept when their number of DISTINCT hit k-mers reaches
``min_distinct_kmers_per_read``.

What is replaced is the probe loop.  Mapping hits to reference coordinates and
SV metadata (``_process_informative_read`` :284-337, ``_collect_kmer_ref_positions``
:97-117) consumes the per-read hit positions returned here; that host
post-processing is the next scope row.
"""
from __future__ import annotations

import os
import logging
from dataclasses import dataclass, field
from typing import Iterator, List, Optional, Set, Tuple

import numpy as np

from .. import jf_io
from .._native import KDF_ERR_NOMEM, KdfError
from ..engine import KmerEngine, mirror_engine, hit_positions
from ..kmer_fasta import load_kmer_set
from ..reads import FLAG_OFF_MODULE3, bam_reader, kmers_to_keys, refuse_fastq, stream_words

logger = logging.getLogger(__name__)

# stream positions per scan launch (the reference batches 5000 reads per query,
# core/bam_scanner.py:247; batch size does not change results)
SCAN_BATCH_BASES = 1 << 26
# host threads of the BAM feeder (BGZF inflate + record parsing); the reference scans contigs in a process pool
READER_THREADS = max(1, min(8, os.cpu_count() or 1))

_worker_engine: Optional[KmerEngine] = None
_worker_kmer_size: Optional[int] = None
last_ledger = None        # the RegionLedger of the last scan_bam_module3 under KDF_DEVICE_REGIONS=1, else None
_worker_min_distinct_kmers_per_read = 1


@dataclass
class InformativeRead:
    """One scanned record that passed the distinct-k-mer threshold."""
    query_name: str
    flag: int
    ref_id: int
    pos: int
    kmer_hit_indices: np.ndarray          # query start indices of hit windows
    n_distinct: int                       # len(unique_in_read)

    @property
    def is_unmapped(self): return bool(self.flag & 0x4)
    @property
    def is_supplementary(self): return bool(self.flag & 0x800)


def _init_scan_worker(proband_data, kmer_size, min_distinct_kmers_per_read=1, device: int = 0):
    """Load the proband-unique k-mers into an HBM table.  *proband_data* is an
    index path ending in ``.jf``, a k-mer FASTA path, or an iterable of canonical
    k-mer strings -- the same dispatch as the reference (:250-281)."""
    global _worker_engine, _worker_kmer_size, _worker_min_distinct_kmers_per_read
    if _worker_engine is not None:
        _worker_engine.close()
        _worker_engine = None
    try:
        if isinstance(proband_data, str) and proband_data.endswith(".jf"):
            eng = mirror_engine(kmer_size, capacity_hint=max(jf_io.index_records(proband_data), 1), device=device)
            jf_io.load_index_into(eng, proband_data, expect_k=kmer_size)
            lo = None
        elif isinstance(proband_data, str):
            lo, hi = load_kmer_set(proband_data, kmer_size, device=device)
            cnt = np.ones(len(lo), np.uint32)
        else:
            lo, hi = kmers_to_keys(list(proband_data), kmer_size)
            cnt = np.ones(len(lo), np.uint32)
        if lo is not None:
            eng = mirror_engine(kmer_size, capacity_hint=max(len(lo), 1), device=device)
            eng.add_pairs(lo, hi, cnt)
    except (KdfError, ValueError, OSError) as e:
        raise RuntimeError(f"jellyfish query failed: {e}") from e
    _worker_engine = eng
    _worker_kmer_size = kmer_size
    _worker_min_distinct_kmers_per_read = min_distinct_kmers_per_read


def _scan_batch(eng: KmerEngine, batch):
    """One batch through the probe -> (distinct uint32[n_reads], hits_of(r) -> int64 query start indices of read r's
    hit windows).  Default: ``KmerEngine.scan`` (the mask comes back, the engine's host loop counts the distinct
    k-mers).  ``KDF_DEVICE_HITS=1``, read here at every call: ``KmerEngine.scan_hits`` -- the per-read rows and the
    compacted hit list are made on the device and only they come back.  Same values either way."""
    offs = batch.offsets
    if os.environ.get("KDF_DEVICE_HITS") == "1":
        rows, pos = eng.scan_hits(batch)

        def hits_of(r):
            s = int(offs[r])
            a, b = np.searchsorted(pos, (s, int(offs[r + 1]) - 1))
            return pos[a:b] - s
        return rows[:, 1], hits_of
    hits, distinct = eng.scan(batch)
    return distinct, lambda r: hit_positions(hits, int(offs[r]), int(offs[r + 1]) - 1)


def scan_bam_for_hits(child_bam, engine: Optional[KmerEngine] = None, min_dk_per_read: Optional[int] = None,
                      batch_bases: int = SCAN_BATCH_BASES, spool=None) -> Iterator[Tuple[int, List[InformativeRead]]]:
    """Scan every non-SECONDARY, non-DUPLICATE record (supplementary kept, no
    QNAME collapse: reference :405-409).  Yields (reads_scanned_in_batch,
    [InformativeRead ...]) per batch, records in file order.  ``spool``: a
    ``spool.ReadSpool`` that takes every scanned batch with its read offsets and
    BAM ordinals, so that another k-mer set is evaluated over the same reads by
    ``spool.read_hits`` / ``select_reads`` and not by a second pass over the BAM
    (a spool that overflows stops taking batches; ``spool.stat("overflowed")``)."""
    refuse_fastq(child_bam, "scan_bam_for_hits (the Module 3 scan)")
    eng = engine or _worker_engine
    if eng is None:
        raise RuntimeError("scan worker not initialised (_init_scan_worker)")
    min_dk = _worker_min_distinct_kmers_per_read if min_dk_per_read is None else min_dk_per_read
    with bam_reader(child_bam, flag_off=FLAG_OFF_MODULE3, collapse=False, max_bases=batch_bases,
                    max_reads=1 << 20, threads=READER_THREADS, want_meta=True) as rd:
        for batch in rd:
            if spool is not None and not spool.stat("overflowed"):
                try:
                    spool.append(batch, keep_reads=True)
                except KdfError as e:                           # neither budget holds the next segment: the scan goes on
                    if e.code != KDF_ERR_NOMEM:
                        raise                                   # (the spool's own error, not a failed query)
                    logger.info("Read spool overflowed after %d reads: %s", spool.n_reads, e)
            try:
                distinct, hits_of = _scan_batch(eng, batch)
            except KdfError as e:
                raise RuntimeError(f"jellyfish query failed: {e}") from e
            out = []
            for r in np.flatnonzero(distinct >= max(min_dk, 1)).tolist():
                out.append(InformativeRead(batch.name(r), int(batch.flags[r]), int(batch.ref_ids[r]),
                                           int(batch.positions[r]), hits_of(r),
                                           int(distinct[r])))
            if min_dk <= 0:
                # reference: `len(unique_in_read) < min_dk_per_read` never true for 0 -> every read kept
                keep = set(np.flatnonzero(distinct == 0).tolist())
                for r in sorted(keep):
                    out.append(InformativeRead(batch.name(r), int(batch.flags[r]), int(batch.ref_ids[r]),
                                               int(batch.positions[r]), np.zeros(0, np.int64), 0))
            yield batch.n_reads, out


def count_informative_reads(child_bam, engine: Optional[KmerEngine] = None,
                            min_dk_per_read: Optional[int] = None):
    """(total_informative, unmapped_informative, total_reads_scanned, informative records)
    with the reference's de-duplication: one task per contig plus one for
    unplaced reads, records de-duplicated by (query_name, is_supplementary)
    inside a task (core/bam_scanner.py:293-299) and again when tasks are merged
    (discovery/pipeline.py:840-846); unmapped informative reads are counted per
    task."""
    tasks = {}
    scanned = 0
    order = []
    for n, infos in scan_bam_for_hits(child_bam, engine, min_dk_per_read):
        scanned += n
        for inf in infos:
            if inf.ref_id not in tasks:
                tasks[inf.ref_id] = []
                order.append(inf.ref_id)
            tasks[inf.ref_id].append(inf)
    seen_global: Set[Tuple[str, bool]] = set()
    kept: List[InformativeRead] = []
    unmapped = 0
    for ref_id in sorted(t for t in order if t >= 0) + ([-1] if -1 in tasks else []):
        seen_local: Set[Tuple[str, bool]] = set()
        for inf in tasks[ref_id]:
            key = (inf.query_name, inf.is_supplementary)
            if key in seen_local:
                continue
            seen_local.add(key)
            if inf.is_unmapped:
                unmapped += 1
                continue
            if key in seen_global:
                continue
            kept.append(inf)
        seen_global |= seen_local
    return len(kept) + unmapped, unmapped, scanned, kept


# ---------------------------------------------------------------------------
# N1: hits -> reference coordinates, per-read SV metadata (host post-processing
# of the scan kernel's output; reference :54-117, :284-337, :340-392)
# ---------------------------------------------------------------------------

_REF_CONSUMING = (0, 2, 3, 7, 8)     # M D N = X
_ALIGNED = (0, 7, 8)                 # M = X  (pysam get_aligned_pairs(matches_only=True))
_QUERY_CONSUMING = (0, 1, 4, 7, 8)   # M I S = X


def _extract_softclips(cigartuples):
    """(left, right) soft-clip lengths; hard clips outside them are skipped and a
    read that is one single soft clip counts on the left only (reference :54-94)."""
    if not cigartuples:
        return (0, 0)
    core = [(op, ln) for op, ln in cigartuples if op != 5]
    if not core:
        return (0, 0)
    left = core[0][1] if core[0][0] == 4 else 0
    right = core[-1][1] if core[-1][0] == 4 else 0
    if len(core) == 1 and core[0][0] == 4:
        right = 0
    return (left, right)


def reference_end(pos, cigartuples):
    """pysam's ``reference_end``: pos + reference bases consumed."""
    return pos + sum(ln for op, ln in cigartuples if op in _REF_CONSUMING)


def _query_to_ref(pos, cigartuples, query_len):
    """int64[query_len]: reference position aligned to each query base, -1 when
    the base is inserted / clipped (only M, = and X pair bases up)."""
    q2r = np.full(query_len, -1, dtype=np.int64)
    q, r = 0, pos
    for op, ln in cigartuples:
        if op in _ALIGNED:
            q2r[q:q + ln] = np.arange(r, r + ln)
            q += ln
            r += ln
        elif op in (1, 4):
            q += ln
        elif op in (2, 3):
            r += ln
    return q2r


def _collect_kmer_ref_positions(pos, cigartuples, query_len, kmer_hit_indices, kmer_size):
    """Counter {reference position: number of hit k-mers covering it} for one
    read (reference :97-117)."""
    import collections
    cov = collections.Counter()
    if len(kmer_hit_indices) == 0:
        return cov
    q2r = _query_to_ref(pos, cigartuples, query_len)
    qpos = (np.asarray(kmer_hit_indices, dtype=np.int64)[:, None] + np.arange(kmer_size)[None, :]).ravel()
    qpos = qpos[qpos < query_len]
    rpos = q2r[qpos]
    rpos = rpos[rpos >= 0]
    if len(rpos):
        u, c = np.unique(rpos, return_counts=True)
        cov.update(dict(zip(u.tolist(), c.tolist())))
    return cov


def _decode_read(batch, r):
    """Upper-case bases of record r of a batch (N for invalid positions)."""
    s, e = int(batch.offsets[r]), int(batch.offsets[r + 1]) - 1
    idx = np.arange(s, e)
    codes = (batch.packed[idx >> 5] >> ((idx & 31) * 2).astype(np.uint64)) & np.uint64(3)
    inv = (batch.invalid[idx >> 6] >> (idx & 63).astype(np.uint64)) & np.uint64(1)
    chars = np.frombuffer(b"ACGT", np.uint8)[codes.astype(np.intp)].copy()
    chars[inv.astype(bool)] = ord("N")
    return chars.tobytes().decode()


class RegionLedger:
    """``KDF_DEVICE_REGIONS=1``: what Module 3 keeps in HBM for the regions' k-mer counts -- for every hit of every KEPT
    read its key row (``keys``: int64 tensors of ``hits x words`` words, one per batch) and the running ordinal of its
    read among the kept reads (``ordinals``: int64 tensors, one per batch).  Names stay on the host: which kept reads
    reach ``read_hits`` is decided there, and ``read_hits`` carries each read's ordinal in place of its k-mer set."""

    def __init__(self, eng: KmerEngine, refs):
        self.eng, self.refs, self.words = eng, list(refs), eng.key_words
        self.keys, self.ordinals, self.n_reads = [], [], 0


class _DeviceCoverage:
    """``KDF_DEVICE_COVERAGE=1``: Module 3's two coverage sums kept on the device.  Two uint32 accumulators of the
    genome's linear length (contig offsets = running sum of the header's reference lengths); per batch the hit mask,
    the read offsets and the CIGAR arrays stay in HBM and ``hit_coverage_dev`` adds the contributing reads; the per-read
    k-mer sets come from ``hit_keys_dev`` (one ``keys_to_kmers`` per distinct key of a read, no read is decoded).  The
    host decides WHICH reads contribute, because it has the names: kept by ``min_dk``, mapped, and the first kept
    record with its (ref_id, name, is_supplementary) in file order -- the reference's de-duplication inside a contig's
    task; coverage is a commutative sum, so the order of the tasks does not matter.  With a ``ledger``
    (``KDF_DEVICE_REGIONS=1``) the key rows stay on the device too and no k-mer set is made."""

    def __init__(self, eng: KmerEngine, ref_lengths, ledger: Optional[RegionLedger] = None):
        import torch
        self.eng = eng
        self.torch = torch
        self.dev = torch.device("cuda", eng.device)
        self.contig_off = np.concatenate(([0], np.cumsum(np.asarray(ref_lengths, dtype=np.int64)))).astype(np.int64)
        self.span = int(self.contig_off[-1])
        self.kcov = torch.zeros(max(self.span, 1), dtype=torch.int32, device=self.dev)
        self.rcov = torch.zeros(max(self.span, 1), dtype=torch.int32, device=self.dev)
        self.seen = set()
        self.ledger = ledger

    @staticmethod
    def fits(eng: KmerEngine, ref_lengths) -> bool:
        """both accumulators within half of the free HBM"""
        from ctypes import byref, c_uint64
        from .. import _native
        free, total = c_uint64(0), c_uint64(0)
        _native.check(_native.load().kdf_device_memory(eng.device, byref(free), byref(total)), None)
        need = 8 * int(sum(int(x) for x in ref_lengths))
        if need > free.value // 2:
            logger.info("KDF_DEVICE_COVERAGE: two accumulators of %d bytes do not fit half of the %d free bytes of HBM; "
                        "coverage is summed on the host", need, free.value)
            return False
        return True

    def _up(self, a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        if a.nbytes % 8:                                                 # (uint32 arrays of odd length)
            a = np.concatenate((a, np.zeros(1, dt)))
        if a.nbytes == 0:
            a = np.zeros(1, np.int64)
        return self.torch.from_numpy(a.view(np.int64)).to(self.dev)

    def batch(self, batch, min_dk: int, k: int):
        """-> (keep int64[m], hit offsets of each kept read relative to its start, k-mer set of each kept read); the
        contributing reads among them are added to the accumulators.  With a ledger the third list holds each kept
        read's ordinal instead, and the key rows of the kept reads' hits join the ledger."""
        from ..reads import keys_to_kmers
        eng, torch = self.eng, self.torch
        n, nr = int(batch.n_bases), int(batch.n_reads)
        offs = np.asarray(batch.offsets, dtype=np.int64)
        pw, mw = stream_words(n)
        dp, dm, do = self._up(batch.packed[:pw], np.uint64), self._up(batch.invalid[:mw], np.uint64), self._up(offs, np.int64)
        dbits = torch.empty((n + 63) // 64, dtype=torch.int64, device=self.dev)
        drows = torch.empty(nr, dtype=torch.int64, device=self.dev)          # one row = 2 x uint32
        torch.cuda.synchronize(self.dev)
        eng.read_hits_dev(dp.data_ptr(), dm.data_ptr(), n, do.data_ptr(), nr, dbits.data_ptr(), drows.data_ptr())
        eng.synchronize()
        rows = drows.cpu().numpy().view(np.uint32).reshape(nr, 2)
        keep = np.flatnonzero(rows[:, 1] >= min_dk) if min_dk > 0 else np.arange(nr)
        # the hit list and the key of every hit: the list stays on the device for hit_keys_dev
        cap = int(rows[:, 0].sum(dtype=np.int64))
        while True:
            dpos = torch.empty(max(cap, 1), dtype=torch.int64, device=self.dev)
            dreads = torch.empty(max(cap, 1), dtype=torch.int64, device=self.dev) if self.ledger is not None else None   # each hit's read
            torch.cuda.synchronize(self.dev)
            if dreads is None:
                rc, got = eng._hit_list_dev(dbits.data_ptr(), n, None, 0, dpos.data_ptr(), None, cap)
            else:
                rc, got = eng._hit_list_dev(dbits.data_ptr(), n, do.data_ptr(), nr, dpos.data_ptr(), dreads.data_ptr(), cap)
            if got <= cap:
                eng._ck(rc)
                break
            cap = got
        W = eng.key_words
        dkeys = torch.empty(max(got, 1) * W, dtype=torch.int64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        eng.hit_keys_dev(dp.data_ptr(), n, dpos.data_ptr(), got, dkeys.data_ptr())
        eng.synchronize()
        pos = dpos[:got].cpu().numpy()
        lo = np.searchsorted(pos, offs[keep], side="left")
        hi = np.searchsorted(pos, offs[keep + 1] - 1, side="left") if len(keep) else lo
        hit_idx, kmers = [], []
        led = self.ledger
        if led is not None:
            # every hit's read -> that read's ordinal among the kept reads (-1: not kept); the kept hits' rows stay in HBM
            ordinal = np.full(nr + 1, -1, np.int64)                       # (the last entry serves a hit outside every read)
            ordinal[keep] = led.n_reads + np.arange(len(keep))
            hit_ord = torch.from_numpy(ordinal).to(self.dev)[dreads[:got]]
            sel = hit_ord >= 0
            led.keys.append(dkeys[:got * W].view(got, W)[sel].reshape(-1))
            led.ordinals.append(hit_ord[sel])
            torch.cuda.synchronize(self.dev)
            kmers = (led.n_reads + np.arange(len(keep))).tolist()
            led.n_reads += len(keep)
        key_rows = dkeys[:got * W].cpu().numpy().view(np.uint64).reshape(got, W) if led is None else None
        for a, b, s in zip(lo.tolist(), hi.tolist(), offs[keep].tolist()):
            hit_idx.append(pos[a:b] - s)
            if led is not None:
                continue
            if a == b:
                kmers.append(set())
                continue
            u = np.unique(key_rows[a:b], axis=0)
            kmers.append(set(keys_to_kmers(u if W > 2 else np.ascontiguousarray(u[:, 0]),
                                           np.ascontiguousarray(u[:, 1]) if W == 2 else None, k)))
        # which reads contribute
        ref_start = np.full(nr, -1, np.int64)
        for r in keep.tolist():
            flag, ref_id = int(batch.flags[r]), int(batch.ref_ids[r])
            key = (ref_id, batch.name(r), bool(flag & 0x800))
            if key in self.seen:
                continue
            self.seen.add(key)
            if flag & 0x4 or ref_id < 0 or ref_id + 1 >= len(self.contig_off):
                continue
            ref_start[r] = int(self.contig_off[ref_id]) + int(batch.positions[r])
        if (ref_start >= 0).any() and self.span:
            drs, dcg, dco = self._up(ref_start, np.int64), self._up(batch.cigar, np.uint32), self._up(batch.cigar_offsets, np.int64)
            torch.cuda.synchronize(self.dev)
            eng.hit_coverage_dev(dbits.data_ptr(), n, do.data_ptr(), nr, drs.data_ptr(), dcg.data_ptr(), len(batch.cigar),
                                 dco.data_ptr(), self.kcov.data_ptr(), self.rcov.data_ptr(), self.span)
            eng.synchronize()
        return keep, hit_idx, kmers

    def counters(self, refs):
        """the ascending list of covered positions -> ({chrom: Counter position -> hit k-mers}, {chrom: Counter
        position -> reads}) in contig coordinates"""
        import collections
        eng, torch = self.eng, self.torch
        kc, rc = collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
        if not self.span:
            return kc, rc
        torch.cuda.synchronize(self.dev)
        _, m = eng._coverage_list_dev(self.kcov.data_ptr(), self.rcov.data_ptr(), 0, self.span, 1, None, None, None, 0)
        if m == 0:
            return kc, rc
        dpos = torch.empty(m, dtype=torch.int64, device=self.dev)
        dk = torch.empty(m, dtype=torch.int32, device=self.dev)
        dr = torch.empty(m, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)
        eng.coverage_list_dev(self.kcov.data_ptr(), self.rcov.data_ptr(), 0, self.span, 1, dpos.data_ptr(), dk.data_ptr(),
                              dr.data_ptr(), m)
        g = dpos.cpu().numpy()
        kv, rv = dk.cpu().numpy().view(np.uint32), dr.cpu().numpy().view(np.uint32)
        ci = np.searchsorted(self.contig_off, g, side="right") - 1
        for c in np.unique(ci).tolist():
            sel = ci == c
            p = (g[sel] - self.contig_off[c]).tolist()
            kc[refs[c]].update(dict(zip(p, kv[sel].tolist())))
            rc[refs[c]].update(dict(zip(p, rv[sel].tolist())))
        return kc, rc


def scan_bam_module3(child_bam, kmer_size=None, min_dk_per_read=None, engine=None,
                     batch_bases: int = SCAN_BATCH_BASES):
    """Module 3 over a whole BAM with the reference's task structure: one task per
    contig (records whose ref_id is that contig, unmapped mates included) plus one
    for unplaced reads, each de-duplicating by (query_name, is_supplementary);
    task results merged in contig order (core/bam_scanner.py:340-507,
    discovery/pipeline.py:733-860).

    Returns the reference's tuple
      (read_hits, reads_seen, unmapped_informative, total_reads_scanned,
       read_sv_meta, kmer_coverage, read_coverage)
    with read_hits = [(ref_name, ref_start, ref_end, query_name, unique_in_read, is_supplementary)].

    ``KDF_DEVICE_COVERAGE=1``: the two coverage sums and the per-read k-mer sets are made on the device
    (``_DeviceCoverage``); the tuple is the same.

    ``KDF_DEVICE_REGIONS=1`` (implies the former): no per-read k-mer set is made.  The key rows of the kept reads' hits
    stay in HBM in ``last_ledger`` (``RegionLedger``), and ``unique_in_read`` of a ``read_hits`` entry is the read's
    ordinal in that ledger; ``discovery.regions._cluster_read_hits_device`` counts the regions' k-mers from it.
    """
    refuse_fastq(child_bam, "scan_bam_module3 (Module 3)")
    import collections
    from ..kmer_utils import canonicalize
    global last_ledger
    last_ledger = None
    eng = engine or _worker_engine
    if eng is None:
        raise RuntimeError("scan worker not initialised (_init_scan_worker)")
    k = kmer_size or _worker_kmer_size or eng.k
    min_dk = _worker_min_distinct_kmers_per_read if min_dk_per_read is None else min_dk_per_read

    per_task = collections.OrderedDict()        # ref_id -> list of informative record dicts, file order
    total_scanned = 0
    rd = bam_reader(child_bam, flag_off=FLAG_OFF_MODULE3, collapse=False, max_bases=batch_bases,
                    max_reads=1 << 20, threads=READER_THREADS, want_aux=True)
    refs = rd.references()
    # KDF_DEVICE_COVERAGE=1, read here at every call (it implies the device hits path): the coverage sums stay in HBM
    dcov = None
    want_regions = os.environ.get("KDF_DEVICE_REGIONS") == "1"       # (read at every call, like the switch it implies)
    if want_regions or os.environ.get("KDF_DEVICE_COVERAGE") == "1":
        lengths = rd.reference_lengths()
        if _DeviceCoverage.fits(eng, lengths):
            dcov = _DeviceCoverage(eng, lengths, RegionLedger(eng, refs) if want_regions else None)
        elif want_regions:
            logger.info("KDF_DEVICE_REGIONS: without the device coverage path the regions are clustered on the host")
    with rd:
        for batch in rd:
            total_scanned += batch.n_reads
            if dcov is not None:
                try:
                    keep, hit_idx, kmers = dcov.batch(batch, min_dk, k)
                except KdfError as e:
                    raise RuntimeError(f"jellyfish query failed: {e}") from e
                for r, idx, km in zip(keep.tolist(), hit_idx, kmers):
                    rec = {
                        "name": batch.name(r), "flag": int(batch.flags[r]), "ref_id": int(batch.ref_ids[r]),
                        "pos": int(batch.positions[r]), "cigar": batch.cigartuples(r), "sa": batch.sa_tag(r),
                        "qlen": int(batch.offsets[r + 1] - batch.offsets[r]) - 1, "hit_idx": idx, "kmers": km,
                    }
                    if dcov.ledger is not None:                 # km is the read's ordinal in the ledger
                        rec["kmers"], rec["ordinal"] = None, km
                    per_task.setdefault(rec["ref_id"], []).append(rec)
                continue
            try:
                distinct, hits_of = _scan_batch(eng, batch)
            except KdfError as e:
                raise RuntimeError(f"jellyfish query failed: {e}") from e
            keep = np.flatnonzero(distinct >= min_dk) if min_dk > 0 else np.arange(batch.n_reads)
            for r in keep.tolist():
                idx = hits_of(r)
                seq = _decode_read(batch, r)
                rec = {
                    "name": batch.name(r), "flag": int(batch.flags[r]), "ref_id": int(batch.ref_ids[r]),
                    "pos": int(batch.positions[r]), "cigar": batch.cigartuples(r), "sa": batch.sa_tag(r),
                    "qlen": len(seq), "hit_idx": idx,
                    "kmers": {canonicalize(seq[p:p + k]) for p in idx.tolist()},
                }
                per_task.setdefault(rec["ref_id"], []).append(rec)

    read_hits, reads_seen, read_sv_meta = [], set(), {}
    kmer_coverage = collections.defaultdict(collections.Counter)
    read_coverage = collections.defaultdict(collections.Counter)
    unmapped_informative = 0
    order = sorted(t for t in per_task if t >= 0) + ([-1] if -1 in per_task else [])
    for ref_id in order:
        seen_local = set()
        for rec in per_task[ref_id]:
            is_supp = bool(rec["flag"] & 0x800)
            key = (rec["name"], is_supp)
            if key in seen_local:                       # _process_informative_read: already seen in this task
                continue
            seen_local.add(key)
            if rec["flag"] & 0x4:                       # unmapped: counted, no coordinates
                unmapped_informative += 1
                continue
            chrom = refs[rec["ref_id"]]
            if dcov is None:
                cov = _collect_kmer_ref_positions(rec["pos"], rec["cigar"], rec["qlen"], rec["hit_idx"], k)
                kmer_coverage[chrom].update(cov)
                for p in cov:
                    read_coverage[chrom][p] += 1
            else:
                kmer_coverage[chrom]                    # (the host path leaves an entry for every contig met here)
            paired = bool(rec["flag"] & 0x1)
            if key not in read_sv_meta:
                read_sv_meta[key] = {
                    "has_sa": rec["sa"] is not None,
                    "sa_str": rec["sa"] if (rec["sa"] is not None and not is_supp) else None,
                    "is_paired": paired,
                    "is_proper_pair": bool(rec["flag"] & 0x2),
                    "mate_is_unmapped": bool(rec["flag"] & 0x8) if paired else False,
                    "max_clip": max([ln for op, ln in rec["cigar"] if op == 4], default=0),
                }
            if key in reads_seen:                       # already reported by an earlier task
                continue
            read_hits.append((chrom, rec["pos"], reference_end(rec["pos"], rec["cigar"]), rec["name"],
                              rec["ordinal"] if "ordinal" in rec else rec["kmers"], is_supp))
        reads_seen |= seen_local
    if dcov is not None:
        try:
            kc, rc = dcov.counters(refs)
        except KdfError as e:
            raise RuntimeError(f"jellyfish query failed: {e}") from e
        for chrom, c in kc.items():
            kmer_coverage[chrom].update(c)
        for chrom, c in rc.items():
            read_coverage[chrom].update(c)
        last_ledger = dcov.ledger
    return (read_hits, reads_seen, unmapped_informative, total_scanned, read_sv_meta,
            kmer_coverage, read_coverage)
