"""The feeders that fill a spool with reads: ``stream_batches_overlapped`` with a spool whose ``keep_reads`` is set, and
``scan_bam_for_hits(spool=)``.  What arrives in the spool -- offsets, read numbering, ordinals -- is held against a
second pass over the same BAM with the same reader settings, batch by batch."""
import os

import numpy as np
import pytest

from conftest import GIAB

pytestmark = pytest.mark.gpu

BAM = os.path.join(GIAB, "HG002_child.bam")
BATCH = 1 << 15                                                     # several batches out of the small golden BAM
ERR_STATE = 6


def _engine(k=31, hint=1 << 18):
    from kmer_denovo_filter_amd import KmerEngine
    return KmerEngine(k, capacity_hint=hint)


def _spool(hbm=1 << 30, host=0, segment_positions=1 << 16):
    from kmer_denovo_filter_amd.spool import ReadSpool
    sp = ReadSpool(0, hbm, host)
    sp.set_option("segment_positions", segment_positions)
    return sp


def _batches(flag_off, collapse, want_meta=False):
    from kmer_denovo_filter_amd.reads import bam_reader
    with bam_reader(BAM, flag_off=flag_off, collapse=collapse, max_bases=BATCH, max_reads=1 << 20, want_meta=want_meta) as rd:
        return list(rd)


def test_count_feeder_hands_the_offsets_on():
    from kmer_denovo_filter_amd.reads import FLAG_OFF_SAMTOOLS_FASTA, bam_reader, stream_batches_overlapped
    batches = _batches(FLAG_OFF_SAMTOOLS_FASTA, True)
    assert len(batches) >= 4
    with _spool() as sp, _spool() as plain, _engine() as eng, _engine() as ref:
        sp.keep_reads = True
        with bam_reader(BAM, max_bases=BATCH, max_reads=1 << 20) as rd:
            n = stream_batches_overlapped(eng, rd, filtered=False, spool=sp)
        with bam_reader(BAM, max_bases=BATCH, max_reads=1 << 20) as rd:
            assert stream_batches_overlapped(ref, rd, filtered=False, spool=plain) == n      # keep_reads off: as before
        assert n == sum(b.n_reads for b in batches) == sp.n_reads > 0
        assert sp.stat("keeps_reads") == 1 and plain.stat("keeps_reads") == 0 and plain.stat("offset_bytes") == 0
        assert sp.stat("batches") == plain.stat("batches") == len(batches) and sp.stat("segments") >= 2
        for i in range(sp.stat("segments")):
            for x, y in zip(sp.read_segment(i), plain.read_segment(i)):
                np.testing.assert_array_equal(x, y)
        assert eng.stats() == ref.stats()
        # the rows of the replay are those of the reader's batches, one by one
        np.testing.assert_array_equal(sp.read_hits(eng), np.concatenate([eng.read_hits(b) for b in batches]))
        depth = sp.read_depth(eng)
        np.testing.assert_array_equal(depth, np.concatenate([eng.read_depth(b) for b in batches]))
        assert int(depth[:, 0].sum()) == eng.stats()[2]             # every counted window belongs to one read
        assert sp.ordinals is None                                  # the count feeder reads no metadata


def test_scan_bam_for_hits_spools_what_it_scans():
    from kmer_denovo_filter_amd.core.bam_scanner import scan_bam_for_hits
    from kmer_denovo_filter_amd.reads import FLAG_OFF_MODULE3
    batches = _batches(FLAG_OFF_MODULE3, False, want_meta=True)
    assert len(batches) >= 4
    with _engine() as a, _engine() as b, _spool() as sp:
        a.count(batches[0])                                         # two k-mer sets: the first batch's, the last one's
        b.count(batches[-1])
        out = list(scan_bam_for_hits(BAM, a, 2, batch_bases=BATCH, spool=sp))
        again = list(scan_bam_for_hits(BAM, a, 2, batch_bases=BATCH))                      # the spool changes no result
        brief = lambda res: [(n, [(i.query_name, i.flag, i.n_distinct, i.kmer_hit_indices.tolist()) for i in infos]) for n, infos in res]
        assert brief(out) == brief(again)
        assert [n for n, _ in out] == [x.n_reads for x in batches] and sp.n_reads == sum(x.n_reads for x in batches)
        np.testing.assert_array_equal(sp.ordinals, np.concatenate([x.ordinals for x in batches]))
        # the scan's own set by replay: the reads it reported
        keep = sp.select_reads(a, 2)
        names = [x.name(r) for x in batches for r in range(x.n_reads)]
        assert [names[r] for r in keep.tolist()] == [i.query_name for _, infos in out for i in infos] and len(keep) > 0
        # the second set without a second pass over the BAM
        rows = sp.read_hits(b)
        np.testing.assert_array_equal(rows, np.concatenate([b.read_hits(x) for x in batches]))
        keep_b = sp.select_reads(b, 2)
        np.testing.assert_array_equal(keep_b, np.flatnonzero(rows[:, 1] >= 2))
        assert 0 < len(keep_b) < sp.n_reads and not np.array_equal(keep_b, keep)
        assert len(np.unique(sp.ordinals[keep_b])) == len(keep_b)


def test_scan_goes_on_when_the_spool_overflows():
    from kmer_denovo_filter_amd._native import KdfError
    from kmer_denovo_filter_amd.core.bam_scanner import scan_bam_for_hits
    from kmer_denovo_filter_amd.reads import FLAG_OFF_MODULE3
    batches = _batches(FLAG_OFF_MODULE3, False, want_meta=True)
    seg_bytes = (2 * 1024 + 4 + 1024 + 2) * 8
    with _engine() as a, _spool(2 * seg_bytes, 0) as sp:            # room for one segment and its offsets, not for two
        sp.set_option("offsets_chunk", 256)                         # (at most 2^16 / 32 entries: 16 KB beside 24 KB)
        a.count(batches[0])
        want = [(n, [i.query_name for i in infos]) for n, infos in scan_bam_for_hits(BAM, a, 2, batch_bases=BATCH)]
        got = [(n, [i.query_name for i in infos]) for n, infos in scan_bam_for_hits(BAM, a, 2, batch_bases=BATCH, spool=sp)]
        assert got == want
        assert sp.stat("overflowed") == 1 and 0 < sp.n_reads < sum(x.n_reads for x in batches)
        with pytest.raises(KdfError) as ei:
            sp.read_hits(a)
        assert ei.value.code == ERR_STATE
