"""The raw range planner of the device BAM feeder (kdf_bamraw_*), on the host alone: its batches, inflated with
Python's zlib and walked by a short restatement of the contract (bamdev_cases.walk), must give the reads of the host
reader -- sequence for sequence, invalid positions included, in order, for every split of the file."""
import os
import zlib

import numpy as np
import pytest

import bamdev_cases as bc
from conftest import GIAB
from kmer_denovo_filter_amd import reads as R

SAMPLES = ("HG002_child", "HG003_father", "HG004_mother")
MODES = ((R.FLAG_OFF_SAMTOOLS_FASTA, True), (R.FLAG_OFF_MODULE3, False))


def host_reads(path, flag_off, collapse, parts):
    out = []
    for p in range(parts):
        with R.bam_reader(path, flag_off, collapse, max_bases=1 << 24, max_reads=1 << 18, part=p, parts=parts) as rd:
            for st in rd:
                out += bc.stream_reads(st)
    return out


def planned_reads(path, flag_off, collapse, parts, subrange_bytes, comp_cap=1 << 24, tail_blocks=0, stats=None):
    """Every part's batches -> reads, replaying unfinished sub-ranges one at a time with a longer tail."""
    out = []
    for p in range(parts):
        with R.bam_raw_reader(path, flag_off, collapse, p, parts, subrange_bytes, comp_cap, tail_blocks) as rd:
            for b in rd:
                span = inflate_batch(b)
                for i, s in enumerate(b.subs):
                    got, done = walk_sub(span, s, flag_off, collapse)
                    tail = 8
                    while not done:                                  # replay this sub-range alone
                        if stats is not None:
                            stats["replays"] = stats.get("replays", 0) + 1
                        with R.bam_raw_reader(path, flag_off, collapse, p, parts, subrange_bytes, comp_cap) as rp:
                            rp.seek(b.first_sub + i)
                            rb = rp.next_into(np.empty(comp_cap, np.uint8), tail_blocks=tail, max_subs=1)
                            got, done = walk_sub(inflate_batch(rb), rb.subs[0], flag_off, collapse)
                        tail *= 4
                    out += got
                if stats is not None:
                    stats["batches"] = stats.get("batches", 0) + 1
                    stats["subs"] = stats.get("subs", 0) + len(b.subs)
                    stats["empty"] = stats.get("empty", 0) + int((b.subs["start"] == R.SUB_NONE).sum())
    return out


def inflate_batch(b):
    span = bytearray()
    for blk in b.blocks:
        assert int(blk["out_off"]) == len(span)
        payload = b.comp[int(blk["comp_off"]):int(blk["comp_off"]) + int(blk["comp_len"])].tobytes()
        data = zlib.decompress(payload, -15) if blk["isize"] else b""
        assert len(data) == int(blk["isize"])
        span += data
    assert len(span) == b.inflated_bytes
    return bytes(span)


def walk_sub(span, s, flag_off, collapse):
    if int(s["start"]) == R.SUB_NONE:
        return [], True
    stop = None if int(s["stop"]) == R.SUB_NONE else int(s["stop"])
    return bc.walk(span, int(s["start"]), stop, flag_off, collapse, bool(int(s["flags"]) & R.SUB_AT_EOF))


@pytest.fixture(scope="module")
def host_whole():
    return {(s, m): host_reads(os.path.join(GIAB, s + ".bam"), *m, 1) for s in SAMPLES for m in MODES}


@pytest.mark.parametrize("sample", SAMPLES)
@pytest.mark.parametrize("parts", (1, 2, 5))
@pytest.mark.parametrize("mode", MODES, ids=("collapse", "module3"))
def test_giab_batches_give_the_host_readers_reads(sample, parts, mode, host_whole):
    path = os.path.join(GIAB, sample + ".bam")
    want = host_reads(path, *mode, parts)
    assert want == host_whole[(sample, mode)]                     # (the yardstick itself: the parts are the whole file)
    stats = {}
    got = planned_reads(path, *mode, parts, os.path.getsize(path) // 12, stats=stats)
    assert stats["subs"] >= 12
    assert got == want


def test_small_batches_and_one_block_tails(host_whole):
    """A compressed buffer of a few blocks forces many batches; a tail of one block forces replays."""
    path = os.path.join(GIAB, "HG002_child.bam")
    stats = {}
    got = planned_reads(path, R.FLAG_OFF_SAMTOOLS_FASTA, True, 3, 40_000, comp_cap=150_000, tail_blocks=1, stats=stats)
    assert stats["batches"] > 6
    assert got == host_whole[("HG002_child", MODES[0])]


_synthetic = bc.synthetic_bam


@pytest.mark.parametrize("parts", (1, 2, 5))
@pytest.mark.parametrize("mode", MODES, ids=("collapse", "module3"))
def test_synthetic_bam_with_small_blocks(tmp_path, parts, mode):
    path = _synthetic(tmp_path)
    want = host_reads(path, *mode, parts)
    assert len(want) > 500
    got = planned_reads(path, *mode, parts, os.path.getsize(path) // 13)
    assert got == want


def test_subranges_smaller_than_a_run_lose_nothing(tmp_path):
    """Cuts every 300 bytes of file: most sub-ranges hold no run boundary and are empty."""
    path = _synthetic(tmp_path, n_runs=120, block=2000)
    want = host_reads(path, R.FLAG_OFF_SAMTOOLS_FASTA, True, 1)
    stats = {}
    got = planned_reads(path, R.FLAG_OFF_SAMTOOLS_FASTA, True, 2, 300, stats=stats)
    assert stats["empty"] > 0
    assert got == want


def test_bam_without_records_and_bad_arguments(tmp_path):
    path = str(tmp_path / "empty.bam")
    bc.write_bgzf(path, bc.bam_header())
    for part in (0, 1):
        with R.bam_raw_reader(path, part=part, parts=2) as rd:
            assert rd.n_subranges == 0 and list(rd) == []
    from kmer_denovo_filter_amd._native import KdfError
    with pytest.raises(KdfError):
        R.bam_raw_reader(path, part=2, parts=2)
    with pytest.raises(KdfError):
        R.bam_raw_reader(str(tmp_path / "missing.bam"))
    with R.bam_raw_reader(os.path.join(GIAB, "HG002_child.bam"), subrange_bytes=1 << 20) as rd:
        with pytest.raises(KdfError, match="does not fit"):
            rd.next_into(np.empty(50_000, np.uint8))


def test_records_longer_than_the_tail_are_replayed(tmp_path):
    """Blocks of 120 bytes: every record spans several, so a tail of one block leaves walks unfinished -- each such
    sub-range is planned again with a longer tail, and no read is lost or doubled."""
    path = _synthetic(tmp_path, n_runs=60, block=120)
    want = host_reads(path, R.FLAG_OFF_SAMTOOLS_FASTA, True, 1)
    stats = {}
    got = planned_reads(path, R.FLAG_OFF_SAMTOOLS_FASTA, True, 1, 800, comp_cap=3000, tail_blocks=1, stats=stats)
    assert stats["replays"] > 0 and stats["batches"] > 3
    assert got == want
