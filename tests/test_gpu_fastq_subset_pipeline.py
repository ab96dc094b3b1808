"""The informative reads of a FASTQ child (``reads.informative_fastq``, ``discovery.pipeline._write_informative_reads_fastq``):
the mini trio's child written as FASTQ -- as one file, and as R1 / R2 by alternating reads -- goes through the discovery
chain's counting legs to the 630 proband-unique k-mers, and the records that carry at least ``min_distinct`` of them come
back out as text.  The truth is pure Python over the read strings: per read, the distinct canonical 31-mers that are in the
set.  ``KDF_FASTQ_FEED_MB=0.25`` forces several chunks.  The feeder rebuilt on the shared chunk walker is held to a count of
the same reads from strings."""
import os

import numpy as np
import pytest

import bamdev_cases as bc
from conftest import GIAB

pytestmark = pytest.mark.gpu

CHILD, MOTHER, FATHER = (os.path.join(GIAB, n) for n in ("HG002_child.bam", "HG004_mother.bam", "HG003_father.bam"))
K, MIN_DISTINCT = 31, 7
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def _reads_of(bam):
    """[(sequence over ACGTN, quality string)] of the BAM as the counting legs read it"""
    from kmer_denovo_filter_amd.reads import bam_reader
    out = []
    with bam_reader(bam, max_bases=1 << 24, max_reads=1 << 18, want_aux=True) as rd:
        for b in rd:
            seqs = bc.stream_reads(b)
            for i, s in enumerate(seqs):
                q = b.qualities(i)
                q = bytes((np.asarray(q, np.uint8) + 33).tolist()) if q is not None else b"I" * len(s)
                assert len(q) == len(s)
                out.append((s.encode(), q))
    return out


def _record(i, s, q):
    return b"@read%d\n%s\n+\n%s\n" % (i, s, q)


def _write_fastq(path, reads, first=0, step=1):
    with open(path, "wb") as f:
        for i, (s, q) in enumerate(reads):
            f.write(_record(first + step * i, s, q))
    return path


def _distinct_in_set(seq: bytes, kmers) -> int:
    """distinct canonical K-mers of the read that are in the set (of canonical k-mers)"""
    seen = set()
    for p in range(len(seq) - K + 1):
        w = seq[p:p + K]
        c = min(w, w.translate(_RC)[::-1])
        if c in kmers:
            seen.add(c)
    return len(seen)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the three samples as FASTQ, the chain's proband-unique k-mers, and the truth per child read"""
    from kmer_denovo_filter_amd.discovery.pipeline import _extract_child_kmers_discovery, _filter_parents_discovery, _subtract_reference_kmers
    d = tmp_path_factory.mktemp("subset_fastq")
    reads = {n: _reads_of(p) for n, p in (("child", CHILD), ("mother", MOTHER), ("father", FATHER))}
    paths = {n: _write_fastq(str(d / (n + ".fastq")), r) for n, r in reads.items()}
    old = {n: os.environ.get(n) for n in ("KDF_FASTQ_FEED_MB", "KDF_FASTQ_MIN_QUAL", "KDF_DEVICE_FEEDER")}
    os.environ["KDF_FASTQ_FEED_MB"] = "0.25"                 # several chunks per sample
    os.environ.pop("KDF_FASTQ_MIN_QUAL", None)
    os.environ.pop("KDF_DEVICE_FEEDER", None)
    try:
        tmp = str(d / "chain")
        os.makedirs(tmp)
        fa, _ = _extract_child_kmers_discovery(paths["child"], None, K, 3, 4, tmp)
        fa2, _ = _subtract_reference_kmers(os.path.join(GIAB, "mini_ref.fa.k31.jf"), fa, tmp)
        n3, fa3 = _filter_parents_discovery(paths["mother"], paths["father"], None, fa2, K, 4, tmp, 0)
        assert n3 == 630
        with open(fa3, "rb") as f:
            kmers = {ln.strip() for ln in f if ln.strip() and not ln.startswith(b">")}
        assert len(kmers) == 630 and all(len(x) == K and x == min(x, x.translate(_RC)[::-1]) for x in kmers)
        child = reads["child"]
        truth = np.array([_distinct_in_set(s, kmers) for s, _ in child], np.uint32)
        n_keep = int((truth >= MIN_DISTINCT).sum())
        assert 0 < n_keep < len(child), "the truth must keep some records and drop some"
        r1, r2 = child[0::2], child[1::2]
        if len(r1) != len(r2):                               # an odd number of reads: the pair holds all but the last
            r1 = r1[:len(r2)]
        paths["r1"] = _write_fastq(str(d / "child_R1.fastq"), r1, 0, 2)
        paths["r2"] = _write_fastq(str(d / "child_R2.fastq"), r2, 1, 2)
        yield {"dir": d, "paths": paths, "reads": reads, "kmers": kmers, "fa3": fa3, "truth": truth, "pair": (r1, r2)}
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def test_unpaired(world):
    from kmer_denovo_filter_amd import reads as R
    from kmer_denovo_filter_amd.discovery.pipeline import _write_informative_reads_fastq
    child, truth = world["reads"]["child"], world["truth"]
    keep = np.flatnonzero(truth >= MIN_DISTINCT)
    prefix = str(world["dir"] / "unpaired")
    kept = _write_informative_reads_fastq(world["paths"]["child"], world["fa3"], K, prefix, MIN_DISTINCT)
    assert kept == [len(keep)]
    with open(prefix + ".fastq", "rb") as f:
        assert f.read() == b"".join(_record(i, *child[i]) for i in keep.tolist())
    info = R.LAST_FASTQ_SUBSET
    assert info["files"] == 1 and not info["paired"] and info["passes"] == 1 and info["chunks"] > 1
    assert info["bytes_read"] == os.path.getsize(world["paths"]["child"]) and info["bytes_written"] == os.path.getsize(prefix + ".fastq")
    assert (info["records"], info["kept"]) == (len(child), len(keep))
    # the results of the file layer itself, with a set of strings as the candidate k-mers
    from kmer_denovo_filter_amd.core import bam_scanner
    bam_scanner._init_scan_worker({x.decode() for x in world["kmers"]}, K)
    out = str(world["dir"] / "direct.fastq")
    res = R.informative_fastq(bam_scanner._worker_engine, world["paths"]["child"], [out], min_distinct=MIN_DISTINCT)
    assert len(res) == 1 and res[0]["records"] == len(child) and res[0]["kept"] == len(keep)
    assert res[0]["ordinals"].dtype == np.int64 and res[0]["distinct"].dtype == np.uint32
    np.testing.assert_array_equal(res[0]["ordinals"], keep)
    np.testing.assert_array_equal(res[0]["distinct"], truth[keep])
    with open(out, "rb") as f, open(prefix + ".fastq", "rb") as g:
        assert f.read() == g.read()


def test_paired(world):
    from kmer_denovo_filter_amd import reads as R
    from kmer_denovo_filter_amd.discovery.pipeline import _write_informative_reads_fastq
    r1, r2 = world["pair"]
    n = len(r1)
    t1, t2 = world["truth"][0:2 * n:2], world["truth"][1:2 * n:2]
    either = np.flatnonzero((t1 >= MIN_DISTINCT) | (t2 >= MIN_DISTINCT))
    assert 0 < len(either) < n and ((t1 >= MIN_DISTINCT) != (t2 >= MIN_DISTINCT))[either].any(), "some pairs are kept for one mate only"
    prefix = str(world["dir"] / "paired")
    kept = _write_informative_reads_fastq(world["paths"]["r1"] + "," + world["paths"]["r2"], world["fa3"], K, prefix, MIN_DISTINCT)
    assert kept == [len(either), len(either)]
    with open(prefix + ".R1.fastq", "rb") as f:
        assert f.read() == b"".join(_record(2 * i, *r1[i]) for i in either.tolist())
    with open(prefix + ".R2.fastq", "rb") as f:
        assert f.read() == b"".join(_record(2 * i + 1, *r2[i]) for i in either.tolist())
    info = R.LAST_FASTQ_SUBSET
    assert info["paired"] and info["passes"] == 2 and info["files"] == 2 and info["kept"] == 2 * len(either) and info["records"] == 2 * n
    assert info["bytes_read"] == 2 * (os.path.getsize(world["paths"]["r1"]) + os.path.getsize(world["paths"]["r2"]))
    # the file layer's results: a mate's own value; and paired=False takes each file on its own
    from kmer_denovo_filter_amd.core import bam_scanner
    eng = bam_scanner._worker_engine
    outs = [str(world["dir"] / "p1.fastq"), str(world["dir"] / "p2.fastq")]
    res = R.informative_fastq(eng, [world["paths"]["r1"], world["paths"]["r2"]], outs, min_distinct=MIN_DISTINCT)
    for r, t in zip(res, (t1, t2)):
        assert r["records"] == n and r["kept"] == len(either)
        np.testing.assert_array_equal(r["ordinals"], either)
        np.testing.assert_array_equal(r["distinct"], t[either])
    res = R.informative_fastq(eng, [world["paths"]["r1"], world["paths"]["r2"]], outs, min_distinct=MIN_DISTINCT, paired=False)
    for r, t in zip(res, (t1, t2)):
        np.testing.assert_array_equal(r["ordinals"], np.flatnonzero(t >= MIN_DISTINCT))
    assert R.LAST_FASTQ_SUBSET["passes"] == 1 and not R.LAST_FASTQ_SUBSET["paired"]


def test_refusals(world):
    from kmer_denovo_filter_amd import dist_env
    from kmer_denovo_filter_amd import reads as R
    from kmer_denovo_filter_amd.core import bam_scanner
    from kmer_denovo_filter_amd.discovery.pipeline import _write_informative_reads_fastq
    bam_scanner._init_scan_worker({x.decode() for x in world["kmers"]}, K)
    eng = bam_scanner._worker_engine
    d, paths = world["dir"], world["paths"]
    n_child, n_r2 = len(world["reads"]["child"]), len(world["pair"][1])
    with pytest.raises(ValueError, match=rf"{n_child} records.*{n_r2}"):                 # unequal record counts, both named
        R.informative_fastq(eng, [paths["child"], paths["r2"]], [str(d / "u1.fastq"), str(d / "u2.fastq")], min_distinct=MIN_DISTINCT)
    assert not os.path.exists(str(d / "u1.fastq")) and not os.path.exists(str(d / "u2.fastq")), "a refused pair leaves no output behind"
    with pytest.raises(ValueError, match="need two files"):
        _write_informative_reads_fastq(paths["child"], world["fa3"], K, str(d / "x"), paired=True)
    with pytest.raises(ValueError, match=r"\.gz"):
        R.informative_fastq(eng, paths["child"], [str(d / "out.fastq.gz")])
    with pytest.raises(ValueError, match="one output per input"):
        R.informative_fastq(eng, [paths["r1"], paths["r2"]], [str(d / "only.fastq")])
    with pytest.raises(ValueError, match="child.bam is not"):
        _write_informative_reads_fastq(CHILD, world["fa3"], K, str(d / "x"))
    bad = str(d / "bad.fastq")
    with open(paths["child"], "rb") as f:
        text = f.read()
    cut = text.index(b"\n+\n", len(text) // 2)
    with open(bad, "wb") as f:
        f.write(text[:cut + 1] + b"-" + text[cut + 2:])
    with pytest.raises(R._native.FastqFormatError) as ei:
        R.informative_fastq(eng, bad, [str(d / "bad_out.fastq")])
    assert ei.value.rule == R._native.KDF_FQ_BAD_PLUS and ei.value.offset == text.rindex(b"\n@read", 0, cut) + 1 and bad in str(ei.value)
    orig = dist_env.world_rank
    dist_env.world_rank = lambda: (2, 0, False)
    try:
        with pytest.raises(ValueError, match="not sharded"):
            R.informative_fastq(None, paths["child"], [str(d / "r.fastq")])
    finally:
        dist_env.world_rank = orig


def test_min_distinct_zero_reproduces_the_file(world):
    from kmer_denovo_filter_amd import reads as R
    from kmer_denovo_filter_amd.core import bam_scanner
    bam_scanner._init_scan_worker({x.decode() for x in world["kmers"]}, K)
    out = str(world["dir"] / "all.fastq")
    res = R.informative_fastq(bam_scanner._worker_engine, world["paths"]["child"], [out], min_distinct=0)
    with open(out, "rb") as f, open(world["paths"]["child"], "rb") as g:
        assert f.read() == g.read()
    n = len(world["reads"]["child"])
    assert res[0]["kept"] == res[0]["records"] == n
    np.testing.assert_array_equal(res[0]["ordinals"], np.arange(n))
    np.testing.assert_array_equal(res[0]["distinct"], world["truth"])


def test_feeder_on_the_shared_walker(world):
    """``stream_fastq_device`` rebuilt on the chunk walker: LAST_FASTQ_FEEDER and the table of a count from strings"""
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd import reads as R
    child, mother = world["reads"]["child"], world["reads"]["mother"]

    def table(e):
        lo, hi, cnt = e.export_ge(0)
        o = np.argsort(lo, kind="stable")
        return lo[o].tolist(), cnt[o].tolist()
    with KmerEngine(K, capacity_hint=1 << 20) as dev, KmerEngine(K, capacity_hint=1 << 20) as host:
        n = R.stream_fastq_device(dev, [world["paths"]["child"], world["paths"]["mother"]])
        host.count(R.ReadStream.from_strings([s for s, _ in child + mother]))
        assert n == len(child) + len(mother) and table(dev) == table(host)
        size = os.path.getsize(world["paths"]["child"]) + os.path.getsize(world["paths"]["mother"])
        info = R.LAST_FASTQ_FEEDER
        assert info == {"path": "device", "files": 2, "chunks": info["chunks"], "bytes": size, "compressed": False, "min_qual": 0, "records": n,
                        "positions": sum(len(s) + 1 for s, _ in child + mother)}
        assert info["chunks"] > 2
