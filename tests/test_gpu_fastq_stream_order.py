"""The stream-order contract of the device FASTQ feeder with device memory (include/kdf.h "device FASTQ feeder"), observed
with ``tests/stream_order.py`` in the way of the ``fasta_pack_dev`` case of ``tests/test_gpu_stream_order.py``: a decoy text
in the buffer, the true text produced on the caller's stream behind a measured delay, no host synchronisation before the
call, the decoy put back right after it.

``kdf_fastq_pack`` carries a ``mem`` argument instead of a ``_dev`` twin, so the table of that file does not list it; this
file is its table, as ``tests/test_gpu_index_codec_stream_order.py`` is the index codec's.  The call synchronises: the
caller learns the sizes and a possible error."""
import numpy as np
import pytest

import fastq_stream_model as M
import spool_model as SM
import test_gpu_stream_order as T
from stream_order import SYNCS
from test_gpu_stream_order import H, caller_streams, delay, report  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _text(lengths, seed):
    reads = M.reads_of(lengths, seed)
    return M.fq(reads, header=lambda i: b"@r%05d" % i), reads


@pytest.mark.parametrize("min_qual", (0, 50))
def test_fastq_pack_synchronises(H, min_qual):
    from kmer_denovo_filter_amd import _native
    lengths = np.random.default_rng(25).integers(100, 2000, 200).tolist()
    (text, _), (dtext, _) = _text(lengths, 1), _text(lengths[::-1], 2)
    assert len(text) == len(dtext) and text != dtext
    codes, offs = M.pack_file(text, min_qual)
    dcodes, doffs = M.pack_file(dtext, min_qual)
    assert not np.array_equal(codes, dcodes) and not np.array_equal(offs, doffs)
    n, nr = len(codes), len(offs) - 1
    cap_bases, cap_reads = len(text) // 2, len(text) // 4
    pw, mw = SM.stream_words(cap_bases)
    with T.engine(H, 31) as e:
        def call(p):
            return e.fastq_pack_dev(p["text"], len(text), True, _native.FastqState(), p["packed"], p["invalid"], cap_bases, p["offsets"], cap_reads, min_qual)

        def observe(run):
            assert run.ret == (n, nr, len(text))
            return M.from_words(run.read("packed", np.uint64), run.read("invalid", np.uint64), n), run.read("offsets", np.int64, nr + 1)
        T.both(H, [e], f"fastq_pack min_qual={min_qual}", SYNCS, lambda: None, {"text": (np.frombuffer(text, np.uint8), np.frombuffer(dtext, np.uint8))},
               {"packed": pw * 8, "invalid": mw * 8, "offsets": (cap_reads + 1) * 8}, call, observe, (np.asarray(codes, np.uint8), np.asarray(offs, np.int64)))
