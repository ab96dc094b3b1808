"""The stream-order contract of kdf_fq_extract with device memory (include/kdf.h "FASTQ record extract"), observed with
``tests/stream_order.py`` as ``tests/test_gpu_fastq_stream_order.py`` observes the feeder: decoys in the input buffers -- another
well-formed text of the same length, other flags of the same shape -- the true text and flags produced on the caller's
stream behind a measured delay, no host synchronisation before the call, the decoys put back right after it.

The call carries a ``mem`` argument instead of a ``_dev`` twin, so the table of ``tests/test_gpu_stream_order.py`` does not
list it; this file is its table.  The call synchronises: the caller learns the sizes and a possible error."""
import numpy as np
import pytest

import fastq_extract_model as X
import fastq_stream_model as M
import test_gpu_stream_order as T
from stream_order import SYNCS
from test_gpu_stream_order import H, caller_streams, delay, report  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _text(lengths, seed):
    return M.fq(M.reads_of(lengths, seed), header=lambda i: b"@r%05d" % i)


@pytest.mark.parametrize("with_offsets", (True, False))
def test_fastq_extract_synchronises(H, with_offsets):
    lengths = np.random.default_rng(26).integers(100, 2000, 200).tolist()
    text, dtext = _text(lengths, 1), _text(lengths[::-1], 2)
    assert len(text) == len(dtext) and text != dtext
    rng = np.random.default_rng(27)
    keep = (rng.random(len(lengths)) < 0.5).astype(np.uint8)
    dkeep = (1 - keep).astype(np.uint8)
    out, offs, consumed = X.extract_chunk(text, True, keep.tolist())
    assert X.extract_chunk(dtext, True, dkeep.tolist())[0] != out and 0 < len(out) < len(text)
    nr, nk, cap = len(lengths), len(offs) - 1, len(text) + 2
    with T.engine(H, 31) as e:
        def call(p):
            return e.fastq_extract_dev(p["text"], len(text), True, p["keep"], nr, p["out"], cap, p["offsets"] if with_offsets else None)

        def observe(run):
            assert run.ret == (len(out), nk, consumed)
            return run.read("out", np.uint8, len(out)), run.read("offsets", np.int64, nk + 1) if with_offsets else np.asarray(offs, np.int64)
        T.both(H, [e], f"fastq_extract offsets={with_offsets}", SYNCS, lambda: None,
               {"text": (np.frombuffer(text, np.uint8), np.frombuffer(dtext, np.uint8)), "keep": (keep, dkeep)},
               {"out": cap, "offsets": (nr + 1) * 8}, call, observe, (np.frombuffer(out, np.uint8), np.asarray(offs, np.int64)))
