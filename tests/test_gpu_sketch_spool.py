"""``ReadSpool.sketch`` (kdf_spool_sketch): the sketch of a spool's segments equals the sketch of the appended batches
given to the engine one by one, over the HBM tier, the host tier (through the upload slots) and both; the refusals; and
the spool, the slots and the engine's table are as they were.  Fails without the feature (no such method)."""
import numpy as np
import pytest
import torch

import spool_model as M
from test_gpu_spool import SEG_BYTES, _cut_batches, _direct, _dump, _engine, _fill, _segments, _same_segments, _spool, _stream

pytestmark = pytest.mark.gpu

ERR_NOMEM, ERR_STATE = 3, 6
P = 12


@pytest.fixture(scope="module", params=[31, 101])
def case(request):
    """(k, batches of at most 40 000 positions: several batches per segment of 2^16, several segments)"""
    k = request.param
    small = []
    for p, m, n in _cut_batches(k, seed=5):
        codes, inv = M.unpack(p, m, n)
        for a in range(0, n, 40000):
            small.append(M.pack(codes[a:a + 40000], inv[a:a + 40000]) + (len(codes[a:a + 40000]),))
    return k, small


def _batchwise(k, batches):
    with _engine(k) as eng:
        eng.sketch_begin(P)
        for p, m, n in batches:
            eng.sketch_add(_stream(p, m, n))
        return eng.sketch_registers(), eng.get_stat("sketch_windows")


@pytest.mark.parametrize("tier", ["hbm", "host", "mixed"])
def test_spool_sketch_equals_batch_by_batch(case, tier):
    k, batches = case
    hbm, host = {"hbm": (1 << 30, 0), "host": (0, 1 << 30), "mixed": (SEG_BYTES + 100, 1 << 30)}[tier]
    want, windows = _batchwise(k, batches)
    assert int(want.max()) > 0 and windows > 0
    with _spool(hbm, host, segment_positions=1 << 16) as sp, _engine(k) as eng, _engine(k) as ref:
        _fill(sp, batches)
        assert sp.stat("segments") >= 4
        assert (sp.stat("hbm_bytes") > 0) == (tier != "host") and (sp.stat("host_bytes") > 0) == (tier != "hbm")
        held, replays = _segments(sp), sp.stat("replays")
        eng.sketch_begin(P)
        sp.sketch(eng)
        assert eng.sketch_registers().tobytes() == want.tobytes()
        assert eng.get_stat("sketch_windows") == windows
        assert eng.stats()[1:] == (0, 0)                                # no key was stored
        sp.sketch(eng)                                                  # again: a max does not move
        assert eng.sketch_registers().tobytes() == want.tobytes() and eng.get_stat("sketch_windows") == 2 * windows
        # the spool and the slots are as they were: a replay gives the table of the batches, the slots take a batch
        _same_segments(sp, held)
        assert sp.stat("replays") == replays
        sp.replay(eng, sp.COUNT)
        _direct(ref, batches)
        for x, y in zip(_dump(ref), _dump(eng)):
            assert (x is None and y is None) or np.array_equal(x, y)
        assert ref.stats()[1:] == eng.stats()[1:]
        eng.upload_async(0, _stream(*batches[0]))
        eng.count_uploaded(0)
        assert eng.sketch_registers().tobytes() == want.tobytes()


def test_refusals(case):
    from kmer_denovo_filter_amd._native import KdfError
    k, batches = case
    # no sketch on
    with _spool(1 << 30, 0, segment_positions=1 << 16) as sp, _engine(k) as eng:
        _fill(sp, batches[:3])
        with pytest.raises(KdfError) as ei:
            sp.sketch(eng)
        assert ei.value.code == ERR_STATE and "kdf_sketch_begin" in str(ei.value)
    # an overflowed spool holds a part of the stream: refused, the registers stay zero
    with _spool(SEG_BYTES, 0, segment_positions=1 << 16) as sp, _engine(k) as eng:
        with pytest.raises(KdfError) as ei:
            _fill(sp, batches)
        assert ei.value.code == ERR_NOMEM and sp.stat("overflowed") == 1
        eng.sketch_begin(P)
        with pytest.raises(KdfError) as ei:
            sp.sketch(eng)
        assert ei.value.code == ERR_STATE and "overflowed" in str(ei.value)
        assert int(eng.sketch_registers().max()) == 0 and eng.get_stat("sketch_windows") == 0
    # host-tier segments need the upload slots: a slot that holds a caller's batch refuses the pass, nothing is added
    with _spool(0, 1 << 30, segment_positions=1 << 16) as sp, _engine(k) as eng:
        _fill(sp, batches[:3])
        eng.sketch_begin(P)
        eng.upload_async(1, _stream(*batches[0]))
        with pytest.raises(KdfError) as ei:
            sp.sketch(eng)
        assert ei.value.code == ERR_STATE and "slot 1" in str(ei.value)
        assert int(eng.sketch_registers().max()) == 0
        eng.count_uploaded(1)                                           # the caller's batch is still there
        assert eng.stats()[2] > 0
        sp.sketch(eng)                                                  # ... and with the slots free the pass goes through
        assert eng.sketch_registers().tobytes() == _batchwise(k, batches[:3])[0].tobytes()


def test_spool_and_engine_on_different_devices():
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd._native import KdfError
    from kmer_denovo_filter_amd.spool import ReadSpool
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    with ReadSpool(1, 1 << 20, 0) as sp, KmerEngine(31, capacity_hint=1 << 10, device=0) as eng:
        eng.sketch_begin(P)
        with pytest.raises(KdfError) as ei:
            sp.sketch(eng)
        assert ei.value.code == 1
