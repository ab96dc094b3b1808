"""The stream-order contract of the index record codec with device memory (include/kdf.h "index record codec"), observed
with ``tests/stream_order.py`` in the way of the ``format_kmers_dev`` and ``parse_kmer_fasta_dev`` cases of
``tests/test_gpu_stream_order.py``: decoys in the buffers, the true inputs produced on the caller's stream behind a measured
delay, no host synchronisation before the call, the decoys put back right after it.

The codec's entry points carry a ``mem`` argument instead of a ``_dev`` twin, so the table of that file does not list them;
this file is their table.  ``kdf_index_encode`` and ``kdf_jf_positions`` do not synchronise: they return inside the delay
window.  ``kdf_index_decode`` (the caller learns the bad record) and ``kdf_jf_order`` (the sort) synchronise."""
import numpy as np
import pytest

import test_gpu_stream_order as T
from stream_order import NO_SYNC, SYNCS
from test_gpu_stream_order import H, caller_streams, delay, report  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

KS = (31, 47, 65)
JF_KS = (31, 47)                                         # Jellyfish's order takes k <= 63
N = 3001


def body_of(keys, counts, k, perm=None):
    kb = (2 * k + 7) // 8
    order = range(len(keys)) if perm is None else [int(i) for i in perm]
    return np.frombuffer(b"".join(int(keys[i]).to_bytes(kb, "little") + int(counts[i]).to_bytes(4, "little") for i in order), np.uint8)


def drawn(k, seed):
    """(true keys, decoy keys, true counts, decoy counts, rng): random 2k-bit keys (Python ints), the decoys others of the same form"""
    rng = np.random.default_rng(seed)
    draw = lambda: [int.from_bytes(rng.bytes(52), "little") & ((1 << (2 * k)) - 1) for _ in range(N)]      # noqa: E731
    keys, decoys = draw(), draw()
    assert not set(keys) & set(decoys)
    counts = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    return keys, decoys, counts, rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32), rng


@pytest.mark.parametrize("k", KS)
def test_index_encode_does_not_synchronise(H, k):
    keys, decoys, counts, dcounts, rng = drawn(k, 41)
    perm, dperm = rng.permutation(N).astype(np.uint32), rng.permutation(N).astype(np.uint32)
    with T.engine(H, 31) as e:                           # (the key form follows the call's k, not the engine's)
        R = e.index_record_bytes(k)
        for label, pm in (("", None), (" perm", (perm, dperm))):
            want = body_of(keys, counts, k, None if pm is None else pm[0])
            assert len(want) == N * R
            inputs = dict(T.key_inputs(keys, decoys, k), counts=(counts, dcounts), **({"perm": pm} if pm else {}))
            T.both(H, [e], f"index_encode{label} k={k}", NO_SYNC, lambda: None, inputs, {"bytes": len(want)},
                   lambda p: e.index_encode_dev(p["lo"], p.get("hi"), p["counts"], p.get("perm"), N, k, 0, N * R, p["bytes"]),
                   lambda run: run.read("bytes", np.uint8, N * R), want)


@pytest.mark.parametrize("k", JF_KS)
def test_jf_positions_does_not_synchronise(H, k):
    from kmer_denovo_filter_amd import jf_io
    keys, decoys, _, _, _ = drawn(k, 42)
    cols, size = jf_io.jf_make_matrix(2 * k, 20), 1 << 20
    c = T.key_cols(keys, k)
    want = jf_io.jf_positions(cols, 2 * k, c["lo"], c.get("hi")) & np.uint64(size - 1)
    with T.engine(H, 31) as e:
        T.both(H, [e], f"jf_positions k={k}", NO_SYNC, lambda: None, T.key_inputs(keys, decoys, k), {"pos": N * 8},
               lambda p: e.jf_positions_dev(p["lo"], p.get("hi"), N, k, cols, size, p["pos"]),
               lambda run: run.read("pos", np.uint64, N), want)


@pytest.mark.parametrize("k", KS)
def test_index_decode_synchronises(H, k):
    keys, decoys, counts, dcounts, _ = drawn(k, 43)
    data, other = body_of(keys, counts, k), body_of(decoys, dcounts, k)
    want = dict(T.key_cols(keys, k), counts=counts)
    W = T.PM.key_words(k)
    with T.engine(H, 31) as e:
        def observe(run):
            got = {"lo": run.read("lo", np.uint64, N * (W if k > 63 else 1)).reshape(want["lo"].shape), "counts": run.read("counts", np.uint32, N)}
            if 32 < k <= 63:
                got["hi"] = run.read("hi", np.uint64, N)
            return got
        T.both(H, [e], f"index_decode k={k}", SYNCS, lambda: None, {"bytes": (data, other)},
               {"lo": N * 8 * (W if k > 63 else 1), "hi": N * 8, "counts": N * 4},
               lambda p: e.index_decode_dev(p["bytes"], N, k, 4, p["lo"], p["hi"] if 32 < k <= 63 else None, p["counts"]), observe, want)


@pytest.mark.parametrize("k", JF_KS)
def test_jf_order_synchronises(H, k):
    from kmer_denovo_filter_amd import jf_io
    from kmer_denovo_filter_amd import keys as K
    keys, decoys, _, _, _ = drawn(k, 44)
    keys = sorted(set(keys))                             # (distinct, so the order is unique)
    decoys = decoys[:len(keys)]
    n = len(keys)
    cols, size = jf_io.jf_make_matrix(2 * k, 10), 1 << 10
    c = T.key_cols(keys, k)
    words = K.from_pair(c["lo"], c.get("hi"), k)
    want = K.order(words, jf_io.jf_positions(cols, 2 * k, c["lo"], c.get("hi")) & np.uint64(size - 1)).astype(np.uint32)
    with T.engine(H, 31) as e:
        T.both(H, [e], f"jf_order k={k}", SYNCS, lambda: None, T.key_inputs(keys, decoys, k), {"perm": n * 4},
               lambda p: e.jf_order_dev(p["lo"], p.get("hi"), n, k, cols, size, p["perm"]),
               lambda run: run.read("perm", np.uint32, n), want)
