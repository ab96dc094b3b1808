"""kdf_window_counts_dev / kdf_read_depth_dev at full size against a truth that shares only the stream layout with
the engine, in the manner of tests/test_gpu_full_size_truth.py.

A synth stream of 1 M reads x 150 bp (151 M positions) at k = 31 and k = 63, the table counted from it.  The key of
EVERY position comes from ``tests/stream_truth.windows`` (torch, one base at a time over the packed words), its count
from ``kdf_query_dev`` on those keys; ``window_counts_dev`` must equal that position by position, its valid words bit by
bit, and ``read_depth_dev`` the torch segment reduction of it row by row.  No position and no read is skipped."""
import pytest
import torch

import stream_truth as ST

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
READS, READ_LEN, CHUNK = 1_000_000, 150, 1 << 24
LOW_MAX = 2


@pytest.mark.parametrize("k", [31, 63])
def test_every_position_and_every_read(k):
    from kmer_denovo_filter_amd import KmerEngine
    from kmer_denovo_filter_amd.synth import synth_stream
    ds = synth_stream(READS, READ_LEN, 20_000_000, seed=20260421, device=DEV)
    torch.cuda.synchronize()
    n, L1 = ds.n_bases, READ_LEN + 1
    assert n == READS * L1 and ds.n_reads == READS
    T = (n + 63) // 64
    stream = (ds.packed, ds.invalid, n)
    with KmerEngine(k, capacity_hint=1 << 26) as e:
        e.count_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), n)
        got_c = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        got_v = torch.full((T,), -1, dtype=torch.int64, device=DEV)
        offs = torch.arange(READS + 1, dtype=torch.int64, device=DEV) * L1
        got_r = torch.full((READS, 6), -1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        e.window_counts_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), n, got_c.data_ptr(), got_v.data_ptr())
        e.read_depth_dev(ds.packed.data_ptr(), ds.invalid.data_ptr(), n, offs.data_ptr(), READS, LOW_MAX, got_r.data_ptr())
        e.synchronize()
        # the truth, chunk by chunk: every one of the n positions
        want_c = torch.empty(n, dtype=torch.int64, device=DEV)
        want_v = torch.empty(n, dtype=torch.bool, device=DEV)
        compared = 0
        for a in range(0, n, CHUNK):
            b = min(a + CHUNK, n)
            lo, hi, ok = ST.windows(*ST.decode(stream, a, b + k - 1), k)      # (positions at or past n decode as invalid)
            assert lo.numel() == b - a
            lo, hi = lo.contiguous(), hi.contiguous()
            q = torch.empty(b - a, dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            e.query_dev(lo.data_ptr(), hi.data_ptr() if k > 32 else None, b - a, q.data_ptr())
            e.synchronize()
            want_c[a:b] = torch.where(ok, q.to(torch.int64) & 0xFFFFFFFF, torch.zeros_like(lo))
            want_v[a:b] = ok
            compared += b - a
            del lo, hi, ok, q
        assert compared == n
    got = got_c.to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got, want_c), f"{int((got != want_c).sum())} of {n} counts differ from the truth"
    pos = torch.arange(n, dtype=torch.int64, device=DEV)
    bits = ((got_v[pos >> 6] >> (pos & 63)) & 1) != 0
    assert torch.equal(bits, want_v), f"{int((bits != want_v).sum())} of {n} valid bits differ from the truth"
    if n % 64:
        assert int(got_v[-1].item()) >> (n % 64) == 0
    del pos, bits, got
    valid_windows = int(want_v.sum().item())
    assert valid_windows > (READ_LEN - k + 1) * READS * 3 // 4 and int((want_c > 1).sum().item()) > valid_windows // 2
    # the segment reduction over the reads' offsets (every read is L1 positions long)
    assert torch.equal(offs[1:] - offs[:-1], torch.full((READS,), L1, dtype=torch.int64, device=DEV))
    c, v = want_c.view(READS, L1), want_v.view(READS, L1)
    windows = v.sum(1)
    big = torch.full_like(c, 1 << 40)
    want_r = torch.stack([windows, (v & (c > 0)).sum(1), (v & (c <= LOW_MAX)).sum(1),
                          torch.where(windows > 0, torch.where(v, c, big).min(1).values, torch.zeros_like(windows)),
                          torch.where(v, c, torch.zeros_like(c)).max(1).values, torch.where(v, c, torch.zeros_like(c)).sum(1)], dim=1)
    assert want_r.shape == (READS, 6)
    assert torch.equal(got_r, want_r), f"{int((got_r != want_r).any(1).sum())} of {READS} rows differ from the truth"
    assert int(want_r[:, 2].sum().item()) > 0
