"""kdf_window_counts_dev / kdf_read_depth_dev against streams whose words at and past ``n_bases`` are dirty, in the
manner of tests/test_gpu_stream_tail.py (its streams, fillings and scan indexes are used as they are).

Device buffers have exactly ``kdf_stream_words(n_bases)`` words; everything at and past n_bases is all ones, zeros,
random bases or the rest of a longer stream; n_bases cuts a read, is a multiple of 64 and is not.  The index holds the
PHANTOM keys (every window that could be formed from the dirty words), so a kernel that trusts those words returns a
count, not a miss that looks right.  Outputs carry guard regions filled with a pattern: counts past n_bases, valid words
past ceil(n_bases / 64) and rows past n_reads must keep it, and no valid bit may lie above n_bases - k.  Every buffer has
its stated size: nothing here reads or writes out of bounds on purpose."""
import numpy as np
import pytest
import torch

import depth_truth as DT
from test_gpu_stream_tail import FILLINGS, dev, new_engine, report, scan_index, streams, truth

pytestmark = pytest.mark.gpu

PATTERN32, PATTERN64, GUARD = 0x3C3C3C3C, 0x3C3C3C3C3C3C3C3C, 192
_KEYS = {}


def index_of(k, keys, counts):
    if k > 63:
        return dict(zip(keys, counts.tolist()))
    lo, hi = keys[0].numpy().view(np.uint64).tolist(), keys[1].numpy().view(np.uint64).tolist()
    return {(h << 64) | l: c for l, h, c in zip(lo, hi, counts.tolist())}


def expected(k, s, index, low_max):
    """(counts[n], valid[n], rows) of the stream's first n positions: the reads cut at n (no window reaches past n)"""
    if (k, s.name) not in _KEYS:
        _KEYS[(k, s.name)] = DT.keys_of_reads(s.cut, k)
    keys = _KEYS[(k, s.name)]
    c, v, offs = DT.profile(s.cut, k, index, keys)
    assert np.array_equal(offs, s.offsets()) and s.n <= len(c) <= s.n + 1      # (the cut read's separator lies at n)
    assert not v[max(s.n - k + 1, 0):].any()
    return c[:s.n], v[:s.n], DT.depth_rows(s.cut, k, index, low_max, keys)


@pytest.mark.parametrize("k", [31, 63, 101])
def test_depth_dev_dirty_tail(k):
    bad = []
    for s in streams(k):
        truth(k, s)                                             # (the precondition: the truth does not depend on the filling)
        n, T, nr = s.n, (s.n + 63) // 64, len(s.cut)
        offs = torch.from_numpy(s.offsets().astype(np.int64)).cuda()
        for f in FILLINGS:
            keys, counts, want_hits = scan_index(k, s, f)
            want_c, want_v, want_r = expected(k, s, index_of(k, keys, counts), 1)
            assert np.array_equal(np.packbits(np.pad(want_c != 0, (0, T * 64 - n)), bitorder="little").view(np.uint64), want_hits)
            d = dev(s, f)
            with new_engine(k) as e:
                if e.long:
                    import kmer_truth as KT
                    e.add_pairs(KT.rows(keys, e.key_words), None, counts)
                else:
                    e.add_pairs(keys[0].numpy().view(np.uint64), keys[1].numpy().view(np.uint64) if e.wide else None, counts)
                dc = torch.full((n + GUARD,), PATTERN32, dtype=torch.int32, device="cuda")
                dv = torch.full((T + GUARD,), PATTERN64, dtype=torch.int64, device="cuda")
                dr = torch.full((nr * 6 + GUARD,), PATTERN64, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                e.window_counts_dev(d[0].data_ptr(), d[1].data_ptr(), n, dc.data_ptr(), dv.data_ptr())
                e.read_depth_dev(d[0].data_ptr(), d[1].data_ptr(), n, offs.data_ptr(), nr, 1, dr.data_ptr())
                e.synchronize()
            c, v, r = dc.cpu().numpy(), dv.cpu().numpy(), dr.cpu().numpy()
            why = []
            if not ((c[n:] == PATTERN32).all() and (v[T:] == PATTERN64).all() and (r[nr * 6:] == PATTERN64).all()):
                why.append("a guard region was written")
            got_v = DT.bits(v[:T].view(np.uint64), T * 64)
            if got_v[max(n - k + 1, 0):].any():
                why.append("a valid bit above n_bases - k")
            if not np.array_equal(got_v[:n], want_v):
                why.append(f"{int((got_v[:n] != want_v).sum())} valid bits differ")
            if not np.array_equal(c[:n].view(np.uint32), want_c):
                why.append(f"{int((c[:n].view(np.uint32) != want_c).sum())} counts differ")
            if not np.array_equal(r[:nr * 6].view(np.uint64).reshape(nr, 6), want_r):
                why.append("rows differ")
            if why:
                bad.append(f"{s.name}/{f}: " + ", ".join(why))
    report(bad)
