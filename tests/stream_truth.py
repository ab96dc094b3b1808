"""An independent truth for counts of a packed read stream at ANY size: torch tensor ops only, on whatever device
the stream's tensors live on (the CPU in ``tests/test_stream_truth.py``, HBM in ``tests/test_gpu_full_size_truth.py``).

What it shares with the engine: the stream layout written in ``include/kdf.h`` and nothing else.  Base i is bits
``2 * (i % 32)`` of ``packed[i // 32]``; bit ``i % 64`` of ``invalid[i // 64]`` marks an invalid position; positions
``>= n_bases`` are invalid whatever the padding words hold; a window counts iff none of its k positions is invalid.
It imports neither the package (``keys``, ``devkeys``, ``reads``, the native library) nor the oracle, and it reads
only the packed words of a ``synth.DeviceStream`` -- none of the generator's intermediate base tensors.

Key rule (k <= 63): A = 0, C = 1, G = 2, T = 3, leftmost base most significant; canonical = unsigned minimum of the
k-mer and its reverse complement.  Keys are (lo, hi) int64 tensors holding the bit patterns of the low 64 bits and of
the rest (hi = 0 for k <= 32).  Unsigned order of an int64 word is the signed order of ``word ^ SIGN``; hi stays below
2^62, so its signed order is its unsigned order.  Ascending 128-bit order = a stable sort by lo, then a stable sort
by hi.  A truth is ``(lo, hi, counts int64)``: ascending distinct keys and their counts.

Memory.  Windows are formed ``chunk`` starts at a time (each chunk reads k - 1 positions past its end, so windows
that straddle a chunk boundary are formed once, by the chunk that holds their start): about a dozen int64 temporaries
per start, ~100 bytes x chunk = 13 GB at the default 2^27, whatever the stream's length.  The valid keys of all
chunks are then sorted in one piece, and that sort is the peak: per valid window, the keys (8 bytes, 16 for k > 32),
torch.sort's values and int64 indices (16) and its double buffer (16), plus for k > 32 the gathered (lo, hi) of each
of the two stable sorts (16) -- 40 bytes per window at k <= 32 and 64 at k > 32 by this count; measured on the MI355X
(``torch.cuda.max_memory_allocated``): 64.0 bytes per
valid window at k = 31 (1.16 G windows: 74.5 GB, 1.15 s) and 72.0 at k = 63 (0.83 G windows: 59.5 GB, 3.2 s) -- the
gathers keep their inputs alive longer than the count assumes.  One torch.sort takes fewer than 2^31 elements: a stream
with more valid windows than that is counted piece by piece (sub-streams cut at a tile boundary between reads) or
``key_slice`` by ``key_slice``, and merged by ``accumulate``.

Key slices.  ``slice_of`` cuts the key SPACE into S ranges by the key's top 16 bits (the 2k-bit value, so a property
of the key and not of any hash): slice s holds the keys with ``top16 * S >> 16 == s``.  The slices are ascending
ranges of a sorted dump, equal in width and not in population (canonical keys lean towards the low end: the first of
S slices holds about 1 - (1 - 1/S)^2 of them)."""
import torch

SIGN = -(1 << 63)
CHUNK = 1 << 27


def _parts(stream):
    if isinstance(stream, (tuple, list)):
        packed, invalid, n_bases = stream
    else:
        packed, invalid, n_bases = stream.packed, stream.invalid, stream.n_bases
    return packed, invalid, int(n_bases)


def decode(stream, a, b):
    """(codes int64, invalid bool) of the stream positions [a, b), read from the packed words; positions at or past
    n_bases are invalid (and read no word)."""
    packed, invalid, n_bases = _parts(stream)
    pos = torch.arange(a, b, dtype=torch.int64, device=packed.device)
    past = pos >= n_bases
    at = pos.clamp(max=max(n_bases - 1, 0))
    codes = (packed[at >> 5] >> ((at & 31) << 1)) & 3
    inv = (((invalid[at >> 6] >> (at & 63)) & 1) != 0) | past
    return codes, inv


def _lt(alo, ahi, blo, bhi):
    """a < b as unsigned 128-bit numbers"""
    return (ahi < bhi) | ((ahi == bhi) & ((alo ^ SIGN) < (blo ^ SIGN)))


def windows(codes, inv, k):
    """(lo, hi, valid) of the canonical key of every window start 0 .. len(codes) - k: one base at a time, the forward
    k-mer shifted left by two bits (carried into hi), the reverse complement's base j placed at bits 2j."""
    n = codes.numel() - k + 1
    z = lambda: torch.zeros(n, dtype=torch.int64, device=codes.device)
    flo, fhi, rlo, rhi = z(), z(), z(), z()
    bad = torch.zeros(n, dtype=torch.bool, device=codes.device)
    for j in range(k):
        b = codes[j:j + n]
        bad |= inv[j:j + n]
        if k > 32:
            fhi = (fhi << 2) | ((flo >> 62) & 3)
        flo = (flo << 2) | b
        if 2 * j < 64:
            rlo |= (3 - b) << (2 * j)
        else:
            rhi |= (3 - b) << (2 * j - 64)
    fwd = _lt(flo, fhi, rlo, rhi)
    return torch.where(fwd, flo, rlo), torch.where(fwd, fhi, rhi), ~bad


def slice_of(lo, hi, k, S):
    """The key slice (0 .. S - 1) of every key: ``top16 * S >> 16`` with top16 the top 16 bits of the 2k-bit key
    (a key of fewer than 16 bits is shifted up)."""
    bits = 2 * k
    if bits <= 16:
        top = lo << (16 - bits)
    elif bits <= 64:
        top = (lo >> (bits - 16)) & 0xFFFF
    elif bits - 16 >= 64:
        top = (hi >> (bits - 16 - 64)) & 0xFFFF
    else:                                             # the 16 bits straddle the two words
        sh = bits - 16
        top = (((lo >> sh) & ((1 << (64 - sh)) - 1)) | (hi << (64 - sh))) & 0xFFFF
    return (top * S) >> 16


def sort_keys(lo, hi, *cols):
    """(lo, hi, *cols) reordered to ascending 128-bit key order; stable (equal keys keep their order)."""
    o = torch.sort(lo ^ SIGN, stable=True).indices
    if bool((hi != 0).any()):
        o = o[torch.sort(hi[o], stable=True).indices]
    return (lo[o], hi[o]) + tuple(c[o] for c in cols)


def _segment_sum(lo, hi, weights):
    """Sorted keys with repeats -> (distinct lo, distinct hi, summed int64 weights; weights None: run lengths)."""
    n = lo.numel()
    if n == 0:
        e = torch.zeros(0, dtype=torch.int64, device=lo.device)
        return e, e.clone(), e.clone()
    new = torch.ones(n, dtype=torch.bool, device=lo.device)
    new[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    first = torch.nonzero(new).flatten()
    if weights is None:
        end = torch.cat([first[1:], torch.tensor([n], dtype=torch.int64, device=lo.device)])
        return lo[first], hi[first], end - first
    seg = torch.cumsum(new.to(torch.int64), 0) - 1
    tot = torch.zeros(first.numel(), dtype=torch.int64, device=lo.device).index_add_(0, seg, weights.to(torch.int64))
    return lo[first], hi[first], tot


def count_truth(stream, k, key_slice=None, chunk=CHUNK):
    """-> (lo, hi, counts int64, n_valid_windows) of ``stream`` (a DeviceStream or (packed, invalid, n_bases)).
    ``key_slice=(s, S)``: only the keys of slice s of S (``slice_of``) are kept; n_valid_windows still counts every
    valid window of the stream."""
    assert 1 <= k <= 63 and chunk >= 1
    packed, invalid, n_bases = _parts(stream)
    los, his, n_valid = [], [], 0
    for a in range(0, max(n_bases - k + 1, 0), chunk):
        b = min(a + chunk, n_bases - k + 1)            # window starts [a, b) read positions [a, b + k - 1)
        lo, hi, ok = windows(*decode((packed, invalid, n_bases), a, b + k - 1), k)
        n_valid += int(ok.sum())
        if key_slice is not None:
            ok &= slice_of(lo, hi, k, key_slice[1]) == key_slice[0]
        los.append(lo[ok]); his.append(hi[ok])
        del lo, hi, ok
    if not los:
        e = torch.zeros(0, dtype=torch.int64, device=packed.device)
        return e, e.clone(), e.clone(), 0
    lo, hi = torch.cat(los), torch.cat(his)
    del los, his
    lo, hi = sort_keys(lo, hi)
    return _segment_sum(lo, hi, None) + (n_valid,)


def accumulate(parts):
    """Merge the (lo, hi, counts, ...) of several batches into one truth: concatenate, sort, segment-sum."""
    lo, hi, cnt = (torch.cat([p[i] for p in parts]) for i in range(3))
    lo, hi, cnt = sort_keys(lo, hi, cnt)
    return _segment_sum(lo, hi, cnt)


def take_slice(truth, k, s, S):
    """The rows of a truth (or of any sorted (lo, hi, counts)) whose key lies in slice s of S."""
    keep = slice_of(truth[0], truth[1], k, S) == s
    return truth[0][keep], truth[1][keep], truth[2][keep]


def lower_bound(plo, phi, flo, fhi):
    """For every key f: the number of keys of the ascending set p that are below it (a plain binary search, all keys
    at once)."""
    n = plo.numel()
    l = torch.zeros(flo.numel(), dtype=torch.int64, device=flo.device)
    r = torch.full_like(l, n)
    for _ in range(max(n, 1).bit_length()):
        m = ((l + r) >> 1).clamp(max=max(n - 1, 0))
        open_ = l < r
        below = _lt(plo[m], phi[m], flo, fhi) if n else torch.zeros_like(open_)
        l = torch.where(open_ & below, m + 1, l)
        r = torch.where(open_ & ~below, m, r)
    return l


def member(plo, phi, flo, fhi):
    """bool per key f: is it in the ascending set p?"""
    n = plo.numel()
    if n == 0:
        return torch.zeros(flo.numel(), dtype=torch.bool, device=flo.device)
    at = lower_bound(plo, phi, flo, fhi)
    c = at.clamp(max=n - 1)
    return (at < n) & (plo[c] == flo) & (phi[c] == fhi)


def filtered_truth(parent_truth, filter_keys):
    """The ``count --if`` truth: the count of every filter key (lo, hi) in a count truth, 0 for a key that the parent
    does not hold; in the filter keys' order."""
    plo, phi, pcnt = parent_truth[:3]
    flo, fhi = filter_keys
    n = plo.numel()
    if n == 0:
        return torch.zeros(flo.numel(), dtype=torch.int64, device=flo.device)
    at = lower_bound(plo, phi, flo, fhi)
    c = at.clamp(max=n - 1)
    hit = (at < n) & (plo[c] == flo) & (phi[c] == fhi)
    return torch.where(hit, pcnt[c], torch.zeros_like(pcnt[c]))


def rows_ge(truth, n):
    """rows with count >= n (``dump -L n``)"""
    keep = truth[2] >= n
    return truth[0][keep], truth[1][keep], truth[2][keep]


def rows_le(truth, m):
    """rows with count <= m"""
    keep = truth[2] <= m
    return truth[0][keep], truth[1][keep], truth[2][keep]


def keys_minus(keys, other):
    """the keys (lo, hi) that the ascending set ``other`` (lo, hi, ...) does not hold, order kept"""
    keep = ~member(other[0], other[1], keys[0], keys[1])
    return keys[0][keep], keys[1][keep]
