"""An independent truth for the table join (include/kdf.h, "Table join"), written from the header's text alone: numpy and
a dict, importing neither the package nor the oracle (in the way of ``tests/merge_truth.py`` and ``tests/long_truth.py``).

  An entry (key, c) of table A is SELECTED iff
    - it is stored (every listed entry is, a count of 0 included),
    - min_count <= c <= max_count, and
    - when there is a table B: other_min <= oc <= other_max, where oc is B's count of the key -- 0 when B does not hold
      the key, and 0 when it holds it with count 0.
  Every bound is inclusive; UINT32_MAX (or None here) as an upper bound means none.  Without B the other bounds are
  ignored and every oc reads 0.

Keys are hashable Python values: ints for k <= 32, (lo, hi) tuples for wide keys, tuples of W words for long keys.
``key_order`` gives each form's ascending order, the order of a sorted export."""
import numpy as np

UINT32_MAX = 0xFFFFFFFF


def keys_of(lo, hi=None):
    """The key list of an export: (n,) lo [+ (n,) hi for wide keys], or (n, W) rows of long keys."""
    lo = np.asarray(lo, dtype=np.uint64)
    if lo.ndim == 2:
        return [tuple(r) for r in lo.tolist()]
    if hi is None:
        return lo.tolist()
    return list(zip(lo.tolist(), np.asarray(hi, dtype=np.uint64).tolist()))


def key_order(key):
    """Sort key: a wide key orders by (hi, lo), a row by its words from the top one down."""
    if isinstance(key, tuple):
        return tuple(reversed(key))
    return key


def _upper(v):
    return UINT32_MAX if v is None else int(v)


def join(a_keys, a_counts, b_keys=None, b_counts=None, min_count=1, max_count=None, other_min=0, other_max=0):
    """-> (keys, counts, other_counts) of the selected entries of A, ascending key order.  ``b_keys`` None: no table B."""
    a_counts = [int(c) for c in a_counts]
    assert len(a_keys) == len(a_counts) and len(set(a_keys)) == len(a_keys), "A lists a key twice"
    have_b = b_keys is not None
    b = {}
    if have_b:
        b = dict(zip(b_keys, (int(c) for c in b_counts)))
        assert len(b) == len(b_keys), "B lists a key twice"
    lo_a, hi_a, lo_b, hi_b = int(min_count), _upper(max_count), int(other_min), _upper(other_max)
    out = []
    for key, c in zip(a_keys, a_counts):
        if not lo_a <= c <= hi_a:
            continue
        oc = b.get(key, 0) if have_b else 0
        if have_b and not lo_b <= oc <= hi_b:
            continue
        out.append((key, c, oc))
    out.sort(key=lambda e: key_order(e[0]))
    return [e[0] for e in out], [e[1] for e in out], [e[2] for e in out]


def count(*args, **kw):
    return len(join(*args, **kw)[0])
