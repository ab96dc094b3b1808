"""Unit cases of the join model (tests/join_truth.py): the selection rule of include/kdf.h "Table join" on lists small
enough to check by eye.  No GPU, no package import."""
import numpy as np

import join_truth as J

A_KEYS = [10, 11, 12, 13, 14, 15]
A_CNT = [0, 1, 2, 3, 4, 5]
B_KEYS = [11, 12, 13, 99]
B_CNT = [7, 0, 2, 4]           # 12 is stored in B with count 0; 99 is not in A


def sel(**kw):
    return J.join(A_KEYS, A_CNT, B_KEYS, B_CNT, **kw)


def test_bounds_on_own_count_are_inclusive():
    keys, cnt, oc = sel(min_count=2, max_count=4, other_min=0, other_max=None)
    assert keys == [12, 13, 14] and cnt == [2, 3, 4] and oc == [0, 2, 0]
    assert sel(min_count=3, max_count=3, other_min=0, other_max=None)[0] == [13]
    assert sel(min_count=6, max_count=None, other_min=0, other_max=None)[0] == []


def test_bounds_on_other_count_are_inclusive():
    assert sel(min_count=0, max_count=None, other_min=2, other_max=7)[0] == [11, 13]
    assert sel(min_count=0, max_count=None, other_min=2, other_max=6)[0] == [13]
    assert sel(min_count=0, max_count=None, other_min=3, other_max=7)[0] == [11]
    assert sel(min_count=0, max_count=None, other_min=7, other_max=7) == ([11], [1], [7])


def test_stored_count_zero_reads_as_absent():
    # reference subtraction: other 0..0 keeps the keys B lacks AND the one B stores with count 0
    keys, cnt, oc = sel(min_count=1, max_count=None, other_min=0, other_max=0)
    assert keys == [12, 14, 15] and oc == [0, 0, 0]
    # ... and other >= 1 drops both alike
    assert sel(min_count=0, max_count=None, other_min=1, other_max=None)[0] == [11, 13]


def test_min_count_zero_takes_stored_zero_counts_of_a():
    assert sel(min_count=0, max_count=0, other_min=0, other_max=None) == ([10], [0], [0])
    assert J.count(A_KEYS, A_CNT, B_KEYS, B_CNT, min_count=0, max_count=None, other_min=0, other_max=None) == 6


def test_uint32_max_is_unbounded():
    big = A_CNT[:-1] + [J.UINT32_MAX]
    assert J.join(A_KEYS, big, None, None, min_count=1, max_count=J.UINT32_MAX)[0] == [11, 12, 13, 14, 15]
    assert J.join(A_KEYS, big, None, None, min_count=1, max_count=None)[0] == [11, 12, 13, 14, 15]
    assert J.join(A_KEYS, big, None, None, min_count=1, max_count=J.UINT32_MAX - 1)[0] == [11, 12, 13, 14]
    bb = [J.UINT32_MAX, 0, 2, 4]
    assert J.join(A_KEYS, A_CNT, B_KEYS, bb, min_count=0, other_min=3, other_max=J.UINT32_MAX)[0] == [11]
    assert J.join(A_KEYS, A_CNT, B_KEYS, bb, min_count=0, other_min=3, other_max=None)[0] == [11]


def test_other_none_ignores_the_other_bounds():
    keys, cnt, oc = J.join(A_KEYS, A_CNT, None, None, min_count=0, max_count=2, other_min=5, other_max=7)
    assert keys == [10, 11, 12] and cnt == [0, 1, 2] and oc == [0, 0, 0]
    # an EMPTY table B is not "no table": the bounds then apply to oc = 0
    assert J.join(A_KEYS, A_CNT, [], [], min_count=0, max_count=2, other_min=5, other_max=7)[0] == []


def test_key_forms_and_order():
    lo = np.array([5, 1, 3], np.uint64)
    hi = np.array([0, 2, 1], np.uint64)
    wide = J.keys_of(lo, hi)
    assert wide == [(5, 0), (1, 2), (3, 1)]
    keys, cnt, _ = J.join(wide, [1, 2, 3], None, None, min_count=1)
    assert keys == [(5, 0), (3, 1), (1, 2)] and cnt == [1, 3, 2]           # ascending by (hi, lo)
    rows = J.keys_of(np.array([[9, 9, 1], [0, 0, 2], [8, 0, 1]], np.uint64))
    keys, cnt, _ = J.join(rows, [1, 2, 3], None, None, min_count=1)
    assert keys == [(8, 0, 1), (9, 9, 1), (0, 0, 2)] and cnt == [3, 1, 2]   # from the top word down
    assert J.keys_of(np.array([7, 2], np.uint64)) == [7, 2]
