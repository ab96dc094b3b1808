"""The model of include/kdf.h "regions of informative reads", written from the header's text alone in plain Python and
numpy: the literal sort-and-sweep for kdf_cluster_intervals*, a ``set`` of row tuples per group for
kdf_group_distinct*.  No engine import: the tests compare the engine (and the mirror's host sweep) against this."""
import numpy as np


def cluster_intervals(chrom, start, end, merge_distance):
    """-> (region_of int64[n], regions int64 (m, 4): chrom, start of the first interval, max end, members)"""
    chrom = np.asarray(chrom, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    region_of = np.full(len(chrom), -1, np.int64)
    order = sorted((i for i in range(len(chrom)) if chrom[i] >= 0), key=lambda i: (int(chrom[i]), int(start[i])))
    regions = []
    cur_chrom, running_end = None, None                  # E_i: the maximum end over the earlier intervals of the same chrom
    for i in order:
        c, s, e = int(chrom[i]), int(start[i]), int(end[i])
        if cur_chrom != c:                               # the first of its chrom
            regions.append([c, s, e, 0])
            cur_chrom, running_end = c, e
        elif s > running_end + int(merge_distance):
            regions.append([c, s, e, 0])
        running_end = max(running_end, e)
        g = len(regions) - 1
        regions[g][2] = max(regions[g][2], e)
        regions[g][3] += 1
        region_of[i] = g
    return region_of, np.asarray(regions, dtype=np.int64).reshape(-1, 4)


def group_distinct(group, keys, n_groups):
    """-> uint64[n_groups]: distinct rows of the entries of each group; groups outside [0, n_groups) and rows of
    all-ones words are ignored"""
    group = np.asarray(group, dtype=np.int64)
    keys = np.asarray(keys, dtype=np.uint64)
    if keys.ndim == 1:
        keys = keys.reshape(-1, 1)
    ones = int(np.uint64(0xFFFFFFFFFFFFFFFF))
    sets = [set() for _ in range(max(int(n_groups), 0))]
    for g, row in zip(group.tolist(), keys.tolist()):
        if 0 <= g < n_groups and not all(w == ones for w in row):
            sets[g].add(tuple(row))
    return np.asarray([len(s) for s in sets], dtype=np.uint64)
