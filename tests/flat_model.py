"""CPU model of diskann::flat::FlatIndex::knn_search (diskann/src/flat/index.rs:57-99): every element goes, in ascending id
order, through NeighborPriorityQueue::insert (diskann/src/neighbor/queue.rs:130-171) on a queue of capacity k; the queue's
first k entries are the result.  Two statements of it -- the literal inserts and the closed form the GPU path implements
-- and the lattice the reference's goldens (tests/golden/flat_knn_search.json) were recorded on.  No test functions."""
import json
import math
import os

import numpy as np

from gridutil import grid_data

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flat_knn_search.json")


def flat_knn(dists, k):
    """positions and distances of the queue after inserting dists[0], dists[1], ... one by one.
    insert: a NaN is dropped; a full queue drops a candidate whose distance is above its last one; otherwise the
    candidate goes in at the lower bound -- the first entry whose distance is >= its own -- and a full queue loses its
    last entry."""
    queue = []  # (distance, position)
    for pos, d in enumerate(dists):
        d = np.float32(d)
        if math.isnan(d):
            continue
        if len(queue) == k and queue[-1][0] < d:
            continue
        lb = 0
        while lb < len(queue) and queue[lb][0] < d:
            lb += 1
        queue.insert(lb, (d, pos))
        if len(queue) > k:
            queue.pop()
    return _result(queue)


def flat_knn_closed(dists, k):
    """the first k non-NaN elements under (distance ascending with -0.0 == +0.0, position descending)"""
    items = [(np.float32(d), pos) for pos, d in enumerate(dists) if not math.isnan(d)]
    items.sort(key=lambda e: (float(e[0]), -e[1]))  # (-0.0 == 0.0 as Python floats: the position decides)
    return _result(items[:k])


def _result(entries):
    pos = np.array([p for _, p in entries], dtype=np.int64)
    d = np.array([x for x, _ in entries], dtype=np.float32)
    return pos, d


def padded(pos, d, k, ids=None):
    """the k places of an output row: ids (positions mapped through `ids`) and distances, 0xFFFFFFFF / +inf behind"""
    out_i = np.full(k, 0xFFFFFFFF, np.uint32)
    out_d = np.full(k, np.inf, np.float32)
    out_i[:len(pos)] = pos if ids is None else np.asarray(ids)[pos]
    out_d[:len(pos)] = d
    return out_i, out_d


def grid_rows(dims, size):
    """the rows of the reference's flat test provider: the lattice, no start point (comparisons == size ** dims)"""
    return grid_data(dims, size)


def golden_rows():
    """[(case name, row dict)] of the three golden files"""
    with open(GOLDEN) as f:
        g = json.load(f)
    return [(name, row) for name in sorted(g) for row in g[name]]


def l2_f32(query, rows):
    """squared L2 of small integer-valued lattice points: exact in f32 whatever the summation order"""
    diff = np.asarray(rows, dtype=np.float32) - np.asarray(query, dtype=np.float32)[None, :]
    return (diff * diff).sum(1, dtype=np.float32)
