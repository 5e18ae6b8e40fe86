"""Models of the exhaustive ground-truth scans (dann_flat_filtered_search_batch, dann_flat_range_search_batch) over the
distances of the scanned slots in scan order: the reference's compute_ground_truth_from_data with query_bitmaps feeds the
queue of flat_model only the matching points, and compute_range_ground_truth_from_data lists every matching point within
the radius in ascending id order (diskann-tools/src/utils/ground_truth.rs:285-353, 589-693)."""
import numpy as np

import flat_model as fm


def filtered_knn(dists, match, k):
    """(positions, distances) of the literal inserts and of the closed form over the matching subsequence, mapped back
    to positions of `dists`; the two must agree (the caller asserts it where it matters)"""
    dists = np.asarray(dists, np.float32)
    keep = np.flatnonzero(np.asarray(match, bool))
    pos, d = fm.flat_knn(dists[keep], k)
    cpos, cd = fm.flat_knn_closed(dists[keep], k)
    return (keep[pos], d), (keep[cpos], cd)


def range_scan(dists, match, radius, inner=None):
    """(positions, distances) with d <= radius and, given an inner radius, not d <= inner (range_search.rs:326-335), in
    ascending position; a NaN distance fails the first comparison"""
    dists = np.asarray(dists, np.float32)
    radius = np.float32(radius)
    out = []
    for p in np.flatnonzero(np.asarray(match, bool)):
        d = dists[p]
        if d <= radius and not (inner is not None and d <= np.float32(inner)):
            out.append(p)
    pos = np.array(out, np.int64)
    return pos, dists[pos]
