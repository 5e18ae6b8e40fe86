"""CPU statement of dann_mv_flat_search_batch: compute_multivec_ground_truth_from_data (diskann-tools/src/utils/
ground_truth.rs:696-787).  Per (query, document) the MaxSim scores of tests/maxsim_model.py, one of three aggregations written
in np.float32 steps, then the literal queue of tests/flat_model.py over the accepted documents.  No test functions."""
import numpy as np

import flat_model as fm
import maxsim_model as mm

CHAMFER, AVG_OF_MINS, MIN_PAIRWISE, AVERAGE_PAIRWISE = 0, 1, 2, 3
AGGREGATIONS = [CHAMFER, AVG_OF_MINS, MIN_PAIRWISE]
# Document lengths against the 32-row tile (329 rows), and the set the GPU tests scan: ten repetitions span three chunks of
# CHUNK rows -- the plan's chunk for a small call, which tests/test_mv_flat_model_host.py checks on the plan itself -- a
# document that fills the fourth chunk to its end puts two empty documents exactly on a chunk boundary, and the set ends
# with an empty document
LENS = [1, 2, 31, 32, 33, 64, 65, 0, 0, 1, 100]
CHUNK = 1024
TILE_LENS = tuple(LENS * 10 + [4 * CHUNK - 10 * sum(LENS), 0, 0, 5, 0])


def all_scores(dtype, order, Q, docs):
    """the per-row scores of Q against every document: the expensive part, shared by the aggregations"""
    return [mm.scores(dtype, order, Q, D) for D in docs]


def aggregate(aggregation, sc, nd):
    """one document's distance from its per-row scores `sc` (nd: the document's rows)"""
    sc = np.asarray(sc, np.float32)
    with np.errstate(all="ignore"):
        if aggregation == CHAMFER:
            return mm.chamfer_of(sc, nd)  # (a document without rows: 0.0, the sum never runs)
        if aggregation == AVG_OF_MINS:
            s = np.float32(0.0)
            for v in sc:
                s = np.float32(s + v)
            return np.float32(s / np.float32(len(sc)))  # (no rows in the query: 0.0 / 0.0)
        m = mm.F32_MAX
        for v in sc:
            if v < m:
                m = v
        return np.float32(m)


def search(scores, docs, aggregation, k, first=0, n=None, match=None):
    """(ids[k], dists[k], cmps) of one query: `scores` = all_scores(...), match = a bool per document or None"""
    n = len(docs) - first if n is None else n
    ids = [d for d in range(first, first + n) if match is None or match[d]]
    dists = np.array([aggregate(aggregation, scores[d], len(docs[d])) for d in ids], np.float32)
    pos, d = fm.flat_knn(dists, k)
    out_i, out_d = fm.padded(pos, d, k, ids=np.asarray(ids, np.uint32))
    return out_i, out_d, len(ids)
