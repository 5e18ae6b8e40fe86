"""CPU restatement of graph consolidation (DiskANNIndex::consolidate_vector, diskann/src/graph/index.rs:1819-1930) over
the oracle's Index, in the pool order include/dann.h defines for dann_consolidate: the vertex's own live neighbours in
list order, then the live neighbours of each deleted neighbour, the deleted neighbours in list order."""
import numpy as np

import oracle

COMPLETE, DELETED = 0, 1


def pair_distance(oix, x, y):
    """d(row x, row y) as the index evaluates it: the oracle's element-type distance, or for SQ-8 rows the compensated
    distance with the index's quantiser parameters (CompensatedSquaredL2 / IP / CosineNormalized), or for a TABLE index
    the caller's table entry, x naming the table row"""
    if oix.dtype == oracle.TABLE:
        return np.float32(oix.table[x, y])
    return row_distance(oix, oix.rows[x, :oix.row_bytes], oix.rows[y, :oix.row_bytes])


def row_distance(oix, a, b):
    """pair_distance for two row images (payload bytes) that need not be stored in the index"""
    if oix.dtype != oracle.SQ8:
        dt = oracle.NP_DTYPE[oix.dtype]
        return oracle.distance(oix.dtype, oix.metric, np.ascontiguousarray(a).view(dt), np.ascontiguousarray(b).view(dt))
    import ctypes as C
    dim = oix.dim
    a = np.ascontiguousarray(a[:dim + 4])
    b = np.ascontiguousarray(b[:dim + 4])
    metric = oix.metric if oix.metric != oracle.COSINE_NORMALIZED else oracle.L2
    d = oracle.lib().orc_sq8_distance(metric, a.ctypes.data, C.c_float(a[dim:].view(np.float32)[0]), b.ctypes.data,
                                      C.c_float(b[dim:].view(np.float32)[0]), dim, C.c_float(oix._c.sq_scale),
                                      C.c_float(oix._c.sq_shift_norm_sq))
    if oix.metric == oracle.COSINE_NORMALIZED:
        d = np.float32(1.0) - (np.float32(1.0) - np.float32(d) / np.float32(2.0))
    return np.float32(d)


def robust_prune_list(oix, cfg, v, pool):
    """robust_prune_list (index.rs:2397-2454, force_saturate = false): d(v, c) in pool order, skipping v, then the prune"""
    pool = [int(i) for i in pool if int(i) != v]
    dists = np.array([pair_distance(oix, v, i) for i in pool], np.float32)
    out, _ = oix.prune_pool(cfg, v, np.array(pool, np.uint32), dists, force_saturate=False)
    return out


def consolidate_vector(oix, cfg, deleted, v):
    """one vertex; `deleted` is a boolean array over the slots.  Rewrites oix.adj[v] where the reference would."""
    if deleted[v]:
        return DELETED
    pool, seen, dead = [], set(), []
    self_listed = False
    for i in oix.neighbors(v):
        i = int(i)
        if deleted[i]:
            dead.append(i)
        elif i == v:
            self_listed = True  # in the reference's HashSet until the self-loop is removed, after this test
        elif i not in seen:
            seen.add(i)
            pool.append(i)
    if not dead and len(pool) + int(self_listed) <= cfg.pruned_degree:
        return COMPLETE
    for d in dead:
        for i in oix.neighbors(d):
            i = int(i)
            if not deleted[i] and i != v and i not in seen:
                seen.add(i)
                pool.append(i)
    if len(pool) < cfg.pruned_degree:
        oix.set_neighbors(v, pool)
    else:
        oix.set_neighbors(v, robust_prune_list(oix, cfg, v, pool))
    return COMPLETE


def consolidate(oix, cfg, deleted, ids=None, drop_deleted=False):
    """consolidate_vector on every id in order (None: every slot, start points included) -> kinds"""
    if ids is None:
        ids = range(oix.adj.shape[0])
    kinds = np.array([consolidate_vector(oix, cfg, deleted, int(v)) for v in ids], np.int32)
    if drop_deleted:
        oix.adj[np.asarray(deleted, bool), 0] = 0  # drop_adj_list (index.rs:1060)
    return kinds
