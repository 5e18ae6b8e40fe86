"""CPU statement of the multi-vector scores (diskann-quantization/src/multi_vector/), made from what the oracle exports.

kernel order     (build_max_sim(Auto | V3 | V4).compute_max_sim): ip(i, j) = one fma chain over k from +0.0 -- the entry
                 [i, nq + j] of oracle.gram_chain over the stacked rows (fma(a, b, c) == fma(b, a, c)) -- then
                 scores[i] = -max_j ip(i, j), f32::MAX for a document without rows
reference order  (MaxSim::evaluate, Chamfer::evaluate, MaxSimIsa::Reference): scores[i] = min_j
                 InnerProduct::evaluate(q_i, d_j) = oracle.distance(dtype, IP, q_i, d_j), the minimum from f32::MAX
Chamfer          the sequential f32 sum of scores[i] in query-row order; 0.0 for a document or a query without rows
"""
import numpy as np

import oracle

KERNEL, REFERENCE = 0, 1
F32_MAX = np.float32(np.finfo(np.float32).max)


def scores(dtype, order, Q, D):
    """the MaxSim scores of query matrix Q against document matrix D (rows of dtype's element type), f32[rows(Q)]"""
    npdt = oracle.NP_DTYPE[dtype]
    Q = np.ascontiguousarray(Q, dtype=npdt)
    D = np.ascontiguousarray(D, dtype=npdt)
    nq, nd = len(Q), len(D)
    out = np.full(nq, F32_MAX, np.float32)
    if nd == 0 or nq == 0:
        return out
    if order == KERNEL:
        ip = oracle.gram_chain(np.vstack([Q, D]).astype(np.float32))[:nq, nq:]  # (widening f16 is exact)
        return (-ip.max(axis=1)).astype(np.float32)
    for i in range(nq):
        m = F32_MAX
        for j in range(nd):
            d = np.float32(oracle.distance(dtype, oracle.INNER_PRODUCT, Q[i], D[j]))
            if d < m:
                m = d
        out[i] = m
    return out


def chamfer_of(sc, nd):
    """Chamfer::evaluate from the scores: a sequential f32 sum; a document without rows never reaches the sum"""
    if nd == 0:
        return np.float32(0.0)
    s = np.float32(0.0)
    for v in np.asarray(sc, np.float32):
        s = np.float32(s + v)
    return s


def chamfer(dtype, order, Q, D):
    return chamfer_of(scores(dtype, order, Q, D), len(D))
