"""CPU statement of ProjectedEigen (diskann-quantization/src/multi_vector/distance/projected_eigen.rs, evaluated in
fallback.rs:105-147, 207-226), made from what the oracle exports.

score[i] = the sequential f32 sum over the document's rows j of -(ip(i, j) * ip(i, j)), from +0.0, every operation rounded
on its own; the distance = the sequential f32 sum of score[i] in query-row order, from +0.0.  Only ip depends on the order:
kernel order     one fma chain over k from +0.0: the entry [i, nq + j] of oracle.gram_chain over the stacked rows
reference order  InnerProduct::evaluate(q_i, d_j) = oracle.distance(dtype, IP, q_i, d_j)
"""
import numpy as np

import oracle

KERNEL, REFERENCE = 0, 1


def scores(dtype, order, Q, D):
    """score[i] of query matrix Q against document matrix D (rows of dtype's element type), f32[rows(Q)]"""
    npdt = oracle.NP_DTYPE[dtype]
    Q, D = np.ascontiguousarray(Q, dtype=npdt), np.ascontiguousarray(D, dtype=npdt)
    nq, nd = len(Q), len(D)
    out = np.zeros(nq, np.float32)
    if nd == 0 or nq == 0:
        return out
    if order == KERNEL:
        ip = oracle.gram_chain(np.vstack([Q, D]).astype(np.float32))[:nq, nq:]  # (widening f16 is exact)
    else:
        ip = np.array([[oracle.distance(dtype, oracle.INNER_PRODUCT, q, d) for d in D] for q in Q], np.float32)
    for j in range(nd):  # the sum over j is sequential; the query rows are independent of each other
        out = out + -(ip[:, j] * ip[:, j])
    return out


def total_of(sc):
    """the sequential f32 sum of the per-row scores, from +0.0"""
    s = np.float32(0.0)
    for v in np.asarray(sc, np.float32):
        s = np.float32(s + v)
    return s


def exact(Q, D):
    """(the float64 value, sum over the pairs of (sum_k |q_ik d_jk|)^2: what the rounding-error bound scales with)"""
    Q, D = np.asarray(Q, np.float64), np.asarray(D, np.float64)
    return -((Q @ D.T) ** 2).sum(), ((np.abs(Q) @ np.abs(D).T) ** 2).sum()
