"""CPU statement of the multi-vector scores over MinMax-quantised rows (diskann-quantization/src/minmax/multi/max_sim.rs:
MinMaxKernel::max_sim_kernel, MaxSim::evaluate, Chamfer::evaluate), made from tests/minmax_model.py: query image x is the
FIRST argument of the inner-product distance, document image y the second, scores[i] = min_j IP(x_i, y_j) from f32::MAX.
The raw product is an exact integer, so there is one order only; Chamfer is maxsim_model.chamfer_of."""
import numpy as np

import minmax_model as mm
from maxsim_model import F32_MAX, chamfer_of  # noqa: F401  (chamfer_of: re-export)

PAIRS = [(1, 1), (2, 2), (4, 4), (8, 8), (8, 4), (8, 2), (8, 1)]  # (query bits, document bits): bits/distances.rs:1621


def empty(bits, dim):
    """a matrix of no images (minmax_model.compress cannot take 0 rows)"""
    return np.zeros((0, mm.layer_bytes(bits, dim)), np.uint8)


def scores_mm(Q, D, dim, qbits, dbits):
    """the MaxSim scores of query images Q (codes of qbits) against document images D (codes of dbits), f32[rows(Q)]"""
    if len(D) == 0:
        return np.full(len(Q), F32_MAX, np.float32)
    if len(Q) == 0:
        return np.zeros(0, np.float32)
    return mm.distance_matrix(mm.IP, Q, D, dim, dbits, qbits=qbits).min(axis=1)


def chamfer_mm(Q, D, dim, qbits, dbits):
    return chamfer_of(scores_mm(Q, D, dim, qbits, dbits), len(D))
