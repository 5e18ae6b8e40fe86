"""tests/maxsim_mm_model.py against plain arithmetic, the bias identity the int8 matrix-core kernel rests on, and the
presence of the two new C calls.  No GPU."""
import os
import re

import numpy as np
import pytest

import minmax_model as mm
from helpers import bits
from maxsim_mm_model import PAIRS, chamfer_mm, empty, scores_mm
from maxsim_model import F32_MAX, chamfer_of

SHAPES = [(1, 1, 4), (1, 5, 8), (5, 1, 8), (3, 4, 16), (7, 7, 32), (2, 3, 128)]  # the reference's own (nq, nd, dim)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_pairs_are_the_references():
    assert PAIRS == [(1, 1), (2, 2), (4, 4), (8, 8), (8, 4), (8, 2), (8, 1)]


@pytest.mark.parametrize("qbits,dbits", PAIRS)
@pytest.mark.parametrize("nq,nd,dim", SHAPES)
def test_twin_rows_score_the_negated_best_raw_product(qbits, dbits, nq, nd, dim):
    """a = 1, b = 0: v = raw exactly (every intermediate an integer below 2^24), so scores = -max_j raw"""
    rng = np.random.default_rng(1000 * nq + 10 * nd + dim + qbits + dbits)
    cq = rng.integers(0, 1 << qbits, (nq, dim)).astype(np.uint8)
    cd = rng.integers(0, 1 << dbits, (nd, dim)).astype(np.uint8)
    Q, D = mm.twin_rows(cq, qbits), mm.twin_rows(cd, dbits)
    raw = cq.astype(np.float64) @ cd.astype(np.float64).T
    want = (-raw.max(axis=1)).astype(np.float32)
    got = scores_mm(Q, D, dim, qbits, dbits)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert chamfer_mm(Q, D, dim, qbits, dbits) == np.float32(want.astype(np.float64).sum())


def reference_input(n, dim, offset):
    """generate_input_mat (max_sim.rs:186-194): ((i + offset) * dim + j) as f32 * 0.1"""
    i, j = np.meshgrid(np.arange(n), np.arange(dim), indexing="ij")
    return ((i + offset) * dim + j).astype(np.float32) * np.float32(0.1)


@pytest.mark.parametrize("qbits,dbits", PAIRS)
@pytest.mark.parametrize("nq,nd,dim", SHAPES)
def test_the_references_inputs_match_a_naive_fold(qbits, dbits, nq, nd, dim):
    """test_matches_naive (max_sim.rs:239-292): queries at offset 0, documents at offset nq, grid_scale 1.0; expected =
    per query row the fold of f32::min from f32::MAX over one MinMaxIP evaluation per document row"""
    Q = mm.compress(reference_input(nq, dim, 0), qbits, 1.0)[0]
    D = mm.compress(reference_input(nd, dim, nq), dbits, 1.0)[0]
    want = np.empty(nq, np.float32)
    for i in range(nq):
        m = F32_MAX
        for j in range(nd):
            d = mm.distance_matrix(mm.IP, Q[i:i + 1], D[j:j + 1], dim, dbits, qbits=qbits)[0, 0]
            m = d if d < m else m
        want[i] = m
    got = scores_mm(Q, D, dim, qbits, dbits)
    assert np.array_equal(bits(got), bits(want))
    s = np.float32(0.0)
    for v in want:
        s = np.float32(s + v)
    assert bits(chamfer_mm(Q, D, dim, qbits, dbits)) == bits(s)


@pytest.mark.parametrize("qbits,dbits", PAIRS)
def test_empty_document_and_empty_query(qbits, dbits):
    dim = 8
    Q = mm.compress(np.arange(24, dtype=np.float32).reshape(3, dim), qbits)[0]
    D = mm.compress(np.arange(16, dtype=np.float32).reshape(2, dim), dbits)[0]
    sc = scores_mm(Q, empty(dbits, dim), dim, qbits, dbits)
    assert np.array_equal(bits(sc), bits(np.full(3, F32_MAX, np.float32)))
    assert bits(chamfer_mm(Q, empty(dbits, dim), dim, qbits, dbits)) == bits(np.float32(0.0))
    assert len(scores_mm(empty(qbits, dim), D, dim, qbits, dbits)) == 0
    assert bits(chamfer_mm(empty(qbits, dim), D, dim, qbits, dbits)) == bits(np.float32(0.0))
    assert chamfer_of(sc, 0) == 0.0


def biased(codes, beta):
    """the bytes the matrix cores see: c - 128 for an 8-bit side, padded with zeros AFTER biasing to a multiple of 32;
    and their sum over k < dim"""
    n, dim = codes.shape
    out = np.zeros((n, (dim + 31) // 32 * 32), np.int32)
    out[:, :dim] = codes.astype(np.int32) - (128 if beta else 0)
    assert out.min() >= -128 and out.max() <= 127
    return out, out[:, :dim].sum(axis=1, dtype=np.int32)


@pytest.mark.parametrize("beta_q", [0, 1])
@pytest.mark.parametrize("beta_d", [0, 1])
@pytest.mark.parametrize("dim", [1, 31, 33, 128, 4096])
def test_the_bias_identity_in_wrapping_int32(beta_q, beta_d, dim):
    """sum cq cd == sum q' d' + 128 beta_d sum q' + 128 beta_q sum d' + 16384 beta_q beta_d dim, every step an int32"""
    rng = np.random.default_rng(100 * dim + 2 * beta_q + beta_d)
    top_q, top_d = (255 if beta_q else 15), (255 if beta_d else 15)
    cq = rng.integers(0, top_q + 1, (5, dim)).astype(np.uint8)
    cd = rng.integers(0, top_d + 1, (6, dim)).astype(np.uint8)
    cq[0], cd[0] = top_q, top_d  # every code at its maximum: 255^2 * 4096 < 2^31
    cq[1], cd[1] = 0, 0
    true = cq.astype(np.int64) @ cd.astype(np.int64).T
    assert true.max() < (1 << 31)
    qp, qs = biased(cq, beta_q)
    dp, ds = biased(cd, beta_d)
    with np.errstate(over="ignore"):
        acc = (qp @ dp.T).astype(np.int32)  # (the padding columns take part: they must add nothing)
        got = (acc + np.int32(128 * beta_d) * qs[:, None] + np.int32(128 * beta_q) * ds[None, :]
               + np.int32(16384 * beta_q * beta_d) * np.int32(dim))
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), true)
    if beta_q and beta_d and dim == 4096:
        assert true[0, 0] == 266_342_400 and true[0, 0] > (1 << 24)


def test_padding_before_biasing_would_be_wrong():
    """the trap: a byte at k >= dim stored as 0 ^ 0x80 = -128 adds 128 * 128 per padded column"""
    dim = 5
    c = np.full((1, dim), 200, np.uint8)
    qp, qs = biased(c, 1)
    wrong = qp.copy()
    wrong[:, dim:] = -128
    assert (wrong @ wrong.T)[0, 0] - (qp @ qp.T)[0, 0] == 27 * 16384


def test_the_new_calls_are_declared_and_exported():
    import diskann_amd as da
    hdr = open(os.path.join(ROOT, "include", "dann.h")).read()
    assert re.search(r"int32_t\s+dann_mvset_set_query_dtype\(dann_mvset\*\s*set,\s*int32_t\s+dtype\);", hdr)
    assert re.search(r"int32_t\s+dann_mvset_get_query_dtype\(const dann_mvset\*\s*set,\s*int32_t\*\s*out\);", hdr)
    L = da.lib()
    for name in ("dann_mvset_set_query_dtype", "dann_mvset_get_query_dtype"):
        assert name in da._ffi.SYMBOLS and getattr(L, name) is not None
    assert da._ffi.SYMBOLS["dann_abi_version"] is not None and L.dann_abi_version() == 5
