"""tests/maxsim_model.py against plain arithmetic: on small integer-valued rows every summation order is exact, so both
orders of the model must equal a float64 numpy computation and each other; on random rows they agree to the reference's own
kernel tolerance (multi_vector/distance/implementations.rs:518-519) but not necessarily bit for bit."""
import numpy as np
import pytest

import oracle
from helpers import bits
from maxsim_model import F32_MAX, KERNEL, REFERENCE, chamfer, chamfer_of, scores

SHAPES = [(1, 1, 4), (1, 5, 8), (5, 1, 8), (3, 4, 16), (7, 7, 32), (2, 3, 128)]  # the reference's own (nq, nd, dim)


def int_rows(rng, n, dim):
    return rng.integers(-4, 5, (n, dim)).astype(np.float32)


@pytest.mark.parametrize("dtype", [oracle.F32, oracle.F16])
@pytest.mark.parametrize("nq,nd,dim", SHAPES)
def test_both_orders_equal_float64_on_integer_rows(dtype, nq, nd, dim):
    rng = np.random.default_rng(1000 * nq + 10 * nd + dim)
    Q, D = int_rows(rng, nq, dim), int_rows(rng, nd, dim)
    want = (-(Q.astype(np.float64) @ D.astype(np.float64).T).max(axis=1)).astype(np.float32)
    wsum = np.float32(want.astype(np.float64).sum())
    for order in (KERNEL, REFERENCE):
        sc = scores(dtype, order, Q, D)
        assert np.array_equal(sc, want), (order, sc, want)
        assert chamfer(dtype, order, Q, D) == wsum
    assert np.array_equal(scores(dtype, KERNEL, Q, D), scores(dtype, REFERENCE, Q, D))


def test_the_reference_doc_comment_example():
    """multi_vector/distance/mod.rs:19-41"""
    Q = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    D = np.array([[1, 0, 0], [0, 0, 1]], np.float32)
    for order in (KERNEL, REFERENCE):
        sc = scores(oracle.F32, order, Q, D)
        assert sc.tolist() == [-1.0, 0.0]
        assert chamfer(oracle.F32, order, Q, D) == -1.0


@pytest.mark.parametrize("order", [KERNEL, REFERENCE])
def test_empty_document_and_empty_query(order):
    Q = np.ones((3, 8), np.float32)
    empty = np.zeros((0, 8), np.float32)
    sc = scores(oracle.F32, order, Q, empty)
    assert np.array_equal(bits(sc), bits(np.full(3, F32_MAX, np.float32)))
    assert bits(chamfer(oracle.F32, order, Q, empty)) == bits(np.float32(0.0))  # the callback never runs
    assert len(scores(oracle.F32, order, empty, Q)) == 0
    assert bits(chamfer(oracle.F32, order, empty, Q)) == bits(np.float32(0.0))


def test_chamfer_is_a_sequential_f32_sum():
    sc = np.array([1e8, 1.0, -1e8, 1.0], np.float32)
    assert chamfer_of(sc, 1) == np.float32(1.0)  # ((1e8 + 1) - 1e8) + 1: the first 1 is lost, a pairwise sum keeps 2


@pytest.mark.parametrize("dtype", [oracle.F32, oracle.F16])
def test_the_orders_agree_to_the_kernel_tolerance_on_random_rows(dtype):
    rng = np.random.default_rng(7)
    npdt = oracle.NP_DTYPE[dtype]
    differ = 0
    for nq, nd, dim in SHAPES + [(9, 40, 100)]:
        Q = rng.standard_normal((nq, dim)).astype(npdt)
        D = rng.standard_normal((nd, dim)).astype(npdt)
        a, b = scores(dtype, KERNEL, Q, D), scores(dtype, REFERENCE, Q, D)
        scale = np.abs(Q.astype(np.float64)) @ np.abs(D.astype(np.float64)).T
        assert np.all(np.abs(a.astype(np.float64) - b) <= 1e-4 * scale.max(axis=1)), (nq, nd, dim)
        differ += int(np.any(bits(a) != bits(b)))
    assert differ, "the two orders are different summations: some shape must show it"
