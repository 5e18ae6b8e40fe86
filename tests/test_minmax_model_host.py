"""tests/minmax_model.py pinned without a GPU: the distance forms against float64 dot products of the decompressed
vectors (the reference's own unit-test tolerances, minmax/vectors.rs:566-620, or tighter ones derived from f32's precision), the compressor's post-conditions
(minmax/quantizer.rs:632-757), the exact twin against the oracle's U8 L2 distance in both argument orders, and that the
random sample the GPU test draws contains pairs whose two argument orders differ in bits."""
import numpy as np
import pytest

import minmax_model as m
import oracle
from helpers import bits as fbits
from minmax_builders import random_rows


EPS = 2.0 ** -24  # half an ulp of f32, relative


@pytest.mark.parametrize("bits", m.BITS)
def test_distances_against_float64(bits):
    """The model against float64 arithmetic on the decompressed vectors a * code + b, with the header's own (f32) n and
    norm_squared as the reference's test takes them.  Bounds, per metric:
      InnerProduct      the reference asserts 1e-3 relative (vectors.rs:566-572); here |got - want| / |want| < 1e-6: nothing
                        cancels on these inputs (codes, a, b >= 0) and |v - ip| <= 10 EPS ip = 6e-7 ip, see below.
                        Measured worst 2.3e-7.
      Cosine            |got - want| < 1e-6 or |got - want| / want < 1e-3: the reference's (vectors.rs:598-607).
      CosineNormalized  the reference asserts 1e-6 relative to 1 - ip (vectors.rs:613-620) on vectors of at most 2^bits - 1
                        dimensions.  1 - v cancels where ip is near 1 (dim 1 at 1 bit: worst 1.3e-5 relative), so the
                        bound here is 1e-6 of the larger operand, max(|1 - ip|, ip): v is a sum of four non-negative
                        terms, evaluated with at most 8 roundings on inputs n that carry one more, so
                        |v - ip| <= 10 EPS ip = 6e-7 ip, and the subtraction adds EPS |1 - v|.
      L2                pure relative error fails through cancellation (x == y gives want == 0).  Bound: 1e-6 (nx + ny).
                        -2 v carries 2 * 10 EPS ip <= 10 EPS (nx + ny) = 6e-7 (nx + ny) because 2 ip <= nx + ny; the
                        two additions and the two f32 norms add at most 4 EPS (nx + ny) = 2.4e-7 (nx + ny)."""
    rng = np.random.default_rng(10 + bits)
    worst = {}
    for dim in (1, 7, 33, 100, 128, 260):
        x, y = random_rows(rng, 24, dim, bits), random_rows(rng, 40, dim, bits)
        fx, fy = m.decompress(x, bits, dim), m.decompress(y, bits, dim)
        ip = fx @ fy.T
        nx, ny = m.header(x)[4].astype(np.float64)[:, None], m.header(y)[4].astype(np.float64)[None, :]
        assert np.allclose(nx[:, 0], (fx * fx).sum(1), rtol=2 * EPS) and np.allclose(ny[0], (fy * fy).sum(1), rtol=2 * EPS)
        want = {m.L2: nx + ny - 2.0 * ip, m.IP: -ip, m.COSINE: 1.0 - ip / (np.sqrt(nx) * np.sqrt(ny)),
                m.COSINE_NORMALIZED: 1.0 - ip}
        got = {metric: m.distance_matrix(metric, x, y, dim, bits).astype(np.float64) for metric in m.METRICS}
        err = {metric: np.abs(got[metric] - want[metric]) for metric in m.METRICS}
        figures = {m.IP: err[m.IP] / np.abs(want[m.IP]),
                   m.COSINE: err[m.COSINE],
                   m.COSINE_NORMALIZED: err[m.COSINE_NORMALIZED] / np.maximum(np.abs(want[m.COSINE_NORMALIZED]), ip),
                   m.L2: err[m.L2] / (nx + ny)}
        for metric in m.METRICS:
            worst[metric] = max(worst.get(metric, 0.0), float(figures[metric].max()))
        print("bits", bits, "dim", dim, {k: float(v.max()) for k, v in figures.items()})
        assert (figures[m.IP] < 1e-6).all(), (bits, dim)
        assert ((err[m.COSINE] < 1e-6) | (err[m.COSINE] / np.abs(want[m.COSINE]) < 1e-3)).all(), (bits, dim)
        assert (figures[m.COSINE_NORMALIZED] < 1e-6).all(), (bits, dim)
        assert (figures[m.L2] < 1e-6).all(), (bits, dim)
    print("worst figure per metric", bits, worst)


def test_argument_order_matters_on_the_sample():
    """(t0 + x.n * y.b) + y.n * x.b: the two orders differ in the last bit for a few percent of random pairs.  The GPU
    test's order check needs such pairs in ITS sample: same generator, same seed"""
    for bits in m.BITS:
        rows = random_rows(np.random.default_rng(7000 + bits), 96, 100, bits)
        d = m.distance_matrix(m.L2, rows, rows, 100, bits)
        differ = int((fbits(d) != fbits(d.T)).sum())
        assert differ > 20, (bits, differ)
        assert np.array_equal(fbits(np.diag(d)), fbits(np.diag(d.T)))


@pytest.mark.parametrize("bits", m.BITS)
def test_compressor_post_conditions(bits):
    rng = np.random.default_rng(30 + bits)
    top = (1 << bits) - 1
    for dim in (1, 7, 64, 100):
        # the all-equal vector: codes 0, b the value, reconstruction exact up to the 1e-8 floor of the range
        x = np.full((3, dim), 1.5, np.float32)
        rows, loss, nan = m.compress(x, bits)
        _, b, n, a, ns = m.header(rows)
        assert not nan.any() and (m.codes_of(rows, bits, dim) == 0).all() and (b == 1.5).all() and (n == 0).all()
        assert np.allclose(ns, dim * 2.25, rtol=1e-6) and (loss == 0).all()
        assert (m.header(rows)[0] == dim).all()
        if dim == 1:
            continue
        # two distinct values: the smaller maps to code 0, the larger to the top code, nothing in between
        x = np.where(rng.random((5, dim)) < 0.5, np.float32(-2.0), np.float32(3.0)).astype(np.float32)
        x[:, 0], x[:, 1] = -2.0, 3.0
        rows, loss, nan = m.compress(x, bits)
        codes = m.codes_of(rows, bits, dim)
        assert ((codes == 0) == (x == -2.0)).all() and ((codes == top) == (x == 3.0)).all()
        assert np.allclose(m.decompress(rows, bits, dim), x, atol=1e-5)
        # random vectors, grid_scale 1: reconstruction within one grid step (half a step, bits > 1), padding bits zero
        x = rng.normal(0.0, 2.0, (6, dim)).astype(np.float32)
        rows, loss, nan = m.compress(x, bits)
        _, b, n, a, ns = m.header(rows)
        rec = m.decompress(rows, bits, dim)
        step = a.astype(np.float64)[:, None]
        if bits > 1:
            assert (np.abs(rec - x) <= 0.5 * step + 1e-5).all()
        else:  # the 1-bit range is (mean of the values below the mean, mean of the others): the nearer end
            t = (x - b[:, None].astype(np.float64)) / step
            clear = np.abs(t - 0.5) > 1e-4
            assert ((m.codes_of(rows, bits, dim) == 1) == (t >= 0.5))[clear].all()
            assert (b <= x.mean(1) + 1e-5).all() and (b + a >= x.mean(1) - 1e-5).all()
        assert np.allclose(loss, ((rec - x) ** 2).sum(1), rtol=1e-4, atol=1e-6)
        assert np.allclose(ns, (rec * rec).sum(1), rtol=1e-5) and np.allclose(n, a * m.codes_of(rows, bits, dim).sum(1), rtol=1e-6)
        assert np.array_equal(m.pack(m.codes_of(rows, bits, dim), bits), rows[:, m.HEADER:])
        # grid_scale 0.9 narrows the range: the extremes clamp to the end codes
        rows9, _, _ = m.compress(x, bits, 0.9)
        c9 = m.codes_of(rows9, bits, dim)
        if bits > 1:
            assert (c9[np.arange(6), x.argmin(1)] == 0).all() and (c9[np.arange(6), x.argmax(1)] == top).all()
            assert (m.header(rows9)[3] < a).all()
    x = np.ones((2, 8), np.float32)
    x[1, 3] = np.nan
    _, _, nan = m.compress(x, bits)
    assert nan.tolist() == [False, True]


def test_twin_is_exact_in_both_orders():
    rng = np.random.default_rng(50)
    for bits, dim, hi in ((1, 128, 2), (2, 100, 4), (4, 64, 16), (8, 129, 256), (8, 260, 180), (8, 32, 256)):
        codes = rng.integers(0, hi, (20, dim), dtype=np.uint8)
        rows = m.twin_rows(codes, bits)
        d = m.distance_matrix(m.L2, rows, rows, dim, bits)
        want = np.array([[oracle.distance(oracle.U8, oracle.L2, codes[i], codes[j]) for j in range(20)] for i in range(20)],
                        np.float32)
        assert np.array_equal(fbits(d), fbits(want)) and np.array_equal(fbits(d.T), fbits(want)), (bits, dim)
    with pytest.raises(AssertionError):
        m.twin_rows(np.full((1, 130), 255, np.uint8), 8)  # 2 * 255^2 * 130 >= 2^24


def test_image_layout():
    codes = np.array([[1, 0, 1, 1, 0, 0, 0, 1, 1]], np.uint8)
    row = m.make_rows(codes, 1, [0.5], [2.0], [0.25], [9.0])[0]
    assert row.size == m.layer_bytes(1, 9) == 22
    assert row[:4].view(np.uint32)[0] == 9 and row[4:20].view(np.float32).tolist() == [0.5, 2.0, 0.25, 9.0]
    assert row[20:].tolist() == [0b10001101, 0b1]
    assert m.layer_bytes(8, 128) == 148 and m.layer_bytes(4, 7) == 24 and m.store_stride(8, 128) == 160
    assert np.array_equal(m.codes_of(m.make_rows(np.arange(16, dtype=np.uint8)[None] % 4, 2, [0], [0], [1], [0]), 2, 16)[0],
                          np.arange(16) % 4)
