"""tests/transform_model.py pinned without a GPU: the structure of hadamard_v3 on integers (where every order is exact),
its accuracy against a float64 matrix product, that its ORDER is the micro kernel's and not the plain butterfly's, and
the two transforms against their matrix formulas (double_hadamard.rs:33-36).

The error bound: a butterfly stage rounds once per element, and with relative roundings of at most u = 2^-24 a stage
keeps the error in the 2-norm sense (the stage is sqrt(2) times an orthogonal map), so log2(n) stages cost at most
log2(n) u |x|_2 in any coordinate of the scaled result; the micro kernel's chain rounds seven times where the three
butterfly stages it replaces round three times (+4), the multiplication by m rounds once and m itself carries up to two
roundings (+3): (log2 n + 8) u |x|_2, with one to spare."""
import numpy as np
import pytest

import transform_model as tm

U = 2.0 ** -24
LENGTHS = [1 << p for p in range(11)]


def sylvester(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def bound(n):
    return (np.log2(n) + 8) * U


def signs(rng, n):
    return (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)).astype(np.uint32)


def sgn(s):
    return np.where(np.asarray(s) != 0, -1.0, 1.0)


def test_s_is_the_sylvester_h8():
    assert np.array_equal(tm.S8, sylvester(8).astype(np.float32))
    assert np.array_equal(tm.S8, tm.S8.T)


@pytest.mark.parametrize("n", LENGTHS)
def test_structure_on_integers(n):
    x = np.random.default_rng(n).integers(-999, 1000, (16, n))
    want = x @ sylvester(n).astype(np.int64)
    assert np.abs(want).max() < 1 << 24  # every partial sum is an integer an f32 holds: any order is exact
    for f in (tm.hadamard_v3, tm.hadamard_plain):
        got = f(x.astype(np.float32), scale=False)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want), f.__name__
    scaled = tm.hadamard_v3(x.astype(np.float32))
    m = np.float32(1.0) / np.sqrt(np.float32(n))
    assert np.array_equal(scaled, want.astype(np.float32) * m if n > 1 else want.astype(np.float32))


@pytest.mark.parametrize("n", LENGTHS)
def test_accuracy_against_f64(n):
    x = np.random.default_rng(100 + n).standard_normal((20, n)).astype(np.float32)
    want = x.astype(np.float64) @ sylvester(n) / np.sqrt(n)
    err = np.abs(tm.hadamard_v3(x).astype(np.float64) - want).max(axis=1)
    norm = np.linalg.norm(x.astype(np.float64), axis=1)
    print(n, (err / (U * norm)).max())
    assert (err <= bound(n) * norm).all(), (err / (U * norm)).max()


@pytest.mark.parametrize("n", LENGTHS)
def test_the_order_is_pinned(n):
    x = np.random.default_rng(0).standard_normal((20, n)).astype(np.float32)
    a, b = tm.hadamard_v3(x).view(np.uint32), tm.hadamard_plain(x).view(np.uint32)
    differ = int((a != b).sum())
    print(n, differ, a.size)
    if n < 64:
        assert differ == 0
    else:
        assert 2 * differ > a.size, (differ, a.size)  # the 8-term chain is not three butterfly stages
        assert np.abs(a.astype(np.int64) - b.astype(np.int64))[a != b].max() < 1 << 16  # (but the same numbers)


def test_signed_zero_and_length_one():
    z = np.full((1, 64), -0.0, np.float32)
    assert not np.signbit(tm.hadamard_v3(z)[0, 0])  # the chain starts from +0.0: +0.0 + -0.0 = +0.0
    assert np.signbit(tm.hadamard_plain(np.full((1, 8), -0.0, np.float32))[0, 0])  # -0.0 + -0.0 = -0.0
    one = np.array([[3.5]], np.float32)
    assert np.array_equal(tm.hadamard_v3(one), one)  # not even the scaling


PADDING = [(1, 1), (5, 8), (63, 64), (64, 64), (65, 128), (100, 128), (128, 128), (129, 256), (768, 1024)]


@pytest.mark.parametrize("dim,padded", PADDING)
@pytest.mark.parametrize("sub", [False, True])
def test_padding_hadamard_against_its_matrix(dim, padded, sub):
    rng = np.random.default_rng(dim * 2 + sub)
    s = signs(rng, dim)
    idx = np.sort(rng.choice(padded, dim, replace=False)).astype(np.uint32) if sub else None
    x = rng.standard_normal((20, dim)).astype(np.float32)
    got = tm.padding_hadamard(x, s, padded, idx)
    z = np.zeros((20, padded))
    z[:, :dim] = x * sgn(s)
    want = z @ sylvester(padded) / np.sqrt(padded)
    scale = 1.0
    if sub:
        scale = np.sqrt(padded / dim)
        want = want[:, idx] * scale
    assert got.shape == want.shape and got.dtype == np.float32
    norm = np.linalg.norm(x.astype(np.float64), axis=1)
    # subsampled: the product with rescale rounds once more and rescale carries two roundings (+3)
    assert (np.abs(got - want).max(axis=1) <= scale * (bound(padded) + 3 * U * sub) * norm).all()


# (input_dim, output_dim): equal (64 and 128: the intermediate length is a power of two and both transforms still run),
# larger (zero padding), smaller (subsample)
DOUBLE = [(1, 1), (2, 2), (3, 3), (5, 5), (63, 63), (64, 64), (65, 65), (96, 96), (100, 100), (128, 128), (129, 129),
          (200, 200), (768, 768), (1000, 1000), (100, 128), (100, 150), (768, 512), (100, 64)]


@pytest.mark.parametrize("dim,out", DOUBLE)
def test_double_hadamard_against_its_matrix(dim, out):
    rng = np.random.default_rng(dim * 1000 + out)
    o = max(dim, out)
    t = 1 << (o.bit_length() - 1)
    s0, s1 = signs(rng, dim), signs(rng, o)
    idx = np.sort(rng.choice(dim, out, replace=False)).astype(np.uint32) if out < dim else None
    x = rng.standard_normal((20, dim)).astype(np.float32)
    got = tm.double_hadamard(x, s0, s1, idx)
    z = np.zeros((20, o))
    z[:, :dim] = x * sgn(s0)
    h = sylvester(t) / np.sqrt(t)
    z[:, :t] = z[:, :t] @ h
    z *= sgn(s1)
    z[:, o - t:] = z[:, o - t:] @ h
    scale = 1.0
    if idx is not None:
        scale = np.sqrt(o / out)
        z = z[:, idx] * scale
    assert got.shape == z.shape == (20, out) and got.dtype == np.float32
    norm = np.linalg.norm(x.astype(np.float64), axis=1)
    # two Hadamards, each within the bound (both keep the norm)
    assert (np.abs(got - z).max(axis=1) <= scale * (2 * bound(t) + 3 * U * (idx is not None)) * norm).all()
    if o == t and t >= 2:  # follow the code, not its comment: a single transform would be something else
        once = tm.padding_hadamard(x, s0, t)
        assert not np.array_equal(got, once)


def test_null_is_a_copy():
    x = np.random.default_rng(1).standard_normal((3, 7)).astype(np.float32)
    assert np.array_equal(tm.null(x), x)
