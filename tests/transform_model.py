"""CPU model of the quantisers' transforms (diskann-quantization/src/algorithms/hadamard.rs and transforms/): every
f32 operation on its own and in the order of the reference's x86-64 V3 path.  numpy only; rows are transformed side by
side, (rows, len) in and out.

hadamard_v3 (hadamard.rs:22-371), len a power of two:
    len == 1    nothing, not even the scaling
    len <  64   in-place butterflies (l, r) -> (l + r, l - r) at strides 1, 2, 4 .. len / 2 (the recursion at :194-227)
    len >= 64   every aligned block of 64 goes through micro_kernel_64 (:248-371): for each sub-block a of eight elements
                d[a][j] = (((+0.0 + s(0,j) x[8a]) + s(1,j) x[8a+1]) + ..) + s(7,j) x[8a+7], s(k,j) = (-1)^popcount(k & j)
                -- an FMA chain whose products are exact, so one rounding per addition, k ascending -- then butterflies at
                strides 8, 16, 32 inside the block and 64 .. len / 2 over the vector.  Strides 1, 2, 4 are NOT butterflies
                there: an eight-term sequential sum.
    then every element times m = 1 / sqrt((f32)len), both correctly rounded.
hadamard_plain is the butterfly form at every length: kept only to show that the two differ in the last bit.

padding_hadamard (padding_hadamard.rs:204-273), double_hadamard (double_hadamard.rs:238-287, as its code runs: both
transforms run even when the intermediate length is a power of two, and otherwise the two windows overlap) and null.

This is a restatement from reading the reference; the reference holds no golden vector for its transforms."""
import numpy as np

f32 = np.float32
SIGN = np.uint32(0x80000000)
S8 = np.array([[-1.0 if bin(k & j).count("1") & 1 else 1.0 for j in range(8)] for k in range(8)], np.float32)


def _butterfly(v, s):
    """in place, stride s, on a contiguous (rows, len) array"""
    rows, n = v.shape
    w = v.reshape(rows, n // (2 * s), 2, s)
    l, r = w[:, :, 0, :].copy(), w[:, :, 1, :].copy()
    w[:, :, 0, :] = l + r
    w[:, :, 1, :] = l - r


def _scale(v):
    return v * (f32(1.0) / np.sqrt(f32(v.shape[1])))


def _check(x):
    v = np.array(x, dtype=np.float32, ndmin=2, order="C")  # (a copy)
    n = v.shape[1]
    assert n >= 1 and n & (n - 1) == 0, n
    return v, n


def hadamard_plain(x, scale=True):
    v, n = _check(x)
    if n == 1:
        return v
    s = 1
    while s < n:
        _butterfly(v, s)
        s *= 2
    return _scale(v) if scale else v


def hadamard_v3(x, scale=True):
    v, n = _check(x)
    if n < 64:
        return hadamard_plain(v, scale)
    w = v.reshape(v.shape[0], n // 8, 8)
    d = np.zeros_like(w)  # +0.0
    for k in range(8):
        d = d + S8[k][None, None, :] * w[:, :, k:k + 1]
    v = np.ascontiguousarray(d.reshape(v.shape[0], n))
    s = 8
    while s < n:
        _butterfly(v, s)
        s *= 2
    return _scale(v) if scale else v


def _signs(s):
    s = np.ascontiguousarray(s, dtype=np.uint32).reshape(-1)
    assert np.all((s == 0) | (s == SIGN))
    return s


def _flip(x, signs):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) ^ signs[None, :]).view(np.float32)


def _finish(tmp, subsample):
    if subsample is None:
        return tmp
    idx = np.asarray(subsample, dtype=np.int64)
    rescale = np.sqrt(f32(tmp.shape[1]) / f32(idx.size))
    assert rescale.dtype == np.float32
    return tmp[:, idx] * rescale


def null(x):
    return np.array(x, dtype=np.float32, ndmin=2)


def padding_hadamard(x, signs, padded_dim, subsample=None, hadamard=hadamard_v3):
    signs = _signs(signs)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, signs.size)
    tmp = np.zeros((x.shape[0], padded_dim), np.float32)
    tmp[:, :signs.size] = _flip(x, signs)
    return _finish(hadamard(tmp), subsample)


def double_hadamard(x, signs0, signs1, subsample=None, hadamard=hadamard_v3):
    signs0, signs1 = _signs(signs0), _signs(signs1)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, signs0.size)
    out_dim = signs1.size if subsample is None else len(subsample)
    o = max(signs0.size, out_dim)
    t = 1 << (o.bit_length() - 1)
    tmp = np.zeros((x.shape[0], o), np.float32)
    tmp[:, :signs0.size] = _flip(x, signs0)
    tmp[:, :t] = hadamard(tmp[:, :t])
    m = min(o, signs1.size)
    tmp[:, :m] = _flip(tmp[:, :m], signs1[:m])
    tmp[:, o - t:] = hadamard(tmp[:, o - t:])
    return _finish(tmp, subsample)
