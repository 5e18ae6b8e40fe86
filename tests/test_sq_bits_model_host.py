"""The CPU model of SQ4 / SQ1 rows (tests/sq_bits_model.py), pinned to the oracle at 8 bits, and the row layout the
library reports for the packed types.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle
import sq_bits_model as m

METRICS = (oracle.L2, oracle.INNER_PRODUCT, oracle.COSINE_NORMALIZED)


def _setup(rng, n, dim):
    data = rng.normal(0.3, 0.5, (n, dim)).astype(np.float32)
    shift = (data.mean(0) - 2.0 * data.std(0)).astype(np.float32)
    scale = float(np.float32(4.0 * data.std()))
    snorm = float(np.float32((shift ** 2).sum(dtype=np.float32)))
    return data, shift, scale, snorm


def _orc_distance(metric, x, y, dim, scale, snorm):
    L = oracle.lib()
    want = L.orc_sq8_distance(metric if metric != oracle.COSINE_NORMALIZED else oracle.L2, x.ctypes.data,
                              C.c_float(x[dim:].view(np.float32)[0]), y.ctypes.data,
                              C.c_float(y[dim:].view(np.float32)[0]), dim, C.c_float(scale), C.c_float(snorm))
    if metric == oracle.COSINE_NORMALIZED:
        want = np.float32(1.0) - (np.float32(1.0) - np.float32(want) / np.float32(2.0))
    return np.float32(want)


def test_model_at_8_bits_is_the_oracle():
    rng = np.random.default_rng(1)
    L = oracle.lib()
    for dim in (7, 33, 128):
        data, shift, scale, snorm = _setup(rng, 40, dim)
        data[3, 0], data[4, 1] = 1e9, -1e9
        got = m.compress(data, shift, scale, 8)
        want = np.zeros((40, dim + 4), np.uint8)
        for i in range(40):
            c = np.zeros(1, np.float32)
            L.orc_sq8_compress(data[i].ctypes.data, dim, shift.ctypes.data, C.c_float(scale), want[i].ctypes.data,
                               c.ctypes.data)
            want[i, dim:] = c.view(np.uint8)
        assert np.array_equal(got, want), dim
        for metric in METRICS:
            for i in range(0, 40, 2):
                d = m.distance(metric, got[i], got[i + 1], dim, 8, scale, snorm)
                assert d.view(np.uint32) == _orc_distance(metric, got[i], got[i + 1], dim, scale, snorm).view(np.uint32)


def test_packing_known_answer():
    # scalar/vectors.rs:128-151: the 4-bit values 1, 2, 3, 4 are the bytes 0x21 0x43
    assert m.pack(np.array([1, 2, 3, 4], np.uint8), 4).tolist() == [0x21, 0x43]
    assert m.pack(np.array([1, 2, 3], np.uint8), 4).tolist() == [0x21, 0x03]           # padding bits zero
    assert m.pack(np.array([1, 0, 0, 1, 0, 0, 0, 0, 1], np.uint8), 1).tolist() == [0x09, 0x01]
    rng = np.random.default_rng(2)
    for bits in (1, 4, 8):
        for dim in (1, 7, 8, 9, 33):
            c = rng.integers(0, 1 << bits, (5, dim), dtype=np.uint8)
            p = m.pack(c, bits)
            assert p.shape == (5, m.code_bytes(bits, dim))
            assert np.array_equal(m.unpack(p, bits, dim), c)


@pytest.mark.parametrize("bits", [1, 4])
def test_twin_equals_the_model(bits):
    """orc_sq8_distance on unpacked codes with the matched scale == the low-bit formula, bit for bit"""
    rng = np.random.default_rng(3 + bits)
    for dim in (7, 33, 128):
        data, shift, scale, snorm = _setup(rng, 60, dim)
        scale, scale8 = m.matched_scale8(bits, scale)
        assert m.k_const(8, scale8) == m.k_const(bits, scale)
        rows = m.compress(data, shift, scale, bits)
        tw = m.twin_rows(rows, bits, dim)
        for metric in METRICS:
            for i in range(0, 60, 2):
                d = m.distance(metric, rows[i], rows[i + 1], dim, bits, scale, snorm)
                w = _orc_distance(metric, tw[i], tw[i + 1], dim, scale8, snorm)
                assert d.view(np.uint32) == w.view(np.uint32), (dim, metric, i)


def test_library_layout_of_packed_rows():
    import diskann_amd as da
    L = da.lib()
    assert (da.SQ1, da.SQ4) == (17, 20)
    assert L.dann_layer_bytes(da.SQ4, 128) == 68 and L.dann_inmem2_row_stride(da.SQ4, 128) == 96
    assert L.dann_layer_bytes(da.SQ1, 100) == 17 and L.dann_inmem2_row_stride(da.SQ1, 100) == 32
    for bits, dt in ((1, da.SQ1), (4, da.SQ4)):
        for dim in (1, 7, 8, 9, 128, 1025):
            assert L.dann_layer_bytes(dt, dim) == m.layer_bytes(bits, dim)
    assert L.dann_layer_bytes(7, 4) == da._ffi.EINVAL      # 7 stays an invalid dtype, 6 unassigned
    assert L.dann_layer_bytes(6, 4) == da._ffi.EINVAL
    assert L.dann_layer_bytes(16, 4) == da._ffi.EINVAL and L.dann_layer_bytes(24, 4) == da._ffi.EINVAL
