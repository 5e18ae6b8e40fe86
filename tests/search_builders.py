"""Index builders shared by the GPU test modules and tests/search_matrix.py: the same bytes under the oracle (or its twin,
or the CPU model) and under the HIP library.  Everything up to `attach_gpu()` runs without a GPU when the rows are
compressed on the CPU (`compress=` / the spherical model's own compressor); `gpu=True`, the default, is what the GPU test
modules use."""
import ctypes as C

import numpy as np

import oracle
import spherical_model as sph
import sq_bits_model as sqm
from helpers import random_graph


def _da():
    import diskann_amd as da
    return da


def sq_dtype(bits):
    da = _da()
    return {1: da.SQ1, 4: da.SQ4, 8: da.SQ8}[bits]


def sph_dtype(bits):
    da = _da()
    return {1: da.SPH1, 2: da.SPH2, 4: da.SPH4}[bits]


def orc_sq8_compress(x, shift, scale):
    """the oracle's SQ-8 compressor, row by row: code bytes + the f32 compensation"""
    L = oracle.lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    shift = np.ascontiguousarray(shift, dtype=np.float32)
    out = np.zeros((x.shape[0], x.shape[1] + 4), np.uint8)
    for i in range(x.shape[0]):
        c = np.zeros(1, np.float32)
        L.orc_sq8_compress(x[i].ctypes.data, x.shape[1], shift.ctypes.data, C.c_float(scale),
                           out[i].ctypes.data, c.ctypes.data)
        out[i, x.shape[1]:] = c.view(np.uint8)
    return out


def sq_setup(rng, n, dim):
    """rows and ScalarQuantizer parameters as train.rs would produce them: shift = mean - 2 std, scale = 4 std"""
    data = rng.normal(0.3, 0.5, (n, dim)).astype(np.float32)
    shift = (data.mean(0) - 2.0 * data.std(0)).astype(np.float32)
    scale = float(np.float32(4.0 * data.std()))
    snorm = float(np.float32((shift ** 2).sum(dtype=np.float32)))
    return data, shift, scale, snorm


def _start_rows(data, nstart):
    """the mean row, then the first rows of the data: `nstart` start points"""
    return np.concatenate([data.mean(0, keepdims=True).astype(np.float32), data[:nstart - 1]])


class SqBitsCase:
    """SQ4 / SQ1 (and, for the matrix, SQ8) rows: compressed rows, the GPU provider and the oracle's SQ-8 twin (same
    integer sums, matched scale: identical distance bits).  compress(x, shift, scale, bits): the library's by default"""

    def __init__(self, bits, metric, n, dim, R, seed, adj=True, maxdeg=None, tags=False, nstart=1, compress=None, gpu=True):
        rng = np.random.default_rng(seed)
        if compress is None:
            compress = _da().sq_compress
        self.bits, self.metric, self.n, self.dim, self.R, self.nstart = bits, metric, n, dim, R, nstart
        data, self.shift, scale, self.snorm = sq_setup(rng, n, dim)
        self.data = data
        self.scale, self.scale8 = sqm.matched_scale8(bits, scale) if bits != 8 else (scale, scale)
        self.compress = compress
        self.rows = compress(data, self.shift, self.scale, bits)
        self.start = compress(_start_rows(data, nstart), self.shift, self.scale, bits)
        self.adj = random_graph(rng, n, R, nstart=nstart) if adj else None
        self.maxdeg = maxdeg or R
        self.tags = tags
        self.oix = sqm.oracle_twin(metric, dim, n, self.maxdeg, bits, self.rows, self.start, self.scale8, self.snorm, self.adj)
        self.rng = rng
        self.gix = None
        if gpu:
            self.attach_gpu()

    def attach_gpu(self):
        # tags: the Store layout on the GPU side (stride of the reference, a tag byte after the payload); every slot is
        # published, so the twin without tags returns the same results
        da = _da()
        dt = sq_dtype(self.bits)
        stride = da.lib().dann_inmem2_row_stride(dt, self.dim) if self.tags else 0
        self.gix = da.Provider(dt, self.metric, self.dim, self.n, self.maxdeg, self.start, sq_scale=self.scale,
                               sq_shift_norm_sq=self.snorm, row_stride=stride, inline_tags=self.tags)
        self.gix.set_elements(0, self.rows)
        if self.adj is not None:
            self.gix.upload_graph(self.adj)
        return self.gix

    def queries(self, nq):
        qf = self.rng.normal(0.3, 0.5, (nq, self.dim)).astype(np.float32)
        q = self.compress(qf, self.shift, self.scale, self.bits)
        return qf, q, sqm.twin_rows(q, self.bits, self.dim)


class SphModelCase:
    """realistic spherically quantised rows (the model's compressor) under a random graph, the GPU provider over them"""

    def __init__(self, bits, metric, n, dim, R, seed, tags=False, nstart=1, gpu=True):
        rng = np.random.default_rng(seed)
        self.bits, self.metric, self.n, self.dim, self.R, self.rng, self.nstart = bits, metric, n, dim, R, rng, nstart
        self.data = rng.normal(0.2, 1.0, (n, dim)).astype(np.float32)
        self.qz = sph.Quantizer(self.data, bits, metric)
        self.rows = self.qz.rows(self.data)
        self.start = self.qz.rows(_start_rows(self.data, nstart))
        self.adj = random_graph(rng, n, R, nstart=nstart)
        self.tags = tags
        self.all_rows = np.concatenate([self.rows, self.start])
        self.gix = None
        if gpu:
            self.attach_gpu()

    def attach_gpu(self):
        da = _da()
        dt = sph_dtype(self.bits)
        stride = da.lib().dann_inmem2_row_stride(dt, self.dim) if self.tags else 0
        self.gix = da.Provider(dt, self.metric, self.dim, self.n, self.R, self.start, sq_shift_norm_sq=self.qz.ssn,
                               row_stride=stride, inline_tags=self.tags)
        self.gix.set_elements(0, self.rows)
        self.gix.upload_graph(self.adj)
        return self.gix


class SphTwin:
    """flat spherical rows (rows whose L2 is exactly the squared distance of their codes) and the oracle's U8 L2 twin.
    code_range (lo, hi): codes drawn from [lo, hi) -- flat rows need sum((code - offset)^2) exact in f16, which 4-bit codes
    of more than some 36 dimensions only are when they stay near the middle of the grid"""

    def __init__(self, bits, dim, n, R, seed, adj=True, maxdeg=None, nstart=1, tags=False, gpu=True, code_range=None):
        rng = np.random.default_rng(seed)
        self.bits, self.dim, self.n, self.R, self.rng, self.nstart = bits, dim, n, R, rng, nstart
        self.lo, self.hi = code_range or (0, 1 << bits)
        self.codes = rng.integers(self.lo, self.hi, (n, dim), dtype=np.uint8)
        self.rows = sph.flat_rows(self.codes, bits)
        self.scodes = rng.integers(self.lo, self.hi, (nstart, dim), dtype=np.uint8)
        self.adj = random_graph(rng, n, R, nstart=nstart) if adj else None
        self.maxdeg = maxdeg or R
        self.tags = tags
        self.oix = oracle.Index(oracle.U8, oracle.L2, dim, n, self.maxdeg, self.scodes)
        self.oix.set_rows(0, self.codes)
        if adj:
            self.oix.adj[:] = self.adj
        self.gix = None
        if gpu:
            self.attach_gpu()

    def attach_gpu(self):
        da = _da()
        dt = sph_dtype(self.bits)
        stride = da.lib().dann_inmem2_row_stride(dt, self.dim) if self.tags else 0
        self.gix = da.Provider(dt, da.L2, self.dim, self.n, self.maxdeg, sph.flat_rows(self.scodes, self.bits),
                               row_stride=stride, inline_tags=self.tags)
        self.gix.set_elements(0, self.rows)
        if self.adj is not None:
            self.gix.upload_graph(self.adj)
        return self.gix

    def queries(self, nq):
        qc = self.rng.integers(self.lo, self.hi, (nq, self.dim), dtype=np.uint8)
        return sph.flat_rows(qc, self.bits), qc
