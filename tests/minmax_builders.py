"""Index builders of the MinMax tests (tests/test_gpu_minmax.py, tests/test_minmax_model_host.py): random row images,
compressed rows under a random graph, and the exact twin of the oracle's U8 L2 index (minmax_model.twin_rows)."""
import numpy as np

import minmax_model as mm
import oracle
from helpers import random_graph


def _da():
    import diskann_amd
    return diskann_amd


def mm_dtype(bits):
    return 48 + bits


def random_rows(rng, n, dim, bits, garbage=False):
    """as the reference's unit test draws them (minmax/vectors.rs:567-590): uniform codes, a and b uniform in [0, 2]; n
    and norm_squared follow from them.  garbage: random bits in the padding of the last code byte"""
    codes = rng.integers(0, 1 << bits, (n, dim), dtype=np.uint8)
    a = rng.uniform(0.0, 2.0, n).astype(np.float32)
    b = rng.uniform(0.0, 2.0, n).astype(np.float32)
    c = codes.astype(np.float64)
    nn = (a.astype(np.float64) * c.sum(1)).astype(np.float32)
    v = a.astype(np.float64)[:, None] * c + b.astype(np.float64)[:, None]
    rows = mm.make_rows(codes, bits, b, nn, a, (v * v).sum(1).astype(np.float32))
    used = dim * bits - 8 * (mm.code_bytes(bits, dim) - 1)
    if garbage and used < 8:
        rows[:, -1] |= (rng.integers(0, 256, n, dtype=np.uint8) << used).astype(np.uint8)
    return rows


class MmModelCase:
    """rows compressed by the model's MinMaxQuantizer from normal data, under a random graph; the GPU provider over them"""

    def __init__(self, bits, metric, n, dim, R, seed, tags=False, nstart=1):
        rng = np.random.default_rng(seed)
        self.bits, self.metric, self.n, self.dim, self.R, self.rng, self.nstart = bits, metric, n, dim, R, rng, nstart
        data = rng.normal(0.2, 1.0, (n + nstart, dim)).astype(np.float32)
        self.all_rows, _, _ = mm.compress(data, bits, 0.95)
        self.adj = random_graph(rng, n, R, nstart=nstart)
        da = _da()
        dt = mm_dtype(bits)
        stride = da.lib().dann_inmem2_row_stride(dt, dim) if tags else 0
        self.gix = da.Provider(dt, metric, dim, n, R, self.all_rows[n:], row_stride=stride, inline_tags=tags)
        self.gix.set_elements(0, self.all_rows[:n])
        self.gix.upload_graph(self.adj)

    def queries(self, nq):
        q, _, _ = mm.compress(self.rng.normal(0.2, 1.0, (nq, self.dim)).astype(np.float32), self.bits, 0.95)
        return q


class MmTwin:
    """twin rows (a = 1, b = 0: L2 is exactly the squared distance of the codes) and the oracle's U8 L2 index over the
    codes.  hi: codes drawn from [0, hi) -- the twin needs 2 * (hi - 1)^2 * dim < 2^24"""

    def __init__(self, bits, dim, n, R, seed, adj=True, maxdeg=None, nstart=1, hi=None, gpu=True):
        rng = np.random.default_rng(seed)
        self.bits, self.dim, self.n, self.R, self.rng, self.nstart = bits, dim, n, R, rng, nstart
        self.hi = hi or (1 << bits)
        self.codes = rng.integers(0, self.hi, (n, dim), dtype=np.uint8)
        self.rows = mm.twin_rows(self.codes, bits)
        self.scodes = rng.integers(0, self.hi, (nstart, dim), dtype=np.uint8)
        self.adj = random_graph(rng, n, R, nstart=nstart) if adj else None
        self.maxdeg = maxdeg or R
        self.oix = oracle.Index(oracle.U8, oracle.L2, dim, n, self.maxdeg, self.scodes)
        self.oix.set_rows(0, self.codes)
        if adj:
            self.oix.adj[:] = self.adj
        self.gix = None
        if gpu:
            self.attach_gpu()

    def attach_gpu(self):
        da = _da()
        self.gix = da.Provider(mm_dtype(self.bits), da.L2, self.dim, self.n, self.maxdeg, mm.twin_rows(self.scodes, self.bits))
        self.gix.set_elements(0, self.rows)
        if self.adj is not None:
            self.gix.upload_graph(self.adj)
        return self.gix

    def queries(self, nq):
        qc = self.rng.integers(0, self.hi, (nq, self.dim), dtype=np.uint8)
        return mm.twin_rows(qc, self.bits), qc
