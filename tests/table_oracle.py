"""Builders of the quantised-row mutation tests (tests/test_gpu_quant_mutations.py): the GPU Provider over the byte images
of MinMax / spherical rows, and the oracle's distance-table index (oracle.TABLE) over T, the numpy model's distance of
every row image (stored slots, start points in their slots, then the queries) as the FIRST argument against every stored
slot as the second.  The oracle then runs its own prune / insert / search on exactly the distances the kernels must
produce, under every metric the row type has.  Everything up to attach_gpu() runs without a GPU."""
import numpy as np

import minmax_model as mm
import oracle
import spherical_model as sph
from helpers import random_graph
from minmax_builders import mm_dtype, random_rows
from search_builders import _start_rows, sph_dtype


def _da():
    import diskann_amd
    return diskann_amd


def tie_rich_rows(rng, n, dim, bits, classes=4, distinct=20):
    """order-sensitive MinMax rows: `classes` header classes (a in [0.25, 2], b in [-1, 2]) over `distinct` code rows
    (0: every code row its own), n and norm_squared derived from them as random_rows derives them.  Many candidate pairs
    then sit exactly on RobustPrune's comparisons, where the last bit of the asymmetric epilogue decides."""
    base = rng.integers(0, 1 << bits, (distinct or n, dim), dtype=np.uint8)
    codes = base[rng.integers(0, base.shape[0], n)] if distinct else base
    ca = rng.uniform(0.25, 2.0, classes).astype(np.float32)
    cb = rng.uniform(-1.0, 2.0, classes).astype(np.float32)
    k = rng.integers(0, classes, n)
    a, b = ca[k], cb[k]
    c = codes.astype(np.float64)
    nn = (a.astype(np.float64) * c.sum(1)).astype(np.float32)
    v = a.astype(np.float64)[:, None] * c + b.astype(np.float64)[:, None]
    ns = (v * v).sum(1).astype(np.float32)
    assert (ns > 0).all()
    return mm.make_rows(codes, bits, b, nn, a, ns)


class TableCase:
    """all_rows: (n + nstart) images, the start points last; queries: nq more images; T: (n + nstart + nq, n + nstart)"""

    def _finish(self, metric, n, nstart, maxdeg, all_rows, queries, T, adj, gpu):
        self.metric, self.n, self.nstart, self.maxdeg = metric, n, nstart, maxdeg
        self.all_rows, self.query_rows, self.T, self.adj = all_rows, queries, np.ascontiguousarray(T, dtype=np.float32), adj
        assert self.T.shape == (n + nstart + queries.shape[0], n + nstart) and np.isfinite(self.T).all()
        self.oix = self.table_index(self.T)
        self.gix = None
        if gpu:
            self.attach_gpu()

    def table_index(self, T):
        """a fresh table oracle over T (or over a variant of it, such as the transpose of its square part)"""
        oix = oracle.Index(oracle.TABLE, self.metric, 1, self.n, self.maxdeg, np.zeros(self.nstart), table=T)
        if self.adj is not None:
            oix.adj[:] = self.adj
        return oix

    def transposed(self):
        """T with its slot x slot part transposed: what a kernel that swapped (x, y) would compute"""
        ns = self.n + self.nstart
        Tt = self.T.copy()
        Tt[:ns] = self.T[:ns].T
        return Tt

    def attach_gpu(self):
        self.gix = self._provider()
        self.gix.set_elements(0, self.all_rows[:self.n])
        if self.adj is not None:
            self.gix.upload_graph(self.adj)
        return self.gix

    def query_key(self, j):
        return np.array([self.n + self.nstart + j], np.uint32)


class MmTableCase(TableCase):
    """MinMax rows: rows="model" compressed by the model's compressor from normal data (as MmModelCase), "reference" the
    reference's own draw (minmax_builders.random_rows), "ties" tie_rich_rows"""

    def __init__(self, bits, metric, n, dim, R, seed, rows="model", adj=True, maxdeg=None, nstart=1, nq=0, gpu=True,
                 classes=4, distinct=20):
        rng = np.random.default_rng(seed)
        self.bits, self.dim, self.R, self.rng = bits, dim, R, rng
        total = n + nstart + nq
        if rows == "model":
            images, _, _ = mm.compress(rng.normal(0.2, 1.0, (total, dim)).astype(np.float32), bits, 0.95)
        elif rows == "reference":
            images = random_rows(rng, total, dim, bits)
        else:
            images = tie_rich_rows(rng, total, dim, bits, classes, distinct)
        _, _, _, _, ns = mm.header(images)
        assert (ns > 0).all()
        graph = random_graph(rng, n, R, nstart=nstart) if adj else None
        maxdeg = maxdeg or R
        if graph is not None and maxdeg != R:
            graph = np.pad(graph, ((0, 0), (0, maxdeg - R)))
        T = mm.distance_matrix(metric, images, images[:n + nstart], dim, bits)
        self._finish(metric, n, nstart, maxdeg, images[:n + nstart], images[n + nstart:], T, graph, gpu)

    def _provider(self):
        da = _da()
        return da.Provider(mm_dtype(self.bits), self.metric, self.dim, self.n, self.maxdeg, self.all_rows[self.n:])


class SphTableCase(TableCase):
    """spherically quantised rows from the model's Quantizer (as SphModelCase), row x row distances (SAME_AS_DATA)"""

    def __init__(self, bits, metric, n, dim, R, seed, adj=True, maxdeg=None, nstart=1, nq=0, gpu=True):
        rng = np.random.default_rng(seed)
        self.bits, self.dim, self.R, self.rng = bits, dim, R, rng
        data = rng.normal(0.2, 1.0, (n, dim)).astype(np.float32)
        self.qz = sph.Quantizer(data, bits, metric)
        images = np.concatenate([self.qz.rows(data), self.qz.rows(_start_rows(data, nstart))])
        if nq:
            images = np.concatenate([images, self.qz.rows(rng.normal(0.2, 1.0, (nq, dim)).astype(np.float32))])
        graph = random_graph(rng, n, R, nstart=nstart) if adj else None
        maxdeg = maxdeg or R
        if graph is not None and maxdeg != R:
            graph = np.pad(graph, ((0, 0), (0, maxdeg - R)))
        T = sph.distance_matrix(metric, images, images[:n + nstart], dim, bits, sph.SAME_AS_DATA, ssn=self.qz.ssn)
        self._finish(metric, n, nstart, maxdeg, images[:n + nstart], images[n + nstart:], T, graph, gpu)

    def _provider(self):
        da = _da()
        return da.Provider(sph_dtype(self.bits), self.metric, self.dim, self.n, self.maxdeg, self.all_rows[self.n:],
                           sq_shift_norm_sq=self.qz.ssn)
