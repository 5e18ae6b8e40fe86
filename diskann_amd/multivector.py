"""Multi-vector (late-interaction) scoring: dann_mvset + dann_maxsim_batch / dann_chamfer_rerank_batch.

A document and a query are small matrices of token rows.  MaxSim: per query row, the best inner product over the document's
rows, as a similarity score (negated); Chamfer: their sum over the query's rows.  `order` picks whose bits come back
(include/dann.h): MAXSIM_KERNEL = MaxSimKernel::compute_max_sim (matrix cores), MAXSIM_REFERENCE = MaxSim::evaluate /
Chamfer::evaluate (the pair distance function).

MinMax-quantised sets (MM1 / MM2 / MM4 / MM8, diskann-quantization/src/minmax/multi/): documents and queries are
(rows, dann_layer_bytes(dtype, dim)) uint8 matrices of canonical images, as dann_minmax_compress writes them; `dim` must be
given.  `query_dtype` is the queries' width: the set's own, or MM8 on a narrower set.  Both orders return the same bits
there; MAXSIM_KERNEL runs the int8 matrix cores, MAXSIM_REFERENCE a plain kernel.
"""
import ctypes as C

import numpy as np

from ._ffi import F16, F32, MAXSIM_KERNEL, MAXSIM_REFERENCE, MM1, MM2, MM4, MM8, check, lib

_NP = {F32: np.float32, F16: np.float16}
_MM = (MM1, MM2, MM4, MM8)
SKIP = 0xFFFFFFFF  # a cand_ids entry that is not scored


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def csr(mats, np_dtype, dim, offset_dtype):
    """(offsets, packed rows) of a list of (rows_i x dim) matrices; matrices without rows are allowed"""
    mats = [np.ascontiguousarray(m, dtype=np_dtype).reshape(-1, dim) for m in mats]
    off = np.zeros(len(mats) + 1, offset_dtype)
    if mats:
        off[1:] = np.cumsum([m.shape[0] for m in mats])
    rows = np.ascontiguousarray(np.vstack(mats)) if mats and off[-1] else np.zeros((0, dim), np_dtype)
    return off, rows


class MultiVectorSet:
    """An immutable, device-resident set of multi-vector documents (dann_mvset)."""

    def __init__(self, dtype, docs, device=-1, dim=None, query_dtype=None):
        if dtype not in _NP and dtype not in _MM:
            raise ValueError("multi-vector sets hold F32, F16 or MM1 / MM2 / MM4 / MM8 rows")
        if dim is None:
            if dtype in _MM:
                raise ValueError("dim is needed for a MinMax set: it cannot be read off the images' shape")
            if not len(docs):
                raise ValueError("dim is needed for a set without documents")
            dim = np.asarray(docs[0]).shape[-1]
        self.dtype, self.dim, self.ndocs = dtype, int(dim), len(docs)
        off, rows = csr(docs, *self._row_shape(dtype), np.uint64)
        self.nrows = int(off[-1])
        h = C.c_void_p()
        check(lib().dann_mvset_create(device, dtype, self.dim, self.ndocs, _vp(off), _vp(rows), C.byref(h)),
              "dann_mvset_create")
        self._h = h
        if query_dtype is not None:
            self.query_dtype = query_dtype

    def _row_shape(self, dtype):
        """(numpy element type, elements per row) of the rows of `dtype` that the C calls take"""
        if dtype in _MM:
            return np.uint8, check(lib().dann_layer_bytes(dtype, self.dim), "dann_layer_bytes")
        return _NP[dtype], self.dim

    @property
    def query_dtype(self):
        """the dtype of the queries' rows (dann_mvset_get_query_dtype): the set's own unless set otherwise"""
        out = C.c_int32()
        check(lib().dann_mvset_get_query_dtype(self._h, C.byref(out)), "dann_mvset_get_query_dtype")
        return out.value

    @query_dtype.setter
    def query_dtype(self, dtype):
        check(lib().dann_mvset_set_query_dtype(self._h, dtype), "dann_mvset_set_query_dtype")

    def close(self):
        if getattr(self, "_h", None):
            lib().dann_mvset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        dt, dim, nd, nr = C.c_int32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(lib().dann_mvset_info(self._h, C.byref(dt), C.byref(dim), C.byref(nd), C.byref(nr)), "dann_mvset_info")
        return dt.value, dim.value, nd.value, nr.value

    def _call_args(self, queries, cand_ids):
        qoff, qrows = csr(queries, *self._row_shape(self.query_dtype), np.uint32)
        cand = np.ascontiguousarray(cand_ids, dtype=np.uint32)
        if cand.ndim == 1:
            cand = np.ascontiguousarray(np.broadcast_to(cand, (len(queries), cand.shape[0])))
        if cand.ndim != 2 or cand.shape[0] != len(queries):
            raise ValueError("cand_ids is (candidates,) or (queries, candidates)")
        return qoff, qrows, cand

    def maxsim(self, queries, cand_ids, order=MAXSIM_KERNEL, per_row=False):
        """Chamfer scores (len(queries) x candidates) of each query against its candidates; skipped entries (SKIP) are
        +inf.  per_row=True also returns the MaxSim scores: a list with one (candidates x rows(q)) array per query."""
        qoff, qrows, cand = self._call_args(queries, cand_ids)
        nq, stride = cand.shape
        chamfer = np.empty((nq, stride), np.float32)
        scores = np.empty(int(qoff[-1]) * stride, np.float32) if per_row else None
        check(lib().dann_maxsim_batch(self._h, order, _vp(qrows), _vp(qoff), nq, _vp(cand), stride, _vp(chamfer),
                                      _vp(scores) if per_row else None), "dann_maxsim_batch")
        if not per_row:
            return chamfer
        out = []
        for q in range(nq):
            lo, n = int(qoff[q]), int(qoff[q + 1] - qoff[q])
            out.append(scores[lo * stride:(lo + n) * stride].reshape(stride, n))
        return chamfer, out

    def chamfer_rerank(self, queries, cand_ids, k, order=MAXSIM_KERNEL):
        """(ids, Chamfer scores, counts): per query its candidates by ascending Chamfer score, equal scores in candidate
        order, the first k (padded with SKIP / +inf); counts[q] = entries written."""
        qoff, qrows, cand = self._call_args(queries, cand_ids)
        nq, stride = cand.shape
        ids = np.empty((nq, k), np.uint32)
        dists = np.empty((nq, k), np.float32)
        counts = np.empty(nq, np.uint32)
        check(lib().dann_chamfer_rerank_batch(self._h, order, _vp(qrows), _vp(qoff), nq, _vp(cand), stride, k, _vp(ids),
                                              _vp(dists), _vp(counts)), "dann_chamfer_rerank_batch")
        return ids, dists, counts


__all__ = ["MultiVectorSet", "MAXSIM_KERNEL", "MAXSIM_REFERENCE", "SKIP", "csr"]
