"""Multi-vector (late-interaction) scoring: dann_mvset + dann_maxsim_batch / dann_chamfer_rerank_batch.

A document and a query are small matrices of token rows.  MaxSim: per query row, the best inner product over the document's
rows, as a similarity score (negated); Chamfer: their sum over the query's rows.  `order` picks whose bits come back
(include/dann.h): MAXSIM_KERNEL = MaxSimKernel::compute_max_sim (matrix cores), MAXSIM_REFERENCE = MaxSim::evaluate /
Chamfer::evaluate (the pair distance function).
"""
import ctypes as C

import numpy as np

from ._ffi import F16, F32, MAXSIM_KERNEL, MAXSIM_REFERENCE, check, lib

_NP = {F32: np.float32, F16: np.float16}
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

    def __init__(self, dtype, docs, device=-1, dim=None):
        if dtype not in _NP:
            raise ValueError("multi-vector sets hold F32 or F16 rows")
        if dim is None:
            if not len(docs):
                raise ValueError("dim is needed for a set without documents")
            dim = np.asarray(docs[0]).shape[-1]
        self.dtype, self.dim, self.ndocs = dtype, int(dim), len(docs)
        off, rows = csr(docs, _NP[dtype], self.dim, np.uint64)
        self.nrows = int(off[-1])
        h = C.c_void_p()
        check(lib().dann_mvset_create(device, dtype, self.dim, self.ndocs, _vp(off), _vp(rows), C.byref(h)),
              "dann_mvset_create")
        self._h = h

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
        qoff, qrows = csr(queries, _NP[self.dtype], self.dim, np.uint32)
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
