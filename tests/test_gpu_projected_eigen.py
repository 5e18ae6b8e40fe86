"""dann_projected_eigen_batch / dann_projected_eigen_rerank_batch on the GPU against tests/projected_eigen_model.py, BIT FOR
BIT: the kernel order (projeig_mfma_kernel, matrix cores) and the reference order (projeig_rows_kernel) each against the
model's same order, and both within the derived rounding bound of the float64 value.

Standard-normal values: nearly every cell changes bits if the order of the document rows, the hand-off between the lane
halves or the carry from tile to tile is wrong.  One set per (dtype, dim); every query length meets every document length.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from helpers import bits
from projected_eigen_model import KERNEL, REFERENCE, exact, scores, total_of

pytestmark = pytest.mark.gpu

DTYPES = [oracle.F32, oracle.F16]
ORDERS = [KERNEL, REFERENCE]
DIMS = [1, 7, 128, 130]  # an odd dim padded to one k-pair; 128 | 130: the last register-resident query tile | two slabs
DOC_ROWS = [0, 1, 16, 17, 32, 33, 70]  # 16 | 17: the hand-off between the halves; 32 | 33: a second tile; 70: three, ragged
Q_ROWS = [0, 1, 33, 129]  # 33: a second wavefront's tile; 129: the second group of four
SKIP = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def case(dtype, dim):
    """(docs, queries, cand, model): model[order][q][d] = the per-row scores of query q against document d"""
    rng = np.random.default_rng(9000 + 10 * dim + dtype)
    npdt = oracle.NP_DTYPE[dtype]
    docs = [rng.standard_normal((n, dim)).astype(np.float32).astype(npdt) for n in DOC_ROWS]
    queries = [rng.standard_normal((n, dim)).astype(np.float32).astype(npdt) for n in Q_ROWS]
    # every document in a different order per query, a skipped entry inside, and a repeated id (a real tie for the rerank)
    cand = np.array([list(np.roll(np.arange(len(docs)), q)) + [SKIP, 3 + q] for q in range(len(queries))], np.uint32)
    cand[:, [2, 7]] = cand[:, [7, 2]]
    model = {o: [[scores(dtype, o, Q, D) for D in docs] for Q in queries] for o in ORDERS}
    return docs, queries, cand, model


def dev(a):
    import torch
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_bits_bound_and_rerank(dtype, dim):
    import torch
    import diskann_amd as da
    from diskann_amd.multivector import csr
    docs, queries, cand, model = case(dtype, dim)
    nq, stride = cand.shape
    qoff, qrows = csr(queries, oracle.NP_DTYPE[dtype], dim, np.uint32)
    L, u = da.lib(), 2.0 ** -24
    with da.MultiVectorSet(dtype, docs, dim=dim) as s:
        dq, do, dc = dev(qrows), dev(qoff), dev(cand)
        for order in ORDERS:
            dist, per_row = s.projected_eigen(queries, cand, order=order, per_row=True)
            assert np.array_equal(bits(dist), bits(s.projected_eigen(queries, cand, order=order)))  # without out_scores
            want = np.full((nq, stride), np.inf, np.float32)
            for q, Q in enumerate(queries):
                for c, d in enumerate(cand[q]):
                    if d == SKIP:
                        assert np.all(np.isposinf(per_row[q][c])) and np.isposinf(dist[q, c])
                        continue
                    sc = model[order][q][d]
                    assert np.array_equal(bits(per_row[q][c]), bits(sc)), (order, q, d)
                    want[q, c] = total_of(sc)
                    assert bits(dist[q, c]) == bits(want[q, c]), (order, q, d)
                    # each ip is off by at most gamma_dim A_ij; squaring doubles that and adds one rounding; the two
                    # sums add d_rows + q_rows roundings
                    n = 2 * dim + len(docs[d]) + len(Q) + 4
                    val, scale = exact(Q, docs[d])
                    assert abs(float(dist[q, c]) - val) <= n * u / (1 - n * u) * scale, (order, q, d)
            # the _device form
            ddist = torch.zeros(nq * stride, dtype=torch.float32, device="cuda")
            dsc = torch.zeros(int(qoff[-1]) * stride, dtype=torch.float32, device="cuda")
            da._ffi.check(L.dann_projected_eigen_batch_device(s._h, order, ptr(dq), ptr(do), nq, ptr(dc), stride, ptr(ddist),
                                                              ptr(dsc)), "dann_projected_eigen_batch_device")
            assert np.array_equal(bits(ddist.cpu().numpy()), bits(dist.reshape(-1)))
            assert np.array_equal(bits(dsc.cpu().numpy()), bits(np.concatenate([p.reshape(-1) for p in per_row])))
            # the rerank: a stable ascending sort of the model's distances, k below / at / above the 8 live candidates
            for k in (3, 8, 11):
                ids, dists, counts = s.projected_eigen_rerank(queries, cand, k, order=order)
                for q in range(nq):
                    live = np.flatnonzero(cand[q] != SKIP)
                    perm = live[np.argsort(want[q, live], kind="stable")]
                    n = min(k, len(live))
                    assert counts[q] == n and ids[q, :n].tolist() == cand[q, perm[:n]].tolist()
                    assert np.array_equal(bits(dists[q, :n]), bits(want[q, perm[:n]]))
                    assert np.all(ids[q, n:] == SKIP) and np.all(np.isposinf(dists[q, n:]))
            di = torch.zeros(nq * k, dtype=torch.int32, device="cuda")
            dd = torch.zeros(nq * k, dtype=torch.float32, device="cuda")
            dn = torch.zeros(nq, dtype=torch.int32, device="cuda")
            da._ffi.check(L.dann_projected_eigen_rerank_batch_device(s._h, order, ptr(dq), ptr(do), nq, ptr(dc), stride, k,
                                                                     ptr(di), ptr(dd), ptr(dn)), "rerank_batch_device")
            assert np.array_equal(di.cpu().numpy().view(np.uint32), ids.reshape(-1))
            assert np.array_equal(bits(dd.cpu().numpy()), bits(dists.reshape(-1)))
            assert np.array_equal(dn.cpu().numpy().view(np.uint32), counts)


def test_status_codes():
    import diskann_amd as da
    E = da._ffi
    L = da.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    q, qoff, cand = np.ones((2, 8), np.float32), np.array([0, 2], np.uint32), np.array([0, 1], np.uint32)
    out, ids, cnt = np.zeros(2, np.float32), np.zeros(2, np.uint32), np.zeros(1, np.uint32)

    def call(h, order=0, cand=cand, out=out):
        return L.dann_projected_eigen_batch(h, order, vp(q), vp(qoff), 1, vp(cand), 2, None if out is None else vp(out), None)

    def rerank(h, order=0):
        return L.dann_projected_eigen_rerank_batch(h, order, vp(q), vp(qoff), 1, vp(cand), 2, 2, vp(ids), vp(out), vp(cnt))

    with da.MultiVectorSet(da.F32, [q[:1], q[1:]]) as s:
        assert call(s._h) == 0 and out.tolist() == [-128.0, -128.0]  # two query rows x one document row of ip = 8
        assert rerank(s._h) == 0 and cnt[0] == 2 and ids.tolist() == [0, 1]
        assert call(s._h, order=2) == E.EINVAL and rerank(s._h, order=2) == E.EINVAL
        assert call(None) == E.EINVAL and call(s._h, out=None) == E.EINVAL
        assert call(s._h, cand=np.array([0, 2], np.uint32)) == E.EBOUNDS  # id == ndocs
    image = np.zeros((2, L.dann_layer_bytes(da.MM8, 8)), np.uint8)
    with da.MultiVectorSet(da.MM8, [image[:1], image[1:]], dim=8) as s:
        assert call(s._h) == E.EUNSUPPORTED and rerank(s._h) == E.EUNSUPPORTED
