"""dann_maxsim_batch / dann_chamfer_rerank_batch on the GPU against tests/maxsim_model.py, BIT FOR BIT: the kernel order
(maxsim_mfma_kernel, matrix cores) and the reference order (maxsim_rows_kernel) each against the model's same order."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import bits
from maxsim_model import F32_MAX, KERNEL, REFERENCE, chamfer_of, scores

pytestmark = pytest.mark.gpu

DTYPES = [oracle.F32, oracle.F16]
ORDERS = [KERNEL, REFERENCE]
SKIP = 0xFFFFFFFF
INT_SHAPES = [(1, 1, 4), (1, 5, 8), (5, 1, 8), (3, 4, 16), (7, 7, 32), (2, 3, 128)]
# (query rows, document rows, dim): every value of each axis of the issue's sweep, (33, 33, 129) and (1, 1, 1) among them
SWEEP = [(1, 1, 1), (5, 0, 2), (31, 3, 3), (32, 31, 7), (33, 32, 8), (64, 33, 33), (70, 65, 100), (5, 130, 128),
         (33, 33, 129), (32, 65, 260), (70, 130, 128), (1, 1, 260)]
# the thresholds the kernels have, each crossed by the smallest shape that does:
THRESHOLDS = [
    (130, 70, 128),  # > 128 query rows: a second group of four query tiles; > 32 document rows: three LDS stages
    (40, 70, 257),   # dim > 128: the K-slab path, 257 = two whole 128-k slabs and a third of one (odd) column
    (3, 40, 32), (3, 40, 64), (3, 40, 65),  # dim 32 | 33 (above), 64 | 65: the 16- / 32- / 64-register query tiles
    (257, 2, 16),    # the reference-order kernel: > 256 / G lane groups, a second pass over the query's rows
]


def scaled_rows(rng, n, dim, npdt):
    """standard_normal x uniform(0.1, 8) row scales, as test_gram_tiles_equal_one_fmaf_chain_per_entry uses"""
    return (rng.standard_normal((n, dim)) * rng.uniform(0.1, 8.0, (n, 1))).astype(npdt)


def check_pairs(dtype, queries, docs, cand=None):
    """every (query, candidate) of `cand` (default: all documents for every query), both orders: per-row scores and
    Chamfer sums equal the model's bits"""
    import diskann_amd as da
    if cand is None:
        cand = np.tile(np.arange(len(docs), dtype=np.uint32), (len(queries), 1))
    with da.MultiVectorSet(dtype, docs, dim=queries[0].shape[1]) as s:
        for order in ORDERS:
            ch, per_row = s.maxsim(queries, cand, order=order, per_row=True)
            ch2 = s.maxsim(queries, cand, order=order)
            assert np.array_equal(bits(ch), bits(ch2)), "Chamfer with and without out_scores"
            for q, Q in enumerate(queries):
                for c, d in enumerate(cand[q]):
                    if d == SKIP:
                        assert np.all(np.isposinf(per_row[q][c])) and np.isposinf(ch[q, c])
                        continue
                    want = scores(dtype, order, Q, docs[d])
                    got = per_row[q][c]
                    assert np.array_equal(bits(got), bits(want)), (order, q, c, np.flatnonzero(bits(got) != bits(want))[:8])
                    assert bits(ch[q, c]) == bits(chamfer_of(want, len(docs[d]))), (order, q, c)


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_shapes(dtype):
    rng = np.random.default_rng(11)
    npdt = oracle.NP_DTYPE[dtype]
    for nq, nd, dim in INT_SHAPES:
        Q = rng.integers(-4, 5, (nq, dim)).astype(npdt)
        D = rng.integers(-4, 5, (nd, dim)).astype(npdt)
        check_pairs(dtype, [Q], [D])
        want = (-(Q.astype(np.float64) @ D.astype(np.float64).T).max(axis=1)).astype(np.float32)
        assert np.array_equal(scores(dtype, KERNEL, Q, D), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq,nd,dim", SWEEP)
def test_shape_sweep_at_the_tile_boundaries(dtype, nq, nd, dim):
    rng = np.random.default_rng(20_000 + 1000 * nq + 10 * nd + dim)
    npdt = oracle.NP_DTYPE[dtype]
    check_pairs(dtype, [scaled_rows(rng, nq, dim, npdt)], [scaled_rows(rng, nd, dim, npdt)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq,nd,dim", THRESHOLDS)
def test_every_threshold_of_the_kernels(dtype, nq, nd, dim):
    rng = np.random.default_rng(30_000 + 1000 * nq + 10 * nd + dim)
    npdt = oracle.NP_DTYPE[dtype]
    check_pairs(dtype, [scaled_rows(rng, nq, dim, npdt)], [scaled_rows(rng, nd, dim, npdt)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nd", [3, 33])
def test_all_negative_documents(dtype, nd):
    """every inner product is negative: a zero-padded document row (ip = 0) would win the maximum if it reached it"""
    rng = np.random.default_rng(41 + nd)
    npdt = oracle.NP_DTYPE[dtype]
    dim = 24
    Q = np.abs(scaled_rows(rng, 5, dim, np.float32)).astype(npdt) + npdt(0.25)
    D = (-Q[rng.integers(0, 5, nd)].astype(np.float32) + 0.01 * rng.standard_normal((nd, dim))).astype(npdt)
    for order in ORDERS:
        assert np.all(scores(dtype, order, Q, D) > 0)
    check_pairs(dtype, [Q], [D])


def batch_case(dtype):
    rng = np.random.default_rng(5)
    npdt = oracle.NP_DTYPE[dtype]
    dim = 20
    docs = [scaled_rows(rng, n, dim, npdt) for n in (4, 0, 37, 1, 9, 33)]
    queries = [scaled_rows(rng, n, dim, npdt) for n in (5, 33, 1)]
    cand = np.array([[2, SKIP, 0, 1, 5], [SKIP, 2, 3, 4, SKIP], [5, 4, 3, 2, 1]], np.uint32)  # document 2: all three queries
    return docs, queries, cand


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_plumbing(dtype):
    docs, queries, cand = batch_case(dtype)
    check_pairs(dtype, queries, docs, cand)


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_forms_equal_host_forms(dtype):
    import torch
    import diskann_amd as da
    from diskann_amd.multivector import csr
    docs, queries, cand = batch_case(dtype)
    npdt = oracle.NP_DTYPE[dtype]
    qoff, qrows = csr(queries, npdt, 20, np.uint32)
    nq, stride, k = cand.shape[0], cand.shape[1], 7
    L = da.lib()

    def dev(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    with da.MultiVectorSet(dtype, docs) as s:
        dq, do, dc = dev(qrows), dev(qoff), dev(cand)
        for order in ORDERS:
            ch, per_row = s.maxsim(queries, cand, order=order, per_row=True)
            dch = torch.zeros(nq * stride, dtype=torch.float32, device="cuda")
            dsc = torch.zeros(int(qoff[-1]) * stride, dtype=torch.float32, device="cuda")
            da._ffi.check(L.dann_maxsim_batch_device(s._h, order, ptr(dq), ptr(do), nq, ptr(dc), stride, ptr(dch), ptr(dsc)),
                          "dann_maxsim_batch_device")
            assert np.array_equal(bits(dch.cpu().numpy()), bits(ch.reshape(-1)))
            flat = np.concatenate([p.reshape(-1) for p in per_row])
            assert np.array_equal(bits(dsc.cpu().numpy()), bits(flat))
            ids, dists, counts = s.chamfer_rerank(queries, cand, k, order=order)
            di = torch.zeros(nq * k, dtype=torch.int32, device="cuda")
            dd = torch.zeros(nq * k, dtype=torch.float32, device="cuda")
            dn = torch.zeros(nq, dtype=torch.int32, device="cuda")
            da._ffi.check(L.dann_chamfer_rerank_batch_device(s._h, order, ptr(dq), ptr(do), nq, ptr(dc), stride, k, ptr(di),
                                                             ptr(dd), ptr(dn)), "dann_chamfer_rerank_batch_device")
            assert np.array_equal(di.cpu().numpy().view(np.uint32), ids.reshape(-1))
            assert np.array_equal(bits(dd.cpu().numpy()), bits(dists.reshape(-1)))
            assert np.array_equal(dn.cpu().numpy().view(np.uint32), counts)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
def test_chamfer_rerank(dtype, order):
    import diskann_amd as da
    rng = np.random.default_rng(61)
    npdt = oracle.NP_DTYPE[dtype]
    dim = 12
    docs = [scaled_rows(rng, n, dim, npdt) for n in (3, 7, 2, 40, 5, 1)]
    docs.append(docs[1].copy())  # document 6 == document 1: a real tie
    docs.append(docs[4].copy())  # document 7 == document 4
    queries = [scaled_rows(rng, n, dim, npdt) for n in (4, 35)]
    cand = np.array([[6, 3, SKIP, 1, 0, 7, 4, 2, SKIP], [4, 7, 5, SKIP, SKIP, 1, 6, 3, 0]], np.uint32)
    with da.MultiVectorSet(dtype, docs) as s:
        for k in (3, 12):  # 12 > the 7 live candidates: padding
            ids, dists, counts = s.chamfer_rerank(queries, cand, k, order=order)
            for q, Q in enumerate(queries):
                live = [int(d) for d in cand[q] if d != SKIP]
                vals = np.array([chamfer_of(scores(dtype, order, Q, docs[d]), len(docs[d])) for d in live], np.float32)
                perm = np.argsort(vals, kind="stable")
                n = min(k, len(live))
                assert counts[q] == n
                assert ids[q, :n].tolist() == [live[i] for i in perm[:n]]
                assert np.array_equal(bits(dists[q, :n]), bits(vals[perm[:n]]))
                assert np.all(ids[q, n:] == SKIP) and np.all(np.isposinf(dists[q, n:]))
            if k == 12:  # the ties came back in candidate order
                assert list(ids[0]).index(6) < list(ids[0]).index(1) and list(ids[1]).index(4) < list(ids[1]).index(7)


def test_status_codes():
    """argument checks: each returns before (or, for the candidate id, instead of) the offending access"""
    import diskann_amd as da
    E = da._ffi
    L = da.lib()
    rows = np.ones((4, 8), np.float32)
    off = np.array([0, 1, 4], np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = C.c_void_p()
    assert L.dann_mvset_create(-1, da.U8, 8, 2, vp(off), vp(rows), C.byref(h)) == E.EINVAL  # an unsupported dtype
    assert L.dann_mvset_create(-1, da.F32, 0, 2, vp(off), vp(rows), C.byref(h)) == E.EINVAL
    assert L.dann_mvset_create(-1, da.F32, 8, 2, None, vp(rows), C.byref(h)) == E.EINVAL
    assert L.dann_mvset_create(-1, da.F32, 8, 2, vp(np.array([0, 3, 2], np.uint64)), vp(rows), C.byref(h)) == E.ELENGTH
    assert L.dann_mvset_create(-1, da.F32, 8, 2, vp(np.array([1, 2, 4], np.uint64)), vp(rows), C.byref(h)) == E.ELENGTH
    assert L.dann_mvset_create(-1, da.F32, 4097, 0, vp(np.zeros(1, np.uint64)), None, C.byref(h)) == E.EUNSUPPORTED
    assert not h.value
    with da.MultiVectorSet(da.F32, [rows[:1], rows[1:]]) as s:
        assert s.info() == (da.F32, 8, 2, 4)
        q = np.ones((2, 8), np.float32)
        qoff = np.array([0, 2], np.uint32)
        cand = np.array([0, 1], np.uint32)
        out = np.zeros(2, np.float32)
        ids = np.zeros(2, np.uint32)
        cnt = np.zeros(1, np.uint32)
        call = lambda order=0, qoff=qoff, cand=cand, stride=2, q=q: L.dann_maxsim_batch(  # noqa: E731
            s._h, order, vp(q), vp(qoff), 1, vp(cand), stride, vp(out), None)
        assert call() == 0
        assert call(order=2) == E.EINVAL and call(order=-1) == E.EINVAL
        assert call(cand=np.array([0, 2], np.uint32)) == E.EBOUNDS  # id == ndocs
        assert call(qoff=np.array([1, 2], np.uint32)) == E.ELENGTH
        assert L.dann_maxsim_batch(s._h, 0, vp(q), vp(np.array([0, 2, 1], np.uint32)), 2, vp(np.zeros(4, np.uint32)), 2,
                                   vp(np.zeros(4, np.float32)), None) == E.ELENGTH
        assert call(stride=0) == E.EUNSUPPORTED and call(stride=4097) == E.EUNSUPPORTED
        big = np.ones((1025, 8), np.float32)  # 1025 query rows
        assert call(q=big, qoff=np.array([0, 1025], np.uint32)) == E.EUNSUPPORTED
        assert L.dann_maxsim_batch(None, 0, vp(q), vp(qoff), 1, vp(cand), 2, vp(out), None) == E.EINVAL
        assert L.dann_maxsim_batch(s._h, 0, vp(q), vp(qoff), 1, vp(cand), 2, None, None) == E.EINVAL
        rr = lambda order=0, k=2, cand=cand: L.dann_chamfer_rerank_batch(  # noqa: E731
            s._h, order, vp(q), vp(qoff), 1, vp(cand), 2, k, vp(ids), vp(out), vp(cnt))
        assert rr() == 0 and cnt[0] == 2
        assert rr(order=7) == E.EINVAL and rr(k=0) == E.EINVAL
        assert rr(cand=np.array([9, 0], np.uint32)) == E.EBOUNDS
        with pytest.raises(da.DannError) as e:
            s.maxsim([q], np.array([[5]], np.uint32))
        assert e.value.status == E.EBOUNDS


def test_through_python():
    import diskann_amd as da
    Q = np.array([[1, 0, 0], [0, 1, 0]], np.float32)  # the doc-comment example of multi_vector/distance/mod.rs
    D = np.array([[1, 0, 0], [0, 0, 1]], np.float32)
    with da.MultiVectorSet(da.F32, [D, np.zeros((0, 3), np.float32)]) as s:
        for order in (da.MAXSIM_KERNEL, da.MAXSIM_REFERENCE):
            ch, per_row = s.maxsim([Q], [0, 1, SKIP], order=order, per_row=True)
            assert per_row[0][0].tolist() == [-1.0, 0.0] and ch[0, 0] == -1.0
            assert np.array_equal(bits(per_row[0][1]), bits(np.full(2, F32_MAX))) and bits(ch[0, 1]) == bits(np.float32(0))
            assert np.isposinf(ch[0, 2])
            ids, dists, counts = s.chamfer_rerank([Q], [1, SKIP, 0], 3, order=order)
            assert ids[0].tolist() == [0, 1, SKIP] and counts[0] == 2 and dists[0, :2].tolist() == [-1.0, 0.0]
        # an empty query: Chamfer 0.0, nothing per row
        ch, per_row = s.maxsim([np.zeros((0, 3), np.float32)], [0], per_row=True)
        assert bits(ch[0, 0]) == bits(np.float32(0)) and per_row[0].shape == (1, 0)
