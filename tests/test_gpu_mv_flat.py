"""dann_mv_flat_search_batch on the GPU against tests/mv_flat_model.py, BIT FOR BIT, ids included: the kernel order
(mvflat_mfma_kernel, matrix cores) and the reference order (mvflat_rows_kernel) each against the model's same order."""
import ctypes as C
import functools

import numpy as np
import pytest

import mv_flat_model as mv
import oracle
from helpers import bits
from maxsim_model import KERNEL, REFERENCE

pytestmark = pytest.mark.gpu

DTYPES = [oracle.F32, oracle.F16]
ORDERS = [KERNEL, REFERENCE]
LENS, TILE_LENS = mv.LENS, mv.TILE_LENS


def rows(rng, n, dim, npdt):
    return (rng.standard_normal((n, dim)) * rng.uniform(0.1, 8.0, (n, 1))).astype(npdt)


@functools.lru_cache(maxsize=None)
def case(dtype, lens, qlens, dim, seed=0, integer=False, repeat=1):
    """(docs, queries, scores[order][query][doc]) of a set with documents of `lens` rows: computed once, shared"""
    rng = np.random.default_rng(seed + dim)
    npdt = oracle.NP_DTYPE[dtype]
    make = (lambda n: rng.integers(-2, 3, (n, dim)).astype(npdt)) if integer else (lambda n: rows(rng, n, dim, npdt))
    docs, queries = [make(n) for n in lens] * repeat, [make(n) for n in qlens]
    return docs, queries, {o: [mv.all_scores(dtype, o, Q, docs) for Q in queries] for o in ORDERS}


def check(dtype, docs, queries, scores, k, orders=ORDERS, aggs=mv.AGGREGATIONS, match=None, **rng_):
    """every output of flat_search equals the model's: ids, distance bits, cmps, written"""
    import diskann_amd as da
    with da.MultiVectorSet(dtype, docs, dim=queries[0].shape[1]) as s:
        for order in orders:
            for agg in aggs:
                ids, dists, st = s.flat_search(queries, k, order=order, aggregation=agg, match=match, stats=True, **rng_)
                for q in range(len(queries)):
                    m = None if match is None else np.asarray(match).reshape(-1, len(docs))[q if np.ndim(match) == 2 else 0]
                    wi, wd, cmps = mv.search(scores[order][q], docs, agg, k, match=m, **{"first": rng_.get("first", 0), "n": rng_.get("n")})
                    assert np.array_equal(ids[q], wi), (order, agg, q, ids[q][:8], wi[:8])
                    assert np.array_equal(bits(dists[q]), bits(wd)), (order, agg, q)
                    assert st["cmps"][q] == cmps and st["hops"][q] == 0
                    assert st["written"][q] == st["result_count"][q] == int((wi != 0xFFFFFFFF).sum())


# (queries of the tile set: 4 rows, none, 2 rows)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS)
def test_document_lengths_against_tiles_and_chunks(dtype, order):
    docs, queries, scores = case(dtype, TILE_LENS, (4, 0, 2), 16)
    check(dtype, docs, queries, scores, 10, orders=[order])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("qn", [1, 31, 32, 33, 128, 129])
def test_query_rows(dtype, qn):
    docs, queries, scores = case(dtype, tuple(LENS + [0]), (qn,), 8, seed=qn)
    check(dtype, docs, queries, scores, 5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [1, 2, 3, 127, 128, 129, 260])
def test_dim_sweep(dtype, dim):
    docs, queries, scores = case(dtype, (3, 33, 0, 40, 1), (5, 33), dim, seed=7)
    check(dtype, docs, queries, scores, 4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nd", [3, 33])
def test_all_negative_documents(dtype, nd):
    """every inner product is negative: a zero row behind a document's end (ip = 0) would win the maximum"""
    rng = np.random.default_rng(41 + nd)
    npdt = oracle.NP_DTYPE[dtype]
    Q = np.abs(rows(rng, 5, 24, np.float32)).astype(npdt) + npdt(0.25)
    docs = [(-Q[rng.integers(0, 5, n)].astype(np.float32) + 0.01 * rng.standard_normal((n, 24))).astype(npdt) for n in (nd, 2, nd)]
    scores = {o: [mv.all_scores(dtype, o, Q, docs)] for o in ORDERS}
    assert all(np.all(sc > 0) for o in ORDERS for sc in scores[o][0])
    check(dtype, docs, [Q], scores, 3)


@pytest.mark.parametrize("k", [1, 3, 20, 60 + 5, 1024])
def test_ties(k):
    """small-integer rows, every document three times: many equal scores (k = 20 cuts through a run); the later wins"""
    docs, queries, scores = case(oracle.F32, (2, 1, 3, 0, 33, 1, 2, 5, 1, 40, 2, 1, 3, 1, 1, 2, 7, 1, 1, 0), (3, 1), 4, integer=True,
                                 repeat=3)
    check(oracle.F32, docs, queries, scores, k)
    import diskann_amd as da
    with da.MultiVectorSet(oracle.F32, docs) as s:
        ids, dists = s.flat_search(queries, k)
    run = (dists[0][:-1] == dists[0][1:]) & (ids[0][1:] != 0xFFFFFFFF)  # (not the padding)
    assert k == 1 or (run.any() and np.all(ids[0][:-1][run] > ids[0][1:][run]))


FILTERS = ["shared", "per_query", "ones", "zeros", "no_tile_no_chunk"]


@pytest.mark.parametrize("kind", FILTERS)
def test_filter(kind):
    docs, queries, scores = case(oracle.F32, TILE_LENS, (4, 0, 2), 16)
    rng = np.random.default_rng(9)
    nd = len(docs)
    match = {"shared": rng.random(nd) < 0.5, "per_query": rng.random((3, nd)) < 0.3, "ones": np.ones(nd, bool),
             "zeros": np.zeros((3, nd), bool), "no_tile_no_chunk": np.ones(nd, bool)}[kind]
    if kind == "no_tile_no_chunk":  # documents 5 .. 7 (64, 65 and no rows) hold whole tiles; 37 .. 70 are the second chunk
        match[5:8] = False
        match[33:71] = False
    check(oracle.F32, docs, queries, scores, 10, match=match)
    if kind == "ones":  # equals the unfiltered call in every output
        import diskann_amd as da
        with da.MultiVectorSet(oracle.F32, docs) as s:
            a, b = s.flat_search(queries, 10, match=match, stats=True), s.flat_search(queries, 10, stats=True)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize("first,n", [(3, 40), (30, 60), (0, 0), (len(TILE_LENS), 0), (len(TILE_LENS) - 3, 3)])
def test_range(first, n):
    docs, queries, scores = case(oracle.F32, TILE_LENS, (4, 0, 2), 16)
    check(oracle.F32, docs, queries, scores, 10, aggs=[mv.CHAMFER, mv.MIN_PAIRWISE], first=first, n=n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_form_equals_host_form(dtype):
    import torch
    import diskann_amd as da
    from diskann_amd.multivector import csr
    docs, queries, _ = case(dtype, (3, 33, 0, 40, 1), (5, 33), 128, seed=7)
    qoff, qrows = csr(queries, oracle.NP_DTYPE[dtype], 128, np.uint32)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    bitsw = np.array([0b10111, 0b01101], np.uint32)
    with da.MultiVectorSet(dtype, docs) as s:
        dq, do, db = dev(qrows), dev(qoff), dev(bitsw)
        f = da._ffi.FlatFilter(db.data_ptr(), 1)
        for order in ORDERS:
            match = np.array([[1, 1, 1, 0, 1], [1, 0, 1, 1, 0]], bool)
            ids, dists, st = s.flat_search(queries, 3, order=order, aggregation=mv.MIN_PAIRWISE, match=match, stats=True)
            di, dd = torch.zeros(6, dtype=torch.int32, device="cuda"), torch.zeros(6, dtype=torch.float32, device="cuda")
            ds = torch.zeros(2 * 20, dtype=torch.uint8, device="cuda")
            da._ffi.check(da.lib().dann_mv_flat_search_batch_device(s._h, order, mv.MIN_PAIRWISE, ptr(dq), ptr(do), 2, 0, 5, 3,
                                                                    C.byref(f), ptr(di), ptr(dd), ptr(ds)), "device form")
            assert np.array_equal(di.cpu().numpy().view(np.uint32), ids.reshape(-1))
            assert np.array_equal(bits(dd.cpu().numpy()), bits(dists.reshape(-1)))
            assert np.array_equal(ds.cpu().numpy(), st.view(np.uint8))


def test_status_codes_and_the_wrapper():
    import diskann_amd as da
    E, L = da._ffi, da.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    D = np.array([[1, 0, 0], [0, 0, 1]], np.float32)
    Q = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    qoff, ids, dists = np.array([0, 2], np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.float32)
    with da.MultiVectorSet(da.F32, [D, np.zeros((0, 3), np.float32)]) as s:
        def call(h=s._h, order=0, agg=0, q=Q, qoff=qoff, nq=1, first=0, n=2, k=2, f=None, ids=ids, dists=dists):
            return L.dann_mv_flat_search_batch(h, order, agg, None if q is None else vp(q), None if qoff is None else vp(qoff),
                                               nq, first, n, k, f, None if ids is None else vp(ids),
                                               None if dists is None else vp(dists), None)
        assert call() == 0 and ids.tolist() == [0, 1] and dists.tolist() == [-1.0, 0.0]  # (mod.rs's doc-comment example)
        assert call(h=None) == E.EINVAL and call(order=2) == E.EINVAL and call(agg=4) == E.EINVAL and call(agg=-1) == E.EINVAL
        assert call(agg=da.MV_AVERAGE_PAIRWISE) == E.EUNSUPPORTED
        assert call(k=0) == E.EINVAL and call(k=1025) == E.EUNSUPPORTED
        assert call(first=1, n=2) == E.EBOUNDS and call(first=3, n=0) == E.EBOUNDS and call(first=2, n=0) == 0
        words = np.ones(4, np.uint32)
        assert call(nq=2, qoff=np.array([0, 1, 2], np.uint32), f=C.byref(E.FlatFilter(words.ctypes.data, 1)), ids=np.zeros(4, np.uint32),
                    dists=np.zeros(4, np.float32)) == 0
        big = da.MultiVectorSet(da.F32, [D[:1]] * 33)
        assert L.dann_mv_flat_search_batch(big._h, 0, 0, vp(Q), vp(np.array([0, 1, 2], np.uint32)), 2, 0, 33, 2,
                                           C.byref(E.FlatFilter(words.ctypes.data, 1)), vp(ids), vp(dists), None) == E.EINVAL
        big.close()
        assert call(nq=0, q=None, qoff=None, ids=None, dists=None) == 0
        assert call(qoff=None) == E.EINVAL and call(ids=None) == E.EINVAL and call(dists=None) == E.EINVAL and call(q=None) == E.EINVAL
        assert call(qoff=np.array([1, 2], np.uint32)) == E.ELENGTH
        assert call(q=np.ones((1025, 3), np.float32), qoff=np.array([0, 1025], np.uint32)) == E.EUNSUPPORTED
        # the wrapper: padding behind the two documents, the empty document's Chamfer 0.0
        wi, wd = s.flat_search([Q], 3)
        assert wi[0].tolist() == [0, 1, 0xFFFFFFFF] and wd[0].tolist() == [-1.0, 0.0, np.inf]
    img = np.zeros((2, da.lib().dann_layer_bytes(da.MM8, 8)), np.uint8)
    with da.MultiVectorSet(da.MM8, [img], dim=8) as s:
        assert L.dann_mv_flat_search_batch(s._h, 0, 0, vp(img), vp(qoff), 1, 0, 1, 1, None, vp(ids), vp(dists), None) == E.EUNSUPPORTED


def test_whole_set_equals_chamfer_rerank_of_all_ids():
    import diskann_amd as da
    docs, queries, _ = case(oracle.F32, tuple(LENS), (5, 33), 128, seed=7)
    with da.MultiVectorSet(oracle.F32, docs) as s:
        for order in ORDERS:
            ids, dists = s.flat_search(queries, len(docs), order=order)
            rid, rd, _ = s.chamfer_rerank(queries, np.arange(len(docs), dtype=np.uint32), len(docs), order=order)
            assert len(set(rd[0].tolist())) >= len(docs) - 1  # distinct scores but for the two empty documents (0.0, 0.0)
            keep = lambda i, d: [(a, b) for a, b in zip(i.tolist(), bits(d).tolist()) if len(docs[a])]  # noqa: E731
            assert all(keep(ids[q], dists[q]) == keep(rid[q], rd[q]) for q in range(2))
