"""MaxSim / Chamfer over MinMax-quantised multi-vector sets on the GPU against tests/maxsim_mm_model.py, BIT FOR BIT: all
seven (query bits, document bits) pairs, and both kernels -- DANN_MAXSIM_KERNEL (maxsim_mm_mfma_kernel, int8 matrix
cores) and DANN_MAXSIM_REFERENCE (maxsim_mm_rows_kernel, plain) -- against the one model: the raw product is an integer and
has no order."""
import ctypes as C

import numpy as np
import pytest

import minmax_model as mm
from helpers import bits
from maxsim_mm_model import PAIRS, empty, scores_mm
from maxsim_model import F32_MAX, chamfer_of

pytestmark = pytest.mark.gpu

KERNEL, REFERENCE = 0, 1
ORDERS = [KERNEL, REFERENCE]
SKIP = 0xFFFFFFFF
INT_SHAPES = [(1, 1, 4), (1, 5, 8), (5, 1, 8), (3, 4, 16), (7, 7, 32), (2, 3, 128)]  # the reference's own
# (query rows, document rows, dim)
SWEEP = [(1, 1, 1), (5, 0, 2), (31, 3, 3), (32, 31, 7), (33, 32, 15), (64, 33, 33), (70, 65, 100), (5, 130, 128),
         (33, 33, 129), (32, 65, 260)]
# the thresholds the kernels have, each crossed by the smallest shape that does:
THRESHOLDS = [
    (130, 70, 128),  # > 128 query rows: a second group of four query tiles; > 64 document rows: three document tiles
    (3, 40, 128), (3, 40, 129),  # the 128-k slab: one slab, the query tiles staged once | two slabs, staged with each
    (3, 40, 256), (3, 40, 257),  # two whole slabs | a third with one column
    (64, 2, 16), (65, 2, 16),    # the plain kernel: 256 / 4 lane groups, one pass over the query's rows | a second
]


def dt(bits_):
    import diskann_amd as da
    return {1: da.MM1, 2: da.MM2, 4: da.MM4, 8: da.MM8}[bits_]


def images(rng, n, dim, bits_):
    """standard_normal x uniform(0.1, 8) row scales, compressed"""
    if n == 0:
        return empty(bits_, dim)
    return mm.compress(rng.standard_normal((n, dim)) * rng.uniform(0.1, 8.0, (n, 1)), bits_)[0]


def check_pairs(qbits, dbits, dim, queries, docs, cand=None, model_queries=None, model_docs=None):
    """every (query, candidate) of `cand` (default: all documents for every query), both kernels: per-row scores and
    Chamfer sums equal the model's bits (the model may be given other images: those the GPU's must be equivalent to)"""
    import diskann_amd as da
    if cand is None:
        cand = np.tile(np.arange(len(docs), dtype=np.uint32), (len(queries), 1))
    mq = queries if model_queries is None else model_queries
    md = docs if model_docs is None else model_docs
    want = {(q, int(d)): scores_mm(mq[q], md[d], dim, qbits, dbits)
            for q in range(len(queries)) for d in np.unique(cand[q]) if d != SKIP}
    with da.MultiVectorSet(dt(dbits), docs, dim=dim, query_dtype=dt(qbits)) as s:
        assert s.query_dtype == dt(qbits) and s.info() == (dt(dbits), dim, len(docs), sum(len(d) for d in docs))
        for order in ORDERS:
            ch, per_row = s.maxsim(queries, cand, order=order, per_row=True)
            ch2 = s.maxsim(queries, cand, order=order)
            assert np.array_equal(bits(ch), bits(ch2)), "Chamfer with and without out_scores"
            for q in range(len(queries)):
                for c, d in enumerate(cand[q]):
                    if d == SKIP:
                        assert np.all(np.isposinf(per_row[q][c])) and np.isposinf(ch[q, c])
                        continue
                    w = want[q, int(d)]
                    got = per_row[q][c]
                    assert np.array_equal(bits(got), bits(w)), (order, q, c, np.flatnonzero(bits(got) != bits(w))[:8])
                    assert bits(ch[q, c]) == bits(chamfer_of(w, len(docs[d]))), (order, q, c)
    return want


@pytest.mark.parametrize("qbits,dbits", PAIRS)
def test_reference_shapes_on_twin_rows(qbits, dbits):
    rng = np.random.default_rng(11 + qbits + dbits)
    for nq, nd, dim in INT_SHAPES:
        cq = rng.integers(0, 1 << qbits, (nq, dim)).astype(np.uint8)
        cd = rng.integers(0, 1 << dbits, (nd, dim)).astype(np.uint8)
        want = check_pairs(qbits, dbits, dim, [mm.twin_rows(cq, qbits)], [mm.twin_rows(cd, dbits)])
        raw = cq.astype(np.float64) @ cd.astype(np.float64).T
        assert np.array_equal(want[0, 0], (-raw.max(axis=1)).astype(np.float32))


def shape_case(seed, qbits, dbits, nq, nd, dim):
    rng = np.random.default_rng([seed, nq, nd, dim, qbits, dbits])
    Q, D = images(rng, nq, dim, qbits), images(rng, nd, dim, dbits)
    sc = scores_mm(Q, D, dim, qbits, dbits)
    assert np.all(np.isfinite(sc)) and np.all(sc != 0), "inside the contract: finite, and no zero among the minima"
    check_pairs(qbits, dbits, dim, [Q], [D])


@pytest.mark.parametrize("qbits,dbits", PAIRS)
@pytest.mark.parametrize("nq,nd,dim", SWEEP)
def test_shape_sweep_at_the_tile_boundaries(qbits, dbits, nq, nd, dim):
    shape_case(7, qbits, dbits, nq, nd, dim)


@pytest.mark.parametrize("qbits,dbits", PAIRS)
@pytest.mark.parametrize("nq,nd,dim", THRESHOLDS)
def test_every_threshold_of_the_kernels(qbits, dbits, nq, nd, dim):
    shape_case(8, qbits, dbits, nq, nd, dim)


@pytest.mark.parametrize("qbits,dbits", PAIRS)
def test_extremes_every_code_at_its_maximum(qbits, dbits):
    """(3, 40, 4096), a = 1, b = 0: for (8, 8) raw = 255^2 * 4096 = 266 342 400 > 2^24 -- the u32 -> f32 rounding and all
    three correction terms of the bias identity are live"""
    nq, nd, dim = 3, 40, 4096

    def top_rows(n, bits_):
        codes = np.full((n, dim), (1 << bits_) - 1, np.uint8)
        c = codes.astype(np.int64)
        return mm.make_rows(codes, bits_, np.zeros(n), c.sum(1), np.ones(n), (c * c).sum(1))

    want = check_pairs(qbits, dbits, dim, [top_rows(nq, qbits)], [top_rows(nd, dbits)])
    raw = ((1 << qbits) - 1) * ((1 << dbits) - 1) * dim
    assert np.array_equal(want[0, 0], np.full(nq, -np.float32(np.uint32(raw)), np.float32))
    if (qbits, dbits) == (8, 8):
        assert raw == 266_342_400 and raw > (1 << 24)


@pytest.mark.parametrize("qbits,dbits", PAIRS)
def test_extremes_random_codes_at_the_largest_dim(qbits, dbits):
    shape_case(9, qbits, dbits, 3, 40, 4096)


@pytest.mark.parametrize("qbits,dbits", PAIRS)
@pytest.mark.parametrize("nd", [3, 33])
def test_phantom_rows_never_reach_the_minimum(qbits, dbits, nd):
    """every true score is positive (documents of negated query rows: negative b): a padded all-zero row would score
    -0.0 and win the minimum if it reached it"""
    rng = np.random.default_rng(41 + nd)
    dim = 24
    x = np.abs(rng.standard_normal((5, dim)) * rng.uniform(0.1, 8.0, (5, 1))).astype(np.float32) + np.float32(0.25)
    y = (-x[rng.integers(0, 5, nd)] + 0.01 * rng.standard_normal((nd, dim))).astype(np.float32)
    Q, D = mm.compress(x, qbits)[0], mm.compress(y, dbits)[0]
    assert np.all(mm.header(D)[1] < 0)
    assert np.all(mm.distance_matrix(mm.IP, Q, D, dim, dbits, qbits=qbits) > 0)
    check_pairs(qbits, dbits, dim, [Q], [D])


def dirty(rows, bits_, dim):
    """the same rows with a wrong header dim field and every unused bit of the last code byte set"""
    _, b, n, a, ns = mm.header(rows)
    out = mm.make_rows(mm.codes_of(rows, bits_, dim), bits_, b, n, a, ns, dim_field=dim + 3)
    assert np.array_equal(out[:, 4:], rows[:, 4:])
    used = dim * bits_ % 8
    if used:
        out[:, -1] |= np.uint8((0xFF << used) & 0xFF)
    return out


@pytest.mark.parametrize("qbits,dbits", [(1, 1), (2, 2), (4, 4), (8, 4), (8, 2), (8, 1)])
@pytest.mark.parametrize("dim", [7, 13])
def test_padding_bits_and_the_header_dim_field_are_not_read(qbits, dbits, dim):
    rng = np.random.default_rng([13, dim, qbits, dbits])
    Q, D = images(rng, 9, dim, qbits), images(rng, 35, dim, dbits)
    dQ, dD = dirty(Q, qbits, dim), dirty(D, dbits, dim)
    assert dim * dbits % 8 and not np.array_equal(dD, D)
    check_pairs(qbits, dbits, dim, [dQ], [dD], model_queries=[Q], model_docs=[D])


def batch_case(qbits, dbits):
    rng = np.random.default_rng(5)
    dim = 20
    docs = [images(rng, n, dim, dbits) for n in (4, 0, 37, 1, 9, 33)]
    queries = [images(rng, n, dim, qbits) for n in (5, 33, 0, 1)]
    cand = np.array([[2, SKIP, 0, 1, 5], [SKIP, 2, 3, 4, SKIP], [0, 1, 2, SKIP, 5], [5, 4, 3, 2, 1]], np.uint32)
    return dim, docs, queries, cand


@pytest.mark.parametrize("qbits,dbits", PAIRS)
def test_batch_plumbing(qbits, dbits):
    dim, docs, queries, cand = batch_case(qbits, dbits)
    check_pairs(qbits, dbits, dim, queries, docs, cand)


@pytest.mark.parametrize("qbits,dbits", PAIRS)
def test_device_forms_equal_host_forms(qbits, dbits):
    import torch
    import diskann_amd as da
    from diskann_amd.multivector import csr
    dim, docs, queries, cand = batch_case(qbits, dbits)
    qoff, qrows = csr(queries, np.uint8, mm.layer_bytes(qbits, dim), np.uint32)
    nq, stride, k = cand.shape[0], cand.shape[1], 7
    L = da.lib()

    def dev(a):
        return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    with da.MultiVectorSet(dt(dbits), docs, dim=dim, query_dtype=dt(qbits)) as s:
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


@pytest.mark.parametrize("qbits,dbits", PAIRS)
@pytest.mark.parametrize("order", ORDERS)
def test_chamfer_rerank(qbits, dbits, order):
    import diskann_amd as da
    rng = np.random.default_rng(61)
    dim = 12
    docs = [images(rng, n, dim, dbits) for n in (3, 7, 2, 40, 5, 1)]
    docs.append(docs[1].copy())  # document 6 == document 1: a real tie
    docs.append(docs[4].copy())  # document 7 == document 4
    queries = [images(rng, n, dim, qbits) for n in (4, 35)]
    cand = np.array([[6, 3, SKIP, 1, 0, 7, 4, 2, SKIP], [4, 7, 5, SKIP, SKIP, 1, 6, 3, 0]], np.uint32)
    with da.MultiVectorSet(dt(dbits), docs, dim=dim, query_dtype=dt(qbits)) as s:
        for k in (3, 12):  # 12 > the 7 live candidates: padding
            ids, dists, counts = s.chamfer_rerank(queries, cand, k, order=order)
            for q, Q in enumerate(queries):
                live = [int(d) for d in cand[q] if d != SKIP]
                vals = np.array([chamfer_of(scores_mm(Q, docs[d], dim, qbits, dbits), len(docs[d])) for d in live], np.float32)
                perm = np.argsort(vals, kind="stable")
                n = min(k, len(live))
                assert counts[q] == n
                assert ids[q, :n].tolist() == [live[i] for i in perm[:n]]
                assert np.array_equal(bits(dists[q, :n]), bits(vals[perm[:n]]))
                assert np.all(ids[q, n:] == SKIP) and np.all(np.isposinf(dists[q, n:]))
            if k == 12:  # the ties came back in candidate order
                assert list(ids[0]).index(6) < list(ids[0]).index(1) and list(ids[1]).index(4) < list(ids[1]).index(7)


def test_status_codes():
    import diskann_amd as da
    E = da._ffi
    L = da.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = C.c_void_p()
    off = np.array([0, 1, 4], np.uint64)
    assert L.dann_mvset_create(-1, da.U8, 8, 2, vp(off), vp(np.ones((4, 8), np.uint8)), C.byref(h)) == E.EINVAL
    assert not h.value
    assert L.dann_mvset_create(-1, da.MM8, 0, 2, vp(off), vp(np.ones((4, 28), np.uint8)), C.byref(h)) == E.EINVAL
    assert L.dann_mvset_create(-1, da.MM4, 4097, 0, vp(np.zeros(1, np.uint64)), None, C.byref(h)) == E.EUNSUPPORTED
    out = C.c_int32(-1)
    assert L.dann_mvset_set_query_dtype(None, da.MM8) == E.EINVAL
    with da.MultiVectorSet(da.F32, [np.ones((2, 8), np.float32)]) as s:
        assert s.query_dtype == da.F32
        assert L.dann_mvset_set_query_dtype(s._h, da.MM8) == E.EINVAL
        assert L.dann_mvset_set_query_dtype(s._h, da.F16) == E.EINVAL
        assert L.dann_mvset_set_query_dtype(s._h, da.F32) == 0
        assert L.dann_mvset_get_query_dtype(s._h, None) == E.EINVAL
    rng = np.random.default_rng(3)
    dim = 8
    with da.MultiVectorSet(da.MM8, [images(rng, 2, dim, 8)], dim=dim) as s:
        assert L.dann_mvset_get_query_dtype(s._h, C.byref(out)) == 0 and out.value == da.MM8  # the default: the set's
        assert L.dann_mvset_set_query_dtype(s._h, da.MM4) == E.EUNSUPPORTED
        assert L.dann_mvset_set_query_dtype(s._h, da.F32) == E.EINVAL and L.dann_mvset_set_query_dtype(s._h, da.U8) == E.EINVAL
        assert s.query_dtype == da.MM8  # a refused setting changes nothing
    with da.MultiVectorSet(da.MM4, [images(rng, 2, dim, 4)], dim=dim) as s:
        assert s.query_dtype == da.MM4
        assert L.dann_mvset_set_query_dtype(s._h, da.MM2) == E.EUNSUPPORTED
        with pytest.raises(da.DannError) as e:
            s.query_dtype = da.MM1
        assert e.value.status == E.EUNSUPPORTED
    docs = [images(rng, 1, dim, 1), images(rng, 3, dim, 1)]
    with da.MultiVectorSet(da.MM1, docs, dim=dim) as s:
        assert L.dann_mvset_set_query_dtype(s._h, da.MM8) == 0 and s.query_dtype == da.MM8
        Q = images(rng, 2, dim, 8)
        with pytest.raises(da.DannError) as e:
            s.maxsim([Q], np.array([[2]], np.uint32))  # id == ndocs
        assert e.value.status == E.EBOUNDS
        for order in ORDERS:
            assert s.maxsim([Q], [0, 1], order=order).shape == (1, 2)
        with pytest.raises(da.DannError) as e:
            s.maxsim([Q], [0], order=2)
        assert e.value.status == E.EINVAL
    with pytest.raises(ValueError):
        da.MultiVectorSet(da.MM8, docs)  # dim cannot be read off the images


def test_through_python_from_dann_minmax_compress():
    """the images dann_minmax_compress writes are the set's rows as they are"""
    import diskann_amd as da
    rng = np.random.default_rng(17)
    dim = 40
    x = (rng.standard_normal((9, dim)) * 3).astype(np.float32)
    L = da.lib()
    lb = L.dann_layer_bytes(da.MM4, dim)
    img = np.zeros((9, lb), np.uint8)
    da._ffi.check(L.dann_minmax_compress(-1, 4, x.ctypes.data_as(C.c_void_p), 9, dim, 1.0,
                                         img.ctypes.data_as(C.c_void_p), None), "dann_minmax_compress")
    assert np.array_equal(img, mm.compress(x, 4)[0])
    Q, D = img[:4], img[4:]
    with da.MultiVectorSet(da.MM4, [D, empty(4, dim)], dim=dim) as s:
        for order in ORDERS:
            ch, per_row = s.maxsim([Q], [0, 1, SKIP], order=order, per_row=True)
            w = scores_mm(Q, D, dim, 4, 4)
            assert np.array_equal(bits(per_row[0][0]), bits(w)) and bits(ch[0, 0]) == bits(chamfer_of(w, 5))
            assert np.array_equal(bits(per_row[0][1]), bits(np.full(4, F32_MAX))) and bits(ch[0, 1]) == bits(np.float32(0))
            assert np.isposinf(ch[0, 2])
