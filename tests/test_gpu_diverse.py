"""dann_diverse_search_batch on the GPU: equal to dann_search_batch where the diverse queue is the plain queue, and equal
to the CPU restatement (tests/diverse_model.py) in ids, distance bits, hops, cmps and result_count over row types,
metrics, attribute cardinalities, missing attributes, diverse_k, L, W, dims and degrees; lattices whose ties make the
queue's removes fail; start points without attributes; the exact global-memory re-run; inline tags; launches of more
than one chunk; the kernel family; the error codes."""
import numpy as np
import pytest

import oracle
from diverse_model import NO_ATTRIBUTE, diverse_search
from gridutil import grid_data, grid_neighbors
from helpers import bits, make_pair, rand_vectors, random_graph

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

ODT = {da.F32: oracle.F32, da.F16: oracle.F16, da.U8: oracle.U8, da.I8: oracle.I8}


def sq8_pair(rng, metric, n, dim, R, adj):
    data = rng.normal(0.3, 0.5, (n, dim)).astype(np.float32)
    shift = (data.mean(0) - 2.0 * data.std(0)).astype(np.float32)
    scale = float(np.float32(4.0 * data.std()))
    codes = da.sq8_compress(data, shift, scale)
    snorm = float(np.float32((shift.astype(np.float32) ** 2).sum(dtype=np.float32)))
    oix = oracle.Index(oracle.SQ8, metric, dim, n, R, codes[:1], sq_scale=scale, sq_shift_norm_sq=snorm)
    oix.set_rows(0, codes)
    oix.adj[:] = adj
    gix = da.Provider(da.SQ8, metric, dim, n, R, codes[:1], sq_scale=scale, sq_shift_norm_sq=snorm)
    gix.set_elements(0, codes)
    gix.upload_graph(adj)
    return oix, gix, codes


def pair(rng, dtype, metric, n, dim, R):
    adj = random_graph(rng, n, R)
    if dtype == da.SQ8:
        return sq8_pair(rng, metric, n, dim, R, adj)
    x = rand_vectors(rng, ODT[dtype], n, dim)
    if metric == da.COSINE_NORMALIZED:
        x = (x.astype(np.float32) / np.linalg.norm(x.astype(np.float32), axis=1, keepdims=True)).astype(x.dtype)
    oix, gix = make_pair(ODT[dtype], metric, x, adj, x[:1], R)
    return oix, gix, x


def queries_for(rng, dtype, data, nq):
    if dtype == da.SQ8:
        return data[rng.choice(data.shape[0], nq)]
    return rand_vectors(rng, ODT[dtype], nq, data.shape[1])


def make_attrs(rng, nslots, cardinality, missing):
    """attributes of every slot, a fraction `missing` of them none; the start point (the last slot) keeps one unless
    every slot is missing (a start point without one ends the search at once: test_start_point_without_attribute)"""
    a = (np.arange(nslots, dtype=np.uint32) if cardinality is None
         else rng.integers(0, cardinality, nslots).astype(np.uint32))
    a[rng.random(nslots) < missing] = NO_ATTRIBUTE
    if missing < 1.0:
        a[-1] = nslots - 1 if cardinality is None else 0
    return a


def check_model(gix, oix, q, L, W, k, dk, tk, attrs, tag):
    gi, gd, gst = gix.diverse_search(da.Knn(L, W), q, k, dk, tk)
    failed = np.zeros(2, np.int64)
    for j in range(q.shape[0]):
        ids, dists, count, cmps, hops, fr = diverse_search(oix, q[j], L, W, k, dk, tk, attrs)
        n = len(ids)
        assert gi[j, :n].tolist() == ids, (tag, j)
        assert np.array_equal(bits(gd[j, :n]), bits(dists)), (tag, j)
        assert (gi[j, n:] == 0xFFFFFFFF).all() and np.isinf(gd[j, n:]).all(), (tag, j)
        assert (int(gst["cmps"][j]), int(gst["hops"][j]), int(gst["result_count"][j])) == (cmps, hops, count), (tag, j)
        failed += fr
    if attrs[oix.capacity] != NO_ATTRIBUTE:  # (a start point without an attribute ends every search at once)
        assert (gst["written"] > 0).any(), tag
    return failed


ROW_CASES = [(da.F32, da.L2), (da.F32, da.INNER_PRODUCT), (da.F32, da.COSINE_NORMALIZED), (da.F16, da.L2),
             (da.F16, da.COSINE_NORMALIZED), (da.U8, da.L2), (da.U8, da.INNER_PRODUCT), (da.I8, da.L2),
             (da.I8, da.COSINE_NORMALIZED), (da.SQ8, da.L2), (da.SQ8, da.INNER_PRODUCT)]


@pytest.mark.parametrize("dtype,metric", ROW_CASES)
def test_row_types_match_model(dtype, metric):
    rng = np.random.default_rng(10 * dtype + metric)
    n, dim, R = 3000, 128, 32
    oix, gix, data = pair(rng, dtype, metric, n, dim, R)
    attrs = make_attrs(rng, n + 1, 7, 0.3)
    gix.set_attributes(0, attrs)
    assert np.array_equal(gix.get_attributes(), attrs)
    q = queries_for(rng, dtype, data, 12)
    check_model(gix, oix, q, 40, 1, 10, 2, 10, attrs, (dtype, metric))
    check_model(gix, oix, q, 40, 4, 10, 1, 10, attrs, (dtype, metric, "W4"))


@pytest.mark.parametrize("cardinality", [1, 2, 7, 100, None])
@pytest.mark.parametrize("missing", [0.0, 0.3, 1.0])
def test_cardinality_and_missing(cardinality, missing):
    rng = np.random.default_rng(7 + (cardinality or 0) + int(missing * 10))
    n, dim, R = 2000, 32, 32
    oix, gix, data = pair(rng, da.F32, da.L2, n, dim, R)
    attrs = make_attrs(rng, n + 1, cardinality, missing)
    gix.set_attributes(0, attrs)
    q = queries_for(rng, da.F32, data, 8)
    for L, W, dk, tk in ((10, 1, 1, 10), (40, 1, 2, 10), (40, 4, 10, 10), (10, 4, 2, 10), (30, 1, 3, 5)):
        check_model(gix, oix, q, L, W, 10, dk, tk, attrs, (cardinality, missing, L, W, dk))


@pytest.mark.parametrize("dim,R", [(768, 32), (128, 64), (768, 64)])
def test_dims_and_degrees(dim, R):
    rng = np.random.default_rng(dim + R)
    n = 2000
    oix, gix, data = pair(rng, da.F32, da.L2, n, dim, R)
    attrs = make_attrs(rng, n + 1, 7, 0.3)
    gix.set_attributes(0, attrs)
    q = queries_for(rng, da.F32, data, 8)
    check_model(gix, oix, q, 40, 1, 10, 2, 10, attrs, (dim, R))
    check_model(gix, oix, q, 40, 4, 10, 1, 10, attrs, (dim, R, 4))


@pytest.mark.parametrize("dtype", [da.F32, da.U8])
def test_unique_attributes_equal_plain_search(dtype):
    """every slot its own attribute, diverse_k == total_k: every local queue holds one entry and the diverse queue acts
    as the plain queue of the same length (diverse L = plain L + the start point) -- except that a candidate equal to a
    full queue's last entry is dropped by the diverse queue (case 3 is strict) and kept by the plain one.  f32 rows:
    bit-identical for every query; u8 rows: for every query where the CPU restatement and the oracle's Knn agree"""
    rng = np.random.default_rng(3 + dtype)
    n, dim, R = 4000, 128, 32
    oix, gix, data = pair(rng, dtype, da.L2, n, dim, R)
    attrs = np.arange(n + 1, dtype=np.uint32)
    gix.set_attributes(0, attrs)
    q = queries_for(rng, dtype, data, 64)
    for L, W in ((20, 1), (64, 4)):
        pi, pd, pst = gix.search(da.Knn(L - 1, W), q, 10)
        gi, gd, gst = gix.diverse_search(da.Knn(L, W), q, 10, 10, 10)
        rows = np.arange(q.shape[0])
        if dtype != da.F32:
            agree = []
            for j in range(q.shape[0]):
                ids, dists, count, cmps, hops, _ = diverse_search(oix, q[j], L, W, 10, 10, 10, attrs)
                n_, oi, od, ost = oix.search(q[j], L - 1, W, 10)
                if ids == oi[:len(ids)].tolist() and (cmps, hops) == (int(ost[0]), int(ost[1])):
                    agree.append(j)
            assert len(agree) >= q.shape[0] // 2, len(agree)
            rows = np.array(agree)
        assert np.array_equal(gi[rows], pi[rows]) and np.array_equal(bits(gd[rows]), bits(pd[rows]))
        for f in ("cmps", "hops", "result_count"):
            assert np.array_equal(gst[f][rows], pst[f][rows]), f


def lattice_pair(dims, size, rng):
    pts = grid_data(dims, size).astype(np.uint8)
    n = pts.shape[0]
    R = 2 * dims + 2
    lists = grid_neighbors(dims, size)
    adj = np.zeros((n + 1, R + 1), np.uint32)
    for i, nb in enumerate(lists):
        extra = [int(x) for x in rng.choice(n, 2, replace=False)]
        nb = nb + [x for x in extra if x not in nb and x != i]
        adj[i, 0] = len(nb)
        adj[i, 1:1 + len(nb)] = nb
    adj[n, 0] = 1
    adj[n, 1] = n - 1
    start = np.full((1, dims), size, np.uint8)
    oix, gix = make_pair(oracle.U8, da.L2, pts, adj, start, R)
    return oix, gix, pts


def test_lattice_ties_reach_failed_removes():
    """integer lattice rows: distances tie all the time, so NeighborPriorityQueue::remove fails in both case 2 (global
    queue) and case 3 (local queue) -- the GPU must keep the same diverged state as the reference"""
    rng = np.random.default_rng(5)
    oix, gix, pts = lattice_pair(3, 10, rng)
    n = pts.shape[0]
    attrs = make_attrs(rng, n + 1, 3, 0.1)
    gix.set_attributes(0, attrs)
    q = rng.integers(0, 10, (24, 3)).astype(np.uint8)
    failed = check_model(gix, oix, q, 12, 1, 10, 3, 4, attrs, "lattice W1")
    failed += check_model(gix, oix, q, 20, 2, 10, 4, 5, attrs, "lattice W2")
    failed += check_model(gix, oix, q, 20, 1, 10, 2, 10, attrs, "lattice dk 2")
    assert failed[0] > 0 and failed[1] > 0, failed


def test_start_point_without_attribute_gives_nothing():
    rng = np.random.default_rng(11)
    n, dim, R = 1000, 32, 32
    oix, gix, data = pair(rng, da.F32, da.L2, n, dim, R)
    q = queries_for(rng, da.F32, data, 16)
    # no attribute store at all: the reference's provider returns None for every id
    gi, gd, gst = gix.diverse_search(da.Knn(20, 1), q, 10, 2, 10)
    assert (gi == 0xFFFFFFFF).all() and np.isinf(gd).all()
    assert (gst["result_count"] == 0).all() and (gst["hops"] == 0).all() and (gst["cmps"] == 1).all()
    # every slot has one but the start point
    attrs = make_attrs(rng, n + 1, 5, 0.0)
    attrs[n] = NO_ATTRIBUTE
    gix.set_attributes(0, attrs)
    gi, gd, gst = gix.diverse_search(da.Knn(20, 1), q, 10, 2, 10)
    assert (gi == 0xFFFFFFFF).all() and (gst["hops"] == 0).all()


def test_global_memory_rerun_equals_default():
    """DANN_DBG_DIVERSE_POOL shrinks the LDS pool so that most queries overflow it and run again with their scratch in
    global memory: same answers"""
    rng = np.random.default_rng(13)
    n, dim, R = 3000, 64, 32
    oix, gix, data = pair(rng, da.F32, da.L2, n, dim, R)
    attrs = make_attrs(rng, n + 1, 100, 0.2)
    gix.set_attributes(0, attrs)
    q = queries_for(rng, da.F32, data, 200)
    ref = gix.diverse_search(da.Knn(64, 2), q, 10, 1, 10)
    gix.kernel_time_reset()
    gix.debug_set(diverse_pool=8)
    small = gix.diverse_search(da.Knn(64, 2), q, 10, 1, 10)
    _, reruns = gix.kernel_time(4)
    gix.debug_set(diverse_pool=None)
    assert reruns > 0 and (ref[2]["written"] > 0).all()
    assert np.array_equal(small[0], ref[0]) and np.array_equal(bits(small[1]), bits(ref[1]))
    for f in ("cmps", "hops", "result_count"):
        assert np.array_equal(small[2][f], ref[2][f])
    check_model(gix, oix, q[:6], 64, 2, 10, 1, 10, attrs, "rerun")


def test_inline_tags_skip_deleted():
    rng = np.random.default_rng(17)
    n, dim, R = 2000, 32, 32
    data = rand_vectors(rng, oracle.F32, n, dim)
    adj = random_graph(rng, n, R)
    stride = da.lib().dann_inmem2_row_stride(da.F32, dim)
    gix = da.Provider(da.F32, da.L2, dim, n, R, data[:1], row_stride=stride, inline_tags=True)
    gix.set_elements(0, data)
    gix.upload_graph(adj)
    oix = oracle.Index(oracle.F32, da.L2, dim, n, R, data[:1], row_stride=stride, tags=True)
    oix.set_rows(0, data)
    oix.adj[:] = adj
    dels = rng.choice(n, 300, replace=False)
    gix.delete_points(dels)
    oix.set_tags(0, gix.get_tags(0, n))
    attrs = make_attrs(rng, n + 1, 7, 0.1)
    gix.set_attributes(0, attrs)
    q = data[:10] + 0.01
    check_model(gix, oix, q, 40, 2, 10, 2, 10, attrs, "tags")
    gi, _, _ = gix.diverse_search(da.Knn(40, 2), q, 10, 2, 10)
    assert not np.isin(gi, dels).any()


def test_many_queries_cross_chunks():
    rng = np.random.default_rng(19)
    n, dim, R = 4000, 32, 32
    oix, gix, data = pair(rng, da.F32, da.L2, n, dim, R)
    attrs = make_attrs(rng, n + 1, 20, 0.1)
    gix.set_attributes(0, attrs)
    q = queries_for(rng, da.F32, data, 70000)  # the host path runs 65 536 queries per launch
    gix.kernel_time_reset()
    (gi, gd, gst), fam = gix.last_family(lambda: gix.diverse_search(da.Knn(20, 1), q, 10, 3, 10))
    assert fam == {"diverse"}
    assert (gst["written"] > 0).mean() > 0.9
    _, launches = gix.kernel_time(0)
    assert launches >= 2
    for j in list(range(4)) + list(range(65530, 65540)) + [69999]:
        ids, dists, count, cmps, hops, _ = diverse_search(oix, q[j], 20, 1, 10, 3, 10, attrs)
        assert gi[j, :len(ids)].tolist() == ids and np.array_equal(bits(gd[j, :len(ids)]), bits(dists))
        assert (int(gst["cmps"][j]), int(gst["hops"][j]), int(gst["result_count"][j])) == (cmps, hops, count)
    # each query's answer is independent of its batch
    sub = gix.diverse_search(da.Knn(20, 1), q[65530:65540], 10, 3, 10)
    assert np.array_equal(sub[0], gi[65530:65540])


def test_errors():
    rng = np.random.default_rng(23)
    n, dim, R = 500, 16, 16
    oix, gix, data = pair(rng, da.F32, da.L2, n, dim, R)
    q = queries_for(rng, da.F32, data, 4)
    for L, dk, tk in ((20, 2, 0), (20, 0, 10), (20, 11, 10), (9, 2, 10)):
        with pytest.raises(da.DannError) as e:
            gix.diverse_search(da.Knn(L, 1), q, 10, dk, tk)
        assert e.value.status == da._ffi.EINVAL, (L, dk, tk)
    with pytest.raises(da.DannError) as e:
        gix.set_attributes(n, np.zeros(2, np.uint32))
    assert e.value.status == da._ffi.EBOUNDS
    with pytest.raises(da.DannError) as e:
        gix.get_attributes(n, 2)
    assert e.value.status == da._ffi.EBOUNDS
    gix.set_attributes(n, np.zeros(1, np.uint32))  # the start point's slot is in range
    piv = rng.standard_normal((256, dim)).astype(np.float32)
    offs = np.array([0, 4, 8, 12, 16], np.uint32)
    pq = da.Provider(da.PQ, da.L2, dim, 100, 16, np.zeros((1, 4), np.uint8), pq_pivots=piv, pq_offsets=offs)
    with pytest.raises(da.DannError) as e:
        pq.diverse_search(da.Knn(20, 1), q, 10, 2, 10)
    assert e.value.status == da._ffi.EUNSUPPORTED
