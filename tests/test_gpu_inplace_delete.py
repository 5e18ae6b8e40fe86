"""dann_inplace_delete / dann_drop_deleted_neighbors on the GPU against the CPU restatement
(tests/inplace_delete_model.py): byte-identical adjacency and equal counters for every row type, all three work-list methods,
several num_to_replace / batch / degree / dimension shapes (the matrix-core prune included), inline tags, both tie orders
on lattices, sequences mixed with drop_deleted_neighbors and consolidate, the reference's cases, searches after the repair
and the error codes."""
import numpy as np
import pytest

import oracle
from consolidate_model import consolidate
from gridutil import grid_data
from helpers import bits, make_pair, rand_vectors, random_graph
from inplace_delete_model import TIE_POSITION, TIE_RUST, drop_deleted_neighbors, inplace_delete, mark_deleted
from test_gpu_consolidate import ODT, pair, same_graph
from test_inplace_delete_host import METHODS, case_setup, check_case, load_cases, modelled

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

ONE, TWO, VTK = da.INPLACE_ONE_HOP, da.INPLACE_TWO_HOP_AND_ONE_HOP, da.INPLACE_VISITED_AND_TOPK
KL = {VTK: (10, 64)}  # VisitedAndTopK { k_value: 10, l_value: 64 }, the reference's streaming runbook
GPU_TIE = {TIE_RUST: da.TIE_RUST, TIE_POSITION: da.TIE_POSITION}
ORACLE_RULE = {TIE_RUST: oracle.DEFAULT_TIE_RULE, TIE_POSITION: oracle.POSITION_TIE_RULE}


def both(gix, oix, deleted, ids, method, ntr, pruned, R, tie=TIE_RUST, max_degree=None):
    """one call on each side -> (gpu counters, model counters)"""
    md = R if max_degree is None else max_degree
    k, l = KL.get(method, (0, 0))
    gix.set_prune_tie_order(GPU_TIE[tie])
    got = gix.inplace_delete(da.build_config(pruned, md, 50), ids, method=method, k=k, l=l, num_to_replace=ntr)
    oracle.set_tie_rule(ORACLE_RULE[tie], 0)
    try:
        want = inplace_delete(oix, oracle.build_config(pruned, md, 50), deleted, ids, method, ntr, tie, k, l)
    finally:
        oracle.set_tie_rule()
    return got, want


def assert_counters(got, want):
    assert got[:8].tolist() == want[:8].tolist(), (got, want)


ROW_CASES = [(da.F32, da.L2), (da.F32, da.INNER_PRODUCT), (da.F32, da.COSINE_NORMALIZED), (da.F16, da.L2),
             (da.F16, da.COSINE_NORMALIZED), (da.U8, da.L2), (da.U8, da.INNER_PRODUCT), (da.I8, da.L2),
             (da.I8, da.INNER_PRODUCT), (da.SQ8, da.L2), (da.SQ8, da.INNER_PRODUCT)]


# ---- 1. row types x methods ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,metric", ROW_CASES)
@pytest.mark.parametrize("method", [ONE, TWO, VTK])
def test_row_types_match_restatement(dtype, metric, method):
    rng = np.random.default_rng(300 + 10 * dtype + metric + method)
    n, dim, R = 1000, 128, 32
    oix, gix = pair(rng, dtype, metric, n, dim, R)
    deleted = np.zeros(n + 1, bool)
    ids = rng.choice(n, 16, replace=False)
    got, want = both(gix, oix, deleted, ids, method, 3, 24, R)
    assert_counters(got, want)
    assert want[7] > 0 and want[1] > 0  # prunes ran
    same_graph(gix, oix)
    assert np.array_equal(gix.get_deleted()[:n + 1], deleted.astype(np.uint8))


# ---- 2. shapes: num_to_replace, batch sizes, degree, dimension (matrix-core prunes) -------------------------------------
@pytest.mark.parametrize("ntr", [1, 3, 8])
@pytest.mark.parametrize("batch", [1, 16, 1000])
@pytest.mark.parametrize("method", [ONE, TWO, VTK])
def test_batches_and_num_to_replace(ntr, batch, method):
    rng = np.random.default_rng(1000 + ntr * 7 + batch + method)
    n, dim, R = 3000, 32, 32
    oix, gix = pair(rng, da.F32, da.L2, n, dim, R)
    deleted = np.zeros(n + 1, bool)
    ids = rng.choice(n, batch, replace=False)
    got, want = both(gix, oix, deleted, ids, method, ntr, 24, R)
    assert_counters(got, want)
    same_graph(gix, oix)


@pytest.mark.parametrize("dtype,dim,R", [(da.F32, 768, 32), (da.F32, 768, 64), (da.F32, 128, 64), (da.F16, 768, 32),
                                         (da.U8, 768, 64)])
@pytest.mark.parametrize("method", [ONE, TWO, VTK])
def test_degrees_and_dimensions(dtype, dim, R, method):
    rng = np.random.default_rng(2000 + dim + R + dtype + method)
    n = 1500
    oix, gix = pair(rng, dtype, da.L2, n, dim, R)
    deleted = np.zeros(n + 1, bool)
    ids = rng.choice(n, 64, replace=False)
    got, want = both(gix, oix, deleted, ids, method, 3, R - 8, R)
    assert_counters(got, want)
    same_graph(gix, oix)
    if dtype in (da.F32, da.F16) and dim == 768:
        assert got[8] == got[7] > 0  # 3 KiB / 1.5 KiB rows: every pruned pool went through the matrix cores
    else:
        assert got[8] == 0


def test_mfma_path_equals_row_kernel():
    rng = np.random.default_rng(77)
    n, dim, R = 1200, 768, 32
    data = rand_vectors(rng, oracle.F32, n, dim)
    adj = random_graph(rng, n, R)
    ids = rng.choice(n, 100, replace=False)
    graphs = []
    for flags in (0, da.BUILD_ROW_KERNEL_ONLY):
        oix, gix = make_pair(oracle.F32, oracle.L2, data, adj, data[:1], R)
        gix.set_build_options(flags)
        got = gix.inplace_delete(da.build_config(24, R, 50), ids, method=TWO)
        assert (got[8] > 0) == (flags == 0)
        graphs.append(gix.download_graph())
    assert np.array_equal(graphs[0], graphs[1])


# ---- 3. inline tags, tie orders ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [ONE, TWO, VTK])
def test_inline_tags_index(method):
    rng = np.random.default_rng(91 + method)
    n, dim, R = 1500, 64, 32
    data = rand_vectors(rng, oracle.F32, n, dim)
    adj = random_graph(rng, n, R)
    stride = da.lib().dann_inmem2_row_stride(da.F32, dim)
    gix = da.Provider(da.F32, da.L2, dim, n, R, data[:1], row_stride=stride, inline_tags=True)
    gix.set_elements(0, data)
    gix.upload_graph(adj)
    oix = oracle.Index(oracle.F32, oracle.L2, dim, n, R, data[:1], row_stride=stride, tags=True)
    oix.set_rows(0, data)
    oix.adj[:] = adj
    # slots that were never published are unreadable too (tag AVAILABLE)
    hidden = np.arange(n - 20, n)
    gix.set_tags(int(hidden[0]), np.zeros(hidden.size, np.uint8))
    oix.set_tags(int(hidden[0]), np.zeros(hidden.size, np.uint8))
    deleted = np.zeros(n + 1, bool)
    ids = rng.choice(n - 20, 50, replace=False)
    got, want = both(gix, oix, deleted, ids, method, 3, 24, R)
    assert_counters(got, want)
    same_graph(gix, oix)
    assert (gix.get_tags(0, n)[ids] == 2).all()
    q = rand_vectors(rng, oracle.F32, 100, dim)
    gi, gd, _ = gix.search(da.Knn(40, 1), q, 10)
    oi, od, _, _ = oix.search_batch(q, 40, 1, 10)
    assert np.array_equal(gi, oi) and np.array_equal(bits(gd), bits(od))
    assert not np.isin(gi, ids).any()


@pytest.mark.parametrize("tie", [TIE_RUST, TIE_POSITION])
@pytest.mark.parametrize("method", [ONE, TWO, VTK])
def test_tie_orders_on_lattices(tie, method):
    rng = np.random.default_rng(13 + method)
    data = grid_data(3, 8)
    n, R = data.shape[0], 16
    adj = random_graph(rng, n, R)
    oix, gix = make_pair(oracle.F32, oracle.L2, data, adj, np.full((1, 3), 4.0, np.float32), R)
    deleted = np.zeros(n + 1, bool)
    ids = rng.choice(n, 40, replace=False)
    got, want = both(gix, oix, deleted, ids, method, 3, 8, R, tie=tie)
    assert_counters(got, want)
    same_graph(gix, oix)


# ---- 4. sequences with drop_deleted_neighbors and consolidate ------------------------------------------------------------
@pytest.mark.parametrize("method", [ONE, TWO, VTK])
def test_sequence_with_drop_and_consolidate(method):
    rng = np.random.default_rng(500 + method)
    n, dim, R = 2000, 64, 32
    oix, gix = pair(rng, da.F32, da.L2, n, dim, R)
    cfg_g, cfg_o = da.build_config(24, R, 50), oracle.build_config(24, R, 50)
    deleted = np.zeros(n + 1, bool)
    order = rng.permutation(n)
    for step, (lo, hi) in enumerate([(0, 30), (30, 130), (130, 131), (131, 300)]):
        got, want = both(gix, oix, deleted, order[lo:hi], method, 3, 24, R)
        assert_counters(got, want)
        same_graph(gix, oix)
        if step == 1:
            kinds = gix.drop_deleted_neighbors(cfg_g, only_orphans=True)
            assert np.array_equal(kinds, drop_deleted_neighbors(oix, cfg_o, deleted, None, True))
            same_graph(gix, oix)
        if step == 2:
            ids = rng.choice(n + 1, 500, replace=False)
            kinds = gix.drop_deleted_neighbors(cfg_g, ids)
            assert np.array_equal(kinds, drop_deleted_neighbors(oix, cfg_o, deleted, ids, False))
            same_graph(gix, oix)
    kinds, _ = gix.consolidate(cfg_g)
    assert np.array_equal(kinds, consolidate(oix, cfg_o, deleted))
    same_graph(gix, oix)
    q = rand_vectors(rng, oracle.F32, 100, dim)
    gi, gd, gst = gix.search(da.Knn(40, 1), q, 10)
    oi, od, oc, ost = oix.search_batch(q, 40, 1, 10)
    assert np.array_equal(gi, oi) and np.array_equal(bits(gd), bits(od))


def test_drop_deleted_neighbors_after_plain_deletes():
    rng = np.random.default_rng(601)
    n, dim, R = 1500, 16, 32
    oix, gix = pair(rng, da.F32, da.L2, n, dim, R)
    deleted = np.zeros(n + 1, bool)
    dels = rng.choice(n, 200, replace=False)
    gix.delete_points(dels)
    mark_deleted(oix, deleted, dels)
    gix.upload_graph(np.where(np.isin(np.arange(n + 1), dels[:50])[:, None], 0, gix.download_graph()))
    oix.adj[dels[:50], 0] = 0
    for only_orphans in (True, False):
        kinds = gix.drop_deleted_neighbors(da.build_config(24, R, 50), only_orphans=only_orphans)
        assert np.array_equal(kinds, drop_deleted_neighbors(oix, oracle.build_config(24, R, 50), deleted, None,
                                                            only_orphans))
        same_graph(gix, oix)


# ---- 5. the reference's cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in load_cases()[0]["cases"] if modelled(c)])
@pytest.mark.parametrize("tags", [False, True])
def test_reference_cases(name, tags):
    g, cases = load_cases()
    case = cases[name]
    vec, start, lists, deg, pruned = case_setup(g, case)
    n, dim = vec.shape
    stride = da.lib().dann_inmem2_row_stride(da.F32, dim) if tags else 0
    gix = da.Provider(da.F32, da.L2, dim, n, deg, start, row_stride=stride, inline_tags=tags)
    gix.set_elements(0, vec)
    adj = np.zeros((n + 1, deg + 1), np.uint32)
    for i, ids in enumerate(lists):
        adj[i, 0] = len(ids)
        adj[i, 1:1 + len(ids)] = ids
    gix.upload_graph(adj)
    before = gix.download_graph()
    gix.inplace_delete(da.build_config(pruned, pruned, 10), case["ids"], method=METHODS[case["method"]],
                       k=case.get("k_value", 0), l=case.get("l_value", 0), num_to_replace=3)
    after = gix.download_graph()
    check_case(case, lambda v: after[v, 1:1 + after[v, 0]].tolist(), n)
    for v in case.get("unchanged", []):
        assert np.array_equal(after[v], before[v])


# ---- 6. errors: nothing changes ------------------------------------------------------------------------------------------
def test_errors_change_nothing():
    rng = np.random.default_rng(71)
    n, dim, R = 500, 16, 16
    oix, gix = pair(rng, da.F32, da.L2, n, dim, R)
    cfg = da.build_config(12, R, 50)
    gix.inplace_delete(cfg, [5, 6], method=ONE)
    graph, dels = gix.download_graph(), gix.get_deleted()

    def refused(status, *args, **kw):
        with pytest.raises(da.DannError) as e:
            gix.inplace_delete(*args, **kw)
        assert e.value.status == status
        assert np.array_equal(gix.download_graph(), graph) and np.array_equal(gix.get_deleted(), dels)

    refused(da._ffi.EBOUNDS, cfg, [7, n + 1])
    refused(da._ffi.EINVAL, cfg, [7, n])  # the start point
    refused(da._ffi.EINVAL, cfg, [7, 5])  # deleted by the earlier call
    refused(da._ffi.EINVAL, da.build_config(12, R + 1, 50), [7])
    refused(da._ffi.EINVAL, cfg, [7], method=7)
    refused(da._ffi.EINVAL, cfg, [7], method=da.INPLACE_VISITED_AND_TOPK, k=10, l=0)
    refused(da._ffi.EINVAL, cfg, [7], method=da.INPLACE_VISITED_AND_TOPK, k=0, l=64)
    with pytest.raises(da.DannError) as e:
        gix.drop_deleted_neighbors(cfg, [n + 1])
    assert e.value.status == da._ffi.EBOUNDS
    assert (gix.inplace_delete(cfg, []) == 0).all()
    # a repeated id counts once
    a = gix.inplace_delete(cfg, [9, 10, 9], method=TWO)
    assert a[0] == 2


def test_unsupported_index_type():
    rng = np.random.default_rng(72)
    dim, nch = 16, 4
    piv = rng.standard_normal((256, dim)).astype(np.float32)
    offs = np.array([0, 4, 8, 12, 16], np.uint32)
    gix = da.Provider(da.PQ, da.L2, dim, 100, 16, np.zeros((1, nch), np.uint8), pq_pivots=piv, pq_offsets=offs)
    with pytest.raises(da.DannError) as e:
        gix.inplace_delete(da.build_config(8, 16, 20), [1])
    assert e.value.status == da._ffi.EUNSUPPORTED


def test_refused_call_leaves_tags_alone():
    """an inline_tags index: a refused call changes neither tags, marks nor rows"""
    rng = np.random.default_rng(73)
    n, dim, R = 400, 16, 16
    data = rand_vectors(rng, oracle.F32, n, dim)
    stride = da.lib().dann_inmem2_row_stride(da.F32, dim)
    gix = da.Provider(da.F32, da.L2, dim, n, R, data[:1], row_stride=stride, inline_tags=True)
    gix.set_elements(0, data)
    gix.upload_graph(random_graph(rng, n, R))
    cfg = da.build_config(12, R, 50)
    gix.inplace_delete(cfg, [3], method=VTK, k=10, l=32)
    tags, graph, dels = gix.get_tags(0, n + 1), gix.download_graph(), gix.get_deleted()
    assert tags[3] == 2 and dels[3] == 1
    for bad in ([4, 3], [4, n + 1], [4, n]):
        with pytest.raises(da.DannError):
            gix.inplace_delete(cfg, bad, method=TWO)
        assert np.array_equal(gix.get_tags(0, n + 1), tags) and np.array_equal(gix.download_graph(), graph)
        assert np.array_equal(gix.get_deleted(), dels)
