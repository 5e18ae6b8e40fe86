"""dann_delete_points / dann_consolidate on the GPU against the CPU restatement (tests/consolidate_model.py): the
reference's consolidate.rs known answers, random graphs of every row type with byte-identical adjacency and equal kinds,
both tie orders on lattices, the matrix-core prune path, subsets, searches after consolidation and the error cases."""
import numpy as np
import pytest

import oracle
from consolidate_model import consolidate
from gridutil import grid_data
from helpers import bits, make_pair, rand_vectors, random_graph
from test_consolidate_host import _cases, deleted_mask, square_cfg, square_index

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

ODT = {da.F32: oracle.F32, da.F16: oracle.F16, da.U8: oracle.U8, da.I8: oracle.I8}


def valid_rows(adj, R):
    """[len, ids[:len]] of every row (entries behind a list's end are not part of the graph)"""
    out = adj.copy()
    for r in range(out.shape[0]):
        out[r, 1 + min(int(out[r, 0]), R):] = 0
    return out


def same_graph(gix, oix):
    g = valid_rows(gix.download_graph(), gix.max_degree)
    o = valid_rows(oix.adj, gix.max_degree)
    bad = np.flatnonzero((g != o).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}: gpu {g[bad[0]][:12]} oracle {o[bad[0]][:12]}"


def data_for(rng, dtype, metric, n, dim):
    x = rand_vectors(rng, ODT[dtype], n, dim)
    if metric == da.COSINE_NORMALIZED:
        x = (x.astype(np.float32) / np.linalg.norm(x.astype(np.float32), axis=1, keepdims=True)).astype(x.dtype)
    return x


def sq8_pair(rng, metric, n, dim, R, adj):
    """SQ-8 rows and quantiser parameters as tests/test_gpu_quant.py builds them"""
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
    return oix, gix


def pair(rng, dtype, metric, n, dim, R, adj=None):
    if adj is None:
        adj = random_graph(rng, n, R)
    if dtype == da.SQ8:
        return sq8_pair(rng, metric, n, dim, R, adj)
    data = data_for(rng, dtype, metric, n, dim)
    return make_pair(ODT[dtype], metric, data, adj, data[:1], R)


def delete_both(gix, rng, n, frac, extra=()):
    deleted = np.zeros(gix.capacity + gix.num_start_points, bool)
    k = int(round(frac * n))
    if k:
        deleted[rng.choice(n, k, replace=False)] = True
    deleted[list(extra)] = True
    if deleted.any():
        gix.delete_points(np.flatnonzero(deleted))
    return deleted


# ---- 1. the reference's known answers -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in _cases()[0]["cases"]])
def test_known_answers(name):
    g, cases = _cases()
    case = cases[name]
    oix, deg = square_index(g, case)
    gix = da.Provider(da.F32, da.L2, 2, 4, deg, np.array(g["start_point"], np.float32))
    gix.set_elements(0, np.array(g["vectors"], np.float32))
    gix.upload_graph(oix.adj)
    if case["deleted"]:
        gix.delete_points(case["deleted"])
    assert np.array_equal(gix.get_deleted().astype(bool), deleted_mask(oix, case))
    cfg = da.build_config(case["pruned_degree"], case["pruned_degree"], 10)
    kinds, _ = gix.consolidate(cfg, case["ids"])
    assert kinds.tolist() == case["kinds"]
    for v, want in case["expected_sorted"].items():
        assert sorted(gix.get_neighbors(int(v)).tolist()) == want, v
    for v, m in case.get("max_len", {}).items():
        assert 0 < len(gix.get_neighbors(int(v))) <= m
    consolidate(oix, square_cfg(case), deleted_mask(oix, case), case["ids"])
    same_graph(gix, oix)


# ---- 2. random graphs against the restatement ------------------------------------------------------------------------
ROW_CASES = [(da.F32, da.L2), (da.F32, da.INNER_PRODUCT), (da.F32, da.COSINE_NORMALIZED), (da.F16, da.L2),
             (da.F16, da.INNER_PRODUCT), (da.F16, da.COSINE_NORMALIZED), (da.U8, da.L2), (da.U8, da.INNER_PRODUCT),
             (da.I8, da.L2), (da.I8, da.INNER_PRODUCT), (da.SQ8, da.L2), (da.SQ8, da.INNER_PRODUCT),
             (da.SQ8, da.COSINE_NORMALIZED)]


@pytest.mark.parametrize("dtype,metric", ROW_CASES)
@pytest.mark.parametrize("frac", [0.0, 0.01, 0.1, 0.5])
def test_random_graph_matches_restatement(dtype, metric, frac):
    rng = np.random.default_rng(100 + 10 * dtype + metric + int(frac * 1000))
    n, dim, R = 1200, 128, 32
    oix, gix = pair(rng, dtype, metric, n, dim, R)
    deleted = delete_both(gix, rng, n, frac)
    cfg = da.build_config(24, R, 50)
    kinds, cnt = gix.consolidate(cfg)
    want = consolidate(oix, oracle.build_config(24, R, 50), deleted)
    assert np.array_equal(kinds, want)
    same_graph(gix, oix)
    assert cnt[0] == n + 1 and cnt[2] > 0


@pytest.mark.parametrize("dtype,dim,R", [(da.F32, 768, 64), (da.F16, 768, 32), (da.F16, 128, 64), (da.U8, 768, 32),
                                         (da.SQ8, 768, 64)])
@pytest.mark.parametrize("frac", [0.01, 0.1, 0.5])
def test_random_graph_other_shapes(dtype, dim, R, frac):
    rng = np.random.default_rng(7 + dim + R + int(frac * 100))
    n = 800
    oix, gix = pair(rng, dtype, da.L2, n, dim, R)
    deleted = delete_both(gix, rng, n, frac)
    kinds, _ = gix.consolidate(da.build_config(R - 8, R, 50))
    assert np.array_equal(kinds, consolidate(oix, oracle.build_config(R - 8, R, 50), deleted))
    same_graph(gix, oix)


def test_corner_cases():
    """every neighbour deleted; deleted neighbours whose lists hold deleted ids; a pool of exactly pruned_degree; a pool
    at its largest size (R = 64, all 64 neighbours deleted, their lists disjoint: 64 x 64 = 4096 candidates)"""
    rng = np.random.default_rng(3)
    R, n, dim = 64, 4300, 32
    adj = random_graph(rng, n, R)
    deleted = np.zeros(n + 1, bool)
    # vertex 0: all neighbours deleted (1..64), their lists disjoint live ids (65 + 64 k ..)
    adj[0, 0] = R
    adj[0, 1:R + 1] = np.arange(1, R + 1)
    deleted[1:R + 1] = True
    for k in range(R):
        adj[1 + k, 0] = R
        adj[1 + k, 1:R + 1] = 65 + 64 * k + np.arange(R)
    live = np.arange(65 + 64 * R, n)
    # vertex live[0]: one deleted neighbour whose list holds deleted ids only besides two live ones
    v = int(live[0])
    adj[v, 0] = 3
    adj[v, 1:4] = [1, int(live[1]), int(live[2])]
    # vertex live[3]: pool of exactly pruned_degree (16): 15 live + one deleted neighbour contributing one new live id
    w, pd = int(live[3]), 16
    adj[w, 0] = 16
    d2 = int(live[30])
    deleted[d2] = True
    adj[w, 1:17] = list(live[10:25]) + [d2]
    adj[d2, 0] = 3
    adj[d2, 1:4] = [3, 4, int(live[40])]
    data = data_for(rng, da.F32, da.L2, n, dim)
    oix, gix = make_pair(oracle.F32, oracle.L2, data, adj, data[:1], R)
    gix.delete_points(np.flatnonzero(deleted))
    kinds, cnt = gix.consolidate(da.build_config(pd, R, 50))
    assert np.array_equal(kinds, consolidate(oix, oracle.build_config(pd, R, 50), deleted))
    same_graph(gix, oix)
    assert cnt[3] == R * R
    assert len(gix.get_neighbors(0)) <= pd and not deleted[gix.get_neighbors(0)].any()


# ---- 3. both tie orders on integer lattices ------------------------------------------------------------------------------
@pytest.mark.parametrize("gpu_order,rule", [(da.TIE_RUST, oracle.DEFAULT_TIE_RULE), (da.TIE_POSITION, oracle.POSITION_TIE_RULE)])
def test_tie_orders_on_lattices(gpu_order, rule):
    rng = np.random.default_rng(11)
    data = grid_data(3, 8)
    n, R = data.shape[0], 16
    adj = random_graph(rng, n, R)
    oix, gix = make_pair(oracle.F32, oracle.L2, data, adj, np.full((1, 3), 4.0, np.float32), R)
    gix.set_prune_tie_order(gpu_order)
    deleted = delete_both(gix, rng, n, 0.3)
    kinds, _ = gix.consolidate(da.build_config(8, R, 50))
    oracle.set_tie_rule(rule, 0)
    try:
        want = consolidate(oix, oracle.build_config(8, R, 50), deleted)
    finally:
        oracle.set_tie_rule()
    assert np.array_equal(kinds, want)
    same_graph(gix, oix)


# ---- 4. the matrix-core prune path --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [da.F32, da.F16])
def test_mfma_path_equals_row_kernel(dtype):
    rng = np.random.default_rng(21 + dtype)
    n, dim, R = 1000, 768, 32
    data = data_for(rng, dtype, da.L2, n, dim)
    adj = random_graph(rng, n, R)
    graphs = []
    for flags in (0, da.BUILD_ROW_KERNEL_ONLY):
        oix, gix = make_pair(ODT[dtype], oracle.L2, data, adj, data[:1], R)
        gix.set_build_options(flags)
        d = delete_both(gix, np.random.default_rng(5), n, 0.1)
        before = gix.build_counters()
        _, cnt = gix.consolidate(da.build_config(24, R, 50))
        after = gix.build_counters()
        if flags == 0:
            assert after[6] > before[6] and after[7] > before[7] and cnt[5] == cnt[2] > 0
            consolidate(oix, oracle.build_config(24, R, 50), d)
            same_graph(gix, oix)
        else:
            assert after[6] == before[6] and cnt[5] == 0
        graphs.append(valid_rows(gix.download_graph(), R))
    assert np.array_equal(graphs[0], graphs[1])


# ---- 5. subsets and repeats ---------------------------------------------------------------------------------------------
def test_subsets_then_rest_equal_one_call_and_repeat_is_noop():
    rng = np.random.default_rng(31)
    n, dim, R = 1500, 64, 32
    data = data_for(rng, da.F32, da.L2, n, dim)
    adj = random_graph(rng, n, R)
    cfg = da.build_config(24, R, 50)
    _, g1 = make_pair(oracle.F32, oracle.L2, data, adj, data[:1], R)
    _, g2 = make_pair(oracle.F32, oracle.L2, data, adj, data[:1], R)
    dels = rng.choice(n, 150, replace=False)
    g1.delete_points(dels)
    g2.delete_points(dels)
    g1.consolidate(cfg)
    order = rng.permutation(n + 1)
    part = np.concatenate([order[:500], order[:40]])  # a repeated id is consolidated once
    k2a, _ = g2.consolidate(cfg, part)
    k2b, _ = g2.consolidate(cfg, order[500:])
    assert np.array_equal(valid_rows(g1.download_graph(), R), valid_rows(g2.download_graph(), R))
    assert (k2a[np.isin(part, dels)] == da.CONSOLIDATE_DELETED).all() and (k2a[~np.isin(part, dels)] == 0).all()
    raw = g1.download_graph()
    kinds, cnt = g1.consolidate(cfg)
    assert np.array_equal(g1.download_graph(), raw) and cnt[1] == 0 and cnt[2] == 0
    assert np.array_equal(np.flatnonzero(kinds), np.sort(dels))


# ---- 6. after consolidation ---------------------------------------------------------------------------------------------
def test_no_live_list_points_at_deleted_and_search_matches_oracle():
    rng = np.random.default_rng(41)
    n, dim, R = 3000, 128, 32
    oix, gix = pair(rng, da.F32, da.L2, n, dim, R)
    deleted = delete_both(gix, rng, n, 0.1)
    gix.consolidate(da.build_config(24, R, 50))
    consolidate(oix, oracle.build_config(24, R, 50), deleted)
    same_graph(gix, oix)
    g = gix.download_graph()
    for v in np.flatnonzero(~deleted):
        assert not deleted[g[v, 1:1 + g[v, 0]]].any(), v
    q = rand_vectors(rng, oracle.F32, 200, dim)
    gi, gd, gst = gix.search(da.Knn(40, 1), q, 10)
    oi, od, oc, ost = oix.search_batch(q, 40, 1, 10)
    assert np.array_equal(gi, oi) and np.array_equal(bits(gd), bits(od))
    assert np.array_equal(gst["cmps"], ost[:, 0]) and np.array_equal(gst["hops"], ost[:, 1])


def test_inline_tags_searches_skip_deleted_at_once():
    rng = np.random.default_rng(51)
    n, dim, R = 2000, 32, 32
    data = rand_vectors(rng, oracle.F32, n, dim)
    adj = random_graph(rng, n, R)
    stride = da.lib().dann_inmem2_row_stride(da.F32, dim)
    gix = da.Provider(da.F32, da.L2, dim, n, R, data[:1], row_stride=stride, inline_tags=True)
    gix.set_elements(0, data)
    gix.upload_graph(adj)
    q = data[:50] + 0.0
    ids0, _, _ = gix.search(da.Knn(40, 1), q, 10)
    assert np.isin(ids0, np.arange(50)).any()
    gix.delete_points(np.arange(50))
    assert (gix.get_tags(0, 50) == 2).all() and (gix.get_tags(50, 10) == 254).all()
    ids1, _, _ = gix.search(da.Knn(40, 1), q, 10)
    assert not np.isin(ids1, np.arange(50)).any()


# ---- 7. DROP_DELETED, errors, no-op --------------------------------------------------------------------------------------
def test_drop_deleted_errors_and_untouched_index():
    rng = np.random.default_rng(61)
    n, dim, R = 600, 16, 16
    oix, gix = pair(rng, da.F32, da.L2, n, dim, R, adj=random_graph(rng, n, R, min_len=4))
    cfg = da.build_config(16, R, 50)  # lists are never longer than pruned_degree
    raw = gix.download_graph()
    kinds, cnt = gix.consolidate(cfg)
    assert np.array_equal(gix.download_graph(), raw) and (kinds == 0).all() and cnt[1] == cnt[2] == 0
    assert not gix.get_deleted().any()
    with pytest.raises(da.DannError) as e:
        gix.delete_points([n])  # the start point
    assert e.value.status == da._ffi.EINVAL
    with pytest.raises(da.DannError) as e:
        gix.delete_points([n + 1])
    assert e.value.status == da._ffi.EBOUNDS
    with pytest.raises(da.DannError) as e:
        gix.consolidate(cfg, [n + 1])
    assert e.value.status == da._ffi.EBOUNDS
    assert not gix.get_deleted().any()
    dels = np.arange(0, n, 7)
    gix.delete_points(dels)
    gix.delete_points(dels[:3])  # twice is fine
    gix.consolidate(cfg, drop_deleted=True)
    g = gix.download_graph()
    assert (g[dels, 0] == 0).all()
    d = np.zeros(n + 1, bool)
    d[dels] = True
    consolidate(oix, oracle.build_config(16, R, 50), d, drop_deleted=True)
    same_graph(gix, oix)


def test_unsupported_index_type():
    rng = np.random.default_rng(71)
    dim, nch = 16, 4
    piv = rng.standard_normal((256, dim)).astype(np.float32)
    offs = np.array([0, 4, 8, 12, 16], np.uint32)
    gix = da.Provider(da.PQ, da.L2, dim, 100, 16, np.zeros((1, nch), np.uint8), pq_pivots=piv, pq_offsets=offs)
    gix.delete_points([3])
    with pytest.raises(da.DannError) as e:
        gix.consolidate(da.build_config(8, 16, 20))
    assert e.value.status == da._ffi.EUNSUPPORTED


# ---- pools of more than 4096 candidates (max_degree > 64) --------------------------------------------------------------
@pytest.mark.parametrize("gpu_order,rule", [(da.TIE_RUST, oracle.DEFAULT_TIE_RULE), (da.TIE_POSITION, oracle.POSITION_TIE_RULE)])
def test_degree_128_half_deleted(gpu_order, rule):
    """R = 128 with half the points deleted: unique pools far beyond the 4096 candidates of the LDS path take the global
    gather and the exact selection of the max_occlusion_size nearest; the lists equal the restatement's.  The vertices
    checked are a sample (the restatement evaluates every pool distance one call at a time)."""
    rng = np.random.default_rng(81)
    n, dim, R = 20000, 8, 128
    adj = np.zeros((n + 1, R + 1), np.uint32)  # full lists, ids drawn with repetition (duplicates are part of the test)
    adj[:, 0] = R
    adj[:, 1:] = rng.integers(0, n, (n + 1, R))
    deleted = np.zeros(n + 1, bool)
    deleted[rng.choice(n, n // 2, replace=False)] = True
    live, dead = np.flatnonzero(~deleted[:n]), np.flatnonzero(deleted[:n])
    # 24 checked vertices: half their list deleted, each deleted neighbour listing live points only -> ~5 600 unique
    for k, v in enumerate(live[:24]):
        dn = dead[64 * k: 64 * (k + 1)]
        adj[v, 1:] = np.concatenate([rng.choice(live, 64, replace=False), dn])
        adj[dn, 1:] = rng.choice(live, (64, R))
    oix, gix = pair(rng, da.F32, da.L2, n, dim, R, adj=adj)
    gix.set_prune_tie_order(gpu_order)
    gix.delete_points(dead)
    ids = np.concatenate([live[:24], dead[:4]]).astype(np.uint32)
    cfg = da.build_config(96, R, 50)
    kinds, cnt = gix.consolidate(cfg, ids)
    oracle.set_tie_rule(rule, 0)
    try:
        want = consolidate(oix, oracle.build_config(96, R, 50), deleted, ids)
    finally:
        oracle.set_tie_rule()
    assert np.array_equal(kinds, want)
    assert cnt[3] > 4096 and cnt[6] == 24
    g = gix.download_graph()
    differ = [int(v) for v in ids[:24]
              if int(g[v, 0]) != int(oix.adj[v, 0]) or not np.array_equal(g[v, 1:1 + g[v, 0]], oix.adj[v, 1:1 + g[v, 0]])]
    if gpu_order == da.TIE_POSITION:
        assert cnt[7] == 0 and not differ, differ
    else:
        # f32 distances do tie among the ~750 nearest of ~5 600 candidates; only the pools the call reports as tied
        # (counter [7]) may order equal distances differently from Rust's sort of the whole pool
        assert len(differ) <= cnt[7], (differ, cnt[7])
