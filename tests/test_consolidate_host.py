"""The CPU restatement of consolidate_vector (tests/consolidate_model.py) reproduces the known answers of the reference's
consolidate.rs cases (tests/golden/consolidate_cases.json), with lists compared as sets where the reference sorts them."""
import json
import os

import numpy as np
import pytest

import oracle
from consolidate_model import consolidate, consolidate_vector

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consolidate_cases.json")


def _cases():
    with open(GOLDEN) as f:
        g = json.load(f)
    return g, {c["name"]: c for c in g["cases"]}


def square_index(g, case):
    vec = np.array(g["vectors"], np.float32)
    lists = case["lists"]
    deg = max(max(len(x) for x in lists), case["pruned_degree"])
    oix = oracle.Index(oracle.F32, oracle.L2, vec.shape[1], vec.shape[0], deg, np.array(g["start_point"], np.float32))
    oix.set_rows(0, vec)
    for i, ids in enumerate(lists):
        oix.set_neighbors(i, ids)
    return oix, deg


def square_cfg(case):
    return oracle.build_config(case["pruned_degree"], case["pruned_degree"], 10)  # MaxDegree::same(), l_build 10


def deleted_mask(oix, case):
    d = np.zeros(oix.adj.shape[0], bool)
    d[case["deleted"]] = True
    return d


@pytest.mark.parametrize("name", [c["name"] for c in _cases()[0]["cases"]])
def test_restatement_reproduces_the_references_cases(name):
    g, cases = _cases()
    case = cases[name]
    oix, _ = square_index(g, case)
    kinds = consolidate(oix, square_cfg(case), deleted_mask(oix, case), case["ids"])
    assert kinds.tolist() == case["kinds"]
    for v, want in case["expected_sorted"].items():
        assert sorted(oix.neighbors(int(v)).tolist()) == want, v
    for v, m in case.get("max_len", {}).items():
        assert 0 < len(oix.neighbors(int(v))) <= m


def test_order_of_the_vertices_does_not_matter():
    """a vertex only reads its own list and those of deleted vertices, which consolidation never rewrites"""
    from helpers import rand_vectors, random_graph
    rng = np.random.default_rng(7)
    n, dim, R = 300, 8, 12
    data = rand_vectors(rng, oracle.F32, n, dim)
    adj = random_graph(rng, n, R)
    deleted = np.zeros(n + 1, bool)
    deleted[rng.choice(n, 60, replace=False)] = True
    cfg = oracle.build_config(8, R, 10)
    graphs = []
    for order in (np.arange(n + 1), rng.permutation(n + 1)):
        oix = oracle.Index(oracle.F32, oracle.L2, dim, n, R, data[:1])
        oix.set_rows(0, data)
        oix.adj[:] = adj
        consolidate(oix, cfg, deleted, order)
        graphs.append(oix.adj.copy())
    assert np.array_equal(graphs[0], graphs[1])
    live = ~deleted
    for v in np.flatnonzero(live):
        nb = oix.neighbors(v)
        assert not deleted[nb].any()


def test_self_listed_vertex_counts_in_the_nothing_to_do_test():
    """the reference's pool still holds the vertex itself when it tests `pool.len() <= degree` (index.rs:1858-1864)"""
    g, cases = _cases()
    case = dict(cases["consolidate_nothing_to_do_returns_complete"])
    case["lists"] = [[0, 1, 4], [0, 4], [3, 4], [2, 4], [0, 1, 2, 3]]
    case["pruned_degree"] = 2
    oix, _ = square_index(g, case)
    assert consolidate_vector(oix, square_cfg(case), deleted_mask(oix, case), 0) == 0
    assert 0 not in oix.neighbors(0).tolist() and len(oix.neighbors(0)) <= 2
