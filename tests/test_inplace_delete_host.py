"""The CPU restatement of in-place deletes (tests/inplace_delete_model.py) against the reference's inplace_delete.rs
cases (tests/golden/inplace_delete_cases.json), and drop_deleted_neighbors with and without only_orphans."""
import json
import os

import numpy as np
import pytest

import oracle
from consolidate_model import COMPLETE, DELETED
from gridutil import grid_data, grid_neighbors, grid_start_point
from inplace_delete_model import (ONE_HOP, candidate_search, TWO_HOP_AND_ONE_HOP, VISITED_AND_TOPK, TIE_POSITION, TIE_RUST,
                                  drop_deleted_neighbors, inplace_delete, multi_inplace_delete, reachable)
from helpers import rand_vectors, random_graph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inplace_delete_cases.json")
METHODS = {"OneHop": ONE_HOP, "TwoHopAndOneHop": TWO_HOP_AND_ONE_HOP, "VisitedAndTopK": VISITED_AND_TOPK}


def load_cases():
    with open(GOLDEN) as f:
        g = json.load(f)
    return g, {c["name"]: c for c in g["cases"]}


def modelled(case):
    return True


def method_args(case):
    """-> (method, k_value, l_value)"""
    return METHODS[case["method"]], case.get("k_value", 0), case.get("l_value", 0)


def case_setup(g, case):
    """-> (vectors, start point, lists incl. the start's, max_degree, pruned_degree)"""
    if case["setup"] == "square":
        vec = np.array(g["square"]["vectors"], np.float32)
        start = np.array(g["square"]["start_point"], np.float32)
        lists = case["lists"]
        deg = max(max(len(x) for x in lists), 4)
        return vec, start, lists, deg, 4
    dims, size = g["grid3"]["dims"], g["grid3"]["size"]
    vec = grid_data(dims, size)
    lists = grid_neighbors(dims, size) + [[size ** dims - 1]]
    return vec, grid_start_point(dims, size), lists, 2 * dims, 4


def case_index(g, case, tags=True):
    vec, start, lists, deg, pruned = case_setup(g, case)
    stride = oracle.inmem2_stride(oracle.F32, vec.shape[1]) if tags else None
    oix = oracle.Index(oracle.F32, oracle.L2, vec.shape[1], vec.shape[0], deg, start, row_stride=stride, tags=tags)
    oix.set_rows(0, vec)
    for i, ids in enumerate(lists):
        oix.set_neighbors(i, ids)
    cfg = oracle.build_config(pruned, pruned, 10)  # MaxDegree::same(), l_build 10
    return oix, cfg


def check_case(case, lists_of, start):
    for v in case.get("absent", {}).get("in", []):
        bad = set(case["absent"]["ids"]) & set(lists_of(v))
        assert not bad, f"{v} still points to {bad}"
    for v in case.get("nonempty", []):
        assert len(lists_of(v)) > 0, v
    for v, want in case.get("contains", {}).items():
        assert set(want) <= set(lists_of(int(v))), (v, lists_of(int(v)))
    for v, want in case.get("equal_sorted", {}).items():
        assert sorted(lists_of(int(v))) == want, (v, lists_of(int(v)))
    if "reachable" in case:
        seen, stack = {start}, [start]
        while stack:
            for i in lists_of(stack.pop()):
                if i not in seen:
                    seen.add(i)
                    stack.append(i)
        assert len(seen) == case["reachable"]


@pytest.mark.parametrize("name", [c["name"] for c in load_cases()[0]["cases"] if modelled(c)])
@pytest.mark.parametrize("tie", [TIE_RUST, TIE_POSITION])
def test_restatement_reproduces_the_references_cases(name, tie):
    g, cases = load_cases()
    case = cases[name]
    oix, cfg = case_index(g, case)
    before = {v: oix.neighbors(v).tolist() for v in case.get("unchanged", [])}
    deleted = np.zeros(oix.adj.shape[0], bool)
    oracle.set_tie_rule(oracle.DEFAULT_TIE_RULE if tie == TIE_RUST else oracle.POSITION_TIE_RULE)
    method, k, l = method_args(case)
    try:
        inplace_delete(oix, cfg, deleted, case["ids"], method, 3, tie, k, l)
    finally:
        oracle.set_tie_rule()
    check_case(case, lambda v: oix.neighbors(v).tolist(), oix.capacity)
    for v, want in before.items():
        assert oix.neighbors(v).tolist() == want, v
    for v in case["ids"]:
        assert oix.neighbors(v).size == 0  # drop_adj_list


def test_square_onehop_known_lists():
    """worked by hand from inplace_delete_inner: 3's in-neighbours 2 and 4 swap replacements that they already hold,
    so the only change is the removed edge"""
    g, cases = load_cases()
    oix, cfg = case_index(g, cases["inplace_delete_onehop"])
    c = inplace_delete(oix, cfg, np.zeros(5, bool), [3], ONE_HOP, 3)
    assert oix.neighbors(2).tolist() == [4] and oix.neighbors(4).tolist() == [0, 1, 2]
    # ids, in-neighbours, candidates, distances (2 rows x 1 + 2 rows x 1), sources, appended, set, pruned
    assert c[:8].tolist() == [1, 2, 2, 4, 2, 0, 2, 0]


def test_repeated_id_counts_once():
    g, cases = load_cases()
    a, cfg = case_index(g, cases["multi_inplace_delete_twohop_and_onehop"])
    b, _ = case_index(g, cases["multi_inplace_delete_twohop_and_onehop"])
    ca = inplace_delete(a, cfg, np.zeros(5, bool), [2, 3, 2], TWO_HOP_AND_ONE_HOP)
    cb = inplace_delete(b, cfg, np.zeros(5, bool), [2, 3], TWO_HOP_AND_ONE_HOP)
    assert np.array_equal(a.adj, b.adj) and ca.tolist() == cb.tolist()


def test_minibatches_run_one_after_another():
    """multi_inplace_delete over chunks equals the chunks applied in turn, and earlier deletes stay unreadable"""
    rng = np.random.default_rng(3)
    n, dim, R = 200, 8, 12
    data = rand_vectors(rng, oracle.F32, n, dim)
    adj = random_graph(rng, n, R)
    cfg = oracle.build_config(8, 10, 20)

    def make():
        oix = oracle.Index(oracle.F32, oracle.L2, dim, n, R, data[:1])
        oix.set_rows(0, data)
        oix.adj[:] = adj
        return oix

    ids = rng.choice(n, 40, replace=False)
    a, b = make(), make()
    da, db = np.zeros(n + 1, bool), np.zeros(n + 1, bool)
    multi_inplace_delete(a, cfg, da, ids, TWO_HOP_AND_ONE_HOP, minibatch=16)
    for lo in range(0, 40, 16):
        inplace_delete(b, cfg, db, ids[lo: lo + 16], TWO_HOP_AND_ONE_HOP)
    assert np.array_equal(a.adj, b.adj) and np.array_equal(da, db)
    assert da[ids].all() and all(a.neighbors(int(v)).size == 0 for v in ids)


def test_drop_deleted_neighbors_with_and_without_orphans():
    g, cases = load_cases()
    for only_orphans, want2 in ((False, [4]), (True, [4, 3])):
        oix, cfg = case_index(g, cases["inplace_delete_onehop"])
        deleted = np.zeros(5, bool)
        deleted[3] = True  # marked, its list [2, 4] still present
        kinds = drop_deleted_neighbors(oix, cfg, deleted, None, only_orphans)
        assert kinds.tolist() == [COMPLETE, COMPLETE, COMPLETE, DELETED, COMPLETE]
        assert oix.neighbors(2).tolist() == want2
        assert oix.neighbors(3).tolist() == [2, 4]  # a deleted vertex is left alone
        assert oix.neighbors(4).tolist() == ([0, 1, 2] if not only_orphans else [0, 1, 2, 3])
        assert oix.neighbors(0).tolist() == [1, 4]  # nothing deleted, short list: not written
        oix.adj[3, 0] = 0  # once 3's list is dropped, only_orphans removes the edge too
        drop_deleted_neighbors(oix, cfg, deleted, None, True)
        assert oix.neighbors(2).tolist() == [4]


def test_drop_deleted_neighbors_batch_equals_the_loop_in_any_order():
    rng = np.random.default_rng(5)
    n, dim, R = 150, 4, 10
    data = rand_vectors(rng, oracle.F32, n, dim)
    adj = random_graph(rng, n, R)
    deleted = np.zeros(n + 1, bool)
    deleted[rng.choice(n, 30, replace=False)] = True
    adj[np.flatnonzero(deleted)[:10], 0] = 0  # some deleted lists already dropped
    cfg = oracle.build_config(6, 10, 20)
    outs = []
    for order in (np.arange(n + 1), rng.permutation(n + 1)):
        oix = oracle.Index(oracle.F32, oracle.L2, dim, n, R, data[:1])
        oix.adj[:] = adj
        drop_deleted_neighbors(oix, cfg, deleted, order, True)
        outs.append(oix.adj.copy())
    assert np.array_equal(outs[0], outs[1])


def test_the_grid_stays_connected_for_every_single_delete():
    """each single TwoHopAndOneHop delete of the 3 x 3 grid keeps the other 8 points and the start reachable"""
    g, cases = load_cases()
    case = cases["inplace_delete_two_hop_and_one_hop_wider_topology"]
    for v in range(9):
        if v == 8:
            continue  # the start's only link (the reference avoids it too)
        oix, cfg = case_index(g, case)
        inplace_delete(oix, cfg, np.zeros(10, bool), [v], TWO_HOP_AND_ONE_HOP)
        assert len(reachable(oix, 9)) == 9, v


def tie_square():
    """the 2-D square plus a data point on the start point (0.5, 0.5): seen from (0, 0) the two are at equal distance"""
    vec = np.array([[0, 0], [0, 1], [1, 0], [1, 1], [0.5, 0.5]], np.float32)
    oix = oracle.Index(oracle.F32, oracle.L2, 2, 5, 5, np.array([0.5, 0.5], np.float32),
                       row_stride=oracle.inmem2_stride(oracle.F32, 2), tags=True)
    oix.set_rows(0, vec)
    for i, ids in enumerate([[1, 2], [0, 4], [0, 4], [1, 2], [1, 2, 3], [0, 1, 2, 3, 4]]):
        oix.set_neighbors(i, ids)
    return oix


def test_copyids_keeps_start_points_and_a_later_tie_goes_in_front():
    """the start point is inserted first; point 4, inserted later at the same distance, goes in front of it (lower
    bound); CopyIds keeps the start point where Translate drops it"""
    oix = tie_square()
    deleted = np.zeros(6, bool)
    deleted[0] = True
    oix.set_tags(0, [2])  # RETIRING: the oracle's search skips it too
    assert candidate_search(oix, deleted, 0, 10) == [4, 5, 2, 1, 3]  # 2 ties with 1 and is inserted after it
    assert candidate_search(oix, deleted, 0, 2) == [4, 5]
    n, ids, _, _ = oix.search(oix.row(0), 10, 1, k=10)
    assert ids[:n].tolist() == [4, 2, 1, 3]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_candidate_search_equals_the_oracles_search_without_start_points(seed):
    """on integer rows (exact distances, many ties) the restated queue, start points dropped, is the oracle's Translate
    output"""
    rng = np.random.default_rng(seed)
    n, dim, R, L = 400, 3, 12, 20
    data = rng.integers(0, 4, (n, dim)).astype(np.uint8)
    oix = oracle.Index(oracle.U8, oracle.L2, dim, n, R, data[:2], row_stride=oracle.inmem2_stride(oracle.U8, dim),
                       tags=True)
    oix.set_rows(0, data)
    oix.adj[:] = random_graph(rng, n, R, nstart=2)
    deleted = np.zeros(n + 2, bool)
    dead = rng.choice(n, 40, replace=False)
    deleted[dead] = True
    oix.set_tags(0, np.where(deleted[:n], 2, 254).astype(np.uint8))
    for v in dead[:10]:
        full = candidate_search(oix, deleted, int(v), L, whole_queue=True)
        want = [i for i in full if i < n][:L]
        cnt, ids, _, _ = oix.search(oix.row(int(v)), L, 1, k=L)
        assert ids[:cnt].tolist() == want, v
