"""CPU checks of the diverse-search restatement (tests/diverse_model.py):

- the queue against the reference's unit tests (tests/golden/diverse_queue_cases.json, from
  diskann/src/neighbor/diverse_priority_queue.rs and neighbor/queue.rs);
- with one attribute per slot and diverse_k == total_k the search equals the oracle's Knn search on the reference's
  grid_search cases;
- every result holds at most diverse_k entries per attribute.
"""
import json
import os

import numpy as np
import pytest

import oracle
from diverse_model import NO_ATTRIBUTE, DiverseNeighborQueue, NeighborPriorityQueue, attribute_fn, diverse_search
from gridutil import grid_data, grid_neighbors, grid_start_point

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "diverse_queue_cases.json")))
GRID = json.load(open(os.path.join(HERE, "golden", "grid_search.json")))


@pytest.mark.parametrize("case", CASES["diverse"], ids=lambda c: c["name"])
def test_diverse_queue_golden(case):
    attrs = {int(k): v for k, v in case["attributes"].items()}
    q = DiverseNeighborQueue(case["l_value"], case["total_k"], case["diverse_k"], attrs.get)
    for i, d in case["inserts"]:
        q.insert(i, np.float32(d))
    if case["post_process"]:
        q.post_process()
    ids = [i for i, _ in q.iter()]
    if "expect_global" in case:
        assert ids == case["expect_global"]
    if "expect_size" in case:
        assert len(ids) == case["expect_size"]
    if "expect_first" in case:
        assert ids[0] == case["expect_first"]
    if "expect_first_distance" in case:
        assert q.iter()[0][1] == np.float32(case["expect_first_distance"])
    for a, n in case.get("expect_local_sizes", {}).items():
        assert q.local[int(a)].size() == n
    for a, lst in case.get("expect_local", {}).items():
        assert q.local[int(a)].ids == lst


@pytest.mark.parametrize("case", CASES["queue"], ids=lambda c: c["name"])
def test_queue_golden(case):
    q = NeighborPriorityQueue(case["capacity"])
    for op in case["ops"]:
        if op[0] == "insert":
            q.insert(op[1], np.float32(op[2]))
        elif op[0] == "remove":
            assert q.remove(op[1], np.float32(op[2])) is op[3], op
        elif op[0] == "expect":
            assert q.ids == op[1], op
        elif op[0] == "pop":
            assert q.closest_notvisited()[0] == op[1], op
        elif op[0] == "cursor":
            assert q.cursor == op[1], op
        elif op[0] == "retain":
            q.retain(lambda i, d, keep=set(op[1]): i in keep)
        elif op[0] == "truncate":
            q.truncate(op[1])
        else:
            raise AssertionError(op)


def grid_index(dims, size):
    data = grid_data(dims, size)
    n = data.shape[0]
    lists = grid_neighbors(dims, size)
    R = max(2 * dims, 1)
    oix = oracle.Index(oracle.F32, oracle.L2, dims, n, R, grid_start_point(dims, size))
    oix.set_rows(0, data)
    for i, nb in enumerate(lists):
        oix.set_neighbors(i, nb)
    oix.set_neighbors(n, [n - 1])
    return oix


@pytest.mark.parametrize("case", GRID, ids=lambda c: os.path.basename(c["source"]))
def test_unique_attributes_equal_knn(case):
    """unique attribute per slot, diverse_k == total_k: every local queue holds one entry, so the diverse queue is the
    plain queue of the same length -- with one difference: case 3 of DiverseNeighborQueue::insert takes a candidate only
    if it is strictly closer than the full global queue's last entry, NeighborPriorityQueue::insert also when it is
    equal.  Where that never happens the search equals the oracle's Knn (ids, distance bits, hops, cmps); on the
    lattices it does happen, and the restatement must say so"""
    oracle.build()
    oix = grid_index(case["grid_dims"], case["grid_size"])
    L, W, k = case["l_value"], case["beam_width"], case["k"]
    attrs = np.arange(oix.capacity + oix.nstart, dtype=np.uint32)
    q = np.asarray(case["query"], np.float32)
    # the plain queue has L + start points entries, the diverse one L
    for lp in (L, L - oix.nstart):
        if lp < k:
            continue
        n, oi, od, ost = oix.search(q, lp, W, k)
        info = {}
        ids, dists, count, cmps, hops, _ = diverse_search(oix, q, lp + oix.nstart, W, k, k, k, attrs, info)
        same = (ids == oi[:n].tolist() and np.array_equal(dists.view(np.uint32), od[:n].view(np.uint32))
                and (cmps, hops) == (int(ost[0]), int(ost[1])))
        if info["tail_ties"] == 0:
            assert same, (lp, ids, oi[:n].tolist(), (cmps, hops), ost)
            assert count == (k - 1 if n == k else n)
        elif not same:
            assert info["tail_ties"] > 0


def test_unique_attributes_without_ties_equal_knn():
    """random f32 rows (no equal distances): the restatement equals the oracle's Knn on every query"""
    oracle.build()
    rng = np.random.default_rng(2)
    n, dim, R = 600, 8, 12
    data = rng.standard_normal((n, dim)).astype(np.float32)
    oix = oracle.Index(oracle.F32, oracle.L2, dim, n, R, data[:1])
    oix.set_rows(0, data)
    for i in range(n + 1):
        oix.set_neighbors(i, rng.choice(n, R, replace=False))
    attrs = np.arange(n + 1, dtype=np.uint32)
    for t in range(20):
        q = rng.standard_normal(dim).astype(np.float32)
        for lp, W in ((10, 1), (30, 2), (50, 4)):
            m, oi, od, ost = oix.search(q, lp, W, 10)
            info = {}
            ids, dists, count, cmps, hops, _ = diverse_search(oix, q, lp + 1, W, 10, 10, 10, attrs, info)
            assert info["tail_ties"] == 0
            assert ids == oi[:m].tolist() and np.array_equal(dists.view(np.uint32), od[:m].view(np.uint32))
            assert (cmps, hops) == (int(ost[0]), int(ost[1]))


@pytest.mark.parametrize("cardinality,diverse_k,missing", [(1, 1, 0.0), (2, 2, 0.3), (7, 1, 0.0), (7, 3, 0.5), (100, 2, 0.0)])
def test_at_most_diverse_k_per_attribute(cardinality, diverse_k, missing):
    oracle.build()
    rng = np.random.default_rng(cardinality * 10 + diverse_k)
    oix = grid_index(3, 8)
    nslots = oix.capacity + oix.nstart
    attrs = rng.integers(0, cardinality, nslots).astype(np.uint32)
    attrs[rng.random(nslots) < missing] = NO_ATTRIBUTE
    for t in range(5):
        q = rng.uniform(-1, 9, 3).astype(np.float32)
        ids, dists, count, cmps, hops, _ = diverse_search(oix, q, 40, 2, 10, diverse_k, 10, attrs)
        vals = [int(attrs[i]) for i in ids]
        assert NO_ATTRIBUTE not in vals
        assert max(np.bincount(vals)) <= diverse_k if vals else True
        assert np.all(np.diff(dists) >= 0)
        assert len(ids) <= min(10, cardinality * diverse_k)


def test_no_attributes_no_results():
    oracle.build()
    oix = grid_index(2, 10)
    ids, dists, count, cmps, hops, _ = diverse_search(oix, np.zeros(2, np.float32), 20, 1, 10, 2, 10, None)
    assert (ids, count, cmps, hops) == ([], 0, 1, 0)
