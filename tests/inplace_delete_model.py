"""CPU restatement of in-place deletes over the oracle's Index, in the order include/dann.h defines for
dann_inplace_delete / dann_drop_deleted_neighbors:
  inplace_delete_inner   diskann/src/graph/index.rs:1585-1747 (work lists 1235-1336)
  multi_inplace_delete   index.rs:1338-1496 (all marks first; n = 1 is inplace_delete)
  add_edge_and_prune     index.rs:2264-2341 (robust_prune_list via consolidate_model)
  drop_deleted_neighbors index.rs:1756-1816
A slot is unreadable when `deleted` marks it or, on an index with inline tags, its tag is below PUBLISHED."""
import bisect

import numpy as np

import oracle
from consolidate_model import COMPLETE, DELETED, pair_distance, robust_prune_list

VISITED_AND_TOPK, TWO_HOP_AND_ONE_HOP, ONE_HOP = 0, 1, 2
TIE_POSITION, TIE_RUST = 0, 1
RETIRING, PUBLISHED = 2, 254
NCOUNTERS = 9


def unreadable(oix, deleted, i):
    i = int(i)
    if i >= oix.adj.shape[0] or deleted[i]:
        return True
    return bool(oix.tag_offset) and int(oix.rows[i, oix.tag_offset]) < PUBLISHED


def sort_unstable_by_distance(ids, dists, tie):
    """pool.sort_unstable_by(fast_distance): Rust's own order (oracle/rust_unstable_sort.h) under TIE_RUST, else
    (distance, position) -- the two zeros are one value either way"""
    if not ids:
        return []
    if tie == TIE_RUST:
        out, _ = oracle.rust_sort(oracle.RUST_SORT_UNSTABLE, np.array(ids, np.uint32), np.array(dists, np.float32))
        return [int(i) for i in out]
    order = sorted(range(len(ids)), key=lambda j: (float(dists[j]) + 0.0, j))
    return [ids[j] for j in order]


def candidate_search(oix, deleted, v, l_value, whole_queue=False):
    """VisitedAndTopK's search (index.rs:1168-1233): search_internal, beam width 1, the row of v as the query, over
    NeighborPriorityQueue (queue.rs:130-318; capacity = search_l = l_value + start points), pair distances d(v, c);
    unreadable slots enter the visited set and are skipped.  -> the CopyIds output: the first min(l_value, size)
    entries in queue order, start points kept"""
    cap = l_value + oix.nstart
    qd, qi, qv = [], [], []
    cursor = 0
    visited = set()

    def insert(i, d):
        nonlocal cursor
        d = float(d)
        if d != d:
            return
        if len(qd) == cap and qd[-1] < d:
            return
        pos = bisect.bisect_left(qd, d)  # lower bound: a later equal distance goes in front
        if len(qd) == cap:
            qd.pop(), qi.pop(), qv.pop()
        qd.insert(pos, d), qi.insert(pos, i), qv.insert(pos, False)
        if pos < cursor:
            cursor = pos

    for s in range(oix.capacity, oix.capacity + oix.nstart):
        visited.add(s)
        insert(s, pair_distance(oix, v, s))
    while cursor < len(qd):
        cur = cursor
        qv[cur] = True
        cursor += 1
        while cursor < len(qd) and qv[cursor]:
            cursor += 1
        nbs = []
        for x in oix.neighbors(qi[cur]):
            x = int(x)
            if x not in visited:
                visited.add(x)
                if not unreadable(oix, deleted, x):
                    nbs.append(x)
        for x in nbs:
            insert(x, pair_distance(oix, v, x))
    return list(qi) if whole_queue else qi[:min(l_value, len(qi))]


def work_lists(oix, deleted, v, method, k_value=0, l_value=0):
    """-> (live out-neighbours, replace candidates, in-neighbours)"""
    one = [int(i) for i in oix.neighbors(v) if not unreadable(oix, deleted, i)]
    if method == VISITED_AND_TOPK:
        res = candidate_search(oix, deleted, v, l_value)
        return one, res[:k_value], [c for c in res if v in set(int(i) for i in oix.neighbors(c))]
    if method == ONE_HOP:
        cand = list(one)
    elif method == TWO_HOP_AND_ONE_HOP:
        cand, seen = [], set()
        for nb in one:
            for x in [nb] + [int(i) for i in oix.neighbors(nb)]:
                if x not in seen and not unreadable(oix, deleted, x):
                    seen.add(x)
                    cand.append(x)
    ins = [c for c in cand if v in set(int(i) for i in oix.neighbors(c))]
    return one, one, ins


def inplace_delete_inner(oix, deleted, v, method, num_to_replace, tie, counters, k_value=0, l_value=0):
    """-> {source: targets} with the reference's insert / push semantics (sources in first-insertion order)"""
    one, rc, ins = work_lists(oix, deleted, v, method, k_value, l_value)
    counters[1] += len(ins)
    counters[2] += len(rc)
    edges = {}

    def best(s):
        pool = [r for r in rc if r != s]
        counters[3] += len(pool) if num_to_replace and pool else 0
        d = [pair_distance(oix, s, r) for r in pool]
        return sort_unstable_by_distance(pool, d, tie)[:num_to_replace]

    for c in ins:
        edges[c] = best(c)  # HashMap::insert: a repeated in-neighbour replaces its (identical) entry
    for o in one:
        for r in best(o):
            edges.setdefault(r, []).append(o)
    return edges


def add_edge_and_prune(oix, cfg, deleted, source, targets, to_remove):
    """-> None (nothing written), 'append', 'set' or 'prune'"""
    lst = [int(i) for i in oix.neighbors(source)]
    removed = any(i in to_remove for i in lst)
    lst = [i for i in lst if i not in to_remove]
    added = 0
    for t in targets:  # extend_from_slice (adjacencylist.rs:102-107): push skips ids already present
        if t not in lst:
            lst.append(t)
            added += 1
    if added == 0 and not removed:
        return None
    if len(lst) <= cfg.max_degree:
        oix.set_neighbors(source, lst)
        return "set" if removed else "append"
    pool = [i for i in lst if i != source and not unreadable(oix, deleted, i)]
    oix.set_neighbors(source, robust_prune_list(oix, cfg, source, pool) if pool else [])
    return "prune"


def mark_deleted(oix, deleted, ids):
    for v in ids:
        deleted[v] = True
        if oix.tag_offset:
            oix.rows[v, oix.tag_offset] = RETIRING


def inplace_delete(oix, cfg, deleted, ids, method, num_to_replace=3, tie=TIE_RUST, k_value=0, l_value=0):
    """one dann_inplace_delete call (one minibatch); `deleted` is updated.  -> counters[0:8] (word 8, the matrix-core
    prunes, is not modelled: 0)"""
    counters = np.zeros(NCOUNTERS, np.uint64)
    uid = list(dict.fromkeys(int(i) for i in ids))
    mark_deleted(oix, deleted, uid)
    maps = [inplace_delete_inner(oix, deleted, v, method, num_to_replace, tie, counters, k_value, l_value) for v in uid]
    sources = list(dict.fromkeys(s for m in maps for s in m))
    rm = set(uid)
    kinds = {"append": 5, "set": 6, "prune": 7}
    for s in sources:
        targets = [t for m in maps for t in m.get(s, [])]
        k = add_edge_and_prune(oix, cfg, deleted, s, targets, rm)
        if k:
            counters[kinds[k]] += 1
    for v in uid:
        oix.adj[v, 0] = 0  # drop_adj_list
    counters[0] = len(uid)
    counters[4] = len(sources)
    return counters


def multi_inplace_delete(oix, cfg, deleted, ids, method, num_to_replace=3, tie=TIE_RUST, minibatch=None, k_value=0,
                         l_value=0):
    ids = [int(i) for i in ids]
    step = minibatch or max(len(ids), 1)
    total = np.zeros(NCOUNTERS, np.uint64)
    for lo in range(0, len(ids), step):
        total += inplace_delete(oix, cfg, deleted, ids[lo: lo + step], method, num_to_replace, tie, k_value, l_value)
    return total


def drop_deleted_neighbors_vertex(oix, cfg, deleted, v, only_orphans):
    if unreadable(oix, deleted, v):
        return DELETED
    lst = [int(i) for i in oix.neighbors(v)]
    pool = [i for i in lst if not unreadable(oix, deleted, i)]
    dead = [i for i in lst if unreadable(oix, deleted, i)]
    if only_orphans:
        pool += [d for d in dead if d < oix.adj.shape[0] and int(oix.adj[d, 0]) != 0]
    if not dead and len(pool) <= cfg.pruned_degree:
        return COMPLETE
    oix.set_neighbors(v, pool)
    return COMPLETE


def drop_deleted_neighbors(oix, cfg, deleted, ids=None, only_orphans=False):
    if ids is None:
        ids = range(oix.adj.shape[0])
    return np.array([drop_deleted_neighbors_vertex(oix, cfg, deleted, int(v), only_orphans) for v in ids], np.int32)


def reachable(oix, start):
    seen, stack = {int(start)}, [int(start)]
    while stack:
        for i in oix.neighbors(stack.pop()):
            if int(i) not in seen:
                seen.add(int(i))
                stack.append(int(i))
    return seen
