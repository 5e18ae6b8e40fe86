"""The search logic of a BetaFilter search (layers/betafilter.rs over index.search(Knn{L, W})) over a table of plain
distances: Filter::apply, NeighborPriorityQueue, the visited rule, cmps / hops, the post-processing.  No distance
arithmetic: dist[s] is the index's own distance of the query to slot s, from a bit-exact seam, passed through apply_beta."""
import bisect

import numpy as np


def apply_beta(plain, match, beta):
    """Filter::apply over all slots: one f32 multiply where the predicate holds"""
    plain = np.asarray(plain, np.float32)
    return np.where(match, plain * np.float32(beta), plain).astype(np.float32)


def knn(dist, adj, capacity, nstart, L, W, k, readable=None):
    """(ids[k], dists[k], cmps, hops); unwritten places 0xFFFFFFFF / +inf.  readable: per slot, of an index with tags"""
    cap = L + nstart
    qd, qid, expanded = [], [], []  # the queue: ascending, a new entry goes in front of equal ones

    def insert(s):
        pos = bisect.bisect_left(qd, float(dist[s]))
        if dist[s] == dist[s] and pos < cap:
            qd.insert(pos, float(dist[s])), qid.insert(pos, s), expanded.insert(pos, False)
            del qd[cap:], qid[cap:], expanded[cap:]

    visited = set(range(capacity, capacity + nstart))
    for s in sorted(visited):
        insert(s)
    cmps, hops = nstart, 0
    while True:
        beam = [p for p in range(len(qid)) if not expanded[p]][:W]
        if not beam:
            break
        nodes = [qid[p] for p in beam]
        for p in beam:
            expanded[p] = True
        hops += len(nodes)
        cand = []
        for node in nodes:
            for nb in map(int, adj[node, 1:1 + min(int(adj[node, 0]), adj.shape[1] - 1)]):
                if nb not in visited:
                    visited.add(nb)
                    if nb < capacity + nstart and (readable is None or readable[nb]):
                        cand.append(nb)
        cmps += len(cand)
        for s in cand:
            insert(s)
    res = [s for s in qid if s < capacity][:k]
    ids, out = np.full(k, 0xFFFFFFFF, np.uint32), np.full(k, np.inf, np.float32)
    ids[:len(res)], out[:len(res)] = res, dist[res]
    return ids, out, cmps, hops
