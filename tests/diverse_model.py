"""CPU restatement of diversity-aware search, for the tests.

- NeighborPriorityQueue (diskann/src/neighbor/queue.rs:92-475): fixed capacity, lower-bound insertion (a new entry goes
  in front of equal distances), the remove that compares only the entry at the lower bound (and so can fail under
  ties), the cursor, retain and truncate.
- DiverseNeighborQueue (diskann/src/neighbor/diverse_priority_queue.rs:63-238).
- graph::search::Diverse over an oracle.Index: search_internal (diskann/src/graph/index.rs:1933-2000) with the diverse
  queue, post_process, then the Knn post-processor (start points dropped, first k).  Neighbours come from
  oix.neighbors and distances from oix.expand_beam, so every distance has the oracle's bits.
"""
import math

import numpy as np

NO_ATTRIBUTE = 0xFFFFFFFF


class NeighborPriorityQueue:
    def __init__(self, capacity):
        self.capacity = capacity
        self.search_l = capacity
        self.ids, self.dists, self.visited = [], [], []
        self.cursor = 0

    def size(self):
        return len(self.ids)

    def is_full(self):
        return len(self.ids) == self.capacity

    def lower_bound(self, d):
        for i, x in enumerate(self.dists):
            if x >= d:
                return i
        return len(self.dists)

    def insert(self, nid, d):
        if math.isnan(d):
            return
        if self.is_full() and self.dists[-1] < d:
            return
        pos = self.lower_bound(d) if self.ids else 0
        if self.is_full():
            self.ids.pop()
            self.dists.pop()
            self.visited.pop()
        self.ids.insert(pos, nid)
        self.dists.insert(pos, d)
        self.visited.insert(pos, False)
        if pos < self.cursor:
            self.cursor = pos

    def remove(self, nid, d):
        if not self.ids:
            return False
        pos = self.lower_bound(d)
        if pos < len(self.ids) and self.ids[pos] == nid:
            del self.ids[pos], self.dists[pos], self.visited[pos]
            if pos < self.cursor and self.cursor > 0:
                self.cursor -= 1
            return True
        return False

    def get(self, i):
        return self.ids[i], self.dists[i]

    def has_notvisited_node(self):
        return self.cursor < min(self.search_l, len(self.ids))

    def closest_notvisited(self):
        if not self.has_notvisited_node():
            return None
        cur = self.cursor
        self.visited[cur] = True
        self.cursor += 1
        while self.cursor < len(self.ids) and self.visited[self.cursor]:
            self.cursor += 1
        return self.ids[cur], self.dists[cur]

    def truncate(self, n):
        if n < len(self.ids):
            del self.ids[n:], self.dists[n:], self.visited[n:]
            self.cursor = 0

    def retain(self, keep):
        if not self.ids:
            return
        kept = [(i, d) for i, d in zip(self.ids, self.dists) if keep(i, d)]
        n = len(self.ids)
        # compaction in place marks every kept entry unvisited; truncate resets the cursor only if it shortens
        self.ids = [i for i, _ in kept] + self.ids[len(kept):]
        self.dists = [d for _, d in kept] + self.dists[len(kept):]
        self.visited = [False] * len(kept) + self.visited[len(kept):]
        assert len(self.ids) == n
        self.truncate(len(kept))

    def iter(self):
        n = min(self.search_l, len(self.ids))
        return list(zip(self.ids[:n], self.dists[:n]))


class DiverseNeighborQueue:
    """`attribute(id)` returns the attribute value or None.  Counts failed removes: [case 2 (global), case 3 (local)]."""

    def __init__(self, l_value, total_k, diverse_k, attribute):
        self.global_queue = NeighborPriorityQueue(l_value)  # ids are (id, attribute)
        self.local = {}
        self.attribute = attribute
        self.dl = diverse_k * l_value // total_k
        self.dk = diverse_k
        self.failed_removes = [0, 0]
        self.tail_ties = 0  # case 3 passed over a candidate equal to the full global queue's last entry

    def insert(self, nid, d):
        a = self.attribute(nid)
        if a is None:
            return
        lq = self.local.setdefault(a, NeighborPriorityQueue(self.dl))
        lfull, gfull = lq.is_full(), self.global_queue.is_full()
        g = self.global_queue
        if not lfull and not gfull:
            lq.insert(nid, d)
            g.insert((nid, a), d)
        elif lfull:
            wid, wd = lq.get(self.dl - 1)
            if d < wd:
                if not g.remove((wid, a), wd):
                    self.failed_removes[0] += 1
                lq.insert(nid, d)
                g.insert((nid, a), d)
        else:
            (wid, wa), wd = g.get(g.search_l - 1)
            if d == wd:
                self.tail_ties += 1
            if d < wd:
                lq.insert(nid, d)
                g.insert((nid, a), d)
                if wa in self.local and not self.local[wa].remove(wid, wd):
                    self.failed_removes[1] += 1

    def post_process(self):
        removed = set()
        for lq in self.local.values():
            if lq.size() > self.dk:
                removed.update(lq.ids[self.dk:])
                lq.truncate(self.dk)
        if removed:
            self.global_queue.retain(lambda i, d: i[0] not in removed)

    def has_notvisited_node(self):
        return self.global_queue.has_notvisited_node()

    def closest_notvisited(self):
        r = self.global_queue.closest_notvisited()
        return None if r is None else (r[0][0], r[1])

    def iter(self):
        return [(i[0], d) for i, d in self.global_queue.iter()]


def attribute_fn(attrs):
    """attrs: array over slots (NO_ATTRIBUTE = None) or None (no store: every slot None)"""
    if attrs is None:
        return lambda i: None
    return lambda i: None if int(attrs[i]) == NO_ATTRIBUTE else int(attrs[i])


def diverse_search(oix, query, l_value, beam_width, k, diverse_k, total_k, attrs, info=None):
    """-> (ids, dists, result_count, cmps, hops, failed_removes).  ids / dists hold the written results (<= k).
    info (a dict, optional) receives "tail_ties" (DiverseNeighborQueue.tail_ties)."""
    q = DiverseNeighborQueue(l_value, total_k, diverse_k, attribute_fn(attrs))
    visited = set()
    starts = [oix.capacity + i for i in range(oix.nstart)]
    sid, sd = oix.expand_beam(query, starts)
    cmps = hops = 0
    for i, d in zip(sid.tolist(), sd.tolist()):
        visited.add(i)
        q.insert(i, np.float32(d))
        cmps += 1
    while q.has_notvisited_node():
        beam = []
        while len(beam) < beam_width:
            r = q.closest_notvisited()
            if r is None:
                break
            beam.append(r[0])
        cand = []
        for node in beam:
            for n in oix.neighbors(node).tolist():
                if n not in visited:
                    visited.add(n)
                    cand.append(n)
        cid, cd = oix.expand_beam(query, cand) if cand else (np.empty(0, np.uint32), np.empty(0, np.float32))
        for i, d in zip(cid.tolist(), cd.tolist()):
            q.insert(i, np.float32(d))
        cmps += len(cid)
        hops += len(beam)
    q.post_process()
    if info is not None:
        info["tail_ties"] = q.tail_ties
    out = [(i, d) for i, d in q.iter()[:l_value] if i < oix.capacity]
    written = out[:k]
    count = k - 1 if len(written) == k else len(written)
    return ([i for i, _ in written], np.array([d for _, d in written], np.float32), count, cmps, hops,
            tuple(q.failed_removes))
