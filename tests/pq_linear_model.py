"""CPU model of the exhaustive scan over PQ code rows (dann_pq_linear_search_batch): the reference's algos::linear_search
(diskann-benchmark/src/exhaustive/algos.rs:42-99) with a product-quantised QueryComputer.  Nothing here shares code with
the GPU path: the tables are the oracle's orc_pq_build_lut (populate_chunk_distances_impl), the sums its orc_pq_lookup
(pq_dist_lookup_single: chunk order, f32, from +0.0), the selection tests/flat_model.py's closed form of the queue
inserts.  Also small builders of PQ indices with uneven chunk offsets.  No test functions."""
import numpy as np

import flat_model as fm
import oracle

EMPTY = 0xFFFFFFFF
TAG_PUBLISHED, TAG_FROZEN = 254, 255
HIDDEN_TAGS = (0, 1, 2, 253)  # AVAILABLE, OWNED, RETIRING and the last value below PUBLISHED


def uneven_offsets(rng, dim, chunks):
    """chunks + 1 strictly increasing offsets from 0 to dim; where dim allows, the first and the last chunk hold one element
    and the others differ in length"""
    assert chunks <= dim
    if chunks == 1:
        return np.array([0, dim], np.uint32)
    lens = np.ones(chunks, np.int64)
    for _ in range(dim - chunks):  # the spare elements go to the inner chunks (to any, when there are only two)
        lens[int(rng.integers(1, chunks - 1)) if chunks > 2 else int(rng.integers(0, 2))] += 1
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    assert off[-1] == dim and (np.diff(off.astype(np.int64)) >= 1).all()
    return off


def tables(metric, pivots, offsets, queries):
    """[nq, chunks, 256] lookup tables of the oracle"""
    pivots = np.ascontiguousarray(pivots, np.float32)
    offsets = np.ascontiguousarray(offsets, np.uint32)
    queries = np.ascontiguousarray(queries, np.float32).reshape(-1, pivots.shape[1])
    chunks = offsets.size - 1
    out = np.zeros((queries.shape[0], chunks, 256), np.float32)
    L = oracle.lib()
    for i in range(queries.shape[0]):
        L.orc_pq_build_lut(metric, pivots.ctypes.data, None, offsets.ctypes.data, chunks, pivots.shape[1],
                           queries[i].ctypes.data, out[i].ctypes.data)
    return out


def distances(lut, codes):
    """[nq, n] table sums of the oracle, row by row"""
    lut = np.ascontiguousarray(lut, np.float32)
    codes = np.ascontiguousarray(codes, np.uint8)
    nq, chunks = lut.shape[0], lut.shape[1]
    assert codes.shape[1] == chunks
    look = oracle.lib().orc_pq_lookup
    out = np.empty((nq, codes.shape[0]), np.float32)
    base, step = codes.ctypes.data, codes.strides[0]
    for q in range(nq):
        table = lut[q].ctypes.data
        out[q] = [look(table, base + i * step, chunks) for i in range(codes.shape[0])]
    return out


def expect(D, slots, k, accept=None):
    """(ids[nq, k], dists[nq, k], written[nq], cmps[nq]) of queries whose distances to all slots of the index are D[q]:
    `slots` are the evaluated ones in ascending order (in the range, readable, not skipped as deleted); accept[q] (a bool
    array over all slots, or one for all queries) keeps the ones the query's filter holds"""
    slots = np.asarray(slots, np.int64)
    ids, dists, written, cmps = [], [], [], []
    for q, row in enumerate(D):
        mine = slots
        if accept is not None:
            a = np.asarray(accept)
            mine = slots[(a if a.ndim == 1 else a[q])[slots]]
        pos, d = fm.flat_knn_closed(row[mine], k)
        i, dd = fm.padded(pos, d, k, mine)
        ids.append(i)
        dists.append(dd)
        written.append(len(pos))
        cmps.append(len(mine))
    return np.stack(ids), np.stack(dists), np.array(written), np.array(cmps)


class PqCase:
    """a PQ index on the GPU and the oracle's distances of its slots: n rows and `nstart` start-point rows of random (or
    given) codes over `chunks` uneven chunks of a `dim`-dimensional space"""

    def __init__(self, da, seed, metric, dim, chunks, n, nstart=1, codes=None, pivots=None, offsets=None, tags=False):
        rng = np.random.default_rng(seed)
        self.rng, self.metric, self.dim, self.chunks, self.n, self.nstart = rng, metric, dim, chunks, n, nstart
        self.offsets = uneven_offsets(rng, dim, chunks) if offsets is None else np.asarray(offsets, np.uint32)
        self.pivots = rng.standard_normal((256, dim)).astype(np.float32) if pivots is None else pivots
        self.codes = rng.integers(0, 256, (n + nstart, chunks), dtype=np.uint8) if codes is None else codes
        assert self.codes.shape == (n + nstart, chunks)
        stride = (chunks + 1 + 15) // 16 * 16 if tags else 0
        self.gix = da.Provider(da.PQ, metric, dim, n, 4, self.codes[n:], row_stride=stride, pq_pivots=self.pivots,
                               pq_offsets=self.offsets, inline_tags=tags)
        self.gix.set_elements(0, self.codes[:n])
        self.slots = np.arange(n + nstart, dtype=np.uint32)

    def queries(self, nq):
        return self.rng.standard_normal((nq, self.dim)).astype(np.float32)

    def D(self, q):
        """[nq, n + nstart] oracle distances of every slot"""
        return distances(tables(self.metric, self.pivots, self.offsets, q), self.codes)

    def close(self):
        self.gix.close()
