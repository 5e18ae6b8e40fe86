"""Prunes and graph mutations on quantised rows, under every metric the row type resolves, against the oracle.

MinMax and spherical rows have no distance in the oracle, so the oracle runs on a distance table (oracle.TABLE,
tests/table_oracle.py): T[x][y] is the numpy model's distance of row image x as the first argument and stored slot y as
the second, on realistic rows with real headers.  SQ4 / SQ1 rows keep their SQ-8 twin (identical distance bits under L2,
IP and CosineNormalized).  Everything is compared exactly: adjacency byte for byte, ids, distance bits, counters.

Cells of test_prune / test_insert / test_record (the full matrix, at dimension 128 and at one tail dimension each:
100 for 8-, 2- and 1-bit rows, 64 for 4-bit rows):
    MM1 MM2 MM4 MM8   x  L2, IP, Cosine, CosineNormalized   (dim 128: rows from the model's compressor; tail dimension:
                                                             the reference's own draw, a and b uniform in [0, 2])
    SPH1 SPH2 SPH4    x  L2, IP, Cosine
    SQ4 SQ1           x  L2, IP, CosineNormalized
alpha = 1.2 (both passes of the sweep) everywhere, plus one cell per type class with alpha = 1.0 and
saturate_after_prune: MM8 L2 100, SPH2 IP 128, SQ4 CosineNormalized 64.

Covering subset of test_build / test_consolidate / test_inplace_delete -- every type once, every (OP, NORM) form of every
type class once ((L2), (IP), (COS), (IP, NORM) for MinMax; (L2), (IP), (COS) for spherical; (IP), (L2, NORM) for SQ4 /
SQ1, whose (L2) form tests/test_gpu_sq_bits.py mutates):
    MM8 L2 100, MM4 IP 64, MM2 Cosine 128, MM1 CosineNormalized 100, SPH1 L2 128, SPH2 IP 100, SPH4 Cosine 64,
    SQ4 IP 128, SQ1 CosineNormalized 100

test_minmax_prunes_keep_the_argument_order: tie-rich MinMax rows on which the oracle alone, run on T and on T with its
slot x slot part transposed, differs in at least 5 lists at the sweep (prune_pool), in multi_insert with IBC_ALL and in
consolidate -- then the GPU must equal the oracle on T.  Cells: L2 at all four widths; IP, Cosine and CosineNormalized at
4, 2 and 1 bit.  Left out: MM8 x IP, Cosine, CosineNormalized -- on 8-bit rows no design tried reached 5 differing lists
at all three sites under these metrics (the two argument orders of the epilogue then differ too rarely to move a prune)."""
import numpy as np
import pytest

import oracle
from consolidate_model import consolidate, pair_distance
from helpers import bits as fbits, random_graph
from inplace_delete_model import TIE_RUST, inplace_delete
from search_builders import SqBitsCase
from table_oracle import MmTableCase, SphTableCase

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

L2, IP, COS, COSN = oracle.L2, oracle.INNER_PRODUCT, oracle.COSINE, oracle.COSINE_NORMALIZED
MNAME = {L2: "l2", IP: "ip", COS: "cos", COSN: "cosn"}
TAIL = {8: 100, 4: 64, 2: 100, 1: 100}
BATCHES = (1, 2, 5, 20, 72)
POOLS = [0, 1, 5, 70, 200, 333]


class Cell:
    """one (family, bits, metric, dim) under the GPU provider and its oracle: a table index, or the SQ-8 twin"""

    def __init__(self, fam, bits, metric, dim, n, R, maxdeg, seed, adj=False, rows=None):
        self.fam, self.bits, self.metric, self.dim, self.n, self.maxdeg = fam, bits, metric, dim, n, maxdeg
        if fam == "mm":
            self.c = MmTableCase(bits, metric, n, dim, R, seed, rows=rows or ("model" if dim == 128 else "reference"),
                                 adj=adj, maxdeg=maxdeg)
        elif fam == "sph":
            self.c = SphTableCase(bits, metric, n, dim, R, seed, adj=adj, maxdeg=maxdeg)
        else:
            self.c = SqBitsCase(bits, metric, n, dim, R, seed, adj=adj, maxdeg=maxdeg)
        self.oix, self.gix, self.rng = self.c.oix, self.c.gix, self.c.rng
        self.adj0 = self.c.adj if adj else np.zeros((n + 1, maxdeg + 1), np.uint32)

    def dists(self, loc, ids):
        if self.fam == "sq":
            return np.array([pair_distance(self.oix, int(loc), int(j)) for j in ids], np.float32)
        return self.c.T[loc, ids]

    def stored_query(self, slot):
        return self.oix.row(slot) if self.fam == "sq" else np.array([slot], np.uint32)

    def set_graph(self, adj=None):
        adj = self.adj0 if adj is None else adj
        self.oix.adj[:] = adj
        self.gix.upload_graph(adj)


def _cfgs(pruned, maxdeg, lb, **kw):
    okw = dict(kw)
    if "intra_batch_candidates" in kw:
        ibc = kw["intra_batch_candidates"]
        kw["intra_batch_candidates"] = {oracle.IBC_NONE: da.IBC_NONE, oracle.IBC_ALL: da.IBC_ALL}.get(ibc, ibc)
    return oracle.build_config(pruned, maxdeg, lb, **okw), da.build_config(pruned, maxdeg, lb, **kw)


def _same_adjacency(gix, oix, maxdeg):
    got = gix.download_graph()
    lens = oix.adj[:, 0]
    assert np.array_equal(got[:, 0], lens)
    mask = np.arange(maxdeg)[None, :] < lens[:, None]
    assert np.array_equal(got[:, 1:][mask], oix.adj[:, 1:][mask])


def _same_graph(gix, oix):
    g, o = gix.download_graph(), oix.adj.copy()
    for a in (g, o):
        for r in range(a.shape[0]):
            a[r, 1 + min(int(a[r, 0]), gix.max_degree):] = 0
    bad = np.flatnonzero((g != o).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}"


def _id(p):
    fam, bits, metric, dim, alpha = p
    return f"{fam}{bits}-{MNAME[metric]}-{dim}" + ("" if alpha == 1.2 else "-alpha1")


FULL = ([("mm", b, m, d, 1.2) for b in (1, 2, 4, 8) for m in (L2, IP, COS, COSN) for d in (128, TAIL[b])] +
        [("sph", b, m, d, 1.2) for b in (1, 2, 4) for m in (L2, IP, COS) for d in (128, TAIL[b])] +
        [("sq", b, m, d, 1.2) for b in (4, 1) for m in (L2, IP, COSN) for d in (128, TAIL[b])] +
        [("mm", 8, L2, 100, 1.0), ("sph", 2, IP, 128, 1.0), ("sq", 4, COSN, 64, 1.0)])
SUBSET = [("mm", 8, L2, 100, 1.2), ("mm", 4, IP, 64, 1.2), ("mm", 2, COS, 128, 1.2), ("mm", 1, COSN, 100, 1.2),
          ("sph", 1, L2, 128, 1.2), ("sph", 2, IP, 100, 1.2), ("sph", 4, COS, 64, 1.2),
          ("sq", 4, IP, 128, 1.2), ("sq", 1, COSN, 100, 1.2)]
N, R, MAXDEG, LB = 600, 8, 10, 24


@pytest.fixture(scope="module", params=FULL, ids=_id)
def cell(request):
    fam, bits, metric, dim, alpha = request.param
    c = Cell(fam, bits, metric, dim, N, R, MAXDEG, 3000 + 97 * FULL.index(request.param))
    c.kw = dict(alpha=alpha, saturate_after_prune=alpha == 1.0)
    return c


def test_prune(cell):
    """prune_batch against prune_pool: pools of 0 .. 333 candidates (past the 256-entry row-kernel path), the location
    among its own candidates, the pool distances d(location, candidate) of the row type, both force_saturate values"""
    c = cell
    ocfg, gcfg = _cfgs(R, MAXDEG, LB, **c.kw)
    rng = np.random.default_rng(11)
    locs = rng.choice(c.n, 12, replace=False).astype(np.uint32)
    pools, dists, off = [], [], [0]
    for i, loc in enumerate(locs):
        ids = rng.choice(c.n, POOLS[i % 6], replace=False).astype(np.uint32)
        if ids.size > 3:
            ids[2] = loc
        pools.append(ids)
        dists.append(c.dists(loc, ids))
        off.append(off[-1] + ids.size)
    for sat in (False, True):
        got = c.gix.prune_batch(gcfg, locs, np.concatenate(pools), np.concatenate(dists), np.array(off, np.uint64),
                                force_saturate=sat)
        for i, loc in enumerate(locs):
            want, _ = c.oix.prune_pool(ocfg, int(loc), pools[i], dists[i], force_saturate=sat)
            assert got[i, 0] == want.size and np.array_equal(got[i, 1:1 + want.size], want), (i, sat)


@pytest.mark.parametrize("ibc", [oracle.IBC_NONE, 4, oracle.IBC_ALL], ids=["none", "max4", "all"])
def test_insert(cell, ibc):
    """insert_batch against multi_insert (the extras site around(ids, position, cand), the bootstrap, the hub back-edge
    lists), then dann_insert of single points with max_backedges 0 and 3 against the oracle's insert.  dann_insert reads
    0 as the reference's default, pruned_degree (include/dann.h); the oracle takes the number of back-edges literally"""
    c = cell
    c.set_graph()
    ocfg, gcfg = _cfgs(R, MAXDEG, LB, intra_batch_candidates=ibc, **c.kw)
    s = 0
    for b in BATCHES + (c.n,):
        slots = np.arange(s, min(s + b, c.n - 2), dtype=np.uint32)
        if slots.size:
            c.oix.multi_insert(ocfg, slots)
            c.gix.insert_batch(gcfg, slots)
        s += b
    _same_adjacency(c.gix, c.oix, c.maxdeg)
    for slot, mb in ((c.n - 2, 0), (c.n - 1, 3)):
        o1, _ = _cfgs(R, MAXDEG, LB, max_backedges=mb or R, **c.kw)
        _, g1 = _cfgs(R, MAXDEG, LB, max_backedges=mb, **c.kw)
        c.oix.insert(o1, slot)
        c.gix.insert(g1, slot)
        _same_adjacency(c.gix, c.oix, c.maxdeg)


def test_record(cell):
    """search_record: a stored row of a general quantised index as the query (the insert search), visit by visit"""
    c = cell
    rng = np.random.default_rng(13)
    c.set_graph(np.pad(random_graph(rng, c.n, R), ((0, 0), (0, c.maxdeg - R))))
    slots = rng.choice(c.n, 12, replace=False).astype(np.uint32)
    rid, rd, rn, st = c.gix.search_record(slots, 30)
    for i, s_ in enumerate(slots):
        _, _, _, ost, orid, ord_ = c.oix.search(c.stored_query(int(s_)), 30, 1, 10, record=True)
        assert rn[i] == orid.size
        assert np.array_equal(rid[i, :rn[i]], orid) and np.array_equal(fbits(rd[i, :rn[i]]), fbits(ord_))
        assert st["cmps"][i] == ost[0] and st["hops"][i] == ost[1]


# ---- build, consolidate, in-place delete: the covering subset --------------------------------------------------------------
@pytest.mark.parametrize("p", SUBSET, ids=_id)
def test_build(p):
    """dann_build against the oracle's multi_insert over the same batch schedule (default intra-batch candidates)"""
    from diskann_amd.sharding import batch_schedule
    fam, bits, metric, dim, _ = p
    n, maxdeg, pruned, lb = 1200, 16, 12, 24
    c = Cell(fam, bits, metric, dim, n, pruned, maxdeg, 4000 + SUBSET.index(p))
    ocfg, gcfg = _cfgs(pruned, maxdeg, lb)
    growth, max_batch = 0.1, 512
    nb = c.gix.build(gcfg, 0, n, growth, max_batch)
    k = 0
    for s0, b in batch_schedule(0, n, growth, max_batch):
        c.oix.multi_insert(ocfg, np.arange(s0, s0 + b, dtype=np.uint32))
        k += 1
    assert k == nb
    _same_adjacency(c.gix, c.oix, maxdeg)


@pytest.fixture(scope="module", params=SUBSET, ids=_id)
def graph_cell(request):
    fam, bits, metric, dim, _ = request.param
    return Cell(fam, bits, metric, dim, 1000, 32, 32, 5000 + SUBSET.index(request.param), adj=True)


def _consolidate(gix, oix, n, deleted):
    """delete, then consolidate every slot: R = 32, pruned degree 24"""
    gix.delete_points(np.flatnonzero(deleted))
    ocfg, gcfg = _cfgs(24, 32, 50)
    kinds, cnt = gix.consolidate(gcfg)
    want = consolidate(oix, ocfg, deleted)
    assert np.array_equal(kinds, want)
    _same_graph(gix, oix)
    assert cnt[0] == n + 1 and cnt[2] > 0  # prunes ran


def _inplace_delete(gix, oix, n):
    deleted = np.zeros(n + 1, bool)
    ids = np.random.default_rng(19).choice(n, 16, replace=False)
    ocfg, gcfg = _cfgs(24, 32, 50)
    gix.set_prune_tie_order(da.TIE_RUST)
    got = gix.inplace_delete(gcfg, ids, method=da.INPLACE_TWO_HOP_AND_ONE_HOP, num_to_replace=3)
    want = inplace_delete(oix, ocfg, deleted, ids, da.INPLACE_TWO_HOP_AND_ONE_HOP, 3, TIE_RUST, 0, 0)
    assert got[:8].tolist() == want[:8].tolist(), (got, want)
    assert want[7] > 0 and want[1] > 0  # prunes ran
    _same_graph(gix, oix)
    assert np.array_equal(gix.get_deleted()[:n + 1], deleted.astype(np.uint8))


def _fresh_provider(case):
    """a new provider over the case's rows and starting graph (deletes cannot be unmarked)"""
    case.gix.close()
    return case.attach_gpu()


def test_consolidate(graph_cell):
    c = graph_cell
    c.gix = _fresh_provider(c.c)
    c.oix.adj[:] = c.adj0
    deleted = np.zeros(c.n + 1, bool)
    deleted[np.random.default_rng(17).choice(c.n, c.n // 10, replace=False)] = True
    _consolidate(c.gix, c.oix, c.n, deleted)


def test_inplace_delete(graph_cell):
    c = graph_cell
    c.gix = _fresh_provider(c.c)
    c.oix.adj[:] = c.adj0
    _inplace_delete(c.gix, c.oix, c.n)


# ---- the MinMax argument order ---------------------------------------------------------------------------------------------
# (dim, distinct code rows, header classes) of the tie-rich rows per width; seeds 900 + bits
ORDER_DESIGN = {8: (100, 20, 3), 4: (64, 40, 3), 2: (100, 20, 3), 1: (100, 20, 4)}
ORDER_CELLS = [(b, L2) for b in (8, 4, 2, 1)] + [(b, m) for m in (IP, COS, COSN) for b in (4, 2, 1)]
ORDER_N = 600


def order_case(bits, metric, gpu):
    dim, distinct, classes = ORDER_DESIGN[bits]
    return MmTableCase(bits, metric, ORDER_N, dim, 32, 900 + bits, rows="ties", gpu=gpu, classes=classes, distinct=distinct)


def order_pools(c):
    rng = np.random.default_rng(1)
    locs, pools = [], []
    for i in range(150):
        locs.append(int(rng.integers(0, c.n)))
        pools.append(rng.choice(c.n, 60 if i % 2 else 120, replace=False).astype(np.uint32))
    return np.array(locs, np.uint32), pools


def order_multi_insert(oix, gix=None):
    ocfg, gcfg = _cfgs(8, 10, 24, intra_batch_candidates=oracle.IBC_ALL)
    s = 0
    for b in BATCHES + (oix.capacity,):
        slots = np.arange(s, min(s + b, oix.capacity), dtype=np.uint32)
        if slots.size:
            oix.multi_insert(ocfg, slots)
            if gix is not None:
                gix.insert_batch(gcfg, slots)
        s += b


def order_deleted(n):
    deleted = np.zeros(n + 1, bool)
    deleted[np.random.default_rng(2).choice(n, n // 10, replace=False)] = True
    return deleted


def order_sensitivity(c):
    """the oracle alone on T and on T with its slot x slot part transposed -> the number of lists that differ at
    (i) prune_pool with the true pool distances, (ii) multi_insert with IBC_ALL, (iii) consolidate"""
    Tt = c.transposed()
    a, b = c.table_index(c.T), c.table_index(Tt)
    ocfg = oracle.build_config(8, 10, 24)
    locs, pools = order_pools(c)
    prune = sum(a.prune_pool(ocfg, int(loc), ids, c.T[loc, ids])[0].tolist() !=
                b.prune_pool(ocfg, int(loc), ids, c.T[loc, ids])[0].tolist() for loc, ids in zip(locs, pools))
    a.adj[:] = 0
    b.adj[:] = 0
    order_multi_insert(a)
    order_multi_insert(b)
    insert = int((a.adj != b.adj).any(axis=1).sum())
    a, b = c.table_index(c.T), c.table_index(Tt)
    ccfg = oracle.build_config(24, 32, 50)
    consolidate(a, ccfg, order_deleted(c.n))
    consolidate(b, ccfg, order_deleted(c.n))
    return prune, insert, int((a.adj != b.adj).any(axis=1).sum())


@pytest.mark.parametrize("bits,metric", ORDER_CELLS, ids=[f"{b}-{MNAME[m]}" for b, m in ORDER_CELLS])
def test_minmax_prunes_keep_the_argument_order(bits, metric):
    """The MinMax epilogue ((t0 + x.n y.b) + y.n x.b) + ... is not symmetric and every prune site passes (x, y) by hand.
    On these rows the order decides prunes: first the oracle alone shows at least 5 differing lists per site between
    T and its transpose (a condition on the inputs), then the GPU must reproduce the oracle on T at the sweep
    (prune_batch), in insert_batch with IBC_ALL (fill_list_distances, the extras, the back-edge prunes), in consolidate
    and in the in-place delete."""
    c = order_case(bits, metric, gpu=True)
    prune, insert, cons = order_sensitivity(c)
    assert prune >= 5 and insert >= 5 and cons >= 5, (prune, insert, cons)
    # (i) the sweep
    ocfg, gcfg = _cfgs(8, 10, 24)
    locs, pools = order_pools(c)
    dists = [c.T[loc, ids] for loc, ids in zip(locs, pools)]
    off = np.concatenate([[0], np.cumsum([p.size for p in pools])]).astype(np.uint64)
    got = c.gix.prune_batch(gcfg, locs, np.concatenate(pools), np.concatenate(dists), off)
    for i, loc in enumerate(locs):
        want, _ = c.oix.prune_pool(ocfg, int(loc), pools[i], dists[i])
        assert got[i, 0] == want.size and np.array_equal(got[i, 1:1 + want.size], want), i
    # (iii) consolidate, then the in-place delete from the same starting graph
    _consolidate(c.gix, c.oix, c.n, order_deleted(c.n))
    _fresh_provider(c)
    c.oix.adj[:] = c.adj
    _inplace_delete(c.gix, c.oix, c.n)
    # (ii) multi_insert with every intra-batch candidate, from an empty graph
    _fresh_provider(c)
    empty = np.zeros_like(c.adj)
    c.oix.adj[:] = empty
    c.gix.upload_graph(empty)
    order_multi_insert(c.oix, c.gix)
    _same_adjacency(c.gix, c.oix, c.maxdeg)
