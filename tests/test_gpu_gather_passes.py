"""The plain float hop's gather runs only the passes that hold a candidate (search_plain_impl.h, `passes`): a trip of
32 row slots is four passes of 8 rows, a hop with nc candidates takes ceil(min(nc, 32) / 8) passes of its first trip and
ceil((nc - 32) / 8) of its second, one straight body per pass count.  It can go wrong exactly where the pass count or
the trip count changes, so nc is driven there: ids, distance bits, cmps, hops, written and result_count are compared
with the oracle bit for bit, and every checked launch must have been served by one wave per query (`one_wave`) or by
persistent waves (`persistent`).

The graph and the oracle alone say that nc is what the test wants it to be (asserted before anything is compared):
  * layout A.  Every start point has the same adjacency list of l distinct ids below N.  The first hop expands a start
    point, nothing but the start points has been visited, so its l neighbours are its candidates whatever the queue
    holds; the other start points find them all visited (hops with nc = 0).  With every other list emptied the oracle
    counts ns + l comparisons for every query: the first hop's cmps increment is l.
  * layout B, for the frozen hop loop.  The start points list 64 ids, among them X1, X2 and X; X1 is the query, X2 and
    X sit 0.25 and 0.5 away from it along one axis, everything else is far away.  X1 and X2 list 64 new ids each and X
    lists l new ones, so the hops after the first expand X1, X2, X in that order and X's hop has nc = l: with every
    other list emptied the oracle counts ns + 192 + l comparisons for the query.  A table that holds T ids freezes
    before the hop that could take it past 3/4 T; the test sets T so that X2's hop (ns + 192 ids) is past that and
    the smallest T the launch plan accepts for 64 neighbours is not: X's hop runs in the frozen loop.
Among the l neighbours are a row with a NaN (never a candidate for the queue) and two equal rows next to the query (a
tie the merge has to order).  The start gather sees ns in {1, 8, 9, 33} rows.  (L = 100 with 33 start points has 133
queue entries and is served by beam_search_kernel: compared all the same.)"""
import numpy as np
import pytest

import oracle
from helpers import bits, make_pair, rand_vectors, random_graph

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

N, DIM, R, NQ = 2000, 128, 64, 64
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40, 41, 56, 57, 63, 64)
LS = (5, 26, 100)
NO_TEAMS = 4  # DANN_DBG_TUNE_OFF bit 4: small launches stay with one wave per query
NAN_ROW, X1, X2, X, D1, D2 = 7, 20, 21, 22, 23, 24


def _rows(rng, dtype):
    data = rand_vectors(rng, dtype, N, DIM)
    data[NAN_ROW, 5] = np.nan
    for i, c in ((X1, 0.0), (X2, 0.25), (X, 0.5), (D1, 0.75), (D2, 0.75)):  # (exact in f16)
        data[i] = data[X1]
        data[i, 0] = c
    return data


_built = {}


def _index(dtype, ns):
    """(oracle index, provider, its twin with the other lists emptied, queries, base graph, id pool) -- once per shape"""
    key = (dtype, ns)
    if key not in _built:
        rng = np.random.default_rng(4100 + dtype * 7 + ns)
        data = _rows(rng, dtype)
        adj = random_graph(rng, N, R, nstart=ns)
        start_rows = rand_vectors(rng, dtype, ns, DIM)
        oix, gix = make_pair(dtype, oracle.L2, data, adj, start_rows, R)
        gix.debug_set(tune_off=NO_TEAMS, pair_min_queries=1 << 30)
        bare = oracle.Index(dtype, oracle.L2, DIM, N, R, start_rows)
        bare.set_rows(0, data)
        queries = rand_vectors(rng, dtype, NQ, DIM)
        queries[0] = data[X1]
        pool = (100 + rng.permutation(N - 100)).astype(np.uint32)
        _built[key] = (oix, gix, bare, queries, adj, pool)
    return _built[key]


def _set_list(adj, node, ids):
    adj[node, 0] = len(ids)
    adj[node, 1:] = 0
    adj[node, 1:1 + len(ids)] = ids


def _graphs(key, layout, ell):
    """(the graph, the same with every list the layout does not set emptied)"""
    _, _, _, _, base, pool = _index(*key)
    ns = key[1]
    adj = base.copy()
    fresh = pool[200:264]
    if layout == "A":
        own = {N + s: np.concatenate(([D1, NAN_ROW, D2], fresh)).astype(np.uint32)[:ell] for s in range(ns)}
    else:
        first = np.concatenate(([X1, X2, X], pool[:61])).astype(np.uint32)
        own = {N + s: first for s in range(ns)}
        own[X1] = pool[61:125]
        own[X2] = pool[125:189]
        own[X] = np.concatenate(([D1, NAN_ROW, D2], fresh)).astype(np.uint32)[:ell]
    for node, ids in own.items():
        assert len(set(ids.tolist())) == len(ids) and (ids < N).all()
        _set_list(adj, node, ids)
    bare = np.zeros_like(adj)
    for node in own:
        bare[node] = adj[node]
    return adj, bare


def _compare(gix, queries, want, L, tag, family="one_wave"):
    oi, od, oc, ost = want
    (gi, gd, gst), fam = gix.last_family(lambda: gix.search(da.Knn(L, 1), queries, 10))
    assert fam <= {"one_wave", "persistent"} and family in fam, (fam, tag)
    assert not gst["status"].any(), tag
    assert np.array_equal(oi, gi), tag
    assert np.array_equal(bits(od), bits(gd)), tag
    assert np.array_equal(ost[:, 0], gst["cmps"]) and np.array_equal(ost[:, 1], gst["hops"]), tag
    assert np.array_equal(oc, gst["written"]) and np.array_equal(ost[:, 2], gst["result_count"]), tag


def _oracle(key, layout, ell, L):
    """the oracle's result on the layout's graph, after the graph and the oracle alone have said that the hop under test
    has `ell` candidates"""
    oix, _, bare_ix, queries, _, _ = _index(*key)
    ns = key[1]
    adj, bare = _graphs(key, layout, ell)
    bare_ix.adj[:] = bare
    bst = bare_ix.search_batch(queries, L, 1, 10, threads=8)[3]
    if layout == "A":
        assert (bst[:, 0] == ns + ell).all(), (layout, ell, L)
    else:
        assert bst[0, 0] == ns + 192 + ell, (layout, ell, L)
    oix.adj[:] = adj
    want = oix.search_batch(queries, L, 1, 10, threads=8)
    if ell >= 3:  # the two equal rows are in the query's result list, next to each other
        i0 = want[0][0].tolist()
        assert {D1, D2} <= set(i0) and abs(i0.index(D1) - i0.index(D2)) == 1 and NAN_ROW not in i0, (layout, ell, L)
    return adj, want


@pytest.mark.parametrize("ns", [1, 8, 9, 33])
@pytest.mark.parametrize("dtype", [oracle.F32, oracle.F16])
def test_first_hop_at_every_pass_and_trip_boundary(dtype, ns):
    key = (dtype, ns)
    _, gix, _, queries, _, _ = _index(*key)
    try:
        for ell in LENGTHS:
            for L in LS:
                adj, want = _oracle(key, "A", ell, L)
                gix.upload_graph(adj)
                for fmt in (32, 16):
                    gix.set_visited_format(fmt)
                    _compare(gix, queries, want, L, (ell, L, fmt))
                    gix.set_visited_bits(64)  # (grown to what 64 neighbours need: the hops after the first few are frozen)
                    _compare(gix, queries, want, L, (ell, L, fmt, "small table"))
                    gix.set_visited_bits(0)
                gix.set_visited_format(0)
                gix.set_max_concurrency(32)
                _compare(gix, queries, want, L, (ell, L, "persistent"), family="persistent")
                gix.set_max_concurrency(0)
    finally:
        gix.set_visited_bits(0)
        gix.set_max_concurrency(0)
        gix.set_visited_format(0)


@pytest.mark.parametrize("ns", [1, 8, 9, 33])
@pytest.mark.parametrize("dtype", [oracle.F32, oracle.F16])
def test_frozen_hop_at_every_pass_and_trip_boundary(dtype, ns):
    key = (dtype, ns)
    _, gix, _, queries, _, _ = _index(*key)
    ids = 128 if ns <= 9 else 256  # ids the table holds; 3/4 of it is more than ns + 64 + 1 and less than ns + 192
    assert ns + R + 1 < 3 * ids // 4 < ns + 192
    try:
        for ell in LENGTHS:
            for L in LS:
                adj, want = _oracle(key, "B", ell, L)
                gix.upload_graph(adj)
                for fmt in (32, 16):
                    gix.set_visited_format(fmt)
                    gix.set_visited_bits(ids if fmt == 32 else ids // 2)  # (a word holds two 16-bit entries)
                    _compare(gix, queries, want, L, (ell, L, fmt))
                gix.set_visited_format(32)
                gix.set_visited_bits(ids)
                gix.set_max_concurrency(32)
                _compare(gix, queries, want, L, (ell, L, "persistent"), family="persistent")
                gix.set_max_concurrency(0)
    finally:
        gix.set_visited_bits(0)
        gix.set_max_concurrency(0)
        gix.set_visited_format(0)
