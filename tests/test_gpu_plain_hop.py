"""The plain float hop (search_plain_impl.h): Knn searches of 128-element f32 / f16 rows under L2 with at most 128 queue
entries run beam_search_plain -- the algorithm of beam_search_one, its hop written without per-lane branches.  Every
result is compared with the oracle bit for bit: ids, distance bits, cmps, hops, written and result_count; every checked
launch must have been served by one wave per query (`one_wave`) or by persistent waves (`persistent`).

The oracle alone says which paths the inputs reach (asserted before anything is compared):
  * a visited table of W words freezes once it holds 3/4 W ids, and a search inserts at least cmps + start points ids;
  * the first hop expands a start point while the queue is not full: every neighbour survives, so a start point of
    degree > 16 takes the merge through LDS;
  * duplicate rows give equal distances inside the result lists (ties in the merge);
  * a node whose adjacency list repeats the start point's finds nothing new: the same search with that list emptied
    has the same cmps and hops -- a hop without survivors."""
import numpy as np
import pytest

import oracle
from helpers import bits, make_pair, rand_vectors, random_graph

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

N, DIM = 4000, 128
LS = (1, 5, 26, 63, 64, 100, 127)
NO_TEAMS = 4  # DANN_DBG_TUNE_OFF bit 4: small launches stay with one wave per query


def _special_rows(data):
    """duplicate rows (ties), a row with a NaN and a row with an inf coordinate"""
    data[100:1100] = data[1100:2100]
    data[2100:2300] = data[1100:1300]
    data[7, 5] = np.nan
    data[8, 9] = np.inf
    return data


_built = {}


def _index(dtype, R, nstart, full):
    """(oracle index, provider, queries, {L: oracle result}) -- built once per shape, the oracle's results computed once"""
    key = (dtype, R, nstart, full)
    if key not in _built:
        rng = np.random.default_rng(900 + dtype * 7 + R + nstart)
        data = _special_rows(rand_vectors(rng, dtype, N, DIM))
        adj = random_graph(rng, N, R, nstart=nstart, min_len=R if full else None)
        oix, gix = make_pair(dtype, oracle.L2, data, adj, data[:nstart], R)
        gix.debug_set(tune_off=NO_TEAMS, pair_min_queries=1 << 30)
        queries = rand_vectors(rng, dtype, 1000, DIM)
        queries[3] = data[1100]  # (a query that sits on a run of duplicate rows)
        _built[key] = (oix, gix, queries, adj, {})
    return _built[key]


def _oracle(key, L, k=10):
    oix, _, queries, _, memo = _index(*key)
    if (L, k) not in memo:
        memo[(L, k)] = oix.search_batch(queries, L, 1, k, threads=8)
    return memo[(L, k)]


def _check(key, nq, L, tag, k=10, family="one_wave"):
    _, gix, queries, _, _ = _index(*key)
    oi, od, oc, ost = _oracle(key, L, k)
    (gi, gd, gst), fam = gix.last_family(lambda: gix.search(da.Knn(L, 1), queries[:nq], k))
    assert fam <= {"one_wave", "persistent"} and family in fam, (fam, tag)
    assert not gst["status"].any(), tag
    assert np.array_equal(oi[:nq], gi), tag
    assert np.array_equal(bits(od[:nq]), bits(gd)), tag
    assert np.array_equal(ost[:nq, 0], gst["cmps"]) and np.array_equal(ost[:nq, 1], gst["hops"]), tag
    assert np.array_equal(oc[:nq], gst["written"]) and np.array_equal(ost[:nq, 2], gst["result_count"]), tag


SHAPES = [(24, 1, False), (24, 3, False), (64, 2, True)]


@pytest.mark.parametrize("R,nstart,full", SHAPES)
@pytest.mark.parametrize("dtype", [oracle.F32, oracle.F16])
def test_plain_hop_equals_the_oracle(dtype, R, nstart, full):
    key = (dtype, R, nstart, full)
    _, gix, _, adj, _ = _index(*key)
    # the oracle alone: ties inside the result lists; the first hop's survivors take the merge through LDS
    oi, od, _, ost = _oracle(key, 26)
    assert (od[:, :-1] == od[:, 1:]).any(), "no equal distances among the results"
    assert (ost[:, 0] > 26 + nstart).all(), "a queue that never fills"
    if full:
        assert (adj[N:, 0] > 16).all()
    for fmt in (32, 16):
        gix.set_visited_format(fmt)
        for nq in (1, 63, 1000):
            for L in LS:
                _check(key, nq, L, (fmt, nq, L))
    gix.set_visited_format(0)


@pytest.mark.parametrize("fmt", [32, 16])
@pytest.mark.parametrize("dtype,R,nstart,full", [(oracle.F32, 24, 1, False), (oracle.F16, 64, 2, True)])
def test_tables_that_freeze_spill_and_overflow(dtype, R, nstart, full, fmt):
    """explicit tables of 64 .. 512 words: frozen within a few hops, continued in the spill tables (1 000 concurrent
    queries recycle them), and queries that outgrow even those are re-run"""
    key = (dtype, R, nstart, full)
    _, gix, _, _, _ = _index(*key)
    gix.set_visited_format(fmt)
    try:
        for words in (64, 128, 256, 512):
            gix.set_visited_bits(words)
            for L in (26, 100):
                ost = _oracle(key, L)[3]
                # (16-bit entries: a table of W words holds 2 W ids; at L = 26 the largest of them stays open)
                if L == 100 or fmt == 32:
                    assert (ost[:, 0] + nstart > (3 * words * (2 if fmt == 16 else 1)) // 4).all(), (words, L)
                _check(key, 1000, L, (fmt, words, L))
                _check(key, 63, L, (fmt, words, L, "small"))
    finally:
        gix.set_visited_bits(0)
        gix.set_visited_format(0)


@pytest.mark.parametrize("dtype", [oracle.F32, oracle.F16])
def test_persistent_waves(dtype):
    key = (dtype, 24, 1, False)
    _, gix, _, _, _ = _index(*key)
    try:
        for fmt in (32, 16):
            gix.set_visited_format(fmt)
            gix.set_max_concurrency(32)
            for L in (26, 64, 127):
                _check(key, 1000, L, (fmt, L, "capped"), family="persistent")
            gix.set_visited_bits(128)
            _check(key, 1000, 100, (fmt, "capped, frozen tables"), family="persistent")
            gix.set_visited_bits(0)
    finally:
        gix.set_visited_bits(0)
        gix.set_max_concurrency(0)
        gix.set_visited_format(0)


@pytest.mark.parametrize("dtype", [oracle.F32, oracle.F16])
def test_scheduled_launch_against_caller_order(dtype, capfd):
    key = (dtype, 24, 1, False)
    _, gix, _, _, _ = _index(*key)
    try:
        gix.debug_set(sched_min_queries=512, verbose=1)
        for off, words in ((NO_TEAMS, "sorted by nearest pivot"), (NO_TEAMS | 128, "in caller order")):
            gix.debug_set(tune_off=off)
            for L in (26, 100):
                capfd.readouterr()
                _check(key, 1000, L, (off, L))
                assert words in capfd.readouterr().err, (off, L)
    finally:
        gix.debug_set(tune_off=NO_TEAMS, sched_min_queries=None, verbose=None)


def test_a_hop_without_survivors():
    """node X repeats the start point's adjacency list and is the query itself: it is expanded right after the start
    point and finds every neighbour visited"""
    rng = np.random.default_rng(77)
    R, x = 64, 1234
    data = rand_vectors(rng, oracle.F32, N, DIM)
    adj = random_graph(rng, N, R, min_len=R)
    adj[N, 1] = x
    adj[x] = adj[N]
    adj_empty = adj.copy()
    adj_empty[x, 0] = 0
    query = data[x:x + 1].copy()
    oix, gix = make_pair(oracle.F32, oracle.L2, data, adj, data[:1], R)
    gix.debug_set(tune_off=NO_TEAMS)
    oix_empty = oracle.Index(oracle.F32, oracle.L2, DIM, N, R, data[:1])
    oix_empty.set_rows(0, data)
    oix_empty.adj[:] = adj_empty
    for L in (5, 26, 100):
        oi, od, oc, ost = oix.search_batch(query, L, 1, 10)
        ei, _, _, est = oix_empty.search_batch(query, L, 1, 10)
        assert oi[0, 0] == x and np.array_equal(oi, ei) and np.array_equal(ost[:, :2], est[:, :2]), L
        for fmt in (32, 16):
            gix.set_visited_format(fmt)
            (gi, gd, gst), fam = gix.last_family(lambda: gix.search(da.Knn(L, 1), query, 10))
            assert fam == {"one_wave"}, fam
            assert np.array_equal(oi, gi) and np.array_equal(bits(od), bits(gd)), (L, fmt)
            assert gst["cmps"][0] == ost[0, 0] and gst["hops"][0] == ost[0, 1] and gst["written"][0] == oc[0], (L, fmt)
