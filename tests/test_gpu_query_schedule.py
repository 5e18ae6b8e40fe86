"""Locality scheduling of large Knn launches (query_schedule.hip): the queries of a launch run grouped by nearest pivot
and dealt to the XCDs in contiguous runs.  Only the order in which queries run may change -- ids, distance bits, the
statistics of every query must be exactly those of the caller-order launch (DANN_DBG_TUNE_OFF bit 128), also when
queries overflow their visited tables and are re-run.  The slot map itself: tests/test_query_schedule_host.py."""
import numpy as np
import pytest

import oracle
from helpers import bits, make_pair, rand_vectors, random_graph

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")


def _blobs(rng, dtype, n, dim, nblobs=32):
    centres = rng.uniform(0, 100, (nblobs, dim)).astype(np.float32)
    x = centres[rng.integers(0, nblobs, n)] + rng.normal(0, 4, (n, dim)).astype(np.float32)
    return x.astype(np.float16 if dtype == oracle.F16 else np.float32)


def _run(gix, capfd, q, L, k, sched):
    gix.debug_set(tune_off=0 if sched else 128)
    gix.kernel_time_reset()
    ids, d, st = gix.search(da.Knn(L), q, k)
    err = capfd.readouterr().err
    return ids, d, st, err


@pytest.mark.parametrize("dtype,persistent", [(oracle.F32, False), (oracle.F16, False), (oracle.F32, True)])
def test_scheduled_launch_equals_caller_order(dtype, persistent, capfd):
    rng = np.random.default_rng(7 + dtype)
    n, dim, R, nq = 6000, 128, 32, 5000
    data = _blobs(rng, dtype, n, dim)
    adj = random_graph(rng, n, R)
    _, gix = make_pair(dtype, oracle.L2, data, adj, data[:1], R)
    q = _blobs(rng, dtype, nq, dim)
    gix.debug_set(sched_min_queries=1024, verbose=1, pair_min_queries=1 << 30)
    if persistent:
        gix.set_max_concurrency(1024)
    for L, k in ((26, 10), (64, 10)):
        ri, rd, rs, rerr = _run(gix, capfd, q, L, k, sched=False)
        si, sd, ss, serr = _run(gix, capfd, q, L, k, sched=True)
        assert "in caller order" in rerr and "sorted by nearest pivot" in serr, (rerr, serr)
        assert ("persistent" in serr) == persistent
        assert not rs["status"].any() and not ss["status"].any()
        assert np.array_equal(ri, si), L
        assert np.array_equal(bits(rd), bits(sd)), L
        assert np.array_equal(rs, ss), L


def test_scheduled_launch_with_retries_equals_caller_order(capfd):
    """a tiny explicit visited table: queries exhaust their table and the spill pool and are re-run (unscheduled)"""
    rng = np.random.default_rng(11)
    n, dim, R, nq = 20000, 128, 32, 4096
    data = _blobs(rng, oracle.F32, n, dim)
    adj = random_graph(rng, n, R)
    _, gix = make_pair(oracle.F32, oracle.L2, data, adj, data[:1], R)
    q = _blobs(rng, oracle.F32, nq, dim)
    gix.debug_set(sched_min_queries=1024, verbose=1, pair_min_queries=1 << 30)
    gix.set_visited_bits(8)
    L, k = 200, 10
    ri, rd, rs, rerr = _run(gix, capfd, q, L, k, sched=False)
    retried_ref = gix.kernel_time(4)[1]
    si, sd, ss, serr = _run(gix, capfd, q, L, k, sched=True)
    retried = gix.kernel_time(4)[1]
    assert "in caller order" in rerr and "sorted by nearest pivot, 8 XCD runs" in serr
    assert retried_ref > 0 and retried > 0, (retried_ref, retried)
    assert np.array_equal(ri, si)
    assert np.array_equal(bits(rd), bits(sd))
    assert np.array_equal(rs, ss)


def test_pivots_follow_mutations(capfd):
    """a mutation marks the pivots stale; the next scheduled launch rebuilds them and still returns the same results"""
    rng = np.random.default_rng(5)
    n, dim, R, nq = 4000, 64, 24, 3000
    data = _blobs(rng, oracle.F32, n, dim)
    adj = random_graph(rng, n, R)
    _, gix = make_pair(oracle.F32, oracle.L2, data, adj, data[:1], R)
    q = _blobs(rng, oracle.F32, nq, dim)
    gix.debug_set(sched_min_queries=1024, verbose=1, pair_min_queries=1 << 30)
    before = _run(gix, capfd, q, 32, 10, sched=True)
    gix.set_elements(0, data[:100][::-1].copy())
    for sched in (True, False, True):
        got = _run(gix, capfd, q, 32, 10, sched=sched)
        assert np.array_equal(got[2]["status"], np.zeros(nq, got[2]["status"].dtype))
        if sched:
            ref = got
        else:
            assert np.array_equal(ref[0], got[0]) and np.array_equal(bits(ref[1]), bits(got[1]))
            assert np.array_equal(ref[2], got[2])
    assert before[0].shape == ref[0].shape
