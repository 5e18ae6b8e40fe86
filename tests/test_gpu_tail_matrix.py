"""Range search's second phase, filtered range search and paged search swept over the table of tests/tail_matrix.py: one
test per index, every case of it against the oracle (its twins for the packed rows) -- ids, distance bits, result_count /
written, cmps, hops and second_round of the range searches; ids, distance bits and counts of every page -- with no
tolerance anywhere.  The limits (out_cap, the scratch list, matched_cap, list_cap) must be refused with DANN_EOVERFLOW and
leave the index as it was.  tests/test_tail_matrix_host.py checks, without a GPU, that the table's inputs reach the loops
the table is for."""
import os

import numpy as np
import pytest

import search_matrix as sm
import tail_matrix as tm
from helpers import bits as fbits

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

BASE_TUNE_OFF = int(os.environ.get("DANN_TUNE_OFF", "0") or 0, 0)
BASE_VISITED_FORMAT = int(os.environ.get("DANN_TEST_VISITED_FORMAT", "0") or 0)
EMPTY = 0xFFFFFFFF


def _search(b, c, q, **override):
    """the range / filtered range call of case c; out_cap: every slot, unless overridden"""
    kw = {**b.range_kw(c), "out_cap": b.nslots, **override}
    if c.sec.startswith("frange"):
        f = tm.opt(c, "filter")
        match = b.match[f] if f == "shared" else b.match[f][:q.shape[0]]
        L, radius = kw.pop("starting_l"), kw.pop("radius")
        return b.gix.filtered_range_search(q, L, radius, match, **kw)
    return b.gix.range_search(q, **kw)


def _same_lists(c, got, ref, what=""):
    gi, gd, gst, gsec = got
    for j, (oi, od, ost) in enumerate(ref):
        tag, k = (tm.case_id(c), what, j), len(oi)
        assert int(gst["status"][j]) == 0, tag
        assert (int(gst["result_count"][j]), int(gst["written"][j])) == (k, k), (tag, int(gst["result_count"][j]), k)
        assert np.array_equal(gi[j, :k], oi) and np.array_equal(fbits(gd[j, :k]), fbits(od)), tag
        assert (gi[j, k:] == EMPTY).all() and np.isposinf(gd[j, k:]).all(), tag
        assert (int(gst["cmps"][j]), int(gst["hops"][j]), int(gsec[j])) == (int(ost[0]), int(ost[1]), int(ost[3])), tag


def _refused(status, fn):
    with pytest.raises(da.DannError) as e:
        fn()
    assert e.value.status == status


def _knn_still_right(b):
    """after a refused call: a Knn search on the same index, scratch and spill tables, equals the oracle's"""
    q = b.q_gpu[:tm.NQ]
    gi, gd, gst = b.gix.search(da.Knn(64, 1), q, 10)
    oi, od, oc, ost = b.oix.search_batch(b.q_ref[:tm.NQ], 64, 1, 10)
    assert np.array_equal(gi, oi) and np.array_equal(fbits(gd), fbits(od)) and not gst["status"].any()
    assert np.array_equal(gst["cmps"], ost[:, 0]) and np.array_equal(gst["hops"], ost[:, 1])


def run_range(b, c):
    gix = b.gix
    kw = b.range_kw(c)
    q = b.q_gpu[:b.nq(c)]
    if kw.get("max_returned") and kw["max_returned"] < kw["starting_l"]:
        # RangeSearchError::LSmallerThanMaxReturned (range_search.rs:93-131): the reference refuses the parameter set too
        return _refused(da._ffi.EINVAL, lambda: _search(b, c, q))
    ref = b.range_reference(c)
    try:
        if tm.opt(c, "vfmt"):
            gix.set_visited_format(tm.opt(c, "vfmt"))
        if tm.opt(c, "loop") == "persistent":
            gix.set_max_concurrency(tm.MAX_CONCURRENCY)
            got, fam = gix.last_family(lambda: _search(b, c, q))
            assert fam == {"persistent"}, (tm.case_id(c), fam)
        else:
            got = _search(b, c, q)
        _same_lists(c, got, ref)
    finally:
        gix.set_max_concurrency(0)
        gix.set_visited_format(BASE_VISITED_FORMAT)


def run_range_rerun(b, c):
    """a 64-entry visited table: the first phase goes on in a spill table, the second phase's seeding of more than 64
    in-range ids cannot, and the query is run again with a table twice as large until it fits"""
    gix = b.gix
    q = b.q_gpu[:tm.NQ]
    ref = b.range_reference(c)
    before = gix.kernel_time(4)[1]
    try:
        gix.set_visited_bits(6)
        got = _search(b, c, q)
    finally:
        gix.set_visited_bits(0)
    assert gix.kernel_time(4)[1] > before, tm.case_id(c)
    _same_lists(c, got, ref)
    _same_lists(c, _search(b, c, q), ref, "automatic table again")


def run_limits(b, c):
    """out_cap below the longest result list, and (plain range search) a scratch list that the longest list overruns:
    DANN_EOVERFLOW -- the reference's output is unbounded, and a silently shortened list cannot be told from a complete
    one; (filtered) a matched list that the first round overruns.  After every refusal the index answers as before"""
    q = b.q_gpu[:tm.NQ]
    ref = b.range_reference(c)
    longest = max(len(r[0]) for r in ref)
    refusals = [dict(out_cap=longest - 1), dict(out_cap=longest // 2)]
    if c.sec == "range-limits":
        assert longest > 4 * 8 + 1024
        refusals.append(dict(out_cap=8))  # the scratch list: 4 * 8 + 1024 entries, max_returned == 0
    else:
        refusals.append(dict(matched_cap=64))
    for over in refusals:
        _refused(da._ffi.EOVERFLOW, lambda: _search(b, c, q, **over))
        _same_lists(c, _search(b, c, q), ref, f"after {over}")
        _knn_still_right(b)
    _same_lists(c, _search(b, c, q, out_cap=longest), ref, "out_cap == the longest list")


def _same_pages(c, session, ref, sizes, nq, what=""):
    ncalls = max(len(p) for p in ref)
    for i in range(ncalls):
        k = sizes[i % len(sizes)]
        ids, d, cnt = session.next_page(k)
        for j in range(nq):
            oi, od = ref[j][i] if i < len(ref[j]) else ((), ())  # (a drained query stays drained)
            n, tag = len(oi), (tm.case_id(c), what, "call", i, "query", j)
            assert int(cnt[j]) == n, (tag, int(cnt[j]), n)
            assert np.array_equal(ids[j, :n], oi) and np.array_equal(fbits(d[j, :n]), fbits(od)), tag
            assert (ids[j, n:] == EMPTY).all() and np.isposinf(d[j, n:]).all(), tag


def run_paged(b, c):
    L = c.qcap - c.ix.nstart
    sizes = tm.page_sizes(c.pset, L)
    ref = b.paged_reference(L, sizes, None if tm.opt(c, "drain") else tm.page_calls(c.pset))
    s = b.gix.paged_search(b.q_gpu[:tm.NQ], L)
    try:
        _same_pages(c, s, ref, sizes, tm.NQ)
    finally:
        s.close()


def run_paged_limits(b, c):
    L = c.qcap - c.ix.nstart
    s = b.gix.paged_search(b.q_gpu[:tm.NQ], L, list_cap=64)
    try:
        _refused(da._ffi.EOVERFLOW, lambda: s.next_page(7))
    finally:
        s.close()
    _knn_still_right(b)
    s = b.gix.paged_search(b.q_gpu[:tm.NQ], L)  # the default cap
    try:
        _same_pages(c, s, b.paged_reference(L, (7,), 12), (7,), tm.NQ, "default list_cap")
    finally:
        s.close()


def run_paged_interleave(b, c):
    """two sessions of different l_value on one index, page by page in turn"""
    Ls = (c.qcap - c.ix.nstart, 128)
    refs = [b.paged_reference(L, (7,), 12) for L in Ls]
    ss = [b.gix.paged_search(b.q_gpu[:tm.NQ], L) for L in Ls]
    try:
        for i in range(12):
            for s, ref, L in zip(ss, refs, Ls):
                ids, d, cnt = s.next_page(7)
                for j in range(tm.NQ):
                    oi, od = ref[j][i]
                    n = len(oi)
                    assert int(cnt[j]) == n and np.array_equal(ids[j, :n], oi) and np.array_equal(fbits(d[j, :n]), fbits(od)), \
                        (tm.case_id(c), L, i, j)
    finally:
        for s in ss:
            s.close()


def run_paged_refused(b, c):
    _refused(da._ffi.EUNSUPPORTED, lambda: b.gix.paged_search(b.q_gpu[:tm.NQ], c.qcap - c.ix.nstart))


RUN = {"range": run_range, "frange": run_range, "range-rerun": run_range_rerun, "range-limits": run_limits,
       "frange-limits": run_limits, "paged": run_paged, "paged-limits": run_paged_limits,
       "paged-interleave": run_paged_interleave, "paged-refused": run_paged_refused}
INDEXES = tm.by_index()


@pytest.mark.parametrize("ix", list(INDEXES), ids=tm.ix_id)
def test_index(ix):
    b = tm.Built(ix, gpu=True)
    try:
        # PQ rows through beam_search_kernel, as tests/test_gpu_search_matrix.py runs them
        extra = BASE_TUNE_OFF | (32 if ix.rt == "PQ" else 0)
        if extra:
            b.gix.debug_set(tune_off=extra)
        for c in INDEXES[ix]:
            RUN[c.sec](b, c)
    finally:
        b.close()
