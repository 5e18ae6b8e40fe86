"""beam_search_kernel swept over the table of tests/search_matrix.py: every case against the oracle (its SQ-8 / U8 twins
for the packed rows, the CPU model's search for the spherical inner product and Cosine) -- ids, distance bits, cmps, hops,
written / result_count, status 0 and the kernel family the table names.  tests/test_search_matrix_host.py checks, without a
GPU, that the table reaches every leaf it is meant to reach and that its inputs fill the queues."""
import os

import numpy as np
import pytest

import search_matrix as sm
from helpers import bits as fbits, teams_on

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

DA_DTYPE = {"F32": da.F32, "F16": da.F16, "U8": da.U8, "I8": da.I8, "SQ8": da.SQ8, "SQ4": da.SQ4, "SQ1": da.SQ1, "SPH1": da.SPH1,
            "SPH2": da.SPH2, "SPH4": da.SPH4, "PQ": da.PQ}
# what the suite's whole-run mode (tests/conftest.py, Provider.__init__) gives every index: a case that sets a knob puts
# these back, not the library's defaults
BASE_TUNE_OFF = int(os.environ.get("DANN_TUNE_OFF", "0") or 0, 0)
BASE_VISITED_FORMAT = int(os.environ.get("DANN_TEST_VISITED_FORMAT", "0") or 0)

_current = {}


@pytest.fixture(scope="module")
def index_of():
    """the index of a group, built on first use; the cases come grouped, so one index is alive at a time"""
    def get(group):
        if _current.get("group") != group:
            old = _current.pop("built", None)
            if old is not None and old.gix is not None:
                old.gix.close()
            _current["group"], _current["built"] = group, sm.Built(group, gpu=True)
        return _current["built"]
    yield get
    old = _current.pop("built", None)
    _current.pop("group", None)
    if old is not None and old.gix is not None:
        old.gix.close()


def _tune_off(gix, extra):
    v = BASE_TUNE_OFF | extra
    gix.debug_set(tune_off=v if v else None)


def _check(c, got, want, what=""):
    gi, gd, gst = got
    ids, d, cmps, hops, written, count = want
    tag = (sm.case_id(c), what)
    assert np.array_equal(gi, ids), tag
    assert np.array_equal(fbits(gd), fbits(d)), tag
    assert np.array_equal(gst["cmps"], cmps) and np.array_equal(gst["hops"], hops), tag
    assert np.array_equal(gst["written"], written) and np.array_equal(gst["result_count"], count), tag
    assert not gst["status"].any(), tag


def _family(c, teams=True):
    return "one_wave" if c.family == "team" and not (teams and teams_on()) else c.family


CASES = [c for cases in sm.groups_in_order().values() for c in cases]


@pytest.mark.parametrize("c", CASES, ids=sm.case_id)
def test_case(c, index_of):
    b = index_of(c.group)
    gix, g = b.gix, c.group
    q = b.q_gpu[:c.nq]
    # PQ rows through beam_search_kernel, not the lookup-table kernel (tests/test_gpu_pqlut.py has that one)
    base_extra = 32 if g.rt == "PQ" else 0
    try:
        _tune_off(gix, base_extra)
        if c.vfmt:
            gix.set_visited_format(c.vfmt)
        if c.loop == "persistent":
            gix.set_max_concurrency(sm.MAX_CONCURRENCY)
        if c.kind == "toolong":
            with pytest.raises(da.DannError) as e:
                gix.search(da.Knn(c.L, c.W), q, sm.K)
            assert e.value.status == da._ffi.EUNSUPPORTED
        elif c.kind == "refused":
            # L + start points = 257: launch_one refuses the server's QS = 8 instantiation before anything is launched,
            # and dann_server_start hands that status to its caller (server.hip: the first launch, under the start)
            with pytest.raises(da.DannError) as e:
                gix.server_start(c.L, sm.K, workers=32)
            assert e.value.status == da._ffi.EUNSUPPORTED
        elif c.loop == "server":
            want = b.reference(c)
            before = gix.search_families()
            gix.server_start(c.L, sm.K, workers=32)
            try:
                tickets = [gix.submit(q[i]) for i in range(c.nq)]
                for i, t in enumerate(tickets):
                    ids, d, st = gix.wait(t)
                    assert np.array_equal(ids, want[0][i]) and np.array_equal(fbits(d), fbits(want[1][i])), (sm.case_id(c), i)
                    assert (int(st["cmps"]), int(st["hops"]), int(st["written"]), int(st["result_count"]), int(st["status"])) == \
                        (int(want[2][i]), int(want[3][i]), int(want[4][i]), int(want[5][i]), 0), (sm.case_id(c), i)
            finally:
                gix.server_stop()
            after = gix.search_families()
            assert {f for f in after if after[f][0] > before[f][0]} == {"server"}
        elif c.kind == "knn":
            want = b.reference(c)
            got, fam = gix.last_family(lambda: gix.search(da.Knn(c.L, c.W), q, sm.K))
            _check(c, got, want)
            assert fam == {_family(c)}, (sm.case_id(c), fam)
            if c.team:  # as test_team_of_wavefronts_per_query_does_not_change_results: once more, one wave per query
                _tune_off(gix, base_extra | 4)
                got, fam = gix.last_family(lambda: gix.search(da.Knn(c.L, c.W), q, sm.K))
                _check(c, got, want, "tune_off=4")
                assert fam == {"one_wave"}, (sm.case_id(c), fam)
        else:
            want = b.reference(c)
            match = (b.match_adaptive if c.kind == "adaptive" else b.match)[:c.nq]
            mode = da.FILTER_MULTIHOP if c.kind == "multihop" else None
            got, fam = gix.last_family(lambda: gix.filtered_search(da.Knn(c.L, c.W), q, sm.K, match, mode=mode, adaptive=c.adaptive))
            gi, gd, gst = got
            ids, d, cmps, hops, written, _ = want
            for j in range(c.nq):  # the assertions of test_inline_random_vs_oracle / test_multihop_random_vs_oracle
                assert np.array_equal(gi[j], ids[j]) and np.array_equal(fbits(gd[j]), fbits(d[j])), (sm.case_id(c), j)
                assert (int(gst["cmps"][j]), int(gst["hops"][j]), int(gst["written"][j])) == (cmps[j], hops[j], written[j]), (sm.case_id(c), j)
            assert not gst["status"].any(), sm.case_id(c)
            assert fam == {"one_wave"}, (sm.case_id(c), fam)
    finally:
        gix.debug_set(tune_off=BASE_TUNE_OFF if BASE_TUNE_OFF else None)
        gix.set_max_concurrency(0)
        gix.set_visited_format(BASE_VISITED_FORMAT)


@pytest.mark.parametrize("rt,metric", sm.UNSUPPORTED_PAIRS, ids=lambda v: str(v))
def test_unsupported_metric_is_refused_not_searched(rt, metric):
    kw = dict(sq_scale=1.0) if rt in sm.SQ_BITS else {}
    if rt == "PQ":
        kw = dict(pq_pivots=np.zeros((256, 16), np.float32), pq_offsets=np.arange(0, 17, 4, dtype=np.uint32))
    width = 4 if rt == "PQ" else sm.layer_bytes(rt, 16)
    with pytest.raises(da.DannError) as e:
        da.Provider(DA_DTYPE[rt], metric, 16, 10, 4, np.zeros((1, width), np.uint8), **kw)
    assert e.value.status == da._ffi.EUNSUPPORTED
