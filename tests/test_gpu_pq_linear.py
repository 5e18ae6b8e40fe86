"""dann_pq_linear_search_batch(_device) on the GPU against tests/pq_linear_model.py: ids, distance BITS and statistics equal
to the model -- the oracle's lookup tables and table sums, tests/flat_model.py's selection.  Everything is bit-exact; no
tolerance anywhere.  The host side: tests/test_pq_linear_model_host.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flat_model as fm
import oracle
import pq_linear_model as pm
from helpers import bits as fbits, random_graph
from test_gpu_spherical import DevBuf

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

EMPTY = pm.EMPTY
# rows one workgroup scores per step (lane = row): the two sizes of the scan's workgroup
_PLAN = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diskann_amd", "csrc", "flat_pq_plan.h")).read()
STEP, WIDE_STEP = (int(re.search(name + r" = (\d+);", _PLAN).group(1)) for name in ("kFlatPqThreads", "kFlatPqWideThreads"))
CUT = 1500  # a forced chunk length that is not a multiple of a step


def check(gix, q, want, k, tag, **kw):
    """the host form against (ids, dists, written, cmps)"""
    ids, d, st = gix.pq_linear_search(q, k, stats=True, **kw)
    wi, wd, wn, wc = want
    assert np.array_equal(ids, wi), tag + ("ids",)
    assert np.array_equal(fbits(d), fbits(wd)), tag + ("distance bits",)
    assert np.array_equal(st["cmps"], wc) and (st["hops"] == 0).all() and (st["status"] == 0).all(), tag + ("stats",)
    assert np.array_equal(st["written"], wn) and np.array_equal(st["result_count"], wn), tag + ("written",)
    return ids, d, st


def sweep(c, q, D, slots, ks, tag, cuts=(None, CUT), accept=None, **kw):
    """every k with the default cut and a forced one: equal to the model, hence identical with and without the cut"""
    for cut in cuts:
        c.gix.debug_set(flat_chunk_rows=cut)
        for k in ks:
            check(c.gix, q, pm.expect(D, slots, k, accept), k, tag + (cut, k), **kw)
    c.gix.debug_set(flat_chunk_rows=None)


# ---- chunk counts: either side of every code-row load width (16-byte pieces) and of the tile-shrinking LDS limits ----------
@pytest.mark.parametrize("metric", [oracle.L2, oracle.INNER_PRODUCT])
@pytest.mark.parametrize("chunks", [1, 3, 4, 5, 16, 17, 37, 64, 65, 128])
def test_chunk_counts(chunks, metric):
    dim = chunks + (0 if chunks in (4, 128) else 3)  # (dim == chunks: every chunk holds one element)
    c = pm.PqCase(da, 100 + 2 * chunks + metric, metric, dim, chunks, 700)
    lens = np.diff(c.offsets.astype(np.int64))
    assert chunks == 1 or (lens.min() == 1 and (dim == chunks or len(set(lens.tolist())) > 1))
    q = c.queries(9)
    D = c.D(q)
    sweep(c, q, D, c.slots[:700], (1, 10), (chunks, metric), cuts=(None, 300))
    c.close()


# ---- row counts around one step of a workgroup and around a chunk boundary -------------------------------------------------
@pytest.fixture(scope="module")
def rows16():
    c = pm.PqCase(da, 7, oracle.L2, 40, 16, 2 * CUT + 2, nstart=2)
    q = c.queries(17)
    yield c, q, c.D(q)
    c.close()


@pytest.mark.parametrize("n", [STEP - 1, STEP, STEP + 1, CUT - 1, CUT, CUT + 1, 2 * CUT, 2 * CUT + 1])
def test_row_counts(rows16, n):
    c, q, D = rows16
    sweep(c, q[:3], D[:3], c.slots[:n], (10,), ("rows", n), n=n)


def test_wide_workgroup(rows16):
    """so many queries that their tiles alone fill the device (two workgroups a compute unit, up to 512 compute units): the
    scan runs its wide workgroup.  4 101 queries, 16 distinct ones tiled; rows around one step of it and a chunk boundary"""
    c, q, D = rows16
    nq = 4101
    rep = np.arange(nq) % 16
    qq = np.ascontiguousarray(q[rep])
    for n in (WIDE_STEP - 1, WIDE_STEP, WIDE_STEP + 1, 2 * CUT + 1):
        for cut, k in ((None, 10), (CUT, 10), (None, 1024)):
            wi, wd, wn, wc = pm.expect(D[:16], c.slots[:n], k)
            c.gix.debug_set(flat_chunk_rows=cut)
            check(c.gix, qq, (wi[rep], wd[rep], wn[rep], wc[rep]), k, ("wide", n, cut, k), n=n)
    c.gix.debug_set(flat_chunk_rows=None)


# ---- query counts: every tile size and a ragged last tile ------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2, 3, 5, 9, 17])
def test_query_counts(rows16, nq):
    c, q, D = rows16
    sweep(c, q[:nq], D[:nq], c.slots[:700], (10,), ("nq", nq), n=700)


# ---- k ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 257, 1024])
def test_k(rows16, k):
    c, q, D = rows16
    n = 2 * CUT + 2
    sweep(c, q[:3], D[:3], c.slots[:n], (k,), ("k", k), n=n)


def test_fewer_rows_than_k_and_empty_calls(rows16):
    c, q, D = rows16
    slots = c.slots[40:45]
    want = pm.expect(D[:3], slots, 10)
    ids, d, _ = check(c.gix, q[:3], want, 10, ("k > n",), first=40, n=5)
    assert (want[2] == 5).all() and (ids[:, 5:] == EMPTY).all() and np.isposinf(d[:, 5:]).all()
    ids, d, st = c.gix.pq_linear_search(q[:3], 4, first=3, n=0, stats=True)
    assert (ids == EMPTY).all() and np.isposinf(d).all()
    assert not st["cmps"].any() and not st["written"].any() and not st["result_count"].any() and not st["hops"].any()
    ids, d = c.gix.pq_linear_search(np.zeros((0, c.dim), np.float32), 4)
    assert ids.shape == (0, 4) and d.shape == (0, 4)


def test_sub_range_with_the_start_points(rows16):
    c, q, D = rows16
    n = 2 * CUT + 2
    slots = c.slots[n - 200:]  # the two start-point slots are part of the range
    assert len(slots) == 202
    sweep(c, q[:5], D[:5], slots, (10, 257), ("sub-range",), cuts=(None, 64), first=n - 200, n=202)


# ---- ties ------------------------------------------------------------------------------------------------------------------
def test_duplicate_code_rows_tie_and_the_later_slot_wins():
    rng = np.random.default_rng(21)
    chunks, n = 5, 2 * CUT + 100
    distinct = rng.integers(0, 256, (6, chunks), dtype=np.uint8)
    codes = distinct[rng.integers(0, 6, n + 1)]
    c = pm.PqCase(da, 22, oracle.L2, 11, chunks, n, codes=codes)
    q = c.queries(3)
    D = c.D(q)
    assert all(len(np.unique(r)) <= 6 for r in D)
    sweep(c, q, D, c.slots[:n], (10, 64, 1024), ("ties",), n=n)
    # in words: the best code row's last k copies, latest first -- across the chunk boundary at CUT too
    c.gix.debug_set(flat_chunk_rows=CUT)
    k = 1024
    ids, d = c.gix.pq_linear_search(q, k, n=n)
    for j in range(3):
        best = np.flatnonzero(D[j, :n] == D[j, :n].min())[::-1]
        m = min(k, len(best))
        assert ids[j, :m].tolist() == best[:m].tolist()
        assert best[:m].min() < CUT < best[:m].max()
        pos, md = fm.flat_knn(D[j, :n], 10)  # and by the literal inserts
        assert ids[j, :10].tolist() == pos.tolist() and np.array_equal(fbits(d[j, :10]), fbits(md))
    c.gix.debug_set(flat_chunk_rows=None)
    c.close()


# ---- special values --------------------------------------------------------------------------------------------------------
def test_nan_query_gives_an_empty_result_and_counts_every_row(rows16):
    c, q, D = rows16
    qn = q[:2].copy()
    qn[0, :] = np.nan  # (every chunk's entries are NaN: every sum is)
    Dn = c.D(qn)
    assert np.isnan(Dn[0]).all() and not np.isnan(Dn[1]).any()
    for cut in (None, CUT):
        c.gix.debug_set(flat_chunk_rows=cut)
        ids, d, st = check(c.gix, qn, pm.expect(Dn, c.slots[:2000], 10), 10, ("nan", cut), n=2000)
        assert (ids[0] == EMPTY).all() and np.isposinf(d[0]).all() and st["cmps"][0] == 2000 and st["written"][0] == 0
    c.gix.debug_set(flat_chunk_rows=None)


@pytest.mark.parametrize("metric", [oracle.L2, oracle.INNER_PRODUCT])
def test_pivot_table_with_infinite_entries(metric):
    rng = np.random.default_rng(23)
    dim, chunks, n = 12, 4, 1800
    pivots = rng.standard_normal((256, dim)).astype(np.float32)
    pivots[rng.integers(0, 256, 30), rng.integers(0, dim, 30)] = np.inf
    pivots[rng.integers(0, 256, 30), rng.integers(0, dim, 30)] = -np.inf
    c = pm.PqCase(da, 24, metric, dim, chunks, n, pivots=pivots)
    q = c.queries(5)
    with np.errstate(invalid="ignore"):
        D = c.D(q)
    assert np.isinf(D).any() and (metric == oracle.L2 or (np.isnan(D).any() and np.isneginf(D).any()))
    sweep(c, q, D, c.slots[:n], (10, 257), ("inf", metric))
    c.close()


# ---- tags, deletes and filters ---------------------------------------------------------------------------------------------
def test_inline_tags_skip_unpublished_slots():
    c = pm.PqCase(da, 25, oracle.L2, 20, 17, 1700, tags=True)
    rng = c.rng
    tags = np.full(1700, pm.TAG_PUBLISHED, np.uint8)
    hidden = rng.choice(1700, 300, replace=False)
    tags[hidden] = rng.choice(pm.HIDDEN_TAGS, 300)
    c.gix.set_tags(0, tags)
    assert np.array_equal(c.gix.get_tags(0, 1700), tags) and c.gix.get_tags(1700, 1)[0] >= pm.TAG_PUBLISHED
    q = c.queries(9)
    D = c.D(q)
    seen = np.setdiff1d(c.slots, hidden)  # (the start point, FROZEN, is readable)
    sweep(c, q, D, seen, (10, 1024), ("tags",), n=1701)
    c.close()


def test_skip_deleted_flag():
    n = 2 * CUT
    c = pm.PqCase(da, 26, oracle.INNER_PRODUCT, 9, 3, n)
    q = c.queries(5)
    D = c.D(q)
    every = c.slots[:n]
    # before any delete there is no deleted state: the flag changes nothing
    check(c.gix, q, pm.expect(D, every, 10), 10, ("no bitmap",), skip_deleted=True)
    gone = c.rng.choice(n, 900, replace=False).astype(np.uint32)
    c.gix.delete_points(gone)
    keep = np.setdiff1d(every, gone)
    sweep(c, q, D, every, (10, 257), ("flag off",))
    sweep(c, q, D, keep, (10, 257), ("flag on",), skip_deleted=True)
    c.close()


def test_filters(rows16):
    c, q, D = rows16
    n = 2 * CUT + 2
    nq, nslots = 9, n + 2
    rng = np.random.default_rng(27)
    shared = rng.random(nslots) < 0.3
    per_query = rng.random((nq, nslots)) < rng.random((nq, 1))
    per_query[3] = False  # a query that accepts nothing
    slots = c.slots[10:n + 1]
    kw = dict(first=10, n=len(slots))
    sweep(c, q[:nq], D[:nq], slots, (10, 257), ("shared",), accept=shared, match=shared, **kw)
    sweep(c, q[:nq], D[:nq], slots, (10, 257), ("per query",), accept=per_query, match=per_query, **kw)
    # an all-ones bitmap equals no filter in every output
    for match in (np.ones(nslots, bool), np.ones((nq, nslots), bool)):
        a = c.gix.pq_linear_search(q[:nq], 10, stats=True, **kw)
        b = c.gix.pq_linear_search(q[:nq], 10, stats=True, match=match, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(fbits(a[1]), fbits(b[1])) and np.array_equal(a[2], b[2])


def test_device_pointer_form_equals_the_host_form(rows16):
    c, q, D = rows16
    gix, nq, k, n = c.gix, 9, 10, 2 * CUT + 2
    rng = np.random.default_rng(28)
    per_query = rng.random((nq, n + 2)) < 0.5
    dq = DevBuf(q[:nq].nbytes, q[:nq])
    di, dd, ds = DevBuf(nq * k * 4), DevBuf(nq * k * 4), DevBuf(nq * da.STATS_DTYPE.itemsize)
    for match in (None, per_query[0], per_query):
        hi, hd, hs = gix.pq_linear_search(q[:nq], k, n=n, stats=True, match=match)
        kw = {}
        if match is not None:
            f, words = gix._flat_filter(match, nq)
            dbits = DevBuf(words.nbytes, words)
            kw = dict(d_bits=dbits.p.value, stride_words=int(f.stride_words))
        gix.pq_linear_search_device(dq.p.value, nq, k, di.p.value, dd.p.value, n=n, d_stats=ds.p.value, **kw)
        assert np.array_equal(di.get(np.uint32, (nq, k)), hi)
        assert np.array_equal(dd.get(np.uint32, (nq, k)), fbits(hd))
        assert np.array_equal(ds.get(da.STATS_DTYPE, (nq,)), hs)
    gix.pq_linear_search_device(dq.p.value, nq, k, di.p.value, dd.p.value, n=n)  # the statistics are optional
    assert np.array_equal(di.get(np.uint32, (nq, k)), gix.pq_linear_search(q[:nq], k, n=n)[0])


# ---- a second reference, on the device -------------------------------------------------------------------------------------
def test_equals_build_lut_and_scan(rows16):
    c, q, D = rows16
    n, k = 2 * CUT + 2, 10
    lut = da.pq_build_lut(c.metric, c.pivots, c.offsets, q[:5])
    every = np.tile(np.arange(n, dtype=np.uint32), 5)
    off = (np.arange(6) * n).astype(np.uint64)
    scanned = da.pq_scan(lut, c.codes, every, off).reshape(5, n)
    assert np.array_equal(fbits(scanned), fbits(D[:5, :n]))
    ids, d = c.gix.pq_linear_search(q[:5], k, n=n)
    for j in range(5):
        pos, md = fm.flat_knn_closed(scanned[j], k)
        assert ids[j].tolist() == pos.tolist() and np.array_equal(fbits(d[j]), fbits(md))


# ---- the graph searches never beat the scan --------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [oracle.L2, oracle.INNER_PRODUCT])
def test_graph_search_never_beats_the_scan(metric):
    rng = np.random.default_rng(29 + metric)
    n, dim, chunks, R, k = 1000, 37, 16, 16, 10
    offsets = pm.uneven_offsets(rng, dim, chunks)
    pivots = rng.standard_normal((256, dim)).astype(np.float32)
    codes = rng.integers(0, 256, (n + 1, chunks), dtype=np.uint8)
    gix = da.Provider(da.PQ, metric, dim, n, R, codes[n:], pq_pivots=pivots, pq_offsets=offsets)
    gix.set_elements(0, codes[:n])
    gix.upload_graph(random_graph(rng, n, R))
    q = rng.standard_normal((20, dim)).astype(np.float32)
    all_i, all_d = gix.pq_linear_search(q, n)  # every row's distance, in the scan's order
    assert (all_i != EMPTY).all()
    order = lambda ids, d: sorted(zip(d.tolist(), (-ids.astype(np.int64)).tolist()))  # noqa: E731

    def never_better(family):
        (gi, gd, gst), fam = gix.last_family(lambda: gix.search(da.Knn(48, 1), q, k))
        assert fam == {family}, fam
        for j in range(len(q)):
            got = gi[j] != EMPTY
            assert got.any()
            of = dict(zip(all_i[j].tolist(), fbits(all_d[j]).tolist()))
            assert [of[i] for i in gi[j][got].tolist()] == fbits(gd[j][got]).tolist(), (family, j)
            mine, scan = order(gi[j][got], gd[j][got]), order(all_i[j][:k], all_d[j][:k])
            assert all(m >= s for m, s in zip(mine, scan)), (family, j)

    gix.debug_set(tune_off=32)
    never_better("one_wave")  # beam_search_kernel<DT_PQ>
    gix.debug_set(tune_off=None)
    never_better("pq_lut")    # the register-table kernel
    gix.pq_pack_neighbors()
    never_better("pq_lut")    # and on the packed layout
    gix.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors(rows16):
    c, q, D = rows16
    gix, n, nq = c.gix, 2 * CUT + 2, 3
    L, E = da.lib(), da._ffi
    ids, d = np.zeros((nq, 4), np.uint32), np.zeros((nq, 4), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    words = (n + 2 + 31) // 32
    bitmap = np.full(nq * words, 0xFFFFFFFF, np.uint32)

    def call(fn=L.dann_pq_linear_search_batch, h=gix._h, queries=p(q), nq=nq, first=0, n=n, k=4, flags=0, f=None, oi=p(ids),
             od=p(d)):
        return fn(h, queries, nq, first, n, k, flags, f, oi, od, None)

    assert call() == E.OK
    for fn in (L.dann_pq_linear_search_batch, L.dann_pq_linear_search_batch_device):
        assert call(fn, k=0) == E.EINVAL
        assert call(fn, flags=2) == E.EINVAL and call(fn, flags=0x80000001) == E.EINVAL
        assert call(fn, queries=None) == E.EINVAL and call(fn, oi=None) == E.EINVAL and call(fn, od=None) == E.EINVAL
        assert call(fn, n=n + 3) == E.EBOUNDS and call(fn, first=n + 2, n=1) == E.EBOUNDS
        assert call(fn, first=0xFFFFFFFF, n=0xFFFFFFFF) == E.EBOUNDS
        assert call(fn, k=1025) == E.EUNSUPPORTED
        short = E.FlatFilter(bitmap.ctypes.data, words - 1)
        assert call(fn, f=C.byref(short)) == E.EINVAL
        assert call(fn, h=None) == E.EINVAL
        # no queries: nothing is read or written, whatever the pointers
        assert call(fn, queries=None, nq=0, oi=None, od=None) == E.OK
    assert call(n=n + 2) == E.OK and call(first=n + 2, n=0) == E.OK
    assert call(f=C.byref(E.FlatFilter(bitmap.ctypes.data, words))) == E.OK
    assert call(f=C.byref(E.FlatFilter(None, 0))) == E.OK  # null bits: every slot matches
    # the flat scans keep refusing PQ rows
    with pytest.raises(da.DannError) as e:
        gix.flat_search(q[:2], 3)
    assert e.value.status == E.EUNSUPPORTED
    with pytest.raises(da.DannError) as e:
        gix.flat_range_search(q[:2], 1.0)
    assert e.value.status == E.EUNSUPPORTED


def test_other_row_types_and_a_missing_table_are_refused():
    E, L = da._ffi, da.lib()
    rng = np.random.default_rng(30)
    data = rng.standard_normal((21, 16)).astype(np.float32)
    fix = da.Provider(da.F32, da.L2, 16, 20, 4, data[20:])
    fix.set_elements(0, data[:20])
    with pytest.raises(da.DannError) as e:
        fix.pq_linear_search(data[:2], 3)
    assert e.value.status == E.EUNSUPPORTED
    fix.close()
    # a PQ index whose pivot table was never attached
    start = rng.integers(0, 256, (1, 4), dtype=np.uint8)
    cfg = E.Config(da.PQ, da.L2, 16, 20, 4, 1, 0, -1, 0.0, 0.0, 4, 0)
    h = C.c_void_p()
    assert L.dann_index_create(C.byref(cfg), start.ctypes.data_as(C.c_void_p), start.nbytes, C.byref(h)) == E.OK
    ids, d = np.zeros((2, 3), np.uint32), np.zeros((2, 3), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for fn in (L.dann_pq_linear_search_batch, L.dann_pq_linear_search_batch_device):
        assert fn(h, p(data), 2, 0, 20, 3, 0, None, p(ids), p(d), None) == E.EINVAL
    L.dann_index_destroy(h)
