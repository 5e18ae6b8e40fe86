"""dann_flat_search_batch(_device) on the GPU against tests/flat_model.py: ids and distance BITS equal to the model, which
is fed the reference distances of the scanned slots -- the oracle's expand_beam where the oracle has the row type (for
the scalar-quantised rows: its SQ-8 twin), else the row type's Python model (spherical_model, minmax_model)."""
import ctypes as C

import numpy as np
import pytest

import flat_model as fm
import minmax_model as mm
import oracle
import spherical_model as sph
from gridutil import grid_start_point
from helpers import bits as fbits, rand_vectors
from minmax_builders import mm_dtype, random_rows as mm_random_rows
from search_builders import SqBitsCase
from test_gpu_spherical import DevBuf, _random_queries as sph_random_queries, _random_rows as sph_random_rows

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

N = 1500                 # two default chunks (1024 + 476); 24 chunks of 64; 15 chunks of 100
NQ = 8 + 3               # one full query tile and a partial one
KS = (1, 10, 65, 1024)   # 65: one more than a wavefront; 1024: the largest k, a 2048-key candidate buffer
CHUNKS = (None, 64, 100)


def oracle_distances(oix, queries, slots):
    """[nq][len(evaluated)] reference distances of `slots` and the slots the reference evaluated (unreadable ones left out)"""
    out, seen = [], None
    for q in queries:
        ids, d = oix.expand_beam(q, slots)
        assert seen is None or np.array_equal(ids, seen)
        seen = ids
        out.append(d)
    return np.stack(out), seen


def expect(D, slots, ks):
    """{k: (ids[nq, k], dists[nq, k], written[nq])} by the closed form: one full ordering per query, cut at every k"""
    res = {k: ([], [], []) for k in ks}
    for row in D:
        pos, d = fm.flat_knn_closed(row, len(row))
        for k in ks:
            i, dd = fm.padded(pos[:k], d[:k], k, slots)
            res[k][0].append(i)
            res[k][1].append(dd)
            res[k][2].append(min(k, len(pos)))
    return {k: (np.stack(v[0]), np.stack(v[1]), np.array(v[2])) for k, v in res.items()}


def check(gix, q, want, k, cmps, tag, **kw):
    ids, d, st = gix.flat_search(q, k, stats=True, **kw)
    wi, wd, wn = want[k]
    assert np.array_equal(ids, wi), tag + ("ids",)
    assert np.array_equal(fbits(d), fbits(wd)), tag + ("distance bits",)
    assert (st["cmps"] == cmps).all() and (st["hops"] == 0).all() and (st["status"] == 0).all(), tag + ("stats",)
    assert np.array_equal(st["written"], wn) and np.array_equal(st["result_count"], wn), tag + ("written",)
    return ids, d


def sweep(gix, q, D, slots, tag, ks=KS, chunks=CHUNKS, **kw):
    """every k under every chunk size: equal to the model, hence identical across chunk sizes"""
    want = expect(D, slots, ks)
    for rows in chunks:
        gix.debug_set(flat_chunk_rows=rows)
        for k in ks:
            check(gix, q, want, k, len(slots), tag + (rows, k), **kw)
    gix.debug_set(flat_chunk_rows=None)


# ---- the reference's goldens ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,size", [(1, 100), (2, 5), (3, 4)])
def test_golden_grids(dims, size):
    """f32 L2 lattices at k in {1, 4, 10}: the golden distance multiset, comparisons and result_count; and the ids of the
    literal sequential inserts (the 2 x 5 and 3 x 4 lattices tie at the k-th place)"""
    rows = fm.grid_rows(dims, size)
    n = len(rows)
    oix = oracle.Index(oracle.F32, oracle.L2, dims, n, 4, grid_start_point(dims, size)[None, :])
    oix.set_rows(0, rows)
    gix = da.Provider(da.F32, da.L2, dims, n, 4, grid_start_point(dims, size)[None, :])
    gix.set_elements(0, rows)
    golden = [r for name, r in fm.golden_rows() if name == f"search_{dims}_{size}"]
    assert len(golden) == 6 and {r["k"] for r in golden} == {1, 4, 10}
    slots = np.arange(n, dtype=np.uint32)
    for r in golden:
        q = np.array([r["query"]], np.float32)
        D, _ = oracle_distances(oix, q, slots)
        for chunk in (None, 7):
            gix.debug_set(flat_chunk_rows=chunk)
            ids, d, st = gix.flat_search(q, r["k"], stats=True)
            assert d[0].tolist() == r["top_k_distances"]
            assert int(st["cmps"][0]) == r["comparisons"] and int(st["result_count"][0]) == r["result_count"]
            pos, md = fm.flat_knn(D[0], r["k"])
            assert ids[0].tolist() == pos.tolist() and np.array_equal(fbits(d[0]), fbits(md))
    gix.close()


# ---- the sweep -----------------------------------------------------------------------------------------------------------
FULL = [(dt, metric, dim) for dt in (oracle.F32, oracle.F16, oracle.U8, oracle.I8)
        for metric in (oracle.L2, oracle.INNER_PRODUCT, oracle.COSINE, oracle.COSINE_NORMALIZED) for dim in (100, 128)]


@pytest.mark.parametrize("dt,metric,dim", FULL)
def test_sweep_full_precision(dt, metric, dim):
    rng = np.random.default_rng(1000 + 100 * dt + 10 * metric + dim)
    data = rand_vectors(rng, dt, N + 1, dim)
    oix = oracle.Index(dt, metric, dim, N, 4, data[N:])
    oix.set_rows(0, data[:N])
    gix = da.Provider(dt, metric, dim, N, 4, data[N:])
    gix.set_elements(0, data[:N])
    q = rand_vectors(rng, dt, NQ, dim)
    slots = np.arange(N, dtype=np.uint32)
    D, seen = oracle_distances(oix, q, slots)
    sweep(gix, q, D, seen, (dt, metric, dim))
    gix.close()


@pytest.mark.parametrize("bits,metric,dim", [(8, m, d) for m in (oracle.L2, oracle.INNER_PRODUCT, oracle.COSINE_NORMALIZED)
                                             for d in (100, 128)] + [(4, oracle.L2, 64), (1, oracle.INNER_PRODUCT, 64)])
def test_sweep_scalar_quantised(bits, metric, dim):
    c = SqBitsCase(bits, metric, N, dim, 4, 2000 + 10 * bits + metric + dim, adj=False)
    _, q, q_twin = c.queries(NQ)
    slots = np.arange(N, dtype=np.uint32)
    D, seen = oracle_distances(c.oix, q_twin, slots)
    sweep(c.gix, q, D, seen, ("SQ", bits, metric, dim))
    c.gix.close()


@pytest.mark.parametrize("bits,layout,metric", [(1, sph.SAME_AS_DATA, sph.L2), (1, sph.FOUR_BIT_TRANSPOSED, sph.IP),
                                                (4, sph.SCALAR_QUANTIZED, sph.COSINE)])
def test_sweep_spherical(bits, layout, metric):
    dim = 64
    rng = np.random.default_rng(3000 + 10 * bits + layout)
    rows = sph_random_rows(rng, N + 1, dim, bits)
    ssn = float(np.float32(rng.uniform(0.0, 9.0)))
    gix = da.Provider({1: da.SPH1, 4: da.SPH4}[bits], metric, dim, N, 4, rows[N:], sq_shift_norm_sq=ssn)
    gix.set_elements(0, rows[:N])
    gix.set_query_layout(layout)
    q = sph_random_queries(rng, NQ, dim, bits, layout)
    D = sph.distance_matrix(metric, q, rows[:N], dim, bits, layout, ssn)
    sweep(gix, q, D, np.arange(N, dtype=np.uint32), ("SPH", bits, layout, metric))
    gix.close()


@pytest.mark.parametrize("bits,metric", [(2, mm.L2), (8, mm.COSINE_NORMALIZED)])
def test_sweep_minmax(bits, metric):
    dim = 64
    rng = np.random.default_rng(4000 + bits)
    rows = mm_random_rows(rng, N + 1, dim, bits)
    gix = da.Provider(mm_dtype(bits), metric, dim, N, 4, rows[N:])
    gix.set_elements(0, rows[:N])
    q = mm_random_rows(rng, NQ, dim, bits)
    D = mm.distance_matrix(metric, q, rows[:N], dim, bits)
    sweep(gix, q, D, np.arange(N, dtype=np.uint32), ("MM", bits, metric))
    gix.close()


# ---- edges ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def u8_ties():
    """u8 rows drawn from {0, 1} at dim 8: at most 9 distinct L2 distances over 1 500 rows"""
    rng = np.random.default_rng(5)
    data = rng.integers(0, 2, (N + 1, 8), dtype=np.uint8)
    oix = oracle.Index(oracle.U8, oracle.L2, 8, N, 4, data[N:])
    oix.set_rows(0, data[:N])
    gix = da.Provider(da.U8, da.L2, 8, N, 4, data[N:])
    gix.set_elements(0, data[:N])
    q = rng.integers(0, 2, (NQ, 8), dtype=np.uint8)
    yield oix, gix, q
    gix.close()


def test_heavy_ties_across_chunks(u8_ties):
    oix, gix, q = u8_ties
    slots = np.arange(N, dtype=np.uint32)
    D, seen = oracle_distances(oix, q, slots)
    assert all(len(np.unique(r)) <= 9 for r in D)
    sweep(gix, q, D, seen, ("ties",), ks=(10, 64))
    # and by the literal inserts
    gix.debug_set(flat_chunk_rows=64)
    ids, d = gix.flat_search(q[:2], 10)
    for j in range(2):
        pos, md = fm.flat_knn(D[j], 10)
        assert ids[j].tolist() == pos.tolist() and np.array_equal(fbits(d[j]), fbits(md))
    gix.debug_set(flat_chunk_rows=None)


def test_fewer_rows_than_k(u8_ties):
    oix, gix, q = u8_ties
    slots = np.arange(40, 45, dtype=np.uint32)
    D, seen = oracle_distances(oix, q, slots)
    want = expect(D, seen, (10,))
    ids, d = check(gix, q, want, 10, 5, ("n < k",), first=40, n=5)
    assert (ids[:, 5:] == 0xFFFFFFFF).all() and np.isinf(d[:, 5:]).all() and (d[:, 5:] > 0).all()
    assert (want[10][2] == 5).all()


def test_sub_range_with_the_start_point(u8_ties):
    oix, gix, q = u8_ties
    slots = np.arange(N - 200, N + 1, dtype=np.uint32)  # slot N is the start point
    D, seen = oracle_distances(oix, q, slots)
    assert len(seen) == 201
    sweep(gix, q, D, seen, ("sub-range",), ks=(10, 64), chunks=(None, 64), first=N - 200, n=201)


def test_empty_range_and_no_queries(u8_ties):
    _, gix, q = u8_ties
    ids, d, st = gix.flat_search(q, 4, first=3, n=0, stats=True)
    assert (ids == 0xFFFFFFFF).all() and np.isposinf(d).all()
    assert not st["cmps"].any() and not st["written"].any() and not st["result_count"].any()
    ids, d = gix.flat_search(np.zeros((0, 8), np.uint8), 4)
    assert ids.shape == (0, 4) and d.shape == (0, 4)


def test_host_form_across_its_query_piece(u8_ties):
    """the host form stages its queries in pieces of 65 536: 65 536 + 7 queries (16 distinct ones, tiled) over 64 slots
    equal the model on both sides of the boundary, and so do the padded answers of an empty scan"""
    oix, gix, _ = u8_ties
    distinct = np.random.default_rng(6).integers(0, 2, (16, 8), dtype=np.uint8)
    nq, n, k = 65536 + 7, 64, 3
    D, seen = oracle_distances(oix, distinct, np.arange(n, dtype=np.uint32))
    wi, wd, wn = expect(D, seen, (k,))[k]
    q = np.ascontiguousarray(np.tile(distinct, (nq // 16 + 1, 1))[:nq])
    ids, d, st = gix.flat_search(q, k, first=0, n=n, stats=True)
    rep = np.arange(nq) % 16
    assert np.array_equal(ids, wi[rep])
    assert np.array_equal(fbits(d), fbits(wd[rep]))
    assert (st["cmps"] == n).all() and (st["hops"] == 0).all() and (st["status"] == 0).all()
    assert np.array_equal(st["written"], wn[rep]) and np.array_equal(st["result_count"], wn[rep])
    ids, d, st = gix.flat_search(q, k, first=0, n=0, stats=True)
    assert ids.shape == (nq, k) and (ids == 0xFFFFFFFF).all() and np.isposinf(d).all()
    assert not st["cmps"].any() and not st["written"].any() and not st["result_count"].any()


def test_nan_row_is_counted_and_never_returned():
    rng = np.random.default_rng(11)
    n, dim = 300, 24
    data = rand_vectors(rng, oracle.F32, n + 1, dim)
    data[17, 3] = np.nan
    data[170] = np.nan
    oix = oracle.Index(oracle.F32, oracle.L2, dim, n, 4, data[n:])
    oix.set_rows(0, data[:n])
    gix = da.Provider(da.F32, da.L2, dim, n, 4, data[n:])
    gix.set_elements(0, data[:n])
    q = rand_vectors(rng, oracle.F32, 3, dim)
    slots = np.arange(n, dtype=np.uint32)
    D, seen = oracle_distances(oix, q, slots)
    assert np.isnan(D[:, 17]).all() and np.isnan(D[:, 170]).all()
    want = expect(D, seen, (10, 300))
    for chunk in (None, 64):
        gix.debug_set(flat_chunk_rows=chunk)
        check(gix, q, want, 10, n, ("nan", chunk))
        ids, d = check(gix, q, want, 300, n, ("nan all", chunk))  # k = n: the two NaN rows leave two places empty
        assert (want[300][2] == n - 2).all() and not np.isin(ids, (17, 170)).any() and not np.isnan(d).any()
    gix.close()


def test_zero_query_under_inner_product():
    """every distance is a zero: -0.0 and +0.0 tie, so the result is the last k slots in descending order, whatever the
    signs, and the distances keep the sign the distance function gave them"""
    rng = np.random.default_rng(12)
    n, dim = 200, 16
    data = rand_vectors(rng, oracle.F32, n + 1, dim)
    data[::3] = 0.0
    oix = oracle.Index(oracle.F32, oracle.INNER_PRODUCT, dim, n, 4, data[n:])
    oix.set_rows(0, data[:n])
    gix = da.Provider(da.F32, da.INNER_PRODUCT, dim, n, 4, data[n:])
    gix.set_elements(0, data[:n])
    q = np.zeros((2, dim), np.float32)
    q[1] = -0.0
    slots = np.arange(n, dtype=np.uint32)
    D, seen = oracle_distances(oix, q, slots)
    assert (D == 0).all()
    want = expect(D, seen, (10,))
    for chunk in (None, 64):
        gix.debug_set(flat_chunk_rows=chunk)
        ids, _ = check(gix, q, want, 10, n, ("zero", chunk))
        assert ids[0].tolist() == list(range(n - 1, n - 11, -1))
    gix.close()


def test_inline_tags_skip_unpublished_slots():
    rng = np.random.default_rng(13)
    n, dim = 400, 32
    stride = da.lib().dann_inmem2_row_stride(da.F32, dim)
    data = rand_vectors(rng, oracle.F32, n + 1, dim)
    oix = oracle.Index(oracle.F32, oracle.L2, dim, n, 4, data[n:], row_stride=stride, tags=True)
    oix.set_rows(0, data[:n])
    hidden = rng.choice(n, 90, replace=False)
    for h, t in zip(hidden, rng.choice([0, 1, 2, 253], 90)):
        oix.set_tags(int(h), [t])
    gix = da.Provider(da.F32, da.L2, dim, n, 4, data[n:], row_stride=stride, inline_tags=True)
    gix.upload_store(oix.rows)
    q = rand_vectors(rng, oracle.F32, NQ, dim)
    slots = np.arange(n + 1, dtype=np.uint32)  # (the start point, FROZEN, is readable)
    D, seen = oracle_distances(oix, q, slots)
    assert len(seen) == n + 1 - 90 and not np.isin(seen, hidden).any()
    sweep(gix, q, D, seen, ("tags",), ks=(10, 400), chunks=(None, 64), n=n + 1)
    gix.close()


def test_skip_deleted_flag(u8_ties):
    oix, _, q = u8_ties
    rng = np.random.default_rng(14)
    data = oix.rows[:, :8].copy()
    gix = da.Provider(da.U8, da.L2, 8, N, 4, data[N:])
    gix.set_elements(0, data[:N])
    slots = np.arange(N, dtype=np.uint32)
    D, _ = oracle_distances(oix, q, slots)
    everything = expect(D, slots, (10, 64))
    # before any delete there is no deleted state: the flag changes nothing
    check(gix, q, everything, 10, N, ("no bitmap",), skip_deleted=True)
    gone = rng.choice(N, 500, replace=False).astype(np.uint32)
    gix.delete_points(gone)
    keep = np.setdiff1d(slots, gone)
    live = expect(D[:, keep], keep, (10, 64))
    for chunk in (None, 64):
        gix.debug_set(flat_chunk_rows=chunk)
        for k in (10, 64):
            check(gix, q, everything, k, N, ("flag off", chunk, k))
            check(gix, q, live, k, len(keep), ("flag on", chunk, k), skip_deleted=True)
    gix.close()


def test_device_pointer_form_equals_the_host_form(u8_ties):
    _, gix, q = u8_ties
    k = 10
    hi, hd, hs = gix.flat_search(q, k, stats=True)
    dq = DevBuf(q.nbytes, q)
    di, dd, ds = DevBuf(NQ * k * 4), DevBuf(NQ * k * 4), DevBuf(NQ * da.STATS_DTYPE.itemsize)
    gix.flat_search_device(dq.p.value, NQ, k, di.p.value, dd.p.value, d_stats=ds.p.value)
    assert np.array_equal(di.get(np.uint32, (NQ, k)), hi)
    assert np.array_equal(dd.get(np.uint32, (NQ, k)), fbits(hd))
    assert np.array_equal(ds.get(da.STATS_DTYPE, (NQ,)), hs)
    gix.flat_search_device(dq.p.value, NQ, k, di.p.value, dd.p.value)  # the statistics are optional
    assert np.array_equal(di.get(np.uint32, (NQ, k)), hi)


def test_errors(u8_ties):
    _, gix, q = u8_ties
    L, E = da.lib(), da._ffi
    ids, d = np.zeros((NQ, 4), np.uint32), np.zeros((NQ, 4), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(fn=L.dann_flat_search_batch, queries=p(q), nq=NQ, first=0, n=N, k=4, flags=0, oi=p(ids), od=p(d)):
        return fn(gix._h, queries, nq, first, n, k, flags, oi, od, None)

    assert call() == E.OK
    for fn in (L.dann_flat_search_batch, L.dann_flat_search_batch_device):
        assert call(fn, k=0) == E.EINVAL
        assert call(fn, flags=2) == E.EINVAL and call(fn, flags=0x80000001) == E.EINVAL
        assert call(fn, queries=None) == E.EINVAL and call(fn, oi=None) == E.EINVAL and call(fn, od=None) == E.EINVAL
        assert call(fn, n=N + 2) == E.EBOUNDS and call(fn, first=N + 1, n=1) == E.EBOUNDS
        assert call(fn, first=0xFFFFFFFF, n=0xFFFFFFFF) == E.EBOUNDS
        assert call(fn, k=1025) == E.EUNSUPPORTED
        # no queries: nothing is read or written, whatever the pointers
        assert call(fn, queries=None, nq=0, oi=None, od=None) == E.OK
    assert call(n=N + 1) == E.OK and call(first=N + 1, n=0) == E.OK and call(k=1024, oi=None) == E.EINVAL
    assert fn(None, p(q), NQ, 0, N, 4, 0, p(ids), p(d), None) == E.EINVAL


def test_pq_rows_are_refused():
    rng = np.random.default_rng(15)
    dim, chunks, n = 16, 4, 20
    pivots = rng.standard_normal((256, dim)).astype(np.float32)
    offsets = np.arange(0, dim + 1, dim // chunks, dtype=np.uint32)
    codes = rng.integers(0, 256, (n + 1, chunks), dtype=np.uint8)
    gix = da.Provider(da.PQ, da.L2, dim, n, 4, codes[n:], pq_pivots=pivots, pq_offsets=offsets)
    gix.set_elements(0, codes[:n])
    with pytest.raises(da.DannError) as e:
        gix.flat_search(rng.standard_normal((2, dim)).astype(np.float32), 3)
    assert e.value.status == da._ffi.EUNSUPPORTED
    gix.close()
