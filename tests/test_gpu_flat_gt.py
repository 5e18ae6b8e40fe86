"""dann_flat_filtered_search_batch / dann_flat_range_search_batch (and their _device forms) on the GPU against
tests/flat_gt_model.py: ids and distance BITS equal to the model, which is fed the reference distances of the scanned
slots from the sources tests/test_gpu_flat.py uses (the oracle's expand_beam, spherical_model, minmax_model); then against
the graph searches as an independent implementation, and the reference's lattice goldens."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import flat_gt_model as gt
import flat_model as fm
import minmax_model as mm
import oracle
import spherical_model as sph
from filtered_cases import build
from helpers import bits as fbits, make_pair, rand_vectors, random_graph
from minmax_builders import mm_dtype, random_rows as mm_random_rows
from search_builders import SqBitsCase
from test_gpu_spherical import DevBuf, _random_queries as sph_random_queries, _random_rows as sph_random_rows

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

N = 1500                 # two default chunks (1024 + 476); 24 chunks of 64; 15 chunks of 100
NQ = 8 + 3               # one full query tile and a partial one
KS = (1, 10, 65, 1024)
CHUNKS = (None, 64, 100)
NSLOTS = N + 1           # the rows and one start point: what a bitmap covers
EMPTY = 0xFFFFFFFF
SINGLE_BITS = (0, 31, 32, 63, 64, 99, 100, 1023, 1024, 1499)


def oracle_distances(oix, queries, slots):
    out, seen = [], None
    for q in queries:
        ids, d = oix.expand_beam(q, slots)
        assert seen is None or np.array_equal(ids, seen)
        seen = ids
        out.append(d)
    return np.stack(out), seen


def per_query(match, nq):
    m = np.asarray(match, bool)
    return np.broadcast_to(m, (nq, m.shape[-1])) if m.ndim == 1 else m


def filters(seed, nslots=NSLOTS, nq=NQ):
    """{name: bool array over the slots, shared (1-D) or per query (2-D)}"""
    rng = np.random.default_rng(seed)
    mixed = rng.random((nq, nslots)) < 0.3  # per-query bitmaps that differ inside a tile
    mixed[0] = False
    mixed[1] = True
    mixed[2] = rng.random(nslots) < 0.01
    return {"empty": np.zeros(nslots, bool), "1%": rng.random(nslots) < 0.01, "50%": rng.random(nslots) < 0.5,
            "ones": np.ones(nslots, bool), "per query": mixed}


def expect_knn(D, seen, match, ks):
    """{k: (ids[nq, k], dists[nq, k], written[nq])} and cmps[nq]: the closed form over every query's matching subsequence"""
    m = per_query(match, len(D))[:, seen]
    res = {k: ([], [], []) for k in ks}
    for row, keep in zip(D, m):
        at = np.flatnonzero(keep)
        pos, d = fm.flat_knn_closed(row[at], len(at))
        pos = at[pos]
        for k in ks:
            i, dd = fm.padded(pos[:k], d[:k], k, seen)
            res[k][0].append(i)
            res[k][1].append(dd)
            res[k][2].append(min(k, len(pos)))
    return {k: (np.stack(v[0]), np.stack(v[1]), np.array(v[2])) for k, v in res.items()}, m.sum(1)


def check_knn(gix, q, want, cmps, k, tag, **kw):
    ids, d, st = gix.flat_search(q, k, stats=True, **kw)
    wi, wd, wn = want[k]
    assert np.array_equal(ids, wi), tag + ("ids",)
    assert np.array_equal(fbits(d), fbits(wd)), tag + ("distance bits",)
    assert np.array_equal(st["cmps"], cmps) and not st["hops"].any() and not st["status"].any(), tag + ("stats",)
    assert np.array_equal(st["written"], wn) and np.array_equal(st["result_count"], wn), tag + ("written",)
    return ids, d, st


def sweep_knn(gix, q, D, seen, match, tag, ks=KS, chunks=CHUNKS, **kw):
    want, cmps = expect_knn(D, seen, match, ks)
    for rows in chunks:
        gix.debug_set(flat_chunk_rows=rows)
        for k in ks:
            check_knn(gix, q, want, cmps, k, tag + (rows, k), match=match, **kw)
    gix.debug_set(flat_chunk_rows=None)


def expect_range(D, seen, match, radius, inner=None):
    """[(slots, dists)] per query and cmps[nq], by the literal predicate"""
    m = np.ones((len(D), len(seen)), bool) if match is None else per_query(match, len(D))[:, seen]
    out = []
    for row, keep in zip(D, m):
        pos, d = gt.range_scan(row, keep, radius, inner)
        out.append((np.asarray(seen)[pos].astype(np.uint32), d))
    return out, m.sum(1)


def check_range(gix, q, D, seen, match, radius, inner, tag, out_cap=None, chunks=CHUNKS, **kw):
    want, cmps = expect_range(D, seen, match, radius, inner)
    counts = np.array([len(w[0]) for w in want], np.uint32)
    for rows in chunks:
        gix.debug_set(flat_chunk_rows=rows)
        ids, d, cnt, st = gix.flat_range_search(q, radius, inner_radius=inner, match=match, out_cap=out_cap, stats=True, **kw)
        assert np.array_equal(cnt, counts), tag + (rows, "counts")
        assert np.array_equal(st["cmps"], cmps) and not st["hops"].any() and not st["status"].any(), tag + (rows, "stats")
        assert np.array_equal(st["result_count"], counts) and np.array_equal(st["written"], counts), tag + (rows,)
        for j, (wi, wd) in enumerate(want):
            assert np.array_equal(ids[j, :len(wi)], wi), tag + (rows, j, "ids")
            assert np.array_equal(fbits(d[j, :len(wi)]), fbits(wd)), tag + (rows, j, "distance bits")
            assert (ids[j, len(wi):] == EMPTY).all() and np.isposinf(d[j, len(wi):]).all(), tag + (rows, j, "padding")
    gix.debug_set(flat_chunk_rows=None)
    return want, counts


# ---- one case per row type ---------------------------------------------------------------------------------------------
def _full(dt, metric, dim, seed):
    rng = np.random.default_rng(seed)
    data = rand_vectors(rng, dt, N + 1, dim)
    oix = oracle.Index(dt, metric, dim, N, 4, data[N:])
    oix.set_rows(0, data[:N])
    gix = da.Provider(dt, metric, dim, N, 4, data[N:])
    gix.set_elements(0, data[:N])
    q = rand_vectors(rng, dt, NQ, dim)
    D, seen = oracle_distances(oix, q, np.arange(N, dtype=np.uint32))
    return gix, q, D, seen


def _u8_ties():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 2, (N + 1, 8), dtype=np.uint8)
    oix = oracle.Index(oracle.U8, oracle.L2, 8, N, 4, data[N:])
    oix.set_rows(0, data[:N])
    gix = da.Provider(da.U8, da.L2, 8, N, 4, data[N:])
    gix.set_elements(0, data[:N])
    q = rng.integers(0, 2, (NQ, 8), dtype=np.uint8)
    D, seen = oracle_distances(oix, q, np.arange(N, dtype=np.uint32))
    return gix, q, D, seen, oix


def _sq4():
    c = SqBitsCase(4, oracle.L2, N, 64, 4, 2104, adj=False)
    _, q, q_twin = c.queries(NQ)
    D, seen = oracle_distances(c.oix, q_twin, np.arange(N, dtype=np.uint32))
    return c.gix, q, D, seen


def _sph1():
    dim, bits, layout = 64, 1, sph.FOUR_BIT_TRANSPOSED
    rng = np.random.default_rng(3011)
    rows = sph_random_rows(rng, N + 1, dim, bits)
    ssn = float(np.float32(rng.uniform(0.0, 9.0)))
    gix = da.Provider(da.SPH1, sph.IP, dim, N, 4, rows[N:], sq_shift_norm_sq=ssn)
    gix.set_elements(0, rows[:N])
    gix.set_query_layout(layout)
    q = sph_random_queries(rng, NQ, dim, bits, layout)
    return gix, q, sph.distance_matrix(sph.IP, q, rows[:N], dim, bits, layout, ssn), np.arange(N, dtype=np.uint32)


def _mm2():
    dim, bits = 64, 2
    rng = np.random.default_rng(4002)
    rows = mm_random_rows(rng, N + 1, dim, bits)
    gix = da.Provider(mm_dtype(bits), mm.L2, dim, N, 4, rows[N:])
    gix.set_elements(0, rows[:N])
    q = mm_random_rows(rng, NQ, dim, bits)
    return gix, q, mm.distance_matrix(mm.L2, q, rows[:N], dim, bits), np.arange(N, dtype=np.uint32)


ROW_TYPES = {"f32 L2 128": lambda: _full(oracle.F32, oracle.L2, 128, 101), "f32 cosine 100": lambda: _full(oracle.F32, oracle.COSINE, 100, 102),
             "f16 IP 128": lambda: _full(oracle.F16, oracle.INNER_PRODUCT, 128, 103), "u8 L2 ties": lambda: _u8_ties()[:4],
             "SQ4 L2 64": _sq4, "SPH1 4-bit transposed": _sph1, "MM2 L2": _mm2}


@pytest.mark.parametrize("name", list(ROW_TYPES))
def test_filtered_knn_by_row_type(name):
    gix, q, D, seen = ROW_TYPES[name]()
    for fname, match in filters(7).items():
        sweep_knn(gix, q, D, seen, match, (name, fname))
    # all ones: flat_search itself, in every output
    for k in (10, 1024):
        a = gix.flat_search(q, k, stats=True)
        b = gix.flat_search(q, k, stats=True, match=np.ones(NSLOTS, bool))
        assert np.array_equal(a[0], b[0]) and np.array_equal(fbits(a[1]), fbits(b[1])) and np.array_equal(a[2], b[2])
    gix.close()


@pytest.mark.parametrize("name", list(ROW_TYPES))
def test_range_by_row_type(name):
    gix, q, D, seen = ROW_TYPES[name]()
    flat = np.sort(D[~np.isnan(D)])
    lo, mid, hi = float(flat[0]), float(flat[len(flat) // 20]), float(flat[-1])
    f = filters(8)
    want, counts = check_range(gix, q, D, seen, None, np.nextafter(np.float32(lo), np.float32(-np.inf)), None, (name, "below"))
    assert not counts.any()
    check_range(gix, q, D, seen, None, mid, None, (name, "mid"))
    want, counts = check_range(gix, q, D, seen, None, hi, None, (name, "max"), out_cap=N)
    assert (counts == N).all()
    check_range(gix, q, D, seen, None, hi, mid, (name, "inner"))
    for fname in ("empty", "1%", "50%", "per query"):
        check_range(gix, q, D, seen, f[fname], float(flat[len(flat) // 3]), None, (name, fname), chunks=(None, 100))
    gix.close()


# ---- filters at the edges (the tie-heavy u8 rows) -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def u8():
    gix, q, D, seen, oix = _u8_ties()
    yield gix, q, D, seen, oix
    gix.close()


def test_single_bits(u8):
    gix, q, D, seen, _ = u8
    for s in SINGLE_BITS:
        match = np.zeros(NSLOTS, bool)
        match[s] = True
        sweep_knn(gix, q, D, seen, match, ("bit", s))
        want, counts = check_range(gix, q, D, seen, match, 8.0, None, ("bit range", s))
        assert (counts == 1).all() and all(w[0].tolist() == [s] for w in want)


def test_k_above_the_number_of_matches(u8):
    gix, q, D, seen, _ = u8
    match = np.zeros(NSLOTS, bool)
    match[[3, 64, 700, 1499]] = True
    want, cmps = expect_knn(D, seen, match, (10,))
    ids, d, st = check_knn(gix, q, want, cmps, 10, ("few",), match=match)
    assert (st["written"] == 4).all() and (ids[:, 4:] == EMPTY).all() and np.isposinf(d[:, 4:]).all()


def test_bits_beyond_the_last_slot_are_ignored(u8):
    gix, q, D, seen, _ = u8
    words = (NSLOTS + 31) // 32
    raw = np.zeros((NQ, words + 2), np.uint32)  # a stride longer than a bitmap, garbage behind the last slot
    raw[:, words - 1] = 0xFFFFFFFF << (NSLOTS % 32) & 0xFFFFFFFF
    raw[:, words:] = 0xFFFFFFFF
    raw[:, 0] = 0b101
    f = da._ffi.FlatFilter(raw.ctypes.data, words + 2)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for k in KS:
        ids, d, st = np.zeros((NQ, k), np.uint32), np.zeros((NQ, k), np.float32), np.zeros(NQ, da.STATS_DTYPE)
        rc = da.lib().dann_flat_filtered_search_batch(gix._h, p(q), NQ, 0, N + 1, k, 0, C.byref(f), p(ids), p(d), p(st))
        assert rc == 0
        m = min(k, 2)
        assert (st["cmps"] == 2).all() and (st["written"] == m).all(), k
        assert all(set(r[:m].tolist()) <= {0, 2} and len(set(r[:m].tolist())) == m for r in ids) and (ids[:, m:] == EMPTY).all(), k
    cnt = np.zeros(NQ, np.uint32)
    rc = da.lib().dann_flat_range_search_batch(gix._h, p(q), NQ, 0, N + 1, 8.0, 0, 0.0, 0, C.byref(f), 0, None, None, p(cnt), None)
    assert rc == 0 and (cnt == 2).all()


def test_only_deleted_or_unreadable_slots_match(u8):
    _, q, D, seen, oix = u8
    data = oix.rows[:, :8].copy()
    gix = da.Provider(da.U8, da.L2, 8, N, 4, data[N:])
    gix.set_elements(0, data[:N])
    gone = np.array([5, 64, 65, 1030], np.uint32)
    gix.delete_points(gone)
    match = np.zeros(NSLOTS, bool)
    match[gone] = True
    for k in KS:
        ids, d, st = gix.flat_search(q, k, stats=True, match=match, skip_deleted=True)
        assert (ids == EMPTY).all() and np.isposinf(d).all() and not st["cmps"].any() and not st["written"].any(), k
    _, _, cnt, st = gix.flat_range_search(q, 8.0, match=match, skip_deleted=True, stats=True)
    assert not cnt.any() and not st["cmps"].any()
    # without the flag the deleted state is not consulted; with it and a wider filter only the live rows count
    sweep_knn(gix, q, D, seen, match, ("flag off",))
    wide = match.copy()
    wide[100:140] = True
    live = wide.copy()
    live[gone] = False
    want, cmps = expect_knn(D, seen, live, KS)
    for chunk in CHUNKS:
        gix.debug_set(flat_chunk_rows=chunk)
        for k in KS:
            check_knn(gix, q, want, cmps, k, ("live", chunk, k), match=wide, skip_deleted=True)
    gix.close()
    # inline tags: a filter that holds only unpublished slots
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
    qf = rand_vectors(rng, oracle.F32, NQ, dim)
    Dt, seen_t = oracle_distances(oix, qf, np.arange(n + 1, dtype=np.uint32))
    match = np.zeros(n + 1, bool)
    match[hidden] = True
    for k in KS:
        ids, _, st = gix.flat_search(qf, k, n=n + 1, stats=True, match=match)
        assert (ids == EMPTY).all() and not st["cmps"].any() and not st["written"].any(), k
    half = np.random.default_rng(14).random((NQ, n + 1)) < 0.5
    sweep_knn(gix, qf, Dt, seen_t, half, ("tags",), n=n + 1)
    check_range(gix, qf, Dt, seen_t, half, float(np.median(Dt)), None, ("tags range",), chunks=(None, 64), n=n + 1)
    gix.close()


# ---- range edges ---------------------------------------------------------------------------------------------------------
def test_range_radius_on_a_shared_value(u8):
    """u8 {0, 1} rows at dim 8: at most 9 distinct distances, so a radius equal to one of them sits on hundreds of rows --
    the radius is inclusive, the inner radius exclusive"""
    gix, q, D, seen, _ = u8
    for radius, inner in ((3.0, None), (4.0, 2.0), (4.0, 4.0), (0.0, None)):
        want, counts = check_range(gix, q, D, seen, None, radius, inner, ("shared", radius, inner))
        assert np.array_equal(counts, ((D <= radius) & ~(D <= (inner if inner is not None else -1.0))).sum(1))
    assert ((D == 3.0).sum(1) > 100).all()


def test_range_count_only_and_overflow(u8):
    gix, q, D, seen, _ = u8
    want, cmps = expect_range(D, seen, None, 3.0)
    counts = np.array([len(w[0]) for w in want], np.uint32)
    ids, d, cnt = gix.flat_range_search(q, 3.0, out_cap=0)
    assert ids.shape == (NQ, 0) and np.array_equal(cnt, counts)
    cap = int(counts.max()) - 1
    assert (counts <= cap).any() and (counts > cap).any()
    for chunk in CHUNKS:
        gix.debug_set(flat_chunk_rows=chunk)
        with pytest.raises(da.DannError) as e:
            gix.flat_range_search(q, 3.0, out_cap=cap, stats=True)
        assert e.value.status == da._ffi.EOVERFLOW
        ids, d, cnt, st = e.value.partial
        assert np.array_equal(cnt, counts) and np.array_equal(st["result_count"], counts)
        assert np.array_equal(st["status"] != 0, counts > cap) and np.array_equal(st["written"], np.minimum(counts, cap))
        for j, (wi, wd) in enumerate(want):
            m = min(len(wi), cap)
            assert np.array_equal(ids[j, :m], wi[:m]) and np.array_equal(fbits(d[j, :m]), fbits(wd[:m])), (chunk, j)
            assert (ids[j, m:] == EMPTY).all() and np.isposinf(d[j, m:]).all()
    gix.debug_set(flat_chunk_rows=None)
    ids, d, cnt = gix.flat_range_search(q, 3.0, out_cap=int(counts.max()))  # the retry holds everything
    assert np.array_equal(cnt, counts)


def test_range_with_nan_rows_and_signed_zeros():
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
    D, seen = oracle_distances(oix, q, np.arange(n, dtype=np.uint32))
    assert np.isnan(D[:, 17]).all()
    want, counts = check_range(gix, q, D, seen, None, float(np.nanmax(D)), None, ("nan",), chunks=(None, 64))
    assert (counts == n - 2).all()
    gix.close()
    # inner product with a zero query: every distance is a zero of either sign, kept as computed
    data = rand_vectors(rng, oracle.F32, n + 1, 16)
    data[::3] = 0.0
    oix = oracle.Index(oracle.F32, oracle.INNER_PRODUCT, 16, n, 4, data[n:])
    oix.set_rows(0, data[:n])
    gix = da.Provider(da.F32, da.INNER_PRODUCT, 16, n, 4, data[n:])
    gix.set_elements(0, data[:n])
    q = np.zeros((2, 16), np.float32)
    q[1] = -0.0
    D, seen = oracle_distances(oix, q, np.arange(n, dtype=np.uint32))
    want, counts = check_range(gix, q, D, seen, None, 0.0, None, ("zeros",), chunks=(None, 64))
    assert (counts == n).all()
    gix.close()


# ---- forms and ranges ----------------------------------------------------------------------------------------------------
def test_device_forms_equal_the_host_forms(u8):
    gix, q, D, seen, _ = u8
    k = 10
    for match in (filters(9)["50%"], filters(9)["per query"]):
        _, bits = gix._flat_filter(match, NQ)
        stride = 0 if bits.shape[0] == 1 else bits.shape[1]
        dq, db = DevBuf(q.nbytes, q), DevBuf(bits.nbytes, bits)
        hi, hd, hs = gix.flat_search(q, k, stats=True, match=match)
        di, dd, ds = DevBuf(NQ * k * 4), DevBuf(NQ * k * 4), DevBuf(NQ * da.STATS_DTYPE.itemsize)
        gix.flat_search_device(dq.p.value, NQ, k, di.p.value, dd.p.value, d_stats=ds.p.value, d_bits=db.p.value, stride_words=stride)
        assert np.array_equal(di.get(np.uint32, (NQ, k)), hi) and np.array_equal(dd.get(np.uint32, (NQ, k)), fbits(hd))
        assert np.array_equal(ds.get(da.STATS_DTYPE, (NQ,)), hs)
        cap = 700
        ri, rd, rc, rs = gix.flat_range_search(q, 3.0, inner_radius=1.0, match=match, out_cap=cap, stats=True)
        di, dd, dc = DevBuf(NQ * cap * 4), DevBuf(NQ * cap * 4), DevBuf(NQ * 4)
        gix.flat_range_search_device(dq.p.value, NQ, 3.0, cap, di.p.value, dd.p.value, dc.p.value, inner_radius=1.0,
                                     d_stats=ds.p.value, d_bits=db.p.value, stride_words=stride)
        assert np.array_equal(di.get(np.uint32, (NQ, cap)), ri) and np.array_equal(dd.get(np.uint32, (NQ, cap)), fbits(rd))
        assert np.array_equal(dc.get(np.uint32, (NQ,)), rc) and np.array_equal(ds.get(da.STATS_DTYPE, (NQ,)), rs)
        gix.flat_range_search_device(dq.p.value, NQ, 3.0, 0, 0, 0, dc.p.value, inner_radius=1.0)  # count only, no filter
        assert np.array_equal(dc.get(np.uint32, (NQ,)), ((D <= 3.0) & ~(D <= 1.0)).sum(1))


def test_host_forms_across_their_query_piece(u8):
    """the host forms stage queries and per-query bitmaps in pieces of 65 536: 65 536 + 7 queries (16 distinct queries and
    bitmaps, tiled) over 64 slots equal the model on both sides of the boundary"""
    gix, _, _, _, oix = u8
    rng = np.random.default_rng(6)
    distinct = rng.integers(0, 2, (16, 8), dtype=np.uint8)
    masks = rng.random((16, NSLOTS)) < 0.4
    nq, n, k = 65536 + 7, 64, 3
    D, seen = oracle_distances(oix, distinct, np.arange(n, dtype=np.uint32))
    want, cmps = expect_knn(D, seen, masks, (k,))
    wi, wd, wn = want[k]
    rep = np.arange(nq) % 16
    q = np.ascontiguousarray(distinct[rep])
    match = masks[rep]
    ids, d, st = gix.flat_search(q, k, first=0, n=n, stats=True, match=match)
    assert np.array_equal(ids, wi[rep]) and np.array_equal(fbits(d), fbits(wd[rep]))
    assert np.array_equal(st["cmps"], cmps[rep]) and np.array_equal(st["written"], wn[rep]) and not st["status"].any()
    rwant, rcmps = expect_range(D, seen, masks, 3.0, 1.0)
    cap = max(len(w[0]) for w in rwant)
    ri, rd, rc, rs = gix.flat_range_search(q, 3.0, inner_radius=1.0, match=match, first=0, n=n, out_cap=cap, stats=True)
    assert np.array_equal(rc, np.array([len(w[0]) for w in rwant], np.uint32)[rep]) and np.array_equal(rs["cmps"], rcmps[rep])
    for j in list(range(16)) + list(range(65536 - 8, nq)):
        wi_j, wd_j = rwant[j % 16]
        assert np.array_equal(ri[j, :len(wi_j)], wi_j) and np.array_equal(fbits(rd[j, :len(wi_j)]), fbits(wd_j)), j
        assert (ri[j, len(wi_j):] == EMPTY).all(), j


def test_sub_ranges_with_and_without_the_start_point(u8):
    gix, q, _, _, oix = u8
    match = filters(10)["per query"]
    for first, n in ((N - 200, 201), (N - 200, 200), (37, 130)):
        D, seen = oracle_distances(oix, q, np.arange(first, first + n, dtype=np.uint32))
        assert len(seen) == n
        sweep_knn(gix, q, D, seen, match, ("sub", first, n), ks=(10, 65), chunks=(None, 64), first=first, n=n)
        check_range(gix, q, D, seen, match, 3.0, 1.0, ("sub range", first, n), chunks=(None, 64), first=first, n=n)
    ids, d, cnt = gix.flat_range_search(q, 3.0, first=3, n=0)
    assert ids.shape == (NQ, 0) and not cnt.any()
    ids, d = gix.flat_search(q, 4, first=3, n=0, match=np.ones(NSLOTS, bool))
    assert (ids == EMPTY).all() and np.isposinf(d).all()


def test_errors(u8):
    gix, q, _, _, _ = u8
    L, E = da.lib(), da._ffi
    words = (NSLOTS + 31) // 32
    bits = np.full(words * NQ, 0xFFFFFFFF, np.uint32)
    ids, d, cnt = np.zeros((NQ, 4), np.uint32), np.zeros((NQ, 4), np.float32), np.zeros(NQ, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    flt = lambda stride=0: C.byref(E.FlatFilter(bits.ctypes.data, stride))  # noqa: E731

    def knn(fn, queries=p(q), nq=NQ, first=0, n=N, k=4, flags=0, f=None, oi=p(ids), od=p(d)):
        return fn(gix._h, queries, nq, first, n, k, flags, f if f is not None else flt(), oi, od, None)

    def rng_(fn, queries=p(q), nq=NQ, first=0, n=N, radius=3.0, has_inner=0, inner=0.0, flags=0, f=None, cap=4, oi=p(ids),
             od=p(d), oc=p(cnt)):
        return fn(gix._h, queries, nq, first, n, radius, has_inner, inner, flags, f, cap, oi, od, oc, None)

    assert knn(L.dann_flat_filtered_search_batch) == E.OK and knn(L.dann_flat_filtered_search_batch, f=flt(words)) == E.OK
    for fn in (L.dann_flat_filtered_search_batch, L.dann_flat_filtered_search_batch_device):
        assert knn(fn, k=0) == E.EINVAL and knn(fn, flags=2) == E.EINVAL
        assert knn(fn, queries=None) == E.EINVAL and knn(fn, oi=None) == E.EINVAL and knn(fn, od=None) == E.EINVAL
        assert knn(fn, f=flt(words - 1)) == E.EINVAL and knn(fn, f=flt(1)) == E.EINVAL
        assert knn(fn, n=N + 2) == E.EBOUNDS and knn(fn, first=N + 1, n=1) == E.EBOUNDS
        assert knn(fn, k=1025) == E.EUNSUPPORTED
        assert knn(fn, queries=None, nq=0, oi=None, od=None) == E.OK
        assert fn(None, p(q), NQ, 0, N, 4, 0, flt(), p(ids), p(d), None) == E.EINVAL
    for fn in (L.dann_flat_range_search_batch, L.dann_flat_range_search_batch_device):
        assert rng_(fn, radius=float("nan")) == E.EINVAL
        assert rng_(fn, has_inner=1, inner=3.5) == E.EINVAL and rng_(fn, has_inner=1, inner=float("nan")) == E.EINVAL
        assert rng_(fn, flags=2) == E.EINVAL
        assert rng_(fn, queries=None) == E.EINVAL and rng_(fn, oc=None) == E.EINVAL
        assert rng_(fn, oi=None) == E.EINVAL and rng_(fn, od=None) == E.EINVAL
        assert rng_(fn, f=flt(words - 1)) == E.EINVAL
        assert rng_(fn, n=N + 2) == E.EBOUNDS and rng_(fn, first=0xFFFFFFFF, n=0xFFFFFFFF) == E.EBOUNDS
        assert rng_(fn, queries=None, nq=0, oi=None, od=None, oc=None) == E.OK
        assert fn(None, p(q), NQ, 0, N, 3.0, 0, 0.0, 0, None, 4, p(ids), p(d), p(cnt), None) == E.EINVAL
    assert rng_(L.dann_flat_range_search_batch, radius=-1.0) == E.OK and not cnt.any()
    assert rng_(L.dann_flat_range_search_batch, radius=0.0, has_inner=0, inner=9.0, cap=0) == E.OK  # an inner radius not given
    assert rng_(L.dann_flat_range_search_batch) == E.EOVERFLOW and (cnt > 4).all()  # (4 places: the counts are the true ones)
    assert rng_(L.dann_flat_range_search_batch, cap=0, oi=None, od=None) == E.OK


def test_pq_rows_are_refused():
    rng = np.random.default_rng(15)
    dim, chunks, n = 16, 4, 20
    pivots = rng.standard_normal((256, dim)).astype(np.float32)
    offsets = np.arange(0, dim + 1, dim // chunks, dtype=np.uint32)
    codes = rng.integers(0, 256, (n + 1, chunks), dtype=np.uint8)
    gix = da.Provider(da.PQ, da.L2, dim, n, 4, codes[n:], pq_pivots=pivots, pq_offsets=offsets)
    gix.set_elements(0, codes[:n])
    qf = rng.standard_normal((2, dim)).astype(np.float32)
    for call in (lambda: gix.flat_search(qf, 3, match=np.ones(n + 1, bool)), lambda: gix.flat_range_search(qf, 1.0)):
        with pytest.raises(da.DannError) as e:
            call()
        assert e.value.status == da._ffi.EUNSUPPORTED
    gix.close()


# ---- against the graph searches, as an independent implementation -----------------------------------------------------------
def test_graph_searches_never_beat_the_exhaustive_scan():
    rng = np.random.default_rng(31)
    n, dim, R, nq = N, 32, 16, NQ
    data = rng.standard_normal((n, dim)).astype(np.float32)
    adj = random_graph(rng, n, R)
    _, gix = make_pair(oracle.F32, oracle.L2, data, adj, data[:1].copy(), R)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    match = rng.random((nq, n + 1)) < 0.3
    match[:, n] = False
    k = 10
    fi, fd = gix.flat_search(q, k, match=match)
    assert all(match[j, fi[j]].all() for j in range(nq))
    for mode in (da.FILTER_INLINE, da.FILTER_MULTIHOP):
        ids, dists, st = gix.filtered_search(da.Knn(40), q, k, match, mode=mode)
        for j in range(nq):
            m = int(st["written"][j])
            assert match[j, ids[j, :m]].all(), (mode, j)
            assert (np.sort(dists[j, :m]) >= fd[j, :m]).all(), (mode, j)
    radius = float(np.sort(fd[:, -1])[nq // 2]) * 1.1
    ri, rd, rc = gix.flat_range_search(q, radius)
    gi, gd, gst, _ = gix.range_search(q, 40, radius, out_cap=n)
    mi, md, mc = gix.flat_range_search(q, radius, match=match)
    hi, hd, hst, _ = gix.filtered_range_search(q, 40, radius, match, out_cap=n)
    assert rc.any() and mc.any()
    for (ei, ed, ec), (si, sd, found) in (((ri, rd, rc), (gi, gd, gst["result_count"])), ((mi, md, mc), (hi, hd, hst["written"]))):
        for j in range(nq):
            exact = dict(zip(ei[j, :ec[j]].tolist(), fbits(ed[j, :ec[j]]).tolist()))
            m = int(found[j])
            assert all(exact.get(int(i)) == int(b) for i, b in zip(si[j, :m], fbits(sd[j, :m]))), j
    gix.close()


def _lattice(g):
    dim = g.data.shape[1]
    px = da.Provider(da.F32, da.L2, dim, g.n, g.max_degree, g.start_vec.reshape(1, -1))
    g.fill(px)
    return px


def test_lattice_goldens_on_the_gpu(golden_dir):
    filtered = json.load(open(os.path.join(golden_dir, "filtered_search.json")))
    plain = json.load(open(os.path.join(golden_dir, "range_search.json")))
    # (case, filter, whether the graph search finds everything the scan finds)
    ranges = [(c, "all", c["name"] in ("basic_range_search", "inner_radius_filtering", "two_round_search")) for c in plain]
    ranges += [(c, c["filter"], c["name"] != "max_results_respected_means_no_second_round") for c in filtered["filtered_range"]]
    for c, rule, everything in ranges:
        g = build("grid", c["grid_dims"], c["grid_size"])
        px = _lattice(g)
        match = g.match(rule).copy()
        match[g.n:] = False
        ids, d, cnt = px.flat_range_search(np.array(c["query"], np.float32), c["radius"], inner_radius=c["inner_radius"], match=match)
        exact = dict(zip(ids[0, :cnt[0]].tolist(), fbits(d[0, :cnt[0]]).tolist()))
        got = {int(r[0]): int(fbits(np.float32(r[1])).ravel()[0]) for r in c["results"]}
        assert got.items() <= exact.items(), c["name"]
        assert not everything or got == exact, c["name"]
        px.close()
    inline_equal = {"inline_adaptive_l_logarithmic", "inline_adaptive_l_max", "inline_adaptive_l_no_scaling",
                    "inline_fixed_no_scaling", "inline_search_reaches_matches_through_non_matching_nodes",
                    "inline_search_returns_only_final_level_matches", "inline_search_three_level_adaptive_l_with_l1_finds_matches"}
    assert len(filtered["inline"]) == 12 and len(filtered["multihop"]) == 2
    equal = set()
    for c in filtered["inline"] + filtered["multihop"]:
        g = build(c["graph"], grid_size=c.get("grid_size"))
        px = _lattice(g)
        match = g.match(c["filter"]).copy()
        match[g.n:] = False
        ids, d, st = px.flat_search(np.array(c["query"], np.float32), c["k"], stats=True, match=match)
        m = int(st["written"][0])
        # what the GPU returned: only matching slots, as many as match (up to k), distances ascending
        assert match[ids[0, :m]].all() and m == min(c["k"], int(match.sum())), c["name"]
        assert int(st["cmps"][0]) == int(match.sum()) and (np.diff(d[0, :m]) >= 0).all(), c["name"]
        res = c["results"] if "results" in c else list(zip(c["result_ids"], c["result_distances"]))
        got = np.sort(np.array([r[1] for r in res], np.float32))
        # the golden's ids match the filter and its sorted distances are, rank by rank, >= the exhaustive ones
        slot_of = {int(o): s for s, o in enumerate(g.orig)}
        assert all(match[slot_of[int(r[0])]] for r in res), c["name"]
        assert len(got) <= m and (got >= d[0, :len(got)]).all(), c["name"]
        if len(got) == m and np.array_equal(fbits(got), fbits(d[0, :m])):
            equal.add(c["name"])
        else:
            assert len(got) < m, c["name"]  # not equal: the graph search returned fewer than the exhaustive count
        px.close()
    # the distance multisets are equal in both multihop cases and in these seven inline cases; the other five are fewer
    assert equal == inline_equal | {c["name"] for c in filtered["multihop"]}
