"""SQ4 / SQ1 rows on the GPU: compression and distances against the CPU model (tests/sq_bits_model.py), every search
kind, the build and the graph mutations against the oracle's SQ-8 twin (same integer sums, matched scale: identical
distance bits) or the Python models running over it."""
import ctypes as C

import numpy as np
import pytest

import oracle
import sq_bits_model as m
from consolidate_model import consolidate
from diverse_model import diverse_search
from helpers import bits as fbits, small_calls_from_threads
from inplace_delete_model import TIE_RUST, inplace_delete
from search_builders import SqBitsCase as Case, sq_setup as _setup

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

DT = {1: da.SQ1, 4: da.SQ4, 8: da.SQ8}
METRICS = (oracle.L2, oracle.INNER_PRODUCT, oracle.COSINE_NORMALIZED)
# lengths at the seams of the gather: a lane reads 16 bytes (SQ4) / 4 bytes (SQ1) per step, 32 dimensions either way, a
# 4-lane group 128 dimensions; a dword holds 8 (SQ4) / 32 (SQ1) codes, a byte 2 / 8
DIMS = {4: (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257),
        1: (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)}


# ---- compression --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 4, 8])
def test_compress_matches_model(bits):
    rng = np.random.default_rng(10 + bits)
    for dim in (1, 7, 8, 9, 63, 64, 65, 100, 257):
        data, shift, scale, _ = _setup(rng, 300, dim)
        data[3, 0], data[4, dim // 2], data[5, dim - 1] = 1e9, -1e9, np.nan
        got = da.sq_compress(data, shift, scale, bits)
        want = m.compress(data, shift, scale, bits)
        assert got.shape == (300, m.layer_bytes(bits, dim))
        assert np.array_equal(got, want), (bits, dim, np.flatnonzero((got != want).any(axis=1))[:5])
        if bits == 8:
            assert np.array_equal(got, da.sq8_compress(data, shift, scale))
        else:  # padding bits of the last code byte are zero
            used = dim * bits - 8 * (m.code_bytes(bits, dim) - 1)
            assert not (got[:, m.code_bytes(bits, dim) - 1] >> used).any()


# ---- distances ----------------------------------------------------------------------------------------------------------
def _random_rows(rng, n, dim, bits, garbage):
    rows = np.zeros((n, m.layer_bytes(bits, dim)), np.uint8)
    cb = m.code_bytes(bits, dim)
    rows[:, :cb] = m.pack(rng.integers(0, 1 << bits, (n, dim), dtype=np.uint8), bits)
    rows[:, cb:] = rng.normal(0.0, 3.0, n).astype(np.float32).view(np.uint8).reshape(n, 4)
    if garbage:
        used = dim * bits - 8 * (cb - 1)
        if used < 8:
            rows[:, cb - 1] |= (rng.integers(0, 256, n, dtype=np.uint8) << used).astype(np.uint8)
    return rows


def _overwrite_store(gix, raw):
    """the whole row buffer of `gix` replaced by `raw` (nslots x row_stride bytes): the one way to put bytes between a
    row's payload and its stride, which no entry point of the library writes"""
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    rows_ptr, _ = gix.device_pointers()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    assert raw.shape[0] == gix.capacity + gix.num_start_points
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(C.c_void_p(rows_ptr), raw.ctypes.data_as(C.c_void_p), raw.nbytes, 1) == 0  # host to device
    assert hip.hipDeviceSynchronize() == 0


@pytest.mark.parametrize("variant", ["packed", "padded", "inline_tags", "garbage"])
@pytest.mark.parametrize("bits", [1, 4])
def test_distances_match_model(bits, variant):
    """distance_pairs and expand_beam, bit for bit; the scale is arbitrary (the library's own evaluation of k)"""
    rng = np.random.default_rng(20 + bits + len(variant))
    n, nids = 48, 40
    for dim in DIMS[bits]:
        rows = _random_rows(rng, n + 1, dim, bits, variant == "garbage")
        query = _random_rows(rng, 1, dim, bits, variant == "garbage")[0]
        scale = float(np.float32(rng.uniform(0.05, 9.0)))
        snorm = float(np.float32(rng.uniform(0.0, 50.0)))
        a, b = rng.integers(0, n, 24).astype(np.uint32), rng.integers(0, n, 24).astype(np.uint32)
        ids = rng.choice(n, nids, replace=False).astype(np.uint32)
        stride = {"packed": 0, "garbage": 0, "inline_tags": da.lib().dann_inmem2_row_stride(DT[bits], dim),
                  "padded": (m.layer_bytes(bits, dim) + 15) // 16 * 16 + 48}[variant]
        for metric in METRICS:
            gix = da.Provider(DT[bits], metric, dim, n, 4, rows[n:], sq_scale=scale, sq_shift_norm_sq=snorm,
                              row_stride=stride, inline_tags=variant == "inline_tags")
            gix.set_elements(0, rows[:n])
            if variant == "padded":  # random bytes from the payload's end to the stride: inside the last wide load
                raw = rng.integers(0, 256, (n + 1, stride), dtype=np.uint8)
                raw[:, :rows.shape[1]] = rows
                _overwrite_store(gix, raw)
            gp = gix.distance_pairs(a, b)
            want = np.array([m.distance(metric, rows[i], rows[j], dim, bits, scale, snorm) for i, j in zip(a, b)], np.float32)
            assert np.array_equal(fbits(gp), fbits(want)), (bits, dim, metric, "pairs")
            gi, gd = gix.expand_beam(query, ids)
            want = np.array([m.distance(metric, query, rows[i], dim, bits, scale, snorm) for i in ids], np.float32)
            assert np.array_equal(gi, ids) and np.array_equal(fbits(gd), fbits(want)), (bits, dim, metric, "expand_beam")
            gix.close()


# ---- a shared index per bit width: compressed rows, the GPU provider and the oracle's twin -----------------------------------
@pytest.fixture(scope="module")
def sq4_l2():
    return Case(4, oracle.L2, 3000, 128, 24, 41)


@pytest.mark.parametrize("bits,dim,metric,tags", [
    (4, 128, oracle.L2, False), (4, 128, oracle.INNER_PRODUCT, False), (4, 128, oracle.COSINE_NORMALIZED, False),
    (1, 128, oracle.L2, False), (1, 128, oracle.INNER_PRODUCT, False), (1, 128, oracle.COSINE_NORMALIZED, False),
    (1, 256, oracle.L2, False), (1, 256, oracle.COSINE_NORMALIZED, False),
    (4, 128, oracle.L2, True), (1, 128, oracle.INNER_PRODUCT, True)])
def test_knn_search_matches_twin(bits, dim, metric, tags):
    """dim 128 runs the fixed-length kernels (query dwords and the SQ4 norm in registers), 256 the run-time loop; tags:
    the 128-d kernels on the Store layout with inline tags"""
    c = Case(bits, metric, 3000, dim, 24, 30 + bits + metric + dim, tags=tags)
    _, q, tq = c.queries(40)
    c.gix.debug_set(pair_min_queries=1)  # (the two-queries-per-wavefront kernel is not instantiated for packed rows)
    c.gix.kernel_time_reset()
    for L, W in ((20, 1), (64, 2), (100, 4)):
        oi, od, oc, ost = c.oix.search_batch(tq, L, W, 10)
        gi, gd, gst = c.gix.search(da.Knn(L, W), q, 10)
        assert np.array_equal(oi, gi) and np.array_equal(fbits(od), fbits(gd)), (L, W)
        assert np.array_equal(ost[:, 0], gst["cmps"]) and np.array_equal(ost[:, 1], gst["hops"]), (L, W)
    oi, od, _, _ = c.oix.search_batch(tq, 30, 1, 10)
    small_calls_from_threads(c.gix, q, 30, 1, 10, oi, od)
    fam = c.gix.search_families()
    assert fam["pair"][0] == 0 and fam["one_wave"][0] > 0, fam


def test_range_search_sq4(sq4_l2):
    c = sq4_l2
    _, q, tq = c.queries(12)
    _, d0 = c.oix.expand_beam(tq[0], np.arange(200, dtype=np.uint32))
    r_small, r_big = float(np.quantile(d0, 0.05)), float(np.quantile(d0, 0.4))
    for L, W, radius, inner, islack, rslack, maxret in ((20, 1, r_small, None, 1.0, 1.0, 0),
                                                        (8, 2, r_big, r_small, 0.25, 1.0, 0),
                                                        (8, 1, r_big, None, 0.5, 1.3, 40)):
        cap = 1500
        gi, gd, gst, gsec = c.gix.range_search(q, L, radius, W, inner, islack, rslack, maxret, out_cap=cap)
        for j in range(q.shape[0]):
            oi, od, ost = c.oix.range_search(tq[j], L, radius, W, inner, islack, rslack, maxret, out_cap=cap)
            k = oi.size
            assert int(gst["result_count"][j]) == k, (L, W, j)
            assert np.array_equal(gi[j, :k], oi) and np.array_equal(fbits(gd[j, :k]), fbits(od)), (L, W, j)
            assert int(gst["cmps"][j]) == int(ost[0]) and int(gst["hops"][j]) == int(ost[1]) and int(gsec[j]) == int(ost[3])


def test_filtered_searches_sq4(sq4_l2):
    c = sq4_l2
    _, q, tq = c.queries(16)
    match = c.rng.random(c.n + 1) < 0.4
    ids, dists, st = c.gix.filtered_search(da.Knn(20), q, 10, match)
    for j in range(q.shape[0]):
        wn, wi, wd, ws = c.oix.inline_filter_search(tq[j], 20, 10, match)
        assert np.array_equal(ids[j], wi) and np.array_equal(fbits(dists[j]), fbits(wd)), j
        assert (int(st["cmps"][j]), int(st["hops"][j]), int(st["written"][j])) == (int(ws[0]), int(ws[1]), wn)
    ids, dists, st = c.gix.filtered_search(da.Knn(24, 2), q, 10, match, mode=da.FILTER_MULTIHOP)
    for j in range(q.shape[0]):
        wn, wi, wd, ws = c.oix.multihop_search(tq[j], 24, 10, match, beam_width=2)
        assert np.array_equal(ids[j], wi) and np.array_equal(fbits(dists[j]), fbits(wd)), j
        assert (int(st["cmps"][j]), int(st["hops"][j]), int(st["written"][j])) == (int(ws[0]), int(ws[1]), wn)
    _, d0 = c.oix.expand_beam(tq[0], np.arange(200, dtype=np.uint32))
    radius = float(np.quantile(d0, 0.3))
    gi, gd, gst, gsec = c.gix.filtered_range_search(q, 12, radius, match, out_cap=1500)
    for j in range(q.shape[0]):
        oi, od, ost = c.oix.filtered_range_search(tq[j], 12, radius, match, out_cap=1500)
        k = oi.size
        assert int(gst["result_count"][j]) == k and np.array_equal(gi[j, :k], oi) and np.array_equal(fbits(gd[j, :k]), fbits(od))


def test_paged_search_sq4(sq4_l2):
    c = sq4_l2
    _, q, tq = c.queries(8)
    L, k, max_pages = 24, 7, 12
    s = c.gix.paged_search(q, L)
    want = [c.oix.paged_search(tq[j], L, k, max_pages=max_pages) for j in range(q.shape[0])]
    for page in range(max_pages):
        ids, dists, counts = s.next_page(k)
        for j in range(q.shape[0]):
            if page < len(want[j]):
                wi, wd = want[j][page]
                n = int(counts[j])
                assert n == len(wi) and np.array_equal(ids[j, :n], wi) and np.array_equal(fbits(dists[j, :n]), fbits(wd))
            else:
                assert counts[j] == 0
    s.close()


def test_diverse_search_sq4(sq4_l2):
    c = sq4_l2
    _, q, tq = c.queries(8)
    attrs = c.rng.integers(0, 7, c.n + 1).astype(np.uint32)
    c.gix.set_attributes(0, attrs)
    for L, W, dk in ((40, 1, 2), (40, 4, 1)):
        gi, gd, gst = c.gix.diverse_search(da.Knn(L, W), q, 10, dk, 10)
        for j in range(q.shape[0]):
            ids, dists, count, cmps, hops, _ = diverse_search(c.oix, tq[j], L, W, 10, dk, 10, attrs)
            n = len(ids)
            assert gi[j, :n].tolist() == ids and np.array_equal(fbits(gd[j, :n]), fbits(dists)), (L, W, j)
            assert (int(gst["cmps"][j]), int(gst["hops"][j]), int(gst["result_count"][j])) == (cmps, hops, count)


def test_save_and_load_vectors_sq4(sq4_l2, tmp_path):
    c = sq4_l2
    path = tmp_path / "rows.bin"
    c.gix.save_vectors_bin(path, 0, 100)
    raw = np.fromfile(path, np.uint8)
    assert raw[:8].view(np.uint32).tolist() == [100, m.layer_bytes(4, c.dim)]
    assert np.array_equal(raw[8:].reshape(100, -1), c.rows[:100])
    other = da.Provider(da.SQ4, da.L2, c.dim, 100, 4, c.start, sq_scale=c.scale, sq_shift_norm_sq=c.snorm)
    assert other.load_vectors_bin(path) == 100
    assert np.array_equal(other.get_element(7), c.rows[7])


def test_search_server_sq4():
    """the resident server stages queries in 16-byte units: SQ4 at dim 120 is 60 code bytes + 4 = 64"""
    c = Case(4, oracle.L2, 2000, 120, 24, 44)
    assert da.lib().dann_layer_bytes(da.SQ4, 120) == 64
    _, q, tq = c.queries(24)
    L, k = 32, 10
    oi, od, _, ost = c.oix.search_batch(tq, L, 1, k)
    c.gix.server_start(L, k, workers=32)
    try:
        tickets = [c.gix.submit(q[i]) for i in range(q.shape[0])]
        for i, t in enumerate(tickets):
            ids, d, st = c.gix.wait(t)
            assert np.array_equal(ids, oi[i]) and np.array_equal(fbits(d), fbits(od[i])), i
            assert (int(st["cmps"]), int(st["hops"])) == (int(ost[i, 0]), int(ost[i, 1])), i
    finally:
        c.gix.server_stop()
    with pytest.raises(da.DannError) as e:  # 68-byte queries: the server's 16-byte rule, as for SQ-8 rows
        Case(4, oracle.L2, 200, 128, 8, 45).gix.server_start(L, k, workers=32)
    assert e.value.status == da._ffi.EUNSUPPORTED


# ---- build --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,dim,metric", [(b, d, m) for m in METRICS for b, d in ((4, 32), (1, 16))],
                         ids=[f"{b}-{d}{t}" for t in ("", "-ip", "-cosn") for b, d in ((4, 32), (1, 16))])
def test_build_matches_twin(bits, dim, metric):
    """SQ1 at dim 16: distances take 17 values, nearly every pool holds ties (default tie order).  Inner product is the
    one metric under which RobustPrune takes its Occluding rule; CosineNormalized is the L2 kernel with an epilogue"""
    n, R, maxdeg, lb = 500, 8, 10, 24
    c = Case(bits, metric, n, dim, R, 50 + bits, adj=False, maxdeg=maxdeg)
    ocfg = oracle.build_config(R, maxdeg, lb, intra_batch_candidates=oracle.IBC_NONE)
    gcfg = da.build_config(R, maxdeg, lb, intra_batch_candidates=da.IBC_NONE)
    s = 0
    for b in (1, 2, 5, 20, 72, 400):
        slots = np.arange(s, min(s + b, n), dtype=np.uint32)
        c.oix.multi_insert(ocfg, slots)
        c.gix.insert_batch(gcfg, slots)
        s += b
    got = c.gix.download_graph()
    lens = c.oix.adj[:, 0]
    assert np.array_equal(got[:, 0], lens)
    mask = np.arange(maxdeg)[None, :] < lens[:, None]
    assert np.array_equal(got[:, 1:][mask], c.oix.adj[:, 1:][mask])


# ---- delete and consolidate ---------------------------------------------------------------------------------------------
def _same_graph(gix, oix):
    g, o = gix.download_graph(), oix.adj.copy()
    for a in (g, o):
        for r in range(a.shape[0]):
            a[r, 1 + min(int(a[r, 0]), gix.max_degree):] = 0
    bad = np.flatnonzero((g != o).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}"


def test_consolidate_sq4():
    _consolidate(4, 61)


def test_consolidate_sq1():
    _consolidate(1, 63)


def _consolidate(bits, seed):
    n, R = 1200, 32
    c = Case(bits, oracle.L2, n, 128, R, seed)
    deleted = np.zeros(n + 1, bool)
    deleted[c.rng.choice(n, n // 10, replace=False)] = True
    c.gix.delete_points(np.flatnonzero(deleted))
    kinds, cnt = c.gix.consolidate(da.build_config(24, R, 50))
    want = consolidate(c.oix, oracle.build_config(24, R, 50), deleted)
    assert np.array_equal(kinds, want)
    _same_graph(c.gix, c.oix)
    assert cnt[0] == n + 1 and cnt[2] > 0


def test_inplace_delete_sq4():
    _inplace_delete(4, 62)


def test_inplace_delete_sq1():
    _inplace_delete(1, 64)


def _inplace_delete(bits, seed):
    n, R = 1000, 32
    c = Case(bits, oracle.L2, n, 128, R, seed)
    deleted = np.zeros(n + 1, bool)
    ids = c.rng.choice(n, 16, replace=False)
    c.gix.set_prune_tie_order(da.TIE_RUST)
    got = c.gix.inplace_delete(da.build_config(24, R, 50), ids, method=da.INPLACE_TWO_HOP_AND_ONE_HOP, num_to_replace=3)
    want = inplace_delete(c.oix, oracle.build_config(24, R, 50), deleted, ids, da.INPLACE_TWO_HOP_AND_ONE_HOP, 3, TIE_RUST, 0, 0)
    assert got[:8].tolist() == want[:8].tolist(), (got, want)
    assert want[7] > 0 and want[1] > 0  # prunes ran
    _same_graph(c.gix, c.oix)
    assert np.array_equal(c.gix.get_deleted()[:n + 1], deleted.astype(np.uint8))


# ---- quantised search + rerank ------------------------------------------------------------------------------------------
def test_sq1_search_with_rerank():
    n, dim, R, L, k = 3000, 64, 16, 40, 10
    c = Case(1, oracle.L2, n, dim, R, 63)
    fp = da.Provider(da.F32, da.L2, dim, n, R, c.data[:1])
    fp.set_elements(0, c.data)
    qf, q, tq = c.queries(30)
    cand, _, _ = c.gix.search(da.Knn(L), q, L)
    ocand, _, _, _ = c.oix.search_batch(tq, L, 1, L)
    assert np.array_equal(cand, ocand)
    ids, d = fp.rerank(qf, cand, k)
    for j in range(30):
        cj = [int(x) for x in ocand[j] if x != 0xFFFFFFFF]
        dd = np.array([oracle.query_distance(oracle.F32, oracle.L2, qf[j], c.data[i]) for i in cj], np.float32)
        order = np.argsort(dd, kind="stable")[:k]
        assert [cj[i] for i in order] == [int(x) for x in ids[j, :len(order)]]
        assert np.array_equal(fbits(dd[order]), fbits(d[j, :len(order)]))


# ---- rejections ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 4])
def test_rejections(bits):
    start = np.zeros((1, m.layer_bytes(bits, 16)), np.uint8)
    with pytest.raises(da.DannError) as e:
        da.Provider(DT[bits], da.COSINE, 16, 10, 4, start, sq_scale=1.0)
    assert e.value.status == da._ffi.EUNSUPPORTED
    with pytest.raises(da.DannError) as e:
        da.Provider(DT[bits], da.L2, 16, 10, 4, start, sq_scale=0.0)
    assert e.value.status == da._ffi.EINVAL
    with pytest.raises(da.DannError) as e:
        da.sq_compress(np.zeros((2, 16), np.float32), np.zeros(16, np.float32), 1.0, 3)
    assert e.value.status == da._ffi.EINVAL
