"""MinMax rows of 4, 2 and 1 bit searched with MM8 query images (MinMaxQuery::EightBit; dann_set_query_dtype(idx,
DANN_MM8)).  Everything is compared bit for bit: one-hot rows against the query's own bytes (every element position),
distances and Knn searches against the CPU model (minmax_model.distance_matrix(..., qbits=8)), every other search kind
against the oracle's U8 L2 twin over the unpacked codes, the flat scans against flat_model / flat_gt_model over the
model's distances.  Every test sets the query dtype, so each fails where the library has no dann_set_query_dtype."""
import ctypes as C

import numpy as np
import pytest

import flat_gt_model as fg
import flat_model as fm
import minmax_model as m
import oracle
from diverse_model import diverse_search
from helpers import bits as fbits
from minmax_builders import MmModelCase, MmTwin, random_rows

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

DT = {1: da.MM1, 2: da.MM2, 4: da.MM4, 8: da.MM8}
ROW_BITS = (4, 2, 1)
# the seams of the 4-lane / 128-element steps and of their tail: a row dword is 8 / 16 / 32 elements, the staged query is
# rounded to 16 (1 bit: 32) bytes
DIMS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300)


def _hip():
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


class DevBuf:
    """a device buffer through the HIP runtime (the device-pointer entry points)"""

    def __init__(self, nbytes, src=None):
        self.hip, self.p, self.n = _hip(), C.c_void_p(), nbytes
        assert self.hip.hipMalloc(C.byref(self.p), max(nbytes, 16)) == 0
        if src is not None:
            src = np.ascontiguousarray(src)
            assert self.hip.hipMemcpy(self.p, src.ctypes.data_as(C.c_void_p), src.nbytes, 1) == 0

    def get(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.n and self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, out.nbytes, 2) == 0
        return out

    def __del__(self):
        if self.p:
            self.hip.hipFree(self.p)


def _overwrite_store(gix, raw):
    """the whole row buffer of `gix` replaced by `raw` (nslots x row_stride bytes)"""
    hip = _hip()
    rows_ptr, _ = gix.device_pointers()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    assert raw.shape == (gix.capacity + gix.num_start_points, gix.row_stride)
    assert hip.hipMemcpy(C.c_void_p(rows_ptr), raw.ctypes.data_as(C.c_void_p), raw.nbytes, 1) == 0
    assert hip.hipDeviceSynchronize() == 0


def _rerank_order(dd):
    key = fbits(dd + np.float32(0.0)).astype(np.int64)
    key = np.where(key & 0x80000000, ~key & 0xFFFFFFFF, key | 0x80000000)
    return np.lexsort((np.arange(dd.size), key))


def _unit_rows(codes, bits):
    """a = 1, b = 0 (n = sum(code), norm_squared = sum(code^2)): the inner product is the raw product of the codes"""
    c = np.ascontiguousarray(codes, dtype=np.uint8).astype(np.int64)
    n = c.shape[0]
    return m.make_rows(codes, bits, np.zeros(n), c.sum(1), np.ones(n), (c * c).sum(1))


def _garbage_padding(rng, rows, bits, dim):
    used = dim * bits - 8 * (m.code_bytes(bits, dim) - 1)
    if used < 8:
        rows[:, -1] |= (rng.integers(0, 256, rows.shape[0], dtype=np.uint8) << used).astype(np.uint8)
    return rows


# ---- 1. every element position ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("bits", ROW_BITS)
def test_every_element_position(bits, dim):
    """row j holds the largest code at element j and zeros elsewhere; the query's bytes are pairwise distinguishable
    within any window of 250 elements.  Under the inner product row j must score exactly -q_j * (2^bits - 1): a wrong
    byte lane, a wrong shift, a wrong plane or a product beyond dim shows as another value.  Random bits in the rows'
    padding, random bytes behind the query in the device buffer of the device-pointer run."""
    rng = np.random.default_rng(1000 * bits + dim)
    top = (1 << bits) - 1
    codes = np.zeros((dim + 1, dim), np.uint8)
    codes[np.arange(dim), np.arange(dim)] = top
    rows = _garbage_padding(rng, _unit_rows(codes, bits), bits, dim)
    qc = ((37 * np.arange(dim) + 11) % 251 + 1).astype(np.uint8)[None, :]
    q = _unit_rows(qc, 8)
    want = -(qc[0].astype(np.float32) * np.float32(top))
    gix = da.Provider(DT[bits], da.INNER_PRODUCT, dim, dim, 4, rows[dim:])
    gix.set_elements(0, rows[:dim])
    gix.set_query_dtype(da.MM8)
    assert gix.query_bytes() == 20 + dim == q.shape[1]
    ids = np.arange(dim, dtype=np.uint32)
    got = gix.expand_beam_batch(q, ids, np.array([0, dim], np.uint64))
    assert np.array_equal(fbits(got), fbits(want)), (bits, dim, np.flatnonzero(got != want)[:8])
    # device pointers: the query image, then bytes that are no query
    buf = np.concatenate([q[0], rng.integers(1, 256, 64, dtype=np.uint8)])
    dq, dc = DevBuf(buf.nbytes, buf), DevBuf(dim * 4, ids)
    di, dd = DevBuf(dim * 4), DevBuf(dim * 4)
    da._ffi.check(da.lib().dann_rerank_batch_device(gix._h, dq.p, 1, dc.p, dim, dim, di.p, dd.p), "dann_rerank_batch_device")
    ri, rd = di.get(np.uint32, (dim,)), dd.get(np.float32, (dim,))
    assert np.array_equal(np.sort(ri), ids) and np.array_equal(fbits(rd), fbits(want[ri])), (bits, dim)
    gix.close()


# ---- 2. distances -------------------------------------------------------------------------------------------------------
DIST_DIMS = (1, 9, 31, 64, 100, 128, 129, 257)


@pytest.mark.parametrize("variant", ["packed", "store", "odd"])
@pytest.mark.parametrize("bits", ROW_BITS)
def test_distances_match_model(bits, variant):
    """dann_query_distance, dann_expand_beam, dann_expand_beam_batch (ragged, one empty list) and dann_rerank_batch with
    MM8 queries, all four metrics; the variants of tests/test_gpu_minmax.py::test_distances_match_model: random bits in the
    padding of the last code byte everywhere; store: the Store stride with inline tags, odd: an odd multiple of 16 beyond
    the payload -- both with random bytes between payload (tag) and stride."""
    rng = np.random.default_rng(3100 + 10 * bits + len(variant))
    n, nq = 48, 6
    for dim in DIST_DIMS:
        rows = random_rows(rng, n + 1, dim, bits, garbage=True)
        lb = rows.shape[1]
        lens = rng.integers(1, n, nq)
        lens[3] = 0
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        ids = np.concatenate([rng.choice(n + 1, l, replace=False) for l in lens]).astype(np.uint32)
        ids[0] = n
        cand = np.stack([rng.permutation(n + 1)[:30] for _ in range(nq)]).astype(np.uint32)
        cand[:, 5], cand[:, 7] = 0xFFFFFFFF, n
        if variant == "store":
            stride = da.lib().dann_inmem2_row_stride(DT[bits], dim)
        elif variant == "odd":
            stride = (lb + 15) // 16 * 16 + 16
            stride += 16 * (stride // 16 % 2 == 0)
        else:
            stride = 0
        q = random_rows(rng, nq, dim, 8)
        for metric in m.METRICS:
            gix = da.Provider(DT[bits], metric, dim, n, 4, rows[n:], row_stride=stride, inline_tags=variant == "store")
            gix.set_elements(0, rows[:n])
            if stride:
                raw = rng.integers(0, 256, (n + 1, stride), dtype=np.uint8)
                raw[:, :lb] = rows
                if variant == "store":
                    raw[:, lb] = gix.get_tags(0, n + 1)
                _overwrite_store(gix, raw)
            gix.set_query_dtype(da.MM8)
            D = m.distance_matrix(metric, q, rows, dim, bits, qbits=8)
            tag = (bits, dim, metric, variant)
            got = gix.expand_beam_batch(q, ids, off)
            want = np.concatenate([D[j, ids[int(off[j]):int(off[j + 1])]] for j in range(nq)])
            assert np.array_equal(fbits(got), fbits(want)), tag + ("expand_beam_batch",)
            for j in (0, nq - 1):
                assert fbits(np.float32(gix.query_distance(q[j], rows[n - j]))) == fbits(D[j, n - j]), tag + ("query_distance",)
            some = np.array([n, 0, 7, n - 1], np.uint32)
            oi, od = gix.expand_beam(q[1], some)
            assert np.array_equal(oi, some) and np.array_equal(fbits(od), fbits(D[1, some])), tag + ("expand_beam",)
            gi, gd = gix.rerank(q, cand, 12)
            for j in range(nq):
                c = [int(x) for x in cand[j] if x != 0xFFFFFFFF]
                dd = D[j, c]
                order = _rerank_order(dd)[:12]
                assert [c[i] for i in order] == gi[j].tolist(), tag + ("rerank", j)
                assert np.array_equal(fbits(dd[order]), fbits(gd[j])), tag + ("rerank", j)
            gix.close()


@pytest.mark.parametrize("bits", ROW_BITS)
def test_the_query_is_the_first_argument(bits):
    """a sample on which the epilogue's two argument orders differ in bits (asserted on the model first): the query must
    be x and the row y"""
    dim, n, nq = 100, 96, 24
    rng = np.random.default_rng(7100 + bits)
    rows = random_rows(rng, n + 1, dim, bits)
    q = random_rows(rng, nq, dim, 8)
    D = m.distance_matrix(m.L2, q, rows, dim, bits, qbits=8)
    swapped = m.distance_matrix(m.L2, rows, q, dim, 8, qbits=bits).T  # the rows as x, the queries as y
    assert int((fbits(D) != fbits(swapped)).sum()) > 20
    gix = da.Provider(DT[bits], da.L2, dim, n, 4, rows[n:])
    gix.set_elements(0, rows[:n])
    gix.set_query_dtype(da.MM8)
    ids = np.tile(np.arange(n + 1, dtype=np.uint32), nq)
    off = (np.arange(nq + 1) * (n + 1)).astype(np.uint64)
    assert np.array_equal(fbits(gix.expand_beam_batch(q, ids, off)), fbits(D.ravel()))


# ---- 3. Knn search against the model's search ---------------------------------------------------------------------------
def _queries8(c, nq):
    q, _, _ = m.compress(c.rng.normal(0.2, 1.0, (nq, c.dim)).astype(np.float32), 8, 0.95)
    return q


def _check_knn(c, nq, cases, tags=None, want_family=None):
    c.gix.set_query_dtype(da.MM8)
    q = _queries8(c, nq)
    D = m.distance_matrix(c.metric, q, c.all_rows, c.dim, c.bits, qbits=8)
    readable = None if tags is None else tags >= 254
    k = 10
    dq = DevBuf(q.nbytes, q)
    c.gix.kernel_time_reset()
    for L, W in cases:
        gi, gd, gst = c.gix.search(da.Knn(L, W), q, k)  # host pointers
        di, dd, ds = DevBuf(nq * k * 4), DevBuf(nq * k * 4), DevBuf(nq * 20)
        da._ffi.check(da.lib().dann_search_batch_device(c.gix._h, dq.p, nq, L, W, k, di.p, dd.p, ds.p),
                      "dann_search_batch_device")
        hi, hd = di.get(np.uint32, (nq, k)), dd.get(np.float32, (nq, k))
        hst = ds.get(np.uint8, (nq * 20,)).view(da.STATS_DTYPE)
        for j in range(nq):
            ids, d, cmps, hops, written = m.knn_search(lambda i: D[j, i], c.adj, c.n, c.nstart, c.R, L, W, k, readable)
            tag = (c.bits, c.dim, c.metric, L, W, j)
            assert cmps > L + c.nstart, tag  # (the queue filled and dropped: the merge's every path ran)
            assert np.array_equal(gi[j], ids) and np.array_equal(fbits(gd[j]), fbits(d)), tag
            assert (int(gst["cmps"][j]), int(gst["hops"][j]), int(gst["written"][j])) == (cmps, hops, written), tag
            assert np.array_equal(hi[j], ids) and np.array_equal(fbits(hd[j]), fbits(d)), tag + ("device",)
            assert (int(hst["cmps"][j]), int(hst["hops"][j]), int(hst["written"][j])) == (cmps, hops, written), tag
    fam = c.gix.search_families()
    assert sum(v[0] for f, v in fam.items() if f not in ("one_wave", "persistent")) == 0, fam
    if want_family:
        assert fam[want_family][0] > 0 and sum(v[0] for f, v in fam.items() if f != want_family) == 0, fam
    else:
        assert fam["one_wave"][0] + fam["persistent"][0] > 0, fam


@pytest.mark.parametrize("dim", [128, 100])
@pytest.mark.parametrize("metric", m.METRICS)
@pytest.mark.parametrize("bits", ROW_BITS)
def test_knn_search_matches_model_search(bits, metric, dim):
    """L + start points at 64 / 65 and 128 / 129 (one, two, three queue registers per lane), W = 1 (plain mode) and 3
    (general); dim 128: whole steps only, dim 100: the tail step alone"""
    c = MmModelCase(bits, metric, 2000, dim, 16, 5200 + 16 * bits + 4 * metric + dim)
    _check_knn(c, 6, ((63, 1), (64, 3), (127, 3), (128, 1)))


def test_knn_search_with_unpublished_slots():
    """inline tags (the general mode's tag reads) on the Store's stride"""
    c = MmModelCase(4, m.L2, 2000, 100, 16, 5290, tags=True)
    tags = np.full(c.n + 1, 254, np.uint8)
    tags[c.rng.choice(c.n, 300, replace=False)] = c.rng.integers(0, 3, 300)
    tags[c.n] = 255
    c.gix.set_tags(0, tags)
    _check_knn(c, 6, ((63, 1), (64, 3)), tags=tags)


def test_knn_search_on_persistent_waves():
    c = MmModelCase(2, m.IP, 2000, 128, 16, 5280)
    c.gix.set_max_concurrency(4)
    _check_knn(c, 12, ((64, 1),), want_family="persistent")
    c.gix.set_max_concurrency(0)


# ---- 4. the oracle's U8 L2 twin -----------------------------------------------------------------------------------------
TWINS = [(4, 128), (4, 64), (2, 100), (2, 128), (1, 128), (1, 100)]


@pytest.mark.parametrize("bits,dim", TWINS)
def test_twin_searches(bits, dim):
    """Knn, range, inline-filtered, multihop, filtered-range, paged and diverse searches: rows twin_rows(codes, bits),
    queries twin_rows(qcodes, 8), the oracle a U8 L2 index over the unpacked codes with the queries' codes as they are"""
    assert 2 * 255 * 255 * dim < (1 << 24)  # every intermediate of the epilogue is an exact integer
    c = MmTwin(bits, dim, 2000, 16, 6300 + bits + dim)
    c.gix.set_query_dtype(da.MM8)
    tq = c.rng.integers(0, 256, (8, dim), dtype=np.uint8)
    q = m.twin_rows(tq, 8)
    nq = q.shape[0]
    for L, W in ((10, 1), (32, 2)):
        oi, od, oc, ost = c.oix.search_batch(tq, L, W, 10)
        gi, gd, gst = c.gix.search(da.Knn(L, W), q, 10)
        assert np.array_equal(oi, gi) and np.array_equal(fbits(od), fbits(gd)), (L, W)
        assert np.array_equal(ost[:, 0], gst["cmps"]) and np.array_equal(ost[:, 1], gst["hops"]), (L, W)
    _, d0 = c.oix.expand_beam(tq[0], np.arange(200, dtype=np.uint32))
    r_small, r_big = float(np.quantile(d0, 0.05)), float(np.quantile(d0, 0.4))
    for L, W, radius, inner, islack, rslack, maxret in ((20, 1, r_small, None, 1.0, 1.0, 0),
                                                        (8, 2, r_big, r_small, 0.25, 1.0, 0),
                                                        (8, 1, r_big, None, 0.5, 1.3, 40)):
        cap = c.n + 1  # (8-bit queries lie far from every 4-, 2- or 1-bit row: a slack of 1.3 takes in the whole index)
        gi, gd, gst, gsec = c.gix.range_search(q, L, radius, W, inner, islack, rslack, maxret, out_cap=cap)
        for j in range(nq):
            oi, od, ost = c.oix.range_search(tq[j], L, radius, W, inner, islack, rslack, maxret, out_cap=cap)
            k = oi.size
            assert int(gst["result_count"][j]) == k, (L, W, j)
            assert np.array_equal(gi[j, :k], oi) and np.array_equal(fbits(gd[j, :k]), fbits(od)), (L, W, j)
            assert int(gst["cmps"][j]) == int(ost[0]) and int(gst["hops"][j]) == int(ost[1]) and int(gsec[j]) == int(ost[3])
    match = c.rng.random(c.n + 1) < 0.4
    ids, dists, st = c.gix.filtered_search(da.Knn(20), q, 10, match)
    for j in range(nq):
        wn, wi, wd, ws = c.oix.inline_filter_search(tq[j], 20, 10, match)
        assert np.array_equal(ids[j], wi) and np.array_equal(fbits(dists[j]), fbits(wd)), j
        assert (int(st["cmps"][j]), int(st["hops"][j]), int(st["written"][j])) == (int(ws[0]), int(ws[1]), wn)
    ids, dists, st = c.gix.filtered_search(da.Knn(24, 2), q, 10, match, mode=da.FILTER_MULTIHOP)
    for j in range(nq):
        wn, wi, wd, ws = c.oix.multihop_search(tq[j], 24, 10, match, beam_width=2)
        assert np.array_equal(ids[j], wi) and np.array_equal(fbits(dists[j]), fbits(wd)), j
        assert (int(st["cmps"][j]), int(st["hops"][j]), int(st["written"][j])) == (int(ws[0]), int(ws[1]), wn)
    radius = float(np.quantile(d0, 0.3))
    gi, gd, gst, gsec = c.gix.filtered_range_search(q, 12, radius, match, out_cap=c.n + 1)
    for j in range(nq):
        oi, od, ost = c.oix.filtered_range_search(tq[j], 12, radius, match, out_cap=c.n + 1)
        k = oi.size
        assert int(gst["result_count"][j]) == k and np.array_equal(gi[j, :k], oi) and np.array_equal(fbits(gd[j, :k]), fbits(od))
    L, k, max_pages = 24, 7, 8
    s = c.gix.paged_search(q[:6], L)
    want = [c.oix.paged_search(tq[j], L, k, max_pages=max_pages) for j in range(6)]
    for page in range(max_pages):
        ids, dists, counts = s.next_page(k)
        for j in range(6):
            if page < len(want[j]):
                wi, wd = want[j][page]
                n = int(counts[j])
                assert n == len(wi) and np.array_equal(ids[j, :n], wi) and np.array_equal(fbits(dists[j, :n]), fbits(wd))
            else:
                assert counts[j] == 0
    s.close()
    attrs = c.rng.integers(0, 7, c.n + 1).astype(np.uint32)
    c.gix.set_attributes(0, attrs)
    for L, W, dk in ((40, 1, 2), (40, 4, 1)):
        gi, gd, gst = c.gix.diverse_search(da.Knn(L, W), q[:6], 10, dk, 10)
        for j in range(6):
            ids, dists, count, cmps, hops, _ = diverse_search(c.oix, tq[j], L, W, 10, dk, 10, attrs)
            n = len(ids)
            assert gi[j, :n].tolist() == ids and np.array_equal(fbits(gd[j, :n]), fbits(dists)), (L, W, j)
            assert (int(gst["cmps"][j]), int(gst["hops"][j]), int(gst["result_count"][j])) == (cmps, hops, count)


# ---- 5. the flat scans --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,dim", [(4, 100), (1, 129)])
def test_flat_scans(bits, dim):
    """dann_flat_search_batch, unfiltered, with a shared and with a per-query filter, and dann_flat_range_search_batch, over
    1500 slots (two default chunks) of few distinct rows: ties everywhere"""
    rng = np.random.default_rng(8000 + bits)
    n, nq, k = 1500, 5, 20
    base = random_rows(rng, 40, dim, bits, garbage=True)
    rows = base[rng.integers(0, 40, n + 1)]
    q = random_rows(rng, nq, dim, 8)
    gix = da.Provider(DT[bits], da.L2, dim, n, 4, rows[n:])
    gix.set_elements(0, rows[:n])
    gix.set_query_dtype(da.MM8)
    D = m.distance_matrix(m.L2, q, rows[:n], dim, bits, qbits=8)
    shared = rng.random(n + 1) < 0.3
    per_query = rng.random((nq, n + 1)) < 0.3
    for name, match in (("all", None), ("shared", shared), ("per query", per_query)):
        ids, d, st = gix.flat_search(q, k, stats=True, match=match)
        for j in range(nq):
            mj = np.ones(n, bool) if match is None else (match[j, :n] if match.ndim == 2 else match[:n])
            (pos, wd), (cpos, cd) = fg.filtered_knn(D[j], mj, k)
            assert np.array_equal(pos, cpos) and np.array_equal(fbits(wd), fbits(cd))
            wi, wdd = fm.padded(pos, wd, k)
            assert np.array_equal(ids[j], wi) and np.array_equal(fbits(d[j]), fbits(wdd)), (bits, name, j)
            assert int(st["cmps"][j]) == int(mj.sum()), (bits, name, j)
    radius, inner = float(np.quantile(D, 0.2)), float(np.quantile(D, 0.05))
    for name, match in (("all", None), ("shared", shared)):
        ids, d, cnt = gix.flat_range_search(q, radius, inner_radius=inner, match=match, out_cap=n)
        for j in range(nq):
            pos, wd = fg.range_scan(D[j], np.ones(n, bool) if match is None else match[:n], radius, inner)
            c = int(cnt[j])
            assert c == pos.size and np.array_equal(ids[j, :c], pos) and np.array_equal(fbits(d[j, :c]), fbits(wd)), (bits, name, j)
        assert int(cnt.sum()) > 0  # (one radius for queries of different scales: some bands are empty, not all)
    gix.close()


# ---- 6. unchanged neighbours --------------------------------------------------------------------------------------------
def test_stored_row_queries_and_a_reset_index_are_unchanged():
    """what takes a stored row as the query -- build, prune_batch, search_record -- gives the same results whether or not
    MM8 is set; an index set to MM8 and back answers a same-width search as a fresh one does"""
    bits, dim, n, R = 4, 100, 1200, 16

    def run(q8):
        c = MmModelCase(bits, m.L2, n, dim, R, 9100)
        gcfg = da.build_config(12, R, 24, intra_batch_candidates=da.IBC_NONE)
        if q8:
            c.gix.set_query_dtype(da.MM8)
            assert c.gix.query_dtype() == da.MM8
        slots = np.arange(0, n, 97, dtype=np.uint32)
        rec = c.gix.search_record(slots, 30)
        locs = np.arange(5, 400, 41, dtype=np.uint32)
        pools = [np.setdiff1d(c.rng.choice(n, 60, replace=False), [l]).astype(np.uint32) for l in locs]
        off = np.concatenate([[0], np.cumsum([p.size for p in pools])]).astype(np.uint64)
        pid = np.concatenate(pools)
        pd = c.gix.distance_pairs(np.repeat(locs, [p.size for p in pools]), pid)
        pruned = c.gix.prune_batch(gcfg, locs, pid, pd, off)
        c.gix.build(gcfg, 0, n, 0.1, 512)
        graph = c.gix.download_graph()
        if q8:
            c.gix.set_query_dtype(DT[bits])
            assert c.gix.query_dtype() == DT[bits] and c.gix.query_bytes() == m.layer_bytes(bits, dim)
        own = c.gix.search(da.Knn(40, 2), c.queries(6), 10)
        return rec, pruned, graph, own

    a, b = run(False), run(True)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(fbits(a[3][1]), fbits(b[3][1]))
    assert np.array_equal(a[3][2]["cmps"], b[3][2]["cmps"])


# ---- 7. statuses --------------------------------------------------------------------------------------------------------
def test_statuses():
    E, L = da._ffi, da.lib()
    out = C.c_int32(-7)
    assert L.dann_set_query_dtype(None, da.MM8) == E.EINVAL and L.dann_get_query_dtype(None, C.byref(out)) == E.EINVAL
    dim = 64
    for bits in m.BITS:
        start = random_rows(np.random.default_rng(bits), 1, dim, bits)
        gix = da.Provider(DT[bits], da.L2, dim, 10, 4, start)
        assert L.dann_get_query_dtype(gix._h, None) == E.EINVAL
        assert gix.query_dtype() == DT[bits]  # the default: the index's own
        for other in m.BITS:
            rc = L.dann_set_query_dtype(gix._h, DT[other])
            if other == bits:
                assert rc == 0 and gix.query_dtype() == DT[bits]
            elif other == 8:
                assert rc == 0 and gix.query_dtype() == da.MM8 and gix.query_bytes() == 20 + dim
                assert L.dann_set_query_dtype(gix._h, DT[bits]) == 0 and gix.query_bytes() == m.layer_bytes(bits, dim)
            else:
                before = gix.query_dtype()
                assert rc == E.EUNSUPPORTED and gix.query_dtype() == before  # a refused setting changes nothing
        for foreign in (da.F32, da.U8, da.SPH1, da.SQ4, da.PQ, 113, 116, 48, 7, -1):
            assert L.dann_set_query_dtype(gix._h, foreign) == E.EINVAL, (bits, foreign)
        with pytest.raises(da.DannError) as e:
            gix.set_query_layout(da.QUERY_EIGHT_BIT)
        assert e.value.status == E.EUNSUPPORTED
        if bits != 8:
            gix.set_query_dtype(da.MM8)
            with pytest.raises(da.DannError) as e:
                gix.set_query_layout(da.QUERY_EIGHT_BIT)
            assert e.value.status == E.EUNSUPPORTED and gix.query_dtype() == da.MM8
            q = np.zeros(20 + dim + 1, np.uint8)
            q[:4] = np.array([dim], np.uint32).view(np.uint8)
            h = C.c_void_p()
            for nbytes, want in ((20 + dim + 1, E.ELENGTH), (20 + dim - 1, E.ELENGTH), (m.layer_bytes(bits, dim), E.ELENGTH),
                                 (20 + dim, 0)):
                assert L.dann_query_create(gix._h, q.ctypes.data_as(C.c_void_p), nbytes, C.byref(h)) == want, (bits, nbytes)
            # a dann_query keeps the dtype it was created under
            gix.set_query_dtype(DT[bits])
            d = C.c_float()
            assert L.dann_query_distance(h, start.ctypes.data_as(C.c_void_p), start.nbytes, C.byref(d)) == 0
            zero_q = np.zeros((1, 20 + dim), np.uint8)
            zero_q[0, :4] = q[:4]
            assert fbits(np.float32(d.value)) == fbits(m.distance_matrix(m.L2, zero_q, start, dim, bits, qbits=8)[0, 0])
            L.dann_query_destroy(h)
        gix.close()
    # indexes that have no MM8 queries: their own dtype is accepted, MM8 is no dtype of theirs
    for dt, start in ((da.F32, np.zeros((1, 8), np.float32)), (da.SPH1, np.zeros((1, 7), np.uint8))):
        f = da.Provider(dt, da.L2, 8, 10, 4, start)
        assert L.dann_set_query_dtype(f._h, dt) == 0 and f.query_dtype() == dt
        assert L.dann_set_query_dtype(f._h, da.MM8) == E.EINVAL and f.query_dtype() == dt
        f.close()
    # dim * 255 * (2^bits - 1) must fit the u32 of the raw product
    top = (1 << 32) // (255 * 15)
    big = da.Provider(da.MM4, da.L2, top + 1, 2, 4, m.make_rows(np.zeros((1, top + 1), np.uint8), 4, [0], [0], [1], [0]))
    assert L.dann_set_query_dtype(big._h, da.MM8) == E.EINVAL and big.query_dtype() == da.MM4
    big.close()


def test_search_server():
    """the server keeps its 16-byte rule: 20 + 108 = 128 is served, 20 + 128 = 148 is refused; the setting is refused
    while the server runs"""
    E = da._ffi
    c = MmModelCase(4, m.L2, 500, 108, 16, 9700)
    c.gix.set_query_dtype(da.MM8)
    q = _queries8(c, 4)
    D = m.distance_matrix(m.L2, q, c.all_rows, c.dim, 4, qbits=8)
    c.gix.server_start(32, 10, workers=8)
    try:
        for other in (da.MM4, da.MM8):
            with pytest.raises(da.DannError) as e:
                c.gix.set_query_dtype(other)
            assert e.value.status == E.EBUSY
        tickets = [c.gix.submit(q[j]) for j in range(4)]
        for j, t in enumerate(tickets):
            ids, d, st = c.gix.wait(t)
            wi, wd, cmps, hops, _ = m.knn_search(lambda i: D[j, i], c.adj, c.n, c.nstart, c.R, 32, 1, 10, None)
            assert np.array_equal(ids, wi) and np.array_equal(fbits(d), fbits(wd)), j
    finally:
        c.gix.server_stop()
    start = random_rows(np.random.default_rng(82), 1, 128, 4)
    gix = da.Provider(da.MM4, da.L2, 128, 10, 4, start)
    gix.set_query_dtype(da.MM8)
    with pytest.raises(da.DannError) as e:
        gix.server_start(32, 10, workers=8)
    assert e.value.status == E.EUNSUPPORTED and gix.query_bytes() == 148
