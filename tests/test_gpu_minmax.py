"""MinMax-quantised rows (MM1 / MM2 / MM4 / MM8) on the GPU.  Everything is compared bit for bit: distances and Knn
searches against the CPU model (tests/minmax_model.py), every other search kind, the build and the graph mutations
against the oracle's U8 L2 twin (rows with a = 1, b = 0, whose L2 is exactly the squared distance of their codes), the
compressor against the model's bytes.  The query layout is DANN_QUERY_SAME_AS_DATA throughout: DANN_QUERY_EIGHT_BIT is
reserved and answers DANN_EUNSUPPORTED (test_rejections)."""
import ctypes as C

import numpy as np
import pytest

import minmax_model as m
import oracle
from consolidate_model import consolidate
from diverse_model import diverse_search
from helpers import bits as fbits
from inplace_delete_model import TIE_RUST, inplace_delete
from minmax_builders import MmModelCase, MmTwin, random_rows

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

DT = {1: da.MM1, 2: da.MM2, 4: da.MM4, 8: da.MM8}
# the seams of the 4-lane / 32-dimension steps (MM1 / MM2 / MM4) and of the 8-lane / 16-byte steps (MM8), with a tail step
# in the last slot
DIMS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 260, 300)


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
    """the whole row buffer of `gix` replaced by `raw` (nslots x row_stride bytes): the one way to put bytes between a
    row's payload and its stride, which no entry point of the library writes"""
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


# ---- 1. distances -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["packed", "store", "odd"])
@pytest.mark.parametrize("bits", m.BITS)
def test_distances_match_model(bits, variant):
    """dann_distance_pairs (both orders), dann_distance, dann_query_distance, dann_expand_beam, dann_expand_beam_batch
    (ragged, one empty list) and dann_rerank_batch.  Random bits in the padding of the last code byte everywhere; store:
    the Store stride with inline tags, odd: an odd multiple of 16 beyond the payload -- both with random bytes between
    payload (tag) and stride.  The last slot of the index (the start point) is read by every entry point."""
    rng = np.random.default_rng(100 + 10 * bits + len(variant))
    n, nq = 48, 6
    for dim in DIMS:
        rows = random_rows(rng, n + 1, dim, bits, garbage=True)
        lb = rows.shape[1]
        assert lb == m.layer_bytes(bits, dim) == da.lib().dann_layer_bytes(DT[bits], dim)
        a = np.concatenate([rng.integers(0, n + 1, 22), [n, 3]]).astype(np.uint32)
        b = np.concatenate([rng.integers(0, n + 1, 22), [5, n]]).astype(np.uint32)
        lens = rng.integers(1, n, nq)
        lens[3] = 0
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        ids = np.concatenate([rng.choice(n + 1, l, replace=False) for l in lens]).astype(np.uint32)
        ids[0] = n
        cand = np.stack([rng.permutation(n + 1)[:30] for _ in range(nq)]).astype(np.uint32)
        cand[:, 5], cand[:, 7] = 0xFFFFFFFF, n
        if variant == "store":
            stride = da.lib().dann_inmem2_row_stride(DT[bits], dim)
            assert stride == m.store_stride(bits, dim)
        elif variant == "odd":
            stride = (lb + 15) // 16 * 16 + 16
            stride += 16 * (stride // 16 % 2 == 0)
        else:
            stride = 0
        q = random_rows(rng, nq, dim, bits, garbage=True)
        for metric in m.METRICS:
            gix = da.Provider(DT[bits], metric, dim, n, 4, rows[n:], row_stride=stride, inline_tags=variant == "store")
            gix.set_elements(0, rows[:n])
            if stride:
                raw = rng.integers(0, 256, (n + 1, stride), dtype=np.uint8)
                raw[:, :lb] = rows
                if variant == "store":
                    raw[:, lb] = gix.get_tags(0, n + 1)
                _overwrite_store(gix, raw)
            R = m.distance_matrix(metric, rows, rows, dim, bits)
            tag = (bits, dim, metric, variant)
            assert np.array_equal(fbits(gix.distance_pairs(a, b)), fbits(R[a, b])), tag + ("pairs",)
            assert np.array_equal(fbits(gix.distance_pairs(b, a)), fbits(R[b, a])), tag + ("pairs, swapped",)
            assert fbits(np.float32(gix.distance(rows[1], rows[n]))) == fbits(R[1, n]), tag + ("distance",)
            assert fbits(np.float32(gix.distance(rows[n], rows[1]))) == fbits(R[n, 1]), tag + ("distance, swapped",)
            D = m.distance_matrix(metric, q, rows, dim, bits)
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


@pytest.mark.parametrize("bits", m.BITS)
def test_pairs_keep_the_argument_order(bits):
    """the sample of tests/test_minmax_model_host.py::test_argument_order_matters_on_the_sample: every ordered pair"""
    dim, n = 100, 96
    rows = random_rows(np.random.default_rng(7000 + bits), n, dim, bits)
    R = m.distance_matrix(m.L2, rows, rows, dim, bits)
    assert int((fbits(R) != fbits(R.T)).sum()) > 20
    gix = da.Provider(DT[bits], da.L2, dim, n - 1, 4, rows[n - 1:])
    gix.set_elements(0, rows[:n - 1])
    a, b = (x.ravel().astype(np.uint32) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    assert np.array_equal(fbits(gix.distance_pairs(a, b)), fbits(R.ravel()))


def test_raw_product_beyond_2_24():
    """MM8, dim 300, every code 255 (every other row: one code 254): raw > 2^24, the u32 -> f32 conversion rounds"""
    rng = np.random.default_rng(5)
    dim, n = 300, 12
    rows = random_rows(rng, n + 1, dim, 8)
    rows[:, m.HEADER:] = 255
    rows[::2, m.HEADER] = 254  # (even x odd rows: raw = 300 * 255^2 - 255, odd and beyond 2^24 -- no f32 holds it)
    raw = m.codes_of(rows, 8, dim).astype(np.int64) @ m.codes_of(rows, 8, dim).astype(np.int64).T
    assert raw.min() > (1 << 24) and (raw.astype(np.float32).astype(np.int64) != raw).any()
    for metric in m.METRICS:
        gix = da.Provider(da.MM8, metric, dim, n, 4, rows[n:])
        gix.set_elements(0, rows[:n])
        R = m.distance_matrix(metric, rows, rows, dim, 8)
        a, b = np.arange(n + 1, dtype=np.uint32), np.arange(n + 1, dtype=np.uint32)[::-1].copy()
        assert np.array_equal(fbits(gix.distance_pairs(a, b)), fbits(R[a, b])), metric
        off = np.array([0, n + 1], np.uint64)
        assert np.array_equal(fbits(gix.expand_beam_batch(rows[2:3], a, off)), fbits(R[2, a])), metric


# ---- 2. Knn search against the model's search ---------------------------------------------------------------------------
def _check_knn(c, nq, cases, tags=None, want_family=None):
    q = c.queries(nq)
    D = m.distance_matrix(c.metric, q, c.all_rows, c.dim, c.bits)
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
    assert fam["team"][0] == 0 and fam["pair"][0] == 0 and fam["pq_lut"][0] == 0, fam
    if want_family:
        assert fam[want_family][0] > 0 and sum(v[0] for f, v in fam.items() if f != want_family) == 0, fam
    else:
        assert fam["one_wave"][0] + fam["persistent"][0] > 0, fam


@pytest.mark.parametrize("dim", [128, 100])
@pytest.mark.parametrize("metric", m.METRICS)
@pytest.mark.parametrize("bits", m.BITS)
def test_knn_search_matches_model_search(bits, metric, dim):
    """dim 128: the fixed-length instantiations (query words in registers); dim 100: the run-time loop.  L + start
    points at 64 / 65 and 128 / 129 (one, two, three queue registers per lane), W = 1 (plain mode) and 3 (general)"""
    c = MmModelCase(bits, metric, 2000, dim, 16, 200 + 16 * bits + 4 * metric + dim)
    _check_knn(c, 6, ((63, 1), (64, 3), (127, 3), (128, 1)))


@pytest.mark.parametrize("bits,dim", [(8, 128), (4, 100), (2, 128), (1, 100)])
def test_knn_search_with_unpublished_slots(bits, dim):
    """inline tags (the general mode's tag reads) on the Store's stride"""
    c = MmModelCase(bits, m.L2, 2000, dim, 16, 290 + bits, tags=True)
    tags = np.full(c.n + 1, 254, np.uint8)
    tags[c.rng.choice(c.n, 300, replace=False)] = c.rng.integers(0, 3, 300)
    tags[c.n] = 255
    c.gix.set_tags(0, tags)
    _check_knn(c, 6, ((63, 1), (64, 3)), tags=tags)


@pytest.mark.parametrize("bits", m.BITS)
def test_knn_search_on_persistent_waves(bits):
    c = MmModelCase(bits, m.IP, 2000, 128, 16, 280 + bits)
    c.gix.set_max_concurrency(4)
    _check_knn(c, 12, ((64, 1),), want_family="persistent")
    c.gix.set_max_concurrency(0)


# ---- 3. the oracle's U8 L2 twin -----------------------------------------------------------------------------------------
TWINS = [(8, 128), (8, 100), (4, 64), (2, 100), (1, 128)]


@pytest.mark.parametrize("bits,dim", TWINS)
def test_twin_searches(bits, dim):
    """Knn, range, inline-filtered, multihop, filtered-range, paged, diverse and recorded searches"""
    c = MmTwin(bits, dim, 2000, 16, 300 + bits + dim)
    q, tq = c.queries(8)
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
        cap = 1500
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
    gi, gd, gst, gsec = c.gix.filtered_range_search(q, 12, radius, match, out_cap=1500)
    for j in range(nq):
        oi, od, ost = c.oix.filtered_range_search(tq[j], 12, radius, match, out_cap=1500)
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
    slots = c.rng.choice(c.n, 12, replace=False).astype(np.uint32)
    rid, rd, rn, st = c.gix.search_record(slots, 30)  # (a stored row as the query)
    for i, s_ in enumerate(slots):
        _, _, _, ost, orid, ord_ = c.oix.search(c.codes[s_], 30, 1, 10, record=True)
        assert rn[i] == orid.size
        assert np.array_equal(rid[i, :rn[i]], orid) and np.array_equal(fbits(rd[i, :rn[i]]), fbits(ord_))
        assert st["cmps"][i] == ost[0] and st["hops"][i] == ost[1]


def _same_adjacency(gix, oix, maxdeg):
    got = gix.download_graph()
    lens = oix.adj[:, 0]
    assert np.array_equal(got[:, 0], lens)
    mask = np.arange(maxdeg)[None, :] < lens[:, None]
    assert np.array_equal(got[:, 1:][mask], oix.adj[:, 1:][mask])


@pytest.mark.parametrize("bits,dim", TWINS)
def test_twin_build(bits, dim):
    """dann_build against the oracle's multi_insert over the same batches: byte-identical adjacency"""
    from diskann_amd.sharding import batch_schedule
    n, maxdeg, pruned, lb = 1500, 16, 12, 24
    c = MmTwin(bits, dim, n, maxdeg, 400 + bits + dim, adj=False)
    ocfg = oracle.build_config(pruned, maxdeg, lb, intra_batch_candidates=oracle.IBC_NONE)
    gcfg = da.build_config(pruned, maxdeg, lb, intra_batch_candidates=da.IBC_NONE)
    growth, max_batch = 0.1, 512
    nb = c.gix.build(gcfg, 0, n, growth, max_batch)
    k = 0
    for s0, b in batch_schedule(0, n, growth, max_batch):
        c.oix.multi_insert(ocfg, np.arange(s0, s0 + b, dtype=np.uint32))
        k += 1
    assert k == nb
    _same_adjacency(c.gix, c.oix, maxdeg)


@pytest.mark.parametrize("bits,dim", [(8, 128), (8, 100), (4, 64)])
def test_twin_insert_and_prune(bits, dim):
    n, R, maxdeg = 600, 8, 10
    c = MmTwin(bits, dim, n, R, 500 + bits + dim, adj=False, maxdeg=maxdeg)
    ocfg = oracle.build_config(R, maxdeg, 24, intra_batch_candidates=oracle.IBC_NONE)
    gcfg = da.build_config(R, maxdeg, 24, intra_batch_candidates=da.IBC_NONE)
    s = 0
    for b in (1, 2, 5, 20, 72, 500):
        slots = np.arange(s, min(s + b, n), dtype=np.uint32)
        c.oix.multi_insert(ocfg, slots)
        c.gix.insert_batch(gcfg, slots)
        s += b
    _same_adjacency(c.gix, c.oix, maxdeg)
    locs = c.rng.choice(n, 12, replace=False).astype(np.uint32)
    pools, dists, off = [], [], [0]
    for i, loc in enumerate(locs):
        cnt = [0, 1, 5, 70, 200, 333][i % 6]
        ids = c.rng.choice(n, cnt, replace=False).astype(np.uint32)
        if cnt > 3:
            ids[2] = loc
        pools.append(ids)
        dists.append(np.array([oracle.distance(oracle.U8, oracle.L2, c.codes[loc], c.codes[j]) for j in ids], np.float32))
        off.append(off[-1] + cnt)
    for sat in (False, True):
        got = c.gix.prune_batch(gcfg, locs, np.concatenate(pools), np.concatenate(dists), np.array(off, np.uint64),
                                force_saturate=sat)
        for i, loc in enumerate(locs):
            want, _ = c.oix.prune_pool(ocfg, int(loc), pools[i], dists[i], force_saturate=sat)
            assert got[i, 0] == want.size and np.array_equal(got[i, 1:1 + want.size], want), (i, sat)


def _same_graph(gix, oix):
    g, o = gix.download_graph(), oix.adj.copy()
    for a in (g, o):
        for r in range(a.shape[0]):
            a[r, 1 + min(int(a[r, 0]), gix.max_degree):] = 0
    bad = np.flatnonzero((g != o).any(axis=1))
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}"


@pytest.mark.parametrize("bits,dim", TWINS)
def test_twin_consolidate(bits, dim):
    n, R = 1200, 32
    c = MmTwin(bits, dim, n, R, 600 + bits + dim)
    deleted = np.zeros(n + 1, bool)
    deleted[c.rng.choice(n, n // 10, replace=False)] = True
    c.gix.delete_points(np.flatnonzero(deleted))
    kinds, cnt = c.gix.consolidate(da.build_config(24, R, 50))
    want = consolidate(c.oix, oracle.build_config(24, R, 50), deleted)
    assert np.array_equal(kinds, want)
    _same_graph(c.gix, c.oix)
    assert cnt[0] == n + 1 and cnt[2] > 0


@pytest.mark.parametrize("bits,dim", [(8, 128), (8, 100), (1, 128)])
def test_twin_inplace_delete(bits, dim):
    n, R = 1000, 32
    c = MmTwin(bits, dim, n, R, 700 + bits + dim)
    deleted = np.zeros(n + 1, bool)
    ids = c.rng.choice(n, 16, replace=False)
    c.gix.set_prune_tie_order(da.TIE_RUST)
    got = c.gix.inplace_delete(da.build_config(24, R, 50), ids, method=da.INPLACE_TWO_HOP_AND_ONE_HOP, num_to_replace=3)
    want = inplace_delete(c.oix, oracle.build_config(24, R, 50), deleted, ids, da.INPLACE_TWO_HOP_AND_ONE_HOP, 3, TIE_RUST, 0, 0)
    assert got[:8].tolist() == want[:8].tolist(), (got, want)
    assert want[7] > 0 and want[1] > 0  # prunes ran
    _same_graph(c.gix, c.oix)
    assert np.array_equal(c.gix.get_deleted()[:n + 1], deleted.astype(np.uint8))


# ---- 4. dann_minmax_compress --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", m.BITS)
def test_compress_matches_model(bits):
    rng = np.random.default_rng(800 + bits)
    for dim in (1, 7, 64, 100, 128, 260):
        x = rng.normal(0.3, 2.0, (40, dim)).astype(np.float32)
        x[0] = 1.25                       # a constant row
        x[1] = rng.normal(0.0, 0.01, dim)
        x[1, dim // 2] = 50.0             # one outlier
        x[2] = -x[2] * 1e-3
        for grid_scale in (1.0, 0.9):
            rows, loss, nan = m.compress(x, bits, grid_scale)
            assert not nan.any()
            got, gloss = da.minmax_compress(x, bits, grid_scale, return_loss=True)
            assert got.shape == rows.shape == (40, da.lib().dann_layer_bytes(DT[bits], dim))
            bad = np.flatnonzero((got != rows).any(axis=1))
            assert bad.size == 0, (bits, dim, grid_scale, bad[:5], m.header(got[bad[:2]]), m.header(rows[bad[:2]]))
            assert np.array_equal(fbits(gloss), fbits(loss)), (bits, dim, grid_scale)
    x = np.ones((3, 9), np.float32)
    x[1, 4] = np.nan
    out = np.zeros((3, m.layer_bytes(bits, 9)), np.uint8)
    rc = da.lib().dann_minmax_compress(-1, bits, x.ctypes.data_as(C.c_void_p), 3, 9, 1.0, out.ctypes.data_as(C.c_void_p), None)
    assert rc == da._ffi.EINVAL
    assert da.lib().dann_minmax_compress(-1, 3, x.ctypes.data_as(C.c_void_p), 3, 9, 1.0, out.ctypes.data_as(C.c_void_p), None) == da._ffi.EINVAL


# ---- 5. rejections ------------------------------------------------------------------------------------------------------
def test_rejections():
    for bits in m.BITS:
        dim = 64
        start = random_rows(np.random.default_rng(bits), 1, dim, bits)
        gix = da.Provider(DT[bits], da.L2, dim, 10, 4, start)
        gix.set_query_layout(da.QUERY_SAME_AS_DATA)
        assert gix.query_bytes() == m.layer_bytes(bits, dim)
        for layout in (da.QUERY_FOUR_BIT_TRANSPOSED, da.QUERY_SCALAR_QUANTIZED, da.QUERY_FULL_PRECISION, da.QUERY_EIGHT_BIT):
            with pytest.raises(da.DannError) as e:
                gix.set_query_layout(layout)
            assert e.value.status == da._ffi.EUNSUPPORTED, (bits, layout)
        for layout in (4, 5, 6, 7, 9, -1):
            with pytest.raises(da.DannError) as e:
                gix.set_query_layout(layout)
            assert e.value.status == da._ffi.EINVAL, (bits, layout)
        h = C.c_void_p()
        q = np.zeros(m.layer_bytes(bits, dim) + 1, np.uint8)  # one byte too long
        q[:start.shape[1]] = start[0]
        assert da.lib().dann_query_create(gix._h, q.ctypes.data_as(C.c_void_p), q.nbytes, C.byref(h)) == da._ffi.ELENGTH
        assert da.lib().dann_query_create(gix._h, q.ctypes.data_as(C.c_void_p), q.nbytes - 1, C.byref(h)) == 0
        da.lib().dann_query_destroy(h)
        # the header's dim through the host-pointer writers
        bad = start.copy()
        bad[0, :4] = np.array([dim + 1], np.uint32).view(np.uint8)
        with pytest.raises(da.DannError) as e:
            gix.set_element(3, bad[0])
        assert e.value.status == da._ffi.EINVAL
        assert da.lib().dann_query_create(gix._h, bad.ctypes.data_as(C.c_void_p), bad.nbytes, C.byref(h)) == da._ffi.EINVAL
        with pytest.raises(da.DannError) as e:
            da.Provider(DT[bits], da.L2, dim, 10, 4, bad)
        assert e.value.status == da._ffi.EINVAL
        gix.set_element(3, start[0])
        assert np.array_equal(gix.get_element(3), start[0])
        gix.close()
    # dim * (2^bits - 1)^2 must fit a u32
    top = (1 << 32) // (255 * 255)
    with pytest.raises(da.DannError) as e:
        da.Provider(da.MM8, da.L2, top + 1, 4, 4, np.zeros((1, m.layer_bytes(8, top + 1)), np.uint8))
    assert e.value.status == da._ffi.EINVAL
    assert da.lib().dann_layer_bytes(7, 4) == da._ffi.EINVAL and da.lib().dann_layer_bytes(48, 4) == da._ffi.EINVAL
    assert da.lib().dann_layer_bytes(da.MM2, 9) == 23 and da.lib().dann_inmem2_row_stride(da.MM8, 128) == 160
    # foreign indexes: 8 is a known layout they do not have, 4 .. 7 are no layouts
    f = da.Provider(da.F32, da.L2, 8, 10, 4, np.zeros((1, 8), np.float32))
    with pytest.raises(da.DannError) as e:
        f.set_query_layout(da.QUERY_EIGHT_BIT)
    assert e.value.status == da._ffi.EUNSUPPORTED
    s = da.Provider(da.SPH1, da.L2, 64, 10, 4, np.zeros((1, 14), np.uint8))
    with pytest.raises(da.DannError) as e:
        s.set_query_layout(da.QUERY_EIGHT_BIT)
    assert e.value.status == da._ffi.EUNSUPPORTED
    for layout in (4, 7):
        with pytest.raises(da.DannError) as e:
            s.set_query_layout(layout)
        assert e.value.status == da._ffi.EINVAL


def test_search_server_keeps_its_16_byte_rule():
    """an MM8 query at 128-d is 148 bytes and is refused like SQ-8's 132"""
    start = random_rows(np.random.default_rng(81), 1, 128, 8)
    gix = da.Provider(da.MM8, da.L2, 128, 10, 4, start)
    with pytest.raises(da.DannError) as e:
        gix.server_start(32, 10, workers=8)
    assert e.value.status == da._ffi.EUNSUPPORTED and gix.query_bytes() == 148


# ---- 6. save and load of vectors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", m.BITS)
def test_save_and_load_vectors(bits, tmp_path):
    rng = np.random.default_rng(900 + bits)
    dim, n = 100, 120
    rows = random_rows(rng, n + 1, dim, bits)
    gix = da.Provider(DT[bits], da.L2, dim, n, 4, rows[n:])
    gix.set_elements(0, rows[:n])
    path = tmp_path / "rows.bin"
    gix.save_vectors_bin(path, 0, 100)
    raw = np.fromfile(path, np.uint8)
    assert raw[:8].view(np.uint32).tolist() == [100, m.layer_bytes(bits, dim)]
    assert np.array_equal(raw[8:].reshape(100, -1), rows[:100])
    other = da.Provider(DT[bits], da.L2, dim, 100, 4, rows[n:])
    assert other.load_vectors_bin(path) == 100
    assert all(np.array_equal(other.get_element(i), rows[i]) for i in range(100))
