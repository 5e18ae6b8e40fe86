"""Spherically quantised rows (SPH1 / SPH2 / SPH4) on the GPU.  Everything is compared bit for bit: distances and Knn
searches against the CPU model (tests/spherical_model.py: random codes and metadata, every query layout and metric),
every other search kind, the build and the graph mutations against the oracle's U8 L2 twin over flat rows (rows whose
L2 is exactly the squared distance of their codes, see the model)."""
import ctypes as C

import numpy as np
import pytest

import oracle
import spherical_model as m
from consolidate_model import consolidate
from diverse_model import diverse_search
from helpers import bits as fbits
from inplace_delete_model import TIE_RUST, inplace_delete
from search_builders import SphModelCase as ModelCase, SphTwin as Twin

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

DT = {1: da.SPH1, 2: da.SPH2, 4: da.SPH4}
LAYOUTS = {1: (m.SAME_AS_DATA, m.FOUR_BIT_TRANSPOSED), 2: (m.SAME_AS_DATA, m.SCALAR_QUANTIZED),
           4: (m.SAME_AS_DATA, m.SCALAR_QUANTIZED)}
METRICS = (m.L2, m.IP, m.COSINE)
# the seams of the gather: a lane reads one dword (1 bit), two (2 bit) or four (4 bit) per step -- 32 dimensions --, a
# 4-lane group 128; a transposed query block is 64 dimensions; the metadata sits at an odd byte for dim 1 .. 8 at 1 bit
DIMS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 260)


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


def _f16_meta(rng, n):
    return m.data_meta_bytes(rng.normal(0.0, 3.0, n).astype(np.float32), rng.normal(0.0, 3.0, n).astype(np.float32),
                             rng.integers(0, 65536, n))


def _random_rows(rng, n, dim, bits, garbage=False):
    rows = np.zeros((n, m.layer_bytes(bits, dim)), np.uint8)
    cb = m.code_bytes(bits, dim)
    rows[:, :cb] = m.pack(rng.integers(0, 1 << bits, (n, dim), dtype=np.uint8), bits)
    rows[:, cb:] = _f16_meta(rng, n)
    if garbage:  # random bits in the padding of the last code byte
        used = dim * bits - 8 * (cb - 1)
        if used < 8:
            rows[:, cb - 1] |= (rng.integers(0, 256, n, dtype=np.uint8) << used).astype(np.uint8)
    return rows


def _random_queries(rng, n, dim, bits, layout, garbage=False):
    if layout == m.SAME_AS_DATA:
        return _random_rows(rng, n, dim, bits, garbage)
    meta = rng.normal(0.0, 3.0, (n, 4)).astype(np.float32).view(np.uint8).reshape(n, 16)
    if layout == m.SCALAR_QUANTIZED:
        return np.concatenate([_random_rows(rng, n, dim, bits, garbage)[:, :m.code_bytes(bits, dim)], meta], axis=1)
    values = rng.integers(0, 16, (n, dim), dtype=np.uint8)
    if garbage and dim % 64:  # the padding lanes of the last block hold anything
        wide = rng.integers(0, 16, (n, (dim + 63) // 64 * 64), dtype=np.uint8)
        wide[:, :dim] = values
        planes = m.transpose4(wide)
    else:
        planes = m.transpose4(values)
    return np.concatenate([planes, meta], axis=1)


# ---- 1. distances -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["packed", "store", "garbage"])
@pytest.mark.parametrize("bits", [1, 2, 4])
def test_distances_match_model(bits, variant):
    """dann_distance_pairs, dann_query_distance, dann_expand_beam_batch (ragged, one empty list) and dann_rerank_batch.
    store: the Store stride with inline tags and random bytes from the tag byte to the stride"""
    rng = np.random.default_rng(100 + 10 * bits + len(variant))
    n, nq = 64, 8
    garbage = variant == "garbage"
    for dim in DIMS:
        rows = _random_rows(rng, n + 1, dim, bits, garbage)
        a, b = rng.integers(0, n, 24).astype(np.uint32), rng.integers(0, n, 24).astype(np.uint32)
        lens = rng.integers(1, n, nq)
        lens[3] = 0
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        ids = np.concatenate([rng.choice(n, l, replace=False) for l in lens]).astype(np.uint32)
        cand = np.stack([rng.permutation(n)[:40] for _ in range(nq)]).astype(np.uint32)
        cand[:, 5] = 0xFFFFFFFF
        stride = da.lib().dann_inmem2_row_stride(DT[bits], dim) if variant == "store" else 0
        for metric in METRICS:
            ssn = float(np.float32(rng.uniform(0.0, 9.0)))
            gix = da.Provider(DT[bits], metric, dim, n, 4, rows[n:], sq_shift_norm_sq=ssn, row_stride=stride,
                              inline_tags=variant == "store")
            gix.set_elements(0, rows[:n])
            if variant == "store":
                assert stride == m.store_stride(bits, dim)
                raw = rng.integers(0, 256, (n + 1, stride), dtype=np.uint8)
                raw[:, :rows.shape[1]] = rows
                raw[:, rows.shape[1]] = gix.get_tags(0, n + 1)
                _overwrite_store(gix, raw)
            want = m.distance_matrix(metric, rows[a], rows[b], dim, bits, m.SAME_AS_DATA, ssn)[np.arange(24), np.arange(24)]
            assert np.array_equal(fbits(gix.distance_pairs(a, b)), fbits(want)), (bits, dim, metric, "pairs")
            for layout in LAYOUTS[bits]:
                gix.set_query_layout(layout)
                assert gix.query_layout() == layout and gix.query_bytes() == m.query_bytes(bits, dim, layout)
                q = _random_queries(rng, nq, dim, bits, layout, garbage)
                D = m.distance_matrix(metric, q, rows[:n], dim, bits, layout, ssn)
                tag = (bits, dim, metric, layout)
                got = gix.expand_beam_batch(q, ids, off)
                want = np.concatenate([D[j, ids[int(off[j]):int(off[j + 1])]] for j in range(nq)])
                assert np.array_equal(fbits(got), fbits(want)), tag + ("expand_beam_batch",)
                for j in (0, nq - 1):
                    d = np.float32(gix.query_distance(q[j], rows[j + 2]))
                    assert fbits(d) == fbits(D[j, j + 2]), tag + ("query_distance",)
                gi, gd = gix.rerank(q, cand, 12)
                for j in range(nq):
                    c = [int(x) for x in cand[j] if x != 0xFFFFFFFF]
                    dd = D[j, c]
                    key = fbits(dd + np.float32(0.0)).astype(np.int64)
                    key = np.where(key & 0x80000000, ~key & 0xFFFFFFFF, key | 0x80000000)
                    order = np.lexsort((np.arange(len(c)), key))[:12]
                    assert [c[i] for i in order] == gi[j].tolist(), tag + ("rerank", j)
                    assert np.array_equal(fbits(dd[order]), fbits(gd[j])), tag + ("rerank", j)
            gix.close()


# ---- 2. Knn search against the model's search ---------------------------------------------------------------------------
KNN_CASES = ([(1, lay, metric) for lay in LAYOUTS[1] for metric in METRICS] +
             [(b, lay, m.L2) for b in (2, 4) for lay in LAYOUTS[b]] + [(2, m.SCALAR_QUANTIZED, m.IP), (4, m.SAME_AS_DATA, m.IP)])


def _check_knn(c, layout, nq, tags=None):
    q = c.qz.queries(c.rng.normal(0.2, 1.0, (nq, c.dim)).astype(np.float32), layout)
    c.gix.set_query_layout(layout)
    D = m.distance_matrix(c.metric, q, c.all_rows, c.dim, c.bits, layout, c.qz.ssn)
    readable = None if tags is None else tags >= 254
    k = 10
    dq = DevBuf(q.nbytes, q)
    c.gix.kernel_time_reset()
    for L in (10, 32):
        for W in (1, 2):
            gi, gd, gst = c.gix.search(da.Knn(L, W), q, k)  # host pointers
            di, dd, ds = DevBuf(nq * k * 4), DevBuf(nq * k * 4), DevBuf(nq * 20)
            da._ffi.check(da.lib().dann_search_batch_device(c.gix._h, dq.p, nq, L, W, k, di.p, dd.p, ds.p),
                          "dann_search_batch_device")
            hi, hd = di.get(np.uint32, (nq, k)), dd.get(np.float32, (nq, k))
            hst = ds.get(np.uint8, (nq * 20,)).view(da.STATS_DTYPE)
            for j in range(nq):
                ids, d, cmps, hops, written = m.knn_search(lambda i: D[j, i], c.adj, c.n, 1, c.R, L, W, k, readable)
                tag = (c.bits, c.dim, c.metric, layout, L, W, j)
                assert np.array_equal(gi[j], ids) and np.array_equal(fbits(gd[j]), fbits(d)), tag
                assert (int(gst["cmps"][j]), int(gst["hops"][j]), int(gst["written"][j])) == (cmps, hops, written), tag
                assert np.array_equal(hi[j], ids) and np.array_equal(fbits(hd[j]), fbits(d)), tag + ("device",)
                assert (int(hst["cmps"][j]), int(hst["hops"][j]), int(hst["written"][j])) == (cmps, hops, written), tag
    fam = c.gix.search_families()
    assert fam["team"][0] == 0 and fam["pair"][0] == 0, fam
    assert fam["one_wave"][0] + fam["persistent"][0] > 0, fam


@pytest.mark.parametrize("dim", [128, 100])
@pytest.mark.parametrize("bits,layout,metric", KNN_CASES)
def test_knn_search_matches_model_search(bits, layout, metric, dim):
    """dim 128: the fixed-length instantiations (query words in registers); dim 100: the run-time loop"""
    c = ModelCase(bits, metric, 2000, dim, 16, 200 + 16 * bits + 4 * layout + metric + dim)
    _check_knn(c, layout, 64)


def test_knn_search_with_unpublished_slots():
    c = ModelCase(1, m.L2, 2000, 128, 16, 290, tags=True)
    tags = np.full(c.n + 1, 254, np.uint8)
    tags[c.rng.choice(c.n, 300, replace=False)] = c.rng.integers(0, 3, 300)
    tags[c.n] = 255
    c.gix.set_tags(0, tags)
    _check_knn(c, m.FOUR_BIT_TRANSPOSED, 32, tags=tags)


# ---- 3. the oracle's U8 L2 twin over flat rows --------------------------------------------------------------------------
TWINS = [(1, 128), (1, 100), (2, 64), (4, 32)]


@pytest.mark.parametrize("bits,dim", TWINS)
def test_twin_searches(bits, dim):
    """Knn, range, inline-filtered, multihop, filtered-range, paged and diverse searches"""
    c = Twin(bits, dim, 2000, 16, 300 + bits + dim)
    q, tq = c.queries(12)
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


def _same_adjacency(gix, oix, maxdeg):
    got = gix.download_graph()
    lens = oix.adj[:, 0]
    assert np.array_equal(got[:, 0], lens)
    mask = np.arange(maxdeg)[None, :] < lens[:, None]
    assert np.array_equal(got[:, 1:][mask], oix.adj[:, 1:][mask])


@pytest.mark.parametrize("bits,dim", TWINS)
def test_twin_build(bits, dim):
    """dann_build against the oracle's multi_insert over the same batches: code distances tie heavily (Hamming distances
    at 1 bit), which exercises the default tie order"""
    from diskann_amd.sharding import batch_schedule
    n, maxdeg, pruned, lb = 1500, 16, 12, 24
    c = Twin(bits, dim, n, maxdeg, 400 + bits + dim, adj=False)
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


@pytest.mark.parametrize("bits,dim", TWINS)
def test_twin_insert_and_prune(bits, dim):
    n, R, maxdeg = 600, 8, 10
    c = Twin(bits, dim, n, R, 500 + bits + dim, adj=False, maxdeg=maxdeg)
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
    c = Twin(bits, dim, n, R, 600 + bits + dim)
    deleted = np.zeros(n + 1, bool)
    deleted[c.rng.choice(n, n // 10, replace=False)] = True
    c.gix.delete_points(np.flatnonzero(deleted))
    kinds, cnt = c.gix.consolidate(da.build_config(24, R, 50))
    want = consolidate(c.oix, oracle.build_config(24, R, 50), deleted)
    assert np.array_equal(kinds, want)
    _same_graph(c.gix, c.oix)
    assert cnt[0] == n + 1 and cnt[2] > 0


@pytest.mark.parametrize("bits,dim", TWINS)
def test_twin_inplace_delete(bits, dim):
    n, R = 1000, 32
    c = Twin(bits, dim, n, R, 700 + bits + dim)
    deleted = np.zeros(n + 1, bool)
    ids = c.rng.choice(n, 16, replace=False)
    c.gix.set_prune_tie_order(da.TIE_RUST)
    got = c.gix.inplace_delete(da.build_config(24, R, 50), ids, method=da.INPLACE_TWO_HOP_AND_ONE_HOP, num_to_replace=3)
    want = inplace_delete(c.oix, oracle.build_config(24, R, 50), deleted, ids, da.INPLACE_TWO_HOP_AND_ONE_HOP, 3, TIE_RUST, 0, 0)
    assert got[:8].tolist() == want[:8].tolist(), (got, want)
    assert want[7] > 0 and want[1] > 0  # prunes ran
    _same_graph(c.gix, c.oix)
    assert np.array_equal(c.gix.get_deleted()[:n + 1], deleted.astype(np.uint8))


# ---- 4. the search server -----------------------------------------------------------------------------------------------
def test_search_server_transposed_queries():
    """the resident server stages queries in 16-byte units: the transposed layout at 128 dimensions is 64 + 16 = 80
    bytes and is served; the row image (16 + 6 = 22 bytes) is refused by that rule"""
    c = ModelCase(1, m.L2, 2000, 128, 16, 800)
    L, k, nq = 32, 10, 24
    with pytest.raises(da.DannError) as e:
        c.gix.server_start(L, k, workers=32)
    assert e.value.status == da._ffi.EUNSUPPORTED and c.gix.query_bytes() == 22
    c.gix.set_query_layout(m.FOUR_BIT_TRANSPOSED)
    assert c.gix.query_bytes() == 80
    q = c.qz.queries(c.rng.normal(0.2, 1.0, (nq, 128)).astype(np.float32), m.FOUR_BIT_TRANSPOSED)
    bi, bd, bst = c.gix.search(da.Knn(L), q, k)
    c.gix.server_start(L, k, workers=32)
    try:
        with pytest.raises(da.DannError) as e:
            c.gix.set_query_layout(m.SAME_AS_DATA)
        assert e.value.status == da._ffi.EBUSY
        tickets = [c.gix.submit(q[i]) for i in range(nq)]
        for i, t in enumerate(tickets):
            ids, d, st = c.gix.wait(t)
            assert np.array_equal(ids, bi[i]) and np.array_equal(fbits(d), fbits(bd[i])), i
            assert (int(st["cmps"]), int(st["hops"])) == (int(bst["cmps"][i]), int(bst["hops"][i])), i
    finally:
        c.gix.server_stop()
    c.gix.set_query_layout(m.SAME_AS_DATA)


# ---- 5. rejections ------------------------------------------------------------------------------------------------------
def test_rejections():
    for bits in (1, 2, 4):
        dim = 64
        gix = da.Provider(DT[bits], da.L2, dim, 10, 4, np.zeros((1, m.layer_bytes(bits, dim)), np.uint8))
        for layout in (m.SAME_AS_DATA, m.FOUR_BIT_TRANSPOSED, m.SCALAR_QUANTIZED, m.FULL_PRECISION):
            if layout in LAYOUTS[bits]:
                gix.set_query_layout(layout)
                h = C.c_void_p()
                q = np.zeros(m.query_bytes(bits, dim, layout) + 1, np.uint8)  # one byte too long
                assert da.lib().dann_query_create(gix._h, q.ctypes.data_as(C.c_void_p), q.nbytes, C.byref(h)) == da._ffi.ELENGTH
                assert da.lib().dann_query_create(gix._h, q.ctypes.data_as(C.c_void_p), q.nbytes - 1, C.byref(h)) == 0
                da.lib().dann_query_destroy(h)
            else:
                with pytest.raises(da.DannError) as e:
                    gix.set_query_layout(layout)
                assert e.value.status == da._ffi.EUNSUPPORTED, (bits, layout)
        with pytest.raises(da.DannError) as e:
            gix.set_query_layout(4)
        assert e.value.status == da._ffi.EINVAL
        gix.close()
    f = da.Provider(da.F32, da.L2, 8, 10, 4, np.zeros((1, 8), np.float32))
    f.set_query_layout(m.SAME_AS_DATA)
    with pytest.raises(da.DannError) as e:
        f.set_query_layout(m.SCALAR_QUANTIZED)
    assert e.value.status == da._ffi.EUNSUPPORTED and f.query_bytes() == 32


# ---- 6. save and load of vectors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 2, 4])
def test_save_and_load_vectors(bits, tmp_path):
    rng = np.random.default_rng(900 + bits)
    dim, n = 100, 120
    rows = _random_rows(rng, n + 1, dim, bits)
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
