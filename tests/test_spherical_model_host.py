"""The CPU model of the spherical rows (tests/spherical_model.py): its Knn search pinned to the oracle's, its transposed
inner product to the dense one, its flat rows to the oracle's u8 L2, and the layout the library reports.  No GPU."""
import numpy as np
import pytest

import oracle
import spherical_model as m
from helpers import bits as fbits, random_graph

SHAPES = ((1, 128), (1, 100), (1, 8), (2, 64), (2, 128), (4, 32))


def test_pack_and_transpose_round_trip():
    rng = np.random.default_rng(1)
    assert m.pack(np.array([1, 2, 3, 4], np.uint8), 4).tolist() == [0x21, 0x43]
    assert m.pack(np.array([1, 2, 3, 0, 3], np.uint8), 2).tolist() == [0b00111001, 0b11]
    assert m.pack(np.array([1, 0, 0, 1, 0, 0, 0, 0, 1], np.uint8), 1).tolist() == [0x09, 0x01]
    for bits in (1, 2, 4):
        for dim in (1, 7, 8, 9, 33, 130):
            c = rng.integers(0, 1 << bits, (5, dim), dtype=np.uint8)
            p = m.pack(c, bits)
            assert p.shape == (5, m.code_bytes(bits, dim)) and np.array_equal(m.unpack(p, bits, dim), c)
    v = rng.integers(0, 16, (3, 70), dtype=np.uint8)
    t = m.transpose4(v)
    assert t.shape == (3, 64) and np.array_equal(m.untranspose4(t, 70), v)
    one = np.zeros(64, np.uint8)
    one[5] = 0b0110  # element 5: bits 1 and 2 -> bit 5 of words 1 and 2
    w = m.transpose4(one).view(np.uint64)
    assert w.tolist() == [0, 1 << 5, 1 << 5, 0]


def test_model_search_is_the_oracle_search():
    """integer-lattice f32 rows, so that distances tie: ids, distance bits, cmps and hops"""
    rng = np.random.default_rng(2)
    n, dim, R, nq, k = 500, 16, 8, 12, 10
    data = rng.integers(-2, 3, (n, dim)).astype(np.float32)
    start = rng.integers(-2, 3, (1, dim)).astype(np.float32)
    adj = random_graph(rng, n, R)
    oix = oracle.Index(oracle.F32, oracle.L2, dim, n, R, start)
    oix.set_rows(0, data)
    oix.adj[:] = adj
    rows = np.concatenate([data, start])
    queries = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
    for L in (5, 20):
        for W in (1, 3):
            oi, od, oc, ost = oix.search_batch(queries, L, W, k)
            for j in range(nq):
                ids, d, cmps, hops, written = m.knn_search(
                    lambda i: oracle.query_distance(oracle.F32, oracle.L2, queries[j], rows[i]), adj, n, 1, R, L, W, k)
                assert np.array_equal(ids, oi[j]) and np.array_equal(fbits(d), fbits(od[j])), (L, W, j)
                assert (cmps, hops, written) == (int(ost[j, 0]), int(ost[j, 1]), int(oc[j])), (L, W, j)


def test_transposed_inner_product_is_the_dense_one():
    rng = np.random.default_rng(3)
    for dim in range(1, 131):
        q4 = rng.integers(0, 16, dim, dtype=np.uint8)
        y = m.pack(rng.integers(0, 2, dim, dtype=np.uint8), 1)
        want = m.ip_dense(m.pack(q4, 4), y, 4, 1, dim)
        planes = m.transpose4(q4)
        assert m.ip_transposed(planes, y, dim) == want, dim
        # the query's padding lanes and the row's padding bits may hold anything
        noisy = np.unpackbits(planes, bitorder="little").reshape(-1, 4, 64)
        e = dim % 64
        if e:
            noisy[-1, :, e:] = rng.integers(0, 2, (4, 64 - e))
        yn = y.copy()
        if dim % 8:
            yn[-1] |= (0xFF << (dim % 8)) & 0xFF
        assert m.ip_transposed(np.packbits(noisy.reshape(-1), bitorder="little"), yn, dim) == want, dim


@pytest.mark.parametrize("bits,dim", SHAPES)
def test_flat_rows_are_the_u8_l2(bits, dim):
    rng = np.random.default_rng(4 + bits + dim)
    codes = rng.integers(0, 1 << bits, (200, dim), dtype=np.uint8)
    rows = m.flat_rows(codes, bits)
    for i in range(0, 200, 2):
        got = m.distance_rows(m.L2, rows[i], rows[i + 1], dim, bits)
        want = np.float32(oracle.distance(oracle.U8, oracle.L2, codes[i], codes[i + 1]))
        assert got.view(np.uint32) == want.view(np.uint32), (bits, dim, i)
        assert float(got) == float(((codes[i].astype(np.int64) - codes[i + 1]) ** 2).sum())


def test_scalar_query_with_matching_meta_is_the_row_form():
    """a QueryMeta with offset = -off, bit_sum = sum(code) and correction 1 restates a flat row: the query form then
    computes <x - off, y - off> in another association, which on flat data (every step exact) gives the same bits"""
    rng = np.random.default_rng(5)
    for bits, dim in ((2, 64), (4, 32)):
        codes = rng.integers(0, 1 << bits, (20, dim), dtype=np.uint8)
        rows = m.flat_rows(codes, bits)
        cb = m.code_bytes(bits, dim)
        off = float(m.offset(bits))
        for i in range(0, 20, 2):
            ms = float(((codes[i].astype(np.float64) - off) ** 2).sum())
            # c = ip - off * qsum + qoff * sy - off * qoff * D with qoff = -off: <x - off, y - off>
            q = np.concatenate([rows[i, :cb], m.query_meta_bytes(np.float32(1), np.float32(codes[i].sum()),
                                                                 np.float32(-off), np.float32(ms))[0]])
            a = m.distance_query(m.L2, q, rows[i + 1], dim, bits, m.SCALAR_QUANTIZED)
            b = m.distance_rows(m.L2, rows[i], rows[i + 1], dim, bits)
            assert a.view(np.uint32) == b.view(np.uint32)


def test_layout_helpers():
    import diskann_amd as da
    L = da.lib()
    assert (da.SPH1, da.SPH2, da.SPH4) == (33, 34, 36)
    for bits, dt in ((1, da.SPH1), (2, da.SPH2), (4, da.SPH4)):
        for dim in (1, 8, 9, 128):
            assert L.dann_layer_bytes(dt, dim) == m.layer_bytes(bits, dim), (bits, dim)
            assert L.dann_inmem2_row_stride(dt, dim) == m.store_stride(bits, dim), (bits, dim)
    assert L.dann_layer_bytes(da.SPH1, 8) == 7 and L.dann_inmem2_row_stride(da.SPH1, 8) == 32
    assert L.dann_layer_bytes(da.SPH4, 128) == 70 and L.dann_inmem2_row_stride(da.SPH4, 128) == 96
    for bad in (6, 7, 16, 24, 32 + 3):
        assert L.dann_layer_bytes(bad, 4) == da._ffi.EINVAL, bad
    # bit_sum is a u16: dim * (2^bits - 1) <= 65535
    for bits, dt in ((1, da.SPH1), (2, da.SPH2), (4, da.SPH4)):
        dim = 65535 // ((1 << bits) - 1) + 1
        with pytest.raises(da.DannError) as e:
            da.Provider(dt, da.L2, dim, 4, 4, np.zeros((1, m.layer_bytes(bits, dim)), np.uint8))
        assert e.value.status == da._ffi.EINVAL, bits
    with pytest.raises(da.DannError) as e:  # SupportedMetric has no CosineNormalized
        da.Provider(da.SPH1, da.COSINE_NORMALIZED, 16, 4, 4, np.zeros((1, m.layer_bytes(1, 16)), np.uint8))
    assert e.value.status == da._ffi.EINVAL
