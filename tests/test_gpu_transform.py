"""The quantisers' transforms on the GPU (dann_transform_*, dann_minmax_quantize(_device)), bit for bit against the CPU
model (tests/transform_model.py: the reference's x86-64 V3 order) unless a test says otherwise.  67 rows throughout: the
last wavefront is partial whatever the rows per wavefront."""
import ctypes as C

import numpy as np
import pytest

import minmax_model as mm
import transform_model as tm
from helpers import bits as fbits, random_graph

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

N = 67
DT = {1: da.MM1, 2: da.MM2, 4: da.MM4, 8: da.MM8}


def signs(rng, n):
    return (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)).astype(np.uint32)


def rows(rng, dim, n=N):
    """standard normal, and one row each of zeros, of -0.0, one-hot and of denormals; no NaN, no infinity"""
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[3] = 0.0
    x[10] = -0.0
    x[17] = 0.0
    x[17, dim // 3] = 1.0
    x[n - 1] = (rng.standard_normal(dim) * 1e-40).astype(np.float32)
    assert np.isfinite(x).all() and (np.abs(x[n - 1]) < 1.17e-38).all()
    return x


def same(got, want, tag=None):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, tag
    bad = np.argwhere(fbits(got) != fbits(want))
    assert bad.size == 0, (tag, len(bad), bad[:4].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:4]])


def subsample(rng, universe, count):
    return np.sort(rng.choice(universe, count, replace=False)).astype(np.uint32)


@pytest.mark.parametrize("n", [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 4096, 16384])
def test_hadamard(n):
    x = rows(np.random.default_rng(n), n)
    t = da.Transform.padding_hadamard(np.zeros(n, np.uint32), n)
    assert (t.input_dim, t.output_dim) == (n, n)
    got = t.apply(x)
    same(got, tm.hadamard_v3(x), n)
    if n >= 64:  # the order is the micro kernel's: the plain butterflies give other last bits
        assert 2 * int((fbits(got) != fbits(tm.hadamard_plain(x))).sum()) > (N - 4) * n
    t.close()


@pytest.mark.parametrize("dim", [1, 5, 63, 64, 65, 100, 128, 129, 768])
@pytest.mark.parametrize("sub", [False, True])
def test_padding_hadamard(dim, sub):
    rng = np.random.default_rng(dim * 2 + sub)
    padded = 1 << (dim - 1).bit_length()
    s = signs(rng, dim)
    idx = subsample(rng, padded, dim) if sub else None
    x = rows(rng, dim)
    t = da.Transform.padding_hadamard(s, padded, idx)
    assert (t.input_dim, t.output_dim) == (dim, dim if sub else padded)
    same(t.apply(x), tm.padding_hadamard(x, s, padded, idx), (dim, sub))


# (input_dim, output_dim): equal (64, 128: the intermediate length is a power of two, both transforms run; 65, 129, 100
# ..: the second window starts at an offset that is no multiple of eight), larger (zero padding), smaller (subsample)
DOUBLE = [(d, d) for d in (1, 2, 3, 5, 63, 64, 65, 96, 100, 128, 129, 200, 768, 1000)] + [
    (100, 128), (100, 150), (768, 512), (100, 64)]


@pytest.mark.parametrize("dim,out", DOUBLE)
def test_double_hadamard(dim, out):
    rng = np.random.default_rng(dim * 1000 + out)
    s0, s1 = signs(rng, dim), signs(rng, max(dim, out))
    idx = subsample(rng, dim, out) if out < dim else None
    x = rows(rng, dim)
    t = da.Transform.double_hadamard(s0, s1, idx)
    assert (t.input_dim, t.output_dim) == (dim, out)
    same(t.apply(x), tm.double_hadamard(x, s0, s1, idx), (dim, out))


def test_null_transform():
    x = rows(np.random.default_rng(5), 37)
    t = da.Transform.null(37)
    assert (t.input_dim, t.output_dim) == (37, 37)
    same(t.apply(x), x)


def _cases(rng):
    """(name, transform, model of it): the register kernel with vector and with scalar accesses, and the LDS kernel"""
    s128, s100, s1 = signs(rng, 128), signs(rng, 100), signs(rng, 100)
    return [("padding128", da.Transform.padding_hadamard(s128, 128), lambda x: tm.padding_hadamard(x, s128, 128)),
            ("padding100", da.Transform.padding_hadamard(s100, 128), lambda x: tm.padding_hadamard(x, s100, 128)),
            ("double100", da.Transform.double_hadamard(s100, s1), lambda x: tm.double_hadamard(x, s100, s1)),
            ("null", da.Transform.null(100), tm.null)]


@pytest.mark.parametrize("pad", [(3, 5), (4, 8)])  # rows that lose / keep their 16-byte alignment
def test_apply_device_with_strides(pad):
    import torch
    rng = np.random.default_rng(11)
    for name, t, model in _cases(rng):
        xs, os_ = t.input_dim + pad[0], t.output_dim + pad[1]
        x = rows(rng, t.input_dim)
        hx = np.full((N, xs), np.nan, np.float32)
        hx[:, :t.input_dim] = x
        dx = torch.from_numpy(hx).cuda()
        dout = torch.full((N, os_), -77.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t.apply_device(dx.data_ptr(), N, dout.data_ptr(), xs, os_)
        got = dout.cpu().numpy()
        same(np.ascontiguousarray(got[:, :t.output_dim]), t.apply(x), name)
        same(np.ascontiguousarray(got[:, :t.output_dim]), model(x), name)
        assert (got[:, t.output_dim:] == -77.0).all(), name  # the floats between the rows are not written
        with pytest.raises(da.DannError) as e:
            t.apply_device(dx.data_ptr(), N, dout.data_ptr(), t.input_dim - 1, os_)
        assert e.value.status == da._ffi.EINVAL


def _quantizers(rng):
    s0, s1 = signs(rng, 100), signs(rng, 100)
    return [(da.Transform.padding_hadamard(s0, 128), lambda x: tm.padding_hadamard(x, s0, 128)),
            (da.Transform.double_hadamard(s0, s1), lambda x: tm.double_hadamard(x, s0, s1))]


@pytest.mark.parametrize("bits", [1, 2, 4, 8])
@pytest.mark.parametrize("grid_scale", [1.0, 0.9])
def test_minmax_quantize(bits, grid_scale):
    import torch
    rng = np.random.default_rng(bits)
    for t, model in _quantizers(rng):
        x = rng.normal(0.2, 1.0, (N, 100)).astype(np.float32)
        y = model(x)
        want, wloss, nan = mm.compress(y, bits, grid_scale)
        assert not nan.any()
        got, gloss = da.minmax_quantize(t, x, bits, grid_scale, return_loss=True)
        assert got.shape == (N, mm.layer_bytes(bits, t.output_dim)) and np.array_equal(got, want)
        assert np.array_equal(fbits(gloss), fbits(wloss))
        old, oloss = da.minmax_compress(y, bits, grid_scale, return_loss=True)  # the entry point without a transform
        assert np.array_equal(got, old) and np.array_equal(fbits(gloss), fbits(oloss))
        # device form, images 7 bytes apart from each other: the bytes between them keep what they held
        lb = got.shape[1]
        dx = torch.from_numpy(x).cuda()
        dimg = torch.full((N, lb + 7), 0xA5, dtype=torch.uint8, device="cuda")
        dloss = torch.zeros(N, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        da.minmax_quantize_device(t, dx.data_ptr(), N, bits, dimg.data_ptr(), grid_scale, out_stride=lb + 7,
                                  loss_ptr=dloss.data_ptr())
        himg = dimg.cpu().numpy()
        assert np.array_equal(himg[:, :lb], want) and (himg[:, lb:] == 0xA5).all()
        assert np.array_equal(fbits(dloss.cpu().numpy()), fbits(wloss))
        bad = x.copy()
        bad[5, 40] = np.nan
        with pytest.raises(da.DannError) as e:
            da.minmax_quantize(t, bad, bits, grid_scale)
        assert e.value.status == da._ffi.EINVAL and "NaN" in str(e.value)


@pytest.mark.parametrize("bits", [4, 8])
def test_end_to_end_on_the_device(bits):
    """f32 rows and queries that live on the device become an MM index and its queries without touching the host"""
    import torch
    n, dim, R, nq, k = 2000, 100, 16, 24, 10
    rng = np.random.default_rng(40 + bits)
    s0, s1 = signs(rng, dim), signs(rng, dim)
    data = rng.normal(0.2, 1.0, (n + 1, dim)).astype(np.float32)
    queries = rng.normal(0.2, 1.0, (nq, dim)).astype(np.float32)
    adj = random_graph(rng, n, R)
    # the host route: model transform -> dann_minmax_compress -> dann_set_elements, host queries
    himg = da.minmax_compress(tm.double_hadamard(data, s0, s1), bits, 0.95)
    hq = da.minmax_compress(tm.double_hadamard(queries, s0, s1), bits, 0.95)
    host = da.Provider(DT[bits], da.L2, dim, n, R, himg[n:])
    host.set_elements(0, himg[:n])
    host.upload_graph(adj)
    # the device route
    t = da.Transform.double_hadamard(s0, s1)
    lb = himg.shape[1]
    ddata, dqueries = torch.from_numpy(data[:n]).cuda(), torch.from_numpy(queries).cuda()
    dimg = torch.empty((n, lb), dtype=torch.uint8, device="cuda")
    dq = torch.empty((nq, lb), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    da.minmax_quantize_device(t, ddata.data_ptr(), n, bits, dimg.data_ptr(), 0.95)
    da.minmax_quantize_device(t, dqueries.data_ptr(), nq, bits, dq.data_ptr(), 0.95)
    assert np.array_equal(dimg.cpu().numpy(), himg[:n]) and np.array_equal(dq.cpu().numpy(), hq)
    dev = da.Provider(DT[bits], da.L2, dim, n, R, himg[n:])
    dev.set_elements_device(0, dimg.data_ptr(), n)
    dev.upload_graph(adj)
    for L in (10, 40):
        hi, hd, hst = host.search(da.Knn(L), hq, k)
        di = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
        dd = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        ds = torch.zeros((nq, 20), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        da._ffi.check(da.lib().dann_search_batch_device(dev._h, C.c_void_p(dq.data_ptr()), nq, L, 1, k,
                                                        C.c_void_p(di.data_ptr()), C.c_void_p(dd.data_ptr()),
                                                        C.c_void_p(ds.data_ptr())), "dann_search_batch_device")
        torch.cuda.synchronize()
        gst = ds.cpu().numpy().reshape(-1).view(da.STATS_DTYPE)
        assert np.array_equal(di.cpu().numpy().view(np.uint32), hi), L
        assert np.array_equal(fbits(dd.cpu().numpy()), fbits(hd)), L
        assert np.array_equal(gst["cmps"], hst["cmps"]) and np.array_equal(gst["hops"], hst["hops"]), L
        assert (hst["cmps"] > L).all()


def _status(parts):
    h = C.c_void_p()
    rc = da.lib().dann_transform_create(-1, C.byref(parts), C.byref(h))
    assert (rc == 0) == bool(h.value)
    if h.value:
        da.lib().dann_transform_destroy(h)
    return rc


def test_rejections():
    E, U = da._ffi.EINVAL, da._ffi.EUNSUPPORTED
    ok, neg = np.zeros(8, np.uint32), np.full(8, 0x80000000, np.uint32)
    u32 = lambda *v: np.array(v, np.uint32)

    def raises(variant, status, f, *a):
        with pytest.raises(da.DannError) as e:
            f(*a)
        assert e.value.status == status and variant in str(e.value), (variant, str(e.value))

    P, D = da.Transform.padding_hadamard, da.Transform.double_hadamard
    # PaddingHadamard::try_from_parts
    raises("InvalidSignRepresentation", E, P, u32(0, 1, 0, 0), 4)
    raises("SignsTooLong", E, P, np.zeros(9, np.uint32), 8)
    raises("DimNotPowerOfTwo", E, P, np.zeros(5, np.uint32), 6)
    raises("DimNotPowerOfTwo", E, P, np.zeros(5, np.uint32), 12)
    raises("SubsampleNotMonotonic", E, P, ok, 8, u32(1, 3, 3))
    raises("SubsampleNotMonotonic", E, P, ok, 8, u32(2, 1))
    raises("LastSubsampleTooLarge", E, P, ok, 8, u32(0, 8))
    raises("SubsampleEmpty", E, P, ok, 8, u32())
    raises("empty", E, P, u32(), 8)
    # DoubleHadamard::try_from_parts
    raises("Signs0Empty", E, D, u32(), ok)
    raises("Signs1TooSmall", E, D, ok, neg[:7])
    raises("Signs0Invalid", E, D, u32(0, 0x80000001), neg)
    raises("Signs1Invalid", E, D, ok, u32(0, 0, 0, 0, 0, 0, 0, 0, 7))
    raises("SubsampleNotMonotonic", E, D, ok, neg, u32(4, 4))
    raises("LastSubsampleTooLarge", E, D, ok, neg, u32(0, 8))
    raises("InvalidSubsampleLength", E, D, ok, neg, u32())
    raises("signs1 must be as long as signs0", E, D, ok, np.zeros(10, np.uint32), u32(0, 1))
    # reserved / unsupported
    assert _status(da._ffi.TransformParts(kind=da._ffi.TRANSFORM_RANDOM_ROTATION, dim=8)) == U
    raises("16384", U, P, np.zeros(4, np.uint32), 32768)
    raises("16384", U, D, np.zeros(5, np.uint32), np.zeros(32768, np.uint32))
    for kind in (-1, 4):
        assert _status(da._ffi.TransformParts(kind=kind, dim=8)) == E
    assert _status(da._ffi.TransformParts(kind=da._ffi.TRANSFORM_NULL, dim=0)) == E
    assert da.lib().dann_transform_create(-1, None, None) == E
    # the quantiser
    t = P(ok, 8)
    x = np.ones((2, 8), np.float32)
    out = np.zeros((2, 28), np.uint8)
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    L = da.lib()
    assert L.dann_minmax_quantize(t._h, 3, 1.0, xp, 2, op, None) == E
    assert L.dann_minmax_quantize(t._h, 8, 0.0, xp, 2, op, None) == E
    assert L.dann_minmax_quantize(t._h, 8, 1.0, None, 2, op, None) == E
    assert L.dann_minmax_quantize(t._h, 8, 1.0, xp, 2, None, None) == E
    assert L.dann_minmax_quantize(None, 8, 1.0, xp, 2, op, None) == E
    assert L.dann_minmax_quantize_device(t._h, 3, 1.0, xp, 8, 2, op, 28, None) == E
    assert L.dann_minmax_quantize(t._h, 8, 1.0, None, 0, None, None) == 0  # n == 0
    assert L.dann_transform_apply(t._h, None, 0, None) == 0
    assert L.dann_transform_apply(t._h, None, 2, op) == E
    assert L.dann_transform_apply_device(t._h, None, 8, 0, None, 8) == 0
    assert L.dann_transform_input_dim(None) == E and L.dann_transform_output_dim(None) == E
    assert L.dann_transform_destroy(None) == 0
