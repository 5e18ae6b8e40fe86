"""SphericalQuantizer::compress_into on the GPU (dann_spherical_*, csrc/spherical_kernels.hip) against the CPU statement
(tests/spherical_compress_model.py): rows and queries byte for byte, the strides, the device-to-device path into an index
and its searches, and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import spherical_compress_model as scm
import spherical_model as sm
from helpers import bits as fbits, random_graph

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

DT = {1: da.SPH1, 2: da.SPH2, 4: da.SPH4}
METRICS = (sm.L2, sm.IP, sm.COSINE)
LDS_CUTOFF = 256  # kSphLdsDim of spherical_kernels.hip: the heap of a wider output_dim lives in global memory
N = 130  # two wavefronts of rows and a tail


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
    def __init__(self, nbytes, src=None):
        self.hip, self.p, self.n = _hip(), C.c_void_p(), nbytes
        assert self.hip.hipMalloc(C.byref(self.p), max(nbytes, 16)) == 0
        if src is not None:
            src = np.ascontiguousarray(src)
            assert src.nbytes <= nbytes and self.hip.hipMemcpy(self.p, src.ctypes.data_as(C.c_void_p), src.nbytes, 1) == 0

    def get(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.n and self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, out.nbytes, 2) == 0
        return out

    def __del__(self):
        if self.p:
            self.hip.hipFree(self.p)


def _signs(rng, n):
    return (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _parts(name):
    """(model transform, constructor of the GPU transform) of a named case"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("null"):
        dim = int(name[4:])
        return scm.Transform.null(dim), lambda: da.Transform.null(dim)
    if name == "pad100":
        s = _signs(rng, 100)
        return scm.Transform.padding_hadamard(s, 128), lambda: da.Transform.padding_hadamard(s, 128)
    if name == "pad100sub96":
        s = _signs(rng, 100)
        sub = np.sort(rng.choice(128, 96, replace=False)).astype(np.uint32)
        return scm.Transform.padding_hadamard(s, 128, sub), lambda: da.Transform.padding_hadamard(s, 128, sub)
    assert name == "double96"
    s0, s1 = _signs(rng, 96), _signs(rng, 96)
    return scm.Transform.double_hadamard(s0, s1), lambda: da.Transform.double_hadamard(s0, s1)


TRANSFORMS = ("null5", "null64", "pad100", "pad100sub96", "double96")


@functools.lru_cache(maxsize=None)
def _inputs(name, n=N):
    """Gaussian rows, integer-lattice rows (ties in the heap), rows with zero elements, a row with one non-zero element
    and the centroid itself; the shift is on the half-integer lattice so that the lattice rows stay on one"""
    mt, _ = _parts(name)
    dim = mt.input_dim
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    shift = (rng.integers(-1, 2, dim) * 0.5).astype(np.float32)
    x = rng.normal(0.1, 1.0, (n, dim)).astype(np.float32)
    k = min(24, n // 4)
    x[:k] = rng.integers(-3, 4, (k, dim)).astype(np.float32)
    zk = min(8, n // 8)
    x[k:k + zk] *= rng.integers(0, 2, (zk, dim)).astype(np.float32)
    if n > k + zk + 2:
        x[k + zk] = 0.0
        x[k + zk, dim // 2] = -1.75
        x[k + zk + 1] = shift
    x.setflags(write=False)
    shift.setflags(write=False)
    return x, shift


@functools.lru_cache(maxsize=None)
def _model(name, metric, pre_scale=1.0, n=N):
    x, shift = _inputs(name, n)
    return scm.Compressor(_parts(name)[0], metric, shift, pre_scale)


@functools.lru_cache(maxsize=None)
def _want_rows(name, metric, bits):
    out, status = _model(name, metric).rows(_inputs(name)[0], bits, return_status=True)
    out.setflags(write=False)
    return out, status


def _gpu(name, metric, pre_scale=1.0, n=N):
    x, shift = _inputs(name, n)
    t = _parts(name)[1]()
    q = da.SphericalCompressor(t, metric, shift, pre_scale)
    t.close()  # the handle keeps its own copy of the transform
    return q


def _diff(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"{bad.size} rows differ, first {bad[:5].tolist()}"


# ---- rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRANSFORMS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", [1, 2, 4])
def test_rows_match_model(bits, metric, name):
    x, _ = _inputs(name)
    want, status = _want_rows(name, metric, bits)
    assert all(s == scm.OK for s in status)
    if metric != sm.COSINE:
        assert not want[24 + 8 + 1].any() and want[24 + 8].any()  # the centroid row: a zero image
    q = _gpu(name, metric)
    got = q.compress(x, bits)
    assert got.shape == want.shape and np.array_equal(got, want), _diff(got, want)
    assert fbits(np.float32(q.shift_norm_sq)) == fbits(np.float32(_model(name, metric).shift_norm_sq))


@pytest.mark.parametrize("dim", [LDS_CUTOFF, LDS_CUTOFF + 1, 2048])
def test_rows_beyond_the_lds_cutoff(dim):
    """output_dim <= LDS_CUTOFF keeps a wavefront's heap in LDS; LDS_CUTOFF + 1 (an odd length) and 2048 use the global
    scratch of the same layout"""
    name = f"null{dim}"
    x, _ = _inputs(name, 3)
    want = _model(name, sm.L2, n=3).rows(x, 4)
    got = _gpu(name, sm.L2, n=3).compress(x, 4)
    assert np.array_equal(got, want), _diff(got, want)


# ---- queries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["null5", "null64", "pad100"])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("bits", [1, 2, 4])
def test_queries_match_model(bits, metric, name):
    x, _ = _inputs(name)
    layout = sm.FOUR_BIT_TRANSPOSED if bits == 1 else sm.SCALAR_QUANTIZED
    mc, q = _model(name, metric), _gpu(name, metric)
    want = mc.queries(x, bits, layout)
    got = q.queries(x, bits, layout)
    assert got.shape == (N, sm.query_bytes(bits, mc.t.output_dim, layout)) and np.array_equal(got, want), _diff(got, want)
    same = q.queries(x, bits, sm.SAME_AS_DATA)
    assert np.array_equal(same, q.compress(x, bits)) and np.array_equal(same, _want_rows(name, metric, bits)[0])


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_query_whose_minimum_is_negative_zero(bits):
    """the fold keeps the last zero's sign, and it reaches offset = min / scale"""
    layout = sm.FOUR_BIT_TRANSPOSED if bits == 1 else sm.SCALAR_QUANTIZED
    x = np.array([[0.0, -0.0, 1.0, 2.0, 0.5], [-0.0, 0.0, 1.0, 2.0, 0.5], [3.0, 0.0, 0.0, -0.0, 1.0]], np.float32)
    shift = np.zeros(5, np.float32)
    want = scm.Compressor(scm.Transform.null(5), sm.L2, shift).queries(x, bits, layout)
    before = want.shape[1] - 16
    offs = [sm.query_meta(w, before)[2] for w in want]
    assert [bool(np.signbit(o)) for o in offs] == [True, False, True] and all(o == 0 for o in offs)
    t = da.Transform.null(5)
    got = da.SphericalCompressor(t, sm.L2, shift).queries(x, bits, layout)
    assert np.array_equal(got, want), _diff(got, want)


# ---- strides ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,layout", [(1, sm.SAME_AS_DATA), (4, sm.SAME_AS_DATA), (1, sm.FOUR_BIT_TRANSPOSED),
                                         (2, sm.SCALAR_QUANTIZED)])
def test_strides_and_untouched_bytes(bits, layout):
    name = "pad100"
    x, _ = _inputs(name)
    mc, q = _model(name, sm.IP), _gpu(name, sm.IP)
    want = mc.queries(x, bits, layout)
    ib = want.shape[1]
    xs = mc.t.input_dim + 3
    os_ = sm.store_stride(bits, mc.t.output_dim) if layout == sm.SAME_AS_DATA else ib + 5
    wide = np.full((N, xs), np.float32(7.5))
    wide[:, :mc.t.input_dim] = x
    dx = DevBuf(wide.nbytes, wide)
    dout = DevBuf(N * os_, np.full(N * os_, 0xA5, np.uint8))
    if layout == sm.SAME_AS_DATA:
        q.compress_device(dx.p.value, N, bits, dout.p.value, x_stride=xs, out_stride=os_)
    else:
        q.queries_device(dx.p.value, N, bits, layout, dout.p.value, x_stride=xs, out_stride=os_)
    got = dout.get(np.uint8, (N, os_))
    assert np.array_equal(got[:, :ib], want), _diff(got[:, :ib], want)
    assert (got[:, ib:] == 0xA5).all()
    # packed, straight into the caller's buffer
    dx2 = DevBuf(x.nbytes, x)
    dout2 = DevBuf(N * ib + 8, np.full(N * ib + 8, 0xA5, np.uint8))
    if layout == sm.SAME_AS_DATA:
        q.compress_device(dx2.p.value, N, bits, dout2.p.value)
    else:
        q.queries_device(dx2.p.value, N, bits, layout, dout2.p.value)
    got = dout2.get(np.uint8, (N * ib + 8,))
    assert np.array_equal(got[:N * ib].reshape(N, ib), want) and (got[N * ib:] == 0xA5).all()


# ---- end to end on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,layout", [(1, sm.FOUR_BIT_TRANSPOSED), (2, sm.SCALAR_QUANTIZED), (4, sm.SAME_AS_DATA)])
def test_device_rows_and_queries_feed_the_search(bits, layout):
    rng = np.random.default_rng(40 + bits)
    n, dim, R, nq, k = 256, 64, 12, 24, 10
    metric = sm.L2 if bits != 2 else sm.IP
    data = rng.normal(0.2, 1.0, (n, dim)).astype(np.float32)
    queries = rng.normal(0.2, 1.0, (nq, dim)).astype(np.float32)
    shift = data.mean(0).astype(np.float32)
    signs = _signs(rng, dim)
    mc = scm.Compressor(scm.Transform.padding_hadamard(signs, dim), metric, shift)
    q = da.SphericalCompressor(da.Transform.padding_hadamard(signs, dim), metric, shift)
    assert fbits(np.float32(q.shift_norm_sq)) == fbits(np.float32(mc.shift_norm_sq))
    ssn = float(mc.shift_norm_sq) if metric != sm.L2 else 0.0
    start = mc.rows(data[:1] * np.float32(0.5) + data[1:2] * np.float32(0.5), bits)
    adj = random_graph(rng, n, R)
    ib, qb = sm.layer_bytes(bits, dim), sm.query_bytes(bits, dim, layout)

    def index():
        gix = da.Provider(DT[bits], metric, dim, n, R, start, sq_shift_norm_sq=ssn)
        gix.upload_graph(adj)
        gix.set_query_layout(layout)
        return gix

    dev, host = index(), index()
    ddata, dimg = DevBuf(data.nbytes, data), DevBuf(n * ib)
    q.compress_device(ddata.p.value, n, bits, dimg.p.value)
    dev.set_elements_device(0, dimg.p.value, n)
    host.set_elements(0, mc.rows(data, bits))
    dq, dqi = DevBuf(queries.nbytes, queries), DevBuf(nq * qb)
    q.queries_device(dq.p.value, nq, bits, layout, dqi.p.value)
    mq = mc.queries(queries, bits, layout)
    for L, W in ((10, 1), (24, 2)):
        di, dd, ds = DevBuf(nq * k * 4), DevBuf(nq * k * 4), DevBuf(nq * 20)
        da._ffi.check(da.lib().dann_search_batch_device(dev._h, dqi.p, nq, L, W, k, di.p, dd.p, ds.p), "dann_search_batch_device")
        gi, gd, gst = host.search(da.Knn(L, W), mq, k)
        hst = ds.get(np.uint8, (nq * 20,)).view(da.STATS_DTYPE)
        assert np.array_equal(di.get(np.uint32, (nq, k)), gi) and np.array_equal(fbits(dd.get(np.float32, (nq, k))), fbits(gd))
        for f in ("cmps", "hops", "result_count", "written"):
            assert np.array_equal(hst[f], gst[f]), f
        assert (gi[:, 0] < n).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _status(fn, *args):
    try:
        fn(*args)
    except da.DannError as e:
        return e.status, str(e)
    return da._ffi.OK, ""


def test_refusals():
    E, U = da._ffi.EINVAL, da._ffi.EUNSUPPORTED
    L = da.lib()
    dim = 16
    rng = np.random.default_rng(50)
    shift = np.zeros(dim, np.float32)
    x = rng.standard_normal((4, dim)).astype(np.float32)
    t = da.Transform.null(dim)
    # dann_spherical_create
    for metric, sh, ps in ((da.COSINE_NORMALIZED, shift, 1.0), (7, shift, 1.0), (sm.L2, np.full(dim, np.nan, np.float32), 1.0),
                           (sm.L2, np.full(dim, np.inf, np.float32), 1.0), (sm.L2, shift, 0.0), (sm.L2, shift, -1.0),
                           (sm.L2, shift, float("nan")), (sm.L2, shift, float("inf"))):
        assert _status(da.SphericalCompressor, t, metric, sh, ps)[0] == E, (metric, ps)
    h = C.c_void_p()
    parts = da._ffi.SphericalParts(metric=sm.L2, shift=shift.ctypes.data_as(C.c_void_p), pre_scale=1.0)
    assert L.dann_spherical_create(None, C.byref(parts), C.byref(h)) == E
    q = da.SphericalCompressor(t, sm.L2, shift)
    # bits and layouts: argument checks
    for bits in (0, 3, 8, -1):
        assert _status(q.compress, x, bits)[0] == E and _status(q.queries, x, bits, sm.SAME_AS_DATA)[0] == E, bits
    assert _status(q.queries, x, 1, sm.FULL_PRECISION)[0] == U and _status(q.queries, x, 4, sm.FULL_PRECISION)[0] == U
    assert _status(q.queries, x, 2, sm.FOUR_BIT_TRANSPOSED)[0] == U and _status(q.queries, x, 4, sm.FOUR_BIT_TRANSPOSED)[0] == U
    assert _status(q.queries, x, 1, sm.SCALAR_QUANTIZED)[0] == U
    assert _status(q.queries, x, 1, da.QUERY_EIGHT_BIT)[0] == U  # a layout no spherical width has, as dann_set_query_layout
    for layout in (-1, 4, 5, 7, 9):
        assert _status(q.queries, x, 1, layout)[0] == E, layout
    # strides below a row / an image, null handle, n == 0
    dx, dout = DevBuf(x.nbytes, x), DevBuf(4 * 64)
    assert _status(q.compress_device, dx.p.value, 4, 4, dout.p.value, dim - 1, 0)[0] == E
    assert _status(q.compress_device, dx.p.value, 4, 4, dout.p.value, 0, sm.layer_bytes(4, dim) - 1)[0] == E
    assert _status(q.queries_device, dx.p.value, 4, 2, sm.SCALAR_QUANTIZED, dout.p.value, 0, sm.query_bytes(2, dim, 2) - 1)[0] == E
    assert L.dann_spherical_compress(None, 1, dx.p, 4, dout.p) == E
    assert L.dann_spherical_compress_queries_device(None, 1, 0, dx.p, dim, 4, dout.p, 64) == E
    assert L.dann_spherical_compress(q._h, 1, None, 0, None) == da._ffi.OK
    assert L.dann_spherical_compress_device(q._h, 4, None, dim, 0, None, 64) == da._ffi.OK
    assert L.dann_spherical_compress_queries(q._h, 2, sm.SCALAR_QUANTIZED, None, 0, None) == da._ffi.OK
    assert L.dann_spherical_compress_queries_device(q._h, 1, sm.FOUR_BIT_TRANSPOSED, None, dim, 0, None, 64) == da._ffi.OK
    # flag words set by kernels that complete: InputContainsNaN
    for bad in (np.nan, 3.0e38):
        y = x.copy()
        y[2, 5] = bad
        y[2, 6] = bad
        for call in ((q.compress, y, 2), (q.queries, y, 1, sm.FOUR_BIT_TRANSPOSED)):
            st, msg = _status(*call)
            assert st == E and "InputContainsNaN" in msg, (bad, msg)
    # EncodingError
    y = x.copy()
    y[1] *= np.float32(300.0 / np.sqrt(float((x[1].astype(np.float64) ** 2).sum())))  # |X|^2 = 90000 > f16's 65504
    for bits in (1, 4):
        st, msg = _status(q.compress, y, bits)
        assert st == E and "MetricSpecific" in msg and scm.Compressor(scm.Transform.null(dim), sm.L2, shift).rows(
            y, bits, True)[1][1] == scm.ENC_MS, msg
    y[1] = x[1] * np.float32(1e6)
    st, msg = _status(q.compress, y, 2)
    assert st == E and "InnerProductCorrection" in msg, msg
    assert _status(q.queries, y, 2, sm.SCALAR_QUANTIZED)[0] == da._ffi.OK  # (a QueryMeta is four f32: nothing to overflow)


def test_bit_sum_above_u16_is_refused():
    """the widest output_dim the transform accepts: 16384 four-bit codes sum to more than 65535"""
    dim = 16384
    x = np.random.default_rng(51).standard_normal((1, dim)).astype(np.float32)
    shift = np.zeros(dim, np.float32)
    q = da.SphericalCompressor(da.Transform.null(dim), sm.L2, shift)
    st, msg = _status(q.compress, x, 4)
    assert st == da._ffi.EINVAL and "BitSum" in msg, msg
    got = q.compress(x, 2)  # 2 bits fit: bytes as the model's
    want = scm.Compressor(scm.Transform.null(dim), sm.L2, shift).rows(x, 2)
    assert np.array_equal(got, want)
