"""CPU model of the MinMax-quantised rows (minmax::Data<NBITS>, diskann-quantization/src/minmax): the byte images, the
four distance functions with every f32 operation on its own and in the reference's association, the compressor with
its sequential f32 sums, and exact twin rows.  numpy only.

Row (front-canonical, meta/vector.rs:124-146): the 20-byte MinMaxCompensation (vectors.rs:43-51, little-endian u32 dim,
f32 b, f32 n, f32 a, f32 norm_squared), then ceil(dim * bits / 8) code bytes in the Dense permutation (element i at
bits [i * bits, (i + 1) * bits), little-endian within a byte; 8 bits: one byte per code).  A row stands for the
vector a * code + b; n = a * sum(code), norm_squared = |a * code + b|^2.

Distances (vectors.rs:206-229 and :231-473), x the first argument, y the second, raw the exact u32 inner product of
the codes:
    t0 = (x.a * y.a) * (f32)raw
    v  = ((t0 + x.n * y.b) + y.n * x.b) + (x.b * y.b) * (f32)dim
    L2 = (-2 v + x.norm_squared) + y.norm_squared, IP = -v, Cosine = 1 - v / (sqrt(x.ns) * sqrt(y.ns)), CosN = 1 - v
The epilogue is NOT symmetric in x and y: the two orders differ in the last bit for a few percent of random pairs.

twin_rows: a = 1, b = 0, n = sum(code), norm_squared = sum(code^2).  Then v = raw and L2 = sum((x - y)^2) exactly,
every intermediate an integer below 2^24 in magnitude, provided 2 * (hi - 1)^2 * dim < 2^24 for codes in [0, hi): an
oracle U8 L2 index over the unpacked codes is an exact twin of such an index, in both argument orders."""
import numpy as np

from spherical_model import knn_search, pack as _pack_bits, unpack as _unpack_bits  # noqa: F401  (knn_search: re-export)

f32 = np.float32
COSINE, IP, L2, COSINE_NORMALIZED = 0, 1, 2, 3  # == oracle / diskann_amd metric values
METRICS = (COSINE, IP, L2, COSINE_NORMALIZED)
SAME_AS_DATA, FULL_PRECISION, EIGHT_BIT = 0, 3, 8
HEADER = 20
BITS = (1, 2, 4, 8)


def code_bytes(bits, dim):
    return (dim * bits + 7) // 8


def layer_bytes(bits, dim):
    return HEADER + code_bytes(bits, dim)


def store_stride(bits, dim):
    """the Store's stride (store.rs:198-211): payload + tag byte, rounded up to 32"""
    return (layer_bytes(bits, dim) + 1 + 31) // 32 * 32


def pack(codes, bits):
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    return codes.copy() if bits == 8 else _pack_bits(codes, bits)


def unpack(code_bytes_, bits, dim):
    code_bytes_ = np.ascontiguousarray(code_bytes_, dtype=np.uint8)
    return code_bytes_[..., :dim].copy() if bits == 8 else _unpack_bits(code_bytes_, bits, dim)


def make_rows(codes, bits, b, n, a, norm_squared, dim_field=None):
    """(rows, dim) codes + (rows,) header fields -> (rows, layer_bytes) images, padding bits zero"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    nrows, dim = codes.shape
    out = np.zeros((nrows, layer_bytes(bits, dim)), np.uint8)
    out[:, 0:4] = np.full(nrows, dim if dim_field is None else dim_field, np.uint32).view(np.uint8).reshape(nrows, 4)
    hdr = np.stack([np.asarray(t, np.float32).reshape(nrows) for t in (b, n, a, norm_squared)], axis=1)
    out[:, 4:HEADER] = np.ascontiguousarray(hdr).view(np.uint8).reshape(nrows, 16)
    out[:, HEADER:] = pack(codes, bits)
    return out


def header(rows):
    """(dim u32, b, n, a, norm_squared) columns of (rows, >= 20) images"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    rows = rows.reshape(-1, rows.shape[-1])
    h = np.ascontiguousarray(rows[:, 4:HEADER]).view(np.float32)
    return np.ascontiguousarray(rows[:, 0:4]).view(np.uint32)[:, 0], h[:, 0], h[:, 1], h[:, 2], h[:, 3]


def codes_of(rows, bits, dim):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    rows = rows.reshape(-1, rows.shape[-1])
    return unpack(rows[:, HEADER:], bits, dim)


def decompress(rows, bits, dim):
    """a * code + b in float64"""
    _, b, _, a, _ = header(rows)
    return a.astype(np.float64)[:, None] * codes_of(rows, bits, dim).astype(np.float64) + b.astype(np.float64)[:, None]


def distance_matrix(metric, queries, rows, dim, bits, qbits=None):
    """(nq, n) f32: every query image (codes of `qbits` bits, default the rows' width) as the FIRST argument against
    every row as the second.  numpy evaluates each f32 operation on its own (no fused multiply-add)."""
    qbits = bits if qbits is None else qbits
    X = codes_of(queries, qbits, dim).astype(np.int64)
    Y = codes_of(rows, bits, dim).astype(np.int64)
    raw = X @ Y.T
    assert raw.max(initial=0) < (1 << 32)
    raw = raw.astype(np.uint32).astype(np.float32)  # u32 -> f32: round to nearest even
    _, xb, xn, xa, xs = (t[:, None] for t in header(queries))
    _, yb, yn, ya, ys = (t[None, :] for t in header(rows))
    with np.errstate(all="ignore"):
        t0 = (xa * ya) * raw
        v = ((t0 + xn * yb) + yn * xb) + (xb * yb) * f32(dim)
        if metric == L2:
            r = (f32(-2.0) * v + xs) + ys
        elif metric == IP:
            r = -v
        elif metric == COSINE:
            r = f32(1.0) - v / (np.sqrt(xs) * np.sqrt(ys))
        else:
            r = f32(1.0) - v
    assert r.dtype == np.float32
    return r


def distance_rows(metric, x, y, dim, bits):
    return distance_matrix(metric, x[None, :], y[None, :], dim, bits)[0, 0]


# ---- MinMaxQuantizer::compress_into (quantizer.rs:117-228), NullTransform ------------------------------------------------
def _seq_sum(cols):
    """sequential f32 sum over axis 1, one chain per row"""
    acc = np.zeros(cols.shape[0], np.float32)
    for i in range(cols.shape[1]):
        acc = acc + cols[:, i]
    return acc


def compress(x, bits, grid_scale=1.0):
    """(n, dim) f32 -> (images (n, layer_bytes), loss (n,) f32 = L2Loss::as_f32, nan (n,) bool = InputContainsNaN)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, dim = x.shape
    g = f32(grid_scale)
    with np.errstate(all="ignore"):
        if bits == 1:
            mean = _seq_sum(x) / f32(dim)
            m = (x < mean[:, None]).astype(np.float32)
            mn, mnc = _seq_sum(m * x), _seq_sum(m)
            mx, mxc = _seq_sum((f32(1.0) - m) * x), _seq_sum(f32(1.0) - m)
            lo, hi = np.fmin(mn / mnc, mean), np.fmax(mx / mxc, mean)  # f32::min / max: a NaN operand loses
        else:
            lo, hi = np.fmin.reduce(x, axis=1), np.fmax.reduce(x, axis=1)  # the NaN-ignoring fold
        width = (hi - lo) / f32(2.0)
        mid = lo + width
        lo, hi = mid - width * g, mid + width * g
        top = f32((1 << bits) - 1)
        inv = np.fmax(hi - lo, f32(1e-8)) / top
        t = np.clip((x - lo[:, None]) / inv[:, None], f32(0.0), top)
        # f32::round, half away from zero; t >= 0 after the clamp.  (floor(t + 0.5) would round t = 0.49999997 up: the
        # fraction t - floor(t) is exact, so compare that.)
        fl = np.floor(t)
        code = np.where(t - fl >= f32(0.5), fl + f32(1.0), fl).astype(np.float32)
        vr = code * inv[:, None] + lo[:, None]
        ns = _seq_sum(vr * vr)
        csum = _seq_sum(code)  # (integers below 2^24: order-free)
        d = vr - x
        loss = _seq_sum(d * d)
    nan = np.isnan(x).any(axis=1)
    codes = np.where(np.isnan(code), 0, code).astype(np.uint8)  # (`NaN as u8` is 0)
    loss = np.where(loss > 0, loss, f32(0.0)).astype(np.float32)
    return make_rows(codes, bits, lo, inv * csum, inv, ns), loss, nan


# ---- exact twins ---------------------------------------------------------------------------------------------------------
def twin_rows(codes, bits):
    """rows with a = 1, b = 0, n = sum(code), norm_squared = sum(code^2): L2 == sum((x - y)^2) of the codes, exactly"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, dim = codes.shape
    hi = int(codes.max(initial=0)) + 1
    assert hi <= (1 << bits) and 2 * (hi - 1) ** 2 * dim < (1 << 24), (hi, dim)
    c = codes.astype(np.int64)
    return make_rows(codes, bits, np.zeros(n), c.sum(1), np.ones(n), (c * c).sum(1))
