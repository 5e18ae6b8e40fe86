"""CPU model of the packed scalar-quantised rows (SQ4 / SQ1; 8 bits for pinning it to the oracle) and the construction
that makes the SQ-8 oracle an exact reference for them.

Layout (CompensatedVector<NBITS>, Dense permutation, diskann-quantization/src/scalar/vectors.rs:128-175): ceil(dim * bits
/ 8) code bytes -- element i at bits [i * bits, (i + 1) * bits), little-endian within a byte -- then the f32 compensation.

The oracle knows SQ-8 only.  Two facts make it exact for the packed widths:
  1. codes unpacked to one byte each have the same integer sums sum((x - y)^2) and sum(x * y);
  2. the only other difference is the epilogue's constant k = (ibs * ibs) * (scale * scale), ibs = 1 / (2^bits - 1).  For
     about half of all f32 scales s there is an f32 s8 whose SQ-8 constant equals k_bits(s) bit for bit
     (matched_scale8 nudges s upward ulp by ulp until one exists).
An oracle SQ8 index over the unpacked rows (compensations unchanged) with sq_scale = s8 -- the twin -- then returns the
distance bits of the low-bit formula from every one of its entry points."""
import ctypes as C
import ctypes.util

import numpy as np

import oracle

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
f32 = np.float32


def fmaf(a, b, c):
    return f32(_libm.fmaf(float(a), float(b), float(c)))


def code_bytes(bits, dim):
    return (dim * bits + 7) // 8


def layer_bytes(bits, dim):
    return code_bytes(bits, dim) + 4


def pack(codes, bits):
    """(n, dim) codes below 2^bits -> (n, ceil(dim * bits / 8)) bytes, padding bits zero"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if codes.ndim == 1:
        return pack(codes[None, :], bits)[0]
    assert bits in (1, 4, 8) and (codes < (1 << bits)).all()
    n, dim = codes.shape
    if bits == 8:
        return codes.copy()
    if bits == 1:
        return np.packbits(codes, axis=1, bitorder="little")
    c = np.zeros((n, (dim + 1) // 2 * 2), np.uint8)
    c[:, :dim] = codes
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def unpack(packed, bits, dim):
    """code bytes (a row's trailing bytes are ignored) -> (n, dim) codes, one byte each"""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    if packed.ndim == 1:
        return unpack(packed[None, :], bits, dim)[0]
    cb = code_bytes(bits, dim)
    p = packed[:, :cb]
    if bits == 8:
        return p.copy()
    if bits == 1:
        return np.unpackbits(p, axis=1, bitorder="little")[:, :dim]
    out = np.empty((p.shape[0], 2 * cb), np.uint8)
    out[:, 0::2] = p & 15
    out[:, 1::2] = p >> 4
    return out[:, :dim].copy()


def ibs(bits):
    return f32(1.0) / f32((1 << bits) - 1)


def k_const(bits, scale):
    """(ibs * ibs) * (scale * scale) in f32, in that order (scalar/mod.rs:129-135, vectors.rs:231-233)"""
    s = f32(scale)
    return f32(f32(ibs(bits) * ibs(bits)) * f32(s * s))


def compress(x, shift, scale, bits):
    """ScalarQuantizer::compress_into::<bits> (quantizer.rs:190-238, 407-430): rows of packed codes + compensation"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x = x.reshape(-1, x.shape[-1])
    shift = np.ascontiguousarray(shift, dtype=np.float32)
    n, dim = x.shape
    mx = f32((1 << bits) - 1)
    inverse_scale = f32(mx / f32(scale))
    with np.errstate(invalid="ignore", over="ignore"):
        c = ((x - shift[None, :]) * inverse_scale).astype(np.float32)
        c = np.where(c < 0, f32(0), np.where(c > mx, mx, c)).astype(np.float32)  # NaN stays NaN
        t = np.trunc(c)
        c = (t + ((c - t) >= f32(0.5)).astype(np.float32)).astype(np.float32)   # round half away from zero (c >= 0)
    codes = np.where(np.isnan(c), 0, c).astype(np.uint8)                        # `NaN as u8` == 0
    out = np.zeros((n, layer_bytes(bits, dim)), np.uint8)
    out[:, :code_bytes(bits, dim)] = pack(codes, bits)
    comp = np.empty(n, np.float32)
    k = f32(f32(scale) * ibs(bits))
    sh = shift.tolist()
    for i in range(n):
        dot, ci = 0.0, c[i].tolist()
        for d in range(dim):
            dot = _libm.fmaf(ci[d], sh[d], dot)  # dot = code.mul_add(shift[d], dot), in element order
        with np.errstate(invalid="ignore", over="ignore"):
            comp[i] = f32(k * f32(dot))
    out[:, code_bytes(bits, dim):] = comp.view(np.uint8).reshape(n, 4)
    return out


def compensation(row, bits, dim):
    cb = code_bytes(bits, dim)
    return np.ascontiguousarray(row[cb:cb + 4]).view(np.float32)[0]


def distance(metric, x, y, dim, bits, scale, shift_norm_sq):
    """CompensatedSquaredL2 / CompensatedIP / CompensatedCosineNormalized (vectors.rs:171-465) of two rows: exact integer
    sums (bits/distances.rs), then the epilogue in f32"""
    ux = unpack(x, bits, dim).astype(np.int64)
    uy = unpack(y, bits, dim).astype(np.int64)
    k = k_const(bits, scale)
    if metric in (oracle.L2, oracle.COSINE_NORMALIZED):
        l2 = f32(k * f32(int(((ux - uy) ** 2).sum())))
        if metric == oracle.L2:
            return l2
        sim = f32(f32(1.0) - f32(l2 / f32(2.0)))
        return f32(f32(1.0) - sim)
    assert metric == oracle.INNER_PRODUCT
    raw = f32(int((ux * uy).sum()))
    r = f32(fmaf(k, raw, f32(shift_norm_sq)) + f32(compensation(y, bits, dim) + compensation(x, bits, dim)))
    return f32(-r)


def _step(v, n):
    v = f32(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, f32(np.inf) if n > 0 else f32(0.0), dtype=np.float32)
    return v


def matched_scale8(bits, scale, max_nudges=4096):
    """(s, s8): the first f32 s >= scale (ulp by ulp) for which an f32 s8 with k_const(8, s8) == k_const(bits, s)
    exists, and that s8 (searched within a few ulps of sqrt(k_bits(s) / (1/255)^2))"""
    s = f32(scale)
    c255 = f32(ibs(8) * ibs(8))
    for _ in range(max_nudges):
        k = k_const(bits, s)
        g = f32(np.sqrt(np.float64(k) / np.float64(c255)))
        for d in range(-8, 9):
            s8 = _step(g, d)
            if k_const(8, s8) == k:
                return float(s), float(s8)
        s = _step(s, 1)
    raise AssertionError("no matching SQ-8 scale found")


def twin_rows(rows, bits, dim):
    """packed rows (codes + compensation) -> SQ-8 rows: one byte per code, the compensation unchanged"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    rows = rows.reshape(-1, rows.shape[-1])
    cb = code_bytes(bits, dim)
    out = np.empty((rows.shape[0], dim + 4), np.uint8)
    out[:, :dim] = unpack(rows, bits, dim)
    out[:, dim:] = rows[:, cb:cb + 4]
    return out


def oracle_twin(metric, dim, capacity, max_degree, bits, rows, start_rows, scale8, shift_norm_sq, adj=None, **kw):
    """the oracle SQ8 index over the unpacked rows with the matched scale (matched_scale8's second value)"""
    oix = oracle.Index(oracle.SQ8, metric, dim, capacity, max_degree, twin_rows(start_rows, bits, dim), sq_scale=scale8,
                       sq_shift_norm_sq=shift_norm_sq, **kw)
    if rows is not None:
        oix.set_rows(0, twin_rows(rows, bits, dim))
    if adj is not None:
        oix.adj[:] = adj
    return oix
