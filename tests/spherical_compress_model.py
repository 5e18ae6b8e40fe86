"""CPU statement of SphericalQuantizer::compress_into (diskann-quantization/src/spherical/quantizer.rs): the data side
(Data<1 | 2 | 4>) and the query sides (Query<4, BitTranspose>, Query<2 | 4, Dense>), every f32 / f64 operation on its own
and in the order the reference's x86-64 V3 code runs them.  numpy; transforms from transform_model, packing, transposition
and meta bytes from spherical_model.

    preprocess :338-381        mul * x - shift, FastL2Norm / InnerProduct in the V3 order (ip_v3), division by the norm
    data :805-861              1 bit :596-647; 2 and 4 bits compress_via_maximum_cosine :871-918 over
    maximize :991-1100         maximize_cosine_similarity, walking SliceHeap (algorithms/heap.rs:69-187) line for line
    queries :1128-1212         the min / max fold as x86-64 runs f32::min / f32::max (minss / maxss of (accumulator, i)
                               plus the NaN select: i comes back unless the accumulator is strictly smaller / larger, so
                               of several zeros the LAST one's sign stays; a NaN i leaves the accumulator)

The one fused operation (mul_add in :898 and the FMA chains of the inner product) is a single rounding: fma32 adds the
exact f64 product and the addend with the rounding error folded in as a sticky bit (round to odd), which makes the final
f64 -> f32 rounding the only one; fma32_exact is the same through exact rationals (the host test compares the two).
A row at the centroid and a row whose shifted norm is not finite give all-zero images; `status` names what the reference
would have returned for each row."""
import math
from fractions import Fraction

import numpy as np

import spherical_model as sm
import transform_model as tm

f32 = np.float32
L2, IP, COSINE = sm.L2, sm.IP, sm.COSINE
OK, NAN, ENC_IPC, ENC_MS, ENC_BITSUM = "ok", "InputContainsNaN", "InnerProductCorrection", "MetricSpecific", "BitSum"
F32_MAX = float(np.finfo(np.float32).max)


# ---- the fused multiply-add, one rounding ------------------------------------------------------------------------------------
def round_fraction_f32(fr):
    """an exact rational -> the nearest f32, ties to even (as a Python float); overflow gives +-inf"""
    if fr == 0:
        return 0.0
    sign = -1.0 if fr < 0 else 1.0
    fr = abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    assert Fraction(2) ** e <= fr < Fraction(2) ** (e + 1)
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    q = fr / ulp
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    val = n * ulp
    if val >= Fraction(2) ** 128:
        return sign * math.inf
    return sign * float(val)  # (24 significant bits: exact in f64)


def fma32_exact(a, b, c):
    """fma(a, b, c) of finite f32 values through exact rationals, rounded once"""
    return f32(round_fraction_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def fma32(a, b, c):
    """elementwise fma(a, b, c) on f32 arrays, rounded once: the product of two f32 is exact in f64; the f64 sum is
    rounded to odd (TwoSum recovers its error), so the f64 -> f32 rounding sees the sticky bit"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where((err > 0), np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


# ---- InnerProduct::evaluate for f32 in the V3 order (diskann-vector simd.rs: Strategy4x1, four f32x8 accumulators) -----------
def ip_v3(x, y):
    """(n, dim) x (n, dim) or (dim,) -> (n,) f32: element e of a full block of eight goes, by one fma, into lane e % 8 of
    accumulator (e / 8) % 4; the accumulators combine as (s0 + s1) + (s2 + s3); the partial block is one more fma into the
    combined vector; then sum_tree ((x0 + x4) + (x2 + x6)) + ((x1 + x5) + (x3 + x7))"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x = x.reshape(-1, x.shape[-1])
    y = np.broadcast_to(np.asarray(y, np.float32), x.shape)
    n, dim = x.shape
    full = dim & ~7
    acc = np.zeros((n, 32), np.float32)
    for base in range(0, full, 32):
        w = min(32, full - base)
        acc[:, :w] = fma32(x[:, base:base + w], y[:, base:base + w], acc[:, :w])
    s = acc.reshape(n, 4, 8)
    with np.errstate(all="ignore"):
        c = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
        rem = dim & 7
        if rem:
            c = c.copy()
            c[:, :rem] = fma32(x[:, full:], y[:, full:], c[:, :rem])
        return (((c[:, 0] + c[:, 4]) + (c[:, 2] + c[:, 6])) + ((c[:, 1] + c[:, 5]) + (c[:, 3] + c[:, 7]))).astype(np.float32)


def seq_sum(cols, dtype=np.float32):
    """sequential sum over axis 1 from 0.0, one chain per row"""
    acc = np.zeros(cols.shape[0], dtype)
    with np.errstate(all="ignore"):
        for i in range(cols.shape[1]):
            acc = acc + cols[:, i]
    return acc


def round_away(t):
    """f32::round: half away from zero (the fraction |t| - floor(|t|) is exact); a NaN stays"""
    a = np.abs(t)
    fl = np.floor(a)
    with np.errstate(invalid="ignore"):
        r = np.where(a - fl >= f32(0.5), fl + f32(1.0), fl)
    return np.copysign(r, t).astype(np.float32)


def clamp(t, lo, hi):
    """f32::clamp: a NaN stays"""
    with np.errstate(invalid="ignore"):
        return np.where(t < lo, lo, np.where(t > hi, hi, t)).astype(np.float32)


# ---- SliceHeap over Pair (heap.rs:69-187, quantizer.rs:933-958) ------------------------------------------------------------
class SliceHeap:
    """values / positions are parallel lists (the Pairs).  Pair's Ord is reversed and a NaN compares Equal:
    x <= y is not (y.value > x.value), x >= y is not (y.value < x.value), x < y is y.value < x.value."""

    def __init__(self, values, positions):
        self.v, self.p = values, positions
        self.heapify()

    def _swap(self, a, b):
        self.v[a], self.v[b] = self.v[b], self.v[a]
        self.p[a], self.p[b] = self.p[b], self.p[a]

    def heapify(self):
        n = len(self.v)
        if n <= 1:
            return
        for i in range((n - 2) // 2, -1, -1):
            self.sift_down(i)

    def sift_down(self, pos):
        v = self.v
        n = len(v)
        child = 2 * pos + 1
        while child <= max(n - 2, 0):  # len.saturating_sub(2)
            child += 1 if not (v[child + 1] > v[child]) else 0  # get(child) <= get(child + 1)
            if not (v[child] < v[pos]):  # get(pos) >= get(child)
                return
            self._swap(pos, child)
            pos = child
            child = 2 * pos + 1
        if child == n - 1 and v[child] < v[pos]:  # get(pos) < get(child)
            self._swap(pos, child)


def maximize_cosine_similarity(v, num_bits, trace=None):
    """v: (dim,) f32 -> optimal_scale (f32).  trace (a list): receives (value, position) of every pop."""
    v = np.asarray(v, np.float32)
    dim = v.size
    eps = f32(0.0001)
    with np.errstate(all="ignore"):
        absv = np.abs(v)
        stop = 1 << (num_bits - 1)
        # crit[r - 1][i] = (r as f32 + eps) / |v_i|; r = 1: (1.0 + eps) / |v_i|
        crit = [((f32(r) + eps) / absv).astype(np.float32).tolist() for r in range(1, stop + 1)]
    a64 = absv.astype(np.float64).tolist()
    current_ip = 0.0
    for a in a64:
        current_ip += a
    current_ip = 0.5 * current_ip
    current_square_norm = 0.25 * float(dim)
    rounded = [1] * dim
    heap = SliceHeap(list(crit[0]), list(range(dim)))
    hv, hp = heap.v, heap.p
    max_similarity = -math.inf
    optimal_scale = 0.0
    while True:
        value, position = hv[0], hp[0]
        if value == F32_MAX:
            break
        if trace is not None:
            trace.append((value, position))
        old_r = rounded[position]
        r = old_r + 1
        rounded[position] = r
        current_ip += a64[position]
        current_square_norm += float(2 * old_r)
        similarity = current_ip / math.sqrt(current_square_norm)
        if similarity > max_similarity:
            max_similarity = similarity
            optimal_scale = value
        hv[0] = crit[r - 1][position] if r < stop else F32_MAX
        heap.sift_down(0)
    return f32(optimal_scale)


# ---- transforms ------------------------------------------------------------------------------------------------------------
class Transform:
    def __init__(self, fn, input_dim, output_dim, preserves_norms):
        self.fn, self.input_dim, self.output_dim, self.preserves_norms = fn, input_dim, output_dim, preserves_norms

    @classmethod
    def null(cls, dim):
        return cls(tm.null, dim, dim, True)

    @classmethod
    def padding_hadamard(cls, signs, padded_dim, subsample=None):
        out = padded_dim if subsample is None else len(subsample)
        return cls(lambda x: tm.padding_hadamard(x, signs, padded_dim, subsample), len(signs), out, subsample is None)

    @classmethod
    def double_hadamard(cls, signs0, signs1, subsample=None):
        out = len(signs1) if subsample is None else len(subsample)
        return cls(lambda x: tm.double_hadamard(x, signs0, signs1, subsample), len(signs0), out, subsample is None)


# ---- the quantiser ---------------------------------------------------------------------------------------------------------
class Compressor:
    def __init__(self, transform, metric, shift, pre_scale=1.0):
        self.t, self.metric = transform, metric
        self.shift = np.ascontiguousarray(shift, dtype=np.float32).reshape(-1)
        assert self.shift.size == transform.input_dim
        self.pre_scale = f32(pre_scale)
        self.shift_norm_sq = f32(ip_v3(self.shift[None, :], self.shift)[0])  # CompensatedIP::new

    def preprocess(self, x):
        """-> (transformed (n, output_dim), shifted_norm, metric_specific, transformed_norm, live): rows that are not
        live (norm 0 or not finite) have transformed rows of zeros"""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.t.input_dim)
        n = x.shape[0]
        with np.errstate(all="ignore"):
            if self.metric == COSINE:
                norm = np.sqrt(ip_v3(x, x))
                mul = np.where(norm == 0, f32(1.0), f32(1.0) / norm).astype(np.float32)
            else:
                mul = np.full(n, self.pre_scale, np.float32)
            shifted = (mul[:, None] * x - self.shift[None, :]).astype(np.float32)
            sn = np.sqrt(ip_v3(shifted, shifted)).astype(np.float32)
            ms = (sn * sn).astype(np.float32) if self.metric == L2 else ip_v3(shifted, self.shift)
            finite = np.isfinite(sn)
            live = finite & (sn != 0)
            unit = np.where(live[:, None], shifted / np.where(live, sn, f32(1.0))[:, None], f32(0.0)).astype(np.float32)
            t = np.ascontiguousarray(self.t.fn(unit), dtype=np.float32)
            tn = np.ones(n, np.float32) if self.t.preserves_norms else np.sqrt(ip_v3(t, t)).astype(np.float32)
        return t, sn, ms, tn, live, finite

    def rows(self, x, bits, return_status=False, return_parts=False):
        """-> (n, layer_bytes(bits, output_dim)) images [, status per row]"""
        t, sn, ms, tn, live, finite = self.preprocess(x)
        n, dim = t.shape
        cb = sm.code_bytes(bits, dim)
        out = np.zeros((n, cb + sm.DATA_META), np.uint8)
        status = [OK if f else NAN for f in finite]
        with np.errstate(all="ignore"):
            if bits == 1:
                codes = (t > 0).astype(np.uint8)
                ipc = ((f32(2.0) * tn) * sn) / seq_sum(np.abs(t))
                scale = None
            else:
                scale = np.zeros(n, np.float32)
                for r in range(n):
                    if live[r]:
                        scale[r] = maximize_cosine_similarity(t[r], bits)
                top = f32((1 << bits) - 1)
                off = top / f32(2.0)
                v = round_away(clamp(t * scale[:, None] + off, f32(0.0), top))
                dv = (v - off).astype(np.float32)
                sip = np.zeros(n, np.float32)
                for i in range(dim):
                    sip = fma32(dv[:, i], t[:, i], sip)
                codes = np.where(np.isnan(v), 0, v).astype(np.uint8)
                ipc = (tn * sn) / sip
            bit_sum = codes.astype(np.int64).sum(1)
            ipc = ipc.astype(np.float32)
            h_ipc, h_ms = ipc.astype(np.float16), ms.astype(np.float16)
        with np.errstate(all="ignore"):
            images = np.concatenate([sm.pack(codes, bits), sm.data_meta_bytes(ipc, ms, bit_sum & 0xFFFF)], axis=1)
        for r in range(n):
            if not live[r]:
                continue
            out[r] = images[r]
            if not np.isfinite(h_ipc[r]):
                status[r] = ENC_IPC
            elif not np.isfinite(h_ms[r]):
                status[r] = ENC_MS
            elif bit_sum[r] > 0xFFFF:
                status[r] = ENC_BITSUM
        if return_parts:
            return out, status, dict(t=t, scale=scale, codes=codes, live=live)
        return (out, status) if return_status else out

    def queries(self, x, bits, layout, return_status=False):
        if layout == sm.SAME_AS_DATA:
            return self.rows(x, bits, return_status)
        assert layout == (sm.FOUR_BIT_TRANSPOSED if bits == 1 else sm.SCALAR_QUANTIZED), (bits, layout)
        qbits = 4 if layout == sm.FOUR_BIT_TRANSPOSED else bits
        t, sn, ms, _, live, finite = self.preprocess(x)
        n, dim = t.shape
        with np.errstate(all="ignore"):
            mn = np.full(n, F32_MAX, np.float32)
            mx = np.full(n, -F32_MAX, np.float32)
            for i in range(dim):
                e = t[:, i]
                nan = np.isnan(e)
                mn = np.where(nan, mn, np.where(mn < e, mn, e)).astype(np.float32)
                mx = np.where(nan, mx, np.where(mx > e, mx, e)).astype(np.float32)
            hi = f32((1 << qbits) - 1)
            scale = ((mx - mn) / hi).astype(np.float32)
            c = clamp(round_away(((t - mn[:, None]) / scale[:, None]).astype(np.float32)), f32(0.0), hi)
            bit_sum = seq_sum(c)
            codes = np.where(np.isnan(c), 0, c).astype(np.uint8)
            meta = sm.query_meta_bytes(sn * scale, bit_sum, mn / scale, ms)
        body = sm.transpose4(codes) if layout == sm.FOUR_BIT_TRANSPOSED else sm.pack(codes, qbits)
        out = np.concatenate([body, meta], axis=1)
        out[~live] = 0
        status = [OK if f else NAN for f in finite]
        return (out, status) if return_status else out
