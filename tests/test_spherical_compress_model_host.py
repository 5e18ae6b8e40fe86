"""The CPU statement of SphericalQuantizer::compress_into (tests/spherical_compress_model.py): the reference's own
property test of the maximiser, the heap's pop order, the single-rounding fma, the inner product pinned to the oracle's,
the branches the GPU tests rely on, and the new declarations.  No GPU."""
import itertools
import math
import os
import re
from fractions import Fraction

import numpy as np

import oracle
import spherical_compress_model as scm
import spherical_model as sm
from helpers import bits as fbits

f32 = np.float32
LATTICE = np.array(list(itertools.product(range(8), repeat=4)), np.float64) - 3.5  # i0 outermost, as the reference's loops


# ---- the reference's property test (quantizer.rs:1249-1356) ---------------------------------------------------------------
def _maximizer_case(target):
    target = np.asarray(target, np.float32)
    scale = scm.maximize_cosine_similarity(target, 3)
    t64 = target.astype(np.float64)
    sims = (LATTICE @ t64) / (np.sqrt((LATTICE * LATTICE).sum(1)) * math.sqrt(float(t64 @ t64)))
    best = LATTICE[int(np.argmax(sims))] + 3.5  # (the first maximum: the reference keeps the best under a strict >)
    clamped = scm.clamp(scm.round_away((target * scale - f32(-3.5)).astype(np.float32)), f32(0.0), f32(7.0)).astype(np.float64)
    if np.array_equal(best, clamped):
        return True
    ratio = (best - 3.5) / (clamped - 3.5)
    return bool((ratio == ratio[0]).all())


def test_maximizer_finds_the_exhaustive_optimum():
    cases = [[-3.5 + i0, -3.5 + i1, -3.5 + i2, -3.5 + i3] for i0 in range(0, 8, 2) for i1 in range(1, 9, 2)
             for i2 in range(0, 8, 2) for i3 in range(1, 9, 2)]
    assert len(cases) == 256
    rng = np.random.default_rng(0x070D9FF8)
    for _ in range(300):
        cases.append((f32(rng.uniform(0.5, 10.0)) * rng.standard_normal(4).astype(np.float32)).astype(np.float32))
    bad = [np.asarray(c).tolist() for c in cases if not _maximizer_case(c)]
    assert not bad, bad[:5]


# ---- heap pop order -----------------------------------------------------------------------------------------------------
def _direct_pops(v, num_bits):
    """maximize_cosine_similarity's pop sequence from a direct transcription of SliceHeap run step by step: Pairs as
    tuples under Pair's Ord spelled out as a comparison function"""
    def cmp(x, y):  # Pair::cmp: other.value.partial_cmp(self.value).unwrap_or(Equal)
        return 1 if y[0] > x[0] else -1 if y[0] < x[0] else 0

    def sift_down(data, pos):
        n = len(data)
        child = 2 * pos + 1
        while child <= max(n - 2, 0):
            child += int(cmp(data[child], data[child + 1]) <= 0)
            if cmp(data[pos], data[child]) >= 0:
                return
            data[pos], data[child] = data[child], data[pos]
            pos = child
            child = 2 * pos + 1
        if child == n - 1 and cmp(data[pos], data[child]) < 0:
            data[pos], data[child] = data[child], data[pos]

    v = np.asarray(v, np.float32)
    eps, stop = f32(0.0001), 1 << (num_bits - 1)
    with np.errstate(all="ignore"):
        data = [(float((f32(1.0) + eps) / abs(x)), i) for i, x in enumerate(v)]
    for i in range((len(data) - 2) // 2, -1, -1) if len(data) > 1 else ():
        sift_down(data, i)
    rounded = [1] * len(v)
    pops = []
    while data[0][0] != scm.F32_MAX:
        value, p = data[0]
        pops.append((value, p))
        rounded[p] += 1
        with np.errstate(all="ignore"):
            data[0] = (float((f32(rounded[p]) + eps) / abs(v[p])) if rounded[p] < stop else scm.F32_MAX, p)
        sift_down(data, 0)
    return pops


def test_heap_pop_order():
    rng = np.random.default_rng(11)
    for dim in (1, 2, 3, 4, 7, 128):
        v = rng.standard_normal(dim).astype(np.float32)
        trace = []
        scm.maximize_cosine_similarity(v, 4, trace)
        values = [t[0] for t in trace]
        assert len(trace) == dim * 7 and values == sorted(values), dim  # tie-free: ascending
        assert trace == _direct_pops(v, 4), dim
    ties = 0
    for dim in (2, 5, 128):
        v = rng.integers(-3, 4, dim).astype(np.float32)  # zeros too: their critical values are +inf and never pop
        for bits in (2, 3, 4):
            trace = []
            scm.maximize_cosine_similarity(v, bits, trace)
            assert trace == _direct_pops(v, bits), (dim, bits)
            assert len(trace) == int(np.count_nonzero(v)) * ((1 << (bits - 1)) - 1), (dim, bits)
            ties += sum(1 for a, b in zip(trace, trace[1:]) if a[0] == b[0])
    assert ties > 500, ties


def test_heap_root_of_equal_values_is_not_position_order():
    """what a sorted-minimum formulation gets wrong: among equal values the pop order is the heap's, not the index's"""
    v = np.full(8, 0.5, np.float32)
    trace = []
    scm.maximize_cosine_similarity(v, 2, trace)
    assert sorted(p for _, p in trace) == list(range(8)) and [p for _, p in trace] != list(range(8))


# ---- the fused multiply-add -----------------------------------------------------------------------------------------------
def test_fma_is_a_single_rounding():
    rng = np.random.default_rng(5)
    # a * b + c one f64 ulp beside an f32 midpoint: the sum rounds to the midpoint in f64 and then the wrong way
    a = f32(1.0 + 2.0 ** -12)
    b = f32(1.0 + 2.0 ** -12)  # a * b = 1 + 2^-11 + 2^-24: exactly the midpoint of two f32 near 1
    cases = [(a, b, f32(2.0 ** -60)), (a, b, f32(-2.0 ** -60)), (a, b, f32(0.0)), (f32(3.0), f32(1.0 / 3.0), f32(-1.0)),
             (f32(2.0 ** -70), f32(2.0 ** -70), f32(2.0 ** -149)), (f32(1e30), f32(1e30), f32(-3.0e38)),
             (f32(16777217.0), f32(1.0), f32(0.5))]
    for _ in range(400):
        x, y = rng.standard_normal(2).astype(np.float32)
        p = Fraction(float(x)) * Fraction(float(y))
        near = f32(-float(p))  # the sum cancels to the product's low bits
        cases.append((x, y, near))
        cases.append((x, y, f32(rng.standard_normal() * 2.0 ** rng.integers(-30, 30))))
    wrong_via_f64 = 0
    for x, y, z in cases:
        want = scm.fma32_exact(x, y, z)
        got = scm.fma32(np.array([x]), np.array([y]), np.array([z]))[0]
        assert fbits(np.array([got]))[0] == fbits(np.array([want]))[0] or (np.isnan(got) and np.isnan(want)), (x, y, z, got, want)
        with np.errstate(all="ignore"):
            wrong_via_f64 += int(f32(float(x) * float(y) + float(z)) != want)
    assert wrong_via_f64 > 0  # the detour through f64 does round twice on these operands
    assert scm.round_fraction_f32(Fraction(2) ** -150) == 0.0 and scm.round_fraction_f32(Fraction(3, 2) * Fraction(2) ** -149) == 2.0 ** -148


def test_inner_product_order_is_the_oracles():
    rng = np.random.default_rng(6)
    for dim in (1, 5, 7, 8, 9, 31, 32, 33, 40, 63, 64, 65, 96, 100, 128, 131, 260):
        x = rng.standard_normal((6, dim)).astype(np.float32)
        y = rng.standard_normal((6, dim)).astype(np.float32)
        got = scm.ip_v3(x, y)
        want = np.array([-oracle.distance(oracle.F32, oracle.INNER_PRODUCT, x[i], y[i]) for i in range(6)], np.float32)
        assert np.array_equal(fbits(got), fbits(want)), dim
        self_ip = scm.ip_v3(x, x)
        want = np.array([-oracle.distance(oracle.F32, oracle.INNER_PRODUCT, x[i], x[i]) for i in range(6)], np.float32)
        assert np.array_equal(fbits(self_ip), fbits(want)), dim


# ---- branches ---------------------------------------------------------------------------------------------------------------
def _signs(rng, n):
    return (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)).astype(np.uint32)


def test_centroid_row_gives_zero_images():
    rng = np.random.default_rng(7)
    shift = rng.standard_normal(5).astype(np.float32)
    x = np.stack([shift, shift + f32(1.0)])
    for metric in (scm.L2, scm.IP):
        c = scm.Compressor(scm.Transform.null(5), metric, shift)
        for bits in (1, 2, 4):
            rows, status = c.rows(x, bits, return_status=True)
            assert not rows[0].any() and rows[1].any() and status == [scm.OK, scm.OK]
            lay = sm.FOUR_BIT_TRANSPOSED if bits == 1 else sm.SCALAR_QUANTIZED
            q = c.queries(x, bits, lay)
            assert q.shape[1] == sm.query_bytes(bits, 5, lay) and not q[0].any() and q[1].any()
    rows, status = scm.Compressor(scm.Transform.null(5), scm.L2, shift).rows(np.array([[np.nan, 0, 0, 0, 0]]), 2, True)
    assert status == [scm.NAN] and not rows.any()


def test_degenerate_query_follows_the_code():
    """one element: min == max, scale 0, (v - min) / scale = 0 / 0, a NaN bit_sum and code 0"""
    c = scm.Compressor(scm.Transform.null(1), scm.L2, np.zeros(1, np.float32))
    q = c.queries(np.array([[2.0]], np.float32), 4, sm.SCALAR_QUANTIZED)[0]
    assert q[0] == 0
    ipc, bit_sum, off, ms = sm.query_meta(q, 1)
    assert ipc == 0.0 and np.isnan(bit_sum) and np.isinf(off) and ms == f32(4.0)


def test_subsampled_transform_takes_the_norm_branch():
    rng = np.random.default_rng(8)
    signs = _signs(rng, 100)
    sub = np.sort(rng.choice(128, 96, replace=False)).astype(np.uint32)
    full = scm.Transform.padding_hadamard(signs, 128)
    part = scm.Transform.padding_hadamard(signs, 128, sub)
    assert full.preserves_norms and not part.preserves_norms and part.output_dim == 96
    x = rng.standard_normal((4, 100)).astype(np.float32)
    c = scm.Compressor(part, scm.L2, np.zeros(100, np.float32))
    t, sn, ms, tn, live, _ = c.preprocess(x)
    assert live.all() and np.array_equal(fbits(tn), fbits(np.sqrt(scm.ip_v3(t, t)))) and (tn != f32(1.0)).all()
    assert (scm.Compressor(full, scm.L2, np.zeros(100, np.float32)).preprocess(x)[3] == f32(1.0)).all()
    # the norm enters the correction: ((2 * tn) * sn) / sum|t| at 1 bit
    rows = c.rows(x, 1)
    want = ((f32(2.0) * tn) * sn) / scm.seq_sum(np.abs(t))
    got = np.array([sm.data_meta(r, 1, 96)[0] for r in rows])
    assert np.array_equal(fbits(got), fbits(want.astype(np.float16).astype(np.float32)))


def test_minimum_of_zeros_keeps_the_last_ones_sign():
    c = scm.Compressor(scm.Transform.null(4), scm.L2, np.zeros(4, np.float32))
    a = c.queries(np.array([[0.0, -0.0, 1.0, 2.0]], np.float32), 2, sm.SCALAR_QUANTIZED)[0]
    b = c.queries(np.array([[-0.0, 0.0, 1.0, 2.0]], np.float32), 2, sm.SCALAR_QUANTIZED)[0]
    off_a, off_b = sm.query_meta(a, 1)[2], sm.query_meta(b, 1)[2]
    assert off_a == 0 and off_b == 0 and np.signbit(off_a) and not np.signbit(off_b)
    assert np.array_equal(a[:1], b[:1])


def test_error_grows_as_bits_shrink():
    """mean |estimate - true squared L2| over one seeded Gaussian set falls from 1 bit to 2 bits to 4 bits (an ordering)"""
    rng = np.random.default_rng(9)
    n, dim = 48, 64
    x = rng.standard_normal((n, dim)).astype(np.float32)
    shift = x.mean(0).astype(np.float32)
    signs = _signs(rng, dim)
    true = ((x[:, None, :].astype(np.float64) - x[None, :, :]) ** 2).sum(2)
    err = {}
    for bits in (1, 2, 4):
        rows = scm.Compressor(scm.Transform.padding_hadamard(signs, dim), scm.L2, shift).rows(x, bits)
        est = sm.distance_matrix(sm.L2, rows, rows, dim, bits).astype(np.float64)
        off = ~np.eye(n, dtype=bool)
        err[bits] = float(np.abs(est - true)[off].mean())
    assert err[1] > err[2] > err[4], err


# ---- the declarations ---------------------------------------------------------------------------------------------------------
NEW = ("dann_spherical_create", "dann_spherical_destroy", "dann_spherical_shift_norm_sq", "dann_spherical_compress",
       "dann_spherical_compress_device", "dann_spherical_compress_queries", "dann_spherical_compress_queries_device")


def test_new_declarations():
    import diskann_amd as da
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "dann.h")).read()
    declared = set(re.findall(r"\b(dann_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    L = da.lib()
    for name in NEW:
        assert name in declared and name in da._ffi.SYMBOLS and getattr(L, name) is not None, name
    assert "SphericalCompressor" in da.__all__ and L.dann_abi_version() == 5
