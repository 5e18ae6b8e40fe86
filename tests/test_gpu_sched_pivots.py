"""The pivots of the locality scheduling (query_schedule.hip) are centres: rows taken at a fixed stride over the live
slots, moved by DANN_DBG_SCHED_LLOYD_ITERS Lloyd iterations over a sample of the rows.  dann_debug_sched_pivots hands
them out; `_train` restates the training in NumPy.  Pivots only ever decide the order in which queries run: every
scheduled launch here is also compared, bit for bit, with the caller-order launch (DANN_DBG_TUNE_OFF bit 128)."""
import numpy as np
import pytest

import oracle
from helpers import bits, random_graph

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

ITERS = 4
_graphs = {}


def _pivot_count(dim):
    stride = (dim + 15) // 16 * 16 + 8
    return min(256, (144 * 1024 - 16) // (stride * 2 + 4) // 32 * 32)


def _graph(n, R):
    if (n, R) not in _graphs:
        _graphs[n, R] = random_graph(np.random.default_rng(n + R), n, R)
    return _graphs[n, R]


def _index(data, R=24):
    dtype = oracle.F16 if data.dtype == np.float16 else oracle.F32
    n, dim = data.shape
    gix = da.Provider(dtype, oracle.L2, dim, n, R, data[:1])
    gix.set_elements(0, data)
    gix.upload_graph(_graph(n, R))
    gix.debug_set(sched_min_queries=1024, pair_min_queries=1 << 30, sched_lloyd_iters=ITERS)
    return gix


def _search(gix, q, sched, L=26, k=10):
    gix.debug_set(tune_off=0 if sched else 128)
    return gix.search(da.Knn(L), q, k)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def _blobs(rng, dtype, n, dim, nblobs=300):
    """more blobs than pivots, of unequal sizes: rows at a fixed stride miss some of them"""
    centres = rng.uniform(0, 100, (nblobs, dim)).astype(np.float32)
    w = rng.uniform(0.2, 5.0, nblobs)
    x = centres[rng.choice(nblobs, n, p=w / w.sum())] + rng.normal(0, 4, (n, dim)).astype(np.float32)
    return x.astype(dtype)


def _finite_amax(x):
    a = np.abs(x[np.isfinite(x)])
    return np.float32(a.max()) if a.size else np.float32(0)


def _scale(amax):
    return np.float32(2.0 ** (8 - int(np.ceil(np.log2(float(amax)))))) if amax > 0 else np.float32(1)


def _seeds(data, P):
    """the documented rule, every slot live: pivot j starts as the row of slot j * n // P"""
    n = len(data)
    return data[[j * n // P for j in range(P)]].astype(np.float32)


def _f16(x):
    return x.astype(np.float16).astype(np.float32)


def _train(data, iters, assign):
    """the library's training on an index whose n slots are all live: (centres as the slab holds them, unscaled; scale).
    assign = "f16": nearest centre on f16-rounded scaled operands, as the key pass; "f32": on the unrounded sample."""
    n, dim = data.shape
    P = _pivot_count(dim)
    seeds = _seeds(data, P)
    if iters == 0:
        scale = _scale(_finite_amax(seeds))
        return _f16(np.where(np.isfinite(seeds), seeds, 0) * scale) / scale, scale
    S = min(64 * P, n)
    sample = data[[j * n // S for j in range(S)]].astype(np.float32)
    scale = _scale(max(_finite_amax(sample), _finite_amax(seeds)))
    c = _f16(np.where(np.isfinite(seeds), seeds, 0) * scale)
    fin = np.isfinite(sample).all(1)
    with np.errstate(all="ignore"):
        q = sample * scale
        if assign == "f16":
            q = _f16(q)
    for _ in range(iters):
        with np.errstate(all="ignore"):
            score = (c * c).sum(1, dtype=np.float32)[None, :] - np.float32(2) * (q @ c.T)
        key = np.where(np.isnan(score).all(1), 0, np.argmin(np.where(np.isnan(score), np.inf, score), axis=1))
        for p in range(P):
            members = sample[(key == p) & fin]
            if len(members) == 0:
                continue
            s = np.zeros(dim, np.float32)
            for row in members:  # in sample order, in f32
                s = s + row
            m = (s / np.float32(len(members)) * scale).astype(np.float16)
            if np.isfinite(m).all():
                c[p] = m.astype(np.float32)
    return c / scale, scale


def _objective(data, centres):
    """mean squared distance of every row to its nearest centre (f64)"""
    x, c = data.astype(np.float64), centres.astype(np.float64)
    d2 = (x * x).sum(1)[:, None] - 2.0 * (x @ c.T) + (c * c).sum(1)[None, :]
    return float(d2.min(1).mean())


@pytest.mark.parametrize("dtype,n,dim", [(np.float32, 8000, 128), (np.float16, 8000, 64), (np.float32, 3000, 768)])
def test_training_improves_the_objective_and_matches_numpy(dtype, n, dim):
    """ITERS Lloyd iterations from the stride rows: the mean squared row-to-nearest-pivot distance falls below that of
    the stride rows themselves, and equals that of the NumPy restatement within twice the gap between the restatement
    assigning on f16-rounded scaled operands (as the key pass does) and on f32 operands -- the only inexact step: sums
    and means are the same f32 operations in the same order.  Computed on the CPU for these inputs (objective of the
    restatement / of the stride rows / tolerance = twice the gap): f32 dim 128: 20360.60 / 59100.80 / 0.0232; f16 dim 64:
    10031.61 / 26207.49 / 0 and f32 dim 768: 444356.14 / 896529.64 / 0 -- f16 rounding moves no row of these two to another
    centre, so they ask for the restatement's objective exactly."""
    rng = np.random.default_rng(dim)
    data = _blobs(rng, dtype, n, dim)
    q = _blobs(rng, dtype, 2048, dim)
    gix = _index(data)
    got = _search(gix, q, sched=True)
    piv, scale = gix.sched_pivots()
    assert piv.shape == (_pivot_count(dim), dim) and np.isfinite(piv).all()
    assert _same(got, _search(gix, q, sched=False))

    rows = _index(data)
    rows.debug_set(sched_lloyd_iters=0)
    _search(rows, q, sched=True)
    stride_piv, _ = rows.sched_pivots()

    c16, s16 = _train(data, ITERS, "f16")
    c32, _ = _train(data, ITERS, "f32")
    assert scale == s16
    o_gpu, o_rows, o16, o32 = (_objective(data, c) for c in (piv, stride_piv, c16, c32))
    tol = 2.0 * abs(o16 - o32)
    print(f"objective: gpu {o_gpu:.6f} numpy(f16) {o16:.6f} numpy(f32) {o32:.6f} stride rows {o_rows:.6f} tol {tol:.6f}")
    assert o_gpu < o_rows
    assert abs(o_gpu - o16) <= tol, (o_gpu, o16, o32, tol)


def test_training_is_deterministic_and_follows_mutations():
    rng = np.random.default_rng(21)
    n, dim = 4000, 64
    data = _blobs(rng, np.float32, n, dim)
    q = _blobs(rng, np.float32, 3000, dim)
    a, b = _index(data), _index(data)
    ra, rb = _search(a, q, sched=True), _search(b, q, sched=True)
    (pa, sa), (pb, sb) = a.sched_pivots(), b.sched_pivots()
    assert sa == sb and np.array_equal(bits(pa), bits(pb))
    assert _same(ra, rb)
    a.set_elements(0, _blobs(rng, np.float32, 100, dim))
    after = _search(a, q, sched=True)
    pa2, _ = a.sched_pivots()
    assert not np.array_equal(bits(pa), bits(pa2))
    assert not after[2]["status"].any()
    assert _same(after, _search(a, q, sched=False))


def _degenerate(name):
    rng = np.random.default_rng(33)
    if name == "few_rows":
        return rng.uniform(0, 100, (100, 64)).astype(np.float32)
    if name == "identical_rows":
        return np.tile(rng.uniform(0, 100, (1, 64)).astype(np.float32), (3000, 1))
    if name == "nan_and_inf":
        data = _blobs(rng, np.float32, 4000, 64)
        data[15, 3] = np.inf  # (every slot of an index of fewer than 64 x 256 rows is a sample row; slot 15 is stride row 1 too)
        data[1, 5] = np.nan
        data[2, 7] = np.inf
        return data
    assert name == "f16_near_max"
    return rng.uniform(-60000, 60000, (4000, 64)).astype(np.float16)


@pytest.mark.parametrize("name", ["few_rows", "identical_rows", "nan_and_inf", "f16_near_max"])
def test_degenerate_inputs(name):
    data = _degenerate(name)
    rng = np.random.default_rng(34)
    q = data[rng.integers(0, len(data), 2048)].astype(np.float32) + rng.normal(0, 1, (2048, data.shape[1])).astype(np.float32)
    q = np.clip(np.nan_to_num(q, nan=0.0, posinf=0.0), -65000, 65000).astype(data.dtype)
    gix = _index(data)
    got = _search(gix, q, sched=True)
    assert _same(got, _search(gix, q, sched=False))
    piv, scale = gix.sched_pivots()
    assert np.isfinite(piv).all() and np.isfinite(scale) and scale > 0
    if name == "identical_rows":
        assert np.allclose(piv, data[0], rtol=2e-3)
    if name == "nan_and_inf":  # the stride rows themselves: the non-finite coordinate of row 15 is stored as 0
        rows = _index(data)
        rows.debug_set(sched_lloyd_iters=0)
        assert _same(got, _search(rows, q, sched=True))
        piv0, scale0 = rows.sched_pivots()
        want, wscale = _train(data, 0, "f16")
        assert scale0 == wscale and piv0[1, 3] == 0 and np.array_equal(bits(piv0), bits(want))


@pytest.mark.parametrize("dtype,n,dim", [(np.float32, 4000, 128), (np.float16, 5000, 64), (np.float32, 100, 64)])
def test_no_iterations_leave_the_stride_rows(dtype, n, dim):
    rng = np.random.default_rng(n)
    data = _blobs(rng, dtype, n, dim)
    q = _blobs(rng, dtype, 2048, dim)
    gix = _index(data)
    gix.debug_set(sched_lloyd_iters=0)
    got = _search(gix, q, sched=True)
    piv, scale = gix.sched_pivots()
    want, wscale = _train(data, 0, "f16")
    assert scale == wscale
    assert np.array_equal(bits(piv), bits(want))
    assert _same(got, _search(gix, q, sched=False))
