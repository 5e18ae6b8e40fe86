"""The prologue of a locality-scheduled launch (query_schedule.hip): the key kernel (every query's nearest pivot, with
unconditional query loads on clamped addresses, and the per-block key counts) and the scatter kernel (block bases from
those counts, the stable scatter into the slot map).  The key kernel also clears the launch's spill-pool counters.

A scheduled launch only changes the order in which queries run, so it must equal the caller-order launch
(DANN_DBG_TUNE_OFF bit 128) bit for bit; the outputs start from a sentinel, so a query that the map lost shows.  The
shapes walk the edges of the code: 32-query groups and sort blocks (nq), the tail of a 16-column step, less than one
step, more than the steps held in registers, the 64-pivot slab (dim), rows that are not 16-byte aligned.  The trained
slab is held to the NumPy restatement of tests/test_gpu_sched_pivots.py: the new loads feed the old keys."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import bits, random_graph
from test_gpu_sched_pivots import _blobs, _f16, _finite_amax, _pivot_count, _scale, _seeds, _train

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

N, R, L, K = 8000, 24, 26, 10
SENTINEL = 0xA5
NQS = (1025, 2047, 2048, 2049, 4097)
_graphs = {}


def _index(data, iters=4):
    dtype = oracle.F16 if data.dtype == np.float16 else oracle.F32
    n, dim = data.shape
    if n not in _graphs:
        _graphs[n] = random_graph(np.random.default_rng(n + R), n, R)
    gix = da.Provider(dtype, oracle.L2, dim, n, R, data[:1])
    gix.set_elements(0, data)
    gix.upload_graph(_graphs[n])
    gix.debug_set(sched_min_queries=1024, pair_min_queries=1 << 30, sched_lloyd_iters=iters)
    return gix


def _device_search(gix, dq, nq, sched):
    """dann_search_batch_device into outputs pre-filled with the sentinel: (ids, distance bits, stats bytes)"""
    import torch
    gix.debug_set(tune_off=0 if sched else 128)
    di = torch.full((nq, K * 4), SENTINEL, dtype=torch.uint8, device="cuda")
    dd = torch.full((nq, K * 4), SENTINEL, dtype=torch.uint8, device="cuda")
    ds = torch.full((nq, da.STATS_DTYPE.itemsize), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    da._ffi.check(da.lib().dann_search_batch_device(gix._h, C.c_void_p(dq.data_ptr()), nq, L, 1, K,
                                                    C.c_void_p(di.data_ptr()), C.c_void_p(dd.data_ptr()),
                                                    C.c_void_p(ds.data_ptr())), "dann_search_batch_device")
    torch.cuda.synchronize()
    return di.cpu().numpy().view(np.uint32), dd.cpu().numpy().view(np.uint32), ds.cpu().numpy()


def _check(gix, dq, nq, what):
    got = _device_search(gix, dq, nq, sched=True)
    want = _device_search(gix, dq, nq, sched=False)
    sentinel = np.uint32(0x01010101) * np.uint32(SENTINEL)
    assert (want[0] != sentinel).all() and not (want[2] == SENTINEL).all(1).any(), what
    for g, w, name in zip(got, want, ("ids", "distances", "stats")):
        assert np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", [128, 100, 13, 136, 768])
def test_scheduled_launch_equals_caller_order(dtype, dim):
    import torch
    rng = np.random.default_rng(1000 + dim)
    data = _blobs(rng, dtype, N, dim)
    q = _blobs(rng, dtype, max(NQS), dim)
    gix = _index(data)
    dq = torch.from_numpy(q).cuda()
    for nq in NQS:
        _check(gix, dq, nq, f"one wave per query, nq {nq}")
    gix.set_max_concurrency(512)
    for nq in NQS:
        _check(gix, dq, nq, f"persistent waves, nq {nq}")
    gix.set_max_concurrency(0)
    assert gix.sched_pivots()[0].shape == (_pivot_count(dim), dim)


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_rows_off_a_16_byte_boundary(dtype):
    """the same queries one element into a buffer: 16-byte loads are not possible, the keys are the same"""
    import torch
    dim, nq = 128, 2049
    rng = np.random.default_rng(7)
    data = _blobs(rng, dtype, N, dim)
    q = _blobs(rng, dtype, nq, dim)
    gix = _index(data)
    flat = torch.zeros(nq * dim + 1, dtype=torch.from_numpy(q).dtype, device="cuda")
    flat[1:] = torch.from_numpy(q).cuda().reshape(-1)
    shifted = flat[1:]
    assert shifted.data_ptr() % 16 != 0
    aligned = torch.from_numpy(q).cuda()
    got = _device_search(gix, shifted, nq, sched=True)
    want = _device_search(gix, aligned, nq, sched=True)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    _check(gix, shifted, nq, "shifted rows")


@pytest.mark.parametrize("name", ["one_vector", "nan_queries"])
def test_degenerate_batches(name):
    """every query the same vector: one pivot takes the whole batch (one key in every sort block); a few NaN queries:
    no pivot wins, they take pivot 0"""
    import torch
    dim, nq = 128, 4097
    rng = np.random.default_rng(11)
    data = _blobs(rng, np.float32, N, dim)
    if name == "one_vector":
        q = np.tile(data[123:124], (nq, 1))
    else:
        q = _blobs(rng, np.float32, nq, dim)
        q[[0, 31, 32, 1000, 2047, 2048, 4096]] = np.nan
        q[77, 5] = np.nan
    gix = _index(data)
    dq = torch.from_numpy(q).cuda()
    _check(gix, dq, nq, name)
    gix.set_max_concurrency(512)
    _check(gix, dq, nq, name + ", persistent waves")


def _one_iteration(data):
    """one Lloyd iteration on an index whose slots are all live, restated like `_train(data, 1, "f16")` of
    tests/test_gpu_sched_pivots.py, except where that restatement is arbitrary: it scores in f32 in NumPy's order, the
    key kernel in f32 in the matrix cores' order, and a sample row whose two nearest centres lie closer than the
    rounding of either evaluation may go to either.  Scores here are exact (f64 on f16 operands: every product and sum
    is exact), `slack` bounds what an f32 evaluation in any order can be off by (n roundings of 2^-24 on sums of at
    most sum |q_i c_i|, resp. sum c_i^2, and the final subtraction), and a row is `open` to every centre whose score
    could come out lowest.  Returns (scale, per centre the set of acceptable slab rows as bytes, rows open to several).
    The means are `_train`'s: the members in sample order, added in f32, divided, scaled, rounded to f16."""
    n, dim = data.shape
    P = _pivot_count(dim)
    seeds = _seeds(data, P)
    S = min(64 * P, n)
    sample = data[[j * n // S for j in range(S)]].astype(np.float32)
    scale = _scale(max(_finite_amax(sample), _finite_amax(seeds)))
    c = _f16(seeds * scale)
    q = _f16(sample * scale).astype(np.float64)
    c64 = c.astype(np.float64)
    norms = (c64 * c64).sum(1)
    score = norms[None, :] - 2.0 * (q @ c64.T)
    slack = dim * 2.0 ** -24 * (2.0 * (np.abs(q) @ np.abs(c64).T) + norms[None, :]) + 2.0 ** -22 * np.abs(score)
    best = score.argmin(1)
    rows = np.arange(S)
    could_win = score - slack <= (score[rows, best] + slack[rows, best])[:, None]
    several = could_win.sum(1) > 1
    accept = []
    for p in range(P):
        sure = np.flatnonzero(could_win[:, p] & ~several)
        maybe = np.flatnonzero(could_win[:, p] & several)
        assert len(maybe) <= 8, (p, len(maybe))
        rows_p = set()
        for pick in range(1 << len(maybe)):
            members = np.sort(np.concatenate([sure, maybe[[(pick >> i) & 1 == 1 for i in range(len(maybe))]]]).astype(np.int64))
            row = c[p]
            if len(members):
                total = np.zeros(dim, np.float32)
                for i in members:
                    total = total + sample[i]
                m = (total / np.float32(len(members)) * scale).astype(np.float16)
                if np.isfinite(m).all():
                    row = m.astype(np.float32)
            rows_p.add((row / scale).astype(np.float32).tobytes())
        accept.append(rows_p)
    return scale, accept, int(several.sum())


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", [100, 136])
def test_one_lloyd_iteration_matches_numpy(dtype, dim):
    """DANN_DBG_SCHED_LLOYD_ITERS = 1: every centre of the slab equals the restatement of one iteration, bit for bit
    after f16 rounding (the key pass assigns the sample rows through the same kernel as the queries, and the counting
    sort orders the members whose f32 sums the centres are).  Against `_train(data, 1, "f16")` as it stands this data
    gives, at dim 136, 254 of 256 centres: sample row 7291 lies 2.34 from centres 38 and 106 at scores of 1.6e6,
    NumPy's own f32 scores put it at the other centre than exact ones do, and the library sides with the exact ones
    (as the parent commit's library does: the two slabs are byte-identical).  `_one_iteration` leaves such a row to
    either centre and nothing else open; where no row is that close (dim 100 here) it is `_train` itself."""
    import torch
    rng = np.random.default_rng(dim)
    data = _blobs(rng, dtype, N, dim)
    gix = _index(data, iters=1)
    dq = torch.from_numpy(_blobs(rng, dtype, 1025, dim)).cuda()
    _check(gix, dq, 1025, "search")
    piv, scale = gix.sched_pivots()
    wscale, accept, several = _one_iteration(data)
    strict, _ = _train(data, 1, "f16")
    assert scale == wscale
    off = [p for p in range(len(piv)) if piv[p].tobytes() not in accept[p]]
    print(f"dim {dim}: {several} sample rows open to several centres; centres unlike _train: "
          f"{np.flatnonzero((bits(piv) != bits(strict)).any(1)).tolist()}; centres outside the restatement: {off}")
    assert not off
