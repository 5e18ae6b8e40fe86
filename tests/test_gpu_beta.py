"""dann_beta_search_batch(_device): BetaFilter search (layers/betafilter.rs) against tests/beta_model.py, bit for bit -- ids,
distance bits, cmps, hops.  The model's plain distances come from the library's bit-exact seams (dann_expand_beam_batch over
every slot; the oracle's expand_beam for PQ codes, which that seam does not take).  One graph, built on the GPU over the
f32 rows, serves every row type."""
import functools

import numpy as np
import pytest

import beta_model as bm
import oracle
from helpers import bits
from search_builders import SqBitsCase

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")
N, DIM, R, NQ, K = 2000, 40, 16, 16, 10
SLOTS = np.arange(N + 1, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def _graph():
    data = np.random.default_rng(7).uniform(-1, 1, (N, DIM)).astype(np.float32)
    p = da.Provider(da.F32, da.L2, DIM, N, R, data.mean(0, keepdims=True))
    p.set_elements(0, data)
    p.build(da.build_config(R, R, 32), 0, N)
    return data, p.download_graph()


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(provider, queries, plain[NQ, slots], adj, readable or None), made once per kind"""
    data, adj = _graph()
    rng = np.random.default_rng(11)
    q = rng.uniform(-1, 1, (NQ, DIM)).astype(np.float32)
    readable = plain = None
    if kind in ("f32_l2", "f32_ip"):
        gix = da.Provider(da.F32, da.L2 if kind == "f32_l2" else da.INNER_PRODUCT, DIM, N, R, data.mean(0, keepdims=True))
        gix.set_elements(0, data)
    elif kind in ("sq4", "sq4_tags"):
        c = SqBitsCase(4, da.L2, N, DIM, R, 5, adj=False, tags=kind == "sq4_tags")
        gix, q = c.gix, c.queries(NQ)[1]
    else:
        bounds = np.linspace(0, DIM, 9).round().astype(np.uint32)
        pivots = rng.standard_normal((256, DIM)).astype(np.float32)
        codes, start = rng.integers(0, 256, (N, 8), dtype=np.uint8), rng.integers(0, 256, (1, 8), dtype=np.uint8)
        oix = oracle.Index(oracle.PQ, oracle.L2, DIM, N, R, start, pq_pivots=pivots, pq_offsets=bounds)
        oix.set_rows(0, codes)
        gix = da.Provider(da.PQ, da.L2, DIM, N, R, start, pq_pivots=pivots, pq_offsets=bounds)
        gix.set_elements(0, codes)
        plain = np.stack([oix.expand_beam(x, SLOTS)[1] for x in q])
    gix.upload_graph(adj)
    if plain is None:
        plain = gix.expand_beam_batch(q, np.tile(SLOTS, NQ), np.arange(NQ + 1, dtype=np.uint64) * SLOTS.size).reshape(NQ, -1)
    if kind == "sq4_tags":  # every 7th slot unreadable (OWNED), after the table was taken from the published rows
        readable = np.ones(N + 1, bool)
        readable[3:N:7] = False
        for s in np.flatnonzero(~readable):
            gix.set_tags(int(s), [1])
    assert plain.shape == (NQ, N + 1) and np.isfinite(plain).all()
    return gix, q, plain, adj, readable


def _match(shared, start_bit):
    m = np.random.default_rng(23).random((1 if shared else NQ, N + 1)) < 0.3
    m[:, N] = start_bit
    return m[0] if shared else m


def _check(kind, got, L, W, match, beta, tag):
    _, _, plain, adj, readable = _case(kind)
    (gi, gd, gst), fam = got
    assert fam == {tag} and not gst["status"].any(), (fam, tag)
    for i in range(NQ):
        d = bm.apply_beta(plain[i], match if match.ndim == 1 else match[i], beta)
        wi, wd, wc, wh = bm.knn(d, adj, N, 1, L, W, K, readable)
        assert np.array_equal(gi[i], wi) and np.array_equal(bits(gd[i]), bits(wd)), (tag, i)
        assert (gst["cmps"][i], gst["hops"][i]) == (wc, wh), (tag, i)


@pytest.mark.parametrize("beta", [0.25, 4.0])
@pytest.mark.parametrize("shared,start_bit", [(True, True), (False, False)])
@pytest.mark.parametrize("L,W", [(24, 1), (70, 2)])
@pytest.mark.parametrize("kind", ["f32_l2", "f32_ip", "sq4", "pq"])
def test_beta_search_equals_the_model(kind, L, W, shared, start_bit, beta):
    gix, q = _case(kind)[:2]
    match = _match(shared, start_bit)
    run = lambda: gix.beta_search(da.Knn(L, W), q, K, match, beta)
    # thresholds at which a plain launch of this size is paired or takes a team where it has the shape (and PQ rows of 8
    # chunks have the table-in-registers kernel): a beta launch is one wave per query, or persistent waves under a cap
    gix.debug_set(pair_min_queries=1, team_max_queries=1 << 20)
    try:
        _check(kind, gix.last_family(run), L, W, match, beta, "one_wave")
        gix.set_max_concurrency(5)  # 16 queries over 5 persistent waves: the loop, its tickets, an uneven share
        _check(kind, gix.last_family(run), L, W, match, beta, "persistent")
    finally:
        gix.set_max_concurrency(0)
        gix.debug_set(pair_min_queries=None, team_max_queries=None)


@pytest.mark.parametrize("kind", ["f32_ip", "sq4", "pq"])
def test_beta_one_or_no_match_is_the_plain_search(kind):
    gix, q = _case(kind)[:2]
    for L, W in ((24, 1), (70, 2)):
        pi, pd, pst = gix.search(da.Knn(L, W), q, K)
        for match, beta in ((_match(True, True), 1.0), (np.zeros(N + 1, bool), 4.0)):
            gi, gd, gst = gix.beta_search(da.Knn(L, W), q, K, match, beta)
            assert np.array_equal(gi, pi) and np.array_equal(bits(gd), bits(pd))
            assert all(np.array_equal(gst[f], pst[f]) for f in ("cmps", "hops", "result_count", "written", "status"))


def test_device_form_and_inline_tags():
    torch = pytest.importorskip("torch")
    gix, q, _, _, readable = _case("sq4_tags")
    match = _match(False, True)
    host = gix.last_family(lambda: gix.beta_search(da.Knn(24, 2), q, K, match, 0.25))
    _check("sq4_tags", host, 24, 2, match, 0.25, "one_wave")
    assert readable[host[0][0]].all()
    f, keep = gix._filter(0, match, NQ)
    dq, db = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q.view(np.uint8), keep.view(np.int32)))
    di = torch.zeros((NQ, K), dtype=torch.int32, device="cuda")
    dd = torch.zeros((NQ, K), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    da._ffi.check(da.lib().dann_beta_search_batch_device(gix._h, dq.data_ptr(), NQ, 24, 2, K, db.data_ptr(), f.stride_words, 0.25,
                                                         di.data_ptr(), dd.data_ptr(), None), "dann_beta_search_batch_device")
    assert np.array_equal(di.cpu().numpy().view(np.uint32), host[0][0])
    assert np.array_equal(bits(dd.cpu().numpy()), bits(host[0][1]))


def test_parameter_errors():
    gix, q = _case("f32_l2")[:2]
    match = _match(True, True)

    def status(fn):
        try:
            return fn() and 0
        except da._ffi.DannError as e:
            return e.status

    assert status(lambda: gix.beta_search(da.Knn(24, 1), q, K, match, float("nan"))) == da._ffi.EINVAL
    for k in (0, 30):  # k == 0 and k > L: whatever the plain search answers
        assert status(lambda: gix.beta_search(da.Knn(24, 1), q, k, match, 0.5)) == status(lambda: gix.search(da.Knn(24, 1), q, k))
    o, d = np.zeros((NQ, K), np.uint32), np.zeros((NQ, K), np.float32)
    assert da.lib().dann_beta_search_batch(gix._h, q.ctypes.data, NQ, 24, 1, K, None, 0, 0.5, o.ctypes.data, d.ctypes.data,
                                           None) == da._ffi.EINVAL
