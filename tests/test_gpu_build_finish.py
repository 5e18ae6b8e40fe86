"""dann_medoid(_device), dann_count_reachable, dann_degree_stats and dann_prune_range on the GPU against the CPU
restatement (tests/build_finish_model.py), bit for bit: the mean's bits and the first-minimum row over dtypes, sizes,
strides and both entries, ties, NaNs and both summation paths; the reference's known answers
(tests/golden/build_finish_cases.json); random, chain and hub graphs; and prune_range over oracle-built indexes of every
row type, the matrix-core path, both tie orders, subsets, repeats and inline tags."""
import ctypes as C

import numpy as np
import pytest

import oracle
import build_finish_model as model
from gridutil import grid_data
from helpers import bits, make_pair, rand_vectors, random_graph
from test_build_finish_host import adversarial_column, fixture_index, golden
from test_consolidate_host import square_cfg

pytestmark = pytest.mark.gpu
da = pytest.importorskip("diskann_amd")

from test_gpu_consolidate import ODT, ROW_CASES, data_for, same_graph, valid_rows  # noqa: E402

NP_OF = {da.F32: np.float32, da.F16: np.float16, da.U8: np.uint8, da.I8: np.int8}
STORE_STRIDE = 544


def rows_of(rng, dtype, n, dim):
    if dtype == da.U8:
        return rng.integers(0, 256, (n, dim), dtype=np.uint8)
    if dtype == da.I8:
        return rng.integers(-128, 128, (n, dim), dtype=np.int8)
    return rng.normal(size=(n, dim)).astype(NP_OF[dtype])


def strided(x, stride=STORE_STRIDE):
    """the rows in a store of `stride`-byte rows, the bytes behind a row filled with 0xFF (they are not part of it)"""
    raw = np.full((x.shape[0], stride), 255, np.uint8)
    raw[:, :x.shape[1] * x.itemsize] = np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], -1)
    return raw


def run_medoid(x, dtype, how):
    """how: host / host_strided / device / device_strided -> (row, mean (numpy), counters)"""
    import torch
    if how == "host":
        return da.medoid(x)
    if how == "host_strided":
        return da.medoid(strided(x), dtype=dtype, dim=x.shape[1])
    if how == "device":
        t = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], -1).copy()).cuda()
        row, mean, cnt = da.medoid(t, dtype=dtype, dim=x.shape[1])
    else:
        t = torch.from_numpy(strided(x)).cuda()
        row, mean, cnt = da.medoid(t, dtype=dtype, dim=x.shape[1])
    return row, mean.cpu().numpy(), cnt


def check_medoid(x, dtype, hows, want=None):
    want = model.medoid(x) if want is None else want
    out = None
    for how in hows:
        row, mean, cnt = run_medoid(x, dtype, how)
        assert row == want[0], (how, row, want[0])
        assert np.array_equal(bits(mean), bits(want[1])), how
        assert cnt[2] == x.shape[0] and cnt[3] == want[2], (how, cnt)
        assert cnt[0] + cnt[1] == x.shape[1] * -(-x.shape[0] // model.RANGE_ROWS)
        out = cnt
    return out


# ---- 1. the medoid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [da.F32, da.F16, da.U8, da.I8])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097])
def test_medoid_matches_model(dtype, n):
    rng = np.random.default_rng(1000 * dtype + n)
    for i, dim in enumerate([1, 5, 32, 100, 128, 131]):
        x = rows_of(rng, dtype, n, dim)
        # every size through all four routes where it is cheap; the large ones alternate
        hows = ("host", "host_strided", "device", "device_strided") if n <= 65 else \
            (("host", "device_strided") if i % 2 == 0 else ("host_strided", "device"))
        check_medoid(x, dtype, hows)


def test_medoid_through_a_torch_tensor_and_an_index_store():
    import torch
    rng = np.random.default_rng(3)
    x = rng.normal(size=(777, 128)).astype(np.float32)
    want = model.medoid(x)
    row, mean, _ = da.medoid(torch.from_numpy(x).cuda())
    assert row == want[0] and np.array_equal(bits(mean.cpu().numpy()), bits(want[1]))
    # the index's own store: 544-byte rows through dann_index_device_pointers
    gix = da.Provider(da.F32, da.L2, 128, 777, 8, x[:1], row_stride=STORE_STRIDE)
    gix.set_elements(0, x)
    rows_ptr, _ = gix.device_pointers()
    out_row, cnt = C.c_int64(-2), np.zeros(4, np.uint64)
    da._ffi.check(da.lib().dann_medoid_device(gix.device, da.F32, C.c_void_p(rows_ptr), 777, 128, STORE_STRIDE,
                                              C.byref(out_row), None, cnt.ctypes.data_as(C.c_void_p)), "dann_medoid_device")
    assert out_row.value == want[0] and cnt[2] == 777


@pytest.mark.parametrize("dtype", [da.F32, da.U8])
def test_medoid_ties_keep_the_earlier_row(dtype):
    """identical nearest rows at (0, n - 1), (63, 64) and across a workgroup boundary of the scan (32 rows per workgroup
    and pass: rows 31 | 32; 2048 workgroups: rows 65535 | 65536 lie one pass apart)"""
    rng = np.random.default_rng(7)
    dim = 32
    for n, (a, b) in [(500, (0, 499)), (500, (63, 64)), (500, (31, 32)), (66000, (65535, 65536))]:
        x = rng.integers(40, 216, (n, dim)).astype(NP_OF[dtype])
        mean = np.round(model.column_sums(x) / n).astype(NP_OF[dtype])
        x[a] = mean
        x[b] = mean
        want = model.medoid(x)
        assert want[0] == a
        check_medoid(x, dtype, ("host", "device"), want)


def test_medoid_nan_and_empty():
    rng = np.random.default_rng(9)
    x = rng.normal(size=(300, 20)).astype(np.float32)
    # a NaN makes the mean NaN, so every distance is: nothing wins, as in the reference
    y = x.copy()
    y[17, 3] = np.nan
    want = model.medoid(y)
    assert want[0] == -1 and want[2] == 300
    check_medoid(y, da.F32, ("host", "device"), want)
    check_medoid(np.full((70, 5), np.nan, np.float32), da.F32, ("host", "device"))
    # no rows: no row wins, and the mean is the zero vector
    row, mean, cnt = da.medoid(np.zeros((0, 8), np.float16))
    assert row == -1 and not mean.any() and not cnt.any()
    # infinite distances never win either: f32::MAX is the bar
    big = np.full((4, 3), 3e38, np.float32)
    big[1] = -3e38
    want = model.medoid(big)
    check_medoid(big, da.F32, ("host", "device"), want)


def test_medoid_nan_row_is_skipped():
    """one row's distance is NaN and the others' are not.  A NaN element makes the whole column's mean NaN, so a lone NaN
    distance needs an infinite mean component: row 0 holds +inf there (inf - inf = NaN), every other row is infinitely
    far, and f32::MAX is the bar -- the NaN is counted, and neither it nor an infinite distance wins"""
    x = np.zeros((5, 2), np.float32)
    x[:, 0] = [np.inf, 1, 2, 3, 4]
    want = model.medoid(x)
    assert want[0] == -1 and want[2] == 1
    check_medoid(x, da.F32, ("host", "device"), want)


def test_medoid_summation_paths():
    rng = np.random.default_rng(11)
    u8 = rng.integers(0, 256, (4097, 33), dtype=np.uint8)
    assert check_medoid(u8, da.U8, ("host",))[1] == 0
    grid = (np.round(rng.normal(size=(4097, 33)) * 1024) / 1024).astype(np.float32)
    assert model.walk_counters(grid)[1] == 0
    assert check_medoid(grid, da.F32, ("device",))[1] == 0
    f16 = rng.normal(size=(4097, 9)).astype(np.float16)
    assert check_medoid(f16, da.F16, ("host",))[1] == 0
    # the adversarial column: the ranges that would round are walked row by row, and the sum is the sequential one
    adv = np.zeros((1002, 3), np.float32)
    adv[:, 1] = adversarial_column()
    adv[:, 2] = 1.0
    par, ser = model.walk_counters(adv)
    assert ser > 0
    want = model.medoid(adv)
    assert want[1][1] == 0.0
    cnt = check_medoid(adv, da.F32, ("host", "device"), want)
    assert (cnt[0], cnt[1]) == (par, ser)
    # standard-normal f32: whether a range fails is decided here, by the restatement of the header's test
    normal = rng.normal(size=(4097, 16)).astype(np.float32)
    par, ser = model.walk_counters(normal)
    cnt = check_medoid(normal, da.F32, ("host",))
    assert (cnt[0], cnt[1]) == (par, ser)
    wild = (rng.normal(size=(3000, 4)) * 10.0 ** rng.integers(-12, 12, (3000, 4))).astype(np.float32)
    par, ser = model.walk_counters(wild)
    assert ser > 0
    cnt = check_medoid(wild, da.F32, ("device_strided",))
    assert (cnt[0], cnt[1]) == (par, ser)


def test_medoid_errors():
    x = np.zeros((4, 8), np.float32)
    L = da.lib()
    row, cnt = C.c_int64(0), np.zeros(4, np.uint64)
    p = x.ctypes.data_as(C.c_void_p)
    for fn in (L.dann_medoid, L.dann_medoid_device):
        assert fn(0, da.SQ8, p, 4, 8, 0, C.byref(row), None, None) == da._ffi.EUNSUPPORTED
        assert fn(0, 99, p, 4, 8, 0, C.byref(row), None, None) == da._ffi.EUNSUPPORTED
        assert fn(0, da.F32, p, 4, 0, 0, C.byref(row), None, None) == da._ffi.EINVAL
        assert fn(0, da.F32, p, 4, 8, 31, C.byref(row), None, None) == da._ffi.EINVAL  # stride below the row's 32 bytes
        assert fn(0, da.F32, p, 4, 8, 34, C.byref(row), None, None) == da._ffi.EINVAL  # not a multiple of the element
        assert fn(0, da.F32, p, 4, 8, 0, None, None, None) == da._ffi.EINVAL


# ---- 2. reachability ----------------------------------------------------------------------------------------------------------
def graph_pair(adj, R, nstart=1):
    """(oracle.Index, Provider) over an adjacency alone (1-d rows that nothing reads)"""
    n = adj.shape[0] - nstart
    data = np.zeros((n, 1), np.float32)
    return make_pair(oracle.F32, oracle.L2, data, adj, np.zeros((nstart, 1), np.float32), R)


def check_reachable(oix, gix, starts=None):
    want = model.count_reachable(oix, starts)
    count, levels, reached = gix.count_reachable(starts, bitmap=True)
    assert (count, levels) == want[:2]
    assert np.array_equal(reached, want[2]) and int(reached.sum()) == count
    assert gix.count_reachable(starts) == want[:2]
    return want


@pytest.mark.parametrize("case", golden()["reachable"], ids=lambda c: f"{c['graph']}-{c['starts']}")
def test_reachable_known_answers(case):
    g = golden()
    oix, deg = fixture_index(g, case["graph"])
    gix = da.Provider(da.F32, da.L2, 2, 4, deg, np.array(g["start_point"], np.float32))
    gix.upload_graph(oix.adj)
    assert check_reachable(oix, gix, case["starts"])[0] == case["count"]
    assert gix.count_reachable(case["starts"] + case["starts"])[0] == case["count"]


def test_reachable_random_digraph_with_unreachable_nodes():
    rng = np.random.default_rng(21)
    n, R = 5000, 8
    adj = np.zeros((n + 1, R + 1), np.uint32)
    for v in range(n + 1):
        ln = int(rng.integers(0, 4))  # 1.5 out-edges on average: 2918 of the 5001 nodes are reachable
        adj[v, 0] = ln
        adj[v, 1:1 + ln] = rng.choice(n, ln, replace=False)
    adj[n, 0] = R
    adj[n, 1:] = rng.choice(n, R, replace=False)
    oix, gix = graph_pair(adj, R)
    want = check_reachable(oix, gix)  # default starts: the start point
    assert want[0] == 2918, "the density is meant to leave nodes unreachable"
    check_reachable(oix, gix, [0, 17, 17, n, 0, 4999])  # several starts, with duplicates
    check_reachable(oix, gix, [3])


def test_reachable_chain_of_3000_levels():
    n, R = 3000, 4
    adj = np.zeros((n + 1, R + 1), np.uint32)
    adj[n, :2] = [1, 0]
    for v in range(n - 1):
        adj[v, :2] = [1, v + 1]
    oix, gix = graph_pair(adj, R)
    want = check_reachable(oix, gix)
    assert want[:2] == (n + 1, n)


def test_reachable_hub_races_are_exact():
    """4000 nodes all list the same 8 targets: every claim of a level races for the same eight bits"""
    n, R = 4008, 64
    adj = np.zeros((n + 64, R + 1), np.uint32)  # 64 start points, each listing 64 of the 4000
    hubs = np.arange(4000, 4008, dtype=np.uint32)
    for v in range(4000):
        adj[v, 0] = 8
        adj[v, 1:9] = hubs
    for s in range(64):
        adj[n + s, 0] = R
        adj[n + s, 1:] = (np.arange(64) * 64 + s) % 4000
    oix, gix = graph_pair(adj, R, nstart=64)
    want = model.count_reachable(oix)
    assert want[:2] == (64 + 4000 + 8, 2)  # the start points list every one of the 4000
    for _ in range(10):
        count, levels, reached = gix.count_reachable(bitmap=True)
        assert (count, levels) == want[:2] and np.array_equal(reached, want[2])


def test_reachable_bounds_and_clamped_length():
    rng = np.random.default_rng(23)
    n, R = 200, 8
    adj = random_graph(rng, n, R)
    adj[5, 0] = R + 9  # a length word past max_degree is clamped (Neighbors::get)
    oix, gix = graph_pair(adj, R)
    check_reachable(oix, gix, [5])
    with pytest.raises(da.DannError) as e:
        gix.count_reachable([n + 1])
    assert e.value.status == da._ffi.EBOUNDS
    gix.set_neighbors(int(adj[n, 1]), [n + 7])  # dann_set_neighbors admits an id past the last slot; the walk finds it
    with pytest.raises(da.DannError) as e:
        gix.count_reachable()
    assert e.value.status == da._ffi.EBOUNDS


# ---- 3. degree statistics ------------------------------------------------------------------------------------------------------
def check_degree(oix, gix, ids=None, deleted=None):
    want = model.degree_stats(oix, ids, deleted)
    s = gix.degree_stats(ids, skip_deleted=deleted is not None)
    got = (s.max_degree, np.float32(s.avg_degree), s.min_degree, s.cnt_less_than_two, s.points, s.total)
    assert got[:1] + got[2:] == want[:1] + want[2:], (got, want)
    assert bits(got[1]) == bits(want[1])
    return s


@pytest.mark.parametrize("case", golden()["degree_stats"], ids=lambda c: c["graph"])
def test_degree_stats_known_answers(case):
    g = golden()
    oix, deg = fixture_index(g, case["graph"])
    gix = da.Provider(da.F32, da.L2, 2, 4, deg, np.array(g["start_point"], np.float32))
    gix.upload_graph(oix.adj)
    s = check_degree(oix, gix)
    assert [s.max_degree, s.avg_degree, s.min_degree, s.cnt_less_than_two] == case["expected"]


def test_degree_stats_random_subsets_and_deleted():
    rng = np.random.default_rng(31)
    n, R = 3001, 20
    adj = random_graph(rng, n, R, min_len=0)
    adj[7, 0] = R + 3  # clamped
    oix, gix = graph_pair(adj, R)
    check_degree(oix, gix)
    ids = rng.integers(0, n + 1, 777)  # repeats count each time; the start point may be asked for
    check_degree(oix, gix, np.concatenate([ids, ids[:100]]))
    empty = gix.degree_stats(np.zeros(0, np.uint32))
    assert (empty.max_degree, empty.avg_degree, empty.min_degree, empty.cnt_less_than_two, empty.points) == (0, 0.0, 0, 0, 0)
    deleted = np.zeros(n + 1, bool)
    check_degree(oix, gix, None, deleted)  # the flag before anything was deleted
    deleted[rng.choice(n, 400, replace=False)] = True
    gix.delete_points(np.flatnonzero(deleted))
    check_degree(oix, gix, None, deleted)
    check_degree(oix, gix, ids, deleted)
    check_degree(oix, gix)  # without the flag the deleted slots still count
    with pytest.raises(da.DannError) as e:
        gix.degree_stats([n + 1])
    assert e.value.status == da._ffi.EBOUNDS


# ---- 4. prune_range ------------------------------------------------------------------------------------------------------------
N, DIM, R, PD = 400, 16, 12, 8


def built_pair(dtype, metric, seed=0, n=N, dim=DIM, r=R, pd=PD, row_stride=0, tags=False):
    """an index the oracle built with slack lists (max_degree r over pruned_degree pd), and its twin on the GPU"""
    rng = np.random.default_rng(500 + 10 * dtype + metric + seed)
    if dtype == da.SQ8:
        data = rng.normal(0.3, 0.5, (n, dim)).astype(np.float32)
        shift = (data.mean(0) - 2.0 * data.std(0)).astype(np.float32)
        scale = float(np.float32(4.0 * data.std()))
        rows = da.sq8_compress(data, shift, scale)
        kw = dict(sq_scale=scale, sq_shift_norm_sq=float(np.float32((shift ** 2).sum(dtype=np.float32))))
        odt = oracle.SQ8
    else:
        rows, kw, odt = data_for(rng, dtype, metric, n, dim), {}, ODT[dtype]
    oix = oracle.Index(odt, metric, dim, n, r, rows[:1], row_stride=row_stride or None, tags=tags, **kw)
    oix.set_rows(0, rows)
    cfg = oracle.build_config(pd, r, 24)
    for s in range(n):
        oix.insert(cfg, s)
    long_lists = int((oix.adj[:n, 0] > pd).sum())
    assert long_lists >= n // 4, f"{long_lists} of {n} lists are longer than {pd}: pick another seed"
    gix = da.Provider(dtype, metric, dim, n, r, rows[:1], row_stride=row_stride, inline_tags=tags, **kw)
    if row_stride:
        gix.upload_store(oix.rows)
    else:
        gix.set_elements(0, rows)
    gix.upload_graph(oix.adj)
    return oix, gix


@pytest.mark.parametrize("dtype,metric", ROW_CASES)
def test_prune_range_matches_model(dtype, metric):
    oix, gix = built_pair(dtype, metric)
    before = oix.adj.copy()
    long_lists = int((before[:N, 0] > PD).sum())
    cnt = gix.prune_range(da.build_config(PD, R, 24))
    pruned, _ = model.prune_range(oix, oracle.build_config(PD, R, 24), range(N))
    same_graph(gix, oix)
    assert pruned == long_lists and cnt[0] == N and cnt[1] == long_lists and cnt[2] == int(before[:N, 0].max()) and cnt[5] == 0
    assert cnt[3] >= int(before[:N, 0][before[:N, 0] > PD].sum()) - long_lists
    assert np.array_equal(gix.download_graph()[N], before[N])  # the start point lies outside the default range
    assert gix.degree_stats().max_degree <= PD
    raw = gix.download_graph()
    again = gix.prune_range(da.build_config(PD, R, 24))
    assert again[1] == 0 and np.array_equal(gix.download_graph(), raw)


def test_prune_range_equals_consolidate_without_deletions():
    oix, g1 = built_pair(da.F32, da.L2)
    _, g2 = built_pair(da.F32, da.L2)
    cfg = da.build_config(PD, R, 24)
    ids = np.arange(N + 1, dtype=np.uint32)
    g1.prune_range(cfg, ids)
    g2.consolidate(cfg, ids)
    assert np.array_equal(valid_rows(g1.download_graph(), R), valid_rows(g2.download_graph(), R))


def test_prune_range_subsets_repeats_and_ranges():
    oix, gix = built_pair(da.F32, da.L2, seed=1)
    cfg, ocfg = da.build_config(PD, R, 24), oracle.build_config(PD, R, 24)
    rng = np.random.default_rng(41)
    before = oix.adj.copy()
    part = rng.choice(N, 120, replace=False)
    ids = np.concatenate([part, part[:30], [N]])  # repeats are pruned once; the start point is an id like any other
    cnt = gix.prune_range(cfg, ids)
    model.prune_range(oix, ocfg, ids)
    same_graph(gix, oix)
    assert cnt[0] == 121 and cnt[1] == int((before[np.append(part, N), 0] > PD).sum())
    rest = np.setdiff1d(np.arange(N), part)
    assert np.array_equal(gix.download_graph()[rest], before[rest])  # the others are untouched
    gix.prune_range(cfg, first=100, n=50)
    model.prune_range(oix, ocfg, range(100, 150))
    same_graph(gix, oix)
    assert gix.prune_range(cfg, first=N + 1, n=0).tolist() == [0] * 6
    for kw in (dict(first=N, n=2), dict(ids=[N + 1])):
        with pytest.raises(da.DannError) as e:
            gix.prune_range(cfg, **kw)
        assert e.value.status == da._ffi.EBOUNDS
    with pytest.raises(da.DannError) as e:
        gix.prune_range(da.build_config(PD, R, 24, alpha=0.5))
    assert e.value.status == da._ffi.EINVAL
    with pytest.raises(da.DannError) as e:
        gix.prune_range(da.build_config(PD, R, 24, max_occlusion_size=5000))
    assert e.value.status == da._ffi.EUNSUPPORTED


def test_prune_range_known_answer():
    g = golden()
    case = g["prune_range"][0]
    oix, deg = fixture_index(g, case["graph"], case["pruned_degree"])
    gix = da.Provider(da.F32, da.L2, 2, 4, deg, np.array(g["start_point"], np.float32))
    gix.set_elements(0, np.array(g["vectors"], np.float32))
    gix.upload_graph(oix.adj)
    gix.prune_range(da.build_config(1, 1, 10), first=case["first"], n=case["n"])
    model.prune_range(oix, square_cfg(case), range(case["first"], case["first"] + case["n"]))
    same_graph(gix, oix)
    for v, m in case["max_len"].items():
        assert len(gix.get_neighbors(int(v))) <= m
    for v, m in case["len"].items():
        assert len(gix.get_neighbors(int(v))) == m


@pytest.mark.parametrize("dtype", [da.F32, da.F16])
def test_prune_range_mfma_path_equals_row_kernel(dtype):
    """rows of 1 KiB: f32 at dim 256, f16 at dim 512"""
    n, dim = 300, 256 if dtype == da.F32 else 512
    graphs = []
    for flags in (da.BUILD_MFMA_BACKEDGE, da.BUILD_ROW_KERNEL_ONLY):
        oix, gix = built_pair(dtype, da.L2, n=n, dim=dim)
        gix.set_build_options(flags)
        cnt = gix.prune_range(da.build_config(PD, R, 24), first=0, n=n)
        if flags == da.BUILD_MFMA_BACKEDGE:
            assert cnt[4] == cnt[1] > 0
            model.prune_range(oix, oracle.build_config(PD, R, 24), range(n))
            same_graph(gix, oix)
        else:
            assert cnt[4] == 0
        graphs.append(valid_rows(gix.download_graph(), R))
    assert np.array_equal(graphs[0], graphs[1])


@pytest.mark.parametrize("gpu_order,rule", [(da.TIE_RUST, oracle.DEFAULT_TIE_RULE), (da.TIE_POSITION, oracle.POSITION_TIE_RULE)])
def test_prune_range_tie_orders_on_a_lattice(gpu_order, rule):
    rng = np.random.default_rng(11)
    data = grid_data(3, 8)
    n, r = data.shape[0], 16
    adj = random_graph(rng, n, r, min_len=10)
    oix, gix = make_pair(oracle.F32, oracle.L2, data, adj, np.full((1, 3), 4.0, np.float32), r)
    gix.set_prune_tie_order(gpu_order)
    gix.prune_range(da.build_config(8, r, 50), np.arange(n + 1))
    oracle.set_tie_rule(rule, 0)
    try:
        model.prune_range(oix, oracle.build_config(8, r, 50), range(n + 1))
    finally:
        oracle.set_tie_rule()
    same_graph(gix, oix)


def test_prune_range_inline_tags():
    """slots below PUBLISHED: as neighbours they stay out of the pool, as ids they are left alone and counted"""
    stride = oracle.inmem2_stride(oracle.F32, DIM)
    oix, gix = built_pair(da.F32, da.L2, seed=2, row_stride=stride, tags=True)
    long_ids = np.flatnonzero(oix.adj[:N, 0] > PD)
    hidden = np.concatenate([long_ids[:5], np.setdiff1d(np.arange(N), long_ids)[:3], oix.neighbors(int(long_ids[7]))[:2]])
    for h in hidden:
        oix.set_tags(int(h), [2])
    gix.upload_store(oix.rows)
    before = oix.adj.copy()
    cnt = gix.prune_range(da.build_config(PD, R, 24))
    pruned, skipped = model.prune_range(oix, oracle.build_config(PD, R, 24), range(N))
    same_graph(gix, oix)
    assert skipped >= 5 and cnt[5] == skipped and cnt[1] == pruned
    assert np.array_equal(gix.download_graph()[long_ids[:5]], before[long_ids[:5]])
    g = gix.download_graph()
    for v in long_ids[5:]:
        if not np.isin(v, hidden):
            assert not np.isin(g[v, 1:1 + g[v, 0]], hidden).any(), v


def test_prune_range_finds_a_neighbour_past_the_last_slot():
    """dann_set_neighbors admits such an id: its row is never read, the list is left as it is, the call says DANN_EBOUNDS
    and the other lists are pruned as the model prunes them"""
    oix, gix = built_pair(da.F32, da.L2, seed=4)
    v = int(np.flatnonzero(oix.adj[:N, 0] > PD)[3])
    bad = oix.neighbors(v)
    bad[2] = N + 1 + 40
    gix.set_neighbors(v, bad)
    with pytest.raises(da.DannError) as e:
        gix.prune_range(da.build_config(PD, R, 24))
    assert e.value.status == da._ffi.EBOUNDS
    assert np.array_equal(gix.get_neighbors(v), bad)
    model.prune_range(oix, oracle.build_config(PD, R, 24), [i for i in range(N) if i != v])
    oix.set_neighbors(v, bad)
    same_graph(gix, oix)


def test_prune_range_refuses_pq_rows():
    rng = np.random.default_rng(61)
    dim, chunks, n = 16, 4, 64
    piv = rng.normal(size=(256, dim)).astype(np.float32)
    off = np.arange(chunks + 1, dtype=np.uint32) * (dim // chunks)
    gix = da.Provider(da.PQ, da.L2, dim, n, R, np.zeros((1, chunks), np.uint8), pq_pivots=piv, pq_offsets=off)
    with pytest.raises(da.DannError) as e:
        gix.prune_range(da.build_config(PD, R, 24))
    assert e.value.status == da._ffi.EUNSUPPORTED


def test_search_after_prune_range_matches_the_oracle():
    oix, gix = built_pair(da.F32, da.L2, seed=3, n=1500, dim=32)
    gix.prune_range(da.build_config(PD, R, 24), np.arange(1501))
    model.prune_range(oix, oracle.build_config(PD, R, 24), range(1501))
    same_graph(gix, oix)
    assert gix.degree_stats(np.arange(1501)).max_degree <= PD
    assert gix.count_reachable() == model.count_reachable(oix)[:2]
    q = rand_vectors(np.random.default_rng(5), oracle.F32, 100, 32)
    gi, gd, gst = gix.search(da.Knn(30, 1), q, 10)
    oi, od, oc, ost = oix.search_batch(q, 30, 1, 10)
    assert np.array_equal(gi, oi) and np.array_equal(bits(gd), bits(od))
    assert np.array_equal(gst["cmps"], ost[:, 0]) and np.array_equal(gst["hops"], ost[:, 1])
