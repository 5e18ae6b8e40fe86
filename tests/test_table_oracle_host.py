"""The oracle's distance-table index (oracle.TABLE) against the oracle itself.  A table index reads every distance from
a matrix the caller supplies (T[key of the first argument][stored slot]); it exists so that the algorithms the oracle
restates -- pinned by the reference's goldens -- can run on row types for which only a numpy model has distances
(tests/table_oracle.py).  These tests show that it is the same algorithm, not a second one:

  * native vs. table: the same build / prune / search / consolidate / in-place-delete sequence on a native F32 / U8 / SQ8
    index and on a table index filled from the native distances gives identical adjacency, ids, distance bits and counters;
  * the reference's grid_insert goldens replayed through a table index give the counters and searches the native replay
    gives (tests/test_oracle_build.py);
  * on a deliberately asymmetric table the prunes of T and of its transpose differ, and a Python restatement of
    occlude_list that reads T[candidate][selected] agrees with the oracle: the first argument is the table row;
  * the entry points that read row bytes answer NaN / an error for a table index."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle
from consolidate_model import consolidate, row_distance
from gridutil import grid_data, grid_start_point
from helpers import bits as fbits
from inplace_delete_model import TIE_RUST, TWO_HOP_AND_ONE_HOP, inplace_delete
from search_builders import orc_sq8_compress, sq_setup

NQ = 6
BATCHES = (1, 2, 5, 20, 72)


def _native_index(kind, metric, n, maxdeg):
    """-> (native index without edges, row images (n), start image, query images (NQ))"""
    rng = np.random.default_rng(1000 + 17 * kind + metric + n)
    if kind == oracle.F32:
        dim = 24
        rows = rng.normal(0.1, 1.0, (n + 1 + NQ, dim)).astype(np.float32)
        if metric == oracle.COSINE_NORMALIZED:
            rows /= np.sqrt((rows.astype(np.float64) ** 2).sum(1))[:, None].astype(np.float32)
        kw = {}
    elif kind == oracle.U8:  # tie-heavy: few values, few dimensions
        dim = 6
        rows = rng.integers(0, 3, (n + 1 + NQ, dim), dtype=np.uint8)
        kw = {}
    else:
        dim = 32
        data, shift, scale, snorm = sq_setup(rng, n + 1 + NQ, dim)
        rows = orc_sq8_compress(data, shift, scale)
        kw = dict(sq_scale=scale, sq_shift_norm_sq=snorm)
    ix = oracle.Index(kind, metric, dim, n, maxdeg, rows[n:n + 1], **kw)
    ix.set_rows(0, rows[:n])
    return ix, rows


def _fill_table(ix, rows):
    """T[x][y] = the native pair distance of row image x (slots, then the start point, then the queries) and slot y, one
    oracle.distance / orc_sq8_distance call per ordered pair"""
    nslots = ix.capacity + ix.nstart
    imgs = [np.ascontiguousarray(r).view(np.uint8).reshape(-1) for r in rows]
    T = np.empty((len(imgs), nslots), np.float32)
    if ix.dtype == oracle.SQ8:
        for x in range(len(imgs)):
            for y in range(nslots):
                T[x, y] = row_distance(ix, imgs[x], imgs[y])
        return T
    fn, dim = oracle.lib().orc_distance, ix.dim
    ptr = [C.c_void_p(i.ctypes.data) for i in imgs]
    for x in range(len(imgs)):
        px = ptr[x]
        T[x] = [fn(ix.dtype, ix.metric, px, ptr[y], dim) for y in range(nslots)]
    return T


_CASES = {}


def _case(kind, metric, n):
    key = (kind, metric, n)
    if key not in _CASES:
        ix, rows = _native_index(kind, metric, n, 12)
        _CASES[key] = (rows, _fill_table(ix, rows), ix._c.sq_scale, ix._c.sq_shift_norm_sq)
    return _CASES[key]


def _sequence(ix, n, queries, stored_query, T, ibc):
    """the whole sequence on one index -> everything observable, as a list of (name, value)"""
    out = []
    nslots = n + 1
    rng = np.random.default_rng(77)
    cfg = oracle.build_config(8, 12, 24, intra_batch_candidates=ibc)
    cnt = np.zeros(5, np.uint64)
    s = 0
    for b in BATCHES + (n,):
        slots = np.arange(s, min(s + b, n - 8), dtype=np.uint32)
        if slots.size:
            ix.multi_insert(cfg, slots, cnt)
        s += b
    out.append(("multi_insert adj", ix.adj.copy()))
    out.append(("multi_insert counters", cnt.copy()))
    for slot in range(n - 8, n):
        ix.insert(oracle.build_config(8, 12, 24, max_backedges=(0 if slot & 1 else 3)), slot, cnt)
    out.append(("insert adj", ix.adj.copy()))
    out.append(("insert counters", cnt.copy()))
    for i, loc in enumerate(rng.choice(n, 12, replace=False)):
        m = [0, 1, 5, 70, 200, 333][i % 6]
        ids = rng.choice(n, m, replace=False).astype(np.uint32)
        if m > 3:
            ids[2] = loc
        for sat in (False, True):
            nb, evals = ix.prune_pool(cfg, int(loc), ids, T[loc, ids], force_saturate=sat)
            out.append((f"prune_pool {i} {sat}", np.append(nb, evals)))
    qs = np.stack([np.ascontiguousarray(q).reshape(-1) for q in queries])
    for L, W in ((10, 1), (32, 2)):
        ids, d, counts, st = ix.search_batch(qs, L, W, 10)
        out += [(f"search_batch {L} ids", ids), (f"search_batch {L} dists", fbits(d)), (f"search_batch {L} counts", counts),
                (f"search_batch {L} stats", st)]
    for slot in rng.choice(n, 6, replace=False):
        k, ids, d, st, rid, rd = ix.search(stored_query(int(slot)), 20, 1, 10, record=True)
        out += [(f"record {slot}", np.concatenate([[k], ids, fbits(d), st, rid, fbits(rd)]))]
    match = rng.random(nslots) < 0.4
    for j, q in enumerate(queries):
        d0 = np.sort(T[nslots + j, :n])
        r_small, r_big = float(d0[n // 20]), float(d0[2 * n // 5])
        for args in ((20, r_small, 1, None, 1.0, 1.0, 0), (8, r_big, 2, r_small, 0.25, 1.0, 0), (8, r_big, 1, None, 0.5, 1.3, 40)):
            ids, d, st = ix.range_search(q, *args, out_cap=nslots)
            out.append((f"range {j} {args[0]}", np.concatenate([ids, fbits(d), st])))
        ids, d, st = ix.filtered_range_search(q, 12, r_big, match, out_cap=nslots)
        out.append((f"filtered range {j}", np.concatenate([ids, fbits(d), st])))
        k, ids, d, st = ix.inline_filter_search(q, 20, 10, match)
        out.append((f"inline {j}", np.concatenate([[k], ids[:k], fbits(d[:k]), st])))
        k, ids, d, st = ix.multihop_search(q, 24, 10, match, beam_width=2)
        out.append((f"multihop {j}", np.concatenate([[k], ids[:k], fbits(d[:k]), st])))
        pages = ix.paged_search(q, 24, 7, max_pages=6)
        out.append((f"paged {j}", np.concatenate([np.concatenate([i, fbits(d)]) for i, d in pages])))
    built = ix.adj.copy()
    deleted = np.zeros(nslots, bool)
    deleted[rng.choice(n, n // 10, replace=False)] = True
    kinds = consolidate(ix, oracle.build_config(6, 12, 24), deleted)
    out += [("consolidate kinds", kinds), ("consolidate adj", ix.adj.copy())]
    ix.adj[:] = built
    deleted = np.zeros(nslots, bool)
    want = inplace_delete(ix, oracle.build_config(6, 12, 24), deleted, rng.choice(n, 16, replace=False), TWO_HOP_AND_ONE_HOP, 3,
                          TIE_RUST, 0, 0)
    out += [("inplace counters", np.asarray(want)), ("inplace adj", ix.adj.copy()), ("inplace deleted", deleted.copy())]
    return out


NATIVE = [(oracle.F32, oracle.L2, 600), (oracle.F32, oracle.INNER_PRODUCT, 400), (oracle.F32, oracle.COSINE, 500),
          (oracle.F32, oracle.COSINE_NORMALIZED, 450), (oracle.U8, oracle.L2, 800), (oracle.SQ8, oracle.L2, 400),
          (oracle.SQ8, oracle.INNER_PRODUCT, 420)]


@pytest.mark.parametrize("ibc", [oracle.IBC_NONE, 4, oracle.IBC_ALL])
@pytest.mark.parametrize("kind,metric,n", NATIVE)
def test_table_index_is_the_native_algorithm(kind, metric, n, ibc):
    rows, T, scale, snorm = _case(kind, metric, n)
    nat, _ = _native_index(kind, metric, n, 12)
    tab = oracle.Index(oracle.TABLE, metric, 1, n, 12, np.zeros(1), table=T)
    nslots = n + 1
    a = _sequence(nat, n, [rows[nslots + j] for j in range(NQ)], lambda s: nat.row(s), T, ibc)
    b = _sequence(tab, n, [np.array([nslots + j], np.uint32) for j in range(NQ)], lambda s: np.array([s], np.uint32), T, ibc)
    assert [k for k, _ in a] == [k for k, _ in b]
    for (name, x), (_, y) in zip(a, b):
        assert np.array_equal(x, y), name
    assert int(a[3][1][1]) > 0 and int(a[3][1][3]) > 0  # pair distances were evaluated, lists were appended to


def _golden_table(payload):
    dims, size = payload["grid_dims"], payload["grid_size"]
    rows = np.concatenate([grid_data(dims, size), grid_start_point(dims, size)[None, :]] +
                          [np.array(sc["query"], np.float32)[None, :] for sc in payload["searches"]])
    n = size ** dims
    T = np.empty((rows.shape[0], n + 1), np.float32)
    for x in range(rows.shape[0]):
        T[x] = [oracle.distance(oracle.F32, oracle.L2, rows[x], rows[y]) for y in range(n + 1)]
    return T, n


def test_grid_insert_goldens_through_a_table_index(golden_dir):
    """every grid_insert golden (three 1-D, six 3-D and six 4-D lattices) replayed with the distances read from a table of
    the lattice's L2 distances: the build counters and both post-build searches of the golden, exactly -- what
    test_grid_insert_all_goldens_exact_with_rust_sort asserts of the native index"""
    import re
    seen = {}
    tables = {}
    for f in json.load(open(os.path.join(golden_dir, "grid_insert.json"))):
        p = f["payload"]
        dims, size = p["grid_dims"], p["grid_size"]
        key = (dims, size, json.dumps([sc["query"] for sc in p["searches"]]))
        if key not in tables:
            tables[key] = _golden_table(p)
        T, n = tables[key]
        m = re.search(r"insert_\d+_\d+_(single|batch_(\d+))/ibc_(\w+)\.json", f["source"])
        batch = None if m.group(1) == "single" else int(m.group(2))
        ibc = {"none": oracle.IBC_NONE, "all": oracle.IBC_ALL, "max_4": 4}[m.group(3)]
        deg = 2 * dims
        cfg = oracle.build_config(min(max(deg - 2, 2), deg), deg, 100, intra_batch_candidates=ibc)  # grid_insert.rs:83-86
        ix = oracle.Index(oracle.TABLE, oracle.L2, 1, n, deg, np.zeros(1), table=T)
        nat = oracle.Index(oracle.F32, oracle.L2, dims, n, deg, grid_start_point(dims, size))
        nat.set_rows(0, grid_data(dims, size))
        cnt, ncnt = np.zeros(5, np.uint64), np.zeros(5, np.uint64)
        for index, counters in ((ix, cnt), (nat, ncnt)):
            if batch is None:
                for i in range(n):
                    index.insert(cfg, i, counters)
            else:
                for s in range(0, n, batch):
                    index.multi_insert(cfg, np.arange(s, min(s + batch, n)), counters)
        im = p["insert_metrics"]
        assert [int(cnt[2]), int(cnt[3]), int(cnt[4])] == [im["set_neighbors"], im["append_neighbors"], im["get_neighbors"]], f["test"]
        assert np.array_equal(ix.adj, nat.adj) and np.array_equal(cnt, ncnt), f["test"]
        for j, sc in enumerate(p["searches"]):
            k, ids, dists, st = ix.search(np.array([n + 1 + j], np.uint32), 10, sc["beam_width"], 10)
            assert k == sc["num_results"]
            assert [int(i) for i in ids[:k]] == [w[0] for w in sc["results"]], f["test"]
            assert [float(d) for d in dists[:k]] == [w[1] for w in sc["results"]], f["test"]
            assert int(st[0]) == sc["comparisons"] and int(st[1]) == sc["hops"], f["test"]
        seen[dims] = seen.get(dims, 0) + 1
    assert seen == {1: 3, 3: 6, 4: 6}


# ---- which index is the row ------------------------------------------------------------------------------------------------
F32MAX = np.float32(np.finfo(np.float32).max)


def py_occlude_list(T, loc, ids, dists, degree, alpha, occluding, saturate):
    """occlude_list (index.rs:2565-2650) over a pool sorted by distance, every f32 operation in numpy; the pair distance of
    candidate i against the already selected rp is T[ids[i]][ids[rp]]: candidate first, selected second"""
    m = len(ids)
    alpha = np.float32(alpha)
    occ = [np.float32(0.0)] * m
    last, nb = [0] * m, [0] * m
    found, cur = 0, np.float32(1.0)
    inc = alpha if alpha < np.float32(1.2) else np.float32(1.2)
    while found < degree and m:
        for i in range(m):
            if found >= degree:
                break
            o, l = occ[i], last[i]
            if o > cur:
                continue
            if ids[i] == loc:
                occ[i] = F32MAX
                continue
            while l != found:
                rp = nb[l]
                l += 1
                if rp >= i:
                    last[i] = l
                    continue
                d_jk = T[ids[i], ids[rp]] if ids[rp] != loc else F32MAX
                d_ik = dists[i]
                if occluding:
                    if d_jk < cur * d_ik:
                        o = cur + np.float32(0.01)
                elif d_jk == 0:
                    o = F32MAX
                else:
                    with np.errstate(all="ignore"):
                        r = np.float32(d_ik) / np.float32(d_jk)
                    o = o if np.isnan(r) else (r if np.isnan(o) or not o > r else o)
                if o > cur:
                    break
            last[i] = l
            if o > cur:
                occ[i] = o
                continue
            occ[i] = F32MAX
            nb[found] = i
            found += 1
        if cur == alpha:
            break
        nxt = np.float32(cur * inc)
        cur = nxt if nxt < alpha else alpha
    out = [int(ids[nb[k]]) for k in range(found)]
    if saturate:
        for i in ids:
            if len(out) >= degree:
                break
            if i != loc and int(i) not in out:
                out.append(int(i))
    return out


@pytest.mark.parametrize("metric", [oracle.L2, oracle.INNER_PRODUCT])
def test_the_first_argument_is_the_table_row(metric):
    n = 400
    rng = np.random.default_rng(5 + metric)
    pts = rng.normal(0, 1, (n + 1, 8))
    sym = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    T = (sym * rng.uniform(0.7, 1.3, sym.shape)).astype(np.float32)  # every entry scaled on its own: T != T^t nearly everywhere
    if metric == oracle.INNER_PRODUCT:
        T = (T - np.float32(8.0)).astype(np.float32)
    assert (T != T.T).mean() > 0.9
    a = oracle.Index(oracle.TABLE, metric, 1, n, 16, np.zeros(1), table=T)
    b = oracle.Index(oracle.TABLE, metric, 1, n, 16, np.zeros(1), table=np.ascontiguousarray(T.T))
    cfg = oracle.build_config(8, 16, 24)
    differ = 0
    for i in range(60):
        loc = int(rng.integers(0, n))
        ids = rng.choice(n, 60, replace=False).astype(np.uint32)
        d = T[loc, ids]  # the same pool distances for both: only the table the sweep reads is transposed
        assert np.unique(d).size == d.size  # no ties: the pool order is the plain sort
        order = np.argsort(d, kind="stable")
        for sat in (False, True):
            want_a, _ = a.prune_pool(cfg, loc, ids, d, force_saturate=sat)
            want_b, _ = b.prune_pool(cfg, loc, ids, d, force_saturate=sat)
            occluding = metric == oracle.INNER_PRODUCT
            assert py_occlude_list(T, loc, ids[order], d[order], 8, 1.2, occluding, sat) == want_a.tolist(), (i, sat)
            assert py_occlude_list(T.T, loc, ids[order], d[order], 8, 1.2, occluding, sat) == want_b.tolist(), (i, sat)
            differ += int(want_a.tolist() != want_b.tolist())
    assert differ >= 30, differ


def test_byte_reading_entry_points_refuse_a_table():
    n = 40
    T = np.random.default_rng(3).random((n + 3, n + 1)).astype(np.float32)
    ix = oracle.Index(oracle.TABLE, oracle.L2, 1, n, 8, np.zeros(1), table=T)
    key = np.array([n + 2], np.uint32)
    ids, d = ix.expand_beam(key, np.arange(n + 1, dtype=np.uint32))
    assert np.array_equal(fbits(d), fbits(T[n + 2]))                       # query x slot = T[key(query)][slot]
    ix.set_neighbors(n, [0, 1, 2])
    assert ix.search(key, 8, 1, 4)[0] == 3
    with pytest.raises(RuntimeError):
        ix.search_batch(key[None, :], 8, 1, 4, fast=True)                  # the AVX twins read row bytes
    with pytest.raises(RuntimeError):
        ix.search(np.array([n + 3], np.uint32), 8, 1, 4)                   # a key past the table
    for fn in (oracle.distance, oracle.query_distance, oracle.distance_scalar_ref):
        assert np.isnan(fn(oracle.TABLE, oracle.L2, key, key))
    assert np.isnan(oracle.query_distance(oracle.TABLE, oracle.L2, key, key, fast=True))
    with pytest.raises(ValueError):
        oracle.bench_distance(oracle.TABLE, oracle.L2, 1, 16, 1)
    with pytest.raises(ValueError):
        oracle.Index(oracle.TABLE, oracle.L2, 1, n, 8, np.zeros(1), table=T[:n])   # fewer keys than slots
    with pytest.raises(ValueError):
        oracle.Index(oracle.F32, oracle.L2, 4, n, 8, np.zeros((1, 4)), table=T)    # a table belongs to a TABLE index
    assert oracle.TABLE == oracle.PQ + 1
