"""The case table of tests/test_gpu_tail_matrix.py and tests/test_tail_matrix_host.py: what runs after a Knn search stops
-- graph::search::Range's second phase and FilteredRange's sort / de-duplication / frontier walk
(diskann_amd/csrc/search_kernel_impl.h) and paged search (diskann_amd/csrc/paged_kernels.hip) -- swept past the first queue
slot, over row type, metric, beam, loop form, visited-entry width, degree and page size, with their limits.  A covering
design like tests/search_matrix.py, whose builders, shapes (4 000 rows, degree 24, 16 queries) and queue-slot rule
(qcap = L + start points; QS = 1, 2, 4, 8, 16 for qcap <= 64 / 128 / 256 / 512 / 1024) it shares.  No test functions.

Every reference answer is the oracle's (oracle.Index.range_search / filtered_range_search / the orc_paged_* session).
The radii of an index are quantiles of the oracle's distances of query 0 to all rows: r_mix (5 % unless QUANTILES says
otherwise) lets some queries into the second round, r_sat (15 %) nearly all, with result lists of 1 000 entries and more.
The graphs are the sweep's own (lists of 20 .. 24 neighbours; full lists at degrees 65 and 100) over the builders' rows."""
import ctypes as C
from collections import namedtuple

import numpy as np

import oracle
import search_matrix as sm
import spherical_model as sph
from helpers import rand_vectors, random_graph
from minmax_builders import MmTwin

L2 = sm.L2
MM_BITS = {"MM1": 1, "MM2": 2, "MM4": 4, "MM8": 8}
ROW_TYPES = sm.ROW_TYPES + tuple(MM_BITS)
N, R, NQ, NQ_PERSISTENT, MAX_CONCURRENCY = sm.N, sm.R, sm.NQ, sm.NQ_PERSISTENT, sm.MAX_CONCURRENCY
FULL_TYPES = ("F32", "U8")
QCAPS_FULL = (64, 65, 128, 129, 257, 513, 1024)   # the range queue axis on FULL_TYPES
QCAPS_REST = (65, 129, 257)                       # ... on every other row type
QCAPS_METRIC = (65, 257)
QCAPS_VISITED = (129, 513)
QCAPS_FILTERED = (64, 65, 129, 257, 513)
QCAPS_PAGED = (64, 65, 129, 257)
QCAPS_PAGED_WIDE = (65, 257)                      # degrees 65 and 100: two expand rounds and two merges a hop
QCAP_PERSISTENT = QCAP_RERUN = 257
PSETS = ("mix", "inner", "maxret", "slack0")
MAX_RETURNED = 300
METRIC_PSETS = ("sat-s1.0", "sat-s1.2")
FILTERS = ("q0.3", "q0.05", "shared")
PAGE_MODES = ("p1", "p7", "pL", "var")
PAGE_MODES_WIDE = ("p7", "pL", "var")
SMALL_N, TIE_DIM, TIE_VALUES, HOLE_FRACTION = 600, 4, 4, 0.1
# quantiles (r_mix, r_sat) of the distances of query 0.  Uniform rows of 100+ dimensions have concentrated distances, so
# how many of the 16 queries a radius lets into the second round depends on where query 0 happens to sit, and the 1-bit
# rows' distances take some 40 values: an index that misses a condition of tests/test_tail_matrix_host.py at the default
# pair gets its own, by (row type, row length) -- the quantile moves, never the condition
DEFAULT_QUANTILES = (0.05, 0.15)
QUANTILES = {("F16", 100): (0.03, 0.15), ("U8", 128): (0.12, 0.3), ("I8", 128): (0.02, 0.15), ("I8", 100): (0.2, 0.4),
             ("SQ4", 128): (0.2, 0.4), ("SQ1", 128): (0.045, 0.15), ("SQ1", 256): (0.04, 0.15), ("SPH1", 128): (0.04, 0.15),
             ("SPH1", 100): (0.03, 0.15), ("SPH2", 100): (0.08, 0.2), ("SPH4", 128): (0.12, 0.3), ("PQ", 100): (0.2, 0.4),
             ("MM1", 128): (0.03, 0.15), ("MM1", 100): (0.03, 0.15), ("MM8", 128): (0.12, 0.2)}

# kind: std (search_matrix.Built / MmTwin) | holes (inline tags, HOLE_FRACTION of the slots unpublished) | ties (rows of
# TIE_DIM elements in 0 .. TIE_VALUES - 1, SMALL_N rows) | drain (SMALL_N rows, paged until nothing is left)
Ix = namedtuple("Ix", "rt metric dim R nstart kind")
# sec: range | range-rerun | range-limits | frange | frange-limits | paged | paged-limits | paged-interleave | paged-refused
# pset: a parameter set of the section (PSETS / METRIC_PSETS / PAGE_MODES); opt: sorted (name, value) pairs -- vfmt,
# loop = persistent, filter
Case = namedtuple("Case", "ix sec qcap W pset opt")


def case_id(c):
    x = c.ix
    s = f"{x.rt}-{sm.METRIC_NAME[x.metric]}-d{x.dim}-R{x.R}-s{x.nstart}-{x.kind}-{c.sec}-q{c.qcap}-W{c.W}-{c.pset}"
    return s + "".join(f"-{k}{v}" for k, v in c.opt)


def ix_id(x):
    return f"{x.rt}-{sm.METRIC_NAME[x.metric]}-d{x.dim}-R{x.R}-s{x.nstart}-{x.kind}"


def opt(c, name, default=None):
    return dict(c.opt).get(name, default)


def _case(ix, sec, qcap, W=1, pset="", **o):
    return Case(ix, sec, qcap, W, pset, tuple(sorted(o.items())))


def queue_ixs(rt, deg=R):
    """the two indexes of a row type: 128-element rows on one start point, run-time length on three (PQ rows: one DIM form)"""
    rd = sm.runtime_dim(rt)
    return Ix(rt, L2, rd if rt == "PQ" else 128, deg, 1, "std"), Ix(rt, L2, rd, deg, 3, "std")


def metric_ixs(rt):
    """inner product / cosine indexes of a row type that have an oracle twin (not the spherical rows: their reference for
    these metrics is the Python model; not the MinMax rows: their twin is L2)"""
    if rt not in sm.ROW_TYPES or rt in sm.SPH_BITS:
        return []
    return [Ix(rt, m, dim, R, 1, "std") for m in sm.other_metrics(rt) for dim in sm.metric_dims(rt, m)]


def build_table():
    t = []
    for rt in ROW_TYPES:
        g128, grt = queue_ixs(rt)
        # 1. range search: the queue axis in plain (beam 1) and general (beam 3) mode
        for g in (g128, grt):
            for q in (QCAPS_FULL if rt in FULL_TYPES else QCAPS_REST):
                t += [_case(g, "range", q, W, p) for W in (1, 3) for p in PSETS]
        for g in metric_ixs(rt):
            t += [_case(g, "range", q, 1, p) for q in QCAPS_METRIC for p in METRIC_PSETS]
        if rt in ("F32", "U8", "SQ4"):
            t += [_case(g128, "range", QCAP_PERSISTENT, 1, p, loop="persistent") for p in ("inner", "slack0")]
        if rt in sm.VISITED_TYPES:
            t += [_case(g128, "range", q, 1, "slack0", vfmt=v) for v in (16, 32) for q in QCAPS_VISITED]
        if rt in FULL_TYPES:
            t.append(_case(g128, "range-rerun", QCAP_RERUN, 1, "slack0"))
            t.append(_case(g128, "range-limits", 129, 1, "slack0"))
        # 2. filtered range search
        if rt in sm.FILTERED_TYPES:
            t += [_case(g128, "frange", q, W, p, filter=f) for q in QCAPS_FILTERED for W in (1, 2) for f in FILTERS for p in PSETS]
            t.append(_case(g128, "frange-limits", 129, 1, "slack0", filter="q0.3"))
        # 3. paged search
        if rt == "PQ":
            t.append(_case(g128, "paged-refused", 65))
            continue
        for g in (g128, grt):
            t += [_case(g, "paged", q, 1, m) for q in QCAPS_PAGED for m in PAGE_MODES]
        if rt in FULL_TYPES:
            t.append(_case(g128, "paged-limits", 65))
            t.append(_case(g128, "paged-interleave", 65))
        wide = (Ix(rt, L2, g128.dim, 65, 1, "std"), Ix(rt, L2, grt.dim, 100, 3, "std"))
        for g in wide:
            t += [_case(g, "paged", q, 1, m) for q in QCAPS_PAGED_WIDE for m in PAGE_MODES_WIDE]
    # paged until nothing is left; equal distances; unpublished slots
    t += [_case(Ix("F32", L2, 16, R, 1, "drain"), "paged", 65, 1, m, drain=1) for m in ("p7", "pL", "var")]
    for rt in ("U8", "I8"):
        t += [_case(Ix(rt, L2, TIE_DIM, 65, 1, "ties"), "paged", 65, 1, m, drain=1) for m in ("p7", "var")]
    for rt in ("F32", "SPH2"):
        g = Ix(rt, L2, 128, R, 1, "holes")
        t += [_case(g, "paged", q, 1, m) for q in (65, 257) for m in ("p7", "var")]
        t += [_case(g, "range", 129, W, "slack0") for W in (1, 3)]
    return t


TABLE = build_table()


def by_index():
    """the table's indexes and per index its cases, in table order (a test session keeps one index at a time)"""
    out = {}
    for c in TABLE:
        out.setdefault(c.ix, []).append(c)
    return out


def qs_of(qcap):
    return 1 if qcap <= 64 else 2 if qcap <= 128 else 4 if qcap <= 256 else 8 if qcap <= 512 else 16


def page_sizes(mode, L):
    """the page sizes of successive next_page calls, cycled"""
    return {"p1": (1,), "p7": (7,), "pL": (L,), "var": (7, 1, L, 3)}[mode]


def page_calls(mode):
    """next_page calls of a session that is not run until it is drained"""
    return {"p1": 40, "p7": 12, "pL": 4, "var": 12}[mode]


# ---- builders -------------------------------------------------------------------------------------------------------------
def _min_len(deg):
    """the shortest adjacency list of an index of this degree: degree - 4, or the degree itself on the wide indexes"""
    return deg - 4 if deg == R else deg


class Built:
    """one index of the table: .oix (the oracle or the oracle's twin), .gix (None without a GPU), .q_gpu / .q_ref (the same
    queries for the library and for the oracle), .match (per-query bitmaps of the two selectivities, one shared bitmap)"""

    def __init__(self, ix, gpu):
        self.ix, self.refs, self.gix = ix, {}, None
        rt, metric, dim, deg, nstart, kind = ix
        seed = sm._seed(sm.Group(rt, metric, dim, deg, nstart, False)) + (0 if kind == "std" else 11)
        self.n = N if kind in ("std", "holes") else SMALL_N
        nqmax = max(NQ, NQ_PERSISTENT)
        if kind == "std" and rt in MM_BITS:
            c = MmTwin(MM_BITS[rt], dim, N, deg, seed, nstart=nstart, gpu=False)
            self.oix = c.oix
            self.q_gpu, self.q_ref = c.queries(nqmax)
            self._make = c.attach_gpu
        elif kind == "std":
            b = sm.Built(sm.Group(rt, metric, dim, deg, nstart, False), gpu=False)
            self.oix, self.q_gpu, self.q_ref = b.oix, b.q_gpu, b.q_ref
            self._make = lambda: b._make(_da())
        elif kind == "holes":
            self._build_holes(seed, nqmax)
        else:
            self._build_small(seed, nqmax)
        if kind == "std":
            # the sweep's own graph over the builder's rows: lists of 20 .. 24 neighbours, so that three nodes of a beam
            # can yield more than 64 candidates (helpers.random_graph's default starts at half the degree: 54 on average,
            # hardly ever 65); the wide indexes' lists are full, so that one node does
            adj = random_graph(np.random.default_rng(seed + 3), N, deg, nstart=nstart, min_len=_min_len(deg))
            self.oix.adj[:] = adj
            make = self._make

            def with_graph():
                gix = make()
                gix.upload_graph(adj)
                return gix
            self._make = with_graph
        self.nslots = self.n + nstart
        frng = np.random.default_rng(seed + 7)
        self.match = {"q0.3": frng.random((nqmax, self.nslots)) < 0.3, "q0.05": frng.random((nqmax, self.nslots)) < 0.05,
                      "shared": frng.random(self.nslots) < 0.3}
        d0 = self.distances(0)[:self.n]
        qm, qsat = QUANTILES.get((rt, dim), DEFAULT_QUANTILES) if kind == "std" and metric == L2 else DEFAULT_QUANTILES
        self.r_mix, self.r_sat = float(np.quantile(d0, qm)), float(np.quantile(d0, qsat))
        if gpu:
            self.gix = self._make()

    def _build_small(self, seed, nqmax):
        rt, metric, dim, deg, nstart, kind = self.ix
        rng = np.random.default_rng(seed)
        dt = sm.ORACLE_DT[rt]
        if kind == "ties":  # most distances tie: a handful of distinct rows
            lo = -2 if rt == "I8" else 0
            draw = lambda n: rng.integers(lo, lo + TIE_VALUES, (n, dim)).astype(oracle.NP_DTYPE[dt])
        else:
            draw = lambda n: rand_vectors(rng, dt, n, dim)
        data = draw(SMALL_N)
        adj = random_graph(rng, SMALL_N, deg, nstart=nstart, min_len=_min_len(deg))
        self.oix = oracle.Index(dt, metric, dim, SMALL_N, deg, data[:nstart])
        self.oix.set_rows(0, data)
        self.oix.adj[:] = adj
        self.q_gpu = self.q_ref = draw(nqmax)

        def make():
            da = _da()
            gix = da.Provider(dt, metric, dim, SMALL_N, deg, data[:nstart])
            gix.set_elements(0, data)
            gix.upload_graph(adj)
            return gix
        self._make = make

    def _build_holes(self, seed, nqmax):
        """the Store layout with HOLE_FRACTION of the slots below PUBLISHED, on both sides: f32 rows as they are; 2-bit
        spherical rows over the oracle's U8 twin of their codes (search_builders.SphTwin), each with its own stride"""
        rt, metric, dim, deg, nstart, _ = self.ix
        rng = np.random.default_rng(seed)
        odt = oracle.F32 if rt == "F32" else oracle.U8
        bits = sm.SPH_BITS.get(rt)
        draw = (lambda n: rand_vectors(rng, odt, n, dim)) if rt == "F32" else \
            (lambda n: rng.integers(0, 1 << bits, (n, dim), dtype=np.uint8))
        data, start = draw(N), draw(nstart)
        adj = random_graph(rng, N, deg, nstart=nstart, min_len=_min_len(deg))
        self.oix = oracle.Index(odt, metric, dim, N, deg, start, row_stride=oracle.inmem2_stride(odt, dim), tags=True)
        self.oix.set_rows(0, data)
        self.oix.adj[:] = adj
        holes = np.sort(rng.choice(N, int(N * HOLE_FRACTION), replace=False))
        tags = rng.choice(np.array([0, 1, 2, 253], np.uint8), holes.size)
        for h, tg in zip(holes, tags):
            self.oix.set_tags(int(h), [tg])
        self.holes = holes
        q = draw(nqmax)
        self.q_ref = q
        self.q_gpu = q if rt == "F32" else sph.flat_rows(q, bits)

        def make():
            da = _da()
            dt = da.F32 if rt == "F32" else sm.DT_CODE[rt]
            rows = (lambda x: x) if rt == "F32" else (lambda x: sph.flat_rows(x, bits))
            gix = da.Provider(dt, metric, dim, N, deg, rows(start), row_stride=da.lib().dann_inmem2_row_stride(dt, dim),
                              inline_tags=True)
            gix.set_elements(0, rows(data))
            for h, tg in zip(holes, tags):
                gix.set_tags(int(h), np.array([tg], np.uint8))
            gix.upload_graph(adj)
            return gix
        self._make = make

    def close(self):
        if self.gix is not None:
            self.gix.close()
            self.gix = None

    def distances(self, j):
        """the oracle's exact distances of query j to every readable slot (NaN where a slot is unpublished)"""
        q = np.ascontiguousarray(self.q_ref[j], dtype=self.oix.query_dtype)  # (PQ rows: an f32 query)
        slots = np.arange(self.nslots, dtype=np.uint32)
        ids, d = np.empty(self.nslots, np.uint32), np.empty(self.nslots, np.float32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        n = oracle.lib().orc_expand_beam(C.byref(self.oix._c), vp(q), vp(slots), self.nslots, vp(ids), vp(d))
        assert n >= 0
        out = np.full(self.nslots, np.nan, np.float32)
        out[ids[:n]] = d[:n]
        return out

    # ---- parameters ----
    def range_kw(self, c):
        """the keyword arguments of a range / filtered range case, the same for Provider and oracle.Index"""
        kw = dict(starting_l=c.qcap - c.ix.nstart, beam_width=c.W)
        if c.pset == "mix":
            kw.update(radius=self.r_mix)
        elif c.pset == "inner":
            kw.update(radius=self.r_sat, initial_slack=0.25, range_slack=1.1, inner_radius=self.r_mix)
        elif c.pset == "maxret":
            kw.update(radius=self.r_sat, max_returned=MAX_RETURNED)
        elif c.pset == "slack0":
            kw.update(radius=self.r_sat, initial_slack=0.0)
        else:
            kw.update(radius=self.r_sat, initial_slack=0.25, range_slack=float(c.pset[5:]))
        return kw

    def nq(self, c):
        return NQ_PERSISTENT if opt(c, "loop") == "persistent" else NQ

    # ---- the oracle's answers, computed once per distinct call ----
    def range_reference(self, c, **override):
        """per query (ids, dists, [cmps, hops, result_count, second_round]); an unbounded output list"""
        kw = dict(self.range_kw(c), **override)
        f = opt(c, "filter") if c.sec.startswith("frange") else None
        key = ("range", f, self.nq(c), tuple(sorted(kw.items())))
        if key not in self.refs:
            out = []
            for j in range(self.nq(c)):
                if f:
                    m = self.match[f] if f == "shared" else self.match[f][j]
                    out.append(self.oix.filtered_range_search(self.q_ref[j], kw["starting_l"], kw["radius"], m,
                                                              **{k: v for k, v in kw.items() if k not in ("starting_l", "radius")}))
                else:
                    out.append(self.oix.range_search(self.q_ref[j], **kw))
            self.refs[key] = out
        return self.refs[key]

    def paged_reference(self, L, sizes, calls=None, nq=NQ):
        """per query the pages [(ids, dists)] of `calls` next_page calls with page sizes cycled from `sizes`; calls = None:
        until two calls in a row return nothing"""
        key = ("paged", L, sizes, calls, nq)
        if key not in self.refs:
            self.refs[key] = [oracle_pages(self.oix, self.q_ref[j], L, sizes, calls) for j in range(nq)]
        return self.refs[key]


def _da():
    import diskann_amd
    return diskann_amd


def oracle_pages(oix, query, L, sizes, calls=None):
    lib = oracle.lib()
    q = np.ascontiguousarray(query, dtype=oracle.NP_DTYPE[oix.dtype])
    h = lib.orc_paged_begin(C.byref(oix._c), q.ctypes.data_as(C.c_void_p), L)
    if not h:
        raise RuntimeError("orc_paged_begin failed")
    pages, empty = [], 0
    try:
        while (calls is None and empty < 2) or (calls is not None and len(pages) < calls):
            k = sizes[len(pages) % len(sizes)]
            ids, d = np.empty(k, np.uint32), np.empty(k, np.float32)
            n = lib.orc_paged_next(h, k, ids.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
            if n < 0:
                raise RuntimeError(f"orc_paged_next failed: {n}")
            empty = empty + 1 if n == 0 else 0
            pages.append((ids[:n].copy(), d[:n].copy()))
    finally:
        lib.orc_paged_end(h)
    return pages


def second_phase_model(b, j, L, W, radius, initial_slack=1.0, range_slack=1.0, max_returned=0, inner_radius=None):
    """range_search.rs' second phase restated over the oracle's distances, to see what the oracle does not report: the
    in-range entries of the first phase and the candidates each hop yields.  Returns (first-phase entries within the
    radius, the largest number of candidates of one hop, the result ids); the caller holds the ids against the oracle's
    own and trusts the two counts only where they agree (the model does not know how the queue orders equal distances)"""
    x, oix = b.ix, b.oix
    D = b.distances(j)
    ids, d, cnt, _ = oix.search_batch(b.q_ref[j:j + 1], L, W, L)
    ids, d = ids[0, :cnt[0]].astype(np.int64), d[0, :cnt[0]]
    starts = np.arange(b.n, b.n + x.nstart)
    all_ids, all_d = np.concatenate([ids, starts]), np.concatenate([d, D[starts]])
    order = np.argsort(all_d, kind="stable")[:L]
    keep = [int(all_ids[i]) for i in order if all_d[i] <= np.float32(radius)]
    first = len(keep)
    visited = set(keep)
    limit = np.float32(radius) * np.float32(range_slack)
    max_ret = max_returned or 1 << 62
    most = 0
    if first >= int(np.float32(L) * np.float32(initial_slack)) and first < max_ret:
        front = 0
        adj = oix.adj
        while front < len(keep) and len(keep) < max_ret:
            beam = keep[front:front + W]
            front += len(beam)
            cand = []
            for node in beam:
                for nb in adj[node, 1:1 + int(adj[node, 0])]:
                    nb = int(nb)
                    if nb not in visited:
                        visited.add(nb)
                        if not np.isnan(D[nb]):
                            cand.append(nb)
            most = max(most, len(cand))
            for nb in cand:
                if D[nb] <= limit and len(keep) < max_ret:
                    keep.append(nb)
    inner = -np.inf if inner_radius is None else np.float32(inner_radius)
    return first, most, [i for i in keep if i < b.n and inner < D[i] <= np.float32(radius)]
