"""Exhaustive (flat) k-NN without a GPU: the CPU model (tests/flat_model.py) against itself and against the reference's
goldens, the sizing header (diskann_amd/csrc/flat_plan.h) compiled with g++, and the three declarations of the entry
points (include/dann.h, diskann_amd/_ffi.py, bindings/rust/dann_sys.rs).  The GPU side: tests/test_gpu_flat.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import flat_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sequential_inserts_equal_the_closed_form():
    """random sequences with heavy ties, both zeros, infinities and NaNs, k below, at and above the length"""
    rng = np.random.default_rng(7)
    pool = np.array([0.0, -0.0, 1.0, 1.0, 2.0, 2.5, -3.0, np.inf, -np.inf, np.nan, 7.0], np.float32)
    for trial in range(400):
        n = int(rng.integers(0, 60))
        d = pool[rng.integers(0, len(pool) if trial % 2 else 5, n)]
        for k in (1, 2, 5, 10, 64):
            pa, da_ = fm.flat_knn(d, k)
            pb, db = fm.flat_knn_closed(d, k)
            assert pa.tolist() == pb.tolist(), (trial, k, d.tolist())
            assert np.array_equal(da_.view(np.uint32), db.view(np.uint32)), (trial, k)
            assert len(pa) == min(k, int((~np.isnan(d)).sum()))


def test_tie_rule_in_words():
    """an equal distance goes in front of the equal ones already there; at the k-th place the later one wins"""
    pos, d = fm.flat_knn([5.0, 1.0, 5.0, 5.0, np.nan, 9.0], 3)
    assert pos.tolist() == [1, 3, 2] and d.tolist() == [1.0, 5.0, 5.0]
    pos, _ = fm.flat_knn([0.0, -0.0, 0.0], 2)
    assert pos.tolist() == [2, 1]


@pytest.mark.parametrize("name,row", fm.golden_rows(), ids=lambda v: v if isinstance(v, str) else f"k{v['k']}q{v['query'][0]:g}")
def test_model_reproduces_the_goldens(name, row):
    rows = fm.grid_rows(row["grid_dims"], row["grid_size"])
    assert len(rows) == row["metrics"]["count"]
    dist = fm.l2_f32(row["query"], rows)
    k = row["k"]
    pos, d = fm.flat_knn(dist, k)
    assert d.tolist() == row["top_k_distances"]
    assert len(dist) == row["comparisons"]          # cmps: every row evaluated
    assert len(pos) == row["result_count"] == min(k, len(rows))
    gt_ids = [int(i) for i, _ in row["ground_truth"]]
    assert [float(x) for _, x in row["ground_truth"]] == d.tolist()
    # the golden's ids are the brute force's (distance, id ascending): the same set wherever the k-th and the (k+1)-th
    # distance differ; on a boundary tie the queue keeps the later id
    s = np.sort(dist)
    if len(s) <= k or s[k - 1] != s[k]:
        assert sorted(gt_ids) == sorted(pos.tolist())
    else:
        tied = np.flatnonzero(dist == s[k - 1])
        kept = [p for p in pos.tolist() if dist[p] == s[k - 1]]
        assert kept == sorted(tied.tolist(), reverse=True)[:len(kept)]


def test_goldens_have_boundary_ties():
    """the 2 x 5 and 3 x 4 lattices tie at the k-th place for some k: what the id comparison on the GPU is for"""
    tie = set()
    for name, row in fm.golden_rows():
        s = np.sort(fm.l2_f32(row["query"], fm.grid_rows(row["grid_dims"], row["grid_size"])))
        if len(s) > row["k"] and s[row["k"] - 1] == s[row["k"]]:
            tie.add(name)
    assert {"search_2_5", "search_3_4"} <= tie


DRIVER = r"""
#include "flat_plan.h"
#include <stdio.h>
using namespace dann;

// one case per line: first n nq k qslot cus forced -> the plan, then how often each slot of [first, first + n) is covered
int main() {
    unsigned first, n, nq, k, qslot, cus, forced;
    while (scanf("%u %u %u %u %u %u %u", &first, &n, &nq, &k, &qslot, &cus, &forced) == 7) {
        const FlatPlan p = flat_plan(n, nq, k, qslot, cus, forced);
        unsigned long long covered = 0, bad = 0, expect = first;
        for (unsigned c = 0; c < p.nchunks; ++c) {
            const unsigned long long lo = flat_chunk_lo(p, first, c), hi = flat_chunk_hi(p, first, n, c);
            if (lo != expect || hi <= lo || hi - lo > p.chunk_rows) ++bad;
            covered += hi - lo;
            expect = hi;
        }
        if (p.nchunks && expect != (unsigned long long)first + n) ++bad;
        printf("%u %u %u %u %u %u %zu %zu %zu %llu %llu\n", p.tile, p.cap, p.chunk_rows, p.nchunks, p.batch, p.merge_cap,
               p.scan_lds, p.merge_lds, p.scratch_bytes(), covered, bad);
    }
    return 0;
}
"""

# (first, n, nq, k, qslot, cus, forced chunk rows)
PLAN_CASES = [
    (0, 1, 1, 1, 512, 256, 0), (0, 1500, 11, 10, 512, 256, 0), (0, 1500, 11, 10, 512, 256, 64), (0, 1500, 11, 65, 400, 256, 100),
    (7, 1501, 11, 1024, 128, 256, 100), (3, 63, 1, 10, 64, 256, 64), (0, 64, 2, 10, 64, 256, 64), (1, 65, 3, 10, 64, 256, 64),
    (0, 1000000, 1, 10, 512, 256, 0), (0, 1000000, 64, 10, 128, 256, 0), (0, 1000000, 4096, 10, 3072, 256, 0),
    (0, 1000000, 4096, 1024, 3072, 256, 0), (4294967295 - 5000, 5000, 9, 10, 512, 304, 999), (0, 4294967295, 1, 1, 16, 256, 0),
    (0, 100, 100000, 10, 512, 256, 0), (0, 1000, 8, 1024, 16384, 256, 0), (0, 1000, 8, 1024, 140000, 256, 0),
]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("flat_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diskann_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    lines = "".join(" ".join(map(str, c)) + "\n" for c in PLAN_CASES)
    r = subprocess.run([str(exe)], input=lines, capture_output=True, text=True, timeout=60, check=True)
    got = [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    assert len(got) == len(PLAN_CASES)
    return got


def test_chunks_cover_the_range_exactly_once(plans):
    for case, p in zip(PLAN_CASES, plans):
        first, n, nq, k, qslot, cus, forced = case
        tile, cap, chunk_rows, nchunks, batch, merge_cap, scan_lds, merge_lds, scratch, covered, bad = p
        if tile == 0:
            assert qslot == 140000, case  # the one case whose query does not fit the LDS
            continue
        assert bad == 0 and covered == n, case
        assert nchunks == -(-n // chunk_rows), case
        if forced:
            assert chunk_rows == forced, case


def test_plan_respects_its_limits(plans):
    for case, p in zip(PLAN_CASES, plans):
        first, n, nq, k, qslot, cus, forced = case
        tile, cap, chunk_rows, nchunks, batch, merge_cap, scan_lds, merge_lds, scratch, covered, bad = p
        if tile == 0:
            continue
        assert tile in (1, 2, 4, 8) and (tile == 1 or tile // 2 < nq), case
        # the candidate buffer keeps a whole step of headroom above k; the merge buffer takes k new keys per round at least
        assert cap & (cap - 1) == 0 and cap >= k + 256, case
        assert merge_cap & (merge_cap - 1) == 0 and merge_cap >= 2 * k, case
        assert tile * (qslot + cap * 8 + 12) + 4 <= scan_lds <= 160 * 1024, case
        assert merge_cap * 8 + qslot <= merge_lds <= 160 * 1024, case
        assert 1 <= batch <= nq and (batch == nq or batch % tile == 0) and -(-batch // tile) <= 65535, case
        assert scratch >= batch * nchunks * k * 8 + nchunks * 4, case
        if not forced:
            assert chunk_rows % 256 == 0 and chunk_rows >= 1024, case
    # the default sizing fills the device: at one query a million rows make at least one workgroup per compute unit
    one = dict(zip(PLAN_CASES, plans))[(0, 1000000, 1, 10, 512, 256, 0)]
    assert one[0] == 1 and 256 <= one[3] <= 4096


def test_header_ffi_and_rust_declare_the_flat_search():
    from diskann_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "dann.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "dann_sys.rs")).read()
    dbg = open(os.path.join(ROOT, "include", "dann_debug.h")).read()
    for name in ("dann_flat_search_batch", "dann_flat_search_batch_device"):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr)
        assert m, name
        args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
        assert len(args) == 10 and args[0] == "dann_index* idx" and args[-1].startswith("dann_search_stats*"), args
        res, argtypes = _ffi.SYMBOLS[name]
        assert res is _ffi._i32 and len(argtypes) == 10
        # pointers where the header has pointers, u32 where it has uint32_t
        for a, t in zip(args, argtypes):
            assert (t is _ffi._vp) == ("*" in a) and (t is _ffi._u32) == a.startswith("uint32_t "), (name, a)
        r = re.search(r"pub fn " + name + r"\((.*?)\) -> i32;", rs)
        assert r, name
        rargs = r.group(1).split(", ")
        assert len(rargs) == 10 and rargs[0] == "idx: *mut DannIndex" and rargs[1].endswith("*const c_void")
        assert rargs[7].endswith("*mut u32") and rargs[8].endswith("*mut f32") and rargs[9].endswith("*mut DannSearchStats")
    assert re.search(r"DANN_FLAT_SKIP_DELETED\s*=\s*1\b", hdr) and _ffi.FLAT_SKIP_DELETED == 1
    assert "queue.rs:130-171" in hdr and "scan position descending" in hdr
    assert re.search(r"DANN_DBG_FLAT_CHUNK_ROWS\s*=\s*21\b", dbg) and re.search(r"DANN_DBG_COUNT\s*=\s*22\b", dbg)
    assert _ffi.DBG_FLAT_CHUNK_ROWS == 21 == _ffi.DBG_KEYS["flat_chunk_rows"]
    assert re.search(r"#define DANN_ABI_VERSION 5\b", hdr)
