"""The exhaustive scan over PQ code rows without a GPU: the three declarations of its entry points (include/dann.h,
diskann_amd/_ffi.py, bindings/rust/dann_sys.rs), the sizing header (diskann_amd/csrc/flat_pq_plan.h) compiled with g++ and
checked over a grid of shapes, and the closed form of the queue inserts on PQ-like distance sequences.  The GPU side:
tests/test_gpu_pq_linear.py."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import flat_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dann_pq_linear_search_batch", "dann_pq_linear_search_batch_device")


def test_header_ffi_and_rust_declare_the_pq_linear_search():
    from diskann_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "dann.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "dann_sys.rs")).read()
    for name in NAMES:
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr)
        assert m, name
        args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
        assert len(args) == 11 and args[0] == "dann_index* idx" and args[1].startswith("const float*"), args
        assert args[7].startswith("const dann_flat_filter*") and args[-1].startswith("dann_search_stats*"), args
        res, argtypes = _ffi.SYMBOLS[name]
        assert res is _ffi._i32 and len(argtypes) == 11
        for i, (a, t) in enumerate(zip(args, argtypes)):
            assert (t is _ffi._u32) == a.startswith("uint32_t "), (name, a)
            if i != 7:
                assert (t is _ffi._vp) == ("*" in a), (name, a)
        r = re.search(r"pub fn " + name + r"\((.*?)\) -> i32;", rs)
        assert r, name
        rargs = r.group(1).split(", ")
        assert len(rargs) == 11 and rargs[0] == "idx: *mut DannIndex" and rargs[1].endswith("*const f32")
        assert rargs[7].endswith("*const DannFlatFilter") and rargs[8].endswith("*mut u32")
        assert rargs[9].endswith("*mut f32") and rargs[10].endswith("*mut DannSearchStats")
    assert "algos.rs:42-99" in hdr and "fixed_chunk_pq_table.rs" in hdr
    assert re.search(r"#define DANN_ABI_VERSION 5\b", hdr)


# ---- the sizing header ---------------------------------------------------------------------------------------------------
DRIVER = r"""
#include "flat_pq_plan.h"
#include <stdio.h>
using namespace dann;

// first the header's constants; then one case per line: chunks first n nq k cus forced -> the plan, then how the slot
// chunks cover [first, first + n)
int main() {
    unsigned chunks, first, n, nq, k, cus, forced;
    printf("%u %u %u\n", kFlatPqThreads, kFlatPqWideThreads, kFlatPqMinChunkRows);
    while (scanf("%u %u %u %u %u %u %u", &chunks, &first, &n, &nq, &k, &cus, &forced) == 7) {
        const FlatPqPlan p = flat_pq_plan(chunks, n, nq, k, cus, forced);
        unsigned long long covered = 0, bad = 0, expect = first;
        if ((unsigned long long)p.nchunks <= 100000)  // (walked where that is quick; the count is checked for all)
            for (unsigned c = 0; c < p.nchunks; ++c) {
                const unsigned long long lo = flat_pq_chunk_lo(p, first, c), hi = flat_pq_chunk_hi(p, first, n, c);
                if (lo != expect || hi <= lo || hi - lo > p.chunk_rows) ++bad;
                covered += hi - lo;
                expect = hi;
            }
        else
            covered = n, expect = (unsigned long long)first + n;
        if (p.nchunks && expect != (unsigned long long)first + n) ++bad;
        printf("%u %u %u %u %u %u %zu %zu %zu %zu %zu %llu %llu %u\n", p.tile, p.cap, p.chunk_rows, p.nchunks, p.batch, p.merge_cap,
               p.scan_lds, p.merge_lds, p.scratch_bytes(), p.table_bytes(), p.list_bytes(), covered, bad, p.threads);
    }
    return 0;
}
"""

LDS_BUDGET = 150 * 1024
SCRATCH_BUDGET = 192 << 20
# (chunks, first, n, nq, k, cus, forced chunk rows): every chunk count on either side of a code-row load width and of the
# tile-shrinking LDS limits, the smallest and the largest k, query counts around every tile size, and row counts from one
# row to the largest index
PLAN_CASES = [c for c in itertools.product((1, 3, 4, 5, 15, 16, 17, 18, 32, 36, 37, 64, 65, 73, 74, 128), (0,),
                                           (1, 255, 256, 257, 4097, 1000000), (1, 2, 3, 5, 9, 17, 4096), (1, 10, 257, 1024),
                                           (256,), (0, 1500))]
PLAN_CASES += [(16, 7, 1501, 11, 10, 304, 100), (16, 4294967295 - 5000, 5000, 9, 10, 304, 999), (128, 0, 2147483646, 1, 1024, 256, 0),
               (16, 0, 4294967295, 100000, 1, 256, 0), (64, 0, 100, 1000000, 1024, 8, 0), (1, 0, 2147483646, 1, 1, 0, 0),
               (128, 0, 1000000, 600000, 1024, 256, 0)]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("flat_pq_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diskann_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    lines = "".join(" ".join(map(str, c)) + "\n" for c in PLAN_CASES)
    r = subprocess.run([str(exe)], input=lines, capture_output=True, text=True, timeout=120, check=True)
    got = [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    threads, wide, min_rows = got.pop(0)
    # lane = row: a step is one row per thread of a workgroup of whole wavefronts
    assert threads % 64 == 0 and wide % 64 == 0 and 64 <= threads < wide <= 1024 and min_rows % wide == 0
    assert len(got) == len(PLAN_CASES)
    return (threads, wide), min_rows, got


def cases(plans):
    return zip(PLAN_CASES, plans[2])


def test_every_accepted_shape_has_a_tile_within_the_lds_budget(plans):
    narrow, wide = plans[0]
    seen = set()
    for case, p in cases(plans):
        chunks, first, n, nq, k, cus, forced = case
        tile, cap, chunk_rows, nchunks, batch, merge_cap, scan_lds, merge_lds, scratch, tables, lists, covered, bad, threads = p
        assert tile in (1, 2, 4, 8), case
        assert tile == 1 or tile // 2 < nq, case
        # the candidate buffer keeps a whole step (a row per thread) of headroom above k
        assert threads in (narrow, wide), case
        seen.add(threads)
        assert cap & (cap - 1) == 0 and cap >= k + threads and cap < 2 * (k + threads), case
        assert merge_cap & (merge_cap - 1) == 0 and merge_cap >= 2 * k, case
        # a table is `chunks` KiB per query; with the buffer, its fill count, threshold key and row count
        assert scan_lds == tile * (chunks * 1024 + cap * 8 + 16), case
        assert scan_lds <= LDS_BUDGET and merge_cap * 8 <= merge_lds <= LDS_BUDGET, case
        # the tile is the largest that fits and is useful at the narrow workgroup; the wide one is taken only where the
        # query tiles fill the device (two workgroups a compute unit) and it leaves that tile as it is
        narrow_cap = 1 << (k + narrow - 1).bit_length()
        if tile < 8 and tile < nq:
            assert 2 * tile * (chunks * 1024 + narrow_cap * 8 + 16) > LDS_BUDGET, case
        if threads == wide:
            assert -(-nq // tile) >= 2 * (cus or 256), case
    assert seen == {narrow, wide}


def test_chunks_cover_the_range_exactly_once(plans):
    min_rows = plans[1]
    for case, p in cases(plans):
        chunks, first, n, nq, k, cus, forced = case
        tile, cap, chunk_rows, nchunks, batch, merge_cap, scan_lds, merge_lds, scratch, tables, lists, covered, bad, threads = p
        assert bad == 0 and covered == n, case
        assert nchunks == -(-n // chunk_rows), case
        if forced:
            assert chunk_rows == forced, case
        else:
            assert chunk_rows >= min_rows and (chunk_rows % threads == 0 or nchunks == 1), case


def test_batch_respects_scratch_and_the_grid_limits(plans):
    for case, p in cases(plans):
        chunks, first, n, nq, k, cus, forced = case
        tile, cap, chunk_rows, nchunks, batch, merge_cap, scan_lds, merge_lds, scratch, tables, lists, covered, bad, threads = p
        assert 1 <= batch <= nq and (batch == nq or batch % tile == 0), case
        assert -(-batch // tile) <= 65535 and nchunks <= 2 ** 31 - 1, case
        assert tables == batch * chunks * 1024 and lists == batch * nchunks * k * 8, case
        assert scratch == tables + lists + batch * nchunks * 4, case
        assert scratch <= SCRATCH_BUDGET or batch == min(tile, nq), case  # (one tile is the least a launch takes)
        # launches of equal size, up to the rounding to whole tiles: no short last launch
        launches = -(-nq // batch)
        last = nq - (launches - 1) * batch
        assert 1 <= last <= batch and last >= batch - launches * tile, case
    # the default sizing fills the device at one query and stages a table once per query tile at many
    by = dict(cases(plans))
    one = by[(16, 0, 1000000, 1, 10, 256, 0)]
    assert one[0] == 1 and 128 <= one[3] <= 512
    many = by[(16, 0, 1000000, 4096, 10, 256, 0)]
    assert many[0] == 4 and many[3] == 1 and many[-1] == 1024
    wide = by[(64, 0, 1000000, 4096, 10, 256, 0)]  # 64 KiB of table a query: two launches, of 2 048 queries each
    assert wide[0] == 2 and wide[4] == 2048 and wide[-1] == 512


# ---- the selection rule on PQ-like sequences -----------------------------------------------------------------------------
def test_closed_form_equals_the_literal_inserts_on_pq_like_sequences():
    """sums of a few table entries: duplicate code rows give exact ties in long runs; tables with +-inf entries give +-inf
    and (inf - inf) NaN sums"""
    rng = np.random.default_rng(20)
    for trial in range(120):
        chunks = int(rng.integers(1, 5))
        lut = rng.standard_normal((chunks, 256)).astype(np.float32)
        if trial % 3 == 1:
            lut[rng.integers(0, chunks), rng.integers(0, 256, 40)] = np.inf
            lut[rng.integers(0, chunks), rng.integers(0, 256, 40)] = -np.inf
        distinct = rng.integers(0, 256, (int(rng.integers(1, 12)), chunks))
        codes = distinct[rng.integers(0, len(distinct), int(rng.integers(0, 90)))]
        d = np.zeros(len(codes), np.float32)
        with np.errstate(invalid="ignore"):
            for c in range(chunks):
                d = d + lut[c, codes[:, c]]
        for k in (1, 2, 10, 64, 257):
            pa, da_ = fm.flat_knn(d, k)
            pb, db = fm.flat_knn_closed(d, k)
            assert pa.tolist() == pb.tolist(), (trial, k)
            assert np.array_equal(da_.view(np.uint32), db.view(np.uint32)), (trial, k)
            assert len(pa) == min(k, int((~np.isnan(d)).sum()))
            # among equal distances the later position comes first
            for a, b in zip(range(len(pa) - 1), range(1, len(pa))):
                if da_[a] == da_[b]:
                    assert pa[a] > pa[b], (trial, k)


def test_a_sum_of_table_entries_is_never_negative_zero():
    """+0.0 + -0.0 == +0.0 and x + -x == +0.0: the key of the scan (which folds -0.0 into +0.0) loses nothing"""
    z = np.float32(0.0)
    for x in (np.float32(-0.0), np.float32(0.0)):
        assert not np.signbit(z + x)
    for x in (np.float32(1.5), np.float32(1e-45), np.float32(3e38)):
        assert not np.signbit((z + x) + -x) and not np.signbit((z + -x) + x)
