"""The models of the exhaustive ground-truth scans (tests/flat_gt_model.py) against the reference's goldens, the literal
inserts against the closed form under masks, the planning header flat_gt_plan.h compiled with g++, and the boundary
(header, ctypes table).  No GPU."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import flat_gt_model as gt
import flat_model as fm
from filtered_cases import build
from helpers import bits as fbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("dann_flat_filtered_search_batch", "dann_flat_range_search_batch", "dann_flat_filtered_search_batch_device",
           "dann_flat_range_search_batch_device")


# ---- 1. the models against the reference's goldens ------------------------------------------------------------------------
# The graph searches return a subset of what an exhaustive scan of the points (slots [0, n), the start point left out as
# the searches leave it out of their results) returns; where they find everything, the two are equal.
@pytest.fixture(scope="module")
def filtered_golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "filtered_search.json")))


def _points_only(g, rule):
    m = g.match(rule).copy()
    m[g.n:] = False
    return m[:g.n]


def _range_case(c, match_rule):
    g = build("grid", c["grid_dims"], c["grid_size"])
    dist = fm.l2_f32(c["query"], g.data)
    pos, d = gt.range_scan(dist, _points_only(g, match_rule), c["radius"], c["inner_radius"])
    got_ids = [int(r[0]) for r in c["results"]]
    got_d = np.array([r[1] for r in c["results"]], np.float32)
    # a subset of the exhaustive set, every distance bit-equal to the scan's
    assert set(got_ids) <= set(pos.tolist()), c["name"]
    assert np.array_equal(fbits(got_d), fbits(dist[got_ids])), c["name"]
    return set(got_ids), pos


def test_range_goldens_are_subsets_of_the_exhaustive_scan(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "range_search.json")))
    assert len(cases) == 5
    full = {"basic_range_search": 11, "inner_radius_filtering": 22, "two_round_search": 109}
    for c in cases:
        got, pos = _range_case(c, "all")
        if c["name"] in full:
            assert got == set(pos.tolist()) and len(pos) == full[c["name"]], c["name"]
        else:  # the two capped cases
            assert c["max_returned"] in (4, 5) and len(got) <= c["max_returned"] and len(pos) == 125, c["name"]
    assert sum(c["name"] in full for c in cases) == 3


def test_filtered_range_goldens_are_subsets_of_the_exhaustive_scan(filtered_golden):
    cases = filtered_golden["filtered_range"]
    assert len(cases) == 7
    div4 = []
    for c in cases:
        got, pos = _range_case(c, c["filter"])
        if c["name"] == "max_results_respected_means_no_second_round":
            assert len(got) == 3 and len(pos) == 109
        else:
            assert got == set(pos.tolist()), c["name"]
        if c["filter"] == "div4":
            div4.append(len(pos))
    assert sorted(div4) == [1, 28]


INLINE_EQUAL = {"inline_adaptive_l_logarithmic", "inline_adaptive_l_max", "inline_adaptive_l_no_scaling",
                "inline_fixed_no_scaling", "inline_search_reaches_matches_through_non_matching_nodes",
                "inline_search_returns_only_final_level_matches", "inline_search_three_level_adaptive_l_with_l1_finds_matches"}


def _knn_case(g, c, ids, dists):
    match = _points_only(g, c["filter"])
    dist = fm.l2_f32(c["query"], g.data)
    (pos, d), (cpos, cd) = gt.filtered_knn(dist, match, c["k"])
    assert pos.tolist() == cpos.tolist() and np.array_equal(fbits(d), fbits(cd)), c["name"]
    slot_of = {int(o): s for s, o in enumerate(g.orig)}
    slots = [slot_of[int(i)] for i in ids]
    assert all(s < g.n and match[s] for s in slots), c["name"]
    got = np.sort(np.array(dists, np.float32))
    assert len(got) <= len(d) and (got >= d[:len(got)]).all(), c["name"]
    return len(got) == len(d) and np.array_equal(got, d)


def test_inline_goldens_never_beat_the_exhaustive_scan(filtered_golden):
    cases = filtered_golden["inline"]
    assert len(cases) == 12
    equal = set()
    for c in cases:
        if _knn_case(build(c["graph"]), c, c["result_ids"], c["result_distances"]):
            equal.add(c["name"])
        elif c["name"] not in INLINE_EQUAL:
            (pos, d), _ = gt.filtered_knn(fm.l2_f32(c["query"], build(c["graph"]).data),
                                          _points_only(build(c["graph"]), c["filter"]), c["k"])
            assert len(c["result_ids"]) < len(pos), c["name"]  # the other five return fewer than the exhaustive count
    assert equal == INLINE_EQUAL


def test_multihop_goldens_equal_the_exhaustive_scan(filtered_golden):
    cases = filtered_golden["multihop"]
    assert len(cases) == 2
    for c in cases:
        g = build(c["graph"], grid_size=c["grid_size"])
        assert _knn_case(g, c, [r[0] for r in c["results"]], [r[1] for r in c["results"]]), c["name"]


# ---- 2. literal inserts against the closed form, under masks ---------------------------------------------------------------
def test_masked_inserts_equal_the_closed_form():
    rng = np.random.default_rng(21)
    pool = np.array([0.0, -0.0, 1.0, 1.0, 2.0, 2.5, -3.0, np.inf, -np.inf, np.nan, 7.0], np.float32)
    for trial in range(300):
        n = int(rng.integers(0, 40))
        seq = pool[rng.integers(0, len(pool), n)]
        match = rng.random(n) < rng.choice([0.0, 0.1, 0.5, 1.0])
        for k in (1, 3, max(1, n), n + 2):
            (pos, d), (cpos, cd) = gt.filtered_knn(seq, match, k)
            assert pos.tolist() == cpos.tolist() and np.array_equal(fbits(d), fbits(cd)), (trial, k)
            assert match[pos].all() and len(pos) == min(k, int((match & ~np.isnan(seq)).sum()))
        # an all-ones mask is flat_model itself
        (pos, d), _ = gt.filtered_knn(seq, np.ones(n, bool), 3)
        wpos, wd = fm.flat_knn(seq, 3)
        assert pos.tolist() == wpos.tolist() and np.array_equal(fbits(d), fbits(wd))


def test_range_predicate_in_words():
    d = np.array([1.0, np.nan, 2.0, -0.0, 2.0, 3.0, 0.0], np.float32)
    on = np.ones(7, bool)
    pos, out = gt.range_scan(d, on, 2.0)
    assert pos.tolist() == [0, 2, 3, 4, 6] and np.signbit(out[2])  # inclusive radius, NaN fails, -0.0 stays -0.0
    pos, _ = gt.range_scan(d, on, 2.0, inner=1.0)
    assert pos.tolist() == [2, 4]  # the inner radius is exclusive: d <= inner is out
    pos, _ = gt.range_scan(d, np.array([1, 1, 0, 0, 1, 1, 0], bool), 2.0)
    assert pos.tolist() == [0, 4]
    pos, _ = gt.range_scan(d, on, -1.0)
    assert len(pos) == 0


# ---- 3. the planning header -----------------------------------------------------------------------------------------------
DRIVER = r"""
#include "flat_gt_plan.h"
#include <stdio.h>
#include <algorithm>
#include <vector>
using namespace dann;

// one case per line: n nq k qslot cus forced -> the filtered plan, the range plan and the offsets of a query's chunks
int main() {
    unsigned n, nq, k, qslot, cus, forced;
    while (scanf("%u %u %u %u %u %u", &n, &nq, &k, &qslot, &cus, &forced) == 6) {
        const FlatFilteredPlan f = flat_filtered_plan(n, nq, k, qslot, cus, forced);
        const FlatRangePlan r = flat_range_plan(n, nq, qslot, cus, forced);
        // the offsets kernel's two-level scan, by the functions it calls, over counts c % 7: every chunk's offset is the
        // number of matches in front of it, so the chunks' segments tile [0, total) exactly
        unsigned bad = 0;
        const unsigned nch = r.nchunks < 200000 ? r.nchunks : 200000, per = flat_range_run_chunks(nch);
        std::vector<uint32_t> counts(nch), sums(kFlatThreads);
        for (unsigned c = 0; c < nch; ++c) counts[c] = c % 7;
        for (unsigned t = 0; t < kFlatThreads; ++t) {
            const unsigned c0 = std::min(t * per, nch), c1 = std::min(c0 + per, nch);
            sums[t] = 0;
            for (unsigned c = c0; c < c1; ++c) sums[t] += counts[c];
        }
        const uint32_t total = flat_range_exclusive_scan(sums.data(), kFlatThreads, 0u);
        for (unsigned t = 0; t < kFlatThreads; ++t) {
            const unsigned c0 = std::min(t * per, nch), c1 = std::min(c0 + per, nch);
            flat_range_exclusive_scan(counts.data() + c0, c1 - c0, sums[t]);
        }
        uint32_t expect = 0;
        for (unsigned c = 0; c < nch; ++c) {
            if (counts[c] != expect) ++bad;
            expect += c % 7;
        }
        if (expect != total || (uint64_t)per * kFlatThreads < nch) ++bad;
        printf("%u %u %u %u %zu %zu %zu %u %u %u %u %zu %zu %u\n", f.p.tile, f.p.chunk_rows, f.p.nchunks, f.p.batch, f.p.scan_lds,
               f.p.merge_lds, f.scratch_bytes(), r.tile, r.chunk_rows, r.nchunks, r.batch, r.lds, r.scratch_bytes(), bad);
    }
    return 0;
}
"""

# (n, nq, k, qslot, cus, forced chunk rows)
PLAN_CASES = [
    (1, 1, 1, 512, 256, 0), (1500, 11, 10, 512, 256, 0), (1500, 11, 10, 512, 256, 64), (1500, 11, 65, 400, 256, 100),
    (1501, 11, 1024, 128, 256, 100), (63, 1, 10, 64, 256, 64), (1000000, 1, 10, 512, 256, 0), (1000000, 64, 10, 512, 256, 0),
    (1000000, 4096, 10, 512, 256, 0), (1000000, 4096, 1024, 3072, 256, 0), (4294967295, 1, 1, 16, 256, 0),
    (100, 100000, 10, 512, 256, 0), (1000, 8, 1024, 16384, 256, 0), (0, 5, 10, 512, 256, 0), (100000000, 100000, 1024, 512, 256, 0),
]
LDS_BUDGET, SCRATCH_BUDGET = 150 * 1024, 192 << 20


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("flat_gt_plan")
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


def test_plans_keep_whole_tiles_and_their_budgets(plans):
    for case, p in zip(PLAN_CASES, plans):
        n, nq, k, qslot, cus, forced = case
        ftile, frows, fchunks, fbatch, flds, fmerge, fscratch, rtile, rrows, rchunks, rbatch, rlds, rscratch, bad = p
        assert bad == 0, case  # the chunks' offsets tile the output exactly
        # range
        assert rtile in (1, 2, 4, 8) and (rtile == 1 or rtile // 2 < nq), case
        assert rchunks == -(-n // rrows) and (not forced or rrows == forced), case
        assert 1 <= rbatch <= nq and (rbatch == nq or rbatch % rtile == 0) and -(-rbatch // rtile) <= 65535, case
        assert rlds <= LDS_BUDGET and rlds >= rtile * (qslot + 256 * 4) + 4352 * 5, case
        assert rscratch >= rbatch * rchunks * 8 + 4, case
        assert rbatch == rtile or rbatch * rchunks * 8 <= SCRATCH_BUDGET, case
        # filtered k-NN
        if n == 0:
            assert ftile == 0, case  # (an empty range is answered without a plan)
            continue
        assert ftile in (1, 2, 4, 8), case
        assert fchunks == -(-n // frows) and (not forced or frows == forced), case
        assert 1 <= fbatch <= nq and (fbatch == nq or fbatch % ftile == 0) and -(-fbatch // ftile) <= 65535, case
        cap = 1 << (k + 256 - 1).bit_length()
        assert ftile * (qslot + cap * 8 + 16) + 4352 * 5 <= flds <= LDS_BUDGET and fmerge <= LDS_BUDGET, case
        assert fscratch == fbatch * fchunks * (k * 8 + 4), case
        assert fbatch == ftile or fscratch <= SCRATCH_BUDGET, case


PIECE_DRIVER = r"""
#include "flat_gt_plan.h"
#include <stdio.h>
int main() {
    unsigned nq, cap;
    unsigned long long stride;
    while (scanf("%u %llu %u", &nq, &stride, &cap) == 3) printf("%u\n", dann::flat_host_piece(nq, stride, cap));
    return 0;
}
"""


def test_host_forms_cut_a_call_into_pieces_that_fit_the_stage(tmp_path):
    """flat_host_piece: at most 65 536 queries, 64 MiB of per-query bitmaps and 64 MiB of result places a piece, never
    fewer than one query; a shared bitmap (stride 0) and a count-only call (out_cap 0) do not bound it"""
    src, exe = tmp_path / "piece.cpp", tmp_path / "piece"
    src.write_text(PIECE_DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diskann_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    stage = 64 << 20
    cases = [(11, 0, 0), (11, 47, 1500), (100000, 0, 0), (100000, 31251, 0), (100000, 0, 4096), (100000, 31251, 1000000),
             (5, 1 << 40, 0), (5, 0, 0xFFFFFFFF), (4096, 31251, 5898), (1, 1, 1), (70000, 1, 1), (600, 31251, 0)]
    r = subprocess.run([str(exe)], input="".join(f"{a} {b} {c}\n" for a, b, c in cases), capture_output=True, text=True,
                       timeout=60, check=True)
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(cases)
    for (nq, stride, cap), piece in zip(cases, got):
        assert 1 <= piece <= min(nq, 65536), (nq, stride, cap)
        limit = min([nq, 65536] + ([stage // (stride * 4)] if stride else []) + ([stage // (cap * 4)] if cap else []))
        assert piece == max(1, limit), (nq, stride, cap)
        # a piece larger than one query fits the stage; the next larger one would not, or would pass a limit
        assert piece == 1 or (piece * stride * 4 <= stage and piece * cap * 4 <= stage), (nq, stride, cap)
    by = dict(zip(cases, got))
    assert by[(11, 47, 1500)] == 11 and by[(100000, 0, 0)] == 65536 and by[(5, 1 << 40, 0)] == 1
    assert by[(100000, 31251, 0)] == 536 and by[(600, 31251, 0)] == 536  # a million slots: 536 bitmaps at a time
    assert by[(100000, 0, 4096)] == 4096 and by[(100000, 31251, 1000000)] == 16


# ---- 4. the boundary ------------------------------------------------------------------------------------------------------
def test_header_and_ffi_declare_the_four_exports():
    from diskann_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "dann.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "dann_sys.rs")).read()
    for name in EXPORTS:
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr)
        assert m, name
        args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
        assert len(args) == (15 if "range" in name else 11) and "const dann_flat_filter*" in " ".join(args), name
        res, argtypes = _ffi.SYMBOLS[name]
        assert res is _ffi._i32 and len(argtypes) == len(args), name
        assert f"pub fn {name}(" in rs, name
    assert re.search(r"typedef struct \{\s*const uint32_t\* bits;[^}]*uint64_t stride_words;[^}]*\} dann_flat_filter;", hdr)
    assert re.search(r"^#define DANN_ABI_VERSION 5$", hdr, flags=re.M)
    assert _ffi.lib().dann_abi_version() == 5
