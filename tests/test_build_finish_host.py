"""The CPU restatement of the build-finishing steps (tests/build_finish_model.py): the medoid's sequential sums and first-minimum
rule, the known answers of the reference's graph/test/cases/index.rs (tests/golden/build_finish_cases.json), and the
exactness test of diskann_amd/csrc/seq_sum.h, compiled here with g++ and held against the restatement."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
import build_finish_model as model
from test_consolidate_host import square_cfg, square_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "build_finish_cases.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def fixture_index(g, graph, pruned_degree=1):
    return square_index(g, {"lists": g["graphs"][graph], "pruned_degree": pruned_degree})


def adversarial_column():
    """[2^60, 1 x 1000, -2^60]: the sequential sum is 0 (each 1 is lost below 2^60's last place); adding the ones first is not"""
    return np.array([2.0 ** 60] + [1.0] * 1000 + [-(2.0 ** 60)], np.float32)


# ---- the medoid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(1, 1), (2, 5), (65, 32), (300, 100), (257, 131)])
def test_medoid_agrees_with_the_oracle_on_f32(n, dim):
    rng = np.random.default_rng(n * 1000 + dim)
    x = rng.normal(size=(n, dim)).astype(np.float32)
    row, mean, nans = model.medoid(x)
    want_row, want_mean = oracle.medoid_f32(x)
    assert row == want_row and nans == 0
    assert np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32))


def test_sequential_sum_of_the_adversarial_column():
    col = adversarial_column()
    assert model.column_sums(col[:, None])[0] == 0.0
    assert float(np.sum(np.sort(col.astype(np.float64)))) != 0.0  # another order gives another sum
    total, par, ser = model.walk_column(col.astype(np.float64))
    assert total == 0.0 and ser > 0  # the test refuses the ranges that would round, and the walk returns the sequential value
    _, mean, _ = model.medoid(col[:, None])
    assert mean[0] == 0.0


def test_first_minimum_and_nan_rules():
    x = np.zeros((6, 3), np.float32)
    x[:, 0] = [5, 1, -1, 1, -1, 7]  # mean 2: rows 1 and 3 tie, row 1 wins
    assert model.medoid(x)[0] == 1
    y = x.copy()
    y[1] = np.nan  # the mean is NaN: every distance is, nothing wins
    row, mean, nans = model.medoid(y)
    assert row == -1 and nans == 6 and np.isnan(mean).all()
    assert model.medoid(np.zeros((0, 4), np.float32))[0] == -1
    for dt in (np.uint8, np.int8, np.float16):
        z = np.array([[1, 2], [3, 4], [5, 6], [3, 4]], dt)
        row, mean, _ = model.medoid(z)
        assert row == 1 and mean.tolist() == [3.0, 4.0]


def test_walk_equals_the_sequential_sum_on_both_paths():
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, 4097).astype(np.float64)
    grid = np.round(rng.normal(size=4097) * 1024) / 1024  # the 2^-10 grid
    for col in (u8, grid):
        total, par, ser = model.walk_column(col)
        assert total == model.column_sums(col[:, None])[0] and ser == 0 and par == 17
    wild = (rng.normal(size=3000) * 10.0 ** rng.integers(-12, 12, 3000)).astype(np.float32).astype(np.float64)
    total, par, ser = model.walk_column(wild)
    assert total == model.column_sums(wild[:, None])[0] and ser > 0


# ---- seq_sum.h on the host ------------------------------------------------------------------------------------------------
HARNESS = r"""
#include "seq_sum.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace dann;
// stdin: the columns, each a count (u64) and that many doubles.  Per column: the sequential sum's bits, the bits of
// the range walk (every range summed BACKWARDS where the test allows any order) and the two range counts.
int main() {
    uint64_t n;
    while (fread(&n, 8, 1, stdin) == 1) {
        std::vector<double> v(n);
        if (n && fread(v.data(), 8, n, stdin) != n) return 2;
        double seq = 0.0;
        for (double x : v) seq += x;
        const uint64_t nr = (n + kMedoidRangeRows - 1) / kMedoidRangeRows;
        std::vector<SeqSummary> s(nr);
        for (uint64_t k = 0; k < nr; ++k) {
            s[k] = SeqSummary{0.0, 0.0, kSeqNone};
            const uint64_t lo = k * kMedoidRangeRows, hi = lo + kMedoidRangeRows < n ? lo + kMedoidRangeRows : n;
            for (uint64_t i = hi; i > lo; --i) seq_take(s[k], v[i - 1]);
        }
        double acc = 0.0;
        uint64_t par = 0, ser = 0;
        for (uint64_t k0 = 0; k0 < nr; k0 += kMedoidGroupRanges) {
            const uint64_t k1 = k0 + kMedoidGroupRanges < nr ? k0 + kMedoidGroupRanges : nr;
            SeqSummary grp = s[k1 - 1];
            for (uint64_t k = k1 - 1; k > k0; --k) grp = seq_join(grp, s[k - 1]);
            if (seq_exact(acc, grp)) { acc += grp.S; par += k1 - k0; continue; }
            for (uint64_t k = k0; k < k1; ++k) {
                if (seq_exact(acc, s[k])) { acc += s[k].S; ++par; continue; }
                ++ser;
                const uint64_t lo = k * kMedoidRangeRows, hi = lo + kMedoidRangeRows < n ? lo + kMedoidRangeRows : n;
                for (uint64_t i = lo; i < hi; ++i) acc += v[i];
            }
        }
        uint64_t a, b;
        memcpy(&a, &seq, 8);
        memcpy(&b, &acc, 8);
        printf("%llu %llu %llu %llu\n", (unsigned long long)a, (unsigned long long)b, (unsigned long long)par,
               (unsigned long long)ser);
    }
    return 0;
}
"""


def seq_columns():
    rng = np.random.default_rng(17)
    cols = [adversarial_column().astype(np.float64),
            rng.integers(0, 256, 4097).astype(np.float64),
            rng.integers(-128, 128, 70000).astype(np.float64),
            rng.normal(size=4097).astype(np.float16).astype(np.float64),
            np.round(rng.normal(size=4097) * 1024) / 1024,
            rng.normal(size=4097).astype(np.float32).astype(np.float64),
            rng.normal(size=40000).astype(np.float32).astype(np.float64),
            (rng.normal(size=3000) * 10.0 ** rng.integers(-12, 12, 3000)).astype(np.float32).astype(np.float64),
            np.array([1.0, np.inf, 2.0, -np.inf] * 100),
            np.array([np.nan] + [1.0] * 300),
            np.zeros(600), np.array([]), np.array([5e-324] * 300 + [1.0]),
            np.array([1.7e308] * 300)]
    return cols


def test_seq_sum_header_on_the_host(tmp_path):
    """seq_sum.h's test, as the medoid uses it, never changes a bit of the sequential sum -- with every parallel range summed
    in the opposite order -- and takes the ranges the Python restatement takes"""
    src = tmp_path / "seq_harness.cpp"
    src.write_text(HARNESS)
    exe = str(tmp_path / "seq_harness")
    r = subprocess.run(["g++", "-std=c++20", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "diskann_amd", "csrc"),
                        str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cols = seq_columns()
    blob = b"".join(np.uint64(len(c)).tobytes() + np.ascontiguousarray(c, np.float64).tobytes() for c in cols)
    r = subprocess.run([exe], input=blob, capture_output=True, timeout=120)
    assert r.returncode == 0
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(cols)
    walked = 0
    for i, (col, line) in enumerate(zip(cols, lines)):
        seq, got, par, ser = (int(x) for x in line.split())
        assert seq == got, f"column {i}: the range walk changed the sum"
        total, mpar, mser = model.walk_column(col)
        seq_value = np.uint64(seq).view(np.float64)
        assert np.float64(total).view(np.uint64) == seq or (total != total and seq_value != seq_value), i
        assert (par, ser) == (mpar, mser), f"column {i}: header {(par, ser)}, restatement {(mpar, mser)}"
        walked += ser
    assert walked > 0
    # integer, f16 and gridded columns never leave the parallel path
    for i in (1, 2, 3, 4):
        assert int(lines[i].split()[3]) == 0, i


# ---- the reference's known answers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", golden()["reachable"], ids=lambda c: f"{c['graph']}-{c['starts']}")
def test_reachable_known_answers(case):
    g = golden()
    oix, _ = fixture_index(g, case["graph"])
    count, levels, reached = model.count_reachable(oix, case["starts"])
    assert count == case["count"] == int(reached.sum())
    assert model.count_reachable(oix, case["starts"] + case["starts"])[0] == case["count"]  # duplicates count once


def test_reachable_defaults_and_levels():
    g = golden()
    oix, _ = fixture_index(g, "square")
    assert model.count_reachable(oix)[:2] == model.count_reachable(oix, [4])[:2] == (5, 1)
    assert model.count_reachable(oix, [0])[1] == 2
    oix, _ = fixture_index(g, "isolated")
    assert model.count_reachable(oix, [4])[1] == 0


@pytest.mark.parametrize("case", golden()["degree_stats"], ids=lambda c: c["graph"])
def test_degree_stats_known_answers(case):
    g = golden()
    oix, _ = fixture_index(g, case["graph"])
    mx, avg, mn, lt2, points, total = model.degree_stats(oix)
    assert [mx, float(avg), mn, lt2] == case["expected"] and points == 4
    assert model.degree_stats(oix, []) == (0, 0.0, 0, 0, 0, 0)
    assert model.degree_stats(oix, [4, 4, 0])[4:] == (3, 2 * len(g["graphs"][case["graph"]][4]) + len(g["graphs"][case["graph"]][0]))


@pytest.mark.parametrize("case", golden()["prune_range"], ids=lambda c: c["graph"])
def test_prune_range_known_answers(case):
    g = golden()
    oix, _ = fixture_index(g, case["graph"], case["pruned_degree"])
    cfg = square_cfg(case)
    pruned, skipped = model.prune_range(oix, cfg, range(case["first"], case["first"] + case["n"]))
    assert pruned == 4 and skipped == 0
    for v, m in case["max_len"].items():
        assert len(oix.neighbors(int(v))) <= m
    for v, m in case["len"].items():
        assert len(oix.neighbors(int(v))) == m
    before = oix.adj.copy()
    assert model.prune_range(oix, cfg, range(5)) == (1, 0)  # now the start point as well
    assert model.prune_range(oix, cfg, range(5)) == (0, 0) and len(oix.neighbors(4)) <= 1
    assert np.array_equal(before[:4], oix.adj[:4])
