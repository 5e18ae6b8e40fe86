"""MinMax rows of 4, 2 and 1 bit searched with MM8 query images (MinMaxQuery::EightBit, dann_set_query_dtype): what can be
checked without a GPU.  The internal row types DT_MM1Q / MM2Q / MM4Q in the dispatcher (row_dispatch.h, compiled with
g++), the two declarations, the LDS slot, the CPU model's qbits = 8 against a float64 evaluation of the decompressed
vectors, and the staging permutation of the kernels (minmax_q8_model.stage) against the plain product."""
import os
import re
import subprocess

import numpy as np
import pytest

import minmax_model as m
import minmax_q8_model as q8
from minmax_builders import random_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "row_dispatch.h"
#include <stdio.h>
using namespace dann;
static const int kTypes[] = {DT_MM1Q, DT_MM2Q, DT_MM4Q};
template <RowSet ROWS>
static void visit_all(const char* set) {
    for (int dt : kTypes)
        for (int metric = 0; metric < 4; ++metric) {
            printf("visit %s %d %d ->", set, dt, metric);
            const int32_t rc = visit_row_op<ROWS>(dt, metric, [&](auto r) {
                using R = decltype(r);
                static_assert(row_op_defined(R::dt, R::op, R::norm), "an undefined triple was instantiated");
                printf(" %d %d %d\n", R::dt, R::op, (int)R::norm);
                return 7;
            });
            if (rc == kNoMetric) printf(" no metric\n");
            else if (rc == kNoRow) printf(" no row\n");
            else if (rc != 7) printf(" ?\n");
        }
}
int main() {
    visit_all<kRowsStored>("stored");
    visit_all<kRowsQuery>("query");
    visit_all<kRowsSearch>("search");
    visit_all<kRowsFloat>("float");
    visit_all<kRowsPair>("pair");
    for (int dt : kTypes) {
        printf("flags %d -> %d %d %d %d %d\n", dt, (int)dt_is_mm(dt), (int)dt_is_mmq(dt), (int)dt_mm_rows(dt), (int)dt_is_packed(dt),
               (int)query_stage_off(dt));
        for (int op = 0; op < 3; ++op) printf("dim128 %d %d -> %d\n", dt, op, (int)search_dim128_defined(dt, op));
    }
    const uint32_t dims[] = {1, 100, 128, 129};
    for (uint32_t dim : dims)
        printf("slot %u -> %u %u %u %u\n", dim, mm_query_lds_bytes(20 + dim), mm_slot_bytes(DT_MM4Q, 20 + dim),
               mm_slot_bytes(DT_MM2Q, 20 + dim), mm_slot_bytes(DT_MM1Q, 20 + dim));
    return 0;
}
"""

MM1Q, MM2Q, MM4Q = 113, 114, 116
OP_L2, OP_IP, OP_COS = 0, 1, 2
# what Cosine, InnerProduct, L2 and CosineNormalized select on DT_MM* rows (tests/test_row_dispatch_host.py TABLE)
MM_OPS = ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), (OP_IP, 1))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    d = tmp_path_factory.mktemp("minmax_q8")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diskann_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True)
    out = {}
    for ln in r.stdout.splitlines():
        key, val = ln.split(" -> ") if " -> " in ln else ln.split(" ->")
        kind, *rest = key.split()
        out.setdefault(kind, {})[tuple(rest)] = val.strip()
    return out


def test_internal_types_are_query_and_search_rows_only(output):
    for dt in (MM1Q, MM2Q, MM4Q):
        assert dt not in (6, 96, -1)
        for metric in range(4):
            for name in ("query", "search"):
                assert output["visit"][(name, str(dt), str(metric))] == "%d %d %d" % ((dt,) + MM_OPS[metric]), (name, dt, metric)
            for name in ("stored", "float", "pair"):
                assert output["visit"][(name, str(dt), str(metric))] == "no row", (name, dt, metric)
        # no stored type (dt_is_mm is what the entry points validate a caller's dtype with), MinMax rows to the kernels,
        # packed (a 4-lane group), staged at slot + 12, and no fixed-128 form
        assert output["flags"][(str(dt),)] == "0 1 1 1 12"
        assert all(output["dim128"][(str(dt), str(op))] == "0" for op in range(3))


def test_lds_slot(output):
    """the image's own slot, mm_query_lds_bytes(20 + dim); the 1-bit rows' eight plane dwords per 32 elements round the
    codes up to 32 bytes instead of 16"""
    for dim, codes16 in ((1, 16), (100, 112), (128, 128), (129, 144)):
        codes32 = (dim + 31) // 32 * 32
        assert output["slot"][(str(dim),)] == "%d %d %d %d" % (32 + codes16, 32 + codes16, 32 + codes16, 32 + codes32), dim


def test_the_new_calls_are_declared():
    hdr = open(os.path.join(ROOT, "include", "dann.h")).read()
    assert re.search(r"int32_t\s+dann_set_query_dtype\(dann_index\*\s*idx,\s*int32_t\s+dtype\);", hdr)
    assert re.search(r"int32_t\s+dann_get_query_dtype\(const dann_index\*\s*idx,\s*int32_t\*\s*out\);", hdr)
    assert re.search(r"#define\s+DANN_ABI_VERSION\s+5\b", hdr)
    rs = open(os.path.join(ROOT, "bindings", "rust", "dann_sys.rs")).read()
    assert re.search(r"pub fn dann_set_query_dtype\(idx: \*mut DannIndex, dtype: i32\) -> i32;", rs)
    assert re.search(r"pub fn dann_get_query_dtype\(idx: \*const DannIndex, out: \*mut i32\) -> i32;", rs)
    import diskann_amd as da
    assert "dann_set_query_dtype" in da._ffi.SYMBOLS and "dann_get_query_dtype" in da._ffi.SYMBOLS
    assert hasattr(da.Provider, "set_query_dtype") and hasattr(da.Provider, "query_dtype")


@pytest.mark.parametrize("bits", (4, 2, 1))
def test_model_with_8_bit_queries_is_the_product_of_the_decompressed_vectors(bits):
    """the reference's own test (minmax/vectors.rs:742-796) with its draw (a, b ~ U[0, 2]): the inner product of an 8-bit
    query and M-bit rows against -sum(decompress(q) * decompress(row)) in float64.  1e-5: the reference compares at 1e-6
    with an f32 sum; float64 against five separate f32 operations needs the wider margin."""
    rng = np.random.default_rng(40 + bits)
    for dim in (1, 7, 64, 100, 128, 129, 300):
        rows = random_rows(rng, 40, dim, bits, garbage=True)
        q = random_rows(rng, 9, dim, 8)
        got = m.distance_matrix(m.IP, q, rows, dim, bits, qbits=8)
        want = -(m.decompress(q, 8, dim) @ m.decompress(rows, bits, dim).T)
        assert np.allclose(got.astype(np.float64), want, rtol=1e-5, atol=0.0), (bits, dim)


@pytest.mark.parametrize("bits", (4, 2, 1))
def test_staged_form_gives_the_plain_product(bits):
    """minmax_q8_model restates the kernels' staging (mmq_stage_query) and their per-dword products (mmq_dot) in numpy:
    over random codes, with garbage in the rows' padding bits, the staged evaluation is the plain integer product, the
    staged bytes are a permutation of the query's (4 and 2 bit) that unstage() inverts, and what lies at or beyond dim
    is zero"""
    rng = np.random.default_rng(70 + bits)
    for dim in (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300):
        qc = rng.integers(1, 256, (5, dim), dtype=np.uint8)
        rows = random_rows(rng, 11, dim, bits, garbage=True)
        staged = q8.stage(qc, bits)
        assert staged.shape[1] == q8.staged_bytes(bits, dim) and staged.shape[1] % (32 if bits == 1 else 16) == 0
        assert np.array_equal(q8.unstage(staged, bits, dim), qc)
        if bits != 1:
            assert np.array_equal(np.sort(staged, axis=1)[:, -dim:], np.sort(qc, axis=1))
            assert not np.sort(staged, axis=1)[:, :-dim].any()
        want = qc.astype(np.int64) @ m.codes_of(rows, bits, dim).astype(np.int64).T
        got = q8.staged_product(staged, rows[:, m.HEADER:], bits, dim)
        assert np.array_equal(got, want), (bits, dim)
