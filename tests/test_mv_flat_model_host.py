"""Exhaustive multi-vector k-NN without a GPU: the CPU model (tests/mv_flat_model.py) against a transcription of the
reference tool's loop, the literal queue against the closed form on tie-heavy lists, and the chunk assignment of
diskann_amd/csrc/maxsim_flat_plan.h compiled with g++.  The GPU side: tests/test_gpu_mv_flat.py."""
import os
import subprocess

import numpy as np
import pytest

import flat_model as fm
import mv_flat_model as mv
import oracle
from helpers import bits
from maxsim_model import REFERENCE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool_avg_of_mins(Q, D):
    """ground_truth.rs:764-776 under Metric::InnerProduct, line by line"""
    distance = np.float32(0.0)
    for q in Q:
        local_min = np.finfo(np.float32).max
        for b in D:
            local_min = min(local_min, np.float32(oracle.distance(oracle.F32, oracle.INNER_PRODUCT, q, b)))
        distance = np.float32(distance + local_min)
    return np.float32(distance / np.float32(len(Q)))


@pytest.mark.parametrize("nq,nd,dim", [(1, 1, 1), (2, 3, 4), (5, 1, 3), (3, 7, 8), (4, 4, 17)])
def test_model_avg_of_mins_is_the_tools_loop(nq, nd, dim):
    rng = np.random.default_rng(100 * nq + 10 * nd + dim)
    Q = rng.integers(-4, 5, (nq, dim)).astype(np.float32)
    D = rng.integers(-4, 5, (nd, dim)).astype(np.float32)
    got = mv.aggregate(mv.AVG_OF_MINS, mv.all_scores(oracle.F32, REFERENCE, Q, [D])[0], nd)
    assert bits(got) == bits(tool_avg_of_mins(Q, D))


def test_queue_equals_closed_form_on_ties():
    rng = np.random.default_rng(3)
    for trial in range(100):
        d = rng.integers(-2, 3, int(rng.integers(0, 40))).astype(np.float32)
        for k in (1, 3, 7, 50):
            pa, da_ = fm.flat_knn(d, k)
            pb, db = fm.flat_knn_closed(d, k)
            assert pa.tolist() == pb.tolist() and np.array_equal(bits(da_), bits(db)), (trial, k)


DRIVER = r"""
#include "maxsim_flat_plan.h"
#include <stdio.h>
#include <vector>
using namespace dann;

// one case per line: chunk_rows first n ndocs off[0 .. ndocs] -> nchunks, then per scanned document its chunk by
// mv_flat_chunk_of and how many chunks' mv_flat_chunk_docs ranges hold it
int main() {
    unsigned long long cr;
    unsigned first, n, ndocs;
    while (scanf("%llu %u %u %u", &cr, &first, &n, &ndocs) == 4) {
        std::vector<uint64_t> off(ndocs + 1);
        for (auto& o : off) { unsigned long long v; if (scanf("%llu", &v) != 1) return 1; o = v; }
        const MvFlatPlan p = mv_flat_plan(off[first + n] - off[first], n, 1, 10, 256, cr);
        printf("%u %llu", p.nchunks, (unsigned long long)p.chunk_rows);
        std::vector<unsigned> held(ndocs, 0), where(ndocs, 0);
        for (unsigned c = 0; c < p.nchunks; ++c) {
            uint32_t lo, hi;
            mv_flat_chunk_docs(off.data(), first, n, p.chunk_rows, p.nchunks, c, &lo, &hi);
            for (uint32_t d = lo; d < hi; ++d) held[d]++, where[d] = c;
        }
        for (unsigned d = first; d < first + n; ++d)
            printf(" %u:%u:%u", held[d], where[d], mv_flat_chunk_of(off[d] - off[first], p.chunk_rows, p.nchunks));
        printf("\n");
    }
    return 0;
}
"""

# (forced chunk rows, first, n, document lengths): documents without rows at the start, in the middle, on a chunk boundary
# and at the end; a range inside the set; the default sizing
CHUNK_CASES = [
    (32, 0, 8, [0, 0, 32, 0, 31, 1, 0, 0]),      # empties at the start, exactly on the boundary 32 | 64, and at the end
    (32, 0, 6, [10, 0, 0, 60, 0, 5]),             # a document that spans two chunks, an empty one behind it
    (64, 0, 5, [64, 64, 0, 64, 0]),               # rows a multiple of the chunk: the last empties' offset == the range's end
    (32, 2, 4, [7, 40, 0, 33, 0, 31, 9]),         # a range that starts and ends inside the set
    (32, 0, 3, [0, 0, 0]),                        # no rows at all: one chunk holds every document
    (0, 0, 40, [1, 2, 31, 32, 33, 64, 65, 0, 0, 1, 100] * 3 + [5, 0, 0, 900, 0, 17, 0]),  # default sizing
    (0, 0, len(mv.TILE_LENS), list(mv.TILE_LENS)),  # the GPU tests' set at the plan's own chunk size
]


@pytest.fixture(scope="module")
def chunkings(tmp_path_factory):
    d = tmp_path_factory.mktemp("mv_flat_plan")
    (d / "driver.cpp").write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diskann_amd", "csrc"),
                    str(d / "driver.cpp"), "-o", str(d / "driver")], check=True, capture_output=True, text=True)
    lines = ""
    for cr, first, n, lens in CHUNK_CASES:
        off = np.concatenate([[0], np.cumsum(lens)])
        lines += f"{cr} {first} {n} {len(lens)} " + " ".join(map(str, off)) + "\n"
    r = subprocess.run([str(d / "driver")], input=lines, capture_output=True, text=True, timeout=60, check=True)
    return [ln.split() for ln in r.stdout.splitlines()]


def test_every_document_belongs_to_exactly_one_chunk(chunkings):
    assert len(chunkings) == len(CHUNK_CASES)
    for (cr, first, n, lens), out in zip(CHUNK_CASES, chunkings):
        nchunks, chunk_rows = int(out[0]), int(out[1])
        docs = [tuple(int(x) for x in e.split(":")) for e in out[2:]]
        assert len(docs) == n and nchunks >= 1 and chunk_rows % 32 == 0 and (cr == 0 or chunk_rows == cr)
        off = np.concatenate([[0], np.cumsum(lens)])
        for i, (held, where, want) in enumerate(docs):
            d = first + i
            assert held == 1 and where == want, (lens, d)
            assert want == min((off[d] - off[first]) // chunk_rows, nchunks - 1), (lens, d)
        assert [w for _, w, _ in docs] == sorted(w for _, w, _ in docs)
    # the forced 32-row cases really put documents on both sides of a boundary
    assert int(chunkings[0][0]) == 2 and int(chunkings[2][0]) == 3 and int(chunkings[4][0]) == 1
    # the GPU tests' set: five chunks of mv.CHUNK rows, the two empty documents behind the filler in the last one
    tile = chunkings[-1]
    assert int(tile[0]) == 5 and int(tile[1]) == mv.CHUNK
    assert [e.split(":")[1] for e in tile[2:]][-5:] == ["3", "4", "4", "4", "4"]
