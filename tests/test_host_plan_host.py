"""diskann_amd/csrc/host_plan.h -- how dann_search_batch moves a call's host buffers (small call, single pass through the
pinned ring or from pageable memory, zero copy, chunked lanes) -- is a pure host function: compiled here with g++ and
tabulated at the boundaries of every threshold it has.  The GPU side of each strategy: tests/test_gpu_server.py (small
calls, zero copy on page-locked and temporarily registered buffers) and the parity suites through Provider.search
(single pass, lanes)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "host_plan.h"
#include <stdio.h>
using namespace dann;

// one case per line: dtype pipeline host_chunk nq k qb q_pinned ids_pinned dists_pinned stats_pinned
int main() {
    int dt;
    unsigned pipe, chunk, nq, k, q, i, d, s;
    unsigned long long qb;
    while (scanf("%d %u %u %u %u %llu %u %u %u %u", &dt, &pipe, &chunk, &nq, &k, &qb, &q, &i, &d, &s) == 10) {
        const HostPlanIn in{dt, pipe, chunk, nq, k, (size_t)qb, q != 0, i != 0, d != 0, s != 0};
        const HostPlan p = plan_host_search(in);
        static const char* names[] = {"Small", "Single", "ZeroCopy", "Lanes"};
        printf("%s %d %d %d %d %u %u %zu %zu %zu %d\n", names[(int)p.strategy], p.ring, p.may_register, p.q_direct,
               p.o_direct, p.cq, p.lanes, p.in_b, p.ids_b, p.out_b, (int)host_chunked(pipe, chunk, nq));
    }
    return 0;
}
"""

F32, F16, U8, I8, SQ8, PQ = range(6)
ALL, NONE = (1, 1, 1, 1), (0, 0, 0, 0)

# (dtype, pipeline, host_chunk, nq, k, qb, (q, ids, dists, stats) pinned) -> (strategy, ring, may_register, q_direct,
# o_direct, cq, lanes): what dann_search_batch did before the strategies were split out of it
CASES = [
    # small calls: at most kSmallCall = 16 queries and a quarter of the 1 MB staging block, default pipeline only
    ((F32, 1, 16384, 1, 10, 512, NONE), ("Small", 1, 0, 0, 0, 1, 0)),
    ((F32, 1, 16384, 16, 10, 512, NONE), ("Small", 1, 0, 0, 0, 16, 0)),
    ((F32, 1, 16384, 17, 10, 512, NONE), ("Single", 1, 0, 0, 0, 17, 0)),
    ((F32, 1, 16384, 16, 10, 16284, NONE), ("Small", 1, 0, 0, 0, 16, 0)),   # 262 144 staging bytes: exactly a quarter
    ((F32, 1, 16384, 16, 10, 16285, NONE), ("Single", 1, 0, 0, 0, 16, 0)),  # 16 more
    ((F32, 0, 16384, 8, 10, 512, NONE), ("Single", 1, 0, 0, 0, 8, 0)),
    ((F32, 2, 16384, 8, 10, 512, NONE), ("Single", 1, 0, 0, 0, 8, 0)),
    ((F32, 8, 16384, 8, 10, 512, NONE), ("Single", 1, 0, 0, 0, 8, 0)),
    ((F32, 9, 16384, 8, 10, 512, NONE), ("Single", 1, 0, 0, 0, 8, 0)),
    ((SQ8, 1, 16384, 16, 10, 132, NONE), ("Small", 1, 0, 0, 0, 16, 0)),
    ((PQ, 1, 16384, 4, 10, 512, NONE), ("Small", 1, 0, 0, 0, 4, 0)),
    # single pass: through the ring while queries + ids + distances + statistics fit 1 MB
    ((F32, 1, 16384, 1713, 10, 512, NONE), ("Single", 1, 0, 0, 0, 1713, 0)),  # 1 048 384 bytes
    ((F32, 1, 16384, 1714, 10, 512, NONE), ("Single", 0, 0, 0, 0, 1714, 0)),  # 1 048 976
    ((F32, 1, 16384, 2545, 1, 384, NONE), ("Single", 1, 0, 0, 0, 2545, 0)),   # exactly 1 048 576
    ((F32, 1, 16384, 2545, 1, 385, NONE), ("Single", 0, 0, 0, 0, 2545, 0)),   # 2 545 more
    ((U8, 1, 16384, 4598, 10, 128, NONE), ("Single", 1, 0, 0, 0, 4598, 0)),   # 1 048 352
    ((U8, 1, 16384, 4599, 10, 128, NONE), ("Single", 0, 0, 0, 0, 4599, 0)),   # 1 048 592
    ((F32, 1, 16384, 1714, 10, 512, ALL), ("Single", 0, 0, 0, 0, 1714, 0)),   # (pinning plays no part unchunked)
    # chunked from two chunks on, unless the pipeline is off
    ((F32, 1, 16384, 32767, 10, 512, NONE), ("Single", 0, 0, 0, 0, 32767, 0)),
    ((F32, 1, 16384, 32768, 10, 512, NONE), ("Lanes", 0, 1, 0, 0, 16384, 2)),
    ((F32, 1, 16384, 32768, 10, 512, ALL), ("ZeroCopy", 0, 0, 1, 1, 16384, 2)),
    ((F32, 0, 16384, 100000, 10, 512, ALL), ("Single", 0, 0, 0, 0, 100000, 0)),
    ((F32, 1, 16384, 100000, 10, 512, NONE), ("Lanes", 0, 1, 0, 0, 16384, 3)),
    # the chunk knob is raised to 256
    ((F32, 1, 100, 511, 10, 512, NONE), ("Single", 1, 0, 0, 0, 511, 0)),
    ((F32, 1, 100, 512, 10, 512, NONE), ("Lanes", 0, 1, 0, 0, 256, 2)),
    ((F32, 1, 0, 512, 10, 512, NONE), ("Lanes", 0, 1, 0, 0, 256, 2)),
    ((F32, 1, 255, 700, 10, 512, NONE), ("Lanes", 0, 1, 0, 0, 256, 3)),
    ((F32, 1, 300, 599, 10, 512, NONE), ("Single", 1, 0, 0, 0, 599, 0)),
    ((F32, 1, 300, 600, 10, 512, NONE), ("Lanes", 0, 1, 0, 0, 300, 2)),
    # lanes: three by default, 2 .. 8 as asked, never more than 8 nor more than there are chunks (5000 / 256: 20 chunks)
    ((F32, 1, 256, 5000, 10, 512, NONE), ("Lanes", 0, 1, 0, 0, 256, 3)),
    ((F32, 2, 256, 5000, 10, 512, NONE), ("Lanes", 0, 0, 0, 0, 256, 2)),
    ((F32, 8, 256, 5000, 10, 512, NONE), ("Lanes", 0, 0, 0, 0, 256, 8)),
    ((F32, 9, 256, 5000, 10, 512, NONE), ("Lanes", 0, 0, 0, 0, 256, 8)),
    ((F32, 8, 16384, 100000, 10, 512, NONE), ("Lanes", 0, 0, 0, 0, 16384, 7)),
    ((F32, 9, 16384, 100000, 10, 512, NONE), ("Lanes", 0, 0, 0, 0, 16384, 7)),
    # an explicit lane count never zero-copies on buffers the caller did not pin ... but does on pinned ones
    ((F32, 2, 16384, 100000, 10, 512, ALL), ("ZeroCopy", 0, 0, 1, 1, 16384, 2)),
    ((F32, 9, 16384, 100000, 10, 512, ALL), ("ZeroCopy", 0, 0, 1, 1, 16384, 7)),
    # zero copy: every buffer pinned (no statistics buffer counts as pinned), rows read once by their kernel
    ((F16, 1, 16384, 40000, 10, 256, ALL), ("ZeroCopy", 0, 0, 1, 1, 16384, 3)),
    ((U8, 1, 16384, 40000, 10, 128, ALL), ("ZeroCopy", 0, 0, 1, 1, 16384, 3)),
    ((I8, 1, 16384, 40000, 10, 128, ALL), ("ZeroCopy", 0, 0, 1, 1, 16384, 3)),
    ((SQ8, 1, 16384, 40000, 10, 132, ALL), ("Lanes", 0, 0, 1, 1, 16384, 3)),
    ((PQ, 1, 16384, 40000, 10, 512, ALL), ("Lanes", 0, 0, 1, 1, 16384, 3)),
    ((SQ8, 1, 16384, 40000, 10, 132, NONE), ("Lanes", 0, 0, 0, 0, 16384, 3)),
    ((PQ, 1, 16384, 40000, 10, 512, NONE), ("Lanes", 0, 0, 0, 0, 16384, 3)),
    # partly pinned: the lanes copy the pinned buffers directly; temporary page-locking may still make it zero copy
    ((F32, 1, 16384, 40000, 10, 512, (1, 0, 0, 1)), ("Lanes", 0, 1, 1, 0, 16384, 3)),
    ((F32, 1, 16384, 40000, 10, 512, (0, 1, 1, 1)), ("Lanes", 0, 1, 0, 1, 16384, 3)),
    ((F32, 1, 16384, 40000, 10, 512, (1, 1, 0, 1)), ("Lanes", 0, 1, 1, 0, 16384, 3)),
    ((F32, 1, 16384, 40000, 10, 512, (1, 1, 1, 0)), ("Lanes", 0, 1, 1, 1, 16384, 3)),
    ((U8, 2, 16384, 40000, 10, 128, (1, 1, 1, 0)), ("Lanes", 0, 0, 1, 1, 16384, 2)),
]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diskann_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)

    def plan(cases):
        lines = "".join(" ".join(map(str, (*c[:6], *c[6]))) + "\n" for c in cases)
        r = subprocess.run([str(exe)], input=lines, capture_output=True, text=True, timeout=60, check=True)
        return [ln.split() for ln in r.stdout.splitlines()]
    return plan


def test_plan_matches_the_table(planner):
    got = planner([c for c, _ in CASES])
    assert len(got) == len(CASES)
    for (case, want), g in zip(CASES, got):
        assert (g[0], *map(int, g[1:7])) == want, (case, g)


def test_staging_sizes_and_the_chunked_test(planner):
    """one pass's staging: queries unpadded, ids | distances | statistics (20 bytes a query) each padded to 16 bytes; host_chunked() is the
    caller's cue to ask about pinning -- exactly the calls that are chunked"""
    got = planner([c for c, _ in CASES])
    for (case, want), g in zip(CASES, got):
        dt, pipe, chunk, nq, k, qb, _ = case
        cq = want[5]
        ids_b = (cq * k * 4 + 15) & ~15
        assert tuple(map(int, g[7:10])) == (cq * qb, ids_b, 2 * ids_b + ((cq * 20 + 15) & ~15)), (case, g)
        assert int(g[10]) == (want[0] in ("Lanes", "ZeroCopy")), (case, g)
