"""diskann_amd/csrc/query_schedule.h -- the slot map of a locality-scheduled search launch -- is a pure function shared by
the scatter kernel and this test, compiled here with g++: for every size, both directions are bijections on [0, n), one
inverts the other, and the slots of one residue class mod `parts` (one XCD under the observed dealing) run one
contiguous run of the sorted order, in order.  The GPU side: tests/test_gpu_query_schedule.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "query_schedule.h"
#include <stdio.h>
#include <vector>
using namespace dann;

// one case per line: n parts -> "ok" or the first violation
int main() {
    unsigned n, parts;
    while (scanf("%u %u", &n, &parts) == 2) {
        std::vector<unsigned char> seen(n, 0);
        const char* bad = nullptr;
        unsigned at = 0;
        for (unsigned s = 0; s < n && !bad; ++s) {
            const unsigned p = sched_source(s, n, parts);
            if (p >= n) bad = "out of range";
            else if (seen[p]++) bad = "not a bijection";
            else if (sched_slot(p, n, parts) != s) bad = "not inverse";
            // slot s + parts follows s in its class: the next sorted position
            else if (s + parts < n && sched_source(s + parts, n, parts) != p + 1) bad = "class not contiguous";
            at = s;
        }
        // the classes in order of their residue cover the sorted order chunk after chunk
        unsigned expect = 0;
        for (unsigned x = 0; x < parts && x < n && !bad; ++x) {
            if (sched_source(x, n, parts) != expect) bad = "chunks out of order", at = x;
            expect += n / parts + (x < n % parts ? 1u : 0u);
        }
        if (bad) printf("%u %u %s at %u\n", n, parts, bad, at);
        else printf("%u %u ok\n", n, parts);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("sched")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "diskann_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(driver, cases):
    inp = "".join(f"{n} {p}\n" for n, p in cases)
    out = subprocess.run([driver], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    return [l for l in out if l]


def test_every_size_up_to_a_few_hundred(driver):
    cases = [(n, p) for n in range(1, 400) for p in (1, 2, 3, 8)]
    out = _run(driver, cases)
    assert len(out) == len(cases)
    assert all(l.endswith(" ok") for l in out), [l for l in out if not l.endswith(" ok")][:5]


def test_ragged_ends_up_to_1e5(driver):
    cases = [(n + d, 8) for n in (1024, 16384, 16384 * 3, 99992, 100000 - 8) for d in range(-9, 10)] + [(100000, 8),
                                                                                                      (100000, 1)]
    out = _run(driver, cases)
    assert all(l.endswith(" ok") for l in out), [l for l in out if not l.endswith(" ok")][:5]


def test_eight_runs_of_the_headline_batch():
    """100 000 queries, 8 XCDs: slot s runs entry s / 8 of chunk s % 8, the chunks 12 500 entries long"""
    n, parts = 100000, 8
    q, r = divmod(n, parts)
    src = lambda s: (s % parts) * q + min(s % parts, r) + s // parts  # noqa: E731
    assert [src(s) for s in range(10)] == [0, 12500, 25000, 37500, 50000, 62500, 75000, 87500, 1, 12501]
    assert src(n - 1) == n - 1
