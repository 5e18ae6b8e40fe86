"""diskann_amd/csrc/row_dispatch.h -- which (DT, OP, NORM) kernel instantiation a (dtype, metric) pair selects, for
which row types each kind of entry point has kernels, and where beam search has its 128-element form -- is a pure host
header: compiled here with g++ and tabulated over every row type of row_types.h and every metric.  The GPU side:
tests/test_gpu_search_matrix.py and the per-type files run every leaf against the oracle.

Where the table comes from.  The expected lines were not printed by row_dispatch.h.  They are read off the ladders of
commit 34fcc3b, the parent of the commit that introduced the header, where every kernel family had a copy of its own:
TABLE is prune_common.h's dispatch<Launcher> (resolve_metric, then the DANN_CASE macro) for the 14 stored row types and
DT_SPH1T, and search_kernel_impl.h's launch_dt for DT_PQ; ROWS is the list of `case` labels of each family's switch;
DIM128 is launch_dt's placement of its <..., 128> instantiations."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "row_dispatch.h"
#include <stdio.h>
using namespace dann;
static const int kTypes[] = {DT_F32, DT_F16, DT_U8, DT_I8, DT_SQ8, DT_PQ, DT_SQ1, DT_SQ4, DT_SPH1, DT_SPH2, DT_SPH4,
                             DT_SPH1T, DT_MM1, DT_MM2, DT_MM4, DT_MM8, 6, 96, -1};
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
    for (int dt : kTypes)
        for (int metric = 0; metric < 4; ++metric) {
            int op = -1;
            bool norm = false;
            const bool ok = resolve_metric(dt, metric, &op, &norm);
            printf("resolve %d %d -> %d %d %d %d\n", dt, metric, (int)ok, op, (int)norm, (int)row_op_defined(dt, op, norm));
        }
    for (int dt : kTypes)
        for (int op = 0; op < 3; ++op) {
            for (int norm = 0; norm < 2; ++norm) printf("defined %d %d %d -> %d\n", dt, op, norm, (int)row_op_defined(dt, op, norm != 0));
            printf("dim128 %d %d -> %d\n", dt, op, (int)search_dim128_defined(dt, op));
        }
    return 0;
}
"""

F32, F16, U8, I8, SQ8, PQ, SQ1, SQ4, SPH1, SPH2, SPH4, SPH1T, MM1, MM2, MM4, MM8 = (
    0, 1, 2, 3, 4, 5, 17, 20, 33, 34, 36, 97, 49, 50, 52, 56)
COSINE, IP, L2, COSN = 0, 1, 2, 3
OP_L2, OP_IP, OP_COS = 0, 1, 2
NO = None  # "metric %d is not defined for dtype %d"

# row type -> what Cosine, InnerProduct, L2 and CosineNormalized select: (OP, NORM)
TABLE = {
    F32:   ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), (OP_IP, 1)),
    F16:   ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), (OP_IP, 1)),
    U8:    ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), (OP_COS, 0)),
    I8:    ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), (OP_COS, 0)),
    SQ8:   (NO,          (OP_IP, 0), (OP_L2, 0), (OP_L2, 1)),
    SQ4:   (NO,          (OP_IP, 0), (OP_L2, 0), (OP_L2, 1)),
    SQ1:   (NO,          (OP_IP, 0), (OP_L2, 0), (OP_L2, 1)),
    SPH1:  ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), NO),
    SPH2:  ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), NO),
    SPH4:  ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), NO),
    SPH1T: ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), NO),
    MM1:   ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), (OP_IP, 1)),
    MM2:   ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), (OP_IP, 1)),
    MM4:   ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), (OP_IP, 1)),
    MM8:   ((OP_COS, 0), (OP_IP, 0), (OP_L2, 0), (OP_IP, 1)),
    PQ:    (NO,          (OP_IP, 0), (OP_L2, 0), NO),
}
STORED = (F32, F16, U8, I8, SQ8, SQ4, SQ1, SPH1, SPH2, SPH4, MM1, MM2, MM4, MM8)
# the row types of each kind of entry point: prune / consolidate / in-place delete / distance pairs take no query and
# so never meet the query layout DT_SPH1T; PQ rows are served by beam search alone
ROWS = {
    "stored": STORED,
    "query": STORED + (SPH1T,),
    "search": STORED + (SPH1T, PQ),
    "float": (F32, F16),
    "pair": (U8, I8, SQ8),
}
NOT_ROW_TYPES = (6, 96, -1)
# beam search's <..., DIM = 128> instantiations, per OP: the row types launch_dt tests `dim == 128` for
DIM128 = {
    OP_L2: (F32, F16, U8, I8, SQ8, SQ4, SQ1, SPH1, SPH2, SPH4, SPH1T, MM1, MM2, MM4, MM8),
    OP_IP: (U8, I8, SQ8, SQ4, SQ1, SPH1, SPH2, SPH4, SPH1T, MM1, MM2, MM4, MM8),
    OP_COS: (U8, I8, SPH1, SPH2, SPH4, SPH1T, MM1, MM2, MM4, MM8),
}


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    d = tmp_path_factory.mktemp("row_dispatch")
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


def test_visitor_matches_the_parent_ladders(output):
    expected = {}
    for name, rows in ROWS.items():
        for dt in tuple(TABLE) + NOT_ROW_TYPES:
            for metric in (COSINE, IP, L2, COSN):
                if dt not in rows:
                    want = "no row"
                elif TABLE[dt][metric] is NO:
                    want = "no metric"
                else:
                    want = "%d %d %d" % ((dt,) + TABLE[dt][metric])
                expected[(name, str(dt), str(metric))] = want
    assert output["visit"] == expected


def test_resolve_metric_answers_only_defined_triples(output):
    produced = set()
    for (dt, metric), val in output["resolve"].items():
        ok, op, norm, defined = (int(x) for x in val.split())
        if int(dt) in TABLE:
            want = TABLE[int(dt)][int(metric)]
            assert (ok, (op, norm) if ok else NO) == (int(want is not NO), want), (dt, metric)
        if ok and int(dt) in TABLE:
            assert defined, (dt, metric)
            produced.add((int(dt), op, norm))
    # ... and every defined triple is some metric's answer: a kernel no (dtype, metric) reaches is not defined
    defined = {tuple(int(x) for x in k) for k, v in output["defined"].items() if v == "1" and int(k[0]) in TABLE}
    assert defined == produced
    assert produced == {(dt, *t) for dt, row in TABLE.items() for t in row if t is not NO}


def test_dim128_predicate(output):
    # over every (DT, OP) that has a kernel at all (scalar-quantised rows have no Cosine, PQ rows neither)
    for dt, row in TABLE.items():
        for op in {t[0] for t in row if t is not NO}:
            assert (output["dim128"][(str(dt), str(op))] == "1") == (dt in DIM128[op]), (dt, op)
