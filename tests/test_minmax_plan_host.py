"""MinMax rows (DT_MM1 / MM2 / MM4 / MM8) in the host-side launch planning: compiled with g++ from row_types.h,
launch_shape.h and launch_plan.h, as tests/test_launch_plan_host.py does.  They plan to the one-wave and persistent
families, never to teams, pairs or the PQ table kernel, at every shape that gives other row types one of those; the
staged query's LDS slot is sized for the image at slot + 12 (codes 16-byte aligned); resolve_metric answers the form of
the epilogue for all four metrics.  Fails to compile before the row types exist."""
import os
import subprocess

import pytest

import minmax_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include "launch_plan.h"
#include <stdio.h>
using namespace dann;
static uint32_t g_words[32];
int main() {
    static_assert(DT_MM1 == 49 && DT_MM2 == 50 && DT_MM4 == 52 && DT_MM8 == 56, "dtype value = 48 + bits");
    static_assert(dt_is_mm(DT_MM1) && dt_is_mm(DT_MM2) && dt_is_mm(DT_MM4) && dt_is_mm(DT_MM8), "dt_is_mm");
    static_assert(!dt_is_mm(DT_SQ8) && !dt_is_mm(DT_SPH4) && !dt_is_mm(DT_U8) && !dt_is_mm(48) && !dt_is_mm(51), "dt_is_mm");
    static_assert(dt_is_packed(DT_MM1) && dt_is_packed(DT_MM2) && dt_is_packed(DT_MM4) && !dt_is_packed(DT_MM8), "lane groups");
    static_assert(query_stage_off(DT_MM8) == 12 && query_stage_off(DT_SQ8) == 0 && query_stage_off(DT_F32) == 0, "staging");
    long long v[10];
    // dtype metric dim degree nq L maxc image_bytes
    while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7]) == 8) {
        SearchArgs a;
        a.ix.dtype = (int32_t)v[0]; a.ix.metric = (int32_t)v[1]; a.ix.dim = (uint32_t)v[2]; a.ix.max_degree = (uint32_t)v[3];
        a.ix.adj_stride = a.ix.max_degree + 1; a.ix.nstart = 1; a.ix.nslots = 5001; a.ix.capacity = 5000;
        a.ix.layer_bytes = a.ix.qbytes = (uint32_t)v[7]; a.ix.row_stride = (a.ix.layer_bytes + 15u) & ~15u;
        a.ix.pq_chunks = 0; a.ix.tag_off = 0;
        a.ix.rows = nullptr; a.ix.adj = nullptr; a.ix.pq_pivots = nullptr; a.ix.pq_offsets = nullptr; a.ix.pq_pack = nullptr;
        a.ix.pq_pack_stride = a.ix.pq_pack_codes = 0; a.ix.sq_k = a.ix.sq_shift_norm_sq = 0.f;
        a.nq = (uint32_t)v[4]; a.l_value = (uint32_t)v[5]; a.beam_width = 1; a.qcap_max = 0; a.filter_mode = 0;
        a.queries = g_words; a.out_ids = g_words; a.ht_entries = 0; a.srv.ring = 0; a.stats = nullptr; a.k = 10;
        a.spill_next = g_words;
        const LaunchKnobs k{256u, (uint32_t)v[6], 0u, 0u, 0u, 1024u, 64u, 64u, 6u};
        const uint32_t inflight = launch_capped(a, k) ? k.max_concurrency : a.nq;
        plan_family(a, k, inflight);
        VisitedCalib cal;
        cal.cap_ids = 0;
        cal.waves = 16;
        uint32_t sized = 0;
        PlanMsg msg;
        if (plan_table(a, k, cal, inflight, &sized, msg) != DANN_OK) return 2;
        cap_grid(a, k);
        if (a.grid) a.team = 0;
        int op = -1;
        bool norm = false;
        const bool ok = resolve_metric(a.ix.dtype, a.ix.metric, &op, &norm);
        printf("%d t%u p%u q%u shapes %d %d %d qlds %u metric %d %d %d\n", search_family(a), a.team, a.pair, a.pqlut,
               (int)team_shape(a), (int)pair_shape(a), (int)pq_lut_shape(a), query_lds_bytes(a.ix), (int)ok, op, (int)norm);
    }
    return 0;
}
"""

OP_L2, OP_IP, OP_COS = 0, 1, 2
FORM = {m.L2: (OP_L2, 0), m.IP: (OP_IP, 0), m.COSINE: (OP_COS, 0), m.COSINE_NORMALIZED: (OP_IP, 1)}
U8, SQ8 = 2, 4


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("minmax_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diskann_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)

    def plan(lines):
        r = subprocess.run([str(exe)], input="".join(" ".join(str(x) for x in ln) + "\n" for ln in lines),
                           capture_output=True, text=True, timeout=60, check=True)
        return [ln.split() for ln in r.stdout.splitlines()]
    return plan


def _parse(f):
    return dict(family=int(f[0]), team=f[1], pair=f[2], pqlut=f[3], shapes=tuple(int(x) for x in f[5:8]), qlds=int(f[9]),
                metric=tuple(int(x) for x in f[11:14]))


def test_minmax_rows_plan_to_one_wave_and_persistent(planner):
    """48 queries at 128-d, degree 32 is the team's shape and 8 192 queries the pair's for U8 / SQ-8 rows (the control
    lines); MinMax rows of every width and metric take one wave per query there, persistent waves under a cap"""
    ONE_WAVE, TEAM, PAIR, PERSISTENT = 0, 1, 2, 3
    lines, want = [], []
    for bits in m.BITS:
        for metric in m.METRICS:
            for dim in (128, 100):
                lb = m.layer_bytes(bits, dim)
                for nq, maxc, fam in ((48, 0, ONE_WAVE), (8192, 0, ONE_WAVE), (8192, 1024, PERSISTENT)):
                    lines.append((48 + bits, metric, dim, 32, nq, 26, maxc, lb))
                    want.append((fam, bits, metric, dim))
    lines += [(U8, m.L2, 128, 32, 48, 26, 0, 128), (U8, m.L2, 128, 32, 8192, 26, 0, 128), (SQ8, m.L2, 128, 32, 48, 26, 0, 132)]
    got = [_parse(f) for f in planner(lines)]
    assert len(got) == len(lines)
    for g, (fam, bits, metric, dim) in zip(got, want):
        tag = (bits, metric, dim)
        assert g["family"] == fam and (g["team"], g["pair"], g["pqlut"]) == ("t0", "p0", "q0"), (tag, g)
        assert g["shapes"] == (0, 0, 0), (tag, g)
        assert g["metric"] == (1,) + FORM[metric], (tag, g)
    assert [g["family"] for g in got[-3:]] == [TEAM, PAIR, TEAM], got[-3:]


def test_query_slot_bytes(planner):
    """the slot holds 12 bytes of lead, the 20-byte header and the code bytes rounded up to the 16-byte step: the codes
    start at byte 32 of the slot"""
    lines, want = [], []
    for bits in m.BITS:
        for dim in (1, 7, 8, 9, 31, 32, 33, 100, 127, 128, 129, 260, 300):
            lb = m.layer_bytes(bits, dim)
            lines.append((48 + bits, m.L2, dim, 32, 48, 26, 0, lb))
            want.append(32 + (m.code_bytes(bits, dim) + 15) // 16 * 16)
    got = [_parse(f)["qlds"] for f in planner(lines)]
    assert got == want
    assert m.layer_bytes(8, 128) == 148 and m.layer_bytes(4, 128) == 84 and m.layer_bytes(1, 128) == 36
