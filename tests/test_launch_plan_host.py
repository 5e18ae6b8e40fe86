"""diskann_amd/csrc/launch_plan.h -- which kernel family a beam-search launch runs, the size, entry width and probing
geometry of its LDS visited table, its tuning bits and what a re-run of overflowed queries changes -- is a pure host
function: compiled here with g++ and tabulated at both sides of every threshold it has.  The GPU side: the family
assertions of tests/test_gpu_pair.py, test_gpu_pqlut.py, test_gpu_visited16.py and the team and server tests.

Where the table comes from.  The expected lines were not produced by launch_plan.h: they are the output of a throwaway
harness built from the text of commit 8df4489 (the parent of the commit that introduced launch_plan.h), where all of
this was part of prepare_launch and search_with_retry in search_kernels.hip.  The harness took, with `git show`, that
commit's IndexView / ServerView / SearchArgs / VisitedCalib, the DT_* / M_* / OP_* vocabulary and resolve_metric, the
launch-shape helpers of the three kernel headers and search_kernels.hip's lines 54-196, 209-217 and 278-473 (with
__host__ / __device__ defined away, hipMalloc / hipMemsetAsync / the register query stubbed out, the calibration map
pre-filled with the case's cap_ids and waves, and fprintf captured for the verbose line's numbers), followed by
search_with_retry's lines 508-519 (the cap on persistent waves; a case's explicit `inflight` replaces the argument
they pass to prepare_launch) and 637-650 (the retry step) around them, read this
file's DRIVER_COMMON and case list, and printed one line per case.  The rows under "# device" at the end of the table
are the configurations of scratch/launch_plan_compare.py with the `waves` the parent derived from the kernels' VGPRs on
an MI355X and the p90 it calibrated; the slot counts and LDS bytes of the parent's verbose lines there
(profiles/launch_plan_parent.txt) are the `sized` fields of those rows."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# shared by the driver below and by the harness the table was produced with: one case per line
#   G words nslots kcap                                  -> ht16_geometry, overflow words (pair, PQ table)
#   P <34 numbers, FIELDS below>                         -> the plan of the first launch
#   R <the same>                                         -> ... and of every re-run of `nfailed` queries until "stop"
DRIVER_COMMON = r"""
static uint32_t g_words[32];  // stands in for every device buffer: only (non-)nullness and work_next's offset matter
static void fill_args(const long long* v, SearchArgs& a) {
    a.ix.dtype = (int32_t)v[0]; a.ix.metric = (int32_t)v[1]; a.ix.dim = (uint32_t)v[2]; a.ix.max_degree = (uint32_t)v[3];
    a.ix.adj_stride = a.ix.max_degree + 1; a.ix.nstart = (uint32_t)v[4]; a.ix.nslots = (uint32_t)v[5];
    a.ix.capacity = a.ix.nslots - a.ix.nstart; a.ix.row_stride = (uint64_t)v[6]; a.ix.pq_chunks = (uint32_t)v[7];
    a.ix.tag_off = (uint32_t)v[8]; a.ix.layer_bytes = a.ix.qbytes = (uint32_t)v[6];
    a.ix.rows = nullptr; a.ix.adj = nullptr; a.ix.pq_pivots = nullptr; a.ix.pq_offsets = nullptr; a.ix.pq_pack = nullptr;
    a.ix.pq_pack_stride = a.ix.pq_pack_codes = 0; a.ix.sq_k = a.ix.sq_shift_norm_sq = 0.f;
    a.nq = (uint32_t)v[9]; a.l_value = (uint32_t)v[10]; a.beam_width = (uint32_t)v[11]; a.qcap_max = (uint32_t)v[12];
    a.filter_mode = (uint32_t)v[13];
    if (v[14]) a.range_ids = g_words;
    if (v[15]) a.rec_ids = g_words;
    if (v[16]) a.qslots = g_words; else a.queries = g_words;
    if (v[17]) a.qmap = g_words;
    if (v[18]) a.out_ids = g_words;
    a.ht_entries = (uint32_t)v[19];
    a.srv.ring = (uint32_t)v[20]; a.srv.workers = a.nq;
    a.stats = nullptr; a.k = 10;
}
static void print_plan(const SearchArgs& a, unsigned sized_slots, size_t sized_lds) {
    printf("%d t%u p%u q%u g%u | %s %u+%u prime %u shift %u tb %u kmax %u open %u | tune %u lds %zu | sized %u %zu",
           search_family(a), a.team, a.pair, a.pqlut, a.grid, a.ht16 ? "ht16" : "ht32", a.ht_entries, a.ht_ov, a.ht_prime,
           a.ht_shift, a.ht_tb, a.ht_kmax, a.ht_open, a.tune, search_lds_bytes(a), sized_slots, sized_lds);
}
static void print_step(const SearchArgs& a) {
    printf(" / %d t%u p%u q%u g%u %s %u+%u nq %u lds %zu", search_family(a), a.team, a.pair, a.pqlut, a.grid,
           a.ht16 ? "ht16" : "ht32", a.ht_entries, a.ht_ov, a.nq, search_lds_bytes(a));
}
"""

DRIVER = r"""
#include "launch_plan.h"
#include <stdio.h>
using namespace dann;
""" + DRIVER_COMMON + r"""
int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'G') {
            unsigned w, n, kc;
            if (scanf("%u %u %u", &w, &n, &kc) != 3) return 1;
            const Ht16Geom g = ht16_geometry(w, n, kc);
            printf("%d shift %u tb %u kmax %u slots %u ov %u %u\n", (int)g.ok, g.shift, g.tb, g.kmax, g.slots,
                   ht16_overflow_words(g, true), ht16_overflow_words(g, false));
            continue;
        }
        long long v[34];
        for (int i = 0; i < 34; ++i)
            if (scanf("%lld", &v[i]) != 1) return 1;
        SearchArgs a;
        fill_args(v, a);
        const uint32_t cus = (uint32_t)v[21];
        const LaunchKnobs k{cus, (uint32_t)v[22], (uint32_t)v[23], (uint32_t)v[24], (uint32_t)v[25],
                            v[26] < 0 ? 4u * cus : (uint32_t)v[26], v[27] < 0 ? 20u * cus : (uint32_t)v[27], (uint32_t)v[28],
                            (uint32_t)v[29]};
        // the order of search_with_retry (search_kernels.hip): family, the calibration's waves (the PQ table kernel's are
        // fixed by its registers), table, the cap on persistent waves, the probing geometry
        a.spill_next = g_words;
        const uint32_t inflight = v[33] >= 0 ? (uint32_t)v[33] : launch_capped(a, k) ? k.max_concurrency : a.nq;
        plan_family(a, k, inflight);
        VisitedCalib cal;
        cal.cap_ids = (uint32_t)v[30];
        cal.waves = a.pqlut ? pq_lut_waves_per_cu(a.ix.pq_chunks) : (uint32_t)v[31];
        const bool autosize = a.ht_entries == 0;
        uint32_t sized = 0;
        PlanMsg msg;
        int32_t rc = plan_table(a, k, cal, inflight, &sized, msg);
        SearchArgs t = a;
        t.ht_entries = sized;
        const unsigned sized_slots = autosize ? (a.ht16 ? sized * 2u : sized) : 0u;
        const size_t sized_lds = autosize ? search_lds_bytes(t) : 0;
        if (rc == DANN_OK) {
            cap_grid(a, k);
            if (a.grid) a.team = 0;
            rc = finish_visited_table(a, k.open_eighths, k.ht16_kcap, msg);
        }
        if (rc != DANN_OK) {
            printf("error %d: %s\n", rc, msg);
            continue;
        }
        print_plan(a, sized_slots, sized_lds);
        while (kind == 'R' && plan_retry(a, k, g_words, (uint32_t)v[32])) {
            if (finish_visited_table(a, k.open_eighths, k.ht16_kcap, msg) != DANN_OK) return 2;
            print_step(a);
        }
        printf(kind == 'R' ? " / stop\n" : "\n");
    }
    return 0;
}
"""

F32, F16, U8, I8, SQ8, PQ, SQ4 = 0, 1, 2, 3, 4, 5, 20
COSINE, IP, L2, COSN = 0, 1, 2, 3
FIELDS = ("dt", "metric", "dim", "degree", "nstart", "nslots", "stride", "chunks", "tag_off",
          "nq", "L", "W", "qcap_max", "filter", "range", "rec", "qslots", "qmap", "out_ids", "entries", "srv",
          "cus", "maxc", "vfmt", "toff", "ton", "team_max", "pair_min", "kcap", "eighths",
          "cap_ids", "waves", "nfailed", "inflight")
# an f32 L2 index of 5 000 x 128 rows, degree 32, one start point, on a 256-CU device; knobs at their defaults
# (team_max / pair_min -1: 4 x / 20 x CUs); no calibration yet (cap_ids 0: the prior), 16 queries per CU by registers;
# inflight -1: what search_with_retry passes (the cap on the concurrency, else nq)
DEFAULTS = dict(dt=F32, metric=L2, dim=128, degree=32, nstart=1, nslots=5001, stride=512, chunks=0, tag_off=0,
                nq=48, L=32, W=1, qcap_max=0, filter=0, range=0, rec=0, qslots=0, qmap=0, out_ids=1, entries=0, srv=0,
                cus=256, maxc=0, vfmt=0, toff=0, ton=0, team_max=-1, pair_min=-1, kcap=64, eighths=6,
                cap_ids=0, waves=16, nfailed=0, inflight=-1)
U8ROWS = dict(dt=U8, stride=128)
PQROWS = dict(dt=PQ, stride=16, chunks=16)


def line(kind, **kw):
    assert not set(kw) - set(FIELDS), kw
    return kind + " " + " ".join(str({**DEFAULTS, **kw}[f]) for f in FIELDS)


def P(**kw):
    return line("P", **kw)


def R(**kw):
    return line("R", **kw)


# (input line, the parent commit's answer)
CASES = [
    # plain_mode: beam width 2, a filter, inline tags, degree 65, 65 start points -- none of them a team (48 queries are one)
    (P(), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42576 | sized 9792 42576'),
    (P(W=2), '0 t0 p0 q0 g0 | ht32 9984+0 prime 9973 shift 0 tb 0 kmax 0 open 7480 | tune 1 lds 41296 | sized 9984 41296'),
    (P(filter=1), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(filter=2), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(tag_off=512), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(degree=64), '0 t0 p0 q0 g0 | ht32 19584+0 prime 19583 shift 0 tb 0 kmax 0 open 14688 | tune 1 lds 79696 | sized 19584 79696'),
    (P(degree=65), '0 t0 p0 q0 g0 | ht32 19904+0 prime 19891 shift 0 tb 0 kmax 0 open 14919 | tune 1 lds 81488 | sized 19904 81488'),
    (P(nstart=64, nslots=5064), '1 t1 p0 q0 g0 | ht32 10304+0 prime 10303 shift 0 tb 0 kmax 0 open 7728 | tune 1 lds 45120 | sized 10304 45120'),
    (P(nstart=65, nslots=5065), '0 t0 p0 q0 g0 | ht32 10304+0 prime 10303 shift 0 tb 0 kmax 0 open 7728 | tune 1 lds 43600 | sized 10304 43600'),
    # team limit: 4 x CUs wavefronts in flight (DANN_DBG_TEAM_MAX_QUERIES), degree 63, 256 queue entries; never for a range
    # search, a caller's query map, the server, persistent waves or under tune_off bit 4; bits 8 / 64 reach the kernel
    (P(nq=1024), '1 t1 p0 q0 g0 | ht32 9344+0 prime 9343 shift 0 tb 0 kmax 0 open 7008 | tune 0 lds 40784 | sized 9344 40784'),
    (P(nq=1025), '0 t0 p0 q0 g0 | ht32 7616+0 prime 7607 shift 0 tb 0 kmax 0 open 5706 | tune 0 lds 31824 | sized 7616 31824'),
    (P(nq=8, team_max=8), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42576 | sized 9792 42576'),
    (P(nq=9, team_max=8), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(degree=63), '1 t1 p0 q0 g0 | ht32 19328+0 prime 19319 shift 0 tb 0 kmax 0 open 14490 | tune 1 lds 80720 | sized 19328 80720'),
    (P(L=255), '1 t1 p0 q0 g0 | ht32 30272+0 prime 30271 shift 0 tb 0 kmax 0 open 22704 | tune 1 lds 126272 | sized 30272 126272'),
    (P(L=256), '0 t0 p0 q0 g0 | ht32 30336+0 prime 30323 shift 0 tb 0 kmax 0 open 22743 | tune 1 lds 124496 | sized 30336 124496'),
    (P(qcap_max=256), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 44352 | sized 9792 44352'),
    (P(qcap_max=257), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42320 | sized 9792 42320'),
    (P(range=1), '0 t0 p0 q0 g0 | ht32 14272+0 prime 14251 shift 0 tb 0 kmax 0 open 10689 | tune 1 lds 58448 | sized 14272 58448'),
    (P(qmap=1), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(srv=64), '4 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(toff=4), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(toff=8), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 3 lds 42576 | sized 9792 42576'),
    (P(toff=64), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 5 lds 42576 | sized 9792 42576'),
    (P(rec=1, qslots=1, out_ids=0), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42576 | sized 9792 42576'),
    (P(nq=48, maxc=32), '3 t0 p0 q0 g32 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(nq=32, maxc=32), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42576 | sized 9792 42576'),
    # team_shape: f32 L2 yes, f32 inner product no, u8 cosine yes, SQ8 cosine no (CosineNormalized is L2-based: yes),
    # packed rows no, dim != 128 no
    (P(metric=IP), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(metric=COSN), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(dt=F16, stride=256), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42576 | sized 9792 42576'),
    (P(**U8ROWS, metric=COSINE), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42192 | sized 9792 42192'),
    (P(**U8ROWS, metric=IP), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42192 | sized 9792 42192'),
    (P(dt=SQ8, stride=144, metric=COSINE), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40160 | sized 9792 40160'),
    (P(dt=SQ8, stride=144, metric=COSN), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42208 | sized 9792 42208'),
    (P(dt=SQ8, stride=144, metric=IP), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42208 | sized 9792 42208'),
    (P(dt=SQ4, stride=80), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40096 | sized 9792 40096'),
    (P(dim=100, stride=400), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40416 | sized 9792 40416'),
    (P(**PQROWS), '5 t0 p0 q1 g0 | ht16 2304+0 prime 4608 shift 19 tb 2 kmax 64 open 3456 | tune 1 lds 10240 | sized 4608 10240'),
    # pair floor: 20 x CUs queries (DANN_DBG_PAIR_MIN_QUERIES), in the call and in flight; not under visited_format 32, tune_off
    # bit 16 or a cap on the concurrency
    (P(**U8ROWS, nq=5119, L=26), '0 t0 p0 q0 g0 | ht32 2304+0 prime 2297 shift 0 tb 0 kmax 0 open 1723 | tune 0 lds 10144 | sized 2304 10144'),
    (P(**U8ROWS, nq=5120, L=26), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(**U8ROWS, nq=63, L=26, pair_min=64), '1 t1 p0 q0 g0 | ht32 8832+0 prime 8831 shift 0 tb 0 kmax 0 open 6624 | tune 1 lds 38304 | sized 8832 38304'),
    (P(**U8ROWS, nq=64, L=26, pair_min=64), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 1 lds 8960 | sized 1840 8960'),
    (P(**U8ROWS, nq=6000, L=26, maxc=5119), '3 t0 p0 q0 g5119 | ht32 2304+0 prime 2297 shift 0 tb 0 kmax 0 open 1723 | tune 0 lds 10144 | sized 2304 10144'),
    (P(**U8ROWS, nq=6000, L=26, maxc=5120), '3 t0 p0 q0 g5120 | ht32 2304+0 prime 2297 shift 0 tb 0 kmax 0 open 1723 | tune 0 lds 10144 | sized 2304 10144'),
    (P(**U8ROWS, nq=6000, L=26, maxc=6000), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(**U8ROWS, nq=6000, L=26, inflight=5119), '0 t0 p0 q0 g0 | ht32 2304+0 prime 2297 shift 0 tb 0 kmax 0 open 1723 | tune 0 lds 10144 | sized 2304 10144'),
    (P(**U8ROWS, nq=6000, L=26, inflight=5120), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(nq=2000, inflight=1024), '1 t1 p0 q0 g0 | ht32 9344+0 prime 9343 shift 0 tb 0 kmax 0 open 7008 | tune 0 lds 40784 | sized 9344 40784'),
    (P(nq=2000, inflight=1025), '0 t0 p0 q0 g0 | ht32 7616+0 prime 7607 shift 0 tb 0 kmax 0 open 5706 | tune 0 lds 31824 | sized 7616 31824'),
    (P(**U8ROWS, nq=5120, L=26, vfmt=32), '0 t0 p0 q0 g0 | ht32 2304+0 prime 2297 shift 0 tb 0 kmax 0 open 1723 | tune 0 lds 10144 | sized 2304 10144'),
    (P(**U8ROWS, nq=5120, L=26, vfmt=16), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(**U8ROWS, nq=5120, L=26, toff=16), '0 t0 p0 q0 g0 | ht32 2304+0 prime 2297 shift 0 tb 0 kmax 0 open 1723 | tune 0 lds 10144 | sized 2304 10144'),
    # pair_shape: L + start points 96 / 97, degree 32 / 33 / 64 / 65, a row stride that is no multiple of 16, other rows
    (P(**U8ROWS, nq=5120, L=31), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(**U8ROWS, nq=5120, L=32), '2 t0 p1 q0 g0 | ht16 952+0 prime 1904 shift 19 tb 4 kmax 64 open 1428 | tune 0 lds 10240 | sized 1904 10240'),
    (P(**U8ROWS, nq=5120, L=64), '2 t0 p1 q0 g0 | ht16 1368+0 prime 2736 shift 19 tb 3 kmax 64 open 2052 | tune 0 lds 14080 | sized 2736 14080'),
    (P(**U8ROWS, nq=5120, L=95), '2 t0 p1 q0 g0 | ht16 1688+0 prime 3376 shift 19 tb 3 kmax 64 open 2532 | tune 0 lds 16640 | sized 3376 16640'),
    (P(**U8ROWS, nq=5120, L=96), '0 t0 p0 q0 g0 | ht16 2176+0 prime 4352 shift 19 tb 2 kmax 64 open 3264 | tune 0 lds 10192 | sized 4352 10192'),
    (P(**U8ROWS, nq=5120, L=26, degree=33), '2 t0 p1 q0 g0 | ht16 984+0 prime 1968 shift 19 tb 4 kmax 64 open 1476 | tune 0 lds 11520 | sized 1968 11520'),
    (P(**U8ROWS, nq=5120, L=26, degree=64), '2 t0 p1 q0 g0 | ht16 1624+0 prime 3248 shift 19 tb 3 kmax 64 open 2436 | tune 0 lds 16640 | sized 3248 16640'),
    (P(**U8ROWS, nq=5120, L=26, degree=65), '0 t0 p0 q0 g0 | ht32 3136+0 prime 3121 shift 0 tb 0 kmax 0 open 2341 | tune 0 lds 13984 | sized 3136 13984'),
    (P(dt=U8, stride=136, nq=5120, L=26), '0 t0 p0 q0 g0 | ht32 2304+0 prime 2297 shift 0 tb 0 kmax 0 open 1723 | tune 0 lds 10160 | sized 2304 10160'),
    (P(dt=I8, stride=128, nq=5120, L=26), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(dt=SQ8, stride=144, nq=5120, L=26), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(nq=5120, L=26), '0 t0 p0 q0 g0 | ht32 2176+0 prime 2161 shift 0 tb 0 kmax 0 open 1621 | tune 0 lds 10016 | sized 2176 10016'),
    (P(**U8ROWS, nq=5120, L=26, nstart=33, nslots=5033), '0 t0 p0 q0 g0 | ht32 2240+0 prime 2239 shift 0 tb 0 kmax 0 open 1680 | tune 0 lds 10144 | sized 2240 10144'),
    (P(**U8ROWS, nq=5120, L=26, range=1), '0 t0 p0 q0 g0 | ht32 2624+0 prime 2621 shift 0 tb 0 kmax 0 open 1966 | tune 0 lds 11424 | sized 2624 11424'),
    # pair table: the first LDS step that holds the p90 with a tenth to spare; a p90 no step holds revokes the pairing
    (P(**U8ROWS, nq=5120, L=26, cap_ids=1255), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(**U8ROWS, nq=5120, L=26, cap_ids=1256), '2 t0 p1 q0 g0 | ht16 1080+0 prime 2160 shift 19 tb 3 kmax 64 open 1620 | tune 0 lds 10240 | sized 2160 10240'),
    (P(**U8ROWS, nq=5120, L=64, degree=64, cap_ids=4000), '2 t0 p1 q0 g0 | ht16 3000+0 prime 6000 shift 19 tb 2 kmax 64 open 4500 | tune 0 lds 28160 | sized 6000 28160'),
    (P(**U8ROWS, nq=5120, L=26, cap_ids=22342), '2 t0 p1 q0 g0 | ht16 16384+0 prime 32768 shift 19 tb 0 kmax 64 open 24576 | tune 0 lds 132672 | sized 32768 132672'),
    (P(**U8ROWS, nq=5120, L=26, cap_ids=22343), '0 t0 p0 q0 g0 | ht16 20224+0 prime 40448 shift 19 tb 0 kmax 64 open 30336 | tune 0 lds 81824 | sized 40448 81824'),
    (P(**U8ROWS, nq=5120, L=26, cap_ids=40000), '0 t0 p0 q0 g0 | ht32 32768+0 prime 32749 shift 0 tb 0 kmax 0 open 24562 | tune 0 lds 132000 | sized 32768 132000'),
    (P(**U8ROWS, nq=5120, L=26, eighths=4), '2 t0 p1 q0 g0 | ht16 1240+0 prime 2480 shift 19 tb 3 kmax 64 open 1240 | tune 0 lds 11520 | sized 2480 11520'),
    (P(**U8ROWS, nq=5120, L=26, eighths=7), '2 t0 p1 q0 g0 | ht16 760+0 prime 1520 shift 19 tb 4 kmax 64 open 1330 | tune 0 lds 7680 | sized 1520 7680'),
    (P(**U8ROWS, nq=5120, L=26, nslots=1000001), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 12 tb 11 kmax 31 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(**U8ROWS, nq=5120, L=26, nslots=100000001), '2 t0 p1 q0 g0 | ht16 8312+128 prime 16624 shift 5 tb 14 kmax 3 open 12468 | tune 0 lds 69120 | sized 16624 69120'),
    # PQ table kernel: chunks 16 / 17, 48 / 49, 64 / 65, 256 / 257 queue entries, L2 and inner product only
    (P(**PQROWS, L=96), '5 t0 p0 q1 g0 | ht16 2176+0 prime 4352 shift 19 tb 2 kmax 64 open 3264 | tune 1 lds 10240 | sized 4352 10240'),
    (P(dt=PQ, chunks=17, stride=32, L=96), '5 t0 p0 q1 g0 | ht16 4736+0 prime 9472 shift 19 tb 1 kmax 64 open 7104 | tune 1 lds 20480 | sized 9472 20480'),
    (P(dt=PQ, chunks=48, stride=48, L=96), '5 t0 p0 q1 g0 | ht16 4736+0 prime 9472 shift 19 tb 1 kmax 64 open 7104 | tune 1 lds 20480 | sized 9472 20480'),
    (P(dt=PQ, chunks=49, stride=64, L=96), '5 t0 p0 q1 g0 | ht16 9856+0 prime 19712 shift 19 tb 0 kmax 64 open 14784 | tune 1 lds 40960 | sized 19712 40960'),
    (P(dt=PQ, chunks=64, stride=64, L=96), '5 t0 p0 q1 g0 | ht16 9856+0 prime 19712 shift 19 tb 0 kmax 64 open 14784 | tune 1 lds 40960 | sized 19712 40960'),
    (P(dt=PQ, chunks=65, stride=80, L=96), '0 t0 p0 q0 g0 | ht32 17728+0 prime 17713 shift 0 tb 0 kmax 0 open 13285 | tune 1 lds 138832 | sized 17728 138832'),
    (P(**PQROWS, L=63), '5 t0 p0 q1 g0 | ht16 2304+0 prime 4608 shift 19 tb 2 kmax 64 open 3456 | tune 1 lds 10240 | sized 4608 10240'),
    (P(**PQROWS, L=64), '5 t0 p0 q1 g0 | ht16 2176+0 prime 4352 shift 19 tb 2 kmax 64 open 3264 | tune 1 lds 10240 | sized 4352 10240'),
    (P(**PQROWS, L=127), '5 t0 p0 q1 g0 | ht16 2176+0 prime 4352 shift 19 tb 2 kmax 64 open 3264 | tune 1 lds 10240 | sized 4352 10240'),
    (P(**PQROWS, L=128), '5 t0 p0 q1 g0 | ht16 1920+0 prime 3840 shift 19 tb 3 kmax 64 open 2880 | tune 1 lds 10240 | sized 3840 10240'),
    (P(**PQROWS, L=255), '5 t0 p0 q1 g0 | ht16 2880+0 prime 5760 shift 19 tb 2 kmax 64 open 4320 | tune 1 lds 14080 | sized 5760 14080'),
    (P(**PQROWS, L=256), '0 t0 p0 q0 g0 | ht32 30336+0 prime 30323 shift 0 tb 0 kmax 0 open 22743 | tune 1 lds 140368 | sized 30336 140368'),
    (P(**PQROWS, metric=IP), '5 t0 p0 q1 g0 | ht16 2304+0 prime 4608 shift 19 tb 2 kmax 64 open 3456 | tune 1 lds 10240 | sized 4608 10240'),
    (P(**PQROWS, metric=COSINE), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 56400 | sized 9792 56400'),
    (P(dt=PQ, chunks=17, stride=16), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 57424 | sized 9792 57424'),
    (P(**PQROWS, vfmt=32), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 56400 | sized 9792 56400'),
    (P(**PQROWS, toff=32), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 56400 | sized 9792 56400'),
    (P(**PQROWS, nq=4096, maxc=1024), '3 t0 p0 q0 g1024 | ht32 5888+0 prime 5881 shift 0 tb 0 kmax 0 open 4411 | tune 0 lds 40784 | sized 5888 40784'),
    (P(**PQROWS, nq=4096, L=96, cap_ids=3000), '5 t0 p0 q1 g0 | ht16 2496+0 prime 4992 shift 19 tb 2 kmax 64 open 3744 | tune 0 lds 11520 | sized 4992 11520'),
    (P(**PQROWS, nq=4096, L=96, cap_ids=44684), '5 t0 p0 q1 g0 | ht16 32768+0 prime 65536 shift 19 tb 0 kmax 64 open 49152 | tune 0 lds 132608 | sized 65536 132608'),
    (P(**PQROWS, nq=4096, L=96, cap_ids=44685), '0 t0 p0 q0 g0 | ht32 32768+0 prime 32749 shift 0 tb 0 kmax 0 open 24562 | tune 0 lds 148816 | sized 32768 148816'),
    (P(**PQROWS, nq=4096, L=96, nslots=1000001), '5 t0 p0 q1 g0 | ht16 2176+0 prime 4352 shift 12 tb 9 kmax 64 open 3264 | tune 0 lds 10240 | sized 4352 10240'),
    # overflow words: none from eight probes per id on (DANN_DBG_HT16_MAX_PROBES 8 / 7 / 3), 128 for a pair, 256 for the PQ table
    ('G 920 5001 64', '1 shift 19 tb 4 kmax 64 slots 1840 ov 0 0'),
    ('G 920 5001 8', '1 shift 19 tb 4 kmax 8 slots 1840 ov 0 0'),
    ('G 920 5001 7', '1 shift 19 tb 4 kmax 7 slots 1840 ov 128 256'),
    ('G 8192 100000001 64', '1 shift 5 tb 14 kmax 3 slots 16384 ov 128 256'),
    ('G 16 100 64', '0 shift 0 tb 0 kmax 0 slots 0 ov 0 0'),
    (P(**U8ROWS, nq=5120, L=26, kcap=8), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 8 open 1380 | tune 0 lds 8960 | sized 1840 8960'),
    (P(**U8ROWS, nq=5120, L=26, kcap=7), '2 t0 p1 q0 g0 | ht16 952+128 prime 1904 shift 19 tb 4 kmax 7 open 1428 | tune 0 lds 10240 | sized 1904 10240'),
    (P(**U8ROWS, nq=5120, L=26, kcap=3), '2 t0 p1 q0 g0 | ht16 952+128 prime 1904 shift 19 tb 4 kmax 3 open 1428 | tune 0 lds 10240 | sized 1904 10240'),
    (P(**PQROWS, nq=4096, L=96, kcap=8), '5 t0 p0 q1 g0 | ht16 2176+0 prime 4352 shift 19 tb 2 kmax 8 open 3264 | tune 0 lds 10240 | sized 4352 10240'),
    (P(**PQROWS, nq=4096, L=96, kcap=7), '5 t0 p0 q1 g0 | ht16 1920+256 prime 3840 shift 19 tb 3 kmax 7 open 2880 | tune 0 lds 10240 | sized 3840 10240'),
    (P(**PQROWS, nq=4096, L=96, kcap=3), '5 t0 p0 q1 g0 | ht16 1920+256 prime 3840 shift 19 tb 3 kmax 3 open 2880 | tune 0 lds 10240 | sized 3840 10240'),
    # choose_visited_table: 16-bit entries where they buy a higher occupancy step and the 32-bit table leaves at most a dozen
    # queries per CU (w32 > 12: stay), the forced formats, the sparser-table walk, a footprint no step holds (waves_of == 0),
    # the share of a CU a small launch has (tune_off bit 2: not taken into account)
    (P(nq=4096, L=56, nslots=10000001, cap_ids=2300), '0 t0 p0 q0 g0 | ht16 2112+0 prime 4224 shift 8 tb 13 kmax 7 open 3168 | tune 0 lds 10000 | sized 4224 10000'),
    (P(nq=4096, L=56, nslots=10000001, cap_ids=2300, vfmt=32), '0 t0 p0 q0 g0 | ht32 3072+0 prime 3067 shift 0 tb 0 kmax 0 open 2301 | tune 0 lds 13840 | sized 3072 13840'),
    (P(nq=4096, L=56, nslots=10000001, cap_ids=2300, vfmt=16), '0 t0 p0 q0 g0 | ht16 2112+0 prime 4224 shift 8 tb 13 kmax 7 open 3168 | tune 0 lds 10000 | sized 4224 10000'),
    (P(nq=4096, L=56, nslots=10000001, cap_ids=1824), '0 t0 p0 q0 g0 | ht32 2432+0 prime 2423 shift 0 tb 0 kmax 0 open 1818 | tune 0 lds 11280 | sized 2432 11280'),
    (P(nq=4096, L=56, nslots=10000001, cap_ids=1825), '0 t0 p0 q0 g0 | ht16 2112+0 prime 4224 shift 8 tb 13 kmax 7 open 3168 | tune 0 lds 10000 | sized 4224 10000'),
    (P(nq=4096, L=56, nslots=10000001, cap_ids=1825, waves=8), '0 t0 p0 q0 g0 | ht32 4672+0 prime 4663 shift 0 tb 0 kmax 0 open 3498 | tune 0 lds 20240 | sized 4672 20240'),
    (P(**U8ROWS, nq=4096, L=26, nslots=1000001, cap_ids=1100, waves=24), '0 t0 p0 q0 g0 | ht32 2304+0 prime 2297 shift 0 tb 0 kmax 0 open 1723 | tune 0 lds 10144 | sized 2304 10144'),
    (P(**U8ROWS, nq=4096, L=26, nslots=1000001, cap_ids=1100, waves=24, vfmt=16), '0 t0 p0 q0 g0 | ht16 2304+0 prime 4608 shift 12 tb 9 kmax 64 open 3456 | tune 0 lds 10144 | sized 4608 10144'),
    (P(nq=4096, L=100, cap_ids=4000), '0 t0 p0 q0 g0 | ht16 2688+0 prime 5376 shift 19 tb 2 kmax 64 open 4032 | tune 0 lds 12656 | sized 5376 12656'),
    (P(nq=4096, L=100, cap_ids=4000, eighths=4), '0 t0 p0 q0 g0 | ht16 4608+0 prime 9216 shift 19 tb 1 kmax 64 open 4608 | tune 0 lds 20336 | sized 9216 20336'),
    (P(nq=4096, L=100, cap_ids=4000, eighths=7), '0 t0 p0 q0 g0 | ht16 2368+0 prime 4736 shift 19 tb 2 kmax 64 open 4144 | tune 0 lds 11376 | sized 4736 11376'),
    (P(nq=4096, L=56, nslots=100000001, cap_ids=2300), '0 t0 p0 q0 g0 | ht32 3072+0 prime 3067 shift 0 tb 0 kmax 0 open 2301 | tune 0 lds 13840 | sized 3072 13840'),
    (P(nq=4096, L=56, nslots=100000001, cap_ids=2300, vfmt=16), '0 t0 p0 q0 g0 | ht16 12288+0 prime 24576 shift 5 tb 14 kmax 3 open 18432 | tune 0 lds 50704 | sized 24576 50704'),
    (P(dt=PQ, chunks=128, stride=128, nq=4096, cap_ids=6000), '0 t0 p0 q0 g0 | ht16 7936+0 prime 15872 shift 19 tb 1 kmax 64 open 11904 | tune 0 lds 163664 | sized 15872 163664'),
    (P(dt=PQ, chunks=128, stride=128, nq=4096, cap_ids=6000, vfmt=16), '0 t0 p0 q0 g0 | ht16 7936+0 prime 15872 shift 19 tb 1 kmax 64 open 11904 | tune 0 lds 163664 | sized 15872 163664'),
    (P(dt=PQ, chunks=150, stride=160, nq=4096, cap_ids=6000), '0 t0 p0 q0 g0 | ht32 8000+0 prime 7993 shift 0 tb 0 kmax 0 open 5995 | tune 0 lds 186448 | sized 8000 186448'),
    (P(dt=PQ, chunks=150, stride=160, nq=4096, cap_ids=6000, vfmt=16), '0 t0 p0 q0 g0 | ht16 24000+0 prime 48000 shift 19 tb 0 kmax 64 open 36000 | tune 0 lds 250448 | sized 48000 250448'),
    (P(nq=300), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42576 | sized 9792 42576'),
    (P(nq=300, toff=2), '1 t1 p0 q0 g0 | ht32 1664+0 prime 1663 shift 0 tb 0 kmax 0 open 1248 | tune 1 lds 10064 | sized 1664 10064'),
    (P(nq=2048, L=100), '0 t0 p0 q0 g0 | ht32 4608+0 prime 4603 shift 0 tb 0 kmax 0 open 3453 | tune 0 lds 20336 | sized 4608 20336'),
    (P(nq=2049, L=100), '0 t0 p0 q0 g0 | ht32 3968+0 prime 3967 shift 0 tb 0 kmax 0 open 2976 | tune 0 lds 17776 | sized 3968 17776'),
    (P(W=4, L=100, nq=4096), '0 t0 p0 q0 g0 | ht32 3200+0 prime 3191 shift 0 tb 0 kmax 0 open 2394 | tune 0 lds 15216 | sized 3200 15216'),
    (P(range=1, nq=4096, L=20), '0 t0 p0 q0 g0 | ht32 2560+0 prime 2557 shift 0 tb 0 kmax 0 open 1918 | tune 0 lds 11504 | sized 2560 11504'),
    # explicit size (dann_set_visited_bits 7 and 15), with and without visited_format 16; the special kernels keep a table they can hold
    (P(entries=128), '1 t1 p0 q0 g0 | ht32 128+0 prime 127 shift 0 tb 0 kmax 0 open 96 | tune 1 lds 3920 | sized 0 0'),
    (P(entries=128, vfmt=16), '1 t1 p0 q0 g0 | ht32 128+0 prime 127 shift 0 tb 0 kmax 0 open 96 | tune 1 lds 3920 | sized 0 0'),
    (P(entries=32768), '1 t1 p0 q0 g0 | ht32 32768+0 prime 32749 shift 0 tb 0 kmax 0 open 24562 | tune 1 lds 134480 | sized 0 0'),
    (P(entries=32768, vfmt=16), '1 t1 p0 q0 g0 | ht32 32768+0 prime 32749 shift 0 tb 0 kmax 0 open 24562 | tune 1 lds 134480 | sized 0 0'),
    (P(entries=128, vfmt=32), '1 t1 p0 q0 g0 | ht32 128+0 prime 127 shift 0 tb 0 kmax 0 open 96 | tune 1 lds 3920 | sized 0 0'),
    (P(entries=128, nq=4096, toff=4), '0 t0 p0 q0 g0 | ht32 128+0 prime 127 shift 0 tb 0 kmax 0 open 96 | tune 0 lds 1872 | sized 0 0'),
    (P(entries=100, nq=4096, vfmt=16), '0 t0 p0 q0 g0 | ht16 128+0 prime 256 shift 19 tb 6 kmax 64 open 192 | tune 0 lds 1872 | sized 0 0'),
    (P(entries=128, nq=4096, vfmt=16, nslots=100000001), '0 t0 p0 q0 g0 | ht16 8192+0 prime 16384 shift 5 tb 14 kmax 3 open 12288 | tune 0 lds 34128 | sized 0 0'),
    (P(**U8ROWS, nq=5120, L=26, entries=128), '0 t0 p0 q0 g0 | ht32 128+0 prime 127 shift 0 tb 0 kmax 0 open 96 | tune 0 lds 1440 | sized 0 0'),
    (P(**U8ROWS, nq=5120, L=26, entries=128, vfmt=16), '2 t0 p1 q0 g0 | ht16 128+0 prime 256 shift 19 tb 6 kmax 64 open 192 | tune 0 lds 2624 | sized 0 0'),
    (P(**U8ROWS, nq=5120, L=26, entries=32768, vfmt=16), '0 t0 p0 q0 g0 | ht16 32768+0 prime 65536 shift 19 tb 0 kmax 64 open 49152 | tune 0 lds 132000 | sized 0 0'),
    (P(**U8ROWS, nq=5120, L=26, entries=128, vfmt=16, kcap=7), '2 t0 p1 q0 g0 | ht16 128+128 prime 256 shift 19 tb 6 kmax 7 open 192 | tune 0 lds 3648 | sized 0 0'),
    (P(**U8ROWS, nq=5120, L=26, entries=128, vfmt=16, nslots=100000001), '2 t0 p1 q0 g0 | ht16 8192+128 prime 16384 shift 5 tb 14 kmax 3 open 12288 | tune 0 lds 68160 | sized 0 0'),
    (P(**PQROWS, entries=128), '5 t0 p0 q1 g0 | ht16 128+0 prime 256 shift 19 tb 6 kmax 64 open 192 | tune 1 lds 1536 | sized 0 0'),
    (P(**PQROWS, entries=32768), '5 t0 p0 q1 g0 | ht16 32768+0 prime 65536 shift 19 tb 0 kmax 64 open 49152 | tune 1 lds 132096 | sized 0 0'),
    (P(**PQROWS, entries=128, kcap=7), '5 t0 p0 q1 g0 | ht16 128+256 prime 256 shift 19 tb 6 kmax 7 open 192 | tune 1 lds 2560 | sized 0 0'),
    (P(**PQROWS, entries=128, vfmt=32), '0 t0 p0 q0 g0 | ht32 128+0 prime 127 shift 0 tb 0 kmax 0 open 96 | tune 1 lds 17744 | sized 0 0'),
    # the floor: the open table holds the start points and one hop (nstart + W x R + 1 ids), or the launch is refused
    (P(entries=128, degree=64, W=4), '0 t0 p0 q0 g0 | ht32 512+0 prime 509 shift 0 tb 0 kmax 0 open 382 | tune 1 lds 4944 | sized 0 0'),
    (P(entries=128, degree=64, W=4, vfmt=16), '0 t0 p0 q0 g0 | ht32 512+0 prime 509 shift 0 tb 0 kmax 0 open 382 | tune 1 lds 4944 | sized 0 0'),
    (P(entries=128, degree=92, nq=4096), '0 t0 p0 q0 g0 | ht32 128+0 prime 127 shift 0 tb 0 kmax 0 open 96 | tune 0 lds 2384 | sized 0 0'),
    (P(entries=128, degree=93, nq=4096), '0 t0 p0 q0 g0 | ht32 256+0 prime 251 shift 0 tb 0 kmax 0 open 189 | tune 0 lds 2896 | sized 0 0'),
    (P(**U8ROWS, nq=5120, L=26, entries=64, vfmt=16, degree=64), '2 t0 p1 q0 g0 | ht16 64+0 prime 128 shift 19 tb 7 kmax 64 open 96 | tune 0 lds 4160 | sized 0 0'),
    (P(W=16, degree=1534), '0 t0 p0 q0 g0 | ht32 32768+0 prime 32749 shift 0 tb 0 kmax 0 open 24562 | tune 1 lds 328528 | sized 32768 328528'),
    (P(W=16, degree=1535), 'error -1: visited table: 1 start points + beam 16 x degree 1535 do not fit the largest LDS table'),
    (P(W=16, degree=1534, entries=128), '0 t0 p0 q0 g0 | ht32 32768+0 prime 32749 shift 0 tb 0 kmax 0 open 24562 | tune 1 lds 328528 | sized 0 0'),
    (P(W=16, degree=1535, entries=128), 'error -1: visited table: 1 start points + beam 16 x degree 1535 do not fit the largest LDS table'),
    (P(W=16, degree=2000, vfmt=16), 'error -1: visited table: 1 start points + beam 16 x degree 2000 do not fit the largest LDS table'),
    # row prefetch: up to 3 x CUs wavefronts in flight, never under tune_off bit 1, always under tune_on bit 1
    (P(nq=768, toff=4), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(nq=769, toff=4), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 0 lds 40528 | sized 9792 40528'),
    (P(nq=768, toff=5), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 0 lds 40528 | sized 9792 40528'),
    (P(nq=4096, ton=1), '0 t0 p0 q0 g0 | ht32 2176+0 prime 2161 shift 0 tb 0 kmax 0 open 1621 | tune 1 lds 10064 | sized 2176 10064'),
    (P(nq=4096, maxc=768), '3 t0 p0 q0 g768 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(nq=4096, maxc=769), '3 t0 p0 q0 g769 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 0 lds 40528 | sized 9792 40528'),
    # retry: a team -> one wave with the same table; pair / PQ table -> one wave with the table doubled; then doubling to
    # 32 768 entries, or until the footprint passes 160 KiB; persistent waves while more queries are left than the cap
    (R(nfailed=1), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42576 | sized 9792 42576 / 0 t0 p0 q0 g0 ht32 9792+0 nq 1 lds 40528 / 0 t0 p0 q0 g0 ht32 19584+0 nq 1 lds 79696 / 0 t0 p0 q0 g0 ht32 32768+0 nq 1 lds 132432 / stop'),
    (R(nq=4096, nfailed=7), '0 t0 p0 q0 g0 | ht32 2176+0 prime 2161 shift 0 tb 0 kmax 0 open 1621 | tune 0 lds 10064 | sized 2176 10064 / 0 t0 p0 q0 g0 ht32 4352+0 nq 7 lds 18768 / 0 t0 p0 q0 g0 ht32 8704+0 nq 7 lds 36176 / 0 t0 p0 q0 g0 ht32 17408+0 nq 7 lds 70992 / 0 t0 p0 q0 g0 ht32 32768+0 nq 7 lds 132432 / stop'),
    (R(**U8ROWS, nq=5120, L=26, nfailed=3), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 0 lds 8960 | sized 1840 8960 / 0 t0 p0 q0 g0 ht16 1840+0 nq 3 lds 8288 / 0 t0 p0 q0 g0 ht16 3680+0 nq 3 lds 15648 / 0 t0 p0 q0 g0 ht16 7360+0 nq 3 lds 30368 / 0 t0 p0 q0 g0 ht16 14720+0 nq 3 lds 59808 / 0 t0 p0 q0 g0 ht16 29440+0 nq 3 lds 118688 / 0 t0 p0 q0 g0 ht16 32768+0 nq 3 lds 132000 / stop'),
    (R(**U8ROWS, nq=5120, L=26, kcap=7, nfailed=3), '2 t0 p1 q0 g0 | ht16 952+128 prime 1904 shift 19 tb 4 kmax 7 open 1428 | tune 0 lds 10240 | sized 1904 10240 / 0 t0 p0 q0 g0 ht16 1904+0 nq 3 lds 8544 / 0 t0 p0 q0 g0 ht16 3808+0 nq 3 lds 16160 / 0 t0 p0 q0 g0 ht16 7616+0 nq 3 lds 31392 / 0 t0 p0 q0 g0 ht16 15232+0 nq 3 lds 61856 / 0 t0 p0 q0 g0 ht16 30464+0 nq 3 lds 122784 / 0 t0 p0 q0 g0 ht16 32768+0 nq 3 lds 132000 / stop'),
    (R(**PQROWS, nq=64, nfailed=2), '5 t0 p0 q1 g0 | ht16 2304+0 prime 4608 shift 19 tb 2 kmax 64 open 3456 | tune 1 lds 10240 | sized 4608 10240 / 0 t0 p0 q0 g0 ht16 4608+0 nq 2 lds 35664 / 0 t0 p0 q0 g0 ht16 9216+0 nq 2 lds 54096 / 0 t0 p0 q0 g0 ht16 18432+0 nq 2 lds 90960 / 0 t0 p0 q0 g0 ht16 32768+0 nq 2 lds 148304 / stop'),
    (R(**PQROWS, nq=64, kcap=3, nslots=1000001, nfailed=2), '5 t0 p0 q1 g0 | ht16 2048+256 prime 4096 shift 12 tb 9 kmax 3 open 3072 | tune 1 lds 10240 | sized 4096 10240 / 0 t0 p0 q0 g0 ht16 4096+0 nq 2 lds 33616 / 0 t0 p0 q0 g0 ht16 8192+0 nq 2 lds 50000 / 0 t0 p0 q0 g0 ht16 16384+0 nq 2 lds 82768 / 0 t0 p0 q0 g0 ht16 32768+0 nq 2 lds 148304 / stop'),
    (R(entries=32768, nq=4096, nfailed=1), '0 t0 p0 q0 g0 | ht32 32768+0 prime 32749 shift 0 tb 0 kmax 0 open 24562 | tune 0 lds 132432 | sized 0 0 / stop'),
    (R(entries=16384, nq=4096, vfmt=16, nfailed=1), '0 t0 p0 q0 g0 | ht16 16384+0 prime 32768 shift 19 tb 0 kmax 64 open 24576 | tune 0 lds 66896 | sized 0 0 / 0 t0 p0 q0 g0 ht16 32768+0 nq 1 lds 132432 / stop'),
    (R(nq=6000, maxc=1024, nfailed=2000), '3 t0 p0 q0 g1024 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 0 lds 40528 | sized 9792 40528 / 3 t0 p0 q0 g1024 ht32 19584+0 nq 2000 lds 79696 / 3 t0 p0 q0 g1024 ht32 32768+0 nq 2000 lds 132432 / stop'),
    (R(nq=6000, maxc=1024, nfailed=1024), '3 t0 p0 q0 g1024 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 0 lds 40528 | sized 9792 40528 / 0 t0 p0 q0 g0 ht32 19584+0 nq 1024 lds 79696 / 0 t0 p0 q0 g0 ht32 32768+0 nq 1024 lds 132432 / stop'),
    (R(dt=PQ, chunks=100, stride=112, nq=4096, nfailed=5), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 0 lds 142416 | sized 9792 142416 / stop'),
    (R(dt=PQ, chunks=128, stride=128, nq=4096, cap_ids=6000, nfailed=5), '0 t0 p0 q0 g0 | ht16 7936+0 prime 15872 shift 19 tb 1 kmax 64 open 11904 | tune 0 lds 163664 | sized 15872 163664 / stop'),
    (R(nq=48, L=255, nfailed=48), '1 t1 p0 q0 g0 | ht32 30272+0 prime 30271 shift 0 tb 0 kmax 0 open 22704 | tune 1 lds 126272 | sized 30272 126272 / 0 t0 p0 q0 g0 ht32 30272+0 nq 48 lds 124224 / 0 t0 p0 q0 g0 ht32 32768+0 nq 48 lds 134208 / stop'),
    # device: the configurations of scratch/launch_plan_compare.py (5 000 rows, degree 32, 256 CUs) with the waves the parent
    # printed from the kernels' VGPRs on an MI355X -- 121 VGPRs: 16, the filtered kernel's 179: 8, the u8 kernel's 60 / 62: 32 --
    # and the p90 it calibrated; 'sized' is the slot count and LDS of its verbose line (profiles/launch_plan_parent.txt)
    (P(nq=48, L=32), '1 t1 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 42576 | sized 9792 42576'),
    (P(nq=48, L=32, toff=4), '0 t0 p0 q0 g0 | ht32 9792+0 prime 9791 shift 0 tb 0 kmax 0 open 7344 | tune 1 lds 40528 | sized 9792 40528'),
    (P(nq=300, L=40, toff=4), '0 t0 p0 q0 g0 | ht32 11072+0 prime 11071 shift 0 tb 0 kmax 0 open 8304 | tune 1 lds 45712 | sized 11072 45712'),
    (P(nq=300, L=40, toff=4, cap_ids=1280), '0 t0 p0 q0 g0 | ht32 10240+0 prime 10223 shift 0 tb 0 kmax 0 open 7668 | tune 1 lds 42384 | sized 10240 42384'),
    (P(nq=300, L=48, toff=4, vfmt=16), '0 t0 p0 q0 g0 | ht16 6080+0 prime 12160 shift 19 tb 1 kmax 64 open 9120 | tune 1 lds 25808 | sized 12160 25808'),
    (P(nq=300, L=48, toff=4, vfmt=16, cap_ids=1408), '0 t0 p0 q0 g0 | ht16 5632+0 prime 11264 shift 19 tb 1 kmax 64 open 8448 | tune 1 lds 24016 | sized 11264 24016'),
    (P(nq=300, L=26, toff=4, vfmt=16, entries=128), '0 t0 p0 q0 g0 | ht16 128+0 prime 256 shift 19 tb 6 kmax 64 open 192 | tune 1 lds 1824 | sized 0 0'),
    (P(nq=300, L=26, toff=4, vfmt=32, entries=128), '0 t0 p0 q0 g0 | ht32 128+0 prime 127 shift 0 tb 0 kmax 0 open 96 | tune 1 lds 1824 | sized 0 0'),
    (P(nq=300, L=56, toff=4, maxc=128), '3 t0 p0 q0 g128 | ht32 13248+0 prime 13241 shift 0 tb 0 kmax 0 open 9931 | tune 1 lds 54544 | sized 13248 54544'),
    (P(nq=300, L=56, toff=4, maxc=128, cap_ids=1536), '3 t0 p0 q0 g128 | ht32 12288+0 prime 12281 shift 0 tb 0 kmax 0 open 9211 | tune 1 lds 50704 | sized 12288 50704'),
    (P(nq=300, L=30, toff=4, filter=1, waves=8), '0 t0 p0 q0 g0 | ht32 9472+0 prime 9467 shift 0 tb 0 kmax 0 open 7101 | tune 1 lds 39232 | sized 9472 39232'),
    (P(nq=300, L=30, toff=4, filter=1, waves=8, cap_ids=1024), '0 t0 p0 q0 g0 | ht32 8192+0 prime 8191 shift 0 tb 0 kmax 0 open 6144 | tune 1 lds 34112 | sized 8192 34112'),
    (P(nq=300, L=20, toff=4, range=1), '0 t0 p0 q0 g0 | ht32 14272+0 prime 14251 shift 0 tb 0 kmax 0 open 10689 | tune 1 lds 58352 | sized 14272 58352'),
    (P(**U8ROWS, nq=64, L=26, pair_min=64, waves=32), '2 t0 p1 q0 g0 | ht16 920+0 prime 1840 shift 19 tb 4 kmax 64 open 1380 | tune 1 lds 8960 | sized 1840 8960'),
    (P(**U8ROWS, nq=64, L=64, pair_min=64, waves=32), '2 t0 p1 q0 g0 | ht16 1368+0 prime 2736 shift 19 tb 3 kmax 64 open 2052 | tune 1 lds 14080 | sized 2736 14080'),
    (P(**U8ROWS, nq=300, L=26, pair_min=64, waves=32, cap_ids=896), '2 t0 p1 q0 g0 | ht16 760+0 prime 1520 shift 19 tb 4 kmax 64 open 1140 | tune 1 lds 7680 | sized 1520 7680'),
    (P(**U8ROWS, nq=64, L=26, pair_min=64, waves=32, kcap=3), '2 t0 p1 q0 g0 | ht16 952+128 prime 1904 shift 19 tb 4 kmax 3 open 1428 | tune 1 lds 10240 | sized 1904 10240'),
    (P(**U8ROWS, nq=64, L=64, pair_min=64, waves=32, kcap=3), '2 t0 p1 q0 g0 | ht16 1400+128 prime 2800 shift 19 tb 3 kmax 3 open 2100 | tune 1 lds 15360 | sized 2800 15360'),
    (P(**U8ROWS, nq=300, L=26, pair_min=64, waves=32, kcap=3, cap_ids=960), '2 t0 p1 q0 g0 | ht16 792+128 prime 1584 shift 19 tb 4 kmax 3 open 1188 | tune 1 lds 8960 | sized 1584 8960'),
    (P(**PQROWS, nq=48, L=32), '5 t0 p0 q1 g0 | ht16 2304+0 prime 4608 shift 19 tb 2 kmax 64 open 3456 | tune 1 lds 10240 | sized 4608 10240'),
    (P(**PQROWS, nq=300, L=32, cap_ids=1088), '5 t0 p0 q1 g0 | ht16 2304+0 prime 4608 shift 19 tb 2 kmax 64 open 3456 | tune 1 lds 10240 | sized 4608 10240'),
    (P(dt=PQ, chunks=48, stride=48, nq=48, L=32), '5 t0 p0 q1 g0 | ht16 4864+0 prime 9728 shift 19 tb 1 kmax 64 open 7296 | tune 1 lds 20480 | sized 9728 20480'),
    (P(dt=PQ, chunks=48, stride=48, nq=300, L=32, cap_ids=1088), '5 t0 p0 q1 g0 | ht16 4864+0 prime 9728 shift 19 tb 1 kmax 64 open 7296 | tune 1 lds 20480 | sized 9728 20480'),
]

MODEL_GEOMETRIES = [(32, 100), (64, 4001), (256, 70000), (1024, 1 << 20), (2048, 1_000_001), (4096, 10_000_001),
                    (928, 1_000_001), (768, 1_000_001), (1504, 10_000_001), (36, 4001), (48, 100), (16, 100),
                    (1024, 100_000_001), (8192, 100_000_001), (1024, 1000), (64, 5001), (256, 3_000_000)]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_plan")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "diskann_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)

    def plan(lines):
        r = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=60,
                           check=True)
        return r.stdout.splitlines()
    return plan


def test_plan_matches_the_table(planner):
    got = planner([c for c, _ in CASES])
    assert len(got) == len(CASES)
    for (case, want), g in zip(CASES, got):
        assert g == want, case


def test_geometry_is_the_python_model(planner):
    """ht16_geometry is what tests/test_visited16_model.py restates: the same answer on that file's cases"""
    spec = importlib.util.spec_from_file_location("visited16_model", os.path.join(ROOT, "tests", "test_visited16_model.py"))
    model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(model)
    got = planner([f"G {w} {n} 64" for w, n in MODEL_GEOMETRIES])
    assert len(got) == len(MODEL_GEOMETRIES)
    for (w, n), g in zip(MODEL_GEOMETRIES, got):
        m, f = model.geometry(w, n), g.split()
        if m is None:
            assert f[0] == "0", (w, n, g)
        else:
            assert (int(f[0]), int(f[2]), int(f[4]), int(f[6]), int(f[8])) == (1, 32 - m["m"], m["tb"], m["kmax"], 2 * w), (w, n, g)
