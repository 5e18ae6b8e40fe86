// Host-side planning of a beam-search launch (search_kernels.hip): kernel family, visited table, tuning bits and the
// re-run of overflowed queries, as pure functions of the launch arguments, the per-index knobs and the calibration, in
// three stages: plan_family, plan_table (the launch's one HIP query sits between them), plan_retry.  Results never
// depend on a plan.  Anonymous namespace, like launch_shape.h.  No HIP here: tests/test_launch_plan_host.py uses g++.
#pragma once
#include <math.h>
#include <stdio.h>

#include "launch_shape.h"

namespace dann {
namespace {

// the per-index inputs, read once per call (search_kernels.hip: launch_knobs)
struct LaunchKnobs {
    uint32_t num_cus, max_concurrency, visited_format;  // dann_set_max_concurrency / dann_set_visited_format
    uint32_t tune_off, tune_on;                         // DANN_DBG_TUNE_OFF / DANN_DBG_TUNE_ON masks
    uint32_t team_max_queries, pair_min_queries;        // DANN_DBG_TEAM_MAX_QUERIES / DANN_DBG_PAIR_MIN_QUERIES
    uint32_t ht16_kcap, open_eighths;                   // DANN_DBG_HT16_MAX_PROBES (1 .. 64) / DANN_DBG_HT16_OPEN_EIGHTHS (4 .. 7)
};
using PlanMsg = char[160];  // filled where a stage returns an error: the caller hands it to set_error

inline size_t search_lds_bytes(const SearchArgs& a) {
    if (a.pair) return 2u * (size_t)pair_lds_layout(pair_qe(a), pair_re(a), a.ht_entries, a.ht_ov).half_bytes;
    if (a.pqlut) return pq_lds_layout(pq_lut_qs(a), a.ht_entries, a.ht_ov).total;
    return search_lds_layout(a.ht_entries, cmax_of(a), lds_queue_entries(a), query_lds_bytes(a.ix), a.team != 0).total;
}

// ---- sizing of the LDS visited table ---------------------------------------------------------
// The table trades occupancy (LDS per query) against probe length and the spill rate; results
// never depend on it.  Measured on MI355X (1M x 128 f32, R = 32, L = 10..250): LDS is allocated in
// 1280-byte granules (128 per CU), occupancy is capped by the kernel's VGPRs anyway (16 queries per CU
// for the 128-d f32 kernel, 24 for the integer kernels) so LDS up to that point is free, and the best
// size sits at the top of the occupancy step that holds about the 90th percentile of comparisons
// per query at 75 % load.
constexpr uint32_t kLdsGranule = 1280, kLdsGranules = 128;

inline uint32_t snap_visited_entries(SearchArgs a, uint32_t cap_ids, uint32_t useful_waves) {
    a.ht_entries = 0;
    const int64_t other = (int64_t)search_lds_bytes(a);
    uint64_t need = ((uint64_t)((double)cap_ids / 0.75) + 63) / 64 * 64;
    need = std::min<uint64_t>(std::max<uint64_t>(need, 256), 32768);
    const uint64_t granules = ((uint64_t)other + need * 4 + kLdsGranule - 1) / kLdsGranule;
    if (granules > kLdsGranules) return (uint32_t)need;
    const uint32_t waves = std::min<uint32_t>(kLdsGranules / (uint32_t)granules, useful_waves);
    int64_t top = ((int64_t)(kLdsGranules / waves) * kLdsGranule - other) / 4 / 64 * 64;
    // beyond ~8 slots per id the probe chains are already one step long; a larger table only costs its wipe
    top = std::min<int64_t>(top, ((int64_t)cap_ids * 8 + 63) / 64 * 64);
    return (uint32_t)std::min<int64_t>(std::max<int64_t>(top, (int64_t)need), 32768);
}

inline uint32_t largest_prime_leq(uint32_t n) {
    for (uint32_t c = n | 1u; c >= 3; c -= 2) {
        if (c > n) continue;
        bool prime = true;
        for (uint32_t d = 3; d * d <= c; d += 2)
            if (c % d == 0) {
                prime = false;
                break;
            }
        if (prime) return c;
    }
    return 2;
}

// ---- 16-bit table entries (SearchArgs::ht16; device side: ht16_insert_open) -----------------------------------------
// Geometry of a table of `words` dwords = `words` buckets of two 16-bit entries (any count) for ids below the index's
// slot count: m id bits; the ids of one bucket are at most ceil(2^m / words) consecutive values, told apart by tb tag
// bits; 16 - tb bits are left for the probe number (at least two: three probes = six places per id).
struct Ht16Geom {
    bool ok = false;
    uint32_t shift = 0, tb = 0, kmax = 0, slots = 0;  // slots = 2 * words: the entries the table holds
};
inline Ht16Geom ht16_geometry(uint32_t words, uint32_t nslots, uint32_t kcap = 64u) {
    Ht16Geom g;
    if (words < 32u || words > 65536u) return g;
    uint32_t m = 1;
    while (m < 32u && (1ull << m) < (uint64_t)nslots) ++m;
    if (m >= 32u) return g;
    const uint64_t per_bucket = ((1ull << m) + words - 1) / words;  // ids of one bucket: at most this many consecutive values
    uint32_t tb = 0;
    while ((1ull << tb) < per_bucket) ++tb;
    if (tb > 14u) return g;  // fewer than 2 bits for the probe number: too few probes per id
    g.tb = tb;
    g.shift = 32u - m;
    g.kmax = std::min<uint32_t>((1u << (16u - tb)) - 1u, std::max<uint32_t>(kcap, 1u));  // (kcap: DANN_DBG_HT16_MAX_PROBES)
    g.slots = words * 2u;
    g.ok = true;
    return g;
}
// Overflow table of the pair / PQ-table kernels (SearchArgs::ht_ov, ov_insert): where a 16-bit entry leaves fewer than
// eight probes per id (indexes of 2^18 slots and more at these table sizes) some percent of a search's ids find all of
// them taken (simulated at 75 % load: 75 of 2 064 ids with three probes, 5 with seven); a small table of 32-bit ids
// takes those instead of freezing the whole table at the first of them.  Words per query (a power of two).
inline uint32_t ht16_overflow_words(const Ht16Geom& g, bool pair) { return !g.ok || g.kmax >= 8u ? 0u : pair ? 128u : 256u; }
// may this launch use 16-bit entries at all?  (plain-mode kernels, one wave per query)
inline bool ht16_eligible(const SearchArgs& a) { return plain_mode(a) && !a.team; }

// probing modulus / slot count, the 16-bit geometry and the open-table limit of the table `a` has been given
inline int32_t finish_visited_table(SearchArgs& a, uint32_t open_eighths, uint32_t kcap, PlanMsg& msg) {
    if (a.ht16) {
        const Ht16Geom g = ht16_geometry(a.ht_entries, a.ix.nslots, kcap);
        if (!g.ok || !ht16_eligible(a)) {
            snprintf(msg, sizeof(msg), "internal: no 16-bit visited table of %u words for %u slots", a.ht_entries, a.ix.nslots);
            return DANN_EINTERNAL;
        }
        a.ht_prime = g.slots;
        a.ht_shift = g.shift;
        a.ht_tb = g.tb;
        a.ht_kmax = g.kmax;
        a.ht_open = (uint32_t)((uint64_t)g.slots * open_eighths / 8u);
    } else {
        a.ht_prime = largest_prime_leq(a.ht_entries);
        a.ht_open = a.ht_prime - (a.ht_prime >> 2);
    }
    return DANN_OK;
}
// ids the open table takes before it is frozen
inline uint64_t visited_open_capacity(const SearchArgs& a, uint32_t open_eighths) {
    return a.ht16 ? (uint64_t)a.ht_entries * 2u * open_eighths / 8u : (uint64_t)largest_prime_leq(a.ht_entries) * 3u / 4u;
}

// sizes the table of an automatically sized launch: the 32-bit table at the top of its occupancy step, or -- where the
// kernel has them and they buy a higher step -- 16-bit entries, also at the top of their step
inline void choose_visited_table(SearchArgs& a, uint32_t cap_ids, uint32_t useful_waves, uint32_t format, uint32_t open_eighths) {
    a.ht16 = 0;
    a.ht_entries = snap_visited_entries(a, cap_ids, useful_waves);
    if (format == 32u || !ht16_eligible(a)) return;
    auto waves_of = [&](uint32_t words) -> uint32_t {
        SearchArgs t = a;
        t.ht_entries = words;
        const uint64_t granules = (search_lds_bytes(t) + kLdsGranule - 1) / kLdsGranule;
        return granules > kLdsGranules ? 0u : std::min<uint32_t>(kLdsGranules / (uint32_t)granules, useful_waves);
    };
    // 16-bit entries the table needs so that cap_ids of them are below its open limit (open_eighths / 8 of the slots)
    const uint64_t need = std::max<uint64_t>(((uint64_t)cap_ids * 8u + open_eighths - 1u) / open_eighths, 512);
    uint32_t words = (uint32_t)std::min<uint64_t>(((need + 1) / 2 + 63) / 64 * 64, 32768);  // multiples of 64 words
    while (words < 32768u && !ht16_geometry(words, a.ix.nslots).ok) words = std::min<uint32_t>(words * 2u, 32768u);
    if (!ht16_geometry(words, a.ix.nslots).ok) return;
    const uint32_t w16 = waves_of(words), w32 = waves_of(a.ht_entries);
    // Measured (profiles/r04a_visited16_sgpr_ab_*.log): where the 32-bit table already lets a dozen and more queries
    // share a CU the search is bound by instruction issue, not by latency -- u8 rows at L = 26 went from 21 to 32
    // queries per CU for -3 % (and +4 % where the SGPR count capped the gain at 24: the 16-bit probe is a few
    // instructions longer); with few queries per CU (10 M x 128 f32 at L = 56: 11 -> 16) the extra residents pay.
    if (format != 16u && (w16 <= w32 || w32 > 12u)) return;
    if (w16 == 0 && format != 16u) return;
    // a sparser table on the same step costs nothing but its wipe (cf. snap_visited_entries)
    while (words + 64u <= 32768u && (uint64_t)(words + 64u) * 2u <= (uint64_t)cap_ids * 8u && waves_of(words + 64u) == w16 &&
           ht16_geometry(words + 64u, a.ix.nslots).ok)
        words += 64u;
    a.ht16 = 1;
    a.ht_entries = words;
}

// prior for a (L, beam) never seen on this index: comparisons per query ~= 4.3 R (L + W)^0.55 on
// Vamana graphs (about half of an expanded node's neighbours were seen before), 90th pct ~= 1.3x
inline uint32_t prior_visited_cap(const SearchArgs& a) {
    const double l = (double)(a.range_ids ? std::max<uint32_t>(a.l_value, 64) : a.l_value) + a.beam_width;
    return (uint32_t)(1.3 * 4.3 * (double)a.ix.max_degree * pow(l, 0.55)) + a.ix.nstart;
}

// which kernel family a launch with these arguments runs (include/dann_debug.h)
inline int search_family(const SearchArgs& a) {
    if (a.srv.ring) return DANN_FAMILY_SERVER;
    if (a.pair) return DANN_FAMILY_PAIR;
    if (a.pqlut) return DANN_FAMILY_PQ_LUT;
    if (a.team) return DANN_FAMILY_TEAM;
    if (a.grid) return DANN_FAMILY_PERSISTENT;
    return DANN_FAMILY_ONE_WAVE;
}

inline uint64_t calib_key(const SearchArgs& a) {
    return ((uint64_t)a.l_value << 32) | ((uint64_t)a.beam_width << 8) | (a.rec_ids ? 1u : 0u) | (a.range_ids ? 2u : 0u) |
           (a.filter_mode << 2);
}

// dann_set_max_concurrency: `max_concurrency` persistent waves share the batch through a counter in the zeroed pad words
// behind the spill pool -- never teams, pairs or the PQ table kernel: those launch one block per query (pair)
inline bool launch_capped(const SearchArgs& a, const LaunchKnobs& k) {
    return k.max_concurrency && a.nq > k.max_concurrency && plain_mode(a);
}
inline void cap_grid(SearchArgs& x, const LaunchKnobs& k) {
    const bool capped = launch_capped(x, k);
    x.grid = capped ? k.max_concurrency : 0u;
    x.work_next = capped ? x.spill_next + 8 : nullptr;
}

// ---- stage 1: the kernel family.  `inflight` is the number of wavefronts the launch keeps resident -----------------
inline void plan_family(SearchArgs& a, const LaunchKnobs& k, uint32_t inflight) {
    // latency regime with at most one query per SIMD: a team of five wavefronts per query -- queue, control, visited
    // filter, two for the row gather (search_kernel_impl.h, team_control_wave).  Knn searches and the build's insert-time
    // searches (the queue wave's pop records the visited node) only; one wave per query where no team instantiation exists.
    // Decided before the table is sized: teams carry more LDS.  DANN_DBG_TUNE_OFF bit 4 (teams) / bit 8 (speculation) /
    // DANN_DBG_TEAM_MAX_QUERIES: development switches.
    const bool will_grid = launch_capped(a, k);  // (search_with_retry sets a.grid after the plan)
    a.team = (inflight <= k.team_max_queries && !a.grid && !will_grid && !a.srv.ring && !a.range_ids && !a.qmap && plain_mode(a) &&
              a.ix.max_degree <= 63u /* an adjacency row fits one 64-lane request */ && !(k.tune_off & 4u) &&
              team_shape(a)) ? 1u : 0u;
    if (k.tune_off & 8u) a.tune |= kTuneNoSpeculation;
    if (k.tune_off & 64u) a.tune |= kTuneNoSelfStart;
    // throughput regime of 128-byte integer rows: two queries per wavefront (search_pair_impl.h).  A pair-hop is longer
    // than a hop of one query, so the pairing pays once the chip is full: measured on 1 M u8 rows at L = 26
    // (scratch/pair_latency.py, kernel us, pair / one wave per query): 4 096 queries 292 / 260, 6 144: 301 / 346,
    // 16 384: 497 / 585, 65 536: 1 423 / 1 801.  DANN_DBG_TUNE_OFF bit 16 / DANN_DBG_PAIR_MIN_QUERIES: switches.
    a.pair = 0;
    a.ht_ov = 0;
    SearchArgs t = a;
    t.team = 0;
    if (a.nq >= k.pair_min_queries && inflight >= k.pair_min_queries && !will_grid && k.visited_format != 32u && pair_shape(t) &&
        !(k.tune_off & 16u)) {
        a.pair = 1;
        a.team = 0;
    }
    // PQ rows of at most 64 chunks, plain Knn search: the lookup table in registers (search_pq_impl.h).
    // DANN_DBG_TUNE_OFF bit 32: development switch.
    a.pqlut = (!will_grid && pq_lut_shape(a) && k.visited_format != 32u && !(k.tune_off & 32u)) ? 1u : 0u;
}

// ---- stage 2: the visited table (a.ht_entries == 0: sized from the calibration, else dann_set_visited_bits) --------
// Gives `a` the largest 16-bit table of the first LDS step -- g0 granules and up, `gdiv` queries sharing a step's bytes,
// `fixed` of them taken -- whose open capacity holds `cap` (the 90th percentile of the comparisons) with a tenth to spare:
// words in multiples of `align`, at most `wcap`, more than `margin` beyond the overflow words.  false: no step fits.
inline bool fit_first_table(SearchArgs& a, const LaunchKnobs& k, uint32_t cap, uint32_t fixed, uint32_t g0, uint32_t gdiv,
                            uint32_t align, uint32_t wcap, uint32_t margin, bool pair) {
    for (uint32_t g = g0; g <= kLdsGranules; ++g) {
        const uint32_t bytes = g * kLdsGranule / gdiv;
        if (bytes <= fixed) continue;
        uint32_t w = std::min<uint32_t>((bytes - fixed) / 4u / align * align, wcap);
        const uint32_t o = ht16_overflow_words(ht16_geometry(w, a.ix.nslots, k.ht16_kcap), pair);
        if (w <= o + margin) continue;
        w -= o;
        if ((uint64_t)w * 2u * k.open_eighths / 8u >= (uint64_t)cap + cap / 10u && ht16_geometry(w, a.ix.nslots).ok &&
            ht16_overflow_words(ht16_geometry(w, a.ix.nslots, k.ht16_kcap), pair) <= o) {
            a.ht16 = 1;
            a.ht_entries = w;
            a.ht_ov = o;
            return true;
        }
    }
    return false;
}
inline uint32_t visited_cap(const SearchArgs& a, const VisitedCalib& cal) { return cal.cap_ids ? cal.cap_ids : prior_visited_cap(a); }

// cal.waves: queries per CU the registers allow.  *sized: the entries before the floor growth (the verbose line's)
inline int32_t plan_table(SearchArgs& a, const LaunchKnobs& k, const VisitedCalib& cal, uint32_t inflight, uint32_t* sized,
                          PlanMsg& msg) {
    if (a.ht_entries == 0) {
        // a launch with fewer queries than the chip has wave slots leaves LDS idle: give each query the share of a CU
        // it will actually have (a sparse table keeps the slowest lane's probe chain short -- the latency regime)
        const uint32_t per_cu = std::max<uint32_t>(1u, (inflight + k.num_cus - 1) / k.num_cus);
        const uint32_t waves = (k.tune_off & 2u) ? cal.waves : std::min<uint32_t>(cal.waves, per_cu);
        const uint32_t cap = visited_cap(a, cal);
        bool fitted = false;
        // pair: one 16-bit table per query, a step's bytes go to a wavefront = two queries; the step decides how many wavefronts
        // share a CU, and the pair kernel lives on that (profiles/r04m: 16 / 8 / 4 wavefronts per CU -> 2.09 / 2.94 / 5.27 ms)
        if (a.pair) fitted = fit_first_table(a, k, cap, pair_lds_layout(pair_qe(a), pair_re(a), 0, 0).half_bytes, 2, 2, 4, 16384, 32, true);
        // PQ table: registers cap the CU at 16 queries = 8 LDS granules each (8 / 4 queries beyond 16 / 48 chunks); the
        // table takes what is left of them (a sparse table costs nothing but its wipe), or a later step
        if (a.pqlut) fitted = fit_first_table(a, k, cap, pq_lds_layout(pq_lut_qs(a), 0, 0).total,
                                              kLdsGranules / pq_lut_waves_per_cu(a.ix.pq_chunks), 1, 64, 32768, 64, false);
        if (!fitted) {  // (no step fits: neither special kernel)
            a.pair = a.pqlut = 0;
            choose_visited_table(a, cap, waves, k.visited_format, k.open_eighths);
        }
    } else {
        // explicit size (dann_set_visited_bits): 16-bit entries only on request (dann_set_visited_format)
        a.ht16 = 0;
        if (a.pair && k.visited_format != 16u) a.pair = 0;  // (the pair kernel has 16-bit tables only)
        if ((k.visited_format == 16u || a.pqlut) && ht16_eligible(a)) {
            uint32_t words = std::max<uint32_t>((a.ht_entries + 63u) / 64u * 64u, 64u);
            while (words < 32768u && !ht16_geometry(words, a.ix.nslots).ok) words = std::min<uint32_t>(words * 2u, 32768u);
            if (ht16_geometry(words, a.ix.nslots).ok) {
                a.ht16 = 1;
                a.ht_entries = words;
                if (a.pair || a.pqlut) a.ht_ov = ht16_overflow_words(ht16_geometry(words, a.ix.nslots, k.ht16_kcap), a.pair != 0);
            }
        }
        if (a.pair && !a.ht16) a.pair = 0;
        if (a.pqlut && !a.ht16) a.pqlut = 0;
        // (the two special kernels carry their own LDS layout: a table they cannot hold goes to beam_search_kernel)
        if ((a.pair || a.pqlut) && search_lds_bytes(a) > 160 * 1024) a.pair = a.pqlut = 0;
        if (!a.pair && !a.pqlut) a.ht_ov = 0;
    }
    *sized = a.ht_entries;
    // the start points are inserted unconditionally and the first hop needs room before the freeze test can
    // trigger: the open table must hold nstart + W * R ids below its 75 % load limit, or ht_visit could probe a
    // full table forever (explicit dann_set_visited_bits sizes and small calibrated sizes are grown, never results)
    const uint64_t floor_ids = (uint64_t)a.ix.nstart + (uint64_t)a.beam_width * a.ix.max_degree + 1;
    while (a.ht_entries < 32768 && visited_open_capacity(a, k.open_eighths) <= floor_ids) a.ht_entries *= 2;
    if (visited_open_capacity(a, k.open_eighths) <= floor_ids) {
        snprintf(msg, sizeof(msg), "visited table: %u start points + beam %u x degree %u do not fit the largest LDS table",
                 a.ix.nstart, a.beam_width, a.ix.max_degree);
        return DANN_EINVAL;
    }
    // latency mode: the launch is bound by per-hop latency, not bandwidth -- rows (and, in teams, adjacency rows) of the
    // predicted next hop are requested a hop ahead.  Measured on 1 M x 128 f32, L = 26 (scratch/prefetch_ab.py, kernel
    // time with / without): 64 queries 131 / 144 us, 256: 146 / 161, 512: 164 / 175, 1024: 200 / 189, 2048: 304 / 246 --
    // from about three queries per CU on, the requests of mispredicted hops cost more than the early ones gain.
    if (inflight <= 3u * k.num_cus && !(k.tune_off & 1u)) a.tune |= kTuneRowPrefetch;
    // development switch DANN_DBG_TUNE_ON bit 1: the row prefetch in the throughput regime too (A/B on large indexes)
    if (k.tune_on & 1u) a.tune |= kTuneRowPrefetch;
    return DANN_OK;
}

// ---- stage 3: `failed` queries (in `list`) of launch `a` exhausted LDS table and spill pool: their re-run, or false = stop
inline bool plan_retry(SearchArgs& a, const LaunchKnobs& k, const uint32_t* list, uint32_t failed) {
    if (a.team) {
        a.team = 0;  // a team never spills its visited table: the same table, one wave per query (which does)
    } else {
        if (!a.pair && !a.pqlut && a.ht_entries >= 32768) return false;
        a.pair = a.pqlut = a.ht_ov = 0;  // pair / PQ table: re-runs go through beam_search_kernel, one query's table doubled
        a.ht_entries = std::min<uint32_t>(a.ht_entries * 2, 32768);
    }
    a.qmap = list;
    a.nq = failed;
    cap_grid(a, k);
    return search_lds_bytes(a) <= 160 * 1024;
}

}  // namespace
}  // namespace dann
