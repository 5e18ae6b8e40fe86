// search_kernels.hip -- the HIP side of a beam-search launch: spill pool, register query, calibration, timing, retry.
// Its decisions (kernel family, visited-table size and geometry, tuning bits, the retry step): launch_plan.h.
#include "dann_internal.h"
#include "launch_plan.h"

namespace dann {
#ifdef DANN_PHASE_CYCLES
unsigned long long* dann_phase_buffer();
#endif
namespace {

// collect the indices of queries whose status is non-zero
__global__ void collect_failed_kernel(const dann_search_stats* stats, const uint32_t* qmap, uint32_t n, uint32_t* count,
                                      uint32_t* list) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t q = qmap ? qmap[t] : t;
    if (stats[q].status) list[atomicAdd(count, 1u)] = q;
}

}  // namespace

constexpr uint32_t kHistBins = 512;

__global__ void cmps_hist_kernel(const dann_search_stats* stats, uint32_t n, uint32_t* hist) {
    __shared__ uint32_t h[kHistBins];
    for (uint32_t i = threadIdx.x; i < kHistBins; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x)
        if (!stats[t].status) atomicAdd(&h[min(stats[t].cmps / 64u, kHistBins - 1u)], 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kHistBins; i += blockDim.x)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

int32_t launch_search(const SearchArgs& a, hipStream_t stream, int* regs_out) {
    if (a.nq == 0) return DANN_OK;
    if (a.l_value == 0 || a.beam_width == 0) {
        set_error("l_value and beam_width must be non-zero (KnnSearchError, knn_search.rs:27-33)");
        return DANN_EINVAL;
    }
    if (a.beam_width > (uint32_t)kMaxBeam) {
        set_error("beam_width %u exceeds the supported maximum of %d", a.beam_width, kMaxBeam);
        return DANN_EUNSUPPORTED;
    }
    const uint32_t qcap = std::max(a.l_value + a.ix.nstart, a.qcap_max);  // the queue registers cover AdaptiveL's resize
    if (a.filter_mode == DANN_FILTER_MULTIHOP && cmax_of(a) > (uint32_t)kWave) {
        set_error("multihop filter search supports beam_width * max_degree <= 64 (got %u x %u)", a.beam_width,
                  a.ix.max_degree);
        return DANN_EUNSUPPORTED;
    }
    const size_t lds = search_lds_bytes(a);
    if (lds > 160 * 1024 && !regs_out) {
        set_error("per-query LDS footprint %zu B exceeds 160 KiB (visited table %u entries)", lds, a.ht_entries);
        return DANN_EOVERFLOW;
    }
    if (a.pqlut && !regs_out) return launch_search_pqlut(a, lds, stream);
    if (a.pair && !regs_out) return launch_search_pair(a, lds, stream);
    switch (a.ix.dtype) {
        case DT_F32: return launch_search_f32(a, qcap, lds, stream, regs_out);
        case DT_F16: return launch_search_f16(a, qcap, lds, stream, regs_out);
        case DT_U8: return launch_search_u8(a, qcap, lds, stream, regs_out);
        case DT_I8: return launch_search_i8(a, qcap, lds, stream, regs_out);
        case DT_SQ8: return launch_search_sq8(a, qcap, lds, stream, regs_out);
        case DT_SQ4: return launch_search_sq4(a, qcap, lds, stream, regs_out);
        case DT_SQ1: return launch_search_sq1(a, qcap, lds, stream, regs_out);
        case DT_SPH1: return launch_search_sph1(a, qcap, lds, stream, regs_out);
        case DT_SPH1T: return launch_search_sph1t(a, qcap, lds, stream, regs_out);
        case DT_SPH2: return launch_search_sph2(a, qcap, lds, stream, regs_out);
        case DT_SPH4: return launch_search_sph4(a, qcap, lds, stream, regs_out);
        case DT_MM1: return launch_search_mm1(a, qcap, lds, stream, regs_out);
        case DT_MM2: return launch_search_mm2(a, qcap, lds, stream, regs_out);
        case DT_MM4: return launch_search_mm4(a, qcap, lds, stream, regs_out);
        case DT_MM8: return launch_search_mm8(a, qcap, lds, stream, regs_out);
        case DT_MM1Q: return launch_search_mm1q(a, qcap, lds, stream, regs_out);
        case DT_MM2Q: return launch_search_mm2q(a, qcap, lds, stream, regs_out);
        case DT_MM4Q: return launch_search_mm4q(a, qcap, lds, stream, regs_out);
        case DT_PQ: return launch_search_pq(a, qcap, lds, stream, regs_out);
    }
    set_error("bad dtype %d", a.ix.dtype);
    return DANN_EINVAL;
}

#ifdef DANN_PHASE_CYCLES
static unsigned long long* g_phase_buf = nullptr;  // debug builds: per-phase cycle sums (SearchArgs::phase_cycles)
unsigned long long* dann_phase_buffer() {
    if (!g_phase_buf) {
        if (hipMalloc((void**)&g_phase_buf, 128) != hipSuccess) return nullptr;
        (void)hipMemset(g_phase_buf, 0, 128);
    }
    return g_phase_buf;
}
extern "C" int32_t dann_debug_phase_cycles(unsigned long long* out, int reset) try {
    unsigned long long* b = dann_phase_buffer();
    if (!b) return DANN_EHIP;
    if (out) (void)hipMemcpy(out, b, 128, hipMemcpyDeviceToHost);
    if (reset) (void)hipMemset(b, 0, 128);
    return 0;
} DANN_CATCH_ALL
#endif

// the planner's per-index inputs (launch_plan.h), read once per call
static LaunchKnobs launch_knobs(const dann_index* idx) {
    return {idx->num_cus, idx->max_concurrency, idx->visited_format, idx->dbg_u32(DANN_DBG_TUNE_OFF, 0u), idx->dbg_u32(DANN_DBG_TUNE_ON, 0u),
            idx->dbg_u32(DANN_DBG_TEAM_MAX_QUERIES, 4u * idx->num_cus), idx->dbg_u32(DANN_DBG_PAIR_MIN_QUERIES, 20u * idx->num_cus),
            std::min(64u, std::max(1u, idx->dbg_u32(DANN_DBG_HT16_MAX_PROBES, 64u))),
            std::min(7u, std::max(4u, idx->dbg_u32(DANN_DBG_HT16_OPEN_EIGHTHS, 6u)))};
}
static int32_t plan_failed(int32_t rc, const PlanMsg& msg) {
    if (rc != DANN_OK) set_error("%s", msg);
    return rc;
}

// everything a beam-search launch needs besides its arguments: the context's spill pool (zeroed counters), the size of
// the LDS visited table (calibrated per (L, beam, mode), never affects results) and the tuning bits.  `inflight` is the
// number of wavefronts the launch keeps resident.  zero_pool = false leaves the pool's counters to the caller
// (search_with_retry: a scheduled launch has them cleared by the scheduler's first kernel).
static int32_t prepare_launch(dann_index* idx, SearchCtx& ctx, SearchArgs& a, const LaunchKnobs& k, uint32_t inflight,
                              bool zero_pool = true) {
    hipStream_t st = ctx.stream;
    // failure flag in pinned host memory: written over the fabric only by a query that
    // overflows (rare), read by the host after the stream sync -- no memset / D2H copy
    if (!ctx.d_spill) {  // 512 spill tables of 2^14 ids (32 MiB), cleaned and released by their users
        const uint32_t slices = 512, sbits = 14;
        // tables | counter (+pad) | busy flags | cmps histogram
        const size_t words = ((size_t)slices << sbits) + 16 + slices + kHistBins;
        DANN_HIP(hipMalloc((void**)&ctx.d_spill, words * 4));
        DANN_HIP(hipMemsetAsync(ctx.d_spill, 0xFF, words * 4, st));
        ctx.spill_slices = slices;
        ctx.spill_bits = sbits;
    }
    a.spill = ctx.d_spill;
    a.spill_slices = ctx.spill_slices;
    a.spill_bits = ctx.spill_bits;
    a.spill_next = ctx.d_spill + ((size_t)ctx.spill_slices << ctx.spill_bits);
    plan_family(a, k, inflight);
    // the pool's allocation counter and busy flags start every launch at zero -- except a team launch, which never
    // touches the pool (a team gives a query that outgrows its table back to the host): one device operation less on
    // the single-query path
    if (!a.team && zero_pool) DANN_HIP(hipMemsetAsync(a.spill_next, 0, (16 + (size_t)ctx.spill_slices) * 4, st));
    // calibration state of this (L, beam, mode) -- shared by concurrent callers: read and written under stat_mu
    VisitedCalib cal;
    const bool autosize = a.ht_entries == 0;
    if (autosize) {
        const uint64_t key = calib_key(a);
        {
            std::lock_guard<std::mutex> lk(idx->stat_mu);
            cal = idx->calib[key];
        }
        if (a.pqlut) cal.waves = pq_lut_waves_per_cu(a.ix.pq_chunks);  // (what pq_search_kernel's table size is compiled for)
        if (!cal.waves) {  // queries per CU the registers of this instantiation allow (512 VGPRs per SIMD lane)
            int regs = 0;
            a.ht_entries = 256;
            int32_t qrc = launch_search(a, st, &regs);
            a.ht_entries = 0;
            if (qrc != DANN_OK) return qrc;
            const uint32_t per_simd = regs > 0 ? 512u / (((uint32_t)regs + 7u) & ~7u) : 4u;
            cal.waves = 4u * std::min<uint32_t>(std::max<uint32_t>(per_simd, 1u), 8u);
            {
                std::lock_guard<std::mutex> lk(idx->stat_mu);
                idx->calib[key].waves = cal.waves;
            }
            if (idx->verbose()) fprintf(stderr, "[dann] search kernel: %d VGPRs -> %u queries per CU\n", regs, cal.waves);
        }
    }
    uint32_t sized = 0;  // (the table before its growth to the floor of nstart + W * R + 1 ids: what the line below reports)
    PlanMsg msg;
    const int32_t prc = plan_table(a, k, cal, inflight, &sized, msg);
    if (autosize && idx->verbose() && (cal.calls & (cal.calls - 1)) == 0) {
        SearchArgs t = a;
        t.ht_entries = sized;
        fprintf(stderr, "[dann] L=%u W=%u: visited cap %u (%s) -> %u %s, %zu B LDS\n", a.l_value, a.beam_width,
                visited_cap(a, cal), cal.cap_ids ? "p90" : "prior", a.ht16 ? sized * 2u : sized,
                a.pair ? "16-bit slots per query, two queries per wavefront" : a.pqlut ? "16-bit slots, PQ table in registers" : a.ht16 ? "16-bit slots" : "entries",
                search_lds_bytes(t));
    }
    return plan_failed(prc, msg);
}

// the persistent server of dann_server_start: sized like a launch that keeps `workers` searches in flight, enqueued on
// the context's stream, not waited for
int32_t launch_search_server(dann_index* idx, SearchCtx& ctx, SearchArgs a) {
    if (!plain_mode(a)) {
        set_error("the search server runs the plain Knn search (beam width 1, no inline tags, degree <= 64)");
        return DANN_EUNSUPPORTED;
    }
    a.nq = a.srv.workers;
    const LaunchKnobs k = launch_knobs(idx);
    int32_t rc = prepare_launch(idx, ctx, a, k, a.srv.workers);
    if (rc != DANN_OK) return rc;
    a.fail_flag = nullptr;
    PlanMsg msg;
    if (int32_t frc = plan_failed(finish_visited_table(a, k.open_eighths, k.ht16_kcap, msg), msg)) return frc;
    rc = launch_search(a, ctx.stream);
    if (rc == DANN_OK) {
        std::lock_guard<std::mutex> lk(idx->stat_mu);
        idx->families[DANN_FAMILY_SERVER].launches += 1;
    }
    return rc;
}

int32_t search_with_retry(dann_index* idx, SearchCtx& ctx, SearchArgs a) {
    hipStream_t st = ctx.stream;
    if (a.nq == 0) return DANN_OK;
    if (ctx.fail_cap < a.nq || !ctx.d_fail) {
        if (ctx.d_fail) (void)hipFree(ctx.d_fail);
        ctx.d_fail = nullptr;
        ctx.fail_cap = 0;
        DANN_HIP(hipMalloc((void**)&ctx.d_fail, (2 * (size_t)a.nq + 4) * 4));
        ctx.fail_cap = a.nq;
    }
    uint32_t* count = ctx.d_fail;
    uint32_t* lists[2] = {ctx.d_fail + 4, ctx.d_fail + 4 + ctx.fail_cap};
    const LaunchKnobs k = launch_knobs(idx);
    const uint32_t inflight = launch_capped(a, k) ? k.max_concurrency : a.nq;
    const bool autosize = a.ht_entries == 0;
    const uint64_t key = calib_key(a);
    if (int32_t prc = prepare_launch(idx, ctx, a, k, inflight, false)) return prc;
    const uint32_t pool_words = a.team ? 0u : 16u + ctx.spill_slices;  // (the counters this launch starts from zero)
    cap_grid(a, k);  // (the counter lives behind the spill pool prepare_launch has just attached)
    if (a.grid) a.team = 0;  // persistent waves over a block: one wave per query
    // locality scheduling (query_schedule.hip): a large Knn launch of f32 / f16 rows runs its queries grouped by nearest
    // pivot, each XCD a contiguous run of the groups (persistent waves: the groups in order), through a slot map of its
    // own -- told apart from a caller's or the retry's map by `caller_qmap`.  DANN_DBG_TUNE_OFF bit 128 /
    // DANN_DBG_SCHED_MIN_QUERIES: development switches.
    const uint32_t* const caller_qmap = a.qmap;
    const uint32_t sched_min = idx->dbg_u32(DANN_DBG_SCHED_MIN_QUERIES, 16384u);
    bool pool_zeroed = false;
    if (a.nq >= sched_min) {
        const bool sched = !a.qmap && a.queries && !a.qslots && !a.rec_ids && !a.range_ids && !a.srv.ring && !a.team &&
                           !a.pair && !a.pqlut && a.filter_mode == 0 && (a.ix.dtype == DT_F32 || a.ix.dtype == DT_F16) &&
                           sched_pivot_count(a.ix.dim) >= 32u && !idx->tune_off(128);
        if (sched) {
            const size_t words = (size_t)a.nq + sched_scratch_words(a.ix.dim, a.nq);
            if (ctx.sched_words < words) {
                if (ctx.d_sched) (void)hipFree(ctx.d_sched);
                ctx.d_sched = nullptr;
                ctx.sched_words = 0;
                DANN_HIP(hipMalloc((void**)&ctx.d_sched, words * 4));
                ctx.sched_words = words;
            }
            {
                std::lock_guard<std::mutex> lk(idx->sched_mu);
                if (!idx->d_sched_piv || idx->sched_stale) {
                    if (int32_t brc = sched_build_pivots(idx, st)) return brc;
                    idx->sched_stale = false;
                }
            }
            if (int32_t mrc = sched_build_map(idx, st, a.queries, a.nq, a.grid ? 1u : 8u, ctx.d_sched + a.nq, ctx.d_sched,
                                              a.spill_next, pool_words))
                return mrc;
            a.qmap = ctx.d_sched;
            pool_zeroed = true;
        }
        if (idx->verbose())
            fprintf(stderr, "[dann] schedule: %u queries %s\n", a.nq,
                    sched ? (a.grid ? "sorted by nearest pivot (persistent waves)" : "sorted by nearest pivot, 8 XCD runs")
                          : "in caller order");
    }
    if (pool_words && !pool_zeroed) DANN_HIP(hipMemsetAsync(a.spill_next, 0, (size_t)pool_words * 4, st));
    volatile uint32_t* hflag = ctx.h_flag;
    *hflag = 0;
    a.fail_flag = ctx.h_flag;
    // HIP events bracket exactly the beam-search launches, on the stream they run on
    float last_ms = 0.f;
    auto timed_launch = [&](SearchArgs& args) -> int32_t {
        PlanMsg msg;
        if (int32_t frc = plan_failed(finish_visited_table(args, k.open_eighths, k.ht16_kcap, msg), msg)) return frc;
#ifdef DANN_PHASE_CYCLES
        args.phase_cycles = dann_phase_buffer();
#endif
        float ms = 0.f;
        constexpr uint32_t kUntimedLaunchQueries = 2048;  // (a launch of that many queries lasts 150-300 us)
        // a Knn call of a few queries is a latency measurement of its caller's: the two event records and the elapsed-time
        // query around it are 4-5 us of ~90 (16 callers sharing launches: 103 k -> 107 k calls/s; a 1 024-query batch: 3 % of its 170 us) -- it is waited for with a
        // plain stream synchronisation and counted with 0 ms unless DANN_DBG_TIME_SMALL_LAUNCHES asks for the events
        const bool timed = args.nq > kUntimedLaunchQueries || args.rec_ids || args.qslots || args.range_ids ||
                           idx->dbg_u32(DANN_DBG_TIME_SMALL_LAUNCHES, 0u) != 0u;
        if (timed) DANN_HIP(hipEventRecord(ctx.ev0, st));
        int32_t r = launch_search(args, st);
        if (r != DANN_OK) return r;
        if (timed) {
            DANN_HIP(hipEventRecord(ctx.ev1, st));
            DANN_HIP(hipEventSynchronize(ctx.ev1));
            DANN_HIP(hipEventElapsedTime(&ms, ctx.ev0, ctx.ev1));
        } else {
            DANN_HIP(hipStreamSynchronize(st));
        }
        last_ms = ms;
        std::lock_guard<std::mutex> lk(idx->stat_mu);
        idx->clocks[0].total_ms += ms;
        KernelClock& fam = idx->families[search_family(args)];
        fam.total_ms += ms;
        fam.launches += 1;
        return DANN_OK;
    };
    int32_t rc = timed_launch(a);
    if (rc != DANN_OK) return rc;
    {
        std::lock_guard<std::mutex> lk(idx->stat_mu);
        idx->clocks[0].launches += 1;  // one logical search = one "launch" (+ rare retry launches, time included)
    }
    // recalibrate on calls 1, 2, 4, 8, ... of this key (a 512-bin histogram of cmps, 2 KiB D2H)
    if (autosize && a.stats && !caller_qmap && !a.range_ids && a.nq >= 256) {
        uint64_t calls;
        {
            std::lock_guard<std::mutex> lk(idx->stat_mu);
            calls = ++idx->calib[key].calls;
        }
        // insert-time searches run on a growing graph (comparisons grow with it): recalibrate on every batch
        if ((calls & (calls - 1)) == 0 || a.rec_ids) {
            uint32_t* d_hist = a.spill_next + 16 + ctx.spill_slices;
            DANN_HIP(hipMemsetAsync(d_hist, 0, kHistBins * 4, st));
            hipLaunchKernelGGL(cmps_hist_kernel, dim3(std::min<uint32_t>((a.nq + 255) / 256, 256)), dim3(256), 0, st,
                               a.stats, a.nq, d_hist);
            uint32_t hist[kHistBins];
            DANN_HIP(hipMemcpyAsync(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost, st));
            DANN_HIP(hipStreamSynchronize(st));
            uint64_t total = 0, acc = 0;
            for (uint32_t b = 0; b < kHistBins; ++b) total += hist[b];
            for (uint32_t b = 0; b < kHistBins && total; ++b) {
                acc += hist[b];
                if (acc * 10 >= total * 9) {
                    std::lock_guard<std::mutex> lk(idx->stat_mu);
                    idx->calib[key].cap_ids = (b + 1) * 64;
                    break;
                }
            }
        }
    }
    if (!*hflag || !a.stats) return DANN_OK;
    // rare path: queries that exhausted LDS table + spill pool are re-run with a larger LDS table
    a.qmap = caller_qmap;  // (a scheduled launch ran every query once: its retries go unscheduled)
    for (int round = 0;; ++round) {
        DANN_HIP(hipMemsetAsync(count, 0, 4, st));
        hipLaunchKernelGGL(collect_failed_kernel, dim3((a.nq + 255) / 256), dim3(256), 0, st, a.stats, a.qmap, a.nq, count,
                           lists[round & 1]);
        uint32_t h = 0;
        DANN_HIP(hipMemcpyAsync(&h, count, 4, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
        if (h == 0 || !plan_retry(a, k, lists[round & 1], h)) return DANN_OK;  // (stop: callers see the per-query status)
        DANN_HIP(hipMemsetAsync(a.spill_next, 0, (16 + (size_t)ctx.spill_slices) * 4, st));
        *hflag = 0;
        rc = timed_launch(a);
        if (rc != DANN_OK) return rc;
        std::lock_guard<std::mutex> lk(idx->stat_mu);
        idx->clocks[4].total_ms += last_ms;
        idx->clocks[4].launches += h;
    }
}

}  // namespace dann
