// host_search.hip -- dann_search_batch: Knn searches with queries and results in host memory.  plan_host_search
// (host_plan.h) picks the way the bytes travel; each way is one function here.
#include <string.h>

#include <chrono>
#include <map>
#include <memory>

#include "dann_internal.h"
#include "host_plan.h"

using namespace dann;

namespace {
constexpr uint32_t kHostChunk = 16384;  // queries per chunk of the lanes

struct HostArgs {  // one dann_search_batch call
    dann_index* idx;
    const void* queries;
    uint32_t nq, l_value, beam, k;
    uint32_t* out_ids;
    float* out_dists;
    dann_search_stats* out_stats;
    size_t qb;  // bytes per query
};

int32_t first_failed_query(const dann_search_stats* stats, uint32_t nq, uint32_t base) {
    for (uint32_t i = 0; i < nq; ++i) {
        if (stats[i].status == (uint32_t)(-DANN_EINVAL)) {
            set_error("query %u: could not retrieve start point (a start slot is not readable)", base + i);
            return DANN_EINVAL;
        }
        if (stats[i].status) {
            set_error("query %u: per-query scratch exhausted (visited table and spill pool); raise the table "
                      "size with dann_set_visited_bits", base + i);
            return DANN_EOVERFLOW;
        }
    }
    return DANN_OK;
}

// the error text of this thread (set_error is thread-local), for handing to another
void grab_error_text(std::string& t) {
    char buf[512] = {0};
    dann_last_error(buf, sizeof buf);
    t = buf;
}

// the context's pinned host staging: page-locked and device-mapped, at least `bytes` (grow-only)
int32_t ensure_host_stage(SearchCtx& ctx, size_t bytes) {
    if (ctx.h_stage_bytes >= bytes) return DANN_OK;
    if (ctx.h_stage) (void)hipHostFree(ctx.h_stage);
    ctx.h_stage = nullptr;
    ctx.h_stage_bytes = 0;
    DANN_HIP(hipHostMalloc(&ctx.h_stage, bytes, hipHostMallocMapped));
    ctx.h_stage_bytes = bytes;
    return DANN_OK;
}

// ---- Small: one launch for `n` waiting calls (same L, beam, k; `total` queries; the queue and the leadership:
// small_calls.h).  kSmallCallDeclined if the staging cannot be mapped: the calls then take Single one by one.
int32_t small_batch_run(dann_index* idx, SmallCall* const* calls, uint32_t n, uint32_t total, size_t qb) {
    CtxLease lease(idx);
    if (lease.status != DANN_OK) return lease.status;
    SearchCtx& ctx = *lease.ctx;
    if (int32_t rc = ensure_host_stage(ctx, kSmallStage)) return rc;
    void* dbase = nullptr;
    if (hipHostGetDevicePointer(&dbase, ctx.h_stage, 0) != hipSuccess) {
        // (a block another path of this context allocated without the mapping: once more, mapped)
        (void)hipGetLastError();
        ctx.h_stage_bytes = 0;
        if (int32_t rc = ensure_host_stage(ctx, kSmallStage)) return rc;
        if (hipHostGetDevicePointer(&dbase, ctx.h_stage, 0) != hipSuccess) {
            (void)hipGetLastError();
            return kSmallCallDeclined;
        }
    }
    const uint32_t k = calls[0]->k;
    const size_t in_b = ((size_t)total * qb + 15) & ~(size_t)15, ids_b = ((size_t)total * k * 4 + 15) & ~(size_t)15;
    uint8_t* const h = reinterpret_cast<uint8_t*>(ctx.h_stage);
    uint8_t* const d = reinterpret_cast<uint8_t*>(dbase);
    size_t off = 0;
    for (uint32_t c = 0; c < n; ++c) {
        memcpy(h + off, calls[c]->queries, (size_t)calls[c]->nq * qb);
        off += (size_t)calls[c]->nq * qb;
    }
    // row types whose kernels read a query more than once get the queries in device memory (one copy for the group);
    // the results still land in the mapped block
    const void* dq = d;
    if (!zero_copy_rows(idx->cfg.dtype)) {
        if (int32_t grc = grow_stage(ctx, 0, in_b + 16)) return grc;
        DANN_HIP(hipMemcpyAsync(ctx.stage[0], h, (size_t)total * qb, hipMemcpyHostToDevice, ctx.stream));
        dq = ctx.stage[0];
    }
    int32_t rc = search_device(idx, ctx, dq, nullptr, total, calls[0]->l_value, calls[0]->beam, k,
                               reinterpret_cast<uint32_t*>(d + in_b), reinterpret_cast<float*>(d + in_b + ids_b),
                               reinterpret_cast<dann_search_stats*>(d + in_b + 2 * ids_b), nullptr, nullptr, 0, nullptr);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipStreamSynchronize(ctx.stream));
    const uint32_t* ri = reinterpret_cast<const uint32_t*>(h + in_b);
    const float* rd = reinterpret_cast<const float*>(h + in_b + ids_b);
    const dann_search_stats* rs = reinterpret_cast<const dann_search_stats*>(h + in_b + 2 * ids_b);
    uint32_t q0 = 0;
    for (uint32_t c = 0; c < n; ++c) {
        SmallCall& r = *calls[c];
        memcpy(r.out_ids, ri + (size_t)q0 * k, (size_t)r.nq * k * 4);
        memcpy(r.out_dists, rd + (size_t)q0 * k, (size_t)r.nq * k * 4);
        if (r.out_stats) memcpy(r.out_stats, rs + q0, (size_t)r.nq * sizeof(dann_search_stats));
        r.rc = first_failed_query(rs + q0, r.nq, 0);
        if (r.rc != DANN_OK) grab_error_text(r.text);
        q0 += r.nq;
    }
    return DANN_OK;
}

// Temporary page-locking of a caller's pageable buffer (hipHostRegister, mapped): the first registration of a range
// costs ~65 us per MB on this runtime, registering it again ~1 us (scratch/probe_host_register.hip) -- a caller that
// reuses its buffers, as a serving loop does, gets the zero-copy launch from its second call on.  Threads may pass one
// buffer at the same time: registrations are counted in a process-wide table, the last user unregisters.
struct TempPins {
    std::mutex mu;
    std::map<const void*, std::pair<size_t, uint32_t>> live;  // base -> (bytes, users)
    bool acquire(const void* p, size_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it != live.end()) {
            if (it->second.first < bytes) return false;  // (registered shorter by another caller: not worth untangling)
            ++it->second.second;
            return true;
        }
        if (hipHostRegister(const_cast<void*>(p), bytes, hipHostRegisterMapped) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        live.emplace(p, std::make_pair(bytes, 1u));
        return true;
    }
    void release(const void* p) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it == live.end()) return;
        if (--it->second.second == 0) {
            (void)hipHostUnregister(const_cast<void*>(p));
            live.erase(it);
        }
    }
    // is [p, p + bytes) host memory the CALLER page-locked (hipHostMalloc / hipHostRegister), not another thread's
    // temporary registration?  Decided under the table's lock: a release elsewhere unregisters and erases inside it.
    bool caller_pinned(const void* p, size_t bytes) {
        std::lock_guard<std::mutex> lk(mu);
        if (!p || !bytes || live.count(p)) return false;
        hipPointerAttribute_t at;
        for (const void* q : {p, (const void*)(reinterpret_cast<const uint8_t*>(p) + bytes - 1)}) {
            if (hipPointerGetAttributes(&at, q) != hipSuccess) {
                (void)hipGetLastError();  // (a pageable pointer is an "invalid value" to the runtime: not an error of this call)
                return false;
            }
            if (at.type != hipMemoryTypeHost) return false;
        }
        return true;
    }
};
TempPins& temp_pins() {
    static TempPins t;
    return t;
}
// the temporary registrations of one call, released when it goes out of scope
struct PinScope {
    const void* held[4] = {nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    bool add(const void* p, size_t bytes) {
        if (!temp_pins().acquire(p, bytes)) return false;
        held[n++] = p;
        return true;
    }
    ~PinScope() {
        for (int i = 0; i < n; ++i) temp_pins().release(held[i]);
    }
};

// Buffers this index has been handed before (same pointers, same batch) are page-locked for the call; true if all of
// them are now.  If re-registering a range turns out expensive here, the runtime does not keep ranges warm: never again.
bool register_seen_buffers(const HostArgs& a, const HostPlanIn& in, PinScope& pins) {
    uint32_t registered_before = 0;
    bool seen = false;
    {
        std::lock_guard<std::mutex> lk(a.idx->stat_mu);
        const dann_index::HostCall key{a.queries, a.out_ids, a.out_dists, a.nq, 0};
        for (auto& h : a.idx->host_calls)
            if (h == key) {
                seen = true;
                registered_before = h.registered++;
            }
        if (!seen) a.idx->host_calls[a.idx->host_calls_next++ % 8u] = key;
    }
    if (!seen) return false;
    const size_t o_bytes = (size_t)a.nq * a.k * 4;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = (in.q_pinned || pins.add(a.queries, (size_t)a.nq * a.qb)) && (in.ids_pinned || pins.add(a.out_ids, o_bytes)) &&
                    (in.dists_pinned || pins.add(a.out_dists, o_bytes)) &&
                    (in.stats_pinned || pins.add(a.out_stats, (size_t)a.nq * sizeof(dann_search_stats)));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (registered_before >= 1 && ms > 1.0) a.idx->host_register_pays.store(false, std::memory_order_relaxed);
    return ok;
}

// ---- Single: copy in, search, copy out -- through the context's pinned ring (copies from / to pageable memory are
// neither asynchronous nor fast on ROCm 7.2), or with hipMemcpyAsync from / to the caller's buffers
int32_t search_host_single(const HostArgs& a, SearchCtx& ctx, const HostPlan& p) {
    if (int32_t rc = grow_stage(ctx, 0, p.in_b + 16)) return rc;  // [0] queries, [1] ids | dists | stats
    if (int32_t rc = grow_stage(ctx, 1, p.out_b + 16)) return rc;
    if (p.ring)
        if (int32_t rc = ensure_host_stage(ctx, kRingBytes)) return rc;
    uint8_t* const ob = reinterpret_cast<uint8_t*>(ctx.stage[1]);
    uint8_t* const hs = p.ring ? reinterpret_cast<uint8_t*>(ctx.h_stage) : nullptr;
    const size_t res_b = (size_t)a.nq * a.k * 4, st_b = (size_t)a.nq * sizeof(dann_search_stats);
    std::vector<dann_search_stats> stats(a.nq);
    if (hs) memcpy(hs, a.queries, p.in_b);
    DANN_HIP(hipMemcpyAsync(ctx.stage[0], hs ? hs : a.queries, p.in_b, hipMemcpyHostToDevice, ctx.stream));
    int32_t rc = search_device(a.idx, ctx, ctx.stage[0], nullptr, a.nq, a.l_value, a.beam, a.k, reinterpret_cast<uint32_t*>(ob),
                               reinterpret_cast<float*>(ob + p.ids_b), reinterpret_cast<dann_search_stats*>(ob + 2 * p.ids_b),
                               nullptr, nullptr, 0, nullptr);
    if (rc != DANN_OK) return rc;
    if (hs) {
        DANN_HIP(hipMemcpyAsync(hs + p.in_b, ob, p.out_b, hipMemcpyDeviceToHost, ctx.stream));
    } else {
        DANN_HIP(hipMemcpyAsync(a.out_ids, ob, res_b, hipMemcpyDeviceToHost, ctx.stream));
        DANN_HIP(hipMemcpyAsync(a.out_dists, ob + p.ids_b, res_b, hipMemcpyDeviceToHost, ctx.stream));
        DANN_HIP(hipMemcpyAsync(stats.data(), ob + 2 * p.ids_b, st_b, hipMemcpyDeviceToHost, ctx.stream));
    }
    DANN_HIP(hipStreamSynchronize(ctx.stream));
    if (hs) {
        memcpy(a.out_ids, hs + p.in_b, res_b);
        memcpy(a.out_dists, hs + p.in_b + p.ids_b, res_b);
        memcpy(stats.data(), hs + p.in_b + 2 * p.ids_b, st_b);
    }
    if (a.out_stats) memcpy(a.out_stats, stats.data(), st_b);
    return first_failed_query(stats.data(), a.nq, 0);
}

// the device addresses of page-locked caller buffers (queries, ids, distances, statistics -- null without); false if
// one was registered without hipHostRegisterMapped
bool device_pointers(const HostArgs& a, void* d[4]) {
    if (hipHostGetDevicePointer(&d[0], const_cast<void*>(a.queries), 0) == hipSuccess &&
        hipHostGetDevicePointer(&d[1], a.out_ids, 0) == hipSuccess && hipHostGetDevicePointer(&d[2], a.out_dists, 0) == hipSuccess &&
        (!a.out_stats || hipHostGetDevicePointer(&d[3], a.out_stats, 0) == hipSuccess))
        return true;
    (void)hipGetLastError();
    return false;
}

// ---- ZeroCopy: the search kernel reads the queries (once each, when its wavefront stages them) and writes the results
// through the mapping -- one launch for the whole batch, where the lanes lose the drain of every chunk's last queries
int32_t search_host_zero_copy(const HostArgs& a, SearchCtx& ctx, void* d[4]) {
    const size_t st_b = (size_t)a.nq * sizeof(dann_search_stats);
    if (!d[3]) {  // statistics the caller did not ask for: the call's status is still read from them
        if (int32_t rc = grow_stage(ctx, 1, st_b + 16)) return rc;
        d[3] = ctx.stage[1];
    }
    int32_t rc = search_device(a.idx, ctx, d[0], nullptr, a.nq, a.l_value, a.beam, a.k, static_cast<uint32_t*>(d[1]),
                               static_cast<float*>(d[2]), static_cast<dann_search_stats*>(d[3]), nullptr, nullptr, 0, nullptr);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipStreamSynchronize(ctx.stream));
    if (a.out_stats) return first_failed_query(a.out_stats, a.nq, 0);
    std::vector<dann_search_stats> hstats(a.nq);
    DANN_HIP(hipMemcpy(hstats.data(), d[3], st_b, hipMemcpyDeviceToHost));
    return first_failed_query(hstats.data(), a.nq, 0);
}

// ---- Lanes: the calling thread and helpers, each with a search context (stream, device staging, pinned ring) of its
// own, take the chunks round robin and run copy in, kernel, copy out of a chunk back to back on their stream; while
// one lane's kernel drains or its thread copies through the ring, another lane's kernel has the chip.  Buffers the
// caller page-locked need no ring: the DMA reads and writes them directly.
struct Lane {
    int32_t rc = DANN_OK;      // a call-level failure (HIP, arguments)
    int32_t failed = DANN_OK;  // the first failed query of this lane's chunks
    uint32_t failed_chunk = ~0u;
    std::string text;          // error text of whichever comes first (set_error is thread-local)
};
struct LaneJob {
    const HostArgs& a;
    const HostPlan& p;
    uint32_t nchunks, step;  // lane t takes chunks t, t + step, ...
};

int32_t run_lane(const LaneJob& j, SearchCtx& lc, uint32_t first, Lane& ln) {
    const HostArgs& a = j.a;
    const HostPlan& p = j.p;
    if (int32_t rc = grow_stage(lc, 0, p.in_b + 16)) return rc;
    if (int32_t rc = grow_stage(lc, 1, p.out_b + 16)) return rc;
    if (int32_t rc = ensure_host_stage(lc, p.in_b + p.out_b)) return rc;
    uint8_t* const h_in = reinterpret_cast<uint8_t*>(lc.h_stage);
    uint8_t* const h_out = h_in + p.in_b;
    uint8_t* const ob = reinterpret_cast<uint8_t*>(lc.stage[1]);
    for (uint32_t c = first; c < j.nchunks; c += j.step) {
        const uint32_t n = std::min(p.cq, a.nq - c * p.cq);
        const uint8_t* src = reinterpret_cast<const uint8_t*>(a.queries) + (size_t)c * p.cq * a.qb;
        if (!p.q_direct) {
            memcpy(h_in, src, (size_t)n * a.qb);
            src = h_in;
        }
        DANN_HIP(hipMemcpyAsync(lc.stage[0], src, (size_t)n * a.qb, hipMemcpyHostToDevice, lc.stream));
        int32_t rc = search_device(a.idx, lc, lc.stage[0], nullptr, n, a.l_value, a.beam, a.k, reinterpret_cast<uint32_t*>(ob),
                                   reinterpret_cast<float*>(ob + p.ids_b), reinterpret_cast<dann_search_stats*>(ob + 2 * p.ids_b),
                                   nullptr, nullptr, 0, nullptr);
        if (rc != DANN_OK) return rc;
        uint32_t* const out_ids = a.out_ids + (size_t)c * p.cq * a.k;
        float* const out_dists = a.out_dists + (size_t)c * p.cq * a.k;
        if (p.o_direct) {  // (the statuses always pass through the ring: the call's return value is read from them)
            DANN_HIP(hipMemcpyAsync(out_ids, ob, (size_t)n * a.k * 4, hipMemcpyDeviceToHost, lc.stream));
            DANN_HIP(hipMemcpyAsync(out_dists, ob + p.ids_b, (size_t)n * a.k * 4, hipMemcpyDeviceToHost, lc.stream));
            DANN_HIP(hipMemcpyAsync(h_out + 2 * p.ids_b, ob + 2 * p.ids_b, (size_t)n * sizeof(dann_search_stats),
                                    hipMemcpyDeviceToHost, lc.stream));
        } else {
            DANN_HIP(hipMemcpyAsync(h_out, ob, p.out_b, hipMemcpyDeviceToHost, lc.stream));
        }
        DANN_HIP(hipStreamSynchronize(lc.stream));
        const dann_search_stats* st = reinterpret_cast<const dann_search_stats*>(h_out + 2 * p.ids_b);
        if (!p.o_direct) {
            memcpy(out_ids, h_out, (size_t)n * a.k * 4);
            memcpy(out_dists, h_out + p.ids_b, (size_t)n * a.k * 4);
        }
        if (a.out_stats) memcpy(a.out_stats + (size_t)c * p.cq, st, (size_t)n * sizeof(dann_search_stats));
        if (ln.failed == DANN_OK && (ln.failed = first_failed_query(st, n, c * p.cq)) != DANN_OK) {
            ln.failed_chunk = c;
            grab_error_text(ln.text);
        }
    }
    return DANN_OK;
}

int32_t search_host_lanes(const HostArgs& a, SearchCtx& ctx, const HostPlan& p) {
    int dev = 0;
    DANN_HIP(hipGetDevice(&dev));
    // helper lanes take a context only if one is free or may still be created: sixteen callers all waiting for a second
    // context would wait for one another
    std::unique_ptr<CtxLease> extra[kMaxLanes - 1];
    uint32_t lanes = 1;
    for (; lanes < p.lanes; ++lanes) {
        extra[lanes - 1].reset(new CtxLease(a.idx, /*try_only=*/true));
        if (extra[lanes - 1]->status != DANN_OK || !extra[lanes - 1]->ctx) {
            extra[lanes - 1].reset();
            break;
        }
    }
    const LaneJob job{a, p, (a.nq + p.cq - 1) / p.cq, lanes};
    Lane ln[kMaxLanes];
    auto run = [&](SearchCtx& lc, uint32_t t) {
        ln[t].rc = run_lane(job, lc, t, ln[t]);
        if (ln[t].rc != DANN_OK) grab_error_text(ln[t].text);
    };
    // (the helpers are joined on every way out of this scope: a joinable std::thread must never be destroyed)
    struct Helpers {
        std::thread th[kMaxLanes - 1];
        ~Helpers() {
            for (auto& t : th)
                if (t.joinable()) t.join();
        }
    } helpers;
    for (uint32_t t = 1; t < lanes; ++t) {
        try {
            helpers.th[t - 1] = std::thread([&, t]() {
                try {
                    (void)hipSetDevice(dev);
                    run(*extra[t - 1]->ctx, t);
                } catch (...) {
                    ln[t].rc = DANN_EINTERNAL;
                    ln[t].text = "exception in a lane of the host-pointer pipeline";
                }
            });
        } catch (...) {}  // no thread to be had (th[t - 1] stays not joinable): the calling thread takes its chunks
    }
    run(ctx, 0);
    for (uint32_t t = 1; t < lanes; ++t)
        if (!helpers.th[t - 1].joinable() && ln[0].rc == DANN_OK) run(ctx, t);  // (after its own)
    for (uint32_t t = 1; t < lanes; ++t)
        if (helpers.th[t - 1].joinable()) helpers.th[t - 1].join();
    const Lane* worst = nullptr;  // a call-level failure of any lane, else the failed query with the smallest index
    for (uint32_t t = 0; t < lanes; ++t)
        if (ln[t].rc != DANN_OK) {
            set_error("%s", ln[t].text.c_str());
            return ln[t].rc;
        } else if (ln[t].failed != DANN_OK && (!worst || ln[t].failed_chunk < worst->failed_chunk))
            worst = &ln[t];
    if (worst) set_error("%s", worst->text.c_str());
    return worst ? worst->failed : DANN_OK;
}
}  // namespace

int32_t dann_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t l_value, uint32_t beam_width,
                          uint32_t k, uint32_t* out_ids, float* out_dists, dann_search_stats* out_stats) try {
    if (!idx) {
        set_error("null index");
        return DANN_EINVAL;
    }
    std::shared_lock<std::shared_mutex> _rd(idx->rw);
    DeviceGuard _guard(idx->device);
    if (nq == 0) return DANN_OK;
    if (!queries || !out_ids || !out_dists) return DANN_EINVAL;
    const size_t qb = idx->query_bytes();  // PQ: f32 queries
    const HostArgs a{idx, queries, nq, l_value, beam_width, k, out_ids, out_dists, out_stats, qb};
    HostPlanIn in{idx->cfg.dtype, idx->dbg_u32(DANN_DBG_HOST_PIPELINE, 1u), idx->dbg_u32(DANN_DBG_HOST_CHUNK, kHostChunk),
                  nq, k, qb, false, false, false, false};
    if (host_chunked(in.pipeline, in.host_chunk, nq)) {  // (only there does the plan depend on the caller's pinning)
        in.q_pinned = temp_pins().caller_pinned(queries, (size_t)nq * qb);
        in.ids_pinned = temp_pins().caller_pinned(out_ids, (size_t)nq * k * 4);
        in.dists_pinned = temp_pins().caller_pinned(out_dists, (size_t)nq * k * 4);
        in.stats_pinned = !out_stats || temp_pins().caller_pinned(out_stats, (size_t)nq * sizeof(dann_search_stats));
    }
    HostPlan plan = plan_host_search(in);
    if (plan.strategy == HostStrategy::Small) {
        SmallCall me(queries, nq, l_value, beam_width, k, out_ids, out_dists, out_stats);
        const int32_t rc = small_call(idx->comb, me, qb, [&](SmallCall* const* calls, uint32_t n, uint32_t total, std::string& text) {
            const int32_t rrc = small_batch_run(idx, calls, n, total, qb);
            if (rrc != DANN_OK && rrc != kSmallCallDeclined) grab_error_text(text);
            return rrc;
        });
        if (rc != DANN_OK && rc != kSmallCallDeclined && !me.text.empty()) set_error("%s", me.text.c_str());
        if (rc != kSmallCallDeclined) return rc;
        plan.strategy = HostStrategy::Single;  // (the combiner declined)
    }
    CtxLease lease(idx);
    if (lease.status != DANN_OK) return lease.status;
    SearchCtx& ctx = *lease.ctx;
    PinScope pins;
    if (plan.may_register && idx->host_register_pays.load(std::memory_order_relaxed) && register_seen_buffers(a, in, pins))
        plan.strategy = HostStrategy::ZeroCopy;
    void* dptr[4] = {nullptr, nullptr, nullptr, nullptr};
    if (plan.strategy == HostStrategy::ZeroCopy && device_pointers(a, dptr)) return search_host_zero_copy(a, ctx, dptr);
    if (plan.strategy == HostStrategy::Single) return search_host_single(a, ctx, plan);
    return search_host_lanes(a, ctx, plan);  // (also ZeroCopy on buffers registered without the mapping)
} DANN_CATCH_ALL
