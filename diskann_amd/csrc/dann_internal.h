// dann_internal.h -- host-side structures shared by the translation units of libdann_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <exception>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <thread>
#include <functional>
#include <unordered_map>
#include <vector>

#include "../../include/dann.h"
#include "../../include/dann_debug.h"
#include "device_buffer.h"  // DevBuf, pow2_at_least
#include "row_dispatch.h"  // visit_row_op, RowSet, kNoMetric / kNoRow
#include "search_args.h"  // IndexView, ServerView, SearchArgs, VisitedCalib
#include "small_calls.h"

struct dann_index;

namespace dann {

void set_error(const char* fmt, ...);
int32_t hip_fail(hipError_t e, const char* what);

#define DANN_HIP(call)                                        \
    do {                                                      \
        hipError_t _e = (call);                               \
        if (_e != hipSuccess) return ::dann::hip_fail(_e, #call); \
    } while (0)

// every extern "C" entry point is a function-try-block closed by this: nothing unwinds across the C boundary
#define DANN_CATCH_ALL                                          \
    catch (const std::bad_alloc&) {                             \
        ::dann::set_error("out of host memory");                \
        return DANN_ENOMEM;                                     \
    }                                                           \
    catch (const std::exception& e) {                           \
        ::dann::set_error("internal error: %s", e.what());      \
        return DANN_EINVAL;                                     \
    }                                                           \
    catch (...) {                                               \
        ::dann::set_error("internal error");                    \
        return DANN_EINVAL;                                     \
    }

// visit_row_op (row_dispatch.h) for a launch site: a metric that is not defined for the row type is the same error
// everywhere; kNoRow comes back, and the site answers a dtype outside its row set in its own words
template <RowSet ROWS, class F>
int32_t dispatch_row_op(int dtype, int metric, F&& f) {
    const int32_t rc = visit_row_op<ROWS>(dtype, metric, f);
    if (rc != kNoMetric) return rc;
    set_error("metric %d is not defined for dtype %d", metric, dtype);
    return DANN_EUNSUPPORTED;
}

// how a launch raises its kernel's limit of dynamic LDS past the default 64 KiB
enum LdsRaise {
    kLdsExact,   // to the launch's own size, on every launch that needs it
    kLds160Once, // to the CU's 160 KiB, once per device for each instantiation
    kLds160      // to 160 KiB, on every launch that needs it
};

// Raise the LDS limit, launch, check.  `what` is the text of a failed launch's error.
template <auto Kern, LdsRaise RAISE = kLdsExact, class... Args>
int32_t launch_kernel(const char* what, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args) {
    if (lds > 64 * 1024) {
        const void* fn = reinterpret_cast<const void*>(Kern);
        if constexpr (RAISE == kLdsExact) {
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute");
        } else {
            static bool raised[64] = {};  // (one per instantiation: Kern is a template argument)
            int dev = 0;
            if (RAISE == kLds160Once) (void)hipGetDevice(&dev);
            if (RAISE == kLds160 || dev < 0 || dev >= 64 || !raised[dev]) {
                hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
                if (RAISE == kLds160Once && dev >= 0 && dev < 64) raised[dev] = true;
            }
        }
    }
    hipLaunchKernelGGL(Kern, grid, block, lds, stream, args...);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return DANN_OK;
}

struct KernelClock {
    double total_ms = 0.0;
    uint64_t launches = 0;
};

// lap tag of a submission-ring entry: never 0 (the ring starts zeroed), consecutive laps differ
__host__ __device__ inline uint32_t server_lap_tag(unsigned long long ticket, uint32_t ring_shift) {
    return (uint32_t)((ticket >> ring_shift) % 4095ull) + 1u;
}

// Everything one in-flight search call needs besides the (read-only) index: its own stream and events, the retry
// scratch, a pool of global-memory visited tables, the failure flag and staging buffers.  The index owns one
// (`main`, also the stream of every mutation) plus a pool of further ones handed to concurrent searches -- the
// reference's model is N workers calling `search` on one shared `&DiskANNIndex`
// (diskann-benchmark-core/src/search/api.rs:409-425); here N callers' launches run side by side on N streams.
struct SearchCtx {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t* d_fail = nullptr;  // retry scratch: [count, pad, list A (cap), list B (cap)]
    size_t fail_cap = 0;
    uint32_t* d_sched = nullptr;  // locality scheduling: [slot map (cap), keys (cap), per-block histograms]
    size_t sched_words = 0;
    uint32_t* d_spill = nullptr;  // spill tables | counter (+pad) | busy flags | cmps histogram
    uint32_t spill_slices = 0, spill_bits = 0;
    uint32_t* h_flag = nullptr;  // pinned, device-visible: set by a query that exhausts its scratch
    // grow-only device staging for the host-pointer search entry (no hipMalloc / hipFree per call)
    // [0] queries, [1] outputs, [2] stats, [3] unused, [4] the arena of the staged host-pointer calls (host_stage.h: range,
    // filtered, diverse, flat; on `main`: rerank, record) and the flat scan's chunk lists (one block, laid out per call)
    void* stage[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t stage_bytes[5] = {0, 0, 0, 0, 0};
    void* h_stage = nullptr;     // pinned host staging (small batches: one H2D + one D2H per call; large: chunk ring)
    size_t h_stage_bytes = 0;
    int32_t init();   // stream, events, failure flag (device already current)
    void destroy();
};

int32_t launch_search(const SearchArgs& a, hipStream_t stream, int* regs_out = nullptr);
// query_schedule.hip: locality scheduling of large launches
uint32_t sched_pivot_count(uint32_t dim);
size_t sched_scratch_words(uint32_t dim, uint32_t nq);
int32_t sched_build_pivots(dann_index* idx, hipStream_t st);
// dann_debug_sched_pivots: the pivot slab as unscaled f32 (DANN_EINVAL before the first scheduled search)
int32_t sched_copy_pivots(const dann_index* idx, float* out, uint32_t cap_floats, uint32_t* out_np, uint32_t* out_stride,
                          float* out_scale);
// (its first kernel also clears zero[0 .. zero_words): the launch's spill-pool counters, with no operation of their own)
int32_t sched_build_map(const dann_index* idx, hipStream_t st, const void* queries, uint32_t nq, uint32_t parts,
                        uint32_t* scratch, uint32_t* qmap, uint32_t* zero, uint32_t zero_words);
// one translation unit per row type (search_<type>.hip) holds the kernel instantiations
#define DANN_DECL_LAUNCH(name) \
    int32_t launch_search_##name(const SearchArgs& a, uint32_t qcap, size_t lds, hipStream_t stream, int* regs_out)
DANN_DECL_LAUNCH(f32);
DANN_DECL_LAUNCH(f16);
DANN_DECL_LAUNCH(u8);
DANN_DECL_LAUNCH(i8);
DANN_DECL_LAUNCH(sq8);
DANN_DECL_LAUNCH(sq4);
DANN_DECL_LAUNCH(sq1);
DANN_DECL_LAUNCH(sph1);
DANN_DECL_LAUNCH(sph1t);
DANN_DECL_LAUNCH(sph2);
DANN_DECL_LAUNCH(sph4);
DANN_DECL_LAUNCH(mm1);
DANN_DECL_LAUNCH(mm2);
DANN_DECL_LAUNCH(mm4);
DANN_DECL_LAUNCH(mm8);
DANN_DECL_LAUNCH(mm1q);
DANN_DECL_LAUNCH(mm2q);
DANN_DECL_LAUNCH(mm4q);
DANN_DECL_LAUNCH(pq);
// search_diverse.hip: dann_diverse_search_batch on device-resident queries and outputs (host-synchronous on `stream`)
int32_t diverse_search_device(dann_index* idx, hipStream_t stream, const void* d_queries, uint32_t nq, uint32_t l_value,
                              uint32_t beam_width, uint32_t k, uint32_t diverse_k, uint32_t total_k, uint32_t* d_ids,
                              float* d_dists, dann_search_stats* d_stats);
#undef DANN_DECL_LAUNCH
int32_t launch_search_pqlut(const SearchArgs& a, size_t lds, hipStream_t stream);  // search_pqlut.hip (SearchArgs::pqlut)
int32_t launch_search_pqlut_g1(const SearchArgs& a, size_t lds, hipStream_t stream);
int32_t launch_search_pqlut_g2(const SearchArgs& a, size_t lds, hipStream_t stream);  // search_pqlut2.hip .. 4: 17 .. 64 chunks
int32_t launch_search_pqlut_g3(const SearchArgs& a, size_t lds, hipStream_t stream);
int32_t launch_search_pqlut_g4(const SearchArgs& a, size_t lds, hipStream_t stream);
int32_t launch_search_pair(const SearchArgs& a, size_t lds, hipStream_t stream);   // search_pair.hip (SearchArgs::pair)
// launch + re-run queries whose visited table overflowed with a table twice as large (up to 2^15)
int32_t search_with_retry(dann_index* idx, SearchCtx& ctx, SearchArgs a);
// enqueue the persistent server kernel (a.srv filled in) on ctx.stream; returns without waiting
int32_t launch_search_server(dann_index* idx, SearchCtx& ctx, SearchArgs a);  // also feeds clocks[0] with the main launch's HIP-event time
// explicit table size set with dann_set_visited_bits, or 0 = let search_with_retry size it
uint32_t auto_visited_entries(const dann_index* idx, uint32_t l_value, uint32_t beam);

// HIP-event time of the MFMA Gram-tile launches of the build path (build_batch.hip; dann_kernel_time which = 5)
int32_t build_tile_clock(const dann_index* idx, double* total_ms, uint64_t* launches);
void build_tile_clock_reset(const dann_index* idx);
// robust_prune_list (force_saturate = false) of caller-built pools straight into the adjacency rows (build_batch.hip;
// graph consolidation, consolidate.hip).  Queued on idx->main.stream; prune_pools_use_gram: whether
// it takes the matrix-core path (the back-edge prunes' policy).
bool prune_pools_use_gram(const dann_index* idx);
int32_t prune_pools_into_rows(dann_index* idx, const dann_build_config& cfg, const uint32_t* d_locs, const uint32_t* d_ids,
                              const float* d_dists, const uint32_t* d_counts, uint32_t stride, uint32_t m, bool* used_gram);
// idx->d_deleted, allocated and cleared on first use (consolidate.hip; dann_delete_points, dann_inplace_delete)
int32_t ensure_deleted_bitmap(dann_index* idx);
// consolidate.hip: the scan / gather / prune pass of dann_consolidate, also run by dann_prune_range (graph_stats.hip).
// The caller holds the index exclusively, has checked cfg and the ids, and made the index's device current.
struct ListPrunePass {
    const char* who = "";            // the entry point, for messages
    const uint32_t* ids = nullptr;   // host; null = the slots [first, first + n)
    uint32_t first = 0, n = 0;
    bool prune_range = false;        // no deleted state: a list longer than pruned_degree is pruned, every other left alone;
                                     // on an inline-tags index unreadable slots are skipped (as neighbours) / left alone (as ids)
    bool drop_deleted = false;       // DANN_CONSOLIDATE_DROP_DELETED
    int32_t* out_kind = nullptr;     // n ConsolidateKind values, or null
    bool want_counters = false;      // read dann_build_counters around the pass (distances, on_matrix_cores)
    // results (distances and on_matrix_cores without want_counters: the gather's share alone, 0)
    uint64_t scanned = 0, unreadable = 0, rewritten = 0, pruned = 0, largest = 0, distances = 0, on_matrix_cores = 0,
             oversized = 0, oversized_tied = 0;
};
int32_t run_list_prunes(dann_index* idx, const dann_build_config* cfg, ListPrunePass& pass);
// medoid_kernels.hip: dann_medoid_device's body (the device is current); times_ms: null, or the two passes' HIP-event times
int32_t medoid_device(int32_t dtype, const void* d_rows, uint64_t nrows, uint32_t dim, uint64_t stride, int64_t* out_row,
                      float* d_out_mean, uint64_t* out_counters, double* times_ms);

// minmax_kernels.hip: MinMaxQuantizer::compress on device buffers (dann_minmax_compress, dann_minmax_quantize(_device))
int32_t launch_minmax_compress(int32_t bits, const float* d_x, uint32_t n, uint32_t dim, float grid_scale, uint8_t* d_out,
                               float* d_out_loss, uint32_t* d_nan_flag, hipStream_t stream);

// maxsim_kernels.hip: multi-vector scores (dann_maxsim_batch, dann_chamfer_rerank_batch).  Rows of documents and of
// queries sit at `stride` / `qstride` bytes, multiples of 16, the bytes behind `dim` zero.  MinMax sets
// (maxsim_mm_kernels.hip): the rows are the packed codes alone, and each row has a 16-byte MmRowHeader beside them.
constexpr uint32_t kMaxSimQueryRows = 1024, kMaxSimDim = 4096, kMaxSimCands = 4096, kMaxSimQueries = 65535;
struct MmRowHeader {
    float b, n, a;             // MinMaxCompensation's b, n, a (norm_squared is not needed by the inner product)
    int32_t sum;               // sum over k < dim of the code as the matrix cores see it: c - 128 for 8-bit codes, else c
};
struct MaxSimArgs {
    const uint8_t* drows;      // the set's rows
    const uint64_t* doff;      // ndocs + 1 row offsets
    uint32_t ndocs, dim, stride;
    uint32_t qstride;          // == stride unless a MinMax query is wider than the set's rows
    const MmRowHeader* dhdr;   // MinMax sets: one per row of drows / qrows; else null
    const MmRowHeader* qhdr;
    const uint8_t* qrows;      // the queries' rows
    const uint32_t* qoff;      // nq + 1 row offsets
    const uint32_t* cand;      // nq x cand_stride document ids
    uint32_t cand_stride;
    float* out_chamfer;        // nq x cand_stride
    float* out_scores;         // null, or q_rows(q) floats at qoff[q] * cand_stride + c * q_rows(q)
    uint32_t* status;          // set to 1 by a candidate id >= ndocs
};
int32_t launch_maxsim(int32_t dtype, int32_t order, const MaxSimArgs& a, uint32_t nq, hipStream_t stream);
// maxsim_mm_kernels.hip.  MinMax images (d_images: nrows x image_bytes, any alignment) -> zero-padded codes at `stride`
// and header records; and the scores of a (query width, row width) pair the reference has.
int32_t launch_mm_repack(int32_t dtype, const uint8_t* d_images, uint32_t image_bytes, uint64_t nrows, uint32_t dim,
                         uint8_t* d_codes, uint32_t stride, MmRowHeader* d_hdr, hipStream_t stream);
int32_t launch_maxsim_mm(int32_t qdtype, int32_t dtype, int32_t order, const MaxSimArgs& a, uint32_t nq, hipStream_t stream);
int32_t launch_chamfer_sort(const uint32_t* d_cand, const float* d_chamfer, uint32_t nq, uint32_t stride, uint32_t ndocs,
                            uint32_t k, uint32_t* d_out_ids, float* d_out_d, uint32_t* d_out_counts, hipStream_t stream);

int32_t launch_expand_beam(const IndexView& ix, const void* d_queries, uint32_t nq, const uint32_t* d_ids,
                           const uint64_t* d_offsets, uint64_t max_len, float* d_out, hipStream_t stream);
int32_t launch_rerank(const IndexView& ix, const void* d_queries, uint32_t nq, const uint32_t* d_cand, uint32_t stride,
                      uint32_t k, uint32_t* d_out_ids, float* d_out_d, hipStream_t stream);
int32_t launch_distance_pairs(const IndexView& ix, const uint32_t* d_a, const uint32_t* d_b, uint32_t n, float* d_out,
                              hipStream_t stream);
// dann_pq_pack_neighbors: writes the packed rows (adjacency + neighbours' code rows) of every slot of the index
int32_t launch_pq_pack(const IndexView& ix, uint8_t* d_pack, uint32_t stride, uint32_t codes_off, hipStream_t stream);
// raw rows x[i] vs y[i] (pair kernel numerics), n pairs of `bytes` each
int32_t launch_distance_raw(const IndexView& ix, const void* d_x, const void* d_y, uint64_t stride, uint32_t n,
                            float* d_out, hipStream_t stream);
// flat_kernels.hip: the exhaustive scan of dann_flat_search_batch(_device), cut up as flat_plan.h says.  One launch pair
// serves at most plan.batch queries over slots [first, first + n), n > 0; `scratch` holds plan.scratch_bytes();
// d_deleted: the deleted bitmap when it is to be honoured, else null.
struct FlatPlan;
uint32_t flat_query_slot_bytes(const IndexView& ix);  // bytes of one staged query in LDS
int32_t launch_flat_search(const IndexView& ix, const FlatPlan& plan, const void* d_queries, uint32_t nq, uint32_t first,
                           uint32_t n, const uint32_t* d_deleted, void* scratch, uint32_t* d_ids, float* d_dists,
                           dann_search_stats* d_stats, hipStream_t stream);
int32_t launch_flat_empty(uint32_t nq, uint32_t k, uint32_t* d_ids, float* d_dists, dann_search_stats* d_stats,
                          hipStream_t stream);
// pq_kernels.hip: the lookup tables [nq][nchunks][256] of nq f32 queries (populate_chunk_distances_impl), device to device
int32_t launch_pq_lut(int32_t metric, const float* d_pivots, const uint32_t* d_offsets, uint32_t nchunks, uint32_t dim,
                      const float* d_queries, uint32_t nq, float* d_lut, hipStream_t stream);
// flat_pq_kernels.hip: the exhaustive scan over PQ code rows of dann_pq_linear_search_batch(_device), cut up as
// flat_pq_plan.h says.  One launch serves at most plan.batch queries over slots [first, first + n), n > 0; `scratch` holds
// plan.scratch_bytes(); d_filter: these queries' bitmaps (null: every slot matches), `stride` words apart (0: one for all).
struct FlatPqPlan;
int32_t launch_flat_pq_search(const IndexView& ix, const FlatPqPlan& plan, const float* d_queries, uint32_t nq, uint32_t first,
                              uint32_t n, const uint32_t* d_deleted, const uint32_t* d_filter, uint64_t stride, void* scratch,
                              uint32_t* d_ids, float* d_dists, dann_search_stats* d_stats, hipStream_t stream);

}  // namespace dann

struct dann_server;  // persistent search server (server.hip)

namespace dann {
// A counter many threads bump at millions of operations per second (the per-query path of the search server): one cell
// per cache line, a thread uses "its" cell; only the rare readers (dann_server_stop, a mutation's busy test) sum them.
// With sixteen callers on ONE atomic the server's throughput halved (4.5 -> 2.2 M queries/s at 64 tickets in flight per
// thread).  All operations are sequentially consistent: the publish-then-look handshakes built on it rely on that.
struct ShardedCounter {
    static constexpr uint32_t kCells = 32;
    struct alignas(64) Cell {
        std::atomic<int64_t> v{0};
    };
    Cell cell[kCells];
    static uint32_t home() {
        static thread_local const uint32_t h = (uint32_t)(std::hash<std::thread::id>()(std::this_thread::get_id()) *
                                                          0x9E3779B97F4A7C15ull >> 59);
        return h & (kCells - 1u);
    }
    void add(int64_t d) { cell[home()].v.fetch_add(d, std::memory_order_seq_cst); }
    int64_t sum() const {
        int64_t s = 0;
        for (const Cell& c : cell) s += c.v.load(std::memory_order_seq_cst);
        return s;
    }
    void reset() {
        for (Cell& c : cell) c.v.store(0, std::memory_order_seq_cst);
    }
};
}  // namespace dann

struct dann_index {
    dann_config cfg;
    int device = 0;
    dann::SearchCtx main;  // stream of every mutation and of the non-concurrent entry points
    uint8_t* d_rows = nullptr;
    uint32_t* d_adj = nullptr;
    uint32_t layer_bytes = 0;
    uint32_t nslots = 0;
    uint32_t visited_bits = 0;
    uint32_t visited_format = 0;   // dann_set_visited_format: 0 = automatic, 32 / 16 = entry width of the LDS visited table
    uint32_t max_concurrency = 0;  // dann_set_max_concurrency: queries in flight per search call (0 = all of them)
    uint32_t prune_tie_order = DANN_TIE_RUST;  // dann_set_prune_tie_order: DANN_TIE_RUST (default) / DANN_TIE_POSITION
    // dann_search_batch on pageable host buffers: the last eight (queries, ids, distances, nq) it was called with (stat_mu)
    // -- a call seen before page-locks its buffers for its duration -- and whether doing so is cheap on this system
    struct HostCall {
        const void* q = nullptr;
        const void* i = nullptr;
        const void* d = nullptr;
        uint32_t nq = 0;
        uint32_t registered = 0;  // calls that page-locked these buffers so far
        bool operator==(const HostCall& o) const { return q == o.q && i == o.i && d == o.d && nq == o.nq; }
    };
    HostCall host_calls[8];
    uint32_t host_calls_next = 0;
    std::atomic<bool> host_register_pays{true};
    // dann_search_batch, small calls: several threads calling side by side are served by one launch (small_calls.h)
    dann::SmallCallQueue comb;
    uint32_t num_cus = 256;      // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    uint32_t build_flags = 0;    // DANN_BUILD_* (dann_set_build_options)
    // [0] back-edge prunes through the MFMA path, [1] ... on the lazy path inside it, [2] / [3] comparisons / hops of
    // the insert-time searches (host side; the device-side counters live in the build scratch)
    uint64_t build_counters[4] = {0, 0, 0, 0};  // [2] comparisons, [3] hops of the insert searches ([0], [1]: unused)
    float* d_pq_pivots = nullptr;
    uint32_t* d_pq_offsets = nullptr;
    // dann_pq_pack_neighbors: adjacency + neighbours' code rows per node; dropped (valid = false) by every mutation
    uint8_t* d_pq_pack = nullptr;
    size_t pq_pack_bytes = 0;
    uint32_t pq_pack_stride = 0, pq_pack_codes = 0;
    bool pq_pack_valid = false;
    // locality scheduling of large search launches (query_schedule.hip): the pivots (centres trained from rows taken at a
    // fixed stride) in the key kernel's layout, built on the first scheduled search and again on the first one after a
    // mutation (sched_mu; they only ever affect speed)
    _Float16* d_sched_piv = nullptr;
    bool sched_stale = true;
    std::mutex sched_mu;
    // dann_delete_points: one bit per slot, set = deleted (DataProvider::delete).  Allocated by the first delete; null =
    // nothing was ever deleted.  Read by dann_consolidate (consolidate.hip).
    uint32_t* d_deleted = nullptr;
    // dann_set_attributes: one u32 per slot (DANN_NO_ATTRIBUTE = none), allocated by the first set; null = no slot has one.
    // Read by the diverse search (search_diverse.hip).
    uint32_t* d_attr = nullptr;
    std::unordered_map<uint64_t, dann::VisitedCalib> calib;  // guarded by stat_mu
    void* build_scratch = nullptr;            // a BuildScratch (build_scratch.h), owned by build_batch.hip
    void (*build_scratch_free)(void*) = nullptr;
    dann::KernelClock clocks[5];  // 4 = beam-search retry launches (ms already in [0]; launches = re-run queries); stat_mu
    dann::KernelClock families[DANN_FAMILY_COUNT];  // beam-search launches per kernel family (dann_debug.h); stat_mu
    // development switches (dann_debug_set; NaN = default).  Plain doubles written by the test / bench thread before
    // the calls they are meant for: relaxed atomics keep concurrent searches well-defined.
    std::atomic<double> dbg[DANN_DBG_COUNT];
    double dbg_value(int key, double dflt) const {
        const double v = dbg[key].load(std::memory_order_relaxed);
        return v == v ? v : dflt;
    }
    uint32_t dbg_u32(int key, uint32_t dflt) const {
        const double v = dbg[key].load(std::memory_order_relaxed);
        return v == v ? (v <= 0.0 ? 0u : v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v) : dflt;
    }
    bool tune_off(uint32_t bit) const { return (dbg_u32(DANN_DBG_TUNE_OFF, 0u) & bit) != 0; }
    bool tune_on(uint32_t bit) const { return (dbg_u32(DANN_DBG_TUNE_ON, 0u) & bit) != 0; }
    bool verbose() const { return dbg_u32(DANN_DBG_VERBOSE, 0u) != 0; }
    std::vector<uint64_t> ext_ids;  // slot -> external id (empty = identity for dynamic slots)
    std::vector<uint8_t> h_tags;    // inline_tags: host mirror of the tag bytes (the reference's Store::tags, store.rs:150)
    // Locking.  `rw` is the index: shared by the Knn search entry points (dann_search_batch(_device), the server),
    // exclusive for everything that mutates the index or uses the `main` context.  Exclusive calls may nest
    // (dann_append_neighbors -> dann_get_neighbors): `mu` serialises them among themselves and `excl_depth` takes /
    // drops `rw` at the outermost level only.  std::shared_mutex does not promise writer priority: a mutation waits
    // for the searches in flight (the reference's writers go through EBR / tags instead; out of scope).
    mutable std::recursive_mutex mu;
    mutable std::shared_mutex rw;
    mutable uint32_t excl_depth = 0;
    mutable std::mutex stat_mu;   // calib, clocks
    // pool of further search contexts for concurrent callers
    std::mutex ctx_mu;
    std::condition_variable ctx_cv;
    std::vector<dann::SearchCtx*> ctx_free;
    uint32_t ctx_created = 0;
    // dann_server_start / dann_search_submit.  submit / wait / poll take no lock: they pin the server (srv_users) for the
    // duration of the call and dann_server_stop unpublishes the pointer, then waits for the pins to drain before it
    // frees anything.  srv_outstanding = tickets submitted and not yet collected; `mutating` = mutations in progress:
    // the two sides of the "no mutation while tickets are outstanding" rule (MutationScope, DANN_EBUSY).
    std::atomic<dann_server*> server{nullptr};
    dann::ShardedCounter srv_users;
    dann::ShardedCounter srv_outstanding;
    std::atomic<uint32_t> mutating{0};
    // spherical rows: iface::QueryLayout of the queries the entry points take (dann_set_query_layout)
    std::atomic<int32_t> query_layout{0};
    // (MinMax rows: QL_EIGHT_BIT says that the queries are MM8 images, dann_set_query_dtype)
    uint32_t query_bytes() const;  // bytes of one query of the query-taking entry points under the current layout
    uint32_t query_bytes(int32_t layout) const;
    dann::IndexView view() const;  // row x row work: a stored row as the query is always the symmetric form
    dann::IndexView qview() const;               // the query-taking entry points: the current layout
    dann::IndexView qview(int32_t layout) const;
};

namespace dann {
// exclusive access (mutations, every entry point that runs on idx->main)
struct ExclusiveGuard {
    const dann_index* i;
    explicit ExclusiveGuard(const dann_index* idx) : i(idx) {
        i->mu.lock();
        if (i->excl_depth++ == 0) i->rw.lock();
    }
    ~ExclusiveGuard() {
        if (--i->excl_depth == 0) i->rw.unlock();
        i->mu.unlock();
    }
    ExclusiveGuard(const ExclusiveGuard&) = delete;
    ExclusiveGuard& operator=(const ExclusiveGuard&) = delete;
};
// a mutation of the index (rows, tags, adjacency, build): refused with DANN_EBUSY while server tickets are outstanding,
// and while it runs dann_search_submit refuses new tickets.  Both sides publish first and look second (sequentially
// consistent): at least one of a racing pair sees the other.
struct MutationScope {
    dann_index* i;
    bool ok;
    explicit MutationScope(const dann_index* idx) : i(const_cast<dann_index*>(idx)) {
        if (i->srv_outstanding.sum() != 0) {  // refused without ever raising `mutating`: no submit bounces on our account
            ok = false;
            return;
        }
        i->mutating.fetch_add(1, std::memory_order_seq_cst);
        ok = i->srv_outstanding.sum() == 0;
        if (!ok) i->mutating.fetch_sub(1, std::memory_order_seq_cst);
        else {  // (the caller holds the index exclusively) derived layouts die with the mutation
            i->pq_pack_valid = false;
            i->sched_stale = true;
        }
    }
    ~MutationScope() {
        if (ok) i->mutating.fetch_sub(1, std::memory_order_seq_cst);
    }
    MutationScope(const MutationScope&) = delete;
    MutationScope& operator=(const MutationScope&) = delete;
};
bool server_quiesce(dann_index* idx);  // server.hip: the resident kernel leaves and is waited for (relaunched by the next
                                       // submit); false: the server is poisoned and was not waited for
#define DANN_MUTATION(idx)                                                                                            \
    ::dann::MutationScope _mut(idx);                                                                                  \
    if (!_mut.ok) {                                                                                                   \
        ::dann::set_error("the index has search-server tickets outstanding: collect them (dann_search_wait) or stop " \
                          "the server before mutating the index");                                                   \
        return DANN_EBUSY;                                                                                            \
    }                                                                                                                 \
    if (!::dann::server_quiesce(const_cast<dann_index*>(static_cast<const dann_index*>(idx)))) {                     \
        ::dann::set_error("the index's search server stopped answering (a wait ran into its limit): dann_server_stop " \
                          "before mutating the index");                                                              \
        return DANN_EHIP;                                                                                             \
    }                                                                                                                 \
    (void)0
// the prune kernels' largest candidate pool (their LDS layout); larger pools are refused, or cut to it first
constexpr uint32_t kMaxPool = 4096;
// build_batch.hip: a dann_build_config against the index, for every entry point that prunes (`what` names it in the
// message).  DANN_EUNSUPPORTED: PQ rows, a metric the row type does not have, max_occlusion_size > kMaxPool;
// DANN_EINVAL: the rest.  Only the build path searches, so only it needs l_build.
int32_t check_build_cfg(const dann_index* idx, const dann_build_config* cfg, const char* what, bool need_l_build);
constexpr uint32_t kTieWorkBytes = 512 + 2048;
constexpr uint32_t kMaxSearchCtx = 16;
// a search context for one concurrent call: from the pool, created on demand (at most kMaxSearchCtx), else waits
struct CtxLease {
    dann_index* idx;
    SearchCtx* ctx = nullptr;
    int32_t status = DANN_OK;
    explicit CtxLease(dann_index* idx, bool try_only = false);
    ~CtxLease();
    CtxLease(const CtxLease&) = delete;
    CtxLease& operator=(const CtxLease&) = delete;
};
// makes `dev` the current device for the length of a call (`ok`: hipSetDevice succeeded)
struct DeviceGuard {
    int prev = -1, cur = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) : cur(dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != cur) (void)hipSetDevice(prev);  // hipSetDevice costs ~0.5 ms on ROCm 7.2
    }
};
// api_search.hip: one Knn search launch (with the overflow retry) on device buffers, on context `ctx`
int32_t search_device(dann_index* idx, SearchCtx& ctx, const void* d_queries, const uint32_t* d_qslots, uint32_t nq,
                      uint32_t l_value, uint32_t beam, uint32_t k, uint32_t* d_ids, float* d_dists,
                      dann_search_stats* d_stats, uint32_t* d_rec_ids, float* d_rec_d, uint32_t rec_stride,
                      uint32_t* d_rec_n);
// api_index.hip: grow the context's device staging block `i` to at least `need` bytes (grow-only, 25 % headroom)
int32_t grow_stage(SearchCtx& ctx, int i, size_t need);
}  // namespace dann

struct dann_query {
    const dann_index* idx;
    int32_t layout = 0;  // the index's query layout when the query was created (its byte image is of that layout)
    void* d_query = nullptr;
};
