// build_batch.hip -- batched Vamana insert on the GPU: the per-index scratch, one multi_insert batch in two phases
// (batch_candidates: insert searches + pool prunes; batch_commit: back-edge aggregation, bootstrap, graph update),
// prune_pools_into_rows for graph consolidation, and the C entry points of the build path.  The prunes themselves are
// launched through prune_rows.h (row kernels) and prune_gram.h (matrix cores); this unit holds no prune kernel.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <mutex>
#include <vector>

#include "prune_gram.h"
#include "prune_rows.h"

namespace dann {
namespace {

// DANN_DBG_POOL_GRAM = 0 keeps the row kernel for the pool prune of large rows (A/B runs)
bool pool_gram_default(const dann_index* idx) { return idx->dbg_u32(DANN_DBG_POOL_GRAM, 1u) != 0u; }

int32_t ensure_scratch(BuildScratch& s, uint32_t batch, uint32_t rec_stride, uint32_t degree) {
    if (batch <= s.batch_cap && rec_stride == s.rec_stride && degree == s.degree) return DANN_OK;
    const uint32_t cap = std::max<uint32_t>(batch, 1024);
    s.batch_cap = 0;  // committed only after every allocation succeeded (a failed hipMalloc must not pass the cache test)
    s.pend_stride = degree + 1;
    const size_t nkeys = (size_t)cap * degree;
    DANN_HIP(s.slots.alloc((size_t)cap * 4));
    DANN_HIP(s.rec_ids.alloc((size_t)cap * rec_stride * 4));
    DANN_HIP(s.rec_d.alloc((size_t)cap * rec_stride * 4));
    DANN_HIP(s.rec_n.alloc((size_t)cap * 4));
    DANN_HIP(s.stats.alloc((size_t)cap * sizeof(dann_search_stats)));
    DANN_HIP(s.pending.alloc((size_t)cap * s.pend_stride * 4));
    DANN_HIP(s.pending2.alloc((size_t)cap * s.pend_stride * 4));
    DANN_HIP(s.keys_in.alloc(nkeys * 8));
    DANN_HIP(s.keys_out.alloc(nkeys * 8));
    DANN_HIP(s.seg_start.alloc(nkeys * 4));
    DANN_HIP(s.seg_len.alloc(nkeys * 4 * 3));  // segment lengths | short worklist | long worklist
    DANN_HIP(s.meta.alloc(128));  // 16 words of flags and counts + the insert searches' totals (stats_reduce_kernel)
    DANN_HIP(hipMemset(s.meta.p, 0, 64));  // the commit phase may run first on this handle (sharded build: empty slice)
    if (!s.counters.p) {
        DANN_HIP(s.counters.alloc((size_t)kStatStripes * 64 + 64));
        DANN_HIP(hipMemset(s.counters.p, 0, (size_t)kStatStripes * 64 + 64));
    }
    size_t tmp = 0;
    DANN_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp, s.keys_in.as<uint64_t>(), s.keys_out.as<uint64_t>(),
                                               (int)nkeys, 0, 64, nullptr));
    s.sort_tmp_bytes = tmp;
    DANN_HIP(s.sort_tmp.alloc(tmp));
    s.batch_cap = cap;
    s.rec_stride = rec_stride;
    s.degree = degree;
    return DANN_OK;
}

// grow-only buffers of the MFMA prunes: sorted lists, Gram blocks and norms of `items` lists
int32_t ensure_gram_scratch(BuildScratch& s, size_t items, uint32_t pcap, uint32_t ng, uint32_t mg) {
    const size_t sorted_elems = items * pcap, gram_elems = items * ng * mg, nrm_elems = items * ng;
    if (s.g_sorted_elems < sorted_elems) {
        s.g_sorted_elems = 0;
        DANN_HIP(s.g_sid.alloc(sorted_elems * 4));
        DANN_HIP(s.g_sd.alloc(sorted_elems * 4));
        s.g_sorted_elems = sorted_elems;
    }
    if (s.g_items < items) {
        s.g_items = 0;
        DANN_HIP(s.g_sn.alloc(items * 4));
        DANN_HIP(s.g_loc.alloc(items * 4));
        DANN_HIP(s.g_order.alloc(items * 4));
        s.g_items = items;
    }
    if (s.g_gram_elems < gram_elems) {
        s.g_gram_elems = 0;
        DANN_HIP(s.g_gram.alloc(gram_elems * 4));
        s.g_gram_elems = gram_elems;
    }
    if (s.g_nrm_elems < nrm_elems) {
        s.g_nrm_elems = 0;
        DANN_HIP(s.g_nrm.alloc(nrm_elems * 4));
        s.g_nrm_elems = nrm_elems;
    }
    return DANN_OK;
}

}  // namespace

int32_t check_build_cfg(const dann_index* idx, const dann_build_config* cfg, const char* what, bool need_l_build) {
    if (!cfg) return DANN_EINVAL;
    if (idx->cfg.dtype == DT_PQ) {
        set_error("%s: not defined on DANN_PQ rows (use the full-precision index)", what);
        return DANN_EUNSUPPORTED;
    }
    int op;
    bool norm;
    if (!resolve_metric(idx->cfg.dtype, idx->cfg.metric, &op, &norm)) {
        set_error("metric %d is not defined for dtype %d", idx->cfg.metric, idx->cfg.dtype);
        return DANN_EUNSUPPORTED;
    }
    if (cfg->pruned_degree == 0 || (need_l_build && cfg->l_build == 0) || cfg->max_degree < cfg->pruned_degree ||
        cfg->max_degree > idx->cfg.max_degree || !(cfg->alpha >= 1.0f)) {
        set_error("%s: invalid config (pruned_degree %u, max_degree %u (provider %u), l_build %u, alpha %g)", what,
                  cfg->pruned_degree, cfg->max_degree, idx->cfg.max_degree, cfg->l_build, (double)cfg->alpha);
        return DANN_EINVAL;
    }
    if (cfg->max_occlusion_size > kMaxPool) {
        set_error("%s: max_occlusion_size %u exceeds the supported %u", what, cfg->max_occlusion_size, kMaxPool);
        return DANN_EUNSUPPORTED;
    }
    return DANN_OK;
}

// what the host wants from the m insert searches of a slice: comparisons, hops, the first search that failed -- three
// words instead of m records through a pageable copy (327 KB per 16 384-point batch)
__global__ __launch_bounds__(256) void stats_reduce_kernel(const dann_search_stats* st, uint32_t m, unsigned long long* sums,
                                                           uint32_t* first_failed) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long c = 0, h = 0;
    uint32_t f = 0;  // m - index of a failed search (0: none): the maximum names the first one
    if (i < m) {
        c = st[i].cmps;
        h = st[i].hops;
        f = st[i].status ? m - i : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o);
        h += __shfl_xor(h, o);
        f = max(f, (uint32_t)__shfl_xor((int)f, o));
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(sums, c);
        atomicAdd(sums + 1, h);
        if (f) atomicMax(first_failed, f);
    }
}

// ---- one multi_insert batch in two phases, everything on the index stream -------------------------
// Phase 1 (candidate generation, index.rs:349-434): insert-time search + RobustPrune for the batch
// positions [lo, hi); writes (hi - lo) rows [len, ids...] of `pend_stride` u32 to d_pending_out.
// Only reads the graph, so ranks holding identical replicas can each take a slice of the batch.
static int32_t batch_candidates(dann_index* idx, const dann_build_config& cfg, BuildScratch& s,
                                const uint32_t* d_slots, uint32_t n, uint32_t lo, uint32_t hi,
                                uint32_t* d_pending_out) {
    const IndexView ix = idx->view();
    PruneCfg pc = to_prune_cfg(idx, cfg);
    pc.counters = s.counters.as<unsigned long long>();
    hipStream_t st = idx->main.stream;
    const uint32_t m = hi - lo;
    if (m == 0) return DANN_OK;
    const uint32_t cand = cfg.intra_batch_candidates == 0xFFFFFFFFu ? n : std::min(cfg.intra_batch_candidates, n);
    const uint32_t nex = (cand != 0 && n > 1) ? std::min(cand, n - 1) : 0;
    SearchArgs sa;
    sa.ix = ix;
    sa.qslots = d_slots + lo;
    sa.nq = m;
    sa.l_value = cfg.l_build;
    sa.beam_width = 1;
    sa.ht_entries = auto_visited_entries(idx, cfg.l_build, 1);
    sa.stats = s.stats.as<dann_search_stats>();
    sa.rec_ids = s.rec_ids.as<uint32_t>();
    sa.rec_dists = s.rec_d.as<float>();
    sa.rec_stride = s.rec_stride;
    sa.rec_n = s.rec_n.as<uint32_t>();
    uint32_t* meta = s.meta.as<uint32_t>();  // [0] nseg [1] nkeys [2] maxseg [3] err [4] appends [5] prunes [6] max record
    DANN_HIP(hipMemsetAsync(meta, 0, 128, st));
    sa.rec_max = meta + 6;
    int32_t rc = search_with_retry(idx, idx->main, sa);
    if (rc != DANN_OK) return rc;
    // the pool's LDS footprint follows the longest record of this batch, not the worst-case bound
    uint32_t h_recmax = 0;
    DANN_HIP(hipMemcpyAsync(&h_recmax, meta + 6, 4, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    h_recmax = std::min<uint32_t>(std::max<uint32_t>(h_recmax, 32), s.rec_stride);
    PoolArgs pa;
    pa.ix = ix;
    pa.cfg = pc;
    pa.locs = d_slots;
    pa.pool_ids = s.rec_ids.as<uint32_t>();
    pa.pool_d = s.rec_d.as<float>();
    pa.offsets = nullptr;
    pa.stride = s.rec_stride;
    pa.counts = s.rec_n.as<uint32_t>();
    pa.cand = cand;
    pa.n = n;
    pa.pos0 = lo;
    pa.pcap = pow2_at_least(h_recmax + nex);
    pa.force_saturate = 0;
    pa.out = d_pending_out;
    pa.out_stride = s.pend_stride;
    pa.err = meta + 3;
    if (pa.pcap > kMaxPool) {
        set_error("candidate pool bound %u exceeds %u: lower l_build or intra_batch_candidates", pa.pcap, kMaxPool);
        return DANN_EUNSUPPORTED;
    }
    // matrix-core path (three kernels: sort, Gram tiles, sweep).  Default for float rows of 1 KiB and more unless
    // DANN_BUILD_ROW_KERNEL_ONLY is set; DANN_BUILD_MFMA_POOL forces it for any row size.
    const bool want_pool_gram = gram_float_rows(ix) && ((idx->build_flags & DANN_BUILD_MFMA_POOL) ||
                                                        (!(idx->build_flags & DANN_BUILD_ROW_KERNEL_ONLY) &&
                                                         ix.layer_bytes >= 1024u && pool_gram_default(idx)));
    if (want_pool_gram) {
        const uint32_t mg = gram_cols(idx);
        const uint32_t ng = std::max<uint32_t>(mg, std::min<uint32_t>(32u * kTileRowBlocks, (h_recmax + nex + 31u) & ~31u));
        rc = ensure_gram_scratch(s, m, pa.pcap, ng, mg);
        if (rc != DANN_OK) return rc;
        rc = launch_pool_sort(s, pa, m, st);
        if (rc != DANN_OK) return rc;
        rc = gram_tiles_and_sweep(idx, s, pa, m, ng, mg, nullptr);
    } else {
        rc = launch_pool_prune(pa, m, st);
    }
    if (rc != DANN_OK) return rc;
    hipLaunchKernelGGL(stats_reduce_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, s.stats.as<dann_search_stats>(), m,
                       reinterpret_cast<unsigned long long*>(meta + 16), meta + 15);
    // meta[3 .. 19] in one copy: [0] the pool overflow flag (meta[3]), [12] the first failed search (meta[15]), [13 .. 16]
    // the two 64-bit totals (meta[16 .. 19])
    struct {
        uint32_t w[17];
    } h_tail = {};
    DANN_HIP(hipMemcpyAsync(h_tail.w, meta + 3, sizeof(h_tail.w), hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    unsigned long long h_sums[2];
    memcpy(h_sums, h_tail.w + 13, sizeof(h_sums));
    if (h_tail.w[0]) {
        set_error("candidate pool overflow in prune (pool cap %u)", pa.pcap);
        return DANN_EOVERFLOW;
    }
    idx->build_counters[2] += h_sums[0];
    idx->build_counters[3] += h_sums[1];
    if (h_tail.w[12]) {
        set_error("insert search %u: visited table or record buffer exhausted", lo + (m - h_tail.w[12]));
        return DANN_EOVERFLOW;
    }
    return DANN_OK;
}

// Phase 2 (graph update, index.rs:911-1024): back-edge aggregation, bootstrap when the graph is
// nearly empty, set_neighbors_bulk, add_edge_and_prune per distinct target.  Deterministic given the
// pending rows of the *whole* batch, so identical replicas stay identical.
static int32_t batch_commit(dann_index* idx, const dann_build_config& cfg, BuildScratch& s, const uint32_t* d_slots,
                            uint32_t n, const uint32_t* d_pending, uint32_t rank = 0, uint32_t world = 1,
                            uint32_t* d_rows_out = nullptr, uint32_t rows_cap = 0, uint32_t* count_out = nullptr,
                            uint32_t backedge_limit = 0xFFFFFFFFu) {
    if (count_out) *count_out = 0;
    s.bootstrap_too_big = false;
    const IndexView ix = idx->view();
    PruneCfg pc = to_prune_cfg(idx, cfg);
    pc.counters = s.counters.as<unsigned long long>();
    hipStream_t st = idx->main.stream;
    const uint32_t cand = cfg.intra_batch_candidates == 0xFFFFFFFFu ? n : std::min(cfg.intra_batch_candidates, n);
    uint32_t* meta = s.meta.as<uint32_t>();
    const uint32_t* pending = d_pending;
    int32_t rc;
    auto aggregate = [&](uint32_t* h_meta) -> int32_t {
        const uint32_t total = n * s.degree;
        DANN_HIP(hipMemsetAsync(meta, 0, 12, st));  // nseg, nkeys, maxseg -- the error word meta[3] is sticky
        launch_make_keys(d_slots, pending, s.pend_stride, n, s.degree, s.keys_in.as<uint64_t>(), backedge_limit, st);
        size_t tmp = s.sort_tmp_bytes;
        DANN_HIP(hipcub::DeviceRadixSort::SortKeys(s.sort_tmp.p, tmp, s.keys_in.as<uint64_t>(),
                                                   s.keys_out.as<uint64_t>(), (int)total, 0, 64, st));
        launch_segments(s.keys_out.as<uint64_t>(), total, s.seg_start.as<uint32_t>(), s.seg_len.as<uint32_t>(), meta, st);
        DANN_HIP(hipMemcpyAsync(h_meta, meta, 16, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
        return DANN_OK;
    };
    uint32_t h_meta[4] = {0, 0, 0, 0};
    // err, appends, prunes, longest record, pad: a commit does not inherit the error word of an earlier call on this
    // handle (phase 1 reports its own errors before it returns); within the commit the word stays sticky
    DANN_HIP(hipMemsetAsync(meta + 3, 0, 20, st));
    rc = aggregate(h_meta);
    if (rc != DANN_OK) return rc;

    // ---- bootstrap (index.rs:926-938) -----------------------------------------------------------------
    const uint32_t resolved = std::max<uint32_t>(cand, 1);
    if (resolved < n && (h_meta[0] + 7) / 8 <= n) {
        ListArgs la;
        la.ix = ix;
        la.cfg = pc;
        la.locs = d_slots;
        la.pending = pending;
        la.pend_stride = s.pend_stride;
        la.n = n;
        la.pcap = pow2_at_least(pc.pruned_degree + n);
        la.out = s.pending2.as<uint32_t>();
        la.out_stride = s.pend_stride;
        la.err = meta + 3;
        if (la.pcap > kMaxPool) {
            // nothing has been written to the graph yet: the caller may insert the same points in smaller batches
            s.bootstrap_too_big = true;
            set_error("bootstrap of a %u-point batch into a nearly empty graph is not supported (cap %u); "
                      "use a geometric batch schedule (dann_build)", n, kMaxPool);
            return DANN_EUNSUPPORTED;
        }
        rc = launch_bootstrap(la, st);
        if (rc != DANN_OK) return rc;
        pending = s.pending2.as<uint32_t>();
        rc = aggregate(h_meta);
        if (rc != DANN_OK) return rc;
        if (h_meta[3]) {
            set_error("candidate pool overflow in bootstrap prune");
            return DANN_EOVERFLOW;
        }
    }

    // ---- graph update -------------------------------------------------------------------------------------
    launch_set_bulk(ix, d_slots, pending, s.pend_stride, n, st);
    if (h_meta[0]) {
        BackArgs ba;
        ba.ix = ix;
        ba.cfg = pc;
        ba.keys = s.keys_out.as<uint64_t>();
        ba.seg_start = s.seg_start.as<uint32_t>();
        ba.seg_len = s.seg_len.as<uint32_t>();
        ba.nseg = h_meta[0];
        ba.nkeys = h_meta[1];
        ba.pcap = 0;  // set per launch below
        ba.err = meta + 3;
        ba.work = nullptr;
        DANN_HIP(hipMemsetAsync(meta + 10, 0, 12, st));  // worklist counts
        // (1) every target: append if the list still fits, else queue it.  Lists of up to `short_cap` entries go
        //     to the short worklist (pool of 128 slots: full occupancy, and the MFMA path when it applies), the
        //     rare long ones (hubs hit by many back-edges in one batch) to a launch of their own whose LDS pool
        //     is sized by the longest of them -- one hub no longer sets the occupancy of the whole batch.
        // default policy: rows of 1 KiB and more (where it is measured to win: 1 M x 768 build 3.50 -> 3.24 s) take the
        // MFMA path unless DANN_BUILD_ROW_KERNEL_ONLY is set; DANN_BUILD_MFMA_BACKEDGE forces it for any row size
        const bool want_gram = prune_pools_use_gram(idx);
        // Gram rows per list: degree + 8 rounded up (96 at R = 64) covers the lists of a steady-state batch; the tiles kernel
        // could take up to 256, but sizing every list's LDS pool and Gram stride for the rare hub costs more than the hubs
        // save (1 M x 768: 3.18 s at 256 against 2.81 s; DANN_DBG_BACKEDGE_GRAM_ROWS raises it for experiments).  Longer
        // lists stay on the row kernel.
        uint32_t pg = std::min<uint32_t>(128u, (ix.max_degree + 8u + 31u) & ~31u);
        if (want_gram) {
            if (const uint32_t e = idx->dbg_u32(DANN_DBG_BACKEDGE_GRAM_ROWS, 0u))
                pg = std::min<uint32_t>(32u * kTileRowBlocks, std::max<uint32_t>(pg, (e + 31u) & ~31u));
        }
        const uint32_t short_pcap = pow2_at_least(std::max<uint32_t>(pg, ix.max_degree + 1u));
        const uint32_t short_cap = want_gram ? pg : short_pcap;
        // small rows without the MFMA path: the single-kernel form (list build + prune per target, its LDS pool sized by
        // the longest list of the batch) only while that pool is small.  One hub with a thousand back-edges in a batch
        // (the 65 536-point batches of a 10 M-point build) sizes EVERY workgroup's LDS for its list -- 2 - 5 lists per CU
        // instead of 20: the phase was 60 % of the 10 M x 128 build (6.2 of 10.3 s).  Beyond kSinglePool entries the split
        // form runs the short lists at full occupancy and the hubs in a launch of their own.  Measured, round 5
        // (scratch/r05_backedge_ab.sh; pool limit 8192 / 512 / 256 / 128 / 64): 10 M x 128 build 10.2 / 6.6 / 6.0 / 6.0 /
        // 6.0 s, 1 M x 128 build 0.64 / 0.64 / 0.62 / 0.61 / 0.61 s (round 2 had measured the split form slower at 1 M:
        // 0.78 against 0.68 s, before the scan kernel served four targets per wavefront).  Rows of 1 KiB and more always
        // take the split form (1 M x 768: 5.2 s -> 3.5 s, 3.25 s with the MFMA path).
        const uint32_t pcap_all = pow2_at_least(ix.max_degree + h_meta[2]);
        const uint32_t single_pool = idx->dbg_u32(DANN_DBG_BACKEDGE_SINGLE_POOL, 128u);
        if (!want_gram && ix.layer_bytes < 1024u && world <= 1u && pcap_all <= single_pool) {
            if (pcap_all > kMaxPool) {
                set_error("a node received %u back-edges in one batch (cap %u): lower max_batch", h_meta[2], kMaxPool);
                return DANN_EOVERFLOW;
            }
            ba.pcap = pcap_all;
            rc = launch_backedge(ba, st);
            if (rc != DANN_OK) return rc;
        } else {
        uint32_t* work = s.seg_len.as<uint32_t>() + (size_t)n * s.degree;  // 2 x nseg entries behind seg_len
        ScanArgs sa;
        sa.ix = ix;
        sa.cfg_max_degree = pc.max_degree;
        sa.keys = ba.keys;
        sa.seg_start = ba.seg_start;
        sa.seg_len = ba.seg_len;
        sa.nseg = ba.nseg;
        sa.short_cap = short_cap;
        sa.work_short = work;
        sa.work_long = work + ba.nseg;
        sa.counts = meta + 10;
        sa.rank = rank;
        sa.world = world;
        launch_backedge_scan(sa, st);
        uint32_t h_counts[3] = {0, 0, 0};
        DANN_HIP(hipMemcpyAsync(h_counts, meta + 10, 12, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
        // (2) long lists first, on the side stream: every list belongs to another target row and a prune reads vector rows
        //     and its own list only, so the two classes do not depend on each other.  A launch of these is as long as its
        //     longest list (1 M x 768: 1.7 ms on average, 170 ms of a 2.4 s build, with a handful of CUs busy: some fifty
        //     hubs per 16 384-point batch, the longest with ~2 000 back-edges -- far beyond the 256 rows of a Gram block).
        hipStream_t side = nullptr;
        bool side_busy = false;
        struct SideGuard {  // an error return below must not leave the side stream working on this scratch
            hipStream_t& s;
            bool& busy;
            ~SideGuard() {
                if (busy) (void)hipStreamSynchronize(s);
            }
        } side_guard{side, side_busy};
        if (h_counts[1]) {
            BackArgs bl = ba;
            bl.work = work + ba.nseg;
            bl.nseg = h_counts[1];
            bl.pcap = pow2_at_least(h_counts[2]);
            bl.count_long = want_gram ? 1u : 0u;
            if (bl.pcap > kMaxPool) {
                set_error("a node received back-edges for a list of %u entries in one batch (cap %u): lower max_batch",
                          h_counts[2], kMaxPool);
                return DANN_EOVERFLOW;
            }
            hipStream_t run_on = st;
            if (h_counts[0]) {  // (with no short lists there is nothing to run beside)
                if (int32_t src = s.side_stream(&side)) return src;
                run_on = side;
                side_busy = true;
            }
            rc = launch_backedge(bl, run_on);
            if (rc != DANN_OK) return rc;
        }
        // (3) short lists
        if (h_counts[0]) {
            BackArgs bs = ba;
            bs.work = work;
            bs.nseg = h_counts[0];
            bs.pcap = short_pcap;
            if (want_gram && pg > ix.max_degree) {
                // three kernels: list + d(target, c) + sort; Gram tiles of the sorted list on the matrix cores; sweep
                const uint32_t nshort = h_counts[0], mg = std::min<uint32_t>(pg, 32u * kTileColBlocks);
                rc = ensure_gram_scratch(s, nshort, bs.pcap, pg, mg);
                if (rc != DANN_OK) return rc;
                rc = launch_backedge_list(s, bs, nshort, st);
                if (rc != DANN_OK) return rc;
                PoolArgs sp{};  // what the sweep reads of it (the lists and their targets come from the scratch)
                sp.ix = ix;
                sp.cfg = pc;
                sp.pcap = bs.pcap;
                sp.force_saturate = 0;
                rc = gram_tiles_and_sweep(idx, s, sp, nshort, pg, mg, s.g_loc.as<uint32_t>());
            } else {
                rc = launch_backedge(bs, st);
            }
            if (rc != DANN_OK) return rc;
        }
        if (side_busy) {  // both classes of lists are written before the rows are exported / the counters are read
            side_busy = false;
            DANN_HIP(hipStreamSynchronize(side));
        }
        if (world > 1u) {  // the rows this rank owns and has just rewritten, for the other replicas
            const uint32_t cnt = h_counts[0] + h_counts[1];
            if (cnt > rows_cap || (cnt && !d_rows_out)) {
                set_error("partitioned commit: %u rewritten rows exceed the export buffer (%u)", cnt, rows_cap);
                return DANN_EOVERFLOW;
            }
            if (cnt) launch_export_rows(ix, ba.keys, ba.seg_start, work, h_counts[0], work + ba.nseg, h_counts[1], d_rows_out, st);
            if (count_out) *count_out = cnt;
        }
        }
    }
    uint32_t h_tail[1] = {0};  // meta[3]: err
    DANN_HIP(hipMemcpyAsync(h_tail, meta + 3, sizeof(h_tail), hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    if (h_tail[0]) {
        set_error("back-edge list overflow");
        return DANN_EOVERFLOW;
    }
    return DANN_OK;
}

static int32_t insert_batch_device(dann_index* idx, const dann_build_config& cfg, BuildScratch& s,
                                   const uint32_t* d_slots, uint32_t n, uint32_t backedge_limit = 0xFFFFFFFFu) {
    int32_t rc = batch_candidates(idx, cfg, s, d_slots, n, 0, n, s.pending.as<uint32_t>());
    if (rc != DANN_OK) return rc;
    return batch_commit(idx, cfg, s, d_slots, n, s.pending.as<uint32_t>(), 0, 1, nullptr, 0, nullptr, backedge_limit);
}

}  // namespace dann

using namespace dann;

namespace dann {
// the last commit on this handle stopped because its batch needs a bootstrap larger than one prune pool (nothing was
// written to the graph): the callers that own a batch schedule (dann_build, dann_build_sharded) halve the batch
bool build_bootstrap_too_big(dann_index* idx) {
    return idx->build_scratch && static_cast<BuildScratch*>(idx->build_scratch)->bootstrap_too_big;
}
}  // namespace dann

static BuildScratch& scratch_of(dann_index* idx) {
    if (!idx->build_scratch) {
        idx->build_scratch = new BuildScratch();
        idx->build_scratch_free = [](void* p) { delete static_cast<BuildScratch*>(p); };
    }
    return *static_cast<BuildScratch*>(idx->build_scratch);
}

namespace dann {
// the back-edge policy (batch_commit): float rows of 1 KiB and more, or DANN_BUILD_MFMA_BACKEDGE, unless
// DANN_BUILD_ROW_KERNEL_ONLY
bool prune_pools_use_gram(const dann_index* idx) {
    const IndexView ix = idx->view();
    return gram_float_rows(ix) && ((idx->build_flags & DANN_BUILD_MFMA_BACKEDGE) ||
                                   (!(idx->build_flags & DANN_BUILD_ROW_KERNEL_ONLY) && ix.layer_bytes >= 1024u));
}

// robust_prune_list (index.rs:2397-2454) with force_saturate = false over m caller-built pools, for graph consolidation
// (consolidate.hip).  Pool i: ids[i * stride + j] and their distances to locs[i], j < counts[i], in pool order (the
// order SortedNeighbors::new receives them in); the pruned list is written straight into locs[i]'s adjacency row, an empty
// pool leaves its row alone.  stride is a power of two >= every count and <= kMaxPool.  The same kernels as the back-edge
// prunes: the row kernel (pool_prune_kernel) or, where dann_set_build_options picks the matrix cores for back-edges, sort +
// Gram tiles + sweep.  Queued on the index stream, nothing waited for.  *used_gram: whether the MFMA path ran.
int32_t prune_pools_into_rows(dann_index* idx, const dann_build_config& cfg, const uint32_t* d_locs, const uint32_t* d_ids,
                              const float* d_dists, const uint32_t* d_counts, uint32_t stride, uint32_t m, bool* used_gram) {
    *used_gram = false;
    if (m == 0) return DANN_OK;
    if (stride > kMaxPool || (stride & (stride - 1u))) {
        set_error("prune_pools_into_rows: pool stride %u", stride);
        return DANN_EINTERNAL;
    }
    BuildScratch& s = scratch_of(idx);
    if (!s.counters.p) {
        DANN_HIP(s.counters.alloc((size_t)kStatStripes * 64 + 64));
        DANN_HIP(hipMemset(s.counters.p, 0, (size_t)kStatStripes * 64 + 64));
    }
    if (!s.meta.p) {
        DANN_HIP(s.meta.alloc(128));
        DANN_HIP(hipMemset(s.meta.p, 0, 128));
    }
    const IndexView ix = idx->view();
    PruneCfg pc = to_prune_cfg(idx, cfg);
    pc.counters = s.counters.as<unsigned long long>();
    hipStream_t st = idx->main.stream;
    PoolArgs pa;
    pa.ix = ix;
    pa.cfg = pc;
    pa.locs = d_locs;
    pa.pool_ids = d_ids;
    pa.pool_d = d_dists;
    pa.offsets = nullptr;
    pa.stride = stride;
    pa.counts = d_counts;
    pa.cand = 0;
    pa.n = m;
    pa.pos0 = 0;
    pa.pcap = stride;
    pa.force_saturate = 0;
    pa.out = nullptr;
    pa.out_stride = 0;
    pa.err = s.meta.as<uint32_t>() + 3;
    pa.into_rows = 1;
    if (!prune_pools_use_gram(idx)) return launch_pool_prune(pa, m, st);
    const uint32_t mg = gram_cols(idx);
    const uint32_t ng = std::max<uint32_t>(mg, std::min<uint32_t>(32u * kTileRowBlocks, stride));
    int32_t rc = ensure_gram_scratch(s, m, stride, ng, mg);
    if (rc != DANN_OK) return rc;
    rc = launch_pool_sort(s, pa, m, st);
    if (rc != DANN_OK) return rc;
    rc = gram_tiles_and_sweep(idx, s, pa, m, ng, mg, d_locs);
    if (rc != DANN_OK) return rc;
    *used_gram = true;
    return DANN_OK;
}
}  // namespace dann

extern "C" {

int32_t dann_insert_batch(dann_index* idx, const dann_build_config* cfg, const uint32_t* slots, uint32_t n) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    DeviceGuard guard(idx->device);
    int32_t rc = check_build_cfg(idx, cfg, "dann_insert_batch", true);
    if (rc != DANN_OK) return rc;
    if (n == 0) return DANN_OK;
    if (!slots) return DANN_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (slots[i] >= idx->cfg.capacity) {
            set_error("slot %u out of bounds (capacity %u)", slots[i], idx->cfg.capacity);
            return DANN_EBOUNDS;
        }
    BuildScratch& s = scratch_of(idx);
    const uint32_t rec_stride = 4 * (cfg->l_build + idx->cfg.num_start_points) + 64;
    rc = ensure_scratch(s, n, rec_stride, cfg->pruned_degree);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(s.slots.p, slots, (size_t)n * 4, hipMemcpyHostToDevice, idx->main.stream));
    return insert_batch_device(idx, *cfg, s, s.slots.as<uint32_t>(), n);
} DANN_CATCH_ALL

// DiskANNIndex::insert (index.rs:226-341): the insert search, the prune, set_neighbors, then add_edge_and_prune for the
// first max_backedges of the new neighbours (:324-327) -- a multi_insert of one point whose back-edges stop there.
int32_t dann_insert(dann_index* idx, const dann_build_config* cfg, uint32_t slot) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    DeviceGuard guard(idx->device);
    int32_t rc = check_build_cfg(idx, cfg, "dann_insert", true);
    if (rc != DANN_OK) return rc;
    if (cfg->max_backedges > cfg->pruned_degree) {  // config/mod.rs:308-311
        set_error("parameter \"max_backedges\" (%u) must not be greater than \"pruned_degree\" (%u)", cfg->max_backedges,
                  cfg->pruned_degree);
        return DANN_EINVAL;
    }
    if (slot >= idx->cfg.capacity) {
        set_error("slot %u out of bounds (capacity %u)", slot, idx->cfg.capacity);
        return DANN_EBOUNDS;
    }
    BuildScratch& s = scratch_of(idx);
    const uint32_t rec_stride = 4 * (cfg->l_build + idx->cfg.num_start_points) + 64;
    rc = ensure_scratch(s, 1, rec_stride, cfg->pruned_degree);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(s.slots.p, &slot, 4, hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));  // (`slot` lives on this frame)
    return insert_batch_device(idx, *cfg, s, s.slots.as<uint32_t>(), 1, cfg->max_backedges ? cfg->max_backedges : cfg->pruned_degree);
} DANN_CATCH_ALL

// multi-GPU build: phase 1 on a slice of the batch, phase 2 with the all-gathered pending rows.
// d_pending_* are DEVICE pointers ((pruned_degree + 1) u32 per row) so that they can be the send /
// receive buffers of an RCCL all-gather.
int32_t dann_insert_batch_candidates(dann_index* idx, const dann_build_config* cfg, const uint32_t* slots, uint32_t n,
                                     uint32_t lo, uint32_t hi, uint32_t* d_pending_out) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DeviceGuard guard(idx->device);
    int32_t rc = check_build_cfg(idx, cfg, "dann_insert_batch_candidates", true);
    if (rc != DANN_OK) return rc;
    if (lo > hi || hi > n) return DANN_EINVAL;
    if (n == 0 || lo == hi) return DANN_OK;
    if (!slots || !d_pending_out) return DANN_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (slots[i] >= idx->cfg.capacity) return DANN_EBOUNDS;
    BuildScratch& s = scratch_of(idx);
    const uint32_t rec_stride = 4 * (cfg->l_build + idx->cfg.num_start_points) + 64;
    rc = ensure_scratch(s, n, rec_stride, cfg->pruned_degree);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(s.slots.p, slots, (size_t)n * 4, hipMemcpyHostToDevice, idx->main.stream));
    return batch_candidates(idx, *cfg, s, s.slots.as<uint32_t>(), n, lo, hi, d_pending_out);
} DANN_CATCH_ALL

int32_t dann_insert_batch_commit(dann_index* idx, const dann_build_config* cfg, const uint32_t* slots, uint32_t n,
                                 const uint32_t* d_pending_all) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    DeviceGuard guard(idx->device);
    int32_t rc = check_build_cfg(idx, cfg, "dann_insert_batch_commit", true);
    if (rc != DANN_OK) return rc;
    if (n == 0) return DANN_OK;
    if (!slots || !d_pending_all) return DANN_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (slots[i] >= idx->cfg.capacity) return DANN_EBOUNDS;
    BuildScratch& s = scratch_of(idx);
    const uint32_t rec_stride = 4 * (cfg->l_build + idx->cfg.num_start_points) + 64;
    rc = ensure_scratch(s, n, rec_stride, cfg->pruned_degree);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(s.slots.p, slots, (size_t)n * 4, hipMemcpyHostToDevice, idx->main.stream));
    return batch_commit(idx, *cfg, s, s.slots.as<uint32_t>(), n, d_pending_all);
} DANN_CATCH_ALL

int32_t dann_insert_batch_commit_part(dann_index* idx, const dann_build_config* cfg, const uint32_t* slots, uint32_t n,
                                      const uint32_t* d_pending_all, uint32_t rank, uint32_t world, uint32_t* d_rows_out,
                                      uint32_t rows_cap, uint32_t* count_out) try {
    if (!idx || !count_out || world == 0 || rank >= world) return DANN_EINVAL;
    *count_out = 0;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    DeviceGuard guard(idx->device);
    int32_t rc = check_build_cfg(idx, cfg, "dann_insert_batch_commit_part", true);
    if (rc != DANN_OK) return rc;
    if (n == 0) return DANN_OK;
    if (!slots || !d_pending_all) return DANN_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (slots[i] >= idx->cfg.capacity) return DANN_EBOUNDS;
    BuildScratch& s = scratch_of(idx);
    const uint32_t rec_stride = 4 * (cfg->l_build + idx->cfg.num_start_points) + 64;
    rc = ensure_scratch(s, n, rec_stride, cfg->pruned_degree);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(s.slots.p, slots, (size_t)n * 4, hipMemcpyHostToDevice, idx->main.stream));
    rc = batch_commit(idx, *cfg, s, s.slots.as<uint32_t>(), n, d_pending_all, rank, world, d_rows_out, rows_cap, count_out);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipStreamSynchronize(idx->main.stream));  // the exported rows are read by the caller's collective next
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_apply_neighbor_rows_device(dann_index* idx, const uint32_t* d_rows, uint32_t count) try {
    if (!idx || (count && !d_rows)) return DANN_EINVAL;
    if (count == 0) return DANN_OK;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    DeviceGuard guard(idx->device);
    launch_apply_rows(idx->view(), d_rows, count, idx->main.stream);
    DANN_HIP(hipGetLastError());
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_set_build_options(dann_index* idx, uint32_t flags) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    idx->build_flags = flags;
    return DANN_OK;
} DANN_CATCH_ALL

}  // extern "C"
// dann_kernel_time(which = 5): the gram_tiles_kernel launches of this index's builds (all pending events resolved)
int32_t dann::build_tile_clock(const dann_index* idx, double* total_ms, uint64_t* launches) {
    if (total_ms) *total_ms = 0.0;
    if (launches) *launches = 0;
    if (!idx->build_scratch) return DANN_OK;
    BuildScratch& s = *static_cast<BuildScratch*>(idx->build_scratch);
    DeviceGuard guard(idx->device);
    s.tile_drain(true);
    if (total_ms) *total_ms = s.tile_ms;
    if (launches) *launches = s.tile_launches;
    return DANN_OK;
}
void dann::build_tile_clock_reset(const dann_index* idx) {
    if (!idx->build_scratch) return;
    BuildScratch& s = *static_cast<BuildScratch*>(idx->build_scratch);
    s.tile_drain(true);
    s.tile_ms = 0.0;
    s.tile_launches = 0;
}
extern "C" {

int32_t dann_build_counters(const dann_index* idx, uint64_t* out, uint32_t n) try {
    if (!idx || (n && !out)) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    uint64_t dev[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sort_fallbacks = 0;
    if (idx->build_scratch) {
        BuildScratch& s = *static_cast<BuildScratch*>(idx->build_scratch);
        if (s.counters.p) {
            DeviceGuard guard(idx->device);
            DANN_HIP(hipStreamSynchronize(idx->main.stream));
            std::vector<uint64_t> stripes((size_t)kStatStripes * 8 + 8);
            DANN_HIP(hipMemcpy(stripes.data(), s.counters.p, stripes.size() * 8, hipMemcpyDeviceToHost));
            for (uint32_t t = 0; t < kStatStripes; ++t)
                for (uint32_t c = 0; c < 8; ++c) dev[c] += stripes[(size_t)t * 8 + c];
            sort_fallbacks = stripes[(size_t)kStatStripes * 8];
        }
    }
    const uint64_t all[11] = {dev[6], dev[7], idx->build_counters[2], idx->build_counters[3],
                              dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], sort_fallbacks};
    for (uint32_t i = 0; i < n; ++i) out[i] = i < 11 ? all[i] : 0u;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_build(dann_index* idx, const dann_build_config* cfg, uint32_t first, uint32_t n, float growth,
                   uint32_t max_batch) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    DeviceGuard guard(idx->device);
    int32_t rc = check_build_cfg(idx, cfg, "dann_build", true);
    if (rc != DANN_OK) return rc;
    if ((uint64_t)first + n > idx->cfg.capacity) return DANN_EBOUNDS;
    if (!(growth > 0.0f) || max_batch == 0) return DANN_EINVAL;
    BuildScratch& s = scratch_of(idx);
    const uint32_t rec_stride = 4 * (cfg->l_build + idx->cfg.num_start_points) + 64;
    rc = ensure_scratch(s, std::min(max_batch, n ? n : 1u), rec_stride, cfg->pruned_degree);
    if (rc != DANN_OK) return rc;
    std::vector<uint32_t> ids;
    uint32_t done = 0;
    int32_t batches = 0;
    uint32_t limit = max_batch;  // shrinks when a batch turns out to need a bootstrap larger than the pool
    while (done < n) {
        // geometric schedule: batch = clamp(ceil(inserted * growth), 1, max_batch)
        uint32_t b = (uint32_t)std::ceil((double)(first + done) * (double)growth);
        b = std::max<uint32_t>(1, std::min(b, limit));
        b = std::min(b, n - done);
        ids.resize(b);
        for (uint32_t i = 0; i < b; ++i) ids[i] = first + done + i;
        DANN_HIP(hipMemcpyAsync(s.slots.p, ids.data(), (size_t)b * 4, hipMemcpyHostToDevice, idx->main.stream));
        DANN_HIP(hipStreamSynchronize(idx->main.stream));
        s.bootstrap_too_big = false;
        rc = insert_batch_device(idx, *cfg, s, s.slots.as<uint32_t>(), b);
        if (rc == DANN_EUNSUPPORTED && s.bootstrap_too_big && b > 1) {
            // multi_insert's bootstrap test (index.rs:926-931) fired for a batch whose members do not fit one prune
            // pool; the graph is untouched at that point, so the same points go in as two smaller batches
            limit = std::max<uint32_t>(1, b / 2);
            continue;
        }
        if (rc != DANN_OK) return rc;
        limit = std::min<uint32_t>(max_batch, limit * 2 > limit ? limit * 2 : limit);
        done += b;
        ++batches;
    }
    return batches;
} DANN_CATCH_ALL

int32_t dann_prune_batch(dann_index* idx, const dann_build_config* cfg, const uint32_t* locs, uint32_t n,
                         const uint32_t* pool_ids, const float* pool_dists, const uint64_t* offsets,
                         int32_t force_saturate, uint32_t* out_adj) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DeviceGuard guard(idx->device);
    int32_t rc = check_build_cfg(idx, cfg, "dann_prune_batch", true);
    if (rc != DANN_OK) return rc;
    if (n == 0) return DANN_OK;
    if (!locs || !pool_ids || !pool_dists || !offsets || !out_adj) return DANN_EINVAL;
    const uint64_t total = offsets[n];
    uint64_t maxlen = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return DANN_EINVAL;
        maxlen = std::max(maxlen, offsets[i + 1] - offsets[i]);
    }
    for (uint64_t i = 0; i < total; ++i)
        if (pool_ids[i] >= idx->nslots) return DANN_EBOUNDS;
    if (maxlen > kMaxPool) {
        set_error("pool of %llu candidates exceeds the supported %u", (unsigned long long)maxlen, kMaxPool);
        return DANN_EUNSUPPORTED;
    }
    const uint32_t ostride = cfg->pruned_degree + 1;
    DevBuf dl, di, dd, doff, dout, derr;
    DANN_HIP(dl.alloc((size_t)n * 4));
    DANN_HIP(di.alloc(total * 4));
    DANN_HIP(dd.alloc(total * 4));
    DANN_HIP(doff.alloc((size_t)(n + 1) * 8));
    DANN_HIP(dout.alloc((size_t)n * ostride * 4));
    DANN_HIP(derr.alloc(4));
    hipStream_t st = idx->main.stream;
    DANN_HIP(hipMemcpyAsync(dl.p, locs, (size_t)n * 4, hipMemcpyHostToDevice, st));
    DANN_HIP(hipMemcpyAsync(di.p, pool_ids, total * 4, hipMemcpyHostToDevice, st));
    DANN_HIP(hipMemcpyAsync(dd.p, pool_dists, total * 4, hipMemcpyHostToDevice, st));
    DANN_HIP(hipMemcpyAsync(doff.p, offsets, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    DANN_HIP(hipMemsetAsync(derr.p, 0, 4, st));
    PoolArgs pa;
    pa.ix = idx->view();
    pa.cfg = to_prune_cfg(idx, *cfg);
    pa.locs = dl.as<uint32_t>();
    pa.pool_ids = di.as<uint32_t>();
    pa.pool_d = dd.as<float>();
    pa.offsets = doff.as<uint64_t>();
    pa.stride = 0;
    pa.counts = nullptr;
    pa.cand = 0;
    pa.n = n;
    pa.pos0 = 0;
    pa.pcap = pow2_at_least((uint32_t)maxlen);
    pa.force_saturate = force_saturate;
    pa.out = dout.as<uint32_t>();
    pa.out_stride = ostride;
    pa.err = derr.as<uint32_t>();
    rc = launch_pool_prune(pa, n, st);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(out_adj, dout.p, (size_t)n * ostride * 4, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    return DANN_OK;
} DANN_CATCH_ALL

}  // extern "C"
