// search_diverse.hip -- graph::search::Diverse (diskann/src/graph/search/diverse_search.rs:180-233) for a batch of
// independent queries, one wavefront per query.
//
// The beam loop is DiskANNIndex::search_internal (diskann/src/graph/index.rs:1933-2000) unchanged: start points go
// through the queue's insert, each hop pops up to W unexpanded entries, reads their adjacency rows, keeps the ids the
// visited set has not seen (in pop order, then adjacency order), evaluates their distances and inserts them one by one
// -- the diverse queue's outcome depends on that order, so the rank merge of the plain kernels does not apply.  The
// queue is DiverseNeighborQueue (diverse_queue.h); after the loop its post_process runs and the first L entries go
// through the Knn post-processor (start points dropped, the first k kept).
//
// Shared with the plain kernels (search_kernel_impl.h / dann_device.h): query staging, the distance groups of the
// generic-length gather (so every distance has the same bits as the other searches'), the exact LDS visited table
// (ht_insert_open) and the inline-tag test.
//
// Scratch per query: queue, pool and visited table in LDS.  A query whose pool or visited table fills up stops and is
// re-run by the host with the same arrays in global memory, sized so that neither can fill up: the pool holds at most
// one entry per inserted id and the table at most one per slot.  The answer never depends on which run produced it.
#include "diverse_queue.h"
#include "search_kernel_impl.h"

namespace dann {
namespace {

struct DiverseArgs {
    IndexView ix;
    const void* queries;     // nq rows of layer bytes
    const uint32_t* qmap;    // optional: run queries qmap[0 .. nq)
    const uint32_t* attr;    // per-slot attribute (kNoAttribute = none)
    uint32_t nq, l_value, beam_width, k, dk, dl;
    uint32_t ht_entries, ht_prime, pool_cap;
    uint8_t* gws;            // null: scratch in LDS; else per launch slot gws + slot * gws_stride
    uint64_t gws_stride;
    uint32_t* out_ids;
    float* out_dists;
    dann_search_stats* stats;
};

__host__ __device__ inline uint32_t dv_cmax(const IndexView& ix, uint32_t W) {
    const uint32_t c1 = (W * ix.max_degree + 63u) & ~63u, c2 = (ix.nstart + 63u) & ~63u;
    return c1 > c2 ? c1 : c2;
}
// bytes of the queue + pool + visited table (16-byte aligned pieces)
__host__ __device__ inline uint64_t dv_ws_bytes(uint32_t L, uint32_t pool, uint32_t ht) {
    return (uint64_t)round16(L * 4u) * 3u + (uint64_t)round16(pool * 4u) * 4u + (uint64_t)ht * 4u;
}
__host__ __device__ inline uint32_t dv_fixed_lds(const IndexView& ix, uint32_t W) {
    return round16(query_lds_bytes(ix)) + 2u * round16(dv_cmax(ix, W) * 4u);
}

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void diverse_search_kernel(DiverseArgs a) {
    extern __shared__ __align__(16) uint8_t smem[];
    using S = Scheme<DT, OP, false>;
    constexpr int G = S::GS;
    constexpr int GROUPS = kWave / G;
    constexpr bool kInt = S::kInt;
    constexpr int U = S::kWide ? kWideRows : kGatherRows;
    using QT = typename std::conditional<kInt, uint8_t, float>::type;
    using RT = typename RowType<DT>::type;

    const IndexView& ix = a.ix;
    const uint32_t lane = threadIdx.x;
    const uint32_t slot = blockIdx.x;
    const uint32_t qi = a.qmap ? a.qmap[slot] : slot;
    const uint32_t R = ix.max_degree, W = a.beam_width, L = a.l_value;
    const uint32_t cmax = dv_cmax(ix, W);
    const SqParams sqp{ix.sq_k, ix.sq_shift_norm_sq};
    uint32_t off = 0;
    QT* qs = reinterpret_cast<QT*>(smem + query_stage_off(DT));
    off += round16(query_lds_bytes(ix));
    uint32_t* cand_id = reinterpret_cast<uint32_t*>(smem + off);
    off += round16(cmax * 4u);
    float* cand_d = reinterpret_cast<float*>(smem + off);
    off += round16(cmax * 4u);
    uint8_t* ws = a.gws ? a.gws + (uint64_t)slot * a.gws_stride : smem + off;
    DiverseQueue q;
    q.lane = lane;
    q.L = L;
    q.dl = a.dl;
    q.dk = a.dk;
    q.pcap = a.pool_cap;
    {
        uint64_t o = 0;
        q.gd = reinterpret_cast<float*>(ws + o);
        o += round16(L * 4u);
        q.gid = reinterpret_cast<uint32_t*>(ws + o);
        o += round16(L * 4u);
        q.ga = reinterpret_cast<uint32_t*>(ws + o);
        o += round16(L * 4u);
        q.pd = reinterpret_cast<float*>(ws + o);
        o += round16(a.pool_cap * 4u);
        q.pseq = reinterpret_cast<uint32_t*>(ws + o);
        o += round16(a.pool_cap * 4u);
        q.pid = reinterpret_cast<uint32_t*>(ws + o);
        o += round16(a.pool_cap * 4u);
        q.pa = reinterpret_cast<uint32_t*>(ws + o);
        o += round16(a.pool_cap * 4u);
        uint32_t* ht = reinterpret_cast<uint32_t*>(ws + o);
        for (uint32_t i = lane; i < a.ht_entries; i += kWave) ht[i] = kEmpty;
    }
    uint32_t* const ht = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(q.pa) + round16(a.pool_cap * 4u));
    const uint32_t ht_mod = a.ht_prime, ht_open = (uint32_t)((uint64_t)a.ht_prime * 3u / 4u);

    // ---- stage the query (f16 widened to f32 once, integer rows as raw bytes) --------------------------------------
    {
        const uint8_t* qsrc = reinterpret_cast<const uint8_t*>(a.queries) + (uint64_t)qi * ix.qbytes;
        if constexpr (kInt) {
            stage_int_query<DT>(reinterpret_cast<uint8_t*>(qs), qsrc, ix.qbytes, ix.dim, lane, kWave);
        } else {
            const RT* src = reinterpret_cast<const RT*>(qsrc);
            for (uint32_t i = lane; i < ix.dim; i += kWave) reinterpret_cast<float*>(qs)[i] = load1(src + i);
        }
    }
    __syncthreads();

    const int g = lane / G, v = lane % G;
    const uint32_t tag_off = ix.tag_off;
    // distances of cand_id[0 .. nc) -> cand_d, the generic-length gather of beam_search_one; unreadable slots (inline
    // tags) are dropped afterwards, emission order kept.  Returns the candidates kept.
    auto gather = [&](uint32_t nc) -> uint32_t {
        for (uint32_t c0 = 0; c0 < nc; c0 += GROUPS * U) {
            const uint8_t* rows[U];
            bool act[U];
            float out[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t c = c0 + u * GROUPS + g;
                act[u] = c < nc;
                const uint32_t id = act[u] ? cand_id[c] : 0u;
                rows[u] = ix.rows + (uint64_t)id * ix.row_stride;
            }
            uint8_t tg[U];
#pragma unroll
            for (int u = 0; u < U; ++u) tg[u] = (tag_off && act[u] && v == 0) ? rows[u][tag_off] : (uint8_t)255;
            group_distance_many<DT, OP, false, U>(qs, rows, act, (int)ix.dim, v, out);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t c = c0 + u * GROUPS + g;
                if (act[u] && v == 0) {
                    cand_d[c] = finish_distance<DT, OP, NORM>(out[u], reinterpret_cast<const uint8_t*>(qs), rows[u],
                                                              ix.dim, sqp);
                    if (tg[u] < kTagPublished) cand_id[c] = kEmpty;
                }
            }
        }
        __syncthreads();
        if (!tag_off) return nc;
        uint32_t w = 0;
        for (uint32_t c0 = 0; c0 < nc; c0 += kWave) {
            const uint32_t c = c0 + lane;
            const uint32_t id = c < nc ? cand_id[c] : kEmpty;
            const float d = c < nc ? cand_d[c] : 0.0f;
            const bool ok = id != kEmpty;
            const uint64_t m = ballot64(ok);
            __syncthreads();
            if (ok) {
                cand_id[w + mbcnt(m)] = id;
                cand_d[w + mbcnt(m)] = d;
            }
            w += (uint32_t)__popcll(m);
            __syncthreads();
        }
        return w;
    };
    auto attr_of = [&](uint32_t id) -> uint32_t { return a.attr ? a.attr[id] : kNoAttribute; };  // (no store: all None)

    uint32_t cmps = 0, hops = 0, ht_count = 0, status = 0;
    // ---- start points: frozen slots [capacity, capacity + nstart) (index.rs:1950-1958) -------------------------------
    {
        const uint32_t ns = ix.nstart;
        for (uint32_t i = lane; i < ns; i += kWave) {
            cand_id[i] = ix.capacity + i;
            ht_visit(ht, ht_mod, ix.capacity + i, true);
        }
        ht_count = ns;
        __syncthreads();
        const uint32_t nsk = gather(ns);
        if (nsk != ns) status = (uint32_t)(-DANN_EINVAL);  // "could not retrieve start point" (provider.rs:408-431)
        cmps = nsk;
        for (uint32_t c = 0; c < nsk && !q.overflow; ++c) {
            const uint32_t id = cand_id[c];
            q.insert(id, cand_d[c], attr_of(id));
        }
    }
    // ---- beam loop -----------------------------------------------------------------------------------------------------
    while (!status && !q.overflow && q.has_notvisited()) {
        uint32_t nb = 0;
        uint32_t nodes[kMaxBeam];
        while (nb < W && q.has_notvisited()) nodes[nb++] = q.closest_notvisited();
        // expand_beam: not-yet-visited neighbours of each node in pop order, adjacency order within a node
        uint32_t nc = 0;
        for (uint32_t b = 0; b < nb && !status; ++b) {
            const uint32_t* prow = ix.adj + (uint64_t)nodes[b] * ix.adj_stride;
            uint32_t len = prow[0];
            len = len < R ? len : R;
            for (uint32_t j0 = 0; j0 < len; j0 += kWave) {
                if (ht_count + kWave > ht_open) {  // the table could fill up: re-run with a larger one
                    status = (uint32_t)(-DANN_EOVERFLOW);
                    break;
                }
                const uint32_t j = j0 + lane;
                const uint32_t id = j < len ? prow[1 + j] : kEmpty;
                const bool ok = j < len && id < ix.nslots;
                const bool isnew = ht_insert_open(ht, ht_mod, id, ok);
                const uint64_t m = ballot64(isnew);
                if (isnew) cand_id[nc + mbcnt(m)] = id;
                nc += (uint32_t)__popcll(m);
                ht_count += (uint32_t)__popcll(m);
            }
        }
        if (status) break;
        __syncthreads();
        const uint32_t nk = gather(nc);
        for (uint32_t c = 0; c < nk && !q.overflow; ++c) {
            const float d = cand_d[c];
            if (q.can_skip(d)) continue;
            const uint32_t id = cand_id[c];
            q.insert(id, d, attr_of(id));
        }
        cmps += nk;
        hops += nb;
    }
    if (q.overflow) status = (uint32_t)(-DANN_EOVERFLOW);
    if (!status) q.post_process();

    // ---- Knn post-processing: best.iter().take(L), start points dropped, the first k written -------------------------
    uint32_t* oi = a.out_ids + (uint64_t)qi * a.k;
    float* od = a.out_dists + (uint64_t)qi * a.k;
    uint32_t written = 0;
    const uint32_t lim = status ? 0u : (q.gsize < L ? q.gsize : L);
    for (uint32_t i0 = 0; i0 < lim && written < a.k; i0 += kWave) {
        const uint32_t i = i0 + lane;
        const uint32_t id = i < lim ? (q.gid[i] & ~kVisitedBit) : kEmpty;
        const bool res = i < lim && id < ix.capacity;
        const uint64_t m = ballot64(res);
        const uint32_t r = written + mbcnt(m);
        if (res && r < a.k) {
            oi[r] = id;
            od[r] = q.gd[i];
        }
        written += (uint32_t)__popcll(m);
    }
    written = written < a.k ? written : a.k;
    for (uint32_t r = written + lane; r < a.k; r += kWave) {
        oi[r] = kEmpty;
        od[r] = __builtin_inff();
    }
    if (lane == 0 && a.stats) {
        dann_search_stats st;
        st.cmps = cmps;
        st.hops = hops;
        // Translate::post_process counts a push only while the buffer still has room afterwards (provider.rs:933-944)
        st.result_count = (a.k && written == a.k) ? a.k - 1u : written;
        st.written = written;
        st.status = status;
        a.stats[qi] = st;
    }
}

template <int DT, int OP, bool NORM>
int32_t launch_dv(const DiverseArgs& a, size_t lds, hipStream_t st) {
    return launch_kernel<diverse_search_kernel<DT, OP, NORM>, kLds160Once>("diverse_search_kernel launch", dim3(a.nq), dim3(kWave),
                                                                            lds, st, a);
}

int32_t launch_dv_rows(const DiverseArgs& a, size_t lds, hipStream_t st) {
    const int32_t rc = dispatch_row_op<kRowsQuery>(a.ix.dtype, a.ix.metric, [&](auto r) {
        using R = decltype(r);
        return launch_dv<R::dt, R::op, R::norm>(a, lds, st);
    });
    if (rc != kNoRow) return rc;
    set_error("diverse search: rows of dtype %d are not supported", a.ix.dtype);
    return DANN_EUNSUPPORTED;
}

uint32_t dv_prime_leq(uint32_t n) {
    for (uint32_t p = n; p > 2; --p) {
        bool prime = (p & 1u) != 0;
        for (uint32_t f = 3; prime && f * f <= p; f += 2) prime = p % f != 0;
        if (prime) return p;
    }
    return 2;
}

}  // namespace

// One batch of device-resident queries: d_queries (nq rows), d_ids / d_dists (nq x k), d_stats (nq).  Runs every query
// with LDS scratch, then re-runs the ones whose pool or visited table filled up with global-memory scratch that cannot
// fill up.  Host-synchronous.
int32_t diverse_search_device(dann_index* idx, hipStream_t st, const void* d_queries, uint32_t nq, uint32_t l_value,
                              uint32_t beam_width, uint32_t k, uint32_t diverse_k, uint32_t total_k, uint32_t* d_ids,
                              float* d_dists, dann_search_stats* d_stats) {
    if (nq == 0) return DANN_OK;
    DiverseArgs a{};
    a.ix = idx->qview();
    a.queries = d_queries;
    a.qmap = nullptr;
    a.attr = idx->d_attr;
    a.nq = nq;
    a.l_value = l_value;
    a.beam_width = beam_width;
    a.k = k;
    a.dk = diverse_k;
    a.dl = (uint32_t)((uint64_t)diverse_k * l_value / total_k);  // diverse_priority_queue.rs:90-104
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.stats = d_stats;
    // LDS scratch: the pool holds twice the queue plus a wavefront (the local queues outgrow the global one only by
    // failed removes and dropped inserts); the visited table about twice what L * R comparisons need, within 160 KiB
    const uint32_t fixed = dv_fixed_lds(a.ix, beam_width);
    uint32_t pool = 2u * l_value + 64u;
    const uint32_t dbg_pool = idx->dbg_u32(DANN_DBG_DIVERSE_POOL, 0u);
    if (dbg_pool) pool = dbg_pool;
    uint32_t ht = 1024;
    while (ht < 16384 && (uint64_t)ht < (uint64_t)l_value * a.ix.max_degree * 2u) ht *= 2;
    const uint64_t floor_ids = (uint64_t)a.ix.nstart + (uint64_t)kWave * 2u;
    while (ht < 32768 && (uint64_t)ht * 3u / 4u <= floor_ids) ht *= 2;
    while (ht > 1024 && fixed + dv_ws_bytes(l_value, pool, ht) > 160u * 1024u) ht /= 2;
    size_t lds = fixed + dv_ws_bytes(l_value, pool, ht);
    if (lds > 160u * 1024u || (uint64_t)dv_prime_leq(ht) * 3u / 4u <= floor_ids) {
        set_error("diverse search: L = %u needs %zu B of LDS per query (160 KiB at most)", l_value, lds);
        return DANN_EUNSUPPORTED;
    }
    a.pool_cap = pool;
    a.ht_entries = ht;
    a.ht_prime = dv_prime_leq(ht);
    a.gws = nullptr;
    a.gws_stride = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DANN_HIP(hipEventCreate(&e0));
    DANN_HIP(hipEventCreate(&e1));
    struct Ev {
        hipEvent_t a, b;
        ~Ev() {
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
        }
    } ev{e0, e1};
    DANN_HIP(hipEventRecord(e0, st));
    if (int32_t rc = launch_dv_rows(a, lds, st)) return rc;
    DANN_HIP(hipEventRecord(e1, st));
    std::vector<dann_search_stats> stats(nq);
    DANN_HIP(hipMemcpyAsync(stats.data(), d_stats, (size_t)nq * sizeof(dann_search_stats), hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    std::vector<uint32_t> failed;
    for (uint32_t i = 0; i < nq; ++i) {
        if (stats[i].status == (uint32_t)(-DANN_EOVERFLOW)) failed.push_back(i);
        else if (stats[i].status) {
            set_error("diverse search: query %u could not read a start point", i);
            return (int32_t)(-(int32_t)stats[i].status);
        }
    }
    float rms = 0.f;
    const size_t nfailed = failed.size();
    // re-runs in global memory, two levels: a table of 2^16 entries and a pool of 4096 + 4 L first (enough for any
    // search measured so far), then -- for what still fills up -- scratch that cannot: the pool takes every id the
    // search can insert, the table every slot
    for (int level = 0; level < 2 && !failed.empty(); ++level) {
        DiverseArgs b = a;
        const uint32_t ns = a.ix.nslots;
        uint32_t h = 1024;
        if (level == 0) {
            b.pool_cap = std::min<uint32_t>(ns, 4096u + 4u * l_value);
            h = 65536;
        } else {
            b.pool_cap = ns;
            while ((uint64_t)h * 3u / 4u < (uint64_t)ns + 2u * kWave && h < (1u << 30)) h *= 2;
            while ((uint64_t)dv_prime_leq(h) * 3u / 4u < (uint64_t)ns + 2u * kWave) h *= 2;
        }
        b.ht_entries = h;
        b.ht_prime = dv_prime_leq(h);
        b.gws_stride = (dv_ws_bytes(l_value, b.pool_cap, h) + 255u) & ~(uint64_t)255u;
        const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(failed.size(), (1ull << 30) / b.gws_stride));
        DevBuf gws, map;
        DANN_HIP(gws.alloc((size_t)chunk * b.gws_stride));
        DANN_HIP(map.alloc(failed.size() * 4));
        uint32_t* d_map = map.as<uint32_t>();
        DANN_HIP(hipMemcpyAsync(d_map, failed.data(), failed.size() * 4, hipMemcpyHostToDevice, st));
        b.gws = gws.as<uint8_t>();
        const size_t blds = dv_fixed_lds(a.ix, beam_width);
        for (size_t o = 0; o < failed.size(); o += chunk) {
            b.qmap = d_map + o;
            b.nq = (uint32_t)std::min<size_t>(chunk, failed.size() - o);
            DANN_HIP(hipEventRecord(e0, st));
            if (int32_t rc = launch_dv_rows(b, blds, st)) return rc;
            DANN_HIP(hipEventRecord(e1, st));
            DANN_HIP(hipStreamSynchronize(st));
            float m2 = 0.f;
            (void)hipEventElapsedTime(&m2, e0, e1);
            rms += m2;
        }
        DANN_HIP(hipMemcpyAsync(stats.data(), d_stats, (size_t)nq * sizeof(dann_search_stats), hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
        std::vector<uint32_t> still;
        for (uint32_t i : failed)
            if (stats[i].status) {
                if (level == 1 || stats[i].status != (uint32_t)(-DANN_EOVERFLOW)) {
                    set_error("diverse search: query %u failed in its re-run (status %u)", i, stats[i].status);
                    return DANN_EINTERNAL;
                }
                still.push_back(i);
            }
        failed.swap(still);
    }
    {
        std::lock_guard<std::mutex> lk(idx->stat_mu);
        idx->clocks[0].total_ms += ms + rms;
        idx->clocks[0].launches += 1;
        idx->families[DANN_FAMILY_DIVERSE].total_ms += ms + rms;
        idx->families[DANN_FAMILY_DIVERSE].launches += 1;
        if (nfailed) {
            idx->clocks[4].total_ms += rms;
            idx->clocks[4].launches += nfailed;
        }
    }
    return DANN_OK;
}

}  // namespace dann
