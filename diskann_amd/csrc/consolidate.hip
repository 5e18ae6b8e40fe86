// consolidate.hip -- deleted state and graph consolidation on the GPU.
//
// Replaces, for a whole index or a list of vertices, the reference calls
//   DataProvider::delete                       diskann/src/provider.rs:165
//   DiskANNIndex::consolidate_vector           diskann/src/graph/index.rs:1819-1930
//     on_neighbors                             index.rs:1072-1109
//     robust_prune_list (force_saturate off)   index.rs:2397-2454
//   drop_adj_list                              index.rs:1060
//
// Every live vertex is repaired on its own: it reads its own list and the lists of its deleted neighbours, and
// consolidation never rewrites a deleted vertex's list, so one batched pass equals the reference's sequential loop in
// any order.  Three steps, a fixed number of host synchronisations per call (two):
//   cons_scan_kernel     16 lanes per vertex: read the row, test the neighbours against the deleted bitmap (1 bit per
//                        slot: 128 KiB per million slots, L2 resident), bound the pool (live neighbours + the lengths of
//                        the deleted neighbours' lists) and queue the vertices that may change into a short or a long
//                        worklist (wave-aggregated atomics);
//   cons_gather_kernel   one wavefront per queued vertex: the unique pool in first-occurrence order (ballot + mbcnt
//                        compaction, duplicates caught by an open-addressing hash set), the decision of consolidate_vector,
//                        short lists written directly, pools to prune left in global memory with their distances d(vertex, c).
//                        Pool and hash set live in LDS up to 4096 candidates, in global memory beyond (pools of up to
//                        max_degree^2 candidates: no size is refused);
//   cons_select_kernel   pools of more than 4096 candidates only: SortedNeighbors::new keeps the max_occlusion_size nearest
//                        (<= 4096), so an exact selection of those by (distance, pool position), handed on in pool order,
//                        leaves the prune the same sorted list;
//   prune_pools_into_rows (build_batch.hip)  the back-edge prune pipeline: row kernel, or sort + Gram tiles + sweep.
// dann_prune_range (graph_stats.hip; DiskANNIndex::prune_range, index.rs:2656-2701) is the same pass (run_list_prunes)
// with no deleted state: lists longer than pruned_degree are queued and always go through robust_prune_list.
// The worklists are processed in chunks, so the pool buffers and the Gram scratch stay bounded for any index size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "dann_device.h"
#include "dann_internal.h"
#include "prune_common.h"

namespace dann {
namespace {

constexpr uint32_t kShortPool = 512;    // pool bounds up to this go to the short worklist
constexpr uint32_t kChunkElems = 4096u * 512u;  // pool entries per chunk (ids + distances: 16 MiB)
constexpr uint32_t kStatLines = 256;    // striped device counters: a workgroup adds to line blockIdx % kStatLines
// counters per line: [0] lists rewritten without prune, [1] pools pruned, [2] largest pool, [3] distances d(vertex, c)
// of the pruned pools, [4] pools of more than kMaxPool candidates, [5] those of [4] whose selected head holds equal
// distances under DANN_TIE_RUST
constexpr uint32_t kStatWords = 6;

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int o = 1; o < 64; o <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

__global__ void mark_deleted_kernel(uint32_t* bm, const uint32_t* slots, uint32_t n, uint8_t* rows, uint64_t row_stride,
                                    uint32_t tag_off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slots[i];
    atomicOr(&bm[s >> 5], 1u << (s & 31u));
    if (tag_off) rows[(uint64_t)s * row_stride + tag_off] = kTagRetiring;
}

__global__ void drop_deleted_kernel(IndexView ix, const uint32_t* bm) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ix.nslots && in_bitmap(bm, i, ix.nslots)) ix.adj[(uint64_t)i * ix.adj_stride] = 0;
}

struct ConsScanArgs {
    IndexView ix;
    const uint32_t* bm;     // deleted bitmap, null = nothing deleted
    const uint32_t* ids;    // null = item i is slot first + i
    uint32_t first;
    uint32_t n;
    uint32_t count_scanned; // dann_prune_range: counts[7] is wanted
    uint32_t check_tags;    // dann_prune_range on an inline-tags index: a vertex whose own slot is unreadable is left alone
    uint32_t* claim;        // explicit ids: bitmap of the vertices already claimed (the first occurrence works), else null
    uint32_t pruned_degree;
    uint8_t* kinds;         // n: ConsolidateKind
    uint32_t* work[3];      // short (bound <= kShortPool), long (<= kMaxPool), huge worklists (gathered in global memory)
    uint32_t* counts;       // [0..2] entries of each worklist, [3..5] the largest bound in each, [7] vertices scanned (a
                            // repeated id once), [8] vertices left alone because their slot is unreadable
};

// Four vertices per wavefront, 16 lanes each.  A vertex is queued when it may change: it has a deleted neighbour, or its
// list is longer than pruned_degree (the gather decides the rest from the exact pool).
__global__ __launch_bounds__(64) void cons_scan_kernel(ConsScanArgs a) {
    const uint32_t lane = threadIdx.x, sub = lane >> 4, sl = lane & 15u;
    const uint32_t item = blockIdx.x * 4u + sub;
    const bool have = item < a.n;
    const uint32_t v = have ? (a.ids ? a.ids[item] : a.first + item) : 0u;
    const bool del = have && in_bitmap(a.bm, v, a.ix.nslots);
    int first = 1;
    if (have && !del && a.claim && sl == 0) {
        const uint32_t bit = 1u << (v & 31u);
        first = (atomicOr(&a.claim[v >> 5], bit) & bit) == 0u;
    }
    first = __shfl(first, (int)(lane & 48u));
    if (have && sl == 0) a.kinds[item] = del ? (uint8_t)DANN_CONSOLIDATE_DELETED : (uint8_t)DANN_CONSOLIDATE_COMPLETE;
    const bool scan = have && !del && first;
    if (a.count_scanned) {
        const uint64_t sm = ballot64(have && first && sl == 0);
        if (lane == 0 && sm) atomicAdd(&a.counts[7], (uint32_t)__popcll(sm));
    }
    const uint32_t* arow = a.ix.adj + (uint64_t)v * a.ix.adj_stride;
    const uint32_t len = scan ? min(arow[0], a.ix.max_degree) : 0u;
    uint32_t ndel = 0, bound = 0;
    for (uint32_t e = sl; e < len; e += 16u) {
        const uint32_t id = arow[1 + e];
        if (in_bitmap(a.bm, id, a.ix.nslots)) {
            ++ndel;
            bound += min(a.ix.adj[(uint64_t)id * a.ix.adj_stride], a.ix.max_degree);
        } else {
            ++bound;
        }
    }
    for (int o = 1; o < 16; o <<= 1) {
        ndel += (uint32_t)__shfl_xor((int)ndel, o);
        bound += (uint32_t)__shfl_xor((int)bound, o);
    }
    bool want = scan && (ndel != 0u || len > a.pruned_degree);
    if (a.check_tags) {  // (the reference reads the list first: a short list is passed over before any row is fetched)
        const bool unreadable = want && a.ix.rows[(uint64_t)v * a.ix.row_stride + a.ix.tag_off] < kTagReadable;
        const uint64_t um = ballot64(unreadable && sl == 0);
        if (lane == 0 && um) atomicAdd(&a.counts[8], (uint32_t)__popcll(um));
        want = want && !unreadable;
    }
    const uint32_t cls = bound <= kShortPool ? 0u : bound <= kMaxPool ? 1u : 2u;
    for (uint32_t c = 0; c < 3; ++c) {
        wave_push(want && cls == c && sl == 0, a.work[c], &a.counts[c], item);
        const uint32_t mb = wave_max(want && cls == c ? bound : 0u);
        if (lane == 0 && mb) atomicMax(&a.counts[3 + c], mb);
    }
}

struct ConsGatherArgs {
    IndexView ix;
    const uint32_t* bm;
    const uint32_t* ids;
    uint32_t first;
    const uint32_t* work;   // worklist of items; this launch: work[lo .. lo + m)
    uint32_t lo;
    uint32_t prune_always;  // dann_prune_range: every queued list goes through robust_prune_list, whatever its pool's size,
                            // and (inline tags) neighbours whose slot is unreadable stay out of the pool
    uint32_t pruned_degree;
    uint32_t pcap;          // pool capacity and stride of the chunk buffers (>= every pool bound of the worklist)
    uint32_t in_global;     // 1: pool and hash set in global memory (pool_ids / hash), else in LDS
    uint32_t* hash;         // in_global: 2 x pcap entries per item
    uint32_t* locs;         // chunk buffers: the vertex, its pool and distances, the pool length (0 = nothing to prune)
    uint32_t* pool_ids;
    float* pool_d;
    uint32_t* counts;
    unsigned long long* stats;  // kStatLines x kStatWords
    uint32_t* err;          // bit 0: a pool outgrew its bound (a bug, never an input); bit 1 (prune_always): a list holds
                            // a neighbour id past the last slot
};

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void cons_gather_kernel(ConsGatherArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x, wi = blockIdx.x;
    // LDS: [dl: max_degree][pool: pcap][hash: 2 pcap] (the last two only without in_global)
    uint32_t* dl = reinterpret_cast<uint32_t*>(smem);  // the deleted neighbours, in list order
    uint32_t* gid = a.pool_ids + (uint64_t)wi * a.pcap;
    uint32_t* pool = a.in_global ? gid : dl + a.ix.max_degree;
    uint32_t* hash = a.in_global ? a.hash + (uint64_t)wi * 2u * a.pcap : dl + a.ix.max_degree + a.pcap;
    const uint32_t hmask = 2u * a.pcap - 1u;
    for (uint32_t i = lane; i <= hmask; i += kWave) hash[i] = kEmpty;
    __syncthreads();
    const uint32_t item = a.work[a.lo + wi];
    const uint32_t v = a.ids ? a.ids[item] : a.first + item;
    const uint32_t nslots = a.ix.nslots, R = a.ix.max_degree;
    const bool skip_unreadable = a.prune_always && a.ix.tag_off;
    uint32_t* arow = a.ix.adj + (uint64_t)v * a.ix.adj_stride;
    const uint32_t len = min(arow[0], R);
    // on_neighbors(vertex): the live neighbours into the pool, the deleted ones into dl
    uint32_t cnt = 0, ndel = 0;
    bool self_in_list = false, bad_id = false;
    for (uint32_t e0 = 0; e0 < len; e0 += kWave) {
        const uint32_t e = e0 + lane;
        const uint32_t id = e < len ? arow[1 + e] : kEmpty;
        const bool del = e < len && in_bitmap(a.bm, id, nslots);
        const uint64_t dm = ballot64(del);
        if (del) dl[ndel + mbcnt(dm)] = id;
        ndel += (uint32_t)__popcll(dm);
        self_in_list |= ballot64(e < len && id == v) != 0ull;
        bool take = e < len && !del && id != v;
        if (a.prune_always) {  // (dann_set_neighbors admits an id past the last slot: its row must not be read)
            const bool bad = take && id >= nslots;
            bad_id |= ballot64(bad) != 0ull;
            take = take && !bad;
        }
        if (skip_unreadable && take) take = a.ix.rows[(uint64_t)id * a.ix.row_stride + a.ix.tag_off] >= kTagReadable;
        cnt = append_unique(pool, hash, hmask, cnt, a.pcap, take ? id : kEmpty, a.err);
    }
    __syncthreads();  // dl is read by every lane below
    if (bad_id) {  // the list is left as it is, and the call answers DANN_EBOUNDS
        if (lane == 0) {
            atomicOr(a.err, 2u);
            a.counts[wi] = 0;
        }
        return;
    }
    unsigned long long* st = a.stats + (size_t)(blockIdx.x & (kStatLines - 1u)) * kStatWords;
    // nothing deleted and no prune required (index.rs:1858-1864: the pool still holds the vertex itself if it is listed)
    if (!a.prune_always && ndel == 0 && cnt + (self_in_list ? 1u : 0u) <= a.pruned_degree) {
        if (lane == 0) a.counts[wi] = 0;
        return;
    }
    // on_neighbors(deleted neighbour): its live neighbours, in the order of the vertex's list (not transitive)
    for (uint32_t k = 0; k < ndel; ++k) {
        const uint32_t d = dl[k];
        const uint32_t* drow = a.ix.adj + (uint64_t)d * a.ix.adj_stride;
        const uint32_t dlen = min(drow[0], R);
        for (uint32_t e0 = 0; e0 < dlen; e0 += kWave) {
            const uint32_t e = e0 + lane;
            const uint32_t id = e < dlen ? drow[1 + e] : kEmpty;
            const bool live = e < dlen && id != v && !in_bitmap(a.bm, id, nslots);
            cnt = append_unique(pool, hash, hmask, cnt, a.pcap, live ? id : kEmpty, a.err);
        }
    }
    __syncthreads();  // the pool's ids, written by every lane, are read by all of them below
    if (lane == 0) atomicMax(&st[2], (unsigned long long)(a.prune_always ? len : cnt));
    if (a.prune_always ? cnt == 0u : cnt < a.pruned_degree) {  // the pool is the new list (set_neighbors)
        for (uint32_t i = lane; i < cnt; i += kWave) arow[1 + i] = pool[i];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            arow[0] = cnt;
            a.counts[wi] = 0;
            atomicAdd(&st[0], 1ull);
        }
        return;
    }
    // robust_prune_list: the pool and d(vertex, c) in pool order for the prune kernels
    float* gd = a.pool_d + (uint64_t)wi * a.pcap;
    if (!a.in_global)
        for (uint32_t i = lane; i < cnt; i += kWave) gid[i] = pool[i];
    fill_list_distances<DT, OP, NORM>(a.ix, v, pool, gd, cnt);
    if (lane == 0) {
        a.locs[wi] = v;
        a.counts[wi] = cnt;
        atomicAdd(&st[1], 1ull);
        atomicAdd(&st[3], (unsigned long long)cnt);
    }
}

constexpr auto kConsGather = [](auto r) { using R = decltype(r); return KernelOf<cons_gather_kernel<R::dt, R::op, R::norm>>{}; };

struct ConsSelectArgs {
    const uint32_t* in_ids;  // gathered pools: stride in_stride, lengths in_cnt (0 = nothing to prune)
    const float* in_d;
    const uint32_t* in_cnt;
    uint32_t in_stride;
    uint64_t* keys;          // scratch, in_stride per item
    uint32_t keep;           // max_occlusion_size
    uint32_t tie_rust;
    uint32_t* out_ids;       // stride kMaxPool
    float* out_d;
    uint32_t* out_cnt;
    unsigned long long* stats;
};

// Pools of more than kMaxPool candidates: SortedNeighbors::new sorts the pool and keeps the `keep` nearest.  The `keep`
// smallest (distance, position) keys are selected exactly and handed on in pool order, so the prune kernels' own sort
// of them yields the same list under DANN_TIE_POSITION, and under DANN_TIE_RUST wherever the selected head has no equal
// distances (the pools where it has are counted: there Rust's order of the full pool is not reproduced).
__global__ __launch_bounds__(256) void cons_select_kernel(ConsSelectArgs a) {
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    const uint32_t cnt = a.in_cnt[b];
    const uint32_t* ids = a.in_ids + (uint64_t)b * a.in_stride;
    const float* d = a.in_d + (uint64_t)b * a.in_stride;
    uint32_t* oid = a.out_ids + (uint64_t)b * kMaxPool;
    float* od = a.out_d + (uint64_t)b * kMaxPool;
    if (cnt <= kMaxPool) {
        for (uint32_t i = t; i < cnt; i += blockDim.x) {
            oid[i] = ids[i];
            od[i] = d[i];
        }
        if (t == 0) a.out_cnt[b] = cnt;
        return;
    }
    uint64_t* keys = a.keys + (uint64_t)b * a.in_stride;
    uint32_t P = 64;
    while (P < cnt) P <<= 1;
    for (uint32_t i = t; i < P; i += blockDim.x) keys[i] = i < cnt ? dist_key(d[i], i) : ~0ull;
    __syncthreads();
    block_bitonic(keys, P);
    const uint32_t keep = min(a.keep, cnt);
    __shared__ int tied;
    if (t == 0) tied = 0;
    __syncthreads();
    if (a.tie_rust)
        for (uint32_t i = t; i < keep && i + 1u < cnt; i += blockDim.x)
            if ((keys[i] >> 32) == (keys[i + 1] >> 32)) tied = 1;
    __syncthreads();
    for (uint32_t i = t; i < P; i += blockDim.x) keys[i] = i < keep ? (keys[i] & 0xFFFFFFFFull) : ~0ull;  // positions
    __syncthreads();
    block_bitonic(keys, P);
    for (uint32_t i = t; i < keep; i += blockDim.x) {
        const uint32_t pos = (uint32_t)keys[i];
        oid[i] = ids[pos];
        od[i] = d[pos];
    }
    if (t == 0) {
        a.out_cnt[b] = keep;
        unsigned long long* st = a.stats + (size_t)(b & (kStatLines - 1u)) * kStatWords;
        atomicAdd(&st[4], 1ull);
        if (tied) atomicAdd(&st[5], 1ull);
    }
}

}  // namespace

int32_t ensure_deleted_bitmap(dann_index* idx) {
    if (idx->d_deleted) return DANN_OK;
    const size_t bytes = (size_t)((idx->nslots + 31u) / 32u) * 4u;
    uint32_t* p = nullptr;
    DANN_HIP(hipMalloc((void**)&p, bytes));
    hipError_t e = hipMemsetAsync(p, 0, bytes, idx->main.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(idx->main.stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return hip_fail(e, "deleted bitmap");
    }
    idx->d_deleted = p;
    return DANN_OK;
}

}  // namespace dann

using namespace dann;

namespace dann {
int32_t run_list_prunes(dann_index* idx, const dann_build_config* cfg, ListPrunePass& pass) {
    const uint32_t* ids = pass.ids;
    const uint32_t n = pass.n;
    int32_t* out_kind = pass.out_kind;
    const uint32_t* bm = pass.prune_range ? nullptr : idx->d_deleted;
    hipStream_t st = idx->main.stream;
    const IndexView ix = idx->view();
    uint64_t bc0[11] = {};
    if (pass.want_counters) {
        if (int32_t rc = dann_build_counters(idx, bc0, 11)) return rc;
    }
    // per-call scratch: ids + claim bitmap, kinds, the two worklists, counts, striped stats, error word
    const size_t claim_words = ids ? (idx->nslots + 31u) / 32u : 0u;
    DevBuf d_ids, d_claim, d_kinds, d_work, d_meta, d_stats;
    if (ids) {
        DANN_HIP(d_ids.alloc((size_t)n * 4));
        DANN_HIP(hipMemcpyAsync(d_ids.p, ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
        DANN_HIP(d_claim.alloc(claim_words * 4));
        DANN_HIP(hipMemsetAsync(d_claim.p, 0, claim_words * 4, st));
    }
    DANN_HIP(d_kinds.alloc(n));
    DANN_HIP(d_work.alloc((size_t)n * 12));
    DANN_HIP(d_meta.alloc(64));
    DANN_HIP(hipMemsetAsync(d_meta.p, 0, 64, st));
    const size_t stats_bytes = (size_t)kStatLines * kStatWords * 8;
    DANN_HIP(d_stats.alloc(stats_bytes));
    DANN_HIP(hipMemsetAsync(d_stats.p, 0, stats_bytes, st));
    uint32_t* meta = d_meta.as<uint32_t>();  // [0..5] scan counts, [6] error word, [7] scanned, [8] unreadable
    uint32_t* work = d_work.as<uint32_t>();

    ConsScanArgs sa;
    sa.ix = ix;
    sa.bm = bm;
    sa.ids = ids ? d_ids.as<uint32_t>() : nullptr;
    sa.first = pass.first;
    sa.n = n;
    sa.count_scanned = pass.prune_range ? 1u : 0u;
    sa.check_tags = pass.prune_range && ix.tag_off ? 1u : 0u;
    sa.claim = ids ? d_claim.as<uint32_t>() : nullptr;
    sa.pruned_degree = cfg->pruned_degree;
    sa.kinds = d_kinds.as<uint8_t>();
    for (int c = 0; c < 3; ++c) sa.work[c] = work + (size_t)c * n;
    sa.counts = meta;
    hipLaunchKernelGGL(cons_scan_kernel, dim3((n + 3u) / 4u), dim3(64), 0, st, sa);
    DANN_HIP(hipGetLastError());
    uint32_t h_counts[9] = {};
    DANN_HIP(hipMemcpyAsync(h_counts, meta, 36, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));

    // the matrix-core path keeps a Gram block per item in the index's build scratch: chunks of it stay at the build's
    // batch scale
    const uint32_t max_chunk = prune_pools_use_gram(idx) ? 2048u : 8192u;
    DevBuf c_locs, c_ids, c_d, c_cnt, c_hash, c_keys, c_sel_ids, c_sel_d, c_sel_cnt;
    size_t c_elems = 0, c_items = 0;
    for (int cls = 0; cls < 3; ++cls) {
        const uint32_t nwork = h_counts[cls];
        if (nwork == 0) continue;
        const bool huge = cls == 2;
        const uint32_t pcap = pow2_at_least(h_counts[3 + cls]);
        const uint32_t chunk =
            std::min<uint32_t>(nwork, std::max<uint32_t>(huge ? 16u : 256u, std::min<uint32_t>(max_chunk, kChunkElems / pcap)));
        if ((size_t)chunk * pcap > c_elems || chunk > c_items) {
            // (earlier classes' buffers serve a later one when large enough; hipFree waits for the work queued on them)
            c_elems = std::max<size_t>(c_elems, (size_t)chunk * pcap);
            DANN_HIP(c_ids.alloc(c_elems * 4));
            DANN_HIP(c_d.alloc(c_elems * 4));
            if (chunk > c_items) {
                c_items = chunk;
                DANN_HIP(c_locs.alloc(c_items * 4));
                DANN_HIP(c_cnt.alloc(c_items * 4));
                DANN_HIP(hipMemsetAsync(c_locs.p, 0, c_items * 4, st));
            }
        }
        if (huge) {  // global pools: hash sets, sort keys and the selected heads (stride kMaxPool)
            DANN_HIP(c_hash.alloc((size_t)chunk * pcap * 8));
            DANN_HIP(c_keys.alloc((size_t)chunk * pcap * 8));
            DANN_HIP(c_sel_ids.alloc((size_t)chunk * kMaxPool * 4));
            DANN_HIP(c_sel_d.alloc((size_t)chunk * kMaxPool * 4));
            DANN_HIP(c_sel_cnt.alloc((size_t)chunk * 4));
        }
        ConsGatherArgs ga;
        ga.ix = ix;
        ga.bm = bm;
        ga.ids = sa.ids;
        ga.first = pass.first;
        ga.prune_always = pass.prune_range ? 1u : 0u;
        ga.work = sa.work[cls];
        ga.pruned_degree = cfg->pruned_degree;
        ga.pcap = pcap;
        ga.in_global = huge ? 1u : 0u;
        ga.hash = huge ? c_hash.as<uint32_t>() : nullptr;
        ga.locs = c_locs.as<uint32_t>();
        ga.pool_ids = c_ids.as<uint32_t>();
        ga.pool_d = c_d.as<float>();
        ga.counts = c_cnt.as<uint32_t>();
        ga.stats = d_stats.as<unsigned long long>();
        ga.err = meta + 6;
        const size_t lds = (size_t)(ix.max_degree + (huge ? 0u : 3u * pcap)) * 4u;
        ConsSelectArgs sel;
        sel.in_ids = ga.pool_ids;
        sel.in_d = ga.pool_d;
        sel.in_cnt = ga.counts;
        sel.in_stride = pcap;
        sel.keys = c_keys.as<uint64_t>();
        sel.keep = cfg->max_occlusion_size ? cfg->max_occlusion_size : 750u;
        sel.tie_rust = idx->prune_tie_order == DANN_TIE_RUST ? 1u : 0u;
        sel.out_ids = c_sel_ids.as<uint32_t>();
        sel.out_d = c_sel_d.as<float>();
        sel.out_cnt = c_sel_cnt.as<uint32_t>();
        sel.stats = ga.stats;
        for (uint32_t lo = 0; lo < nwork; lo += chunk) {
            const uint32_t m = std::min<uint32_t>(chunk, nwork - lo);
            ga.lo = lo;
            int32_t rc = launch_rows(ix, kConsGather, "cons_gather_kernel launch", ga, m, lds, st);
            if (rc != DANN_OK) return rc;
            bool used_gram = false;
            if (huge) {
                hipLaunchKernelGGL(cons_select_kernel, dim3(m), dim3(256), 0, st, sel);
                DANN_HIP(hipGetLastError());
                rc = prune_pools_into_rows(idx, *cfg, ga.locs, sel.out_ids, sel.out_d, sel.out_cnt, kMaxPool, m,
                                           &used_gram);
            } else {
                rc = prune_pools_into_rows(idx, *cfg, ga.locs, ga.pool_ids, ga.pool_d, ga.counts, pcap, m, &used_gram);
            }
            if (rc != DANN_OK) return rc;
        }
    }
    if (pass.drop_deleted && idx->d_deleted) {
        hipLaunchKernelGGL(drop_deleted_kernel, dim3((idx->nslots + 255u) / 256u), dim3(256), 0, st, ix, idx->d_deleted);
        DANN_HIP(hipGetLastError());
    }
    std::vector<uint8_t> h_kinds(out_kind ? n : 0);
    std::vector<unsigned long long> h_stats((size_t)kStatLines * kStatWords);
    uint32_t h_err = 0;
    if (out_kind) DANN_HIP(hipMemcpyAsync(h_kinds.data(), d_kinds.p, n, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipMemcpyAsync(h_stats.data(), d_stats.p, stats_bytes, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipMemcpyAsync(&h_err, meta + 6, 4, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    if (h_err & 2u) {
        set_error("%s: an adjacency list holds a neighbour id out of bounds (%u slots); that list is left as it is", pass.who,
                  idx->nslots);
        return DANN_EBOUNDS;
    }
    if (h_err) {
        set_error("%s: a candidate pool outgrew its bound", pass.who);
        return DANN_EINTERNAL;
    }
    if (out_kind)
        for (uint32_t i = 0; i < n; ++i) out_kind[i] = h_kinds[i];
    uint64_t sums[kStatWords] = {0, 0, 0, 0, 0, 0};
    for (uint32_t l = 0; l < kStatLines; ++l)
        for (uint32_t w = 0; w < kStatWords; ++w) {
            const unsigned long long x = h_stats[(size_t)l * kStatWords + w];
            sums[w] = w == 2 ? std::max<uint64_t>(sums[w], x) : sums[w] + x;
        }
    uint64_t bc1[11] = {};
    if (pass.want_counters) {
        if (int32_t rc = dann_build_counters(idx, bc1, 11)) return rc;
    }
    pass.rewritten = sums[0];
    pass.pruned = sums[1];
    pass.largest = sums[2];
    pass.distances = sums[3] + (bc1[4] - bc0[4]) + (bc1[8] - bc0[8]);
    pass.on_matrix_cores = bc1[0] - bc0[0];  // the sweep of the matrix-core path counts every prune it runs
    pass.oversized = sums[4];
    pass.oversized_tied = sums[5];
    pass.scanned = h_counts[7];
    pass.unreadable = h_counts[8];
    return DANN_OK;
}
}  // namespace dann

extern "C" {

int32_t dann_delete_points(dann_index* idx, const uint32_t* slots, uint32_t n) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    if (n == 0) return DANN_OK;
    if (!slots) return DANN_EINVAL;
    for (uint32_t i = 0; i < n; ++i) {
        if (slots[i] >= idx->nslots) {
            set_error("dann_delete_points: slot %u out of bounds (%u slots)", slots[i], idx->nslots);
            return DANN_EBOUNDS;
        }
        if (slots[i] >= idx->cfg.capacity) {
            set_error("dann_delete_points: slot %u is a start point (frozen, cannot be deleted)", slots[i]);
            return DANN_EINVAL;
        }
    }
    DeviceGuard guard(idx->device);
    if (int32_t rc = ensure_deleted_bitmap(idx)) return rc;
    DevBuf d_slots;
    DANN_HIP(d_slots.alloc((size_t)n * 4));
    hipStream_t st = idx->main.stream;
    DANN_HIP(hipMemcpyAsync(d_slots.p, slots, (size_t)n * 4, hipMemcpyHostToDevice, st));
    const uint32_t tag_off = idx->cfg.inline_tags ? idx->layer_bytes : 0u;
    hipLaunchKernelGGL(mark_deleted_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, idx->d_deleted, d_slots.as<uint32_t>(),
                       n, idx->d_rows, (uint64_t)idx->cfg.row_stride, tag_off);
    DANN_HIP(hipGetLastError());
    DANN_HIP(hipStreamSynchronize(st));
    if (tag_off)
        for (uint32_t i = 0; i < n; ++i) idx->h_tags[slots[i]] = kTagRetiring;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_get_deleted(const dann_index* idx, uint32_t first_slot, uint32_t n, uint8_t* out) try {
    if (!idx || (n && !out)) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    if ((uint64_t)first_slot + n > idx->nslots) return DANN_EBOUNDS;
    if (n == 0) return DANN_OK;
    if (!idx->d_deleted) {
        memset(out, 0, n);
        return DANN_OK;
    }
    DeviceGuard guard(idx->device);
    const uint32_t w0 = first_slot / 32u, w1 = (first_slot + n - 1u) / 32u;
    std::vector<uint32_t> words(w1 - w0 + 1u);
    DANN_HIP(hipMemcpyAsync(words.data(), idx->d_deleted + w0, words.size() * 4, hipMemcpyDeviceToHost, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = first_slot + i;
        out[i] = (uint8_t)((words[s / 32u - w0] >> (s & 31u)) & 1u);
    }
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_consolidate(dann_index* idx, const dann_build_config* cfg, const uint32_t* ids, uint32_t n, uint32_t flags,
                         int32_t* out_kind, uint64_t* out_counters) try {
    if (!idx || !cfg) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    if (int32_t rc = check_build_cfg(idx, cfg, "dann_consolidate", false)) return rc;
    if (flags & ~(uint32_t)DANN_CONSOLIDATE_DROP_DELETED) {
        set_error("dann_consolidate: unknown flags %u", flags);
        return DANN_EINVAL;
    }
    if (ids) {
        if (n == 0) return DANN_OK;
        for (uint32_t i = 0; i < n; ++i)
            if (ids[i] >= idx->nslots) {
                set_error("dann_consolidate: id %u out of bounds (%u slots)", ids[i], idx->nslots);
                return DANN_EBOUNDS;
            }
    } else {
        n = idx->nslots;
    }
    DeviceGuard guard(idx->device);
    ListPrunePass pass;
    pass.who = "dann_consolidate";
    pass.ids = ids;
    pass.n = n;
    pass.drop_deleted = (flags & DANN_CONSOLIDATE_DROP_DELETED) != 0;
    pass.out_kind = out_kind;
    pass.want_counters = out_counters != nullptr;
    if (int32_t rc = run_list_prunes(idx, cfg, pass)) return rc;
    if (out_counters) {
        out_counters[0] = n;
        out_counters[1] = pass.rewritten;
        out_counters[2] = pass.pruned;
        out_counters[3] = pass.largest;
        out_counters[4] = pass.distances;
        out_counters[5] = pass.on_matrix_cores;
        out_counters[6] = pass.oversized;
        out_counters[7] = pass.oversized_tied;
    }
    return DANN_OK;
} DANN_CATCH_ALL

}  // extern "C"
