// graph_stats.hip -- what the reference's in-memory builder runs after its inserts (diskann/src/graph/index.rs):
//   count_reachable_nodes  :2161-2189  dann_count_reachable  a level-synchronous breadth-first walk over the adjacency rows
//   get_degree_stats       :2191-2239  dann_degree_stats     one reduction over the lists' lengths
//   prune_range            :2656-2701  dann_prune_range      consolidate.hip's scan / gather / prune pass without deleted state
//
// The walk: one launch per level.  A wavefront takes frontier nodes; its lanes read the node's adjacency row in one
// request and each claims its neighbour with atomicOr on the visited bitmap -- the returned old word says who set the
// bit, so a node enters the next frontier exactly once under any race -- and the winners are appended with one
// wave-aggregated atomicAdd.  Every claimed node is expanded at the next level, so the sum of the frontiers' sizes is
// the reference's expanded_nodes.len().  Pure graph: no tags, no deleted bitmap, no vectors.
#include <vector>

#include "api_common.h"
#include "wave_lists.h"

namespace dann {
namespace {

struct BfsArgs {
    const uint32_t* adj;
    uint32_t adj_stride, max_degree, nslots;
    const uint32_t* in;     // this level's frontier (the seed launch: the start ids, duplicates allowed)
    uint32_t n_in;
    uint32_t* out;          // the next frontier, nslots entries
    uint32_t* out_count;
    uint32_t* visited;      // (nslots + 31) / 32 words
    uint32_t* err;          // set by a neighbour id >= nslots
};

__device__ __forceinline__ bool bfs_claim(uint32_t* visited, uint32_t id) {
    const uint32_t bit = 1u << (id & 31u);
    return (atomicOr(&visited[id >> 5], bit) & bit) == 0u;
}

__global__ __launch_bounds__(256) void bfs_seed_kernel(BfsArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = i < a.n_in;
    const uint32_t id = have ? a.in[i] : 0u;  // (checked against nslots by the host)
    wave_push(have && bfs_claim(a.visited, id), a.out, a.out_count, id);
}

__global__ __launch_bounds__(256) void bfs_level_kernel(BfsArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t i = wave; i < a.n_in; i += nwaves) {
        const uint32_t* row = a.adj + (uint64_t)a.in[i] * a.adj_stride;
        const uint32_t len = min(row[0], a.max_degree);  // Neighbors::get clamps a length word past max_degree
        for (uint32_t e0 = 0; e0 < len; e0 += 64u) {
            const uint32_t e = e0 + lane;
            const uint32_t id = e < len ? row[1 + e] : 0u;
            const bool bad = e < len && id >= a.nslots;
            if (bad) atomicOr(a.err, 1u);
            wave_push(e < len && !bad && bfs_claim(a.visited, id), a.out, a.out_count, id);
        }
    }
}

struct DegreeArgs {
    const uint32_t* adj;
    uint32_t adj_stride, max_degree, nslots;
    const uint32_t* ids;    // null = item i is slot i
    uint32_t n;
    const uint32_t* skip;   // the deleted bitmap when DANN_DEGREE_SKIP_DELETED asks for it, else null
    unsigned long long* sums;  // [0] total, [1] points, [2] lists shorter than two
    uint32_t* minmax;          // [0] min (starts at UINT32_MAX), [1] max
};

__global__ __launch_bounds__(256) void degree_stats_kernel(DegreeArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool have = i < a.n;
    const uint32_t v = have ? (a.ids ? a.ids[i] : i) : 0u;
    have = have && !in_bitmap(a.skip, v, a.nslots);
    const uint32_t len = have ? min(a.adj[(uint64_t)v * a.adj_stride], a.max_degree) : 0u;
    uint32_t total = len, mn = have ? len : 0xFFFFFFFFu, mx = len;
    const uint64_t pm = ballot64(have), lm = ballot64(have && len < 2u);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        total += (uint32_t)__shfl_xor((int)total, o);
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    }
    if ((threadIdx.x & 63u) == 0u && pm) {
        atomicAdd(&a.sums[0], (unsigned long long)total);
        atomicAdd(&a.sums[1], (unsigned long long)__popcll(pm));
        if (lm) atomicAdd(&a.sums[2], (unsigned long long)__popcll(lm));
        atomicMin(&a.minmax[0], mn);
        atomicMax(&a.minmax[1], mx);
    }
}

}  // namespace
}  // namespace dann

using namespace dann;

extern "C" {

int32_t dann_count_reachable(const dann_index* cidx, const uint32_t* start_ids, uint32_t n_start, uint64_t* out_count,
                             uint32_t* out_levels, uint32_t* out_bitmap) try {
    dann_index* idx = const_cast<dann_index*>(cidx);
    CHECK_IDX_SHARED(idx);
    if (!out_count || (n_start && !start_ids)) {
        set_error("dann_count_reachable: out_count is null, or n_start ids without start_ids");
        return DANN_EINVAL;
    }
    const uint32_t nslots = idx->nslots;
    std::vector<uint32_t> starts;
    if (start_ids) {
        starts.assign(start_ids, start_ids + n_start);
    } else {  // the index's start points
        for (uint32_t s = idx->cfg.capacity; s < nslots; ++s) starts.push_back(s);
    }
    for (uint32_t s : starts)
        if (s >= nslots) {
            set_error("dann_count_reachable: start id %u out of bounds (%u slots)", s, nslots);
            return DANN_EBOUNDS;
        }
    const size_t words = ((size_t)nslots + 31u) / 32u;
    if (starts.empty()) {
        *out_count = 0;
        if (out_levels) *out_levels = 0;
        if (out_bitmap) memset(out_bitmap, 0, words * 4);
        return DANN_OK;
    }
    hipStream_t st = ctx.stream;
    DevBuf d_front, d_vis, d_meta, d_starts;  // two frontiers of nslots; d_meta: [0], [1] the frontiers' counts, [2] error
    DANN_HIP(d_front.alloc((size_t)nslots * 8));
    DANN_HIP(d_vis.alloc(words * 4));
    DANN_HIP(d_meta.alloc(16));
    DANN_HIP(d_starts.alloc(starts.size() * 4));
    DANN_HIP(hipMemsetAsync(d_vis.p, 0, words * 4, st));
    DANN_HIP(hipMemsetAsync(d_meta.p, 0, 16, st));
    DANN_HIP(hipMemcpyAsync(d_starts.p, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
    uint32_t* front[2] = {d_front.as<uint32_t>(), d_front.as<uint32_t>() + nslots};
    uint32_t* meta = d_meta.as<uint32_t>();
    BfsArgs a;
    a.adj = idx->d_adj;
    a.adj_stride = idx->cfg.max_degree + 1u;
    a.max_degree = idx->cfg.max_degree;
    a.nslots = nslots;
    a.visited = d_vis.as<uint32_t>();
    a.err = meta + 2;
    a.in = d_starts.as<uint32_t>();
    a.n_in = (uint32_t)starts.size();
    a.out = front[0];
    a.out_count = meta;
    hipLaunchKernelGGL(bfs_seed_kernel, dim3((a.n_in + 255u) / 256u), dim3(256), 0, st, a);
    DANN_HIP(hipGetLastError());
    uint64_t total = 0;
    uint32_t levels = 0, cur = 0;
    for (uint32_t level = 0;; ++level) {
        uint32_t h[3] = {0, 0, 0};
        DANN_HIP(hipMemcpyAsync(h, meta, 12, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
        if (h[2]) {
            set_error("dann_count_reachable: an adjacency list holds a neighbour id out of bounds (%u slots)", nslots);
            return DANN_EBOUNDS;
        }
        const uint32_t n = h[cur];
        if (n == 0) break;
        total += n;
        levels = level;
        a.in = front[cur];
        a.n_in = n;
        a.out = front[cur ^ 1u];
        a.out_count = meta + (cur ^ 1u);
        DANN_HIP(hipMemsetAsync(a.out_count, 0, 4, st));
        const uint32_t blocks = std::min<uint32_t>((n + 3u) / 4u, idx->num_cus * 8u);
        hipLaunchKernelGGL(bfs_level_kernel, dim3(blocks), dim3(256), 0, st, a);
        DANN_HIP(hipGetLastError());
        cur ^= 1u;
    }
    if (out_bitmap) {
        DANN_HIP(hipMemcpyAsync(out_bitmap, d_vis.p, words * 4, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
    }
    *out_count = total;
    if (out_levels) *out_levels = levels;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_degree_stats(const dann_index* cidx, const uint32_t* ids, uint32_t n, uint32_t flags,
                          dann_degree_summary* out) try {
    dann_index* idx = const_cast<dann_index*>(cidx);
    CHECK_IDX_SHARED(idx);
    if (!out) return DANN_EINVAL;
    if (flags & ~(uint32_t)DANN_DEGREE_SKIP_DELETED) {
        set_error("dann_degree_stats: unknown flags %u", flags);
        return DANN_EINVAL;
    }
    memset(out, 0, sizeof(*out));
    if (ids) {
        for (uint32_t i = 0; i < n; ++i)
            if (ids[i] >= idx->nslots) {
                set_error("dann_degree_stats: id %u out of bounds (%u slots)", ids[i], idx->nslots);
                return DANN_EBOUNDS;
            }
    } else {
        n = idx->cfg.capacity;  // non_start_points_ids
    }
    if (n == 0) return DANN_OK;
    hipStream_t st = ctx.stream;
    DevBuf d_ids, d_acc;  // d_acc: [total, points, short lists (u64)][min, max (u32)]
    DANN_HIP(d_acc.alloc(32));
    const uint32_t init[8] = {0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0};
    DANN_HIP(hipMemcpyAsync(d_acc.p, init, 32, hipMemcpyHostToDevice, st));
    if (ids) {
        DANN_HIP(d_ids.alloc((size_t)n * 4));
        DANN_HIP(hipMemcpyAsync(d_ids.p, ids, (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    DegreeArgs a;
    a.adj = idx->d_adj;
    a.adj_stride = idx->cfg.max_degree + 1u;
    a.max_degree = idx->cfg.max_degree;
    a.nslots = idx->nslots;
    a.ids = ids ? d_ids.as<uint32_t>() : nullptr;
    a.n = n;
    a.skip = (flags & DANN_DEGREE_SKIP_DELETED) ? idx->d_deleted : nullptr;
    a.sums = d_acc.as<unsigned long long>();
    a.minmax = d_acc.as<uint32_t>() + 6;
    hipLaunchKernelGGL(degree_stats_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, a);
    DANN_HIP(hipGetLastError());
    uint32_t h[8];
    DANN_HIP(hipMemcpyAsync(h, d_acc.p, 32, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    uint64_t sums[3];
    memcpy(sums, h, 24);
    if (sums[1] == 0) return DANN_OK;  // (the reference's guard against the division by zero: all zeros)
    out->max_degree = h[7];
    out->min_degree = h[6];
    out->avg_degree = (float)sums[0] / (float)sums[1];  // `total as f32 / total_live_points as f32` (index.rs:2220-2234)
    out->cnt_less_than_two = sums[2];
    out->points = sums[1];
    out->total = sums[0];
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_prune_range(dann_index* idx, const dann_build_config* cfg, const uint32_t* ids, uint32_t first, uint32_t n,
                         uint64_t* out_counters) try {
    if (!idx || !cfg) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    if (int32_t rc = check_build_cfg(idx, cfg, "dann_prune_range", false)) return rc;
    if (ids) {
        for (uint32_t i = 0; i < n; ++i)
            if (ids[i] >= idx->nslots) {
                set_error("dann_prune_range: id %u out of bounds (%u slots)", ids[i], idx->nslots);
                return DANN_EBOUNDS;
            }
    } else if ((uint64_t)first + n > idx->nslots) {
        set_error("dann_prune_range: slots [%u, %llu) are out of bounds (%u slots)", first,
                  (unsigned long long)first + n, idx->nslots);
        return DANN_EBOUNDS;
    }
    if (out_counters)
        for (int i = 0; i < 6; ++i) out_counters[i] = 0;
    if (n == 0) return DANN_OK;
    DeviceGuard guard(idx->device);
    ListPrunePass pass;
    pass.who = "dann_prune_range";
    pass.ids = ids;
    pass.first = ids ? 0u : first;
    pass.n = n;
    pass.prune_range = true;
    pass.want_counters = out_counters != nullptr;
    if (int32_t rc = run_list_prunes(idx, cfg, pass)) return rc;
    if (out_counters) {
        out_counters[0] = pass.scanned;
        out_counters[1] = pass.pruned + pass.rewritten;  // (rewritten: a pool that unreadable neighbours emptied)
        out_counters[2] = pass.largest;
        out_counters[3] = pass.distances;
        out_counters[4] = pass.on_matrix_cores;
        out_counters[5] = pass.unreadable;
    }
    return DANN_OK;
} DANN_CATCH_ALL

}  // extern "C"
