// flat_kernels.hip -- exhaustive k-NN over a range of slots: diskann::flat::FlatIndex::knn_search
// (diskann/src/flat/index.rs:57-99) for a batch of queries.
//
// The reference streams every element in ascending id order through NeighborPriorityQueue::insert
// (diskann/src/neighbor/queue.rs:130-171) on a queue of capacity k.  Its result is the first k non-NaN elements under the
// strict total order (distance ascending with -0.0 == +0.0, scan position descending): the 64-bit key
// dist_key(d, ~slot).  A strict order has one answer whatever the tiling, so:
//
//   flat_scan_kernel   a workgroup owns one tile of queries x one chunk of slots; every distance is the search path's
//                      group_distance_many + finish_distance, unchanged; keys below the query's current k-th key go to
//                      an LDS buffer that is sorted and cut to k when it fills; the chunk's best k keys go to scratch
//   flat_merge_kernel  one workgroup per query merges its chunk lists in rounds of sort and cut, evaluates the
//                      distances of the k rows that are left (a key folds -0.0 into +0.0; the result carries the
//                      distance itself) and writes ids, distances and statistics
#include "flat_impl.h"

namespace dann {
namespace {

constexpr int kWave = kFlatWave;
constexpr int kU = kFlatU;
constexpr uint64_t kNoKey = kFlatNoKey;

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kFlatThreads) void flat_scan_kernel(IndexView ix, FlatArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using S = Scheme<DT, OP, false>;
    constexpr int G = S::G, GROUPS = kWave / G;
    constexpr uint32_t kStep = (kFlatThreads / G) * kU;  // rows a workgroup scores per step
    static_assert(kStep <= kFlatStepRows, "a step must fit the headroom of the candidate buffers");
    using QT = typename std::conditional<S::kInt, uint8_t, float>::type;
    // LDS: tile staged queries | tile candidate buffers | tile threshold keys | tile fill counts | cmps
    uint8_t* const qbase = smem;
    uint64_t* const bufs = reinterpret_cast<uint64_t*>(smem + (size_t)a.tile * a.qslot);
    uint64_t* const thr = bufs + (size_t)a.tile * a.cap;
    uint32_t* const cnt = reinterpret_cast<uint32_t*>(thr + a.tile);
    uint32_t* const cmps = cnt + a.tile;

    const uint32_t chunk = blockIdx.x, q0 = blockIdx.y * a.tile;
    const uint32_t tq = a.nq - q0 < a.tile ? a.nq - q0 : a.tile;
    const uint64_t lo = (uint64_t)a.first + (uint64_t)chunk * a.chunk_rows;
    const uint64_t end = (uint64_t)a.first + a.n;
    const uint64_t hi = lo + a.chunk_rows < end ? lo + a.chunk_rows : end;
    const SqParams sqp{ix.sq_k, ix.sq_shift_norm_sq};

    for (uint32_t t = 0; t < tq; ++t) flat_stage_query<DT, OP>(ix, a.queries, q0 + t, qbase + (size_t)t * a.qslot);
    if (threadIdx.x < a.tile) {
        thr[threadIdx.x] = kNoKey;
        cnt[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) *cmps = 0;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int g = lane / G, v = lane % G;
    uint32_t evaluated = 0;
    for (uint64_t s0 = lo; s0 < hi; s0 += kStep) {
        // loads go out unconditionally at clamped addresses (a slot that is past the chunk, unpublished or deleted
        // reads the chunk's first row) and are selected afterwards
        const uint8_t* rows[kU];
        bool act[kU];
        uint32_t id[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint64_t s = s0 + (uint64_t)((wave * kU + u) * GROUPS + g);
            const bool in = s < hi;
            id[u] = (uint32_t)(in ? s : lo);
            rows[u] = ix.rows + (uint64_t)id[u] * ix.row_stride;
            bool ok = in;
            if (ix.tag_off) ok = ok && rows[u][ix.tag_off] >= kTagReadable;
            if (a.deleted) ok = ok && !in_bitmap(a.deleted, id[u], ix.nslots);
            act[u] = ok;
            if (!ok) rows[u] = ix.rows + lo * ix.row_stride;
            evaluated += (ok && v == 0) ? 1u : 0u;
        }
        for (uint32_t t = 0; t < tq; ++t) {
            const QT* qs = reinterpret_cast<const QT*>(qbase + (size_t)t * a.qslot + query_stage_off(DT));
            float o[kU];
            group_distance_many<DT, OP, false, kU, false>(qs, rows, act, (int)ix.dim, v, o);
            const uint64_t limit = thr[t];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if (act[u] && v == 0) {
                    const float d = finish_distance<DT, OP, NORM>(o[u], reinterpret_cast<const uint8_t*>(qs), rows[u], ix.dim, sqp);
                    if (d == d) {  // (queue.rs: a NaN distance is dropped)
                        const uint64_t key = dist_key(d, ~id[u]);
                        if (key < limit) bufs[(size_t)t * a.cap + atomicAdd(&cnt[t], 1u)] = key;
                    }
                }
            }
        }
        __syncthreads();
        for (uint32_t t = 0; t < tq; ++t) {
            const uint32_t fill = cnt[t];  // (the same for the whole workgroup)
            if (fill + kStep > a.cap) flat_cut_to_k(bufs + (size_t)t * a.cap, a.cap, fill, a.k, &cnt[t], &thr[t]);
        }
        __syncthreads();
    }
    // the chunk's best k keys of every query, ascending, kNoKey behind the last
    for (uint32_t t = 0; t < tq; ++t) {
        const uint32_t fill = cnt[t];
        uint64_t* keys = bufs + (size_t)t * a.cap;
        flat_cut_to_k(keys, a.cap, fill, a.k, &cnt[t], &thr[t]);
        uint64_t* out = a.lists + ((uint64_t)(q0 + t) * a.nchunks + chunk) * a.k;
        for (uint32_t i = threadIdx.x; i < a.k; i += kFlatThreads) out[i] = keys[i];  // (cap > k: pads are in place)
    }
    if (blockIdx.y == 0) {
        if (evaluated) atomicAdd(cmps, evaluated);
        __syncthreads();
        if (threadIdx.x == 0) a.chunk_cmps[chunk] = *cmps;
    }
}

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kFlatThreads) void flat_merge_kernel(IndexView ix, FlatArgs a, uint32_t cmps_stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using S = Scheme<DT, OP, false>;
    constexpr int G = S::G, GROUPS = kFlatThreads / G;
    using QT = typename std::conditional<S::kInt, uint8_t, float>::type;
    uint64_t* const keys = reinterpret_cast<uint64_t*>(smem);
    uint8_t* const qslot = smem + (size_t)a.merge_cap * 8;
    const uint32_t qi = blockIdx.x, k = a.k, P = a.merge_cap;
    flat_stage_query<DT, OP>(ix, a.queries, qi, qslot);
    flat_merge_rounds(keys, a.lists + (uint64_t)qi * a.nchunks * k, (uint64_t)a.nchunks * k, k, P);
    const SqParams sqp{ix.sq_k, ix.sq_shift_norm_sq};
    const QT* qs = reinterpret_cast<const QT*>(qslot + query_stage_off(DT));
    const int g = threadIdx.x / G, v = threadIdx.x % G;
    const uint64_t safe = (uint64_t)a.first;  // n > 0 here: a readable slot
    for (uint32_t r0 = 0; r0 < k; r0 += GROUPS * kU) {
        const uint8_t* rows[kU];
        bool act[kU];
        uint32_t id[kU];
        float o[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t r = r0 + u * GROUPS + g;
            const uint64_t key = r < k ? keys[r] : kNoKey;
            act[u] = key != kNoKey;
            id[u] = act[u] ? ~(uint32_t)key : kEmpty;
            rows[u] = ix.rows + (act[u] ? (uint64_t)id[u] : safe) * ix.row_stride;
        }
        group_distance_many<DT, OP, false, kU, false>(qs, rows, act, (int)ix.dim, v, o);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const uint32_t r = r0 + u * GROUPS + g;
            if (r < k && v == 0) {
                float d = __builtin_inff();
                if (act[u]) d = finish_distance<DT, OP, NORM>(o[u], reinterpret_cast<const uint8_t*>(qs), rows[u], ix.dim, sqp);
                a.out_ids[(uint64_t)qi * k + r] = id[u];
                a.out_dists[(uint64_t)qi * k + r] = d;
            }
        }
    }
    if (a.stats && threadIdx.x == 0)
        flat_merge_stats(a.stats + qi, keys, k, a.chunk_cmps + (uint64_t)qi * cmps_stride, a.nchunks);
}

// n == 0: nothing was scanned
__global__ void flat_empty_kernel(uint32_t nq, uint32_t k, uint32_t* out_ids, float* out_dists, dann_search_stats* stats) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (uint64_t)nq * k) {
        out_ids[i] = kEmpty;
        out_dists[i] = __builtin_inff();
    }
    if (stats && i < nq) stats[i] = dann_search_stats{0, 0, 0, 0, 0};
}

}  // namespace

uint32_t flat_query_slot_bytes(const IndexView& ix) {
    const bool is_int = !(ix.dtype == DT_F32 || ix.dtype == DT_F16);
    return ((is_int ? int_query_slot_bytes(ix.dtype, ix.qbytes) : ix.dim * 4u) + 15u) & ~15u;
}

int32_t launch_flat_empty(uint32_t nq, uint32_t k, uint32_t* d_ids, float* d_dists, dann_search_stats* d_stats,
                          hipStream_t stream) {
    const uint64_t cells = (uint64_t)nq * k > nq ? (uint64_t)nq * k : nq;
    return launch_kernel<flat_empty_kernel>("flat_empty_kernel launch", dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0,
                                            stream, nq, k, d_ids, d_dists, d_stats);
}

// One batch of queries (nq <= plan.batch) over slots [first, first + n), n > 0.  `scratch`: plan.scratch_bytes().
int32_t launch_flat_search(const IndexView& ix, const FlatPlan& plan, const void* d_queries, uint32_t nq, uint32_t first,
                           uint32_t n, const uint32_t* d_deleted, void* scratch, uint32_t* d_ids, float* d_dists,
                           dann_search_stats* d_stats, hipStream_t stream) {
    FlatArgs a;
    a.queries = d_queries;
    a.nq = nq;
    a.first = first;
    a.n = n;
    a.k = plan.k;
    a.chunk_rows = plan.chunk_rows;
    a.nchunks = plan.nchunks;
    a.tile = plan.tile;
    a.cap = plan.cap;
    a.qslot = flat_query_slot_bytes(ix);
    a.merge_cap = plan.merge_cap;
    a.deleted = d_deleted;
    a.lists = reinterpret_cast<uint64_t*>(scratch);
    a.chunk_cmps = reinterpret_cast<uint32_t*>(a.lists + (size_t)plan.batch * plan.nchunks * plan.k);
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.stats = d_stats;
    const uint32_t tiles = (nq + plan.tile - 1) / plan.tile;
    const int32_t rc = dispatch_row_op<kRowsQuery>(ix.dtype, ix.metric, [&](auto r) {
        using R = decltype(r);
        int32_t e = launch_kernel<flat_scan_kernel<R::dt, R::op, R::norm>>("flat_scan_kernel launch", dim3(plan.nchunks, tiles),
                                                                          dim3(kFlatThreads), plan.scan_lds, stream, ix, a);
        if (e != DANN_OK) return e;
        return launch_kernel<flat_merge_kernel<R::dt, R::op, R::norm>>("flat_merge_kernel launch", dim3(nq), dim3(kFlatThreads),
                                                                       plan.merge_lds, stream, ix, a, 0u);
    });
    if (rc != kNoRow) return rc;
    set_error("dann_flat_search_batch: not defined on rows of dtype %d", ix.dtype);
    return DANN_EUNSUPPORTED;
}

int32_t launch_flat_merge(const IndexView& ix, const FlatArgs& a, uint32_t cmps_stride, size_t merge_lds, hipStream_t stream) {
    const int32_t rc = dispatch_row_op<kRowsQuery>(ix.dtype, ix.metric, [&](auto r) {
        using R = decltype(r);
        return launch_kernel<flat_merge_kernel<R::dt, R::op, R::norm>>("flat_merge_kernel launch", dim3(a.nq), dim3(kFlatThreads),
                                                                       merge_lds, stream, ix, a, cmps_stride);
    });
    if (rc != kNoRow) return rc;
    set_error("flat merge: not defined on rows of dtype %d", ix.dtype);
    return DANN_EUNSUPPORTED;
}

}  // namespace dann
