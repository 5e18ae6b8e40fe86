// flat_pq_kernels.hip -- exhaustive k-NN over PQ code rows: the reference's product-exhaustive-search
// (diskann-benchmark/src/exhaustive/product.rs; algos::linear_search, exhaustive/algos.rs:42-99) for a batch of queries.
//
// Per query the reference builds a QueryComputer -- the lookup table of populate_chunk_distances_impl -- and streams every
// code row in id order through NeighborPriorityQueue::insert on a queue of k entries.  A row's distance is
// pq_dist_lookup_single (fixed_chunk_pq_table.rs:82-100): the table entries of its bytes added in chunk order, in f32,
// from +0.0.  The queue's result is the first k non-NaN rows under the strict total order of flat_kernels.hip, the key
// dist_key(d, ~slot).  The running sum is never -0.0 (+0.0 + -0.0 == +0.0, and x + -x == +0.0), so the key loses nothing
// of a distance: the merge unpacks the winners' distances, it does not evaluate them again.
//
//   launch_pq_lut        pq_lut_kernel (pq_kernels.hip), device to device: [query][chunk][256] f32, once per query
//   flat_pq_scan_kernel  a workgroup owns a tile of T queries x a chunk of slots.  It stages the tile's tables into LDS
//                        interleaved -- entry (c, b) of query t at ((c * 256 + b) * T + t) * 4 -- so that one
//                        ds_read_b32 / b64 / b128 (two b128 at T = 8) per (row, chunk) delivers all T entries.  Lane =
//                        row (512 threads, or 1024: flat_pq_plan.h): a lane loads its code row 16 bytes at a time, the next 16 bytes (of this row or of the
//                        lane's next row) requested before the current ones are consumed, and walks the chunks in order
//                        with T running sums.  Loads go out unconditionally at clamped addresses; a slot past the chunk,
//                        unpublished, deleted or filtered out is deselected afterwards.  Selection is flat_scan_kernel's:
//                        keys below the query's current k-th key go to an LDS buffer (one LDS atomic per wavefront and
//                        step), sorted and cut to k before it could overflow; the chunk's best k go to scratch.
//   flat_pq_merge_kernel flat_merge_rounds over a query's chunk lists, then ids, unpacked distances and statistics
#include "flat_impl.h"
#include "flat_pq_plan.h"

namespace dann {
namespace {


struct FlatPqArgs {
    const float* lut;  // [nq][chunks][256]
    uint32_t nq;
    uint32_t first, n, k;
    uint32_t chunk_rows, nchunks;
    uint32_t cap, merge_cap;
    const uint32_t* deleted;  // the deleted bitmap when it is to be honoured, else null
    const uint32_t* fbits;    // the filter's bitmaps (null: every slot matches), fstride words apart (0: one for all)
    uint64_t fstride;
    uint64_t* lists;       // [nq][nchunks][k] keys, ascending, kFlatNoKey behind the last
    uint32_t* chunk_cmps;  // [nq][nchunks] rows evaluated
    uint32_t* out_ids;
    float* out_dists;
    dann_search_stats* stats;  // may be null
};

// the T entries of one (chunk, centroid): one LDS read of 4 T bytes (two of 16 at T = 8)
template <int T>
struct alignas(T >= 4 ? 16 : 4 * T) TableEntry {
    float v[T];
};

// The tile's tables in LDS.  The layout that is built is the interleaved one.  DANN_FLAT_PQ_SPLIT_TABLES compiles the
// other layout of DESIGN.md 3.20.2 -- one table of `entries` f32 per query, T ds_read_b32 per (row, chunk) -- into a
// second library that scratch/pq_linear_rate.py times next to this one; nothing else differs.
template <int T>
struct TileTables {
    TableEntry<T>* tab;
    uint32_t entries;  // chunks * 256
    __device__ __forceinline__ TableEntry<T> get(uint32_t e) const {
#ifdef DANN_FLAT_PQ_SPLIT_TABLES
        TableEntry<T> x;
#pragma unroll
        for (int t = 0; t < T; ++t) x.v[t] = reinterpret_cast<const float*>(tab)[(uint32_t)t * entries + e];
        return x;
#else
        return tab[e];
#endif
    }
    __device__ __forceinline__ void put(uint32_t e, const TableEntry<T>& x) const {
#ifdef DANN_FLAT_PQ_SPLIT_TABLES
#pragma unroll
        for (int t = 0; t < T; ++t) reinterpret_cast<float*>(tab)[(uint32_t)t * entries + e] = x.v[t];
#else
        tab[e] = x;
#endif
    }
};

// acc[t] += table[c][byte j of w][t] for the M chunks c = c0 + j, in this order (M a constant: the reads of a group go out
// together and are consumed as they return)
template <int T, int M>
__device__ __forceinline__ void pq_add_chunks(float (&acc)[T], const TileTables<T>& tab, uint32_t c0, const uint4& w) {
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
    TableEntry<T> e[M];
#pragma unroll
    for (int j = 0; j < M; ++j) e[j] = tab.get((c0 + j) * 256u + ((words[j >> 2] >> (8 * (j & 3))) & 255u));
#pragma unroll
    for (int j = 0; j < M; ++j) {
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = acc[t] + e[j].v[t];
    }
}

template <int T, uint32_t kThreads>
__global__ __launch_bounds__(kThreads) void flat_pq_scan_kernel(IndexView ix, FlatPqArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr uint32_t kStep = kThreads;  // lane = row
    const uint32_t chunks = ix.pq_chunks;
    // LDS: the tile's tables, interleaved | T candidate buffers | T threshold keys | T fill counts | T cmps
    const TileTables<T> tab{reinterpret_cast<TableEntry<T>*>(smem), chunks * 256u};
    uint64_t* const bufs = reinterpret_cast<uint64_t*>(smem + (size_t)chunks * kFlatPqTableBytes * T);
    uint64_t* const thr = bufs + (size_t)T * a.cap;
    uint32_t* const cnt = reinterpret_cast<uint32_t*>(thr + T);
    uint32_t* const cmps = cnt + T;

    const uint32_t chunk = blockIdx.x, q0 = blockIdx.y * T;
    const uint32_t tq = a.nq - q0 < (uint32_t)T ? a.nq - q0 : (uint32_t)T;
    // (first + n <= the index's slots: a chunk's bounds fit 32 bits)
    const uint64_t lo64 = (uint64_t)a.first + (uint64_t)chunk * a.chunk_rows, end = (uint64_t)a.first + a.n;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)(lo64 + a.chunk_rows < end ? lo64 + a.chunk_rows : end);

    {
        const uint32_t entries = chunks * 256u;
        const float* src = a.lut + (uint64_t)q0 * entries;
        for (uint32_t e = threadIdx.x; e < entries; e += kThreads) {
            TableEntry<T> x;
#pragma unroll
            for (int t = 0; t < T; ++t) x.v[t] = (uint32_t)t < tq ? src[(uint64_t)t * entries + e] : 0.0f;
            tab.put(e, x);
        }
    }
    if (threadIdx.x < (uint32_t)T) {
        thr[threadIdx.x] = kFlatNoKey;
        cnt[threadIdx.x] = 0;
        cmps[threadIdx.x] = 0;
    }
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t groups = (chunks + 15u) >> 4;  // 16-byte pieces of a code row (row_stride is a multiple of 16)
    const uint32_t tail = chunks - (groups - 1u) * 16u;  // chunks of the last piece: 1 .. 16
    uint32_t evaluated[T];
#pragma unroll
    for (int t = 0; t < T; ++t) evaluated[t] = 0;

    // the slot a lane scores in the step from s0 on: past the chunk it reads the chunk's first row
    auto slot_of = [&](uint32_t s0) -> uint32_t {
        const uint32_t s = s0 + threadIdx.x;  // (s0 < hi < 2^31: no wrap)
        return s < hi ? s : lo;
    };
    uint4 next = *reinterpret_cast<const uint4*>(ix.rows + (uint64_t)slot_of(lo) * ix.row_stride);
    for (uint32_t s0 = lo; s0 < hi; s0 += kStep) {
        const bool in = s0 + threadIdx.x < hi;
        const uint32_t id = slot_of(s0);
        const uint8_t* const row = ix.rows + (uint64_t)id * ix.row_stride;
        // (s0 + kStep may reach hi: slot_of clamps, and the load after the last step is of the chunk's first row)
        const uint8_t* const row_after = ix.rows + (uint64_t)slot_of(s0 + kStep < hi ? s0 + kStep : lo) * ix.row_stride;
        bool ok = in;
        if (ix.tag_off) ok = ok && row[ix.tag_off] >= kTagReadable;
        if (a.deleted) ok = ok && !in_bitmap(a.deleted, id, ix.nslots);
        float acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = 0.0f;
        for (uint32_t g = 0; g < groups; ++g) {
            const uint4 w = next;
            next = *reinterpret_cast<const uint4*>(g + 1u < groups ? row + 16u * (g + 1u) : row_after);
            if (g + 1u < groups || tail == 16u) {
                pq_add_chunks<T, 16>(acc, tab, g * 16u, w);
            } else {
                for (uint32_t j = 0; j < tail; ++j) {
                    const uint32_t word = j < 4u ? w.x : j < 8u ? w.y : j < 12u ? w.z : w.w;
                    const uint32_t b = (word >> (8u * (j & 3u))) & 255u;
                    const TableEntry<T> e = tab.get((g * 16u + j) * 256u + b);
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[t] = acc[t] + e.v[t];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if ((uint32_t)t < tq) {
                bool okt = ok;
                if (a.fbits) okt = okt && ((a.fbits[(uint64_t)(q0 + t) * a.fstride + (id >> 5)] >> (id & 31u)) & 1u);
                evaluated[t] += (uint32_t)__popcll(ballot64(okt));  // (the same in every lane of a wavefront)
                const float d = acc[t];
                const uint64_t key = dist_key(d, ~id);
                const bool push = okt && d == d && key < thr[t];  // (queue.rs: a NaN distance is dropped)
                const uint64_t m = ballot64(push);
                if (m) {
                    uint32_t base = 0;
                    const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
                    if (lane == leader) base = atomicAdd(&cnt[t], (uint32_t)__popcll(m));
                    base = (uint32_t)__shfl((int)base, (int)leader);
                    if (push) bufs[(size_t)t * a.cap + base + mbcnt(m)] = key;
                }
            }
        }
        __syncthreads();
        for (uint32_t t = 0; t < tq; ++t) {
            const uint32_t fill = cnt[t];  // (the same for the whole workgroup)
            if (fill + kStep > a.cap) flat_cut_to_k<kThreads>(bufs + (size_t)t * a.cap, a.cap, fill, a.k, &cnt[t], &thr[t]);
        }
        __syncthreads();
    }
    // the chunk's best k keys of every query, ascending, kFlatNoKey behind the last; and the rows it evaluated
#pragma unroll
    for (int t = 0; t < T; ++t)
        if ((uint32_t)t < tq && lane == 0 && evaluated[t]) atomicAdd(&cmps[t], evaluated[t]);
    for (uint32_t t = 0; t < tq; ++t) {
        const uint32_t fill = cnt[t];
        uint64_t* keys = bufs + (size_t)t * a.cap;
        flat_cut_to_k<kThreads>(keys, a.cap, fill, a.k, &cnt[t], &thr[t]);
        uint64_t* out = a.lists + ((uint64_t)(q0 + t) * a.nchunks + chunk) * a.k;
        for (uint32_t i = threadIdx.x; i < a.k; i += kThreads) out[i] = keys[i];  // (cap > k: pads are in place)
    }
    __syncthreads();
    if (threadIdx.x < tq) a.chunk_cmps[(uint64_t)(q0 + threadIdx.x) * a.nchunks + chunk] = cmps[threadIdx.x];
}

__global__ __launch_bounds__(kFlatThreads) void flat_pq_merge_kernel(FlatPqArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint64_t* const keys = reinterpret_cast<uint64_t*>(smem);
    const uint32_t qi = blockIdx.x, k = a.k;
    flat_merge_rounds(keys, a.lists + (uint64_t)qi * a.nchunks * k, (uint64_t)a.nchunks * k, k, a.merge_cap);
    for (uint32_t r = threadIdx.x; r < k; r += kFlatThreads) {
        const uint64_t key = keys[r];
        const bool has = key != kFlatNoKey;
        a.out_ids[(uint64_t)qi * k + r] = has ? ~(uint32_t)key : kEmpty;
        a.out_dists[(uint64_t)qi * k + r] = has ? key_dist(key) : __builtin_inff();
    }
    if (a.stats && threadIdx.x == 0) flat_merge_stats(a.stats + qi, keys, k, a.chunk_cmps + (uint64_t)qi * a.nchunks, a.nchunks);
}

template <int T>
int32_t launch_scan(const IndexView& ix, const FlatPqPlan& plan, const FlatPqArgs& a, hipStream_t stream) {
    const dim3 grid(plan.nchunks, (a.nq + T - 1) / T);
    if (plan.threads == kFlatPqWideThreads)
        return launch_kernel<flat_pq_scan_kernel<T, kFlatPqWideThreads>>("flat_pq_scan_kernel launch", grid, dim3(kFlatPqWideThreads),
                                                                         plan.scan_lds, stream, ix, a);
    return launch_kernel<flat_pq_scan_kernel<T, kFlatPqThreads>>("flat_pq_scan_kernel launch", grid, dim3(kFlatPqThreads),
                                                                 plan.scan_lds, stream, ix, a);
}

}  // namespace

// One batch of queries (nq <= plan.batch) over slots [first, first + n), n > 0.  `scratch`: plan.scratch_bytes().
// d_filter: the bitmaps of these queries (null: every slot matches), `stride` words apart (0: one for all).
int32_t launch_flat_pq_search(const IndexView& ix, const FlatPqPlan& plan, const float* d_queries, uint32_t nq, uint32_t first,
                              uint32_t n, const uint32_t* d_deleted, const uint32_t* d_filter, uint64_t stride, void* scratch,
                              uint32_t* d_ids, float* d_dists, dann_search_stats* d_stats, hipStream_t stream) {
    float* const lut = reinterpret_cast<float*>(scratch);
    if (int32_t rc = launch_pq_lut(ix.metric, ix.pq_pivots, ix.pq_offsets, ix.pq_chunks, ix.dim, d_queries, nq, lut, stream))
        return rc;
    FlatPqArgs a;
    a.lut = lut;
    a.nq = nq;
    a.first = first;
    a.n = n;
    a.k = plan.k;
    a.chunk_rows = plan.chunk_rows;
    a.nchunks = plan.nchunks;
    a.cap = plan.cap;
    a.merge_cap = plan.merge_cap;
    a.deleted = d_deleted;
    a.fbits = d_filter;
    a.fstride = stride;
    a.lists = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(scratch) + plan.table_bytes());
    a.chunk_cmps = reinterpret_cast<uint32_t*>(a.lists + (size_t)plan.batch * plan.nchunks * plan.k);
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.stats = d_stats;
    int32_t rc = DANN_EINVAL;
    switch (plan.tile) {
        case 8: rc = launch_scan<8>(ix, plan, a, stream); break;
        case 4: rc = launch_scan<4>(ix, plan, a, stream); break;
        case 2: rc = launch_scan<2>(ix, plan, a, stream); break;
        case 1: rc = launch_scan<1>(ix, plan, a, stream); break;
        default: set_error("dann_pq_linear_search_batch: no query tile of %u", plan.tile); break;
    }
    if (rc != DANN_OK) return rc;
    return launch_kernel<flat_pq_merge_kernel>("flat_pq_merge_kernel launch", dim3(nq), dim3(kFlatThreads), plan.merge_lds,
                                               stream, a);
}

}  // namespace dann
