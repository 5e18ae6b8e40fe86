// flat_impl.h -- what the exhaustive scans share on the device: the launch arguments of the k-NN scan and its merge
// (flat_kernels.hip), the staging of a query image in LDS, the sort-and-cut of a candidate buffer and the rounds of the
// merge.  The filtered scan (flat_gt_kernels.hip) fills the same chunk lists and is finished by the same merge; the scan
// over PQ code rows (flat_pq_kernels.hip) cuts its buffers and merges its lists with the same functions.
#pragma once
#include "dann_device.h"
#include "dann_internal.h"
#include "flat_plan.h"
#include "wave_lists.h"

namespace dann {

constexpr int kFlatWave = 64;
constexpr int kFlatU = 4;  // rows per lane group and step
constexpr uint64_t kFlatNoKey = ~0ull;

struct FlatArgs {
    const void* queries;      // nq images of ix.qbytes
    uint32_t nq;
    uint32_t first, n, k;
    uint32_t chunk_rows, nchunks;
    uint32_t tile, cap, qslot;
    uint32_t merge_cap;
    const uint32_t* deleted;  // the deleted bitmap when it is to be honoured, else null
    uint64_t* lists;          // [nq][nchunks][k] keys, ascending, kFlatNoKey behind the last
    uint32_t* chunk_cmps;     // rows evaluated: [nchunks] (the same for every query) or, under a filter, [nq][nchunks]
    uint32_t* out_ids;
    float* out_dists;
    dann_search_stats* stats;  // may be null
};
// (the k-NN scan's argument block: what only the filtered scan or the merge needs is a kernel argument of its own)
static_assert(sizeof(FlatArgs) == 96, "FlatArgs is the unfiltered scan's argument block and keeps its layout");

template <int DT, int OP>
__device__ __forceinline__ void flat_stage_query(const IndexView& ix, const void* queries, uint32_t qi, uint8_t* slot) {
    using S = Scheme<DT, OP, false>;
    using RT = typename RowType<DT>::type;
    const uint8_t* qsrc = reinterpret_cast<const uint8_t*>(queries) + (uint64_t)qi * ix.qbytes;
    uint8_t* qs = slot + query_stage_off(DT);
    if constexpr (S::kInt) {
        stage_int_query<DT>(qs, qsrc, ix.qbytes, ix.dim, threadIdx.x, blockDim.x);
    } else {
        const RT* src = reinterpret_cast<const RT*>(qsrc);
        for (uint32_t i = threadIdx.x; i < ix.dim; i += blockDim.x) reinterpret_cast<float*>(qs)[i] = load1(src + i);
    }
}

// sorts keys[0, cap) (the first `fill` are set) and returns min(fill, k) through *count, the k-th key through *thr; by a
// workgroup of THREADS threads
template <uint32_t THREADS = kFlatThreads>
__device__ __forceinline__ void flat_cut_to_k(uint64_t* keys, uint32_t cap, uint32_t fill, uint32_t k, uint32_t* count,
                                              uint64_t* thr) {
    for (uint32_t i = fill + threadIdx.x; i < cap; i += THREADS) keys[i] = kFlatNoKey;
    __syncthreads();
    block_bitonic(keys, cap, THREADS);
    if (threadIdx.x == 0) {
        *count = fill < k ? fill : k;
        *thr = fill < k ? kFlatNoKey : keys[k - 1];
    }
}

// The merge's rounds: the best k of lists[0, total) (ascending runs of k keys, kFlatNoKey behind a run's last) end up in
// keys[0, k), ascending.  keys holds P keys, a power of two >= 2 k: keys[0, k) is the best so far, keys[k, P) takes the
// next P - k keys of the lists, and a round sorts both.  Ends with a barrier.
__device__ __forceinline__ void flat_merge_rounds(uint64_t* keys, const uint64_t* lists, uint64_t total, uint32_t k, uint32_t P) {
    for (uint32_t i = threadIdx.x; i < k; i += kFlatThreads) keys[i] = kFlatNoKey;
    for (uint64_t base = 0; base < total; base += P - k) {
        for (uint32_t i = k + threadIdx.x; i < P; i += kFlatThreads) {
            const uint64_t j = base + (i - k);
            keys[i] = j < total ? lists[j] : kFlatNoKey;
        }
        __syncthreads();
        block_bitonic(keys, P, kFlatThreads);
    }
    __syncthreads();
}

// one thread writes a merged query's statistics: cmps = the rows its chunks evaluated, written = the keys that are left
__device__ __forceinline__ void flat_merge_stats(dann_search_stats* out, const uint64_t* keys, uint32_t k, const uint32_t* chunk_cmps,
                                                 uint32_t nchunks) {
    uint32_t written = 0;
    for (uint32_t r = 0; r < k; ++r) written += keys[r] != kFlatNoKey ? 1u : 0u;
    uint32_t cmps = 0;
    for (uint32_t c = 0; c < nchunks; ++c) cmps += chunk_cmps[c];
    dann_search_stats st;
    st.cmps = cmps;
    st.hops = 0;
    st.result_count = written;  // (no Translate post-processor on this path: min(k, rows inserted))
    st.status = 0;
    st.written = written;
    *out = st;
}

// flat_kernels.hip: the merge of the chunk lists of a.nq queries into a.out_ids / a.out_dists / a.stats; query q's rows
// evaluated are a.chunk_cmps[q * cmps_stride + c] (0: one count per chunk for all; nchunks under a filter)
int32_t launch_flat_merge(const IndexView& ix, const FlatArgs& a, uint32_t cmps_stride, size_t merge_lds, hipStream_t stream);

}  // namespace dann
