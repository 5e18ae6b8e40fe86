// query_schedule.hip -- locality scheduling of large Knn search launches (search_with_retry, search_kernels.hip).
//
// One-wave launches of 100 000 queries on 1 M x 128 f32 rows read ~800 random 512-byte rows per query; in caller order
// every XCD's 4 MiB L2 sees the whole index at once (7 % hit rate).  The rows near a query's target are re-read by every
// query of the same region, so running the queries of one region together on one XCD turns those re-reads into L2 hits.
// Per launch: the nearest of P pivots is each query's key; a stable counting sort by key gives the sorted order; the slot
// map of query_schedule.h deals it to the XCDs in contiguous chunks.  The pivots are centres: rows taken at a fixed
// stride over the live slots, then moved by a few Lloyd iterations over a sample of 64 rows per pivot (the key kernel
// assigns, the counting sort groups, one workgroup per centre averages its members in sample order: no float atomics).
// Only the order in which queries run changes -- every query's search is independent of the others and writes its
// results at its own index -- so no result depends on any of this.
//
// Kernels: sched_live_kernel / sched_sample_kernel / sched_pivots_kernel / sched_update_kernel (on the first scheduled
// search and after a mutation: the pivots as scaled f16 in the key kernel's LDS layout), sched_key_kernel
// (v_mfma_f32_32x32x16_f16: queries x pivots inner products), sched_hist_kernel, sched_scan_kernel,
// sched_scatter_kernel (the stable counting sort, writing the slot map directly).
#include <hip/hip_fp16.h>

#include "dann_device.h"
#include "dann_internal.h"
#include "query_schedule.h"

namespace dann {

namespace {

typedef _Float16 sched_f16x8 __attribute__((ext_vector_type(8)));
typedef float sched_f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kKeyThreads = 512;     // 8 waves; one workgroup per CU (the pivot slab is most of the LDS)
constexpr uint32_t kSortThreads = 1024;   // histogram / scatter: 16 waves
constexpr uint32_t kSortPerThread = 2;    // queries per thread of one sort block (49 blocks for 100 000 queries)
constexpr uint32_t kSortBlock = kSortThreads * kSortPerThread;
constexpr uint32_t kPreSteps = 8;         // key kernel: 16-column steps of a query held in registers (dim <= 128)
constexpr uint32_t kLiveScanLimit = 4096; // slots a pivot walks past empty ones before it takes the first start point
constexpr uint32_t kSamplePerPivot = 64;  // training sample: rows per pivot
constexpr uint32_t kSchedLloydIters = 4;  // Lloyd iterations from the stride rows (DANN_DBG_SCHED_LLOYD_ITERS)
constexpr uint32_t kSchedMaxLloydIters = 64;
constexpr int kKeyMaxLds = 144 * 1024;    // the most sched_pivot_count lets a pivot slab take
constexpr uint32_t kUpdateThreads = 128;

// slots in [0, capacity) with a non-empty adjacency list: how many, and one past the highest
__global__ void sched_live_kernel(const uint32_t* adj, uint32_t adj_stride, uint32_t capacity, uint32_t* out2) {
    uint32_t cnt = 0, hi = 0;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < capacity; s += gridDim.x * blockDim.x)
        if (adj[(uint64_t)s * adj_stride] != 0u) {
            ++cnt;
            hi = s + 1u;
        }
    for (int o = 32; o > 0; o >>= 1) {
        cnt += (uint32_t)__shfl_xor((int)cnt, o);
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (cnt) atomicAdd(&out2[0], cnt);
        if (hi) atomicMax(&out2[1], hi);
    }
}

// entry j of n taken at a fixed stride over the live slots: the first live slot at or after j * hi / n (the first start
// point where there is none nearby)
__device__ uint32_t sched_stride_slot(const IndexView& ix, uint32_t hi, uint32_t j, uint32_t n) {
    if (hi) {
        const uint32_t s0 = (uint32_t)((uint64_t)j * hi / n);
        for (uint32_t s = s0; s < hi && s < s0 + kLiveScanLimit; ++s)
            if (ix.adj[(uint64_t)s * ix.adj_stride] != 0u) return s;
    }
    return ix.nstart ? ix.capacity : 0u;
}

// the training sample: row j of ns = stride entry j, widened to f32 (unscaled) into sample[j][dim]; finite[j] = whether
// every coordinate is finite; amax_bits = the largest finite |coordinate| (as bits: non-negative floats order like
// their bits).  One wavefront per sample row.
template <typename T>
__global__ __launch_bounds__(256) void sched_sample_kernel(IndexView ix, const uint32_t* live2, uint32_t ns, float* sample,
                                                           uint8_t* finite, uint32_t* amax_bits) {
    const uint32_t j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (j >= ns) return;
    const uint32_t slot = sched_stride_slot(ix, live2[1], j, ns);
    const T* row = reinterpret_cast<const T*>(ix.rows + (uint64_t)slot * ix.row_stride);
    float m = 0.0f;
    bool fin = true;
    for (uint32_t k = lane; k < ix.dim; k += 64u) {
        const float v = (float)row[k];
        sample[(uint64_t)j * ix.dim + k] = v;
        if (fabsf(v) <= 3.0e38f) m = fmaxf(m, fabsf(v));
        else fin = false;  // (NaN too)
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const bool all_fin = __ballot(!fin) == 0ull;
    if (lane == 0u) {
        finite[j] = all_fin ? 1u : 0u;
        if (m > 0.0f) atomicMax(amax_bits, __float_as_uint(m));
    }
}

// pivot j starts as stride entry j of np, as scaled f16 in rows of `stride` halfs (a non-finite coordinate as 0), then
// the f32 norms of the rounded rows and the scale: a power of two that puts the largest finite |coordinate| of these
// rows and of the training sample (amax_bits, null without training) near 256.  One workgroup of np threads.
template <typename T>
__global__ void sched_pivots_kernel(IndexView ix, const uint32_t* live2, const uint32_t* amax_bits, uint32_t np,
                                    uint32_t stride, _Float16* piv) {
    __shared__ float red[256];
    const uint32_t j = threadIdx.x;
    const uint32_t slot = sched_stride_slot(ix, live2[1], j, np);
    const T* row = reinterpret_cast<const T*>(ix.rows + (uint64_t)slot * ix.row_stride);
    float m = 0.0f;
    for (uint32_t k = 0; k < ix.dim; ++k) {
        const float v = fabsf((float)row[k]);
        if (v <= 3.0e38f) m = fmaxf(m, v);
    }
    red[j] = m;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (j < o && j + o < np) red[j] = fmaxf(red[j], red[j + o]);
        __syncthreads();
    }
    // f16 keeps queries of that magnitude and far beyond
    const float amax = fmaxf(red[0], amax_bits ? __uint_as_float(*amax_bits) : 0.0f);
    const float scale = amax > 0.0f ? exp2f(8.0f - ceilf(log2f(amax))) : 1.0f;
    _Float16* out = piv + (uint64_t)j * stride;
    float nrm = 0.0f;
    for (uint32_t k = 0; k < stride; ++k) {
        const float v = k < ix.dim ? (float)row[k] : 0.0f;
        const _Float16 h = fabsf(v) <= 3.0e38f ? (_Float16)(v * scale) : (_Float16)0.0f;
        out[k] = h;
        nrm = fmaf((float)h, (float)h, nrm);
    }
    float* norms = reinterpret_cast<float*>(piv + (uint64_t)np * stride);
    norms[j] = nrm;
    if (j == 0) norms[np] = scale;
}

// one Lloyd update: centre p <- the mean of its finite sample rows.  `order` holds the sample in centre order, stable
// in sample order (the counting sort with parts = 1), starts[p] = where centre p's members begin.  A thread per
// dimension adds the members in that order in f32 from the unscaled sample; the mean times the scale is rounded to f16
// into the slab, the f32 norm of the rounded values next to it.  A centre without finite members, or whose mean does
// not stay finite, keeps its value.  One workgroup per centre; LDS: dim halfs.
__global__ __launch_bounds__(kUpdateThreads) void sched_update_kernel(const float* sample, const uint8_t* finite,
                                                                      const uint32_t* order, const uint32_t* starts,
                                                                      uint32_t ns, uint32_t dim, uint32_t np,
                                                                      uint32_t stride, _Float16* piv) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sched_smem[];
    _Float16* row = reinterpret_cast<_Float16*>(sched_smem);
    __shared__ uint32_t bad;
    const uint32_t p = blockIdx.x;
    const uint32_t b = min(starts[p], ns), e = p + 1u < np ? min(starts[p + 1u], ns) : ns;
    float* norms = reinterpret_cast<float*>(piv + (uint64_t)np * stride);
    const float scale = norms[np];
    if (threadIdx.x == 0u) bad = 0u;
    uint32_t cnt = 0;
    for (uint32_t m = b; m < e; ++m) cnt += finite[min(order[m], ns - 1u)];
    if (cnt == 0u) return;  // (the whole workgroup)
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < dim; d += blockDim.x) {
        float sum = 0.0f;
        for (uint32_t m = b; m < e; ++m) {
            const uint32_t i = min(order[m], ns - 1u);
            if (finite[i]) sum += sample[(uint64_t)i * dim + d];
        }
        const _Float16 h = (_Float16)(sum / (float)cnt * scale);
        if (!(fabsf((float)h) <= 65504.0f)) bad = 1u;
        row[d] = h;
    }
    __syncthreads();
    if (bad) return;
    _Float16* out = piv + (uint64_t)p * stride;
    for (uint32_t d = threadIdx.x; d < dim; d += blockDim.x) out[d] = row[d];
    if (threadIdx.x == 0u) {
        float nrm = 0.0f;
        for (uint32_t k = 0; k < dim; ++k) nrm = fmaf((float)row[k], (float)row[k], nrm);
        norms[p] = nrm;
    }
}

// keys[q] = the pivot nearest to query q (L2 on the scaled f16 values; ties: the lower pivot).  A wave takes 32 queries x
// all pivots: lane l supplies query / pivot row l & 31, halfs 8 (l >> 5) .. + 7 of each 16-column step, for both operands
// of v_mfma_f32_32x32x16_f16; register r of lane l then holds pivot 32 t + (r & 3) + 8 (r >> 2) + 4 (l >> 5) against
// query l & 31 (the layout gram_tiles_f16_kernel and pq_assign_mfma_kernel use).  LDS: the pivot rows (a row stride of
// 16 mod 256 bytes: the 16-byte reads of 16 consecutive rows cover all 64 banks) and their norms.
template <typename QT>
__global__ __launch_bounds__(kKeyThreads) void sched_key_kernel(const QT* queries, uint32_t nq, uint32_t dim,
                                                                const _Float16* piv, uint32_t np, uint32_t stride,
                                                                uint32_t* keys) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sched_smem[];
    const uint32_t slab = np * stride * 2u, bytes = slab + np * 4u;  // both multiples of 16
    const uint4* src = reinterpret_cast<const uint4*>(piv);
    for (uint32_t i = threadIdx.x; i < bytes / 16u; i += blockDim.x) reinterpret_cast<uint4*>(sched_smem)[i] = src[i];
    const float scale = reinterpret_cast<const float*>(piv + (uint64_t)np * stride)[np];
    __syncthreads();
    const float* norms = reinterpret_cast<const float*>(sched_smem + slab);
    const uint32_t lane = threadIdx.x & 63u, l31 = lane & 31u, hi = lane >> 5;
    const uint32_t nt = np >> 5, ksteps = (dim + 15u) >> 4;
    const uint32_t groups = (nq + 31u) >> 5;
    for (uint32_t g = blockIdx.x * (kKeyThreads / 64u) + (threadIdx.x >> 6); g < groups;
         g += gridDim.x * (kKeyThreads / 64u)) {
        const uint32_t q = g * 32u + l31;
        const QT* qrow = queries + (uint64_t)(q < nq ? q : nq - 1u) * dim;
        sched_f32x16 acc[8];
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        auto frag = [&](uint32_t m) {
            const uint32_t k0 = 16u * m + 8u * hi;
            sched_f16x8 b;
#pragma unroll
            for (int i = 0; i < 8; ++i) b[i] = k0 + i < dim ? (_Float16)((float)qrow[k0 + i] * scale) : (_Float16)0.0f;
            return b;
        };
        auto step = [&](uint32_t m, const sched_f16x8& b) {
            const uint8_t* arow = sched_smem + (uint64_t)l31 * stride * 2u + (16u * m + 8u * hi) * 2u;
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if ((uint32_t)t < nt) {
                    const sched_f16x8 a = *reinterpret_cast<const sched_f16x8*>(arow + (uint64_t)t * 32u * stride * 2u);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[t], 0, 0, 0);
                }
        };
        if (ksteps <= kPreSteps) {  // (dim <= 128) all of the lane's query fragments requested at once: one load latency
            sched_f16x8 pre[kPreSteps];
#pragma unroll
            for (uint32_t m = 0; m < kPreSteps; ++m)
                if (m < ksteps) pre[m] = frag(m);
#pragma unroll
            for (uint32_t m = 0; m < kPreSteps; ++m)
                if (m < ksteps) step(m, pre[m]);
        } else {
            for (uint32_t m = 0; m < ksteps; ++m) step(m, frag(m));
        }
        float best = __builtin_inff();
        uint32_t bi = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if ((uint32_t)t < nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t j = 32u * t + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * hi;
                    const float sc = norms[j] - 2.0f * acc[t][r];
                    if (sc < best) {  // (NaN never wins)
                        best = sc;
                        bi = j;
                    }
                }
        const float ob = __shfl_xor(best, 32);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, 32);
        if ((ob < best) | ((ob == best) & (oi < bi))) bi = oi;
        if (hi == 0u && q < nq) keys[q] = bi;
    }
}

// per sort block (kSortBlock consecutive queries): how many keys of each pivot
__global__ __launch_bounds__(kSortThreads) void sched_hist_kernel(const uint32_t* keys, uint32_t nq, uint32_t np,
                                                                  uint32_t* bh) {
    __shared__ uint32_t h[256];
    for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortBlock;
    for (uint32_t i = threadIdx.x; i < kSortBlock && base + i < nq; i += blockDim.x) atomicAdd(&h[keys[base + i]], 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) bh[(uint64_t)blockIdx.x * np + i] = h[i];
}

// bh[b][p] <- the sorted position of the first key p of block b (one workgroup of 256 threads, thread p = pivot p)
__global__ __launch_bounds__(256) void sched_scan_kernel(uint32_t* bh, uint32_t nb, uint32_t np) {
    __shared__ uint32_t tot[2][256];
    const uint32_t p = threadIdx.x;
    uint32_t run = 0;
    if (p < np)
        for (uint32_t b0 = 0; b0 < nb; b0 += 8u) {  // eight blocks' counts requested at once
            uint32_t v[8];
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) v[i] = b0 + i < nb ? bh[(uint64_t)(b0 + i) * np + p] : 0u;
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i)
                if (b0 + i < nb) {
                    bh[(uint64_t)(b0 + i) * np + p] = run;
                    run += v[i];
                }
        }
    tot[0][p] = p < np ? run : 0u;
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t o = 1; o < 256; o <<= 1) {  // inclusive scan over the pivots
        tot[cur ^ 1][p] = tot[cur][p] + (p >= o ? tot[cur][p - o] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    if (p < np) {
        const uint32_t base = tot[cur][p] - run;
        for (uint32_t b = 0; b < nb; ++b) bh[(uint64_t)b * np + p] += base;
    }
}

// stable scatter: query i of block b goes to sorted position bh[b][key] + (earlier keys equal to it in the block), and
// straight on to its slot: qmap[sched_slot(position)] = i
__global__ __launch_bounds__(kSortThreads) void sched_scatter_kernel(const uint32_t* keys, uint32_t nq, uint32_t np,
                                                                     const uint32_t* bh, uint32_t parts, uint32_t* qmap) {
    constexpr uint32_t kWaves = kSortThreads / 64u;
    __shared__ uint32_t run[256];
    __shared__ uint32_t wc[kWaves][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    for (uint32_t i = tid; i < np; i += blockDim.x) run[i] = bh[(uint64_t)blockIdx.x * np + i];
    const uint64_t below = lane ? ~0ull >> (64u - lane) : 0ull;
    for (uint32_t round = 0; round < kSortPerThread; ++round) {
        for (uint32_t i = tid; i < kWaves * 256u; i += blockDim.x) (&wc[0][0])[i] = 0;
        __syncthreads();
        const uint32_t qi = blockIdx.x * kSortBlock + round * kSortThreads + tid;
        const bool valid = qi < nq;
        const uint32_t key = valid ? keys[qi] : 0xFFFFFFFFu;
        // rank among the earlier lanes of this wave with the same key; the first lane of each key stores the count
        uint32_t rank = 0;
        uint64_t todo = __ballot(valid);
        while (todo) {
            const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
            const uint32_t k = (uint32_t)__shfl((int)key, (int)lead);
            const uint64_t same = __ballot(valid && key == k);
            if (valid && key == k) {
                rank = (uint32_t)__builtin_popcountll(same & below);
                if (lane == lead) wc[w][k] = (uint32_t)__builtin_popcountll(same);
            }
            todo &= ~same;
        }
        __syncthreads();
        if (valid) {
            uint32_t pos = run[key] + rank;
            for (uint32_t v = 0; v < w; ++v) pos += wc[v][key];
            if (pos < nq) qmap[sched_slot(pos, nq, parts)] = qi;
        }
        __syncthreads();
        for (uint32_t i = tid; i < np; i += blockDim.x) {
            uint32_t s = 0;
            for (uint32_t v = 0; v < kWaves; ++v) s += wc[v][i];
            run[i] += s;
        }
        __syncthreads();
    }
}

// halfs per pivot row: the dimension rounded up to 16, plus 8 (a row stride of 16 mod 256 bytes)
uint32_t sched_stride(uint32_t dim) { return (dim + 15u) / 16u * 16u + 8u; }

}  // namespace

// pivots the key kernel's LDS holds for this dimension: up to 256, a multiple of 32, the slab at most 144 KiB (0: none)
uint32_t sched_pivot_count(uint32_t dim) {
    const uint64_t per = (uint64_t)sched_stride(dim) * 2u + 4u;
    return (uint32_t)std::min<uint64_t>(256u, (144u * 1024u - 16u) / per / 32u * 32u);
}

namespace {

// the key pass + the stable counting sort of nq keys: keys | per-block histograms in `scratch`, then qmap
template <typename QT>
int32_t sched_sort_by_pivot(const dann_index* idx, hipStream_t st, const QT* queries, uint32_t nq, uint32_t dim,
                            uint32_t parts, uint32_t* scratch, uint32_t* qmap) {
    const uint32_t np = sched_pivot_count(dim), stride = sched_stride(dim);
    const uint32_t lds = np * stride * 2u + np * 4u;
    uint32_t* keys = scratch;
    uint32_t* bh = scratch + nq;
    const uint32_t nb = (nq + kSortBlock - 1u) / kSortBlock;
    const uint32_t groups = (nq + 31u) / 32u;
    const uint32_t kblocks = std::max<uint32_t>(1u, std::min<uint32_t>((groups + kKeyThreads / 64u - 1u) / (kKeyThreads / 64u), idx->num_cus));
    hipLaunchKernelGGL(sched_key_kernel<QT>, dim3(kblocks), dim3(kKeyThreads), lds, st, queries, nq, dim, idx->d_sched_piv,
                       np, stride, keys);
    hipLaunchKernelGGL(sched_hist_kernel, dim3(nb), dim3(kSortThreads), 0, st, keys, nq, np, bh);
    hipLaunchKernelGGL(sched_scan_kernel, dim3(1), dim3(256), 0, st, bh, nb, np);
    hipLaunchKernelGGL(sched_scatter_kernel, dim3(nb), dim3(kSortThreads), 0, st, keys, nq, np, bh, parts, qmap);
    DANN_HIP(hipGetLastError());
    return DANN_OK;
}

template <typename T>
int32_t sched_build_pivots_t(dann_index* idx, hipStream_t st) {
    const IndexView ix = idx->view();
    const uint32_t np = sched_pivot_count(ix.dim), stride = sched_stride(ix.dim);
    const size_t slab = (size_t)np * stride * 2u + (size_t)np * 4u;
    // the key kernel's LDS limit, at every pivot build and not per search: it belongs to the function, not to an index,
    // so it is set to the most any dimension's slab takes (the training runs the kernel on the f32 sample, the searches
    // on the row type)
    DANN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sched_key_kernel<float>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kKeyMaxLds));
    DANN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sched_key_kernel<T>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kKeyMaxLds));
    if (!idx->d_sched_piv) {
        // pivot rows | norms | scale (+pad) | live count, highest live slot
        DANN_HIP(hipMalloc((void**)&idx->d_sched_piv, slab + 64u));
    }
    uint32_t* live2 = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(idx->d_sched_piv) + slab + 32u);
    DANN_HIP(hipMemsetAsync(live2, 0, 8, st));
    const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((ix.capacity + 255u) / 256u, 4u * idx->num_cus));
    if (ix.capacity) hipLaunchKernelGGL(sched_live_kernel, dim3(blocks), dim3(256), 0, st, ix.adj, ix.adj_stride, ix.capacity, live2);
    // the training sample: 64 rows per pivot at a fixed stride over the live slots (an index of fewer slots: one per slot)
    const uint32_t iters = std::min(kSchedMaxLloydIters, idx->dbg_u32(DANN_DBG_SCHED_LLOYD_ITERS, kSchedLloydIters));
    const uint32_t ns = iters ? std::min<uint32_t>(kSamplePerPivot * np, ix.capacity) : 0u;
    if (ns == 0u) {
        hipLaunchKernelGGL(sched_pivots_kernel<T>, dim3(1), dim3(np), 0, st, ix, live2, (const uint32_t*)nullptr, np, stride,
                           idx->d_sched_piv);
        DANN_HIP(hipGetLastError());
        return DANN_OK;
    }
    // scratch of the training, taken from and returned to the device's pool in stream order (no host wait):
    // sample (f32) | keys, per-block histograms | order | largest |coordinate| (+pad) | finite flags
    const size_t sort_words = sched_scratch_words(ix.dim, ns);
    const size_t words = (size_t)ns * ix.dim + sort_words + ns + 4u;
    uint32_t* d_train = nullptr;
    DANN_HIP(hipMallocAsync((void**)&d_train, words * 4u + ns, st));
    float* sample = reinterpret_cast<float*>(d_train);
    uint32_t* sort = d_train + (size_t)ns * ix.dim;
    uint32_t* order = sort + sort_words;
    uint32_t* amax = order + ns;
    uint8_t* finite = reinterpret_cast<uint8_t*>(amax + 4);
    int32_t rc = DANN_OK;
    if (hipMemsetAsync(amax, 0, 16, st) != hipSuccess) rc = DANN_EHIP;
    if (rc == DANN_OK) {
        hipLaunchKernelGGL(sched_sample_kernel<T>, dim3((ns + 3u) / 4u), dim3(256), 0, st, ix, live2, ns, sample, finite, amax);
        hipLaunchKernelGGL(sched_pivots_kernel<T>, dim3(1), dim3(np), 0, st, ix, live2, (const uint32_t*)amax, np, stride,
                           idx->d_sched_piv);
    }
    for (uint32_t it = 0; it < iters && rc == DANN_OK; ++it) {
        if ((rc = sched_sort_by_pivot<float>(idx, st, sample, ns, ix.dim, 1u, sort, order)) != DANN_OK) break;
        // (after the scan, the first block's row of the histograms holds every centre's first sorted position)
        hipLaunchKernelGGL(sched_update_kernel, dim3(np), dim3(kUpdateThreads), ix.dim * 2u, st, sample, finite, order,
                           sort + ns, ns, ix.dim, np, stride, idx->d_sched_piv);
    }
    const hipError_t le = hipGetLastError(), fe = hipFreeAsync(d_train, st);  // (freed once the kernels above have run)
    if (rc != DANN_OK) return rc;
    DANN_HIP(le);
    DANN_HIP(fe);
    return DANN_OK;
}

}  // namespace

int32_t sched_build_pivots(dann_index* idx, hipStream_t st) {
    return idx->cfg.dtype == DT_F32 ? sched_build_pivots_t<float>(idx, st) : sched_build_pivots_t<_Float16>(idx, st);
}

int32_t sched_copy_pivots(const dann_index* idx, float* out, uint32_t cap_floats, uint32_t* out_np, uint32_t* out_stride,
                          float* out_scale) {
    if (!idx->d_sched_piv) return DANN_EINVAL;
    const uint32_t dim = idx->cfg.dim, np = sched_pivot_count(dim), stride = sched_stride(dim);
    if (out_np) *out_np = np;
    if (out_stride) *out_stride = stride;
    std::vector<uint8_t> h((size_t)np * stride * 2u + (size_t)np * 4u + 4u);
    DANN_HIP(hipDeviceSynchronize());  // (the pivots are built on the stream of whichever search came first)
    DANN_HIP(hipMemcpy(h.data(), idx->d_sched_piv, h.size(), hipMemcpyDeviceToHost));
    const float scale = *reinterpret_cast<const float*>(h.data() + h.size() - 4u);  // (a multiple of 4 bytes in)
    if (out_scale) *out_scale = scale;
    if (!out) return DANN_OK;
    if (cap_floats < np * stride) return DANN_ELENGTH;
    const _Float16* piv = reinterpret_cast<const _Float16*>(h.data());
    for (size_t i = 0; i < (size_t)np * stride; ++i) out[i] = (float)piv[i] / scale;
    return DANN_OK;
}

int32_t sched_build_map(const dann_index* idx, hipStream_t st, const void* queries, uint32_t nq, uint32_t parts,
                        uint32_t* scratch, uint32_t* qmap) {
    const uint32_t dim = idx->cfg.dim;
    return idx->cfg.dtype == DT_F32
               ? sched_sort_by_pivot(idx, st, static_cast<const float*>(queries), nq, dim, parts, scratch, qmap)
               : sched_sort_by_pivot(idx, st, static_cast<const _Float16*>(queries), nq, dim, parts, scratch, qmap);
}

// scratch words a map of nq queries needs (keys + per-block histograms)
size_t sched_scratch_words(uint32_t dim, uint32_t nq) {
    return (size_t)nq + (size_t)((nq + kSortBlock - 1u) / kSortBlock) * sched_pivot_count(dim);
}

}  // namespace dann
