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
// (v_mfma_f32_32x32x16_f16: queries x pivots inner products, and the per-block key counts of the counting sort),
// sched_scatter_kernel (the block bases from those counts and the stable scatter, writing the slot map directly).
#include <hip/hip_fp16.h>

#include "dann_device.h"
#include "dann_internal.h"
#include "query_schedule.h"

namespace dann {

namespace {

typedef _Float16 sched_f16x8 __attribute__((ext_vector_type(8)));
typedef float sched_f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kKeyThreads = 512;     // 8 waves; one workgroup per CU (the pivot slab is most of the LDS)
constexpr uint32_t kKeyMaxBlocks = 256;   // key workgroups = sort blocks of a launch, at most (241 for 100 000 queries)
constexpr uint32_t kKeyMinGroups = kKeyThreads / 64u;  // 32-query groups per key workgroup, at least: one per wave
constexpr uint32_t kSortThreads = 1024;   // scatter: 16 waves
constexpr uint32_t kPreSteps = 8;         // key kernel: 16-column steps of a query held in registers, at most (dim <= 128)
constexpr uint32_t kAheadSteps = 4;       // key kernel otherwise: steps requested ahead of the ones being multiplied
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

// the lane's 8 elements of one 16-column step of its query row, as loaded.  Every load is unconditional, on an address
// clamped into the row, and the elements at or beyond `dim` are replaced by zeros afterwards: a load behind a per-lane
// branch is waited for before the next is issued, and a group's loads must all be in flight at once.  kWide (the rows
// are 16-byte aligned: the base is, and dim is a multiple of 4 (f32) / 8 (f16)): 16-byte loads, each wholly inside or
// wholly outside the row; otherwise one load per element.  load_plain: the same loads unclamped, where dim is a multiple
// of 16 and no step reaches past the row's end (kLoadPlain; frag with dim = ~0 then replaces nothing).
constexpr int kLoadElements = 0, kLoadWide = 1, kLoadPlain = 2;
typedef float sched_f32x4 __attribute__((ext_vector_type(4)));
template <typename QT, bool kWide>
struct sched_raw {
    QT v[8];
    __device__ __forceinline__ void load_plain(const QT* p) {
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) v[i] = p[i];
    }
    __device__ __forceinline__ void load(const QT* qrow, uint32_t k0, uint32_t dim) {
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) v[i] = qrow[min(k0 + i, dim - 1u)];
    }
    __device__ __forceinline__ sched_f16x8 frag(uint32_t k0, uint32_t dim, float scale) const {
        sched_f16x8 b;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) b[i] = k0 + i < dim ? (_Float16)((float)v[i] * scale) : (_Float16)0.0f;
        return b;
    }
};
template <>
struct sched_raw<float, true> {
    sched_f32x4 v[2];
    __device__ __forceinline__ void load_plain(const float* p) {
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) v[j] = *reinterpret_cast<const sched_f32x4*>(p + 4u * j);
    }
    __device__ __forceinline__ void load(const float* qrow, uint32_t k0, uint32_t dim) {
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) v[j] = *reinterpret_cast<const sched_f32x4*>(qrow + min(k0 + 4u * j, dim - 4u));
    }
    __device__ __forceinline__ sched_f16x8 frag(uint32_t k0, uint32_t dim, float scale) const {
        sched_f16x8 b;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) b[i] = k0 + (i & 4u) < dim ? (_Float16)(v[i >> 2][i & 3u] * scale) : (_Float16)0.0f;
        return b;
    }
};
template <>
struct sched_raw<_Float16, true> {
    sched_f16x8 v;
    __device__ __forceinline__ void load_plain(const _Float16* p) { v = *reinterpret_cast<const sched_f16x8*>(p); }
    __device__ __forceinline__ void load(const _Float16* qrow, uint32_t k0, uint32_t dim) {
        v = *reinterpret_cast<const sched_f16x8*>(qrow + min(k0, dim - 8u));
    }
    __device__ __forceinline__ sched_f16x8 frag(uint32_t k0, uint32_t dim, float scale) const {
        sched_f16x8 b;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) b[i] = k0 < dim ? (_Float16)((float)v[i] * scale) : (_Float16)0.0f;
        return b;
    }
};

// TC tiles of 32 pivots against the wave's 32 queries: the accumulators, one 16-column step (arow: the lane's 16 bytes
// of that step in its row of the first tile), and the lane's running minimum of norms[j] - 2 acc over them, in
// ascending pivot order (norms / j0: the lane's first pivot of the first tile)
template <int TC>
__device__ __forceinline__ void sched_zero(sched_f32x16 (&acc)[TC]) {
#pragma unroll
    for (int t = 0; t < TC; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
}
template <int TC>
__device__ __forceinline__ void sched_step(sched_f32x16 (&acc)[TC], const uint8_t* arow, uint32_t stride, const sched_f16x8& b) {
#pragma unroll
    for (int t = 0; t < TC; ++t) {
        const sched_f16x8 a = *reinterpret_cast<const sched_f16x8*>(arow + (uint64_t)t * 64u * stride);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[t], 0, 0, 0);
    }
}
template <int TC>
__device__ __forceinline__ void sched_fold(const sched_f32x16 (&acc)[TC], const float* norms, uint32_t j0, float& best,
                                           uint32_t& bi) {
#pragma unroll
    for (int t = 0; t < TC; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t o = 32u * t + (uint32_t)((r & 3) + 8 * (r >> 2));
            const float sc = norms[o] - 2.0f * acc[t][r];
            if (sc < best) {  // (NaN never wins)
                best = sc;
                bi = j0 + o;
            }
        }
        // (one tile's comparisons at a time: all of them kept as lane masks for a later pass over bi spill scalar registers)
        asm volatile("" : "+v"(best), "+v"(bi));
    }
}

// keys[q] = the pivot nearest to query q (L2 on the scaled f16 values; ties: the lower pivot).  A wave takes 32 queries x
// all 32 NT pivots: lane l supplies query / pivot row l & 31, halfs 8 (l >> 5) .. + 7 of each 16-column step, for both
// operands of v_mfma_f32_32x32x16_f16; register r of lane l then holds pivot 32 t + (r & 3) + 8 (r >> 2) + 4 (l >> 5)
// against query l & 31 (the layout gram_tiles_f16_kernel and pq_assign_mfma_kernel use).  LDS: the pivot rows (a row
// stride of 16 mod 256 bytes: the 16-byte reads of 16 consecutive rows cover all 64 banks) and their norms.
// Workgroup b takes the `per` consecutive 32-query groups of sort block b and leaves cnt[b][p] = how many of its keys
// are p (the first half of the counting sort: no pass over the keys for it); workgroup 0 also clears zero[0 .. zero_words)
// (the spill pool's counter and busy flags of the search launch that follows).
// KS > 0 (kLoadPlain, dim = 16 KS <= 128): all KS steps of a group are requested before the first conversion, and the
// tiles are multiplied in two halves, half the accumulators live beside the fragments.  KS = 0: kAhead steps are
// requested while the kAhead before them are multiplied.  Either is a kernel of its own: in one, the registers of the
// second path spill the first one's loads.
template <typename QT, int kLoad, int NT, int KS>
__global__ __launch_bounds__(kKeyThreads) void sched_key_kernel(const QT* queries, uint32_t nq, uint32_t dim,
                                                                const _Float16* piv, uint32_t stride, uint32_t per,
                                                                uint32_t* keys, uint32_t* cnt, uint32_t* zero,
                                                                uint32_t zero_words) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sched_smem[];
    __shared__ uint32_t hist[32 * NT];
    constexpr uint32_t np = 32u * NT;
    constexpr bool kWide = kLoad != kLoadElements, kPlain = kLoad == kLoadPlain;
    const uint32_t slab = np * stride * 2u, bytes = slab + np * 4u;  // both multiples of 16
    const uint4* src = reinterpret_cast<const uint4*>(piv);
    for (uint32_t i = threadIdx.x; i < bytes / 16u; i += blockDim.x) reinterpret_cast<uint4*>(sched_smem)[i] = src[i];
    for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) hist[i] = 0u;
    if (blockIdx.x == 0u)
        for (uint32_t i = threadIdx.x; i < zero_words; i += blockDim.x) zero[i] = 0u;
    const float scale = reinterpret_cast<const float*>(piv + (uint64_t)np * stride)[np];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, l31 = lane & 31u, hi = lane >> 5;
    const uint32_t ksteps = KS ? (uint32_t)KS : (dim + 15u) >> 4;
    const uint32_t groups = (nq + 31u) >> 5;
    const uint32_t gend = min(groups, (blockIdx.x + 1u) * per);
#pragma unroll 1
    for (uint32_t g = blockIdx.x * per + (threadIdx.x >> 6); g < gend; g += kKeyThreads / 64u) {
        const uint32_t q = g * 32u + l31;
        const QT* qrow = queries + (uint64_t)(q < nq ? q : nq - 1u) * dim;
        const QT* qcol = qrow + 8u * hi;
        // the pivots do not change from group to group: hidden from the compiler, which otherwise reads the whole slab
        // into registers ahead of the loop and spills what does not fit
        uint32_t aoff = l31 * stride * 2u + 16u * hi, noff = slab + 16u * hi;
        asm volatile("" : "+v"(aoff), "+v"(noff));
        const uint8_t* arow = sched_smem + aoff;
        const float* norms = reinterpret_cast<const float*>(sched_smem + noff);
        const uint32_t fdim = kPlain ? 0xFFFFFFFFu : dim;  // (kPlain: no step reaches past the row's end, nothing to replace)
        float best = __builtin_inff();
        uint32_t bi = 0;
        if constexpr (KS > 0) {
            sched_raw<QT, kWide> raw[KS];
#pragma unroll
            for (uint32_t m = 0; m < (uint32_t)KS; ++m) raw[m].load_plain(qcol + 16u * m);
            sched_f16x8 pre[KS];
#pragma unroll
            for (uint32_t m = 0; m < (uint32_t)KS; ++m) pre[m] = raw[m].frag(16u * m + 8u * hi, fdim, scale);
            constexpr int TA = NT > 4 ? 4 : NT, TB = NT - TA;
            {
                sched_f32x16 acc[TA];
                sched_zero(acc);
#pragma unroll
                for (uint32_t m = 0; m < (uint32_t)KS; ++m) sched_step(acc, arow + 32u * m, stride, pre[m]);
                sched_fold(acc, norms, 4u * hi, best, bi);
            }
            if constexpr (TB > 0) {
                sched_f32x16 acc[TB];
                sched_zero(acc);
#pragma unroll
                for (uint32_t m = 0; m < (uint32_t)KS; ++m)
                    sched_step(acc, arow + (uint64_t)TA * 64u * stride + 32u * m, stride, pre[m]);
                sched_fold(acc, norms + 32u * TA, 32u * TA + 4u * hi, best, bi);
            }
        } else {
            // (what the accumulators leave room for; single elements take an address each)
            constexpr uint32_t kAhead = NT <= 4 ? kAheadSteps : kWide ? kAheadSteps / 2u : 1u;
            sched_f32x16 acc[NT];
            sched_zero(acc);
            sched_raw<QT, kWide> raw[kAhead];
            auto request = [&](uint32_t m) {  // kAhead steps from m; past the last step: nothing that is used
#pragma unroll
                for (uint32_t i = 0; i < kAhead; ++i) {
                    if constexpr (kPlain) {
                        if (m + i < ksteps) raw[i].load_plain(qcol + 16u * (m + i));
                    } else {
                        raw[i].load(qrow, 16u * (m + i) + 8u * hi, dim);  // (a clamped address stays inside the row)
                    }
                }
            };
            request(0u);
#pragma unroll 1
            for (uint32_t m0 = 0; m0 < ksteps; m0 += kAhead) {
                sched_f16x8 cur[kAhead];
#pragma unroll
                for (uint32_t i = 0; i < kAhead; ++i) cur[i] = raw[i].frag(16u * (m0 + i) + 8u * hi, fdim, scale);
                request(m0 + kAhead);
#pragma unroll
                for (uint32_t i = 0; i < kAhead; ++i)
                    if (m0 + i < ksteps) sched_step(acc, arow + 32u * (m0 + i), stride, cur[i]);
            }
            sched_fold(acc, norms, 4u * hi, best, bi);
        }
        const float ob = __shfl_xor(best, 32);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, 32);
        if ((ob < best) | ((ob == best) & (oi < bi))) bi = oi;
        if (hi == 0u && q < nq) {
            keys[q] = bi;
            atomicAdd(&hist[bi], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < np; i += blockDim.x) cnt[(uint64_t)blockIdx.x * np + i] = hist[i];
}

// the second half of the stable counting sort.  Sort block b = the block_q consecutive queries of key workgroup b;
// cnt[b][p] = its keys equal to p.  Every workgroup first derives its own bases from the nb x np counts: the keys below
// p in all blocks plus the keys p in the blocks before its own (workgroup 0 leaves them in starts[]: every pivot's
// first sorted position).  Then query i of the block goes to sorted position base[key] + (earlier keys equal to it in
// the block), and straight on to its slot: qmap[sched_slot(position)] = i
__global__ __launch_bounds__(kSortThreads) void sched_scatter_kernel(const uint32_t* keys, uint32_t nq, uint32_t np,
                                                                     const uint32_t* cnt, uint32_t nb, uint32_t block_q,
                                                                     uint32_t parts, uint32_t* qmap, uint32_t* starts) {
    constexpr uint32_t kWaves = kSortThreads / 64u;
    __shared__ uint32_t run[256];
    __shared__ uint32_t wc[kWaves][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    {
        // thread (p, j) adds the counts of pivot p over the blocks j, j + 4, ..: eight loads in flight, on clamped
        // addresses (what lies past the table counts as zero)
        uint32_t* part = &wc[0][0];  // [all | before][4][256], then the two rows of the scan
        const uint32_t p = tid & 255u, j = tid >> 8, pc = min(p, np - 1u);
        uint32_t all = 0, before = 0;
        for (uint32_t b0 = j; b0 < nb; b0 += 32u) {
            uint32_t v[8];
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) v[i] = cnt[(uint64_t)min(b0 + 4u * i, nb - 1u) * np + pc];
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) {
                const uint32_t b = b0 + 4u * i, c = (b < nb && p < np) ? v[i] : 0u;
                all += c;
                before += b < blockIdx.x ? c : 0u;
            }
        }
        part[j * 256u + p] = all;
        part[1024u + j * 256u + p] = before;
        __syncthreads();
        uint32_t tot = 0, bef = 0;
        if (tid < 256u) {
            for (uint32_t i = 0; i < 4u; ++i) {
                tot += part[i * 256u + p];
                bef += part[1024u + i * 256u + p];
            }
            part[2048u + p] = tot;
        }
        __syncthreads();
        uint32_t cur = 0;
        for (uint32_t o = 1; o < 256u; o <<= 1) {  // inclusive scan over the pivots
            if (tid < 256u) part[2048u + (cur ^ 1u) * 256u + p] = part[2048u + cur * 256u + p] + (p >= o ? part[2048u + cur * 256u + p - o] : 0u);
            cur ^= 1u;
            __syncthreads();
        }
        if (tid < 256u) {
            run[p] = part[2048u + cur * 256u + p] - tot + bef;
            if (blockIdx.x == 0u && p < np) starts[p] = run[p];
        }
        __syncthreads();
    }
    const uint64_t below = lane ? ~0ull >> (64u - lane) : 0ull;
    for (uint32_t r0 = 0; r0 < block_q; r0 += kSortThreads) {
        for (uint32_t i = tid; i < kWaves * 256u; i += blockDim.x) (&wc[0][0])[i] = 0;
        __syncthreads();
        const uint32_t qi = blockIdx.x * block_q + r0 + tid;
        const bool valid = r0 + tid < block_q && qi < nq;
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

// the instantiations of the key kernel: for nt tiles of 32 pivots, steps requested ahead; for ks <= kPreSteps steps
// requested at once (dimensions that small have all 256 pivots)
template <typename QT, int kLoad>
const void* sched_key_fn(uint32_t nt) {
    switch (nt) {
    case 1: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoad, 1, 0>);
    case 2: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoad, 2, 0>);
    case 3: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoad, 3, 0>);
    case 4: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoad, 4, 0>);
    case 5: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoad, 5, 0>);
    case 6: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoad, 6, 0>);
    case 7: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoad, 7, 0>);
    default: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoad, 8, 0>);
    }
}
template <typename QT>
const void* sched_key_fn_pre(uint32_t ks) {
    switch (ks) {
    case 1: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoadPlain, 8, 1>);
    case 2: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoadPlain, 8, 2>);
    case 3: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoadPlain, 8, 3>);
    case 4: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoadPlain, 8, 4>);
    case 5: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoadPlain, 8, 5>);
    case 6: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoadPlain, 8, 6>);
    case 7: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoadPlain, 8, 7>);
    default: return reinterpret_cast<const void*>(sched_key_kernel<QT, kLoadPlain, 8, 8>);
    }
}

// the key kernel for these queries: 16-byte loads where every row starts on a 16-byte boundary, unclamped ones where
// no 16-column step reaches past a row's end either
template <typename QT>
const void* sched_key_fn_for(bool base_aligned, uint32_t dim, uint32_t nt) {
    if (!base_aligned || dim % (16u / sizeof(QT)) != 0u) return sched_key_fn<QT, kLoadElements>(nt);
    if (dim % 16u) return sched_key_fn<QT, kLoadWide>(nt);
    return dim <= 16u * kPreSteps && nt == 8u ? sched_key_fn_pre<QT>(dim / 16u) : sched_key_fn<QT, kLoadPlain>(nt);
}

// the key pass + the stable counting sort of nq keys, two kernels: keys | every pivot's first sorted position |
// per-block counts in `scratch`, then qmap.  The key kernel also clears zero[0 .. zero_words).
template <typename QT>
int32_t sched_sort_by_pivot(const dann_index* idx, hipStream_t st, const QT* queries, uint32_t nq, uint32_t dim,
                            uint32_t parts, uint32_t* scratch, uint32_t* qmap, uint32_t* zero, uint32_t zero_words) {
    uint32_t np = sched_pivot_count(dim), stride = sched_stride(dim);
    const uint32_t lds = np * stride * 2u + np * 4u;
    uint32_t* keys = scratch;
    uint32_t* starts = scratch + nq;
    uint32_t* cnt = starts + np;
    const uint32_t groups = (nq + 31u) / 32u;
    uint32_t per = std::max(kKeyMinGroups, (groups + kKeyMaxBlocks - 1u) / kKeyMaxBlocks);
    uint32_t nb = (groups + per - 1u) / per, block_q = per * 32u;
    const _Float16* piv = idx->d_sched_piv;
    const void* key_fn = sched_key_fn_for<QT>((reinterpret_cast<uintptr_t>(queries) & 15u) == 0u, dim, np / 32u);
    void* key_args[] = {&queries, &nq, &dim, &piv, &stride, &per, &keys, &cnt, &zero, &zero_words};
    DANN_HIP(hipLaunchKernel(key_fn, dim3(nb), dim3(kKeyThreads), key_args, lds, st));
    hipLaunchKernelGGL(sched_scatter_kernel, dim3(nb), dim3(kSortThreads), 0, st, keys, nq, np, cnt, nb, block_q, parts, qmap,
                       starts);
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
    for (const bool aligned : {false, true})
        for (const void* fn : {sched_key_fn_for<float>(aligned, ix.dim, np / 32u), sched_key_fn_for<T>(aligned, ix.dim, np / 32u)})
            DANN_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kKeyMaxLds));
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
    // sample (f32) | keys, first sorted positions, per-block counts | order | largest |coordinate| (+pad) | finite flags
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
        if ((rc = sched_sort_by_pivot<float>(idx, st, sample, ns, ix.dim, 1u, sort, order, nullptr, 0u)) != DANN_OK) break;
        // (behind the keys the sort leaves every centre's first sorted position)
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
                        uint32_t* scratch, uint32_t* qmap, uint32_t* zero, uint32_t zero_words) {
    const uint32_t dim = idx->cfg.dim;
    return idx->cfg.dtype == DT_F32
               ? sched_sort_by_pivot(idx, st, static_cast<const float*>(queries), nq, dim, parts, scratch, qmap, zero, zero_words)
               : sched_sort_by_pivot(idx, st, static_cast<const _Float16*>(queries), nq, dim, parts, scratch, qmap, zero,
                                     zero_words);
}

// scratch words a map of nq queries needs (keys + first sorted positions + per-block counts)
size_t sched_scratch_words(uint32_t dim, uint32_t nq) {
    return (size_t)nq + (size_t)(1u + kKeyMaxBlocks) * sched_pivot_count(dim);
}

}  // namespace dann
