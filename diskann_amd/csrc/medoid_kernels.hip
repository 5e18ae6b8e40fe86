// medoid_kernels.hip -- ComputeMedoid on the GPU (diskann-utils/src/sampling/medoid.rs:15-156): the f32 mean of the rows
// from sequential f64 column sums, then the first row nearest to it under SquaredL2.
//
//   medoid_summarize_kernel  one workgroup per range of kMedoidRangeRows rows: a SeqSummary (sum, sum of magnitudes,
//                            lowest set bit) of every column over the range, rows read coalesced along the columns;
//   medoid_walk_kernel       one wavefront per column walks the ranges in row order with the running sum as the carry.
//                            seq_exact (seq_sum.h) says where the sequential sum cannot round: a group of 64 ranges is
//                            tested first, then each range; a range that fails is walked row by row from its carry
//                            (its rows requested up front, added in order).  The result has the bits of the sequential walk;
//   medoid_argmin_kernel     one streaming pass: the mean in LDS, 8 lanes per row with the query distance's f32 x f32 /
//                            f32 x f16 association (group_distance_raw, NACC = 4), a running (d, row) per lane group,
//                            "smaller d, or equal d and smaller row" across lanes, waves and workgroups;
//   medoid_final_kernel      the one cross-workgroup reduction on the (d, row) pairs.  No atomics on floats.
#include <algorithm>

#include "dann_device.h"
#include "dann_internal.h"
#include "seq_sum.h"

namespace dann {

// Row elements as the distance templates see them: found by argument-dependent lookup, loaded with the element's own
// alignment (a caller's stride need not keep rows 16-byte aligned), widened exactly.  u8 / i8 rows go through the
// f32 x f32 kernel as the reference's medoid does (medoid.rs:105-116), not through the integer kernels.
struct MedF32 { float v; };
struct MedF16 { __half v; };
struct MedU8 { uint8_t v; };
struct MedI8 { int8_t v; };
__device__ __forceinline__ float to_f32(MedF32 x) { return x.v; }
__device__ __forceinline__ float to_f32(MedF16 x) { return __half2float(x.v); }
__device__ __forceinline__ float to_f32(MedU8 x) { return (float)x.v; }
__device__ __forceinline__ float to_f32(MedI8 x) { return (float)x.v; }
__device__ __forceinline__ F4 load4(const MedF32* p) {
    struct __attribute__((packed, aligned(4))) P { float x, y, z, w; };
    const P t = *reinterpret_cast<const P*>(p);
    return {t.x, t.y, t.z, t.w};
}
__device__ __forceinline__ F4 load4(const MedF16* p) {
    struct __attribute__((packed, aligned(2))) P { uint32_t a, b; };
    const P t = *reinterpret_cast<const P*>(p);
    const float2 fa = __half22float2(__builtin_bit_cast(__half2, t.a)), fb = __half22float2(__builtin_bit_cast(__half2, t.b));
    return {fa.x, fa.y, fb.x, fb.y};
}
__device__ __forceinline__ F4 load4(const MedU8* p) {
    struct __attribute__((packed, aligned(1))) P { uint32_t a; };
    const uint32_t t = reinterpret_cast<const P*>(p)->a;
    return {(float)(t & 255u), (float)((t >> 8) & 255u), (float)((t >> 16) & 255u), (float)(t >> 24)};
}
__device__ __forceinline__ F4 load4(const MedI8* p) {
    struct __attribute__((packed, aligned(1))) P { uint32_t a; };
    const uint32_t t = reinterpret_cast<const P*>(p)->a;
    return {(float)(int8_t)(t & 255u), (float)(int8_t)((t >> 8) & 255u), (float)(int8_t)((t >> 16) & 255u),
            (float)(int8_t)(t >> 24)};
}

namespace {

constexpr uint32_t kArgminThreads = 256, kArgminMaxBlocks = 2048;
constexpr uint64_t kNoRowYet = ~0ull;

template <typename T>
__device__ __forceinline__ double med_elem(const uint8_t* rows, uint64_t stride, uint64_t r, uint32_t c) {
    return (double)to_f32(reinterpret_cast<const T*>(rows + r * stride)[c]);
}

// summaries: column-major, [c * nranges + k]
template <typename T>
__global__ __launch_bounds__(256) void medoid_summarize_kernel(const uint8_t* __restrict__ rows, uint64_t nrows, uint32_t dim,
                                                               uint64_t stride, uint64_t nranges, double* __restrict__ S,
                                                               double* __restrict__ A, int* __restrict__ G) {
    __shared__ double lS[3][64], lA[3][64];
    __shared__ int lG[3][64];
    const uint32_t x = threadIdx.x & 63u, y = threadIdx.x >> 6;
    const uint64_t k = blockIdx.x;
    const uint64_t r0 = k * kMedoidRangeRows + (uint64_t)y * 64u;
    const uint64_t r1 = r0 + 64u < nrows ? r0 + 64u : nrows;
    for (uint32_t c0 = 0; c0 < dim; c0 += 64u) {
        const uint32_t c = c0 + x;
        SeqSummary s{0.0, 0.0, kSeqNone};
        if (c < dim) {
#pragma unroll 8
            for (uint64_t r = r0; r < r1; ++r) seq_take(s, med_elem<T>(rows, stride, r, c));
        }
        if (y) {
            lS[y - 1][x] = s.S;
            lA[y - 1][x] = s.A;
            lG[y - 1][x] = s.g;
        }
        __syncthreads();
        if (y == 0 && c < dim) {
#pragma unroll
            for (int q = 0; q < 3; ++q) s = seq_join(s, SeqSummary{lS[q][x], lA[q][x], lG[q][x]});
            const uint64_t o = (uint64_t)c * nranges + k;
            S[o] = s.S;
            A[o] = s.A;
            G[o] = s.g;
        }
        __syncthreads();
    }
}

// lane `l`'s value, l wave-uniform: v_readlane, no trip through the LDS crossbar
__device__ __forceinline__ double lane_f64(double v, uint32_t l) {
    const uint64_t b = (uint64_t)__builtin_bit_cast(long long, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)l);
    return __builtin_bit_cast(double, (long long)(((uint64_t)hi << 32) | lo));
}

// counters: [0] ranges summed in parallel, [1] ranges walked row by row
template <typename T>
__global__ __launch_bounds__(64) void medoid_walk_kernel(const uint8_t* __restrict__ rows, uint64_t nrows, uint32_t dim,
                                                         uint64_t stride, uint64_t nranges, const double* __restrict__ S,
                                                         const double* __restrict__ A, const int* __restrict__ G,
                                                         float* __restrict__ mean, unsigned long long* counters) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const double* cS = S + (uint64_t)c * nranges;
    const double* cA = A + (uint64_t)c * nranges;
    const int* cG = G + (uint64_t)c * nranges;
    double acc = 0.0;
    unsigned long long par = 0, ser = 0;
    for (uint64_t k0 = 0; k0 < nranges; k0 += kMedoidGroupRanges) {
        const uint64_t k = k0 + lane;
        const uint32_t in_group = (uint32_t)(nranges - k0 < kMedoidGroupRanges ? nranges - k0 : kMedoidGroupRanges);
        const SeqSummary mine = k < nranges ? SeqSummary{cS[k], cA[k], cG[k]} : SeqSummary{0.0, 0.0, kSeqNone};
        SeqSummary grp = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            SeqSummary o;
            o.S = __shfl_xor(grp.S, d);
            o.A = __shfl_xor(grp.A, d);
            o.g = __shfl_xor(grp.g, d);
            grp = seq_join(grp, o);
        }
        // (every lane holds the same group summary only where the additions are exact; lane 0's is the one tested)
        grp.S = lane_f64(grp.S, 0u);
        grp.A = lane_f64(grp.A, 0u);
        grp.g = __builtin_amdgcn_readlane(grp.g, 0);
        if (seq_exact(acc, grp)) {
            acc += grp.S;
            par += in_group;
            continue;
        }
        for (uint32_t j = 0; j < in_group; ++j) {
            const SeqSummary rs{lane_f64(mine.S, j), lane_f64(mine.A, j), __builtin_amdgcn_readlane(mine.g, (int)j)};
            if (seq_exact(acc, rs)) {
                acc += rs.S;
                ++par;
                continue;
            }
            ++ser;
            const uint64_t r0 = (k0 + j) * kMedoidRangeRows;
            const uint64_t r1 = r0 + kMedoidRangeRows < nrows ? r0 + kMedoidRangeRows : nrows;
            // (the range's rows are all requested before the first addition: one round trip, not one per 64 rows)
            constexpr uint32_t kBatches = kMedoidRangeRows / 64u;
            double v[kBatches];
#pragma unroll
            for (uint32_t q = 0; q < kBatches; ++q) {
                const uint64_t r = r0 + q * 64u + lane;
                v[q] = r < r1 ? med_elem<T>(rows, stride, r, c) : 0.0;
            }
#pragma unroll
            for (uint32_t q = 0; q < kBatches; ++q) {
                const uint64_t b = r0 + q * 64u;
                const uint32_t m = b >= r1 ? 0u : (uint32_t)(r1 - b < 64u ? r1 - b : 64u);
                // (the carry is pinned to vector registers -- no trip through the scalar file per row -- and a whole batch is
                // unrolled: constant lane selects, no taken branch per addition)
                if (m == 64u) {
#pragma unroll
                    for (uint32_t i = 0; i < 64u; ++i) {
                        acc += lane_f64(v[q], i);
                        asm volatile("" : "+v"(acc));
                    }
                } else {
                    for (uint32_t i = 0; i < m; ++i) {
                        acc += lane_f64(v[q], i);
                        asm volatile("" : "+v"(acc));
                    }
                }
            }
        }
    }
    if (lane == 0) {
        mean[c] = (float)(acc / (double)nrows);
        if (par) atomicAdd(&counters[0], par);
        if (ser) atomicAdd(&counters[1], ser);
    }
}

__device__ __forceinline__ bool med_better(float d, uint64_t row, float bd, uint64_t brow) {
    return d < bd || (d == bd && row < brow);
}

template <typename T>
__global__ __launch_bounds__(kArgminThreads) void medoid_argmin_kernel(const uint8_t* __restrict__ rows, uint64_t nrows,
                                                                       uint32_t dim, uint64_t stride,
                                                                       const float* __restrict__ mean, float* part_d,
                                                                       uint64_t* part_row, unsigned long long* counters) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* q = reinterpret_cast<float*>(smem);
    __shared__ float wd[kArgminThreads / 64];
    __shared__ uint64_t wr[kArgminThreads / 64];
    for (uint32_t i = threadIdx.x; i < dim; i += kArgminThreads) q[i] = mean[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, g = lane >> 3;
    const int v = (int)(lane & 7u);
    const uint64_t groups = (uint64_t)gridDim.x * (kArgminThreads / 8u);
    float bd = 3.402823466e+38f;  // f32::MAX
    uint64_t brow = kNoRowYet;
    uint32_t nan = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * (kArgminThreads / 8u) + wave * 8u + g; r < nrows; r += groups) {
        const float d = group_distance_raw<4, OP_L2, 0>(q, reinterpret_cast<const T*>(rows + r * stride), (int)dim, v);
        if (v == 0) {
            if (d != d) ++nan;
            if (d < bd) {  // rows ascend within a lane group: the first minimum stays
                bd = d;
                brow = r;
            }
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float od = __shfl_xor(bd, o);
        const uint64_t orow = (uint64_t)__shfl_xor((unsigned long long)brow, o);
        if (med_better(od, orow, bd, brow)) {
            bd = od;
            brow = orow;
        }
        nan += (uint32_t)__shfl_xor((int)nan, o);
    }
    if (lane == 0) {
        wd[wave] = bd;
        wr[wave] = brow;
        if (nan) atomicAdd(&counters[3], (unsigned long long)nan);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kArgminThreads / 64u; ++w)
            if (med_better(wd[w], wr[w], bd, brow)) {
                bd = wd[w];
                brow = wr[w];
            }
        part_d[blockIdx.x] = bd;
        part_row[blockIdx.x] = brow;
    }
}

__global__ __launch_bounds__(64) void medoid_final_kernel(const float* part_d, const uint64_t* part_row, uint32_t nparts,
                                                          long long* out_row) {
    const uint32_t lane = threadIdx.x;
    float bd = 3.402823466e+38f;
    uint64_t brow = kNoRowYet;
    for (uint32_t i = lane; i < nparts; i += 64u)
        if (med_better(part_d[i], part_row[i], bd, brow)) {
            bd = part_d[i];
            brow = part_row[i];
        }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float od = __shfl_xor(bd, o);
        const uint64_t orow = (uint64_t)__shfl_xor((unsigned long long)brow, o);
        if (med_better(od, orow, bd, brow)) {
            bd = od;
            brow = orow;
        }
    }
    if (lane == 0) *out_row = brow == kNoRowYet ? -1ll : (long long)brow;
}

// one call's device scratch, carved from one allocation: the summaries, the argmin's partial pairs, the row and the
// counters, and the mean when the caller does not want it
struct MedoidScratch {
    uint64_t nranges = 0;
    uint32_t nparts = 0;
    double *S = nullptr, *A = nullptr;
    uint64_t* part_row = nullptr;
    long long* row = nullptr;
    unsigned long long* counters = nullptr;  // 4
    int* G = nullptr;
    float *part_d = nullptr, *mean = nullptr;
    DevBuf buf;
    int32_t alloc(uint64_t nrows, uint32_t dim) {
        nranges = (nrows + kMedoidRangeRows - 1u) / kMedoidRangeRows;
        nparts = (uint32_t)std::min<uint64_t>(kArgminMaxBlocks, (nrows + kArgminThreads / 8u - 1u) / (kArgminThreads / 8u));
        const size_t cells = (size_t)nranges * dim;
        const size_t bytes = cells * 20u + (size_t)nparts * 12u + 40u + (size_t)dim * 4u + 64u;
        DANN_HIP(buf.alloc(bytes));
        uint8_t* p = buf.as<uint8_t>();
        S = reinterpret_cast<double*>(p);
        A = S + cells;
        part_row = reinterpret_cast<uint64_t*>(A + cells);
        row = reinterpret_cast<long long*>(part_row + nparts);
        counters = reinterpret_cast<unsigned long long*>(row + 1);
        G = reinterpret_cast<int*>(counters + 4);
        part_d = reinterpret_cast<float*>(G + cells);
        mean = part_d + nparts;
        return DANN_OK;
    }
};

template <typename T>
int32_t medoid_launch(const uint8_t* rows, uint64_t nrows, uint32_t dim, uint64_t stride, const MedoidScratch& m, float* d_mean,
                      double* times_ms) {
    struct Events {  // (destroyed on every way out)
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } events;
    hipEvent_t* ev = events.e;
    if (times_ms)
        for (int i = 0; i < 3; ++i) DANN_HIP(hipEventCreate(&ev[i]));
    if (times_ms) DANN_HIP(hipEventRecord(ev[0], nullptr));
    hipLaunchKernelGGL(medoid_summarize_kernel<T>, dim3((uint32_t)m.nranges), dim3(256), 0, nullptr, rows, nrows, dim, stride,
                       m.nranges, m.S, m.A, m.G);
    DANN_HIP(hipGetLastError());
    hipLaunchKernelGGL(medoid_walk_kernel<T>, dim3(dim), dim3(64), 0, nullptr, rows, nrows, dim, stride, m.nranges,
                       (const double*)m.S, (const double*)m.A, (const int*)m.G, d_mean, m.counters);
    DANN_HIP(hipGetLastError());
    if (times_ms) DANN_HIP(hipEventRecord(ev[1], nullptr));
    if (int32_t rc = launch_kernel<medoid_argmin_kernel<T>>("medoid_argmin_kernel launch", dim3(m.nparts), dim3(kArgminThreads),
                                                            (size_t)dim * 4, nullptr, rows, nrows, dim, stride,
                                                            (const float*)d_mean, m.part_d, m.part_row, m.counters))
        return rc;
    hipLaunchKernelGGL(medoid_final_kernel, dim3(1), dim3(64), 0, nullptr, (const float*)m.part_d,
                       (const uint64_t*)m.part_row, m.nparts, m.row);
    DANN_HIP(hipGetLastError());
    if (times_ms) {
        DANN_HIP(hipEventRecord(ev[2], nullptr));
        DANN_HIP(hipEventSynchronize(ev[2]));
        float a = 0.f, b = 0.f;
        DANN_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
        DANN_HIP(hipEventElapsedTime(&b, ev[1], ev[2]));
        times_ms[0] = a;
        times_ms[1] = b;
    }
    return DANN_OK;
}

uint32_t med_elem_size(int32_t dtype) { return dtype == DT_F32 ? 4u : dtype == DT_F16 ? 2u : 1u; }

int32_t medoid_check(const char* who, int32_t dtype, const void* rows, uint64_t nrows, uint32_t dim,
                     uint64_t* row_stride_bytes, int64_t* out_row) {
    if (dtype != DT_F32 && dtype != DT_F16 && dtype != DT_U8 && dtype != DT_I8) {
        set_error("%s: dtype %d has no medoid (DANN_F32, DANN_F16, DANN_U8, DANN_I8)", who, dtype);
        return DANN_EUNSUPPORTED;
    }
    if (dim == 0 || !out_row || (nrows && !rows)) {
        set_error("%s: dim must be positive, rows and out_row non-null", who);
        return DANN_EINVAL;
    }
    if (dim > 16000u) {
        set_error("%s: dim %u is more than the 16000 the mean's LDS copy holds", who, dim);
        return DANN_EUNSUPPORTED;
    }
    const uint64_t es = med_elem_size(dtype), packed = (uint64_t)dim * es;
    if (*row_stride_bytes == 0) *row_stride_bytes = packed;
    if (*row_stride_bytes < packed || *row_stride_bytes % es != 0 || (uint64_t)(uintptr_t)rows % es != 0) {
        set_error("%s: row stride %llu is below the row's %llu bytes, or rows are not aligned to their elements", who,
                  (unsigned long long)*row_stride_bytes, (unsigned long long)packed);
        return DANN_EINVAL;
    }
    return DANN_OK;
}

}  // namespace

// rows, out_mean (may be null): device memory; *out_row, out_counters (4, may be null), times_ms (2, may be null): host
int32_t medoid_device(int32_t dtype, const void* d_rows, uint64_t nrows, uint32_t dim, uint64_t stride, int64_t* out_row,
                      float* d_out_mean, uint64_t* out_counters, double* times_ms) {
    if (nrows == 0) {  // the reference returns a zero vector and no row
        if (d_out_mean) {
            DANN_HIP(hipMemsetAsync(d_out_mean, 0, (size_t)dim * 4, nullptr));
            DANN_HIP(hipStreamSynchronize(nullptr));
        }
        *out_row = -1;
        if (out_counters) out_counters[0] = out_counters[1] = out_counters[2] = out_counters[3] = 0;
        if (times_ms) times_ms[0] = times_ms[1] = 0.0;
        return DANN_OK;
    }
    if ((nrows + kMedoidRangeRows - 1u) / kMedoidRangeRows > 0x7FFFFFFFull) {
        set_error("dann_medoid: %llu rows are more than one call takes", (unsigned long long)nrows);
        return DANN_EUNSUPPORTED;
    }
    MedoidScratch m;
    if (int32_t rc = m.alloc(nrows, dim)) return rc;
    DANN_HIP(hipMemsetAsync(m.row, 0, 40, nullptr));  // the row and the four counters
    float* mean = d_out_mean ? d_out_mean : m.mean;
    const uint8_t* rows = static_cast<const uint8_t*>(d_rows);
    int32_t rc;
    switch (dtype) {
        case DT_F32: rc = medoid_launch<MedF32>(rows, nrows, dim, stride, m, mean, times_ms); break;
        case DT_F16: rc = medoid_launch<MedF16>(rows, nrows, dim, stride, m, mean, times_ms); break;
        case DT_U8: rc = medoid_launch<MedU8>(rows, nrows, dim, stride, m, mean, times_ms); break;
        default: rc = medoid_launch<MedI8>(rows, nrows, dim, stride, m, mean, times_ms); break;
    }
    if (rc != DANN_OK) return rc;
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    DANN_HIP(hipMemcpy(h, m.row, 40, hipMemcpyDeviceToHost));  // (waits for the null stream: the scratch is freed on return)
    *out_row = (int64_t)(long long)h[0];
    if (out_counters) {
        out_counters[0] = h[1];
        out_counters[1] = h[2];
        out_counters[2] = nrows;
        out_counters[3] = h[4];
    }
    return DANN_OK;
}

}  // namespace dann

using namespace dann;

extern "C" int32_t dann_medoid_device(int32_t device, int32_t dtype, const void* rows, uint64_t nrows, uint32_t dim,
                                      uint64_t row_stride_bytes, int64_t* out_row, float* out_mean,
                                      uint64_t* out_counters) try {
    if (int32_t rc = medoid_check("dann_medoid_device", dtype, rows, nrows, dim, &row_stride_bytes, out_row)) return rc;
    int cur = 0;
    if (device < 0) DANN_HIP(hipGetDevice(&cur));
    DeviceGuard guard(device < 0 ? cur : device);
    if (!guard.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    return medoid_device(dtype, rows, nrows, dim, row_stride_bytes, out_row, out_mean, out_counters, nullptr);
} DANN_CATCH_ALL

extern "C" int32_t dann_medoid(int32_t device, int32_t dtype, const void* rows, uint64_t nrows, uint32_t dim,
                               uint64_t row_stride_bytes, int64_t* out_row, float* out_mean, uint64_t* out_counters) try {
    if (int32_t rc = medoid_check("dann_medoid", dtype, rows, nrows, dim, &row_stride_bytes, out_row)) return rc;
    int cur = 0;
    if (device < 0) DANN_HIP(hipGetDevice(&cur));
    DeviceGuard guard(device < 0 ? cur : device);
    if (!guard.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    // (the last row need not have a whole stride behind it)
    const size_t bytes = nrows ? (size_t)(nrows - 1u) * row_stride_bytes + (size_t)dim * med_elem_size(dtype) : 0u;
    DevBuf d_rows, d_mean;
    DANN_HIP(d_rows.alloc(bytes));
    DANN_HIP(d_mean.alloc((size_t)dim * 4));
    if (bytes) DANN_HIP(hipMemcpy(d_rows.p, rows, bytes, hipMemcpyHostToDevice));
    if (int32_t rc = medoid_device(dtype, d_rows.p, nrows, dim, row_stride_bytes, out_row, d_mean.as<float>(), out_counters,
                                   nullptr))
        return rc;
    if (out_mean) DANN_HIP(hipMemcpy(out_mean, d_mean.p, (size_t)dim * 4, hipMemcpyDeviceToHost));
    return DANN_OK;
} DANN_CATCH_ALL

// the two passes' HIP-event times (ms): [0] column sums (summaries + walk), [1] argmin (scan + reduction)
extern "C" int32_t dann_debug_medoid_times(int32_t device, int32_t dtype, const void* d_rows, uint64_t nrows, uint32_t dim,
                                           uint64_t row_stride_bytes, int64_t* out_row, uint64_t* out_counters,
                                           double* out_ms) try {
    if (!out_ms) return DANN_EINVAL;
    if (int32_t rc = medoid_check("dann_debug_medoid_times", dtype, d_rows, nrows, dim, &row_stride_bytes, out_row)) return rc;
    int cur = 0;
    if (device < 0) DANN_HIP(hipGetDevice(&cur));
    DeviceGuard guard(device < 0 ? cur : device);
    if (!guard.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    return medoid_device(dtype, d_rows, nrows, dim, row_stride_bytes, out_row, nullptr, out_counters, out_ms);
} DANN_CATCH_ALL
