// distance_kernels.hip -- stand-alone batched distance kernels (the parity seam and the
// gather-distance roofline kernel).
//
//   expand_beam_kernel   == ExpandBeam::expand_beam for a batch of (query, id list) pairs
//                           diskann-inmem/src/provider.rs:492-497, 620-690
//   pair_kernel          == layers::Distance::evaluate between stored rows (RobustPrune's
//                           primitive) diskann-inmem/src/layers/full.rs:224-242,
//                           diskann/src/graph/internal/prune.rs:212-215
#include "dann_device.h"
#include "dann_internal.h"
#include "wave_lists.h"

namespace dann {
namespace {

constexpr int kWave = 64;
constexpr int kChunk = 512;  // candidate ids per workgroup

template <int DT, int OP, bool NORM, int DIM>
__global__ __launch_bounds__(kWave) void expand_beam_kernel(IndexView ix, const void* queries, const uint32_t* ids,
                                                            const uint64_t* offsets, float* out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using S = Scheme<DT, OP, false>;
    constexpr int G = S::G, GROUPS = kWave / G;
    constexpr bool kInt = S::kInt;
    using QT = typename std::conditional<kInt, uint8_t, float>::type;
    using RT = typename RowType<DT>::type;
    const uint32_t lane = threadIdx.x, qi = blockIdx.x;
    const uint64_t lo = offsets[qi] + (uint64_t)blockIdx.y * kChunk;
    const uint64_t hi_all = offsets[qi + 1];
    if (lo >= hi_all) return;
    const uint64_t hi = lo + kChunk < hi_all ? lo + kChunk : hi_all;
    QT* qs = reinterpret_cast<QT*>(smem + query_stage_off(DT));
    const SqParams sqp{ix.sq_k, ix.sq_shift_norm_sq};
    const uint8_t* qsrc = reinterpret_cast<const uint8_t*>(queries) + (uint64_t)qi * ix.qbytes;
    if constexpr (kInt) {
        stage_int_query<DT>(reinterpret_cast<uint8_t*>(qs), qsrc, ix.qbytes, ix.dim, lane, kWave);
    } else {
        const RT* src = reinterpret_cast<const RT*>(qsrc);
        for (uint32_t i = lane; i < ix.dim; i += kWave) reinterpret_cast<float*>(qs)[i] = load1(src + i);
    }
    __syncthreads();
    const int g = lane / G, v = lane % G;
    if constexpr (DIM > 0 && !kInt) {
        constexpr int NTQ = DIM / (4 * G), U = 4;
        F4 xq[NTQ];
#pragma unroll
        for (int t = 0; t < NTQ; ++t) xq[t] = load4(reinterpret_cast<const float*>(qs) + t * 4 * G + 4 * v);
        for (uint64_t c0 = lo; c0 < hi; c0 += GROUPS * U) {
            const RT* rows[U];
            bool act[U];
            float o[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint64_t c = c0 + u * GROUPS + g;
                act[u] = c < hi;
                uint32_t id = act[u] ? ids[c] : 0u;
                rows[u] = reinterpret_cast<const RT*>(ix.rows + (uint64_t)id * ix.row_stride);
            }
            group_distance_pre<S::NACC, OP, DIM, U>(xq, rows, act, v, o);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint64_t c = c0 + u * GROUPS + g;
                if (act[u] && v == 0) out[c] = post_op<OP, NORM>(o[u]);
            }
        }
    } else {
        for (uint64_t c0 = lo; c0 < hi; c0 += GROUPS) {
            uint64_t c = c0 + g;
            if (c < hi) {
                const uint8_t* row = ix.rows + (uint64_t)ids[c] * ix.row_stride;
                float d = group_distance<DT, OP, false, 0>(qs, row, (int)ix.dim, v);
                if (v == 0) out[c] = finish_distance<DT, OP, NORM>(d, reinterpret_cast<const uint8_t*>(qs), row, ix.dim, sqp);
            }
        }
    }
}

// Rerank (full_precision.rs:348-397): one wave per query; distances of up to 512 candidates by the
// search-path groups, bitonic sort of (distance bits, position) keys in LDS, first k written.
template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void rerank_kernel(IndexView ix, const void* queries, const uint32_t* cand,
                                                       uint32_t stride, uint32_t k, uint32_t* out_ids,
                                                       float* out_d) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using S = Scheme<DT, OP, false>;
    constexpr int G = S::G, GROUPS = kWave / G;
    constexpr bool kInt = S::kInt;
    using QT = typename std::conditional<kInt, uint8_t, float>::type;
    using RT = typename RowType<DT>::type;
    const uint32_t lane = threadIdx.x, qi = blockIdx.x;
    uint32_t pcap = 64;
    while (pcap < stride) pcap <<= 1;
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);
    uint32_t* cid = reinterpret_cast<uint32_t*>(smem + (size_t)pcap * 8);
    float* cd = reinterpret_cast<float*>(smem + (size_t)pcap * 12);
    QT* qs = reinterpret_cast<QT*>(smem + (size_t)pcap * 16 + query_stage_off(DT));
    const SqParams sqp{ix.sq_k, ix.sq_shift_norm_sq};
    const uint8_t* qsrc = reinterpret_cast<const uint8_t*>(queries) + (uint64_t)qi * ix.qbytes;
    if constexpr (kInt) {
        stage_int_query<DT>(reinterpret_cast<uint8_t*>(qs), qsrc, ix.qbytes, ix.dim, lane, kWave);
    } else {
        const RT* src = reinterpret_cast<const RT*>(qsrc);
        for (uint32_t i = lane; i < ix.dim; i += kWave) reinterpret_cast<float*>(qs)[i] = load1(src + i);
    }
    // compact valid candidates, order preserved
    uint32_t n = 0;
    for (uint32_t i0 = 0; i0 < stride; i0 += kWave) {
        const uint32_t i = i0 + lane;
        const uint32_t id = i < stride ? cand[(uint64_t)qi * stride + i] : kEmpty;
        const bool ok = id != kEmpty && id < ix.nslots;
        const uint64_t m = ballot64(ok);
        if (ok) cid[n + mbcnt(m)] = id;
        n += (uint32_t)__popcll(m);
    }
    __syncthreads();
    const int g = lane / G, v = lane % G;
    constexpr int U = 4;
    for (uint32_t c0 = 0; c0 < n; c0 += GROUPS * U) {
        const uint8_t* rows[U];
        bool act[U];
        float o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t c = c0 + u * GROUPS + g;
            act[u] = c < n;
            rows[u] = ix.rows + (uint64_t)(act[u] ? cid[c] : 0u) * ix.row_stride;
        }
        // (wide groups are a search-kernel layout; here G = S::G lanes per row for every row type)
        group_distance_many<DT, OP, false, U, false>(qs, rows, act, (int)ix.dim, v, o);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t c = c0 + u * GROUPS + g;
            if (act[u] && v == 0)
                cd[c] = finish_distance<DT, OP, NORM>(o[u], reinterpret_cast<const uint8_t*>(qs), rows[u], ix.dim, sqp);
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < pcap; i += kWave) keys[i] = i < n ? dist_key(cd[i], i) : ~0ull;
    __syncthreads();
    block_bitonic(keys, pcap, kWave);
    for (uint32_t r = lane; r < k; r += kWave) {
        uint32_t id = kEmpty;
        float d = __builtin_inff();
        if (r < n) {
            const uint32_t pos = (uint32_t)keys[r];
            id = cid[pos];
            d = cd[pos];
        }
        out_ids[(uint64_t)qi * k + r] = id;
        out_d[(uint64_t)qi * k + r] = d;
    }
}

template <int DT, int OP, bool NORM>
int32_t launch_rerank_t(const IndexView& ix, const void* q, uint32_t nq, const uint32_t* cand, uint32_t stride,
                        uint32_t k, uint32_t* oi, float* od, hipStream_t stream) {
    uint32_t pcap = 64;
    while (pcap < stride) pcap <<= 1;
    const bool is_int = Scheme<DT, OP, false>::kInt;
    const size_t lds = (size_t)pcap * 16 + (((is_int ? int_query_slot_bytes(DT, ix.qbytes) : ix.dim * 4u) + 15u) & ~15u);
    return launch_kernel<rerank_kernel<DT, OP, NORM>>("rerank_kernel launch", dim3(nq), dim3(kWave), lds, stream, ix, q, cand,
                                                      stride, k, oi, od);
}

// pair i: rows xa[i], yb[i] given as byte pointers base + id*stride (stored rows) or
// base + i*stride (raw rows).
template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(256) void pair_kernel(const uint8_t* xbase, const uint8_t* ybase, uint64_t xstride,
                                                   uint64_t ystride, const uint32_t* a, const uint32_t* b, uint32_t n,
                                                   uint32_t dim, SqParams sqp, float* out) {
    using S = Scheme<DT, OP, true>;
    constexpr int G = S::G;
    using RT = typename RowType<DT>::type;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t p = tid / G;
    const int v = tid % G;
    if (p >= n) return;  // whole groups exit together (G divides 64)
    const uint8_t* x = xbase + (uint64_t)(a ? a[p] : p) * xstride;
    const uint8_t* y = ybase + (uint64_t)(b ? b[p] : p) * ystride;
    float d;
    if constexpr (dt_is_packed(DT) || dt_is_mm(DT)) {
        d = group_distance_rows<DT, OP>(x, y, (int)dim, v);
    } else if constexpr (S::kInt) {
        d = group_distance_int<OP, DT == DT_I8>(x, y, (int)dim, v);
    } else {
        d = group_distance_raw<S::NACC, OP, 0>(reinterpret_cast<const RT*>(x), reinterpret_cast<const RT*>(y), (int)dim,
                                               v);
    }
    if (v == 0) out[p] = finish_distance<DT, OP, NORM>(d, x, y, dim, sqp);
}

template <int DT, int OP, bool NORM>
int32_t launch_pairs_t(const uint8_t* xb, const uint8_t* yb, uint64_t xs, uint64_t ys, const uint32_t* a,
                       const uint32_t* b, uint32_t n, uint32_t dim, SqParams sqp, float* out, hipStream_t stream) {
    constexpr int G = Scheme<DT, OP, true>::G;
    const uint64_t threads = (uint64_t)n * G;
    const uint32_t blocks = (uint32_t)((threads + 255) / 256);
    return launch_kernel<pair_kernel<DT, OP, NORM>>("pair_kernel launch", dim3(blocks), dim3(256), 0, stream, xb, yb, xs, ys, a,
                                                    b, n, dim, sqp, out);
}

int32_t launch_pairs_rows(int32_t dtype, int32_t metric, const uint8_t* xb, const uint8_t* yb, uint64_t xs, uint64_t ys,
                         const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t dim, SqParams sqp, float* out,
                         hipStream_t stream) {
    if (n == 0) return DANN_OK;
    const int32_t rc = dispatch_row_op<kRowsStored>(dtype, metric, [&](auto r) {
        using R = decltype(r);
        return launch_pairs_t<R::dt, R::op, R::norm>(xb, yb, xs, ys, a, b, n, dim, sqp, out, stream);
    });
    if (rc != kNoRow) return rc;
    set_error("bad dtype %d", dtype);
    return DANN_EINVAL;
}

template <int DT, int OP, bool NORM, int DIM>
int32_t launch_eb_t(const IndexView& ix, const void* q, uint32_t nq, uint32_t chunks, const uint32_t* ids,
                    const uint64_t* offsets, float* out, hipStream_t stream) {
    const bool is_int = Scheme<DT, OP, false>::kInt;
    size_t lds = ((is_int ? int_query_slot_bytes(DT, ix.qbytes) : ix.dim * 4u) + 15u) & ~15u;
    return launch_kernel<expand_beam_kernel<DT, OP, NORM, DIM>>("expand_beam_kernel launch", dim3(nq, chunks), dim3(kWave), lds,
                                                                stream, ix, q, ids, offsets, out);
}

}  // namespace

// `d_offsets[nq+1]` on device; `max_len` = longest list (host-known) sizes the grid.
int32_t launch_expand_beam(const IndexView& ix, const void* d_queries, uint32_t nq, const uint32_t* d_ids,
                           const uint64_t* d_offsets, uint64_t max_len, float* d_out, hipStream_t stream) {
    if (nq == 0 || max_len == 0) return DANN_OK;
    const uint32_t chunks = (uint32_t)((max_len + kChunk - 1) / kChunk);
    if (chunks > 65535u) {
        set_error("id list too long for one launch (%llu ids)", (unsigned long long)max_len);
        return DANN_EUNSUPPORTED;
    }
    const int32_t rc = dispatch_row_op<kRowsQuery>(ix.dtype, ix.metric, [&](auto r) {
        using R = decltype(r);
        if constexpr (R::dt == DT_F32 && R::op == OP_L2 && !R::norm) {  // the one form with the row length fixed at 128
            if (ix.dim == 128)
                return launch_eb_t<R::dt, R::op, R::norm, 128>(ix, d_queries, nq, chunks, d_ids, d_offsets, d_out, stream);
        }
        return launch_eb_t<R::dt, R::op, R::norm, 0>(ix, d_queries, nq, chunks, d_ids, d_offsets, d_out, stream);
    });
    if (rc != kNoRow) return rc;
    set_error("bad dtype %d", ix.dtype);
    return DANN_EINVAL;
}

int32_t launch_rerank(const IndexView& ix, const void* d_queries, uint32_t nq, const uint32_t* d_cand, uint32_t stride,
                      uint32_t k, uint32_t* d_out_ids, float* d_out_d, hipStream_t stream) {
    if (nq == 0) return DANN_OK;
    if (stride == 0 || stride > 4096) {
        set_error("rerank supports 1..4096 candidates per query (got %u)", stride);
        return DANN_EUNSUPPORTED;
    }
    const int32_t rc = dispatch_row_op<kRowsQuery>(ix.dtype, ix.metric, [&](auto r) {
        using R = decltype(r);
        return launch_rerank_t<R::dt, R::op, R::norm>(ix, d_queries, nq, d_cand, stride, k, d_out_ids, d_out_d, stream);
    });
    return rc == kNoRow ? DANN_EINVAL : rc;
}

int32_t launch_distance_pairs(const IndexView& ix, const uint32_t* d_a, const uint32_t* d_b, uint32_t n, float* d_out,
                              hipStream_t stream) {
    return launch_pairs_rows(ix.dtype, ix.metric, ix.rows, ix.rows, ix.row_stride, ix.row_stride, d_a, d_b, n, ix.dim,
                            SqParams{ix.sq_k, ix.sq_shift_norm_sq}, d_out, stream);
}

int32_t launch_distance_raw(const IndexView& ix, const void* d_x, const void* d_y, uint64_t stride, uint32_t n,
                            float* d_out, hipStream_t stream) {
    return launch_pairs_rows(ix.dtype, ix.metric, reinterpret_cast<const uint8_t*>(d_x),
                            reinterpret_cast<const uint8_t*>(d_y), stride, stride, nullptr, nullptr, n, ix.dim,
                            SqParams{ix.sq_k, ix.sq_shift_norm_sq}, d_out, stream);
}

}  // namespace dann


// ---- diagnostics: what a plain streaming read achieves on this device (the "achievable" line next to the 8 TB/s peak)
namespace dann {
namespace {
__global__ __launch_bounds__(256) void stream_read_kernel(const uint4* __restrict__ p, uint64_t n16, uint32_t* sink) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t acc = 0;
    for (; i + 3 * stride < n16; i += 4 * stride) {  // four independent 16-byte loads in flight per lane
        const uint4 a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
        acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
    }
    for (; i < n16; i += stride) {
        const uint4 a = p[i];
        acc ^= a.x ^ a.y ^ a.z ^ a.w;
    }
    if (acc == 0x9E3779B9u) atomicAdd(sink, 1u);  // keeps the loads alive; practically never true
}
}  // namespace
}  // namespace dann

extern "C" int32_t dann_debug_stream_read_gbps(int32_t device, uint64_t bytes, uint32_t reps, double* gbps) try {
    using namespace dann;
    if (!gbps || bytes < (1u << 20) || reps == 0) return DANN_EINVAL;
    if (device >= 0) DANN_HIP(hipSetDevice(device));
    void* buf = nullptr;
    uint32_t* sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DANN_HIP(hipMalloc(&buf, bytes));
    DANN_HIP(hipMalloc((void**)&sink, 4));
    DANN_HIP(hipMemset(buf, 1, bytes));
    DANN_HIP(hipMemset(sink, 0, 4));
    DANN_HIP(hipEventCreate(&e0));
    DANN_HIP(hipEventCreate(&e1));
    const uint64_t n16 = bytes / 16;
    const dim3 grid(256 * 16), block(256);
    hipLaunchKernelGGL(stream_read_kernel, grid, block, 0, 0, (const uint4*)buf, n16, sink);
    DANN_HIP(hipEventRecord(e0, 0));
    for (uint32_t r = 0; r < reps; ++r) hipLaunchKernelGGL(stream_read_kernel, grid, block, 0, 0, (const uint4*)buf, n16, sink);
    DANN_HIP(hipEventRecord(e1, 0));
    DANN_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    DANN_HIP(hipEventElapsedTime(&ms, e0, e1));
    *gbps = (double)n16 * 16.0 * reps / (ms * 1e-3) / 1e9;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(buf);
    (void)hipFree(sink);
    return DANN_OK;
} DANN_CATCH_ALL
