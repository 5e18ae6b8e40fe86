// maxsim_stage.h -- the LDS stage the matrix-core multi-vector kernels share (maxsim_kernels.hip: one workgroup per
// (query, candidate) pair; maxsim_flat_kernels.hip: the exhaustive scan): a 32-row x 128-k slab of f32 or f16 rows,
// widened to f32, transposed and swizzled for conflict-free MFMA operand reads.
#pragma once
#include "dann_device.h"
#include "dann_internal.h"

namespace dann {
namespace {

typedef float ms_f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kMsSlabK = 128;     // k values of one LDS slab
constexpr uint32_t kMsSlabFloats = kMsSlabK * 32u;

// One 32-row x 128-k slab, transposed and swizzled: element (k, r) sits at word 32 k + (r ^ swz(k)), swz(k) =
// 4 ((k / E) & 7), E = the elements of one 16-byte request.  The MFMA operand read of k-step m -- lane l takes
// (k = 2 m + (l >> 5), r = l & 31) -- touches 32 distinct banks per lane half for every swz; the stage's writes do too:
// a lane half holds 4 consecutive rows x 8 consecutive requests, and r ^ 4 (request & 7) spreads them over all 32 banks.
// So the stage keeps full-line 16-byte requests (8 lanes per 128 bytes of a row) AND conflict-free transposed writes.
template <typename RT>
__device__ __forceinline__ uint32_t ms_swz(uint32_t k) {
    constexpr uint32_t E = 16u / sizeof(RT);
    return ((k / E) & 7u) << 2;
}

__device__ __forceinline__ void ms_widen(const uint4& v, float (&f)[4], float) {
    f[0] = __builtin_bit_cast(float, v.x), f[1] = __builtin_bit_cast(float, v.y);
    f[2] = __builtin_bit_cast(float, v.z), f[3] = __builtin_bit_cast(float, v.w);
}
__device__ __forceinline__ void ms_widen(const uint4& v, float (&f)[8], __half) {  // v_cvt_f32_f16: exact
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float2 p = __half22float2(__builtin_bit_cast(__half2, w[i]));
        f[2 * i] = p.x, f[2 * i + 1] = p.y;
    }
}

// Fill `slab` with rows[0 .. nrows) x bytes [byte0, byte0 + 128 sizeof(RT)) of a row; rows >= nrows and bytes >=
// `stride` read as zero.  NT threads, thread `t` of them.  Every request is issued unconditionally at a clamped address
// (a load under a per-lane condition gets a wait of its own) and zeroed afterwards.
template <typename RT, uint32_t NT>
__device__ __forceinline__ void ms_stage(float* slab, const uint8_t* rows, uint32_t stride, uint32_t nrows, uint32_t byte0,
                                         uint32_t t) {
    constexpr uint32_t E = 16u / sizeof(RT), NREQ = 32u * (kMsSlabK / E), PASSES = NREQ / NT;
    static_assert(NREQ % NT == 0, "whole passes");
    uint4 v[PASSES];
    bool ok[PASSES];
#pragma unroll
    for (uint32_t p = 0; p < PASSES; ++p) {
        const uint32_t i = p * NT + t, row = (i >> 3) & 31u, req = (i & 7u) + ((i >> 8) << 3), byte = byte0 + (req << 4);
        ok[p] = row < nrows && byte < stride;
        v[p] = *reinterpret_cast<const uint4*>(rows + (ok[p] ? (uint64_t)row * stride + byte : 0u));
    }
#pragma unroll
    for (uint32_t p = 0; p < PASSES; ++p) {
        const uint32_t i = p * NT + t, row = (i >> 3) & 31u, req = (i & 7u) + ((i >> 8) << 3);
        float f[E];
        ms_widen(v[p], f, RT{});
        float* dst = slab + (req * E) * 32u + (row ^ ((req & 7u) << 2));
#pragma unroll
        for (uint32_t j = 0; j < E; ++j) dst[j * 32u] = ok[p] ? f[j] : 0.0f;
    }
}

// ms_stage in two halves, for a kernel that keeps a tile's requests in flight while it multiplies the tile before:
// ms_fetch issues the requests of rows[0 .. nrows) x the row's first 128 k into `f`, ms_place writes them to `slab`.
template <typename RT, uint32_t NT>
struct MsFetch {
    static constexpr uint32_t E = 16u / sizeof(RT), PASSES = 32u * (kMsSlabK / E) / NT;
    uint4 v[PASSES];
    uint32_t nrows;
};
template <typename RT, uint32_t NT>
__device__ __forceinline__ void ms_fetch(MsFetch<RT, NT>& f, const uint8_t* rows, uint32_t stride, uint32_t nrows, uint32_t t) {
    f.nrows = nrows;
#pragma unroll
    for (uint32_t p = 0; p < MsFetch<RT, NT>::PASSES; ++p) {
        const uint32_t i = p * NT + t, row = (i >> 3) & 31u, req = (i & 7u) + ((i >> 8) << 3), byte = req << 4;
        const bool ok = row < nrows && byte < stride;
        f.v[p] = *reinterpret_cast<const uint4*>(rows + (ok ? (uint64_t)row * stride + byte : 0u));
    }
}
template <typename RT, uint32_t NT>
__device__ __forceinline__ void ms_place(float* slab, const MsFetch<RT, NT>& f, uint32_t stride, uint32_t t) {
    constexpr uint32_t E = MsFetch<RT, NT>::E;
#pragma unroll
    for (uint32_t p = 0; p < MsFetch<RT, NT>::PASSES; ++p) {
        const uint32_t i = p * NT + t, row = (i >> 3) & 31u, req = (i & 7u) + ((i >> 8) << 3);
        const bool ok = row < f.nrows && (req << 4) < stride;
        float x[E];
        ms_widen(f.v[p], x, RT{});
        float* dst = slab + (req * E) * 32u + (row ^ ((req & 7u) << 2));
#pragma unroll
        for (uint32_t j = 0; j < E; ++j) dst[j * 32u] = ok ? x[j] : 0.0f;
    }
}

}  // namespace
}  // namespace dann
