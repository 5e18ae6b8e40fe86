// maxsim_kernels.hip -- multi-vector (late-interaction) scores: MaxSim per query row and their Chamfer sum
// (diskann-quantization/src/multi_vector/: MaxSim, Chamfer, build_max_sim / MaxSimKernel::compute_max_sim).
//
// A query and a document are small row-major matrices of `dim`-long rows (f32 or f16, both of one type).  Two orders,
// because their bits differ (DANN_MAXSIM_KERNEL / DANN_MAXSIM_REFERENCE):
//
//   kernel order     scores[i] = -max_j ip(i, j), the maximum from f32::MIN, ip(i, j) ONE fma chain over k = 0 .. dim - 1
//                    from +0.0 (kernels/f32/v3.rs; f16 widened first, exactly).  v_mfma_f32_32x32x2_f32 is that chain
//                    bit for bit (pq_kernels.hip, pq_assign_mfma_kernel), so this order runs on the matrix cores:
//                    maxsim_mfma_kernel.
//   reference order  scores[i] = min_j InnerProduct::evaluate(q_i, d_j), the minimum from f32::MAX (fallback.rs:79-103):
//                    the pair function behind dann_distance_pairs, in a plain double loop: maxsim_rows_kernel.
//
// Chamfer = the sequential f32 sum of scores[i] in query-row order from 0.0; an empty document scores f32::MAX per row
// and has Chamfer 0.0 (the reference's callback never runs), an empty query has Chamfer 0.0.
//
// Outside the contract (as in the reference's own tests): NaN / infinite inputs (the CPU's vmaxps operand rule is not
// reproduced) and products that underflow to -0.0 (the sign of a zero maximum is then ambiguous in the reference).
//
// Rows, of documents and of queries, arrive here at a stride of whole 16-byte units, the bytes behind `dim` zero: every
// stage request is one aligned 16-byte load and a zero k-term is exact (fma(0, 0, s) = s; s is never -0.0).
#include <float.h>

#include "dann_device.h"
#include "dann_internal.h"
#include "maxsim_pair.h"
#include "wave_lists.h"

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

// ---- kernel order, on the matrix cores ---------------------------------------------------------------------------------
// One workgroup per (query, candidate); wavefront w owns the 32-row query tile w of a group of four, and a query of more
// than 128 rows is walked group by group (the document is then read again, from L2).  A = document rows (tile row i),
// B = query rows (tile column j): lane l holds 16 document rows of ONE query row -- register r = document row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the tile, query row l & 31 -- so the maximum over a tile's document rows and the
// running maximum over the document's tiles stay in the lane; the partner lane (l ^ 32) is combined once at the end.
// A document tile (32 rows) is staged once in LDS and read by all four wavefronts.  One accumulator set runs through the
// whole row -- ceil(dim / 2) MFMAs, an odd dim's last k-pair padded with zeros -- so no chain is ever split:
//   KS > 0   dim <= 2 KS <= 128: the wavefront's query tile is KS registers (one B operand per k-step), loaded once
//            through the slab and kept across the document's tiles;
//   KS == 0  any dim: 128-k slabs of the document tile AND of each wavefront's query tile are staged in turn while the
//            accumulators persist.
// Document rows past the document's end are masked out of the maximum (a zero row's ip = 0 would beat an all-negative
// document); query rows past the query's end are never written.
// LDS (floats): [scores: kMaxSimQueryRows][document slab: 4096]([query slabs: 4 x 4096] for KS == 0).
template <typename RT, int KS>
__global__ __launch_bounds__(kMsThreads) void maxsim_mfma_kernel(MaxSimArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ms_smem[];
    const MsPair p = ms_pair(a);
    if (!p.live) return;
    float* const sc = ms_smem;
    float* const dslab = ms_smem + kMaxSimQueryRows;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, l31 = lane & 31u, hi = lane >> 5;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    // wavefront w sits on SIMD w % 4: a one-tile query would put every workgroup's MFMAs on SIMD 0, so the tile owner
    // rotates with the workgroup
    const uint32_t wv = (wave + blockIdx.x + blockIdx.y) & (kMsWaves - 1u);
    const uint32_t qtiles = (p.qn + 31u) >> 5;
    const uint32_t esz = (uint32_t)sizeof(RT);
    for (uint32_t g0 = 0; g0 < qtiles; g0 += kMsWaves) {
        const uint32_t qt = g0 + wv;
        const bool has = qt < qtiles;
        const uint32_t qrows_here = has ? (p.qn - (qt << 5) < 32u ? p.qn - (qt << 5) : 32u) : 0u;
        const uint8_t* const qtile = p.q + (uint64_t)(has ? qt << 5 : 0u) * a.stride;
        float bq[KS > 0 ? KS : 1];
        if constexpr (KS > 0) {
            // the group's query tiles, one after the other through the document slab, each into its owner's registers
            for (uint32_t w = 0; w < kMsWaves && g0 + w < qtiles; ++w) {
                const uint32_t t = g0 + w, n = p.qn - (t << 5) < 32u ? p.qn - (t << 5) : 32u;
                __syncthreads();
                ms_stage<RT, kMsThreads>(dslab, p.q + (uint64_t)(t << 5) * a.stride, a.stride, n, 0u, tid);
                __syncthreads();
                if (wv == w) {
#pragma unroll
                    for (int m = 0; m < KS; ++m) {
                        const uint32_t k = 2u * (uint32_t)m + hi;
                        bq[m] = dslab[k * 32u + (l31 ^ ms_swz<RT>(k))];
                    }
                }
            }
        }
        float mx = -FLT_MAX;
        for (uint64_t ds = 0; ds < p.dn; ds += 32u) {
            const uint32_t dn_here = p.dn - ds < 32u ? (uint32_t)(p.dn - ds) : 32u;
            const uint8_t* const dtile = p.d + ds * a.stride;
            ms_f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            if constexpr (KS > 0) {
                __syncthreads();  // the slab's last readers are done
                ms_stage<RT, kMsThreads>(dslab, dtile, a.stride, dn_here, 0u, tid);
                __syncthreads();
                if (has) {
#pragma unroll
                    for (int m = 0; m < KS; ++m) {
                        const uint32_t k = 2u * (uint32_t)m + hi;
                        const float av = dslab[k * 32u + (l31 ^ ms_swz<RT>(k))];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bq[m], acc, 0, 0, 0);
                    }
                }
            } else {
                float* const qslab = dslab + kMsSlabFloats * (1u + wave);
                for (uint32_t k0 = 0; k0 < a.dim; k0 += kMsSlabK) {
                    __syncthreads();
                    ms_stage<RT, kMsThreads>(dslab, dtile, a.stride, dn_here, k0 * esz, tid);
                    if (has) ms_stage<RT, 64u>(qslab, qtile, a.stride, qrows_here, k0 * esz, lane);
                    __syncthreads();
                    if (has) {
                        const uint32_t left = a.dim - k0, steps = left >= kMsSlabK ? kMsSlabK / 2u : (left + 1u) >> 1;
                        for (uint32_t m = 0; m < steps; ++m) {
                            const uint32_t k = 2u * m + hi, o = k * 32u + (l31 ^ ms_swz<RT>(k));
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dslab[o], qslab[o], acc, 0, 0, 0);
                        }
                    }
                }
            }
            if (has) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t i = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * hi;
                    const float v = acc[r];
                    mx = (i < dn_here && v > mx) ? v : mx;
                }
            }
        }
        if (has) {
            const float other = __shfl_xor(mx, 32);
            mx = other > mx ? other : mx;
            const uint32_t row = (qt << 5) + l31;
            if (hi == 0u && row < p.qn) {
                const float s = -mx;  // the negation comes last: a maximum of +0.0 gives -0.0
                sc[row] = s;
                if (p.scores) p.scores[row] = s;
            }
        }
    }
    ms_chamfer(p, sc);
}

// ---- reference order, deliberately plain -------------------------------------------------------------------------------
// One workgroup per (query, candidate); a lane group of Scheme<DT, IP, pair>::G lanes walks the document's rows for one
// query row at a time with the bit-exact pair function (group_distance_rows: what dann_distance_pairs runs), the running
// minimum from f32::MAX in the group's first lane.
template <int DT>
__global__ __launch_bounds__(kMsThreads) void maxsim_rows_kernel(MaxSimArgs a) {
    __shared__ float sc[kMaxSimQueryRows];
    const MsPair p = ms_pair(a);
    if (!p.live) return;
    constexpr int G = Scheme<DT, OP_IP, true>::G;
    const uint32_t g = threadIdx.x / G, groups = kMsThreads / G;
    const int v = (int)(threadIdx.x % G);
    for (uint32_t i = g; i < p.qn; i += groups) {  // whole groups leave together (G divides 64)
        const uint8_t* x = p.q + (uint64_t)i * a.stride;
        float mn = FLT_MAX;
        for (uint64_t j = 0; j < p.dn; ++j) {
            const float raw = group_distance_rows<DT, OP_IP>(x, p.d + j * a.stride, (int)a.dim, v);
            const float d = post_op<OP_IP, false>(raw);
            mn = d < mn ? d : mn;
        }
        if (v == 0) {
            sc[i] = mn;
            if (p.scores) p.scores[i] = mn;
        }
    }
    ms_chamfer(p, sc);
}

// ---- the rerank's sort ---------------------------------------------------------------------------------------------------
// rerank_kernel's sort and padding (distance_kernels.hip) over distances that are already there: live candidates
// compacted in candidate order, a bitonic sort of (distance bits, position) keys -- equal distances keep candidate order,
// -0.0 == +0.0 -- and the first k written, the rest padded with 0xFFFFFFFF / +infinity.  One workgroup per query.
__global__ __launch_bounds__(kMsThreads) void chamfer_sort_kernel(const uint32_t* cand, const float* chamfer, uint32_t stride,
                                                                 uint32_t ndocs, uint32_t k, uint32_t* out_ids,
                                                                 float* out_d, uint32_t* out_counts) {
    extern __shared__ __attribute__((aligned(16))) uint8_t srt_smem[];
    __shared__ uint32_t wave_n[kMsWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, qi = blockIdx.x;
    uint32_t pcap = 64;
    while (pcap < stride) pcap <<= 1;
    uint64_t* keys = reinterpret_cast<uint64_t*>(srt_smem);
    uint32_t* pos_of = reinterpret_cast<uint32_t*>(srt_smem + (size_t)pcap * 8);  // compacted slot -> candidate position
    uint32_t n = 0;
    for (uint32_t i0 = 0; i0 < stride; i0 += kMsThreads) {
        const uint32_t i = i0 + tid;
        const uint32_t id = i < stride ? cand[(uint64_t)qi * stride + i] : kEmpty;
        const bool ok = id != kEmpty && id < ndocs;
        const uint64_t m = ballot64(ok);
        if (lane == 0) wave_n[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kMsWaves; ++w) {
            before += w < wave ? wave_n[w] : 0u;
            total += wave_n[w];
        }
        if (ok) pos_of[n + before + mbcnt(m)] = i;
        n += total;
        __syncthreads();
    }
    for (uint32_t i = tid; i < pcap; i += kMsThreads)
        keys[i] = i < n ? dist_key(chamfer[(uint64_t)qi * stride + pos_of[i]], i) : ~0ull;
    __syncthreads();
    block_bitonic(keys, pcap, kMsThreads);
    for (uint32_t r = tid; r < k; r += kMsThreads) {
        uint32_t id = kEmpty;
        float d = __builtin_inff();
        if (r < n) {
            const uint32_t pos = pos_of[(uint32_t)keys[r]];
            id = cand[(uint64_t)qi * stride + pos];
            d = chamfer[(uint64_t)qi * stride + pos];
        }
        out_ids[(uint64_t)qi * k + r] = id;
        out_d[(uint64_t)qi * k + r] = d;
    }
    if (tid == 0) out_counts[qi] = n < k ? n : k;
}

template <typename RT>
int32_t launch_mfma(const MaxSimArgs& a, dim3 grid, hipStream_t stream) {
    const size_t lds_reg = (kMaxSimQueryRows + kMsSlabFloats) * sizeof(float);
    const size_t lds_slab = (kMaxSimQueryRows + kMsSlabFloats * (1u + kMsWaves)) * sizeof(float);
    const char* what = "maxsim_mfma_kernel launch";
    if (a.dim <= 32)
        return launch_kernel<maxsim_mfma_kernel<RT, 16>>(what, grid, dim3(kMsThreads), lds_reg, stream, a);
    if (a.dim <= 64)
        return launch_kernel<maxsim_mfma_kernel<RT, 32>>(what, grid, dim3(kMsThreads), lds_reg, stream, a);
    if (a.dim <= 128)
        return launch_kernel<maxsim_mfma_kernel<RT, 64>>(what, grid, dim3(kMsThreads), lds_reg, stream, a);
    return launch_kernel<maxsim_mfma_kernel<RT, 0>>(what, grid, dim3(kMsThreads), lds_slab, stream, a);
}

}  // namespace

int32_t launch_maxsim(int32_t dtype, int32_t order, const MaxSimArgs& a, uint32_t nq, hipStream_t stream) {
    if (nq == 0) return DANN_OK;
    const dim3 grid(a.cand_stride, nq);
    if (order == DANN_MAXSIM_KERNEL)
        return dtype == DT_F32 ? launch_mfma<float>(a, grid, stream) : launch_mfma<__half>(a, grid, stream);
    const char* what = "maxsim_rows_kernel launch";
    if (dtype == DT_F32) return launch_kernel<maxsim_rows_kernel<DT_F32>>(what, grid, dim3(kMsThreads), 0, stream, a);
    return launch_kernel<maxsim_rows_kernel<DT_F16>>(what, grid, dim3(kMsThreads), 0, stream, a);
}

int32_t launch_chamfer_sort(const uint32_t* d_cand, const float* d_chamfer, uint32_t nq, uint32_t stride, uint32_t ndocs,
                            uint32_t k, uint32_t* d_out_ids, float* d_out_d, uint32_t* d_out_counts, hipStream_t stream) {
    if (nq == 0) return DANN_OK;
    uint32_t pcap = 64;
    while (pcap < stride) pcap <<= 1;
    return launch_kernel<chamfer_sort_kernel>("chamfer_sort_kernel launch", dim3(nq), dim3(kMsThreads), (size_t)pcap * 12, stream,
                                              d_cand, d_chamfer, stride, ndocs, k, d_out_ids, d_out_d, d_out_counts);
}

}  // namespace dann
