// projected_eigen_kernels.hip -- the third multi-vector distance of diskann-quantization/src/multi_vector/distance/:
// ProjectedEigen (projected_eigen.rs; evaluated by FallbackKernel::projected_eigen_kernel, fallback.rs:105-147, 207-226).
//
//   score[i]             = sum over the document's rows j, in row order, of -(ip(i, j) * ip(i, j)), from +0.0
//   ProjectedEigen(Q, D) = sum over the query's rows i, in row order, of score[i], from +0.0
//
// Both sums are sequential f32 sums and every operation rounds on its own: the multiply, the (exact) negation, the add.
// The unit is compiled with -ffp-contract=off and without the packed f32 instructions (build.py).  Two orders, as for
// MaxSim (maxsim_kernels.hip), and only ip(i, j) differs between them:
//
//   reference order  ip = InnerProduct::evaluate(q_i, d_j), the pair function behind dann_distance_pairs: the reference,
//                    bit for bit (projeig_rows_kernel).
//   kernel order     ip = ONE fma chain over k = 0 .. dim - 1 from +0.0 (f16 widened first, exactly), which is what
//                    v_mfma_f32_32x32x2_f32 produces (projeig_mfma_kernel).  The reference has no SIMD kernel for this
//                    distance: this order is this project's own.
//
// A document without rows has score +0.0 per row and total +0.0; a query without rows has total +0.0.  A zero padding row
// contributes -(0 * 0) = -0.0 and s + -0.0 == s for every s, +0.0 included: padded document rows need no mask, and no
// result is ever -0.0.  Outside the contract: NaN / infinite inputs and ip * ip that overflows.
#include "dann_device.h"
#include "dann_internal.h"
#include "maxsim_pair.h"
#include "maxsim_stage.h"

namespace dann {
namespace {

// ---- kernel order, on the matrix cores ---------------------------------------------------------------------------------
// maxsim_mfma_kernel's shape: one workgroup per (query, candidate), wavefront w owns the 32-row query tile w of a group of
// four, a document tile (32 rows) is staged once in LDS and read by all four, A = document rows, B = query rows, one
// accumulator set through the whole row (KS > 0: the query tile in KS registers for dim <= 2 KS <= 128; KS == 0: 128-k
// slabs of both for any dim).  What is new is that the document rows must be folded IN ROW ORDER:
//
// The MFMA result gives lane l = 32 hi + c the tile rows (r & 3) + 8 (r >> 2) + 4 hi of column c in register r.  Tile row
// t of the A operand is therefore fed with document row pe_doc_row(t) -- a permutation of the LDS READ index, the stage is
// unchanged, and a permutation of 32 words of one k line still touches 32 distinct banks whatever ms_swz adds -- so that
// register r of lane half hi holds document row 16 hi + r.  Half 0 then folds rows 0 .. 15 into the running sum (16
// multiplies, 16 dependent adds), hands it to lane l + 32, half 1 folds rows 16 .. 31 and hands it back: two cross-lane
// moves per tile, the sum in registers across the document's tiles.  (Both halves execute both folds; the half whose turn
// it is not computes a value nobody reads.)
// LDS (floats): [scores: kMaxSimQueryRows][document slab: 4096]([query slabs: 4 x 4096] for KS == 0).
__device__ __forceinline__ uint32_t pe_doc_row(uint32_t t) {
    // the inverse of t = (r & 3) + 8 (r >> 2) + 4 hi at document row 16 hi + r
    return (((t >> 2) & 1u) << 4) + (t & 3u) + ((t >> 3) << 2);
}

template <typename RT, int KS>
__global__ __launch_bounds__(kMsThreads) void projeig_mfma_kernel(MaxSimArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pe_smem[];
    const MsPair p = ms_pair(a, 0.0f);
    if (!p.live) return;
    float* const sc = pe_smem;
    float* const dslab = pe_smem + kMaxSimQueryRows;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, l31 = lane & 31u, hi = lane >> 5;
    const uint32_t drow = pe_doc_row(l31);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    // the tile owner rotates with the workgroup, as in maxsim_mfma_kernel: a one-tile query must not pin SIMD 0
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
        float sum = 0.0f;  // (meaningful in lane half 0 between tiles)
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
                        const float av = dslab[k * 32u + (drow ^ ms_swz<RT>(k))];
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
                            const uint32_t k = 2u * m + hi, s = ms_swz<RT>(k);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dslab[k * 32u + (drow ^ s)], qslab[k * 32u + (l31 ^ s)],
                                                                       acc, 0, 0, 0);
                        }
                    }
                }
            }
            if (has) {
                float sq[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) sq[r] = -(acc[r] * acc[r]);
                float lo = sum;
#pragma unroll
                for (int r = 0; r < 16; ++r) lo = lo + sq[r];  // half 0: the tile's rows 0 .. 15
                float up = __shfl_xor(lo, 32);
#pragma unroll
                for (int r = 0; r < 16; ++r) up = up + sq[r];  // half 1: rows 16 .. 31, on top of half 0's sum
                sum = __shfl_xor(up, 32);
            }
        }
        if (has) {
            const uint32_t row = (qt << 5) + l31;
            if (hi == 0u && row < p.qn) {
                sc[row] = sum;
                if (p.scores) p.scores[row] = sum;
            }
        }
    }
    ms_chamfer(p, sc);  // the same sequential fold over the query's rows as Chamfer's
}

// ---- reference order, deliberately plain -------------------------------------------------------------------------------
// maxsim_rows_kernel's walk: a lane group of Scheme<DT, IP, pair>::G lanes per query row, the bit-exact pair function per
// document row (group_distance_rows), the sequential sum in the group's first lane.
template <int DT>
__global__ __launch_bounds__(kMsThreads) void projeig_rows_kernel(MaxSimArgs a) {
    __shared__ float sc[kMaxSimQueryRows];
    const MsPair p = ms_pair(a, 0.0f);
    if (!p.live) return;
    constexpr int G = Scheme<DT, OP_IP, true>::G;
    const uint32_t g = threadIdx.x / G, groups = kMsThreads / G;
    const int v = (int)(threadIdx.x % G);
    for (uint32_t i = g; i < p.qn; i += groups) {  // whole groups leave together (G divides 64)
        const uint8_t* x = p.q + (uint64_t)i * a.stride;
        float sum = 0.0f;
        for (uint64_t j = 0; j < p.dn; ++j) {
            const float raw = group_distance_rows<DT, OP_IP>(x, p.d + j * a.stride, (int)a.dim, v);
            const float ip = post_op<OP_IP, false>(raw);  // InnerProduct::evaluate: the negated inner product
            sum = sum + -(ip * ip);
        }
        if (v == 0) {
            sc[i] = sum;
            if (p.scores) p.scores[i] = sum;
        }
    }
    ms_chamfer(p, sc);
}

template <typename RT>
int32_t launch_mfma(const MaxSimArgs& a, dim3 grid, hipStream_t stream) {
    const size_t lds_reg = (kMaxSimQueryRows + kMsSlabFloats) * sizeof(float);
    const size_t lds_slab = (kMaxSimQueryRows + kMsSlabFloats * (1u + kMsWaves)) * sizeof(float);
    const char* what = "projeig_mfma_kernel launch";
    if (a.dim <= 32)
        return launch_kernel<projeig_mfma_kernel<RT, 16>>(what, grid, dim3(kMsThreads), lds_reg, stream, a);
    if (a.dim <= 64)
        return launch_kernel<projeig_mfma_kernel<RT, 32>>(what, grid, dim3(kMsThreads), lds_reg, stream, a);
    if (a.dim <= 128)
        return launch_kernel<projeig_mfma_kernel<RT, 64>>(what, grid, dim3(kMsThreads), lds_reg, stream, a);
    return launch_kernel<projeig_mfma_kernel<RT, 0>>(what, grid, dim3(kMsThreads), lds_slab, stream, a);
}

}  // namespace

int32_t launch_projected_eigen(int32_t dtype, int32_t order, const MaxSimArgs& a, uint32_t nq, hipStream_t stream) {
    if (nq == 0) return DANN_OK;
    const dim3 grid(a.cand_stride, nq);
    if (order == DANN_MAXSIM_KERNEL)
        return dtype == DT_F32 ? launch_mfma<float>(a, grid, stream) : launch_mfma<__half>(a, grid, stream);
    const char* what = "projeig_rows_kernel launch";
    if (dtype == DT_F32) return launch_kernel<projeig_rows_kernel<DT_F32>>(what, grid, dim3(kMsThreads), 0, stream, a);
    return launch_kernel<projeig_rows_kernel<DT_F16>>(what, grid, dim3(kMsThreads), 0, stream, a);
}

}  // namespace dann
