// maxsim_mm_kernels.hip -- MaxSim / Chamfer over MinMax-quantised token rows (diskann-quantization/src/minmax/multi/:
// MinMaxMeta<NBITS>, MinMaxKernel::max_sim_kernel, MaxSim::evaluate, Chamfer::evaluate), for the reference's seven
// (query bits, document bits) pairs: (1,1) (2,2) (4,4) (8,8) (8,4) (8,2) (8,1).
//
// Query row x is the kernel's FIRST argument, document row y its second (minmax/vectors.rs:206-229):
//   raw = the exact u32 inner product of the codes;  v = minmax_value(raw as f32, x, y, dim)  (dann_device.h)
//   scores[i] = min_j -v(i, j), the minimum from f32::MAX;  Chamfer = their sequential f32 sum (ms_chamfer)
// raw is an integer, so it has no summation order; the f32 epilogue has one statement, minmax_value.  Both orders of
// dann.h therefore return the same bits and `order` only picks the kernel:
//   DANN_MAXSIM_KERNEL     maxsim_mm_mfma_kernel: raw on the int8 matrix cores (v_mfma_i32_32x32x32_i8)
//   DANN_MAXSIM_REFERENCE  maxsim_mm_rows_kernel: raw by the dot / popcount helpers of the search kernels on the packed codes,
//                          or a plain unpack-and-multiply loop -- no matrix cores, no bias
//
// Device layout (mm_repack_kernel, from the canonical images): the codes stay packed, at a stride of whole 16-byte units,
// every bit at or beyond dim * bits zero; beside them one MmRowHeader per row.  An image's u32 dim field is not read.
#include <float.h>

#include "dann_device.h"
#include "dann_internal.h"
#include "maxsim_pair.h"

namespace dann {
namespace {

typedef int mm_i32x4 __attribute__((ext_vector_type(4)));
typedef int mm_i32x16 __attribute__((ext_vector_type(16)));

// ---- repack ---------------------------------------------------------------------------------------------------------------
// sum of the BITS-wide fields of a dword
template <int BITS>
__device__ __forceinline__ uint32_t mm_field_sum(uint32_t w) {
    if constexpr (BITS == 8) return __builtin_amdgcn_udot4(w, 0x01010101u, 0u, false);
    else if constexpr (BITS == 4) return __builtin_amdgcn_udot8(w, 0x11111111u, 0u, false);
    else if constexpr (BITS == 2) return (uint32_t)__builtin_popcount(w & 0x55555555u) + 2u * (uint32_t)__builtin_popcount(w & 0xAAAAAAAAu);
    else return (uint32_t)__builtin_popcount(w);
}

// One wavefront per row.  Images are byte-aligned only (20 + code bytes each), so they are read byte by byte, every byte
// at a clamped address and zeroed afterwards; the bits at or beyond dim * BITS of the last code byte are cleared.
template <int BITS>
__global__ __launch_bounds__(kMsThreads) void mm_repack_kernel(const uint8_t* images, uint32_t image_bytes, uint64_t nrows,
                                                              uint32_t dim, uint8_t* codes, uint32_t stride, MmRowHeader* hdr) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row = (uint64_t)blockIdx.x * kMsWaves + (threadIdx.x >> 6);
    if (row >= nrows) return;  // (whole wavefronts)
    const uint8_t* img = images + row * image_bytes;
    const uint32_t total_bits = dim * (uint32_t)BITS, cb = (total_bits + 7u) >> 3;
    uint32_t* out = reinterpret_cast<uint32_t*>(codes + row * stride);
    uint32_t sum = 0;
    for (uint32_t w = lane; w < (stride >> 2); w += 64u) {
        uint32_t word = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t i = 4u * w + j;
            const uint32_t byte = img[kMmHeader + (i < cb ? i : 0u)];
            word |= (i < cb ? byte : 0u) << (8u * j);
        }
        const uint32_t first = 32u * w;  // the word's first bit
        const uint32_t nb = total_bits > first ? total_bits - first : 0u;
        word &= nb >= 32u ? 0xFFFFFFFFu : ((1u << nb) - 1u);
        out[w] = word;
        sum += mm_field_sum<BITS>(word);
    }
    for (int o = 1; o < 64; o <<= 1) sum += (uint32_t)__shfl_xor((int)sum, o);
    if (lane == 0) {
        MmRowHeader h;
        h.b = load_f32_unaligned(img + 4);
        h.n = load_f32_unaligned(img + 8);
        h.a = load_f32_unaligned(img + 12);
        h.sum = (int32_t)sum - (BITS == 8 ? 128 * (int32_t)dim : 0);
        hdr[row] = h;
    }
}

// ---- kernel order, on the int8 matrix cores --------------------------------------------------------------------------------
// The workgroup shape of maxsim_mfma_kernel (maxsim_kernels.hip): one workgroup per (query, candidate), wavefront w owns
// the 32-row query tile w of a group of four, queries of more than 128 rows are walked group by group, a document tile of
// 32 rows is staged once in LDS and read by all four wavefronts.  A = document rows, B = query rows: lane l holds, in
// register r, document row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the tile against query row l & 31, so the running minimum
// stays in the lane and the partner lane l ^ 32 is combined once at the end.
//
// Staging unpacks the codes to one SIGNED byte each: 1-, 2- and 4-bit codes as they are, 8-bit codes as c - 128 = c ^ 0x80
// where k < dim and 0 beyond (pad AFTER biasing).  With beta = 1 for an 8-bit side, 0 otherwise, and primes for the bytes:
//   sum cq cd = sum q' d' + 128 beta_d sum q' + 128 beta_q sum d' + 16384 beta_q beta_d dim      (all in i32; < 2^31)
// sum q', sum d' are the header records' `sum` fields.  The lane -> k map of the MFMA's operands need not be known: both
// operands are read from LDS at the same k assignment -- lane l reads bytes [32 m + 16 (l >> 5), + 16) of row l & 31 in
// k-step m -- and integer addition commutes.
//
// A slab is 32 rows x 128 k at a row stride of 144 bytes: the operand reads (16 bytes per lane, 8 consecutive rows per
// 128 bytes of banks) and the stage's 16-byte writes (8 lanes per row) are aligned and conflict-free.  One accumulator set
// runs through ceil(dim / 32) k-steps, slab after slab.  dim <= 128: the group's query tiles are staged once and stay in
// LDS across the document's tiles; else they are staged again with each document slab.
// LDS: [scores: kMaxSimQueryRows f32][document tile headers: 32 x 16][document slab][4 query slabs].
constexpr uint32_t kMmSlabK = 128, kMmRowStride = kMmSlabK + 16u, kMmSlabBytes = 32u * kMmRowStride;
constexpr size_t kMmLds = kMaxSimQueryRows * 4u + 32u * sizeof(MmRowHeader) + (size_t)kMmSlabBytes * (1u + kMsWaves);

// 16 codes starting at code index k0 (a multiple of 16) of a packed row -> 16 bytes, element order kept.  `src` is the
// 2 BITS source bytes (in the low dwords); `dim` bounds the 8-bit bias.
template <int BITS>
__device__ __forceinline__ uint4 mm_unpack16(const uint4& src, uint32_t k0, uint32_t dim) {
    uint32_t o[4];
    if constexpr (BITS == 8) {
        const uint32_t s[4] = {src.x, src.y, src.z, src.w};
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t k = k0 + 4u * j, nv = dim > k ? dim - k : 0u;  // codes of this dword below dim
            o[j] = s[j] ^ (nv >= 4u ? 0x80808080u : (0x80808080u & ((1u << (8u * nv)) - 1u)));
        }
    } else if constexpr (BITS == 4) {
        const uint32_t s[2] = {src.x, src.y};
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            uint32_t h = (s[j >> 1] >> (16u * (j & 1u))) & 0xFFFFu;  // four nibbles
            h = (h | (h << 8)) & 0x00FF00FFu;
            o[j] = (h | (h << 4)) & 0x0F0F0F0Fu;
        }
    } else if constexpr (BITS == 2) {
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            uint32_t h = (src.x >> (8u * j)) & 0xFFu;  // four 2-bit fields
            h = (h | (h << 12)) & 0x000F000Fu;
            o[j] = (h | (h << 6)) & 0x03030303u;
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) o[j] = (((src.x >> (4u * j)) & 0xFu) * 0x00204081u) & 0x01010101u;  // four bits
    }
    return uint4{o[0], o[1], o[2], o[3]};
}

// the 2 BITS bytes at `p` (aligned to their size), in the low dwords of a uint4
template <int BITS>
__device__ __forceinline__ uint4 mm_load_src(const uint8_t* p) {
    if constexpr (BITS == 8) return *reinterpret_cast<const uint4*>(p);
    else if constexpr (BITS == 4) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        return uint4{t.x, t.y, 0u, 0u};
    } else if constexpr (BITS == 2) return uint4{*reinterpret_cast<const uint32_t*>(p), 0u, 0u, 0u};
    else return uint4{(uint32_t)*reinterpret_cast<const uint16_t*>(p), 0u, 0u, 0u};
}

// One slab request: thread t of 256 takes row t >> 3, codes [k0 + 16 (t & 7), + 16) of the slab that starts at code k0.
// Rows >= nrows and codes at or beyond the row's stride read as zero: every load is issued unconditionally at a clamped
// address (the first row's first bytes) and zeroed afterwards.
template <int BITS>
struct MmReq {
    uint4 v;
    bool ok;
    __device__ __forceinline__ void load(const uint8_t* rows, uint32_t stride, uint32_t nrows, uint32_t k0, uint32_t t) {
        const uint32_t row = t >> 3, byte = ((k0 + 16u * (t & 7u)) * (uint32_t)BITS) >> 3;
        ok = row < nrows && byte < stride;
        v = mm_load_src<BITS>(rows + (ok ? (uint64_t)row * stride + byte : 0u));
    }
    __device__ __forceinline__ void store(uint8_t* slab, uint32_t k0, uint32_t dim, uint32_t t) const {
        const uint4 u = mm_unpack16<BITS>(v, k0 + 16u * (t & 7u), dim);
        *reinterpret_cast<uint4*>(slab + (t >> 3) * kMmRowStride + 16u * (t & 7u)) = ok ? u : uint4{0u, 0u, 0u, 0u};
    }
};

template <int QBITS, int DBITS>
__global__ __launch_bounds__(kMsThreads) void maxsim_mm_mfma_kernel(MaxSimArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mm_smem[];
    const MsPair p = ms_pair(a);
    if (!p.live) return;
    constexpr int32_t BQ = QBITS == 8 ? 1 : 0, BD = DBITS == 8 ? 1 : 0;
    float* const sc = reinterpret_cast<float*>(mm_smem);
    MmRowHeader* const dh = reinterpret_cast<MmRowHeader*>(mm_smem + kMaxSimQueryRows * 4u);
    uint8_t* const dslab = reinterpret_cast<uint8_t*>(dh + 32);
    uint8_t* const qslabs = dslab + kMmSlabBytes;
    const MmRowHeader* const qhdr = a.qhdr + p.q0;
    const MmRowHeader* const dhdr = a.dhdr + p.d0;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, l31 = lane & 31u, hi = lane >> 5;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    // (the tile owner rotates with the workgroup, as in maxsim_mfma_kernel: a one-tile query would load SIMD 0 alone)
    const uint32_t wv = (wave + blockIdx.x + blockIdx.y) & (kMsWaves - 1u);
    const uint32_t qtiles = (p.qn + 31u) >> 5;
    const bool one_slab = a.dim <= kMmSlabK;
    const uint8_t* const qslab = qslabs + wv * kMmSlabBytes;
    const uint32_t opnd = l31 * kMmRowStride + 16u * hi;  // the lane's operand bytes of k-step 0
    for (uint32_t g0 = 0; g0 < qtiles; g0 += kMsWaves) {
        const uint32_t qt = g0 + wv;
        const bool has = qt < qtiles;
        // the group's four query tiles (tiles past the query's end: zero rows) into the four query slabs
        auto stage_queries = [&](uint32_t k0) {
            MmReq<QBITS> r[kMsWaves];
#pragma unroll
            for (uint32_t w = 0; w < kMsWaves; ++w) {
                const uint32_t first = (g0 + w) << 5;
                const uint32_t n = first < p.qn ? (p.qn - first < 32u ? p.qn - first : 32u) : 0u;
                r[w].load(p.q + (uint64_t)(n ? first : 0u) * a.qstride, a.qstride, n, k0, tid);
            }
#pragma unroll
            for (uint32_t w = 0; w < kMsWaves; ++w) r[w].store(qslabs + w * kMmSlabBytes, k0, a.dim, tid);
        };
        // the lane's query row: its header stays in registers (a clamped read for rows past the query's end)
        const uint32_t qrow = (qt << 5) + l31;
        const MmRowHeader xh = qhdr[has && qrow < p.qn ? qrow : 0u];
        if (one_slab) {
            __syncthreads();  // the last group's readers are done
            stage_queries(0u);
        }
        float mn = FLT_MAX;
        for (uint64_t ds = 0; ds < p.dn; ds += 32u) {
            const uint32_t dn_here = p.dn - ds < 32u ? (uint32_t)(p.dn - ds) : 32u;
            const uint8_t* const dtile = p.d + ds * a.stride;
            mm_i32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0;
            for (uint32_t k0 = 0; k0 < a.dim; k0 += kMmSlabK) {
                __syncthreads();  // the slabs' last readers are done
                MmReq<DBITS> rd;
                rd.load(dtile, a.stride, dn_here, k0, tid);
                MmRowHeader hd = dhdr[ds + (tid < dn_here ? tid : 0u)];
                if (!one_slab) stage_queries(k0);
                rd.store(dslab, k0, a.dim, tid);
                if (k0 == 0u && tid < 32u) dh[tid] = hd;
                __syncthreads();
                if (has) {
                    const uint32_t left = a.dim - k0, steps = left >= kMmSlabK ? kMmSlabK / 32u : (left + 31u) >> 5;
                    for (uint32_t m = 0; m < steps; ++m) {
                        const mm_i32x4 av = *reinterpret_cast<const mm_i32x4*>(dslab + opnd + 32u * m);
                        const mm_i32x4 bv = *reinterpret_cast<const mm_i32x4*>(qslab + opnd + 32u * m);
                        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc, 0, 0, 0);
                    }
                }
            }
            if (has) {
                const int32_t fixed = 128 * BD * xh.sum + 16384 * BQ * BD * (int32_t)a.dim;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t i = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * hi;
                    const MmRowHeader yh = dh[i];
                    const int32_t raw = acc[r] + fixed + 128 * BQ * yh.sum;
                    const float d = -minmax_value((float)(uint32_t)raw, xh.b, xh.n, xh.a, yh.b, yh.n, yh.a, a.dim);
                    // rows past the document's end are masked out: a phantom zero row scores -0.0 and would beat a
                    // document whose true scores are all positive
                    mn = (i < dn_here && d < mn) ? d : mn;
                }
            }
        }
        if (has) {
            const float other = __shfl_xor(mn, 32);
            mn = other < mn ? other : mn;
            if (hi == 0u && qrow < p.qn) {
                sc[qrow] = mn;
                if (p.scores) p.scores[qrow] = mn;
            }
        }
    }
    ms_chamfer(p, sc);
}

// ---- reference order, deliberately plain -----------------------------------------------------------------------------------
// One workgroup per (query, candidate); a group of four lanes walks the document's rows for one query row at a time, the
// running minimum from f32::MAX (valid in every lane of the group; the first writes).  Equal widths: lane v takes the code
// dwords v, v + 4, ... of both rows through mm_dot (v_dot4_u32_u8 / v_dot8_u32_u4 / popcount) -- the rows' zero padding
// needs no mask.  (8, narrower): lane v takes codes v, v + 4, ..., one byte against one unpacked field.
constexpr uint32_t kMmRowsG = 4, kMmRowsGroups = kMsThreads / kMmRowsG;

template <int QBITS, int DBITS>
__device__ __forceinline__ uint32_t mm_rows_raw(const uint8_t* x, const uint8_t* y, uint32_t dim, uint32_t stride, uint32_t v) {
    uint32_t t = 0;
    if constexpr (QBITS == DBITS) {
        const uint32_t* xw = reinterpret_cast<const uint32_t*>(x);
        const uint32_t* yw = reinterpret_cast<const uint32_t*>(y);
        for (uint32_t w = v; w < (stride >> 2); w += kMmRowsG) t = mm_dot<DBITS>(xw[w], yw[w], t);
    } else {
        static_assert(QBITS == 8, "the mixed pairs have an 8-bit query");
        for (uint32_t k = v; k < dim; k += kMmRowsG) {
            const uint32_t bit = k * (uint32_t)DBITS;
            t += (uint32_t)x[k] * (((uint32_t)y[bit >> 3] >> (bit & 7u)) & ((1u << DBITS) - 1u));
        }
    }
    return group4_sum(t);
}

template <int QBITS, int DBITS>
__global__ __launch_bounds__(kMsThreads) void maxsim_mm_rows_kernel(MaxSimArgs a) {
    __shared__ float sc[kMaxSimQueryRows];
    const MsPair p = ms_pair(a);
    if (!p.live) return;
    const uint32_t g = threadIdx.x / kMmRowsG, v = threadIdx.x % kMmRowsG;
    for (uint32_t i = g; i < p.qn; i += kMmRowsGroups) {  // whole groups leave together
        const uint8_t* x = p.q + (uint64_t)i * a.qstride;
        const MmRowHeader xh = a.qhdr[p.q0 + i];
        float mn = FLT_MAX;
        for (uint64_t j = 0; j < p.dn; ++j) {
            const uint32_t raw = mm_rows_raw<QBITS, DBITS>(x, p.d + j * a.stride, a.dim, a.stride, v);
            const MmRowHeader yh = a.dhdr[p.d0 + j];
            const float d = -minmax_value((float)raw, xh.b, xh.n, xh.a, yh.b, yh.n, yh.a, a.dim);
            mn = d < mn ? d : mn;
        }
        if (v == 0) {
            sc[i] = mn;
            if (p.scores) p.scores[i] = mn;
        }
    }
    ms_chamfer(p, sc);
}

template <int QBITS, int DBITS>
int32_t launch_pair(int32_t order, const MaxSimArgs& a, dim3 grid, hipStream_t stream) {
    if (order == DANN_MAXSIM_KERNEL)
        return launch_kernel<maxsim_mm_mfma_kernel<QBITS, DBITS>>("maxsim_mm_mfma_kernel launch", grid, dim3(kMsThreads), kMmLds,
                                                                  stream, a);
    return launch_kernel<maxsim_mm_rows_kernel<QBITS, DBITS>>("maxsim_mm_rows_kernel launch", grid, dim3(kMsThreads), 0, stream, a);
}

}  // namespace

int32_t launch_mm_repack(int32_t dtype, const uint8_t* d_images, uint32_t image_bytes, uint64_t nrows, uint32_t dim,
                         uint8_t* d_codes, uint32_t stride, MmRowHeader* d_hdr, hipStream_t stream) {
    if (nrows == 0) return DANN_OK;
    const dim3 grid((uint32_t)((nrows + kMsWaves - 1u) / kMsWaves)), block(kMsThreads);
    const char* what = "mm_repack_kernel launch";
    switch (dtype) {
        case DT_MM1: return launch_kernel<mm_repack_kernel<1>>(what, grid, block, 0, stream, d_images, image_bytes, nrows, dim, d_codes, stride, d_hdr);
        case DT_MM2: return launch_kernel<mm_repack_kernel<2>>(what, grid, block, 0, stream, d_images, image_bytes, nrows, dim, d_codes, stride, d_hdr);
        case DT_MM4: return launch_kernel<mm_repack_kernel<4>>(what, grid, block, 0, stream, d_images, image_bytes, nrows, dim, d_codes, stride, d_hdr);
        case DT_MM8: return launch_kernel<mm_repack_kernel<8>>(what, grid, block, 0, stream, d_images, image_bytes, nrows, dim, d_codes, stride, d_hdr);
    }
    return DANN_EINVAL;
}

int32_t launch_maxsim_mm(int32_t qdtype, int32_t dtype, int32_t order, const MaxSimArgs& a, uint32_t nq, hipStream_t stream) {
    if (nq == 0) return DANN_OK;
    const dim3 grid(a.cand_stride, nq);
    if (qdtype == dtype) {
        switch (dtype) {
            case DT_MM1: return launch_pair<1, 1>(order, a, grid, stream);
            case DT_MM2: return launch_pair<2, 2>(order, a, grid, stream);
            case DT_MM4: return launch_pair<4, 4>(order, a, grid, stream);
            case DT_MM8: return launch_pair<8, 8>(order, a, grid, stream);
        }
    } else if (qdtype == DT_MM8) {
        switch (dtype) {
            case DT_MM1: return launch_pair<8, 1>(order, a, grid, stream);
            case DT_MM2: return launch_pair<8, 2>(order, a, grid, stream);
            case DT_MM4: return launch_pair<8, 4>(order, a, grid, stream);
        }
    }
    set_error("no MinMax kernel for query dtype %d on rows of dtype %d", qdtype, dtype);
    return DANN_EUNSUPPORTED;
}

}  // namespace dann
