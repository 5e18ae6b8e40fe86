// gram_tiles.hip -- the Gram tile kernels of the matrix-core prune (prune_gram.hip describes the three-kernel pipeline and
// what the sweep does with a Gram entry), the longest-first order of their workgroups, and dann_debug_gram_tiles.
//
// One 8-wave workgroup per candidate list: the lower-triangular 32 x 32 tiles of G = C[0..ng) x C[0..mg)^T, dealt out to
// the waves one at a time; rows streamed through two 32-column LDS slabs (the next slab's global loads in flight under
// the MFMAs, written to the other slab behind them, one barrier per slab).  Two kernels:
//   gram_tiles_kernel<RT>   f32 slabs, v_mfma_f32_32x32x2_f32: one k-ordered f32 FMA chain per entry, the reference's bit for
//                           bit; RT = float, or __half widened exactly while a slab is filled (DANN_DBG_GRAM_F16_WIDEN;
//                           dann_debug_gram_tiles: DANN_F16 | 0x100);
//   gram_tiles_f16_kernel   f16 rows kept as halves, v_mfma_f32_32x32x16_f16 (the builds' default for f16 rows).
// They state the deal of tiles to waves and the slab loop twice.  One kernel over a slab policy was tried: its f32
// instantiations compile to the same machine code, the f16 matrix-core one to a loop with one more scalar branch per
// slab, 0.3 % slower on a 200 000 x 768 build -- so the two stay as they are (tests/test_gram_tile_assignment.py models
// the deal once; a fix to one copy has to be made in the other).
#include <algorithm>
#include <vector>

#include "build_common.h"
#include "gram_tiles.h"

namespace dann {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTilePasses = kTileRowBlocks / 2;  // slab fill: 64 rows per pass

template <typename RT>
__device__ __forceinline__ float4 tile_load4(const uint8_t* p);  // 4 consecutive elements, widened exactly
template <>
__device__ __forceinline__ float4 tile_load4<float>(const uint8_t* p) {
    return *reinterpret_cast<const float4*>(p);
}
template <>
__device__ __forceinline__ float4 tile_load4<__half>(const uint8_t* p) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    const float2 a = __half22float2(__builtin_bit_cast(__half2, t.x)), b = __half22float2(__builtin_bit_cast(__half2, t.y));
    return float4{a.x, a.y, b.x, b.y};
}
template <typename RT>
__device__ __forceinline__ float4 tile_fetch4(const uint8_t* row, uint32_t k, uint32_t dim);
template <>
__device__ __forceinline__ float4 tile_fetch4<float>(const uint8_t* row, uint32_t k, uint32_t dim) {
    const float* r = reinterpret_cast<const float*>(row);
    float4 q = {0.f, 0.f, 0.f, 0.f};
    if (k + 3u < dim) {
        q = *reinterpret_cast<const float4*>(r + k);
    } else if (k < dim) {
        q.x = r[k];
        if (k + 1u < dim) q.y = r[k + 1u];
        if (k + 2u < dim) q.z = r[k + 2u];
    }
    return q;
}
template <>
__device__ __forceinline__ float4 tile_fetch4<__half>(const uint8_t* row, uint32_t k, uint32_t dim) {
    const __half* r = reinterpret_cast<const __half*>(row);
    float4 q = {0.f, 0.f, 0.f, 0.f};
    if (k + 3u < dim) {
        const uint2 t = *reinterpret_cast<const uint2*>(r + k);
        const float2 a = __half22float2(__builtin_bit_cast(__half2, t.x)), b = __half22float2(__builtin_bit_cast(__half2, t.y));
        q = {a.x, a.y, b.x, b.y};
    } else if (k < dim) {
        q.x = __half2float(r[k]);
        if (k + 1u < dim) q.y = __half2float(r[k + 1u]);
        if (k + 2u < dim) q.z = __half2float(r[k + 2u]);
    }
    return q;
}

// one 32-column slab of the NT tiles of a wave (tile t: row-block operand at ao[t], column-block operand at bo[t], float
// offsets into the slab).  The operands come from LDS in chunks of CK k-pairs, the next chunk requested before the MFMAs of
// the current one are issued.  The scheduling barriers pin that order: left to itself the compiler puts every read directly
// in front of its MFMAs (read, wait, two MFMAs, read, wait, ...), and all operands of a slab up front would be 96 registers.
template <int NT>
__device__ __forceinline__ void tile_slab(const float* lane_base, const uint32_t (&sa)[3], const uint32_t (&sb)[3],
                                          f32x16 (&acc)[NT]) {
    constexpr int CK = NT == 3 ? 2 : 4, NC = 16 / CK;
    float av[2][NT][CK], bv[2][NT][CK];
    // operand addresses: one per-lane base plus wave-uniform offsets (formed here, per slab: six address registers kept
    // across the loop are six registers too many next to 48 accumulators)
    const float* ao[NT];
    const float* bo[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        ao[t] = lane_base + sa[t];
        bo[t] = lane_base + sb[t];
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < CK; ++j) {
            av[0][t][j] = ao[t][2 * j];
            bv[0][t][j] = bo[t][2 * j];
        }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c + 1 < NC) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < CK; ++j) {
                    av[(c + 1) & 1][t][j] = ao[t][2 * (CK * (c + 1) + j)];
                    bv[(c + 1) & 1][t][j] = bo[t][2 * (CK * (c + 1) + j)];
                }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < CK; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c & 1][t][j], bv[c & 1][t][j], acc[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// MAXNT: the most tiles a wave of this launch can own (ceil(T / 8) for the launch's ng x mg).  Launches of short lists
// (back-edge lists: 96 rows, six tiles) are compiled without the 32- and 48-accumulator paths and fit three workgroups
// per CU instead of two.
template <typename RT, int MAXNT>
__global__ __launch_bounds__(512, MAXNT == 1 ? 6 : 4) void gram_tiles_kernel(TileArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // two slabs of 32 columns (rows x 33 floats each): slab k + 1 is written while the MFMAs of slab k are in the pipe --
    // one barrier per slab, and the only phase of a workgroup without MFMA work is the first fill
    const uint32_t slab_floats = tile_slab_rows(a.ng) * 33u;
    float* const slab0 = reinterpret_cast<float*>(smem);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, item = a.order ? a.order[blockIdx.x] : blockIdx.x;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));  // wave-uniform for the compiler too
    // Wave w sits on SIMD w % 4, and two workgroups share a CU: odd workgroups count their waves in reverse, so that the
    // waves with one tile more than the others are not on the same SIMDs in both.
    const uint32_t wv = (blockIdx.x & 1u) ? (uint32_t)(kTileRowBlocks - 1) - wave : wave;
    const uint32_t N = a.sn[item];
    const uint32_t nrows = N < a.ng ? N : a.ng, ncols = N < a.mg ? N : a.mg;
    if (nrows == 0) return;
    const uint32_t TR = (nrows + 31u) >> 5, TC = (ncols + 31u) >> 5;
    const uint32_t* ids = a.sid + (uint64_t)item * a.pcap;
    const uint32_t dim = a.ix.dim;
    // slab fill: 8 threads x 4 elements per row, 64 rows per pass.  Every request of the steady state is unconditional
    // (a load under a per-lane condition gets its own s_waitcnt and the prefetch degenerates to one request in flight):
    // rows that do not exist or cannot be retrieved point at row 0 and are zeroed when the slab is written.
    const uint32_t lr = tid >> 3, c4 = (tid & 7u) << 2;
    // (register diet: 48 accumulators + 16 prefetch registers leave little under the 128 of two workgroups per CU -- a
    // row is kept as its id, kEmpty for a zero row, and its address is formed at the request)
    uint32_t rowid[kTilePasses];
    double nsq[kTilePasses];
#pragma unroll
    for (int p = 0; p < kTilePasses; ++p) {
        const uint32_t r = ((uint32_t)p << 6) + lr;
        const uint32_t id = r < nrows ? ids[r] : kEmpty;
        rowid[p] = id < a.ix.nslots ? id : kEmpty;  // ids the sweep excludes anyway (not retrievable) read as zero rows
        nsq[p] = 0.0;
    }
    const uint8_t* const rows_c4 = a.ix.rows + (size_t)c4 * sizeof(RT);
    auto row_ptr = [&](int p) -> const uint8_t* {
        return rows_c4 + (uint64_t)(rowid[p] != kEmpty ? rowid[p] : 0u) * a.ix.row_stride;
    };
    float4 nxt[kTilePasses];
    const uint32_t dim_full = dim & ~31u;  // slabs below this are complete: one 4-element request per thread and row
    // The tiles of the item -- row block b has min(b, TC - 1) + 1 of them, column blocks 0 .. min(b, TC - 1) -- in row-major
    // order q = 0 .. T - 1; wave wv takes q = wv, wv + 8, wv + 16: at most one tile more than any other wave (a wave per
    // row block, as until round 4, leaves 1 + 2 + 3 + 3 + 3 tiles on five waves of a 160-row item: the SIMD with two of
    // them sets the pace of every slab).
    const uint32_t l31 = lane & 31u, hi = lane >> 5;
    uint32_t T = 0;
    for (uint32_t b = 0; b < TR; ++b) T += (b < TC ? b : TC - 1u) + 1u;
    const uint32_t nt = T > wv ? (T - wv + 7u) >> 3 : 0u;  // <= 3: T <= 21
    uint32_t trb[3] = {0, 0, 0}, tcb[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        uint32_t q = wv + 8u * (uint32_t)t, b = 0;
        if ((uint32_t)t < nt) {
            for (;;) {
                const uint32_t c = (b < TC ? b : TC - 1u) + 1u;
                if (q < c) break;
                q -= c;
                ++b;
            }
            trb[t] = b;
            tcb[t] = q;
        }
    }
    const float* const lane_base = slab0 + l31 * 33u + hi;
    const uint32_t fill_passes = (TR + 1u) >> 1;  // whole passes (wave-uniform): rows past the item's last are zero rows
    auto write_slab = [&](float* slab) {
#pragma unroll
        for (int p = 0; p < kTilePasses; ++p) {
            if ((uint32_t)p < fill_passes) {
                float4 q = nxt[p];
                if (rowid[p] == kEmpty) q = float4{0.f, 0.f, 0.f, 0.f};
                float* dst = slab + (((uint32_t)p << 6) + lr) * 33u + c4;
                dst[0] = q.x, dst[1] = q.y, dst[2] = q.z, dst[3] = q.w;
                nsq[p] += (double)q.x * q.x + (double)q.y * q.y + (double)q.z * q.z + (double)q.w * q.w;
            }
        }
    };
    float* const g = a.gram + (uint64_t)item * a.ng * a.mg;
    // The whole slab loop is instantiated per tile count of the wave (0 .. 3).  A branch on the count inside the loop makes
    // the accumulators a three-way merge in every iteration: the compiler then keeps two copies of all 48 of them (and
    // moves one into the other every slab), which is what drove this kernel into scratch until round 4.
    auto run = [&](auto ntc) {
        constexpr int NT = decltype(ntc)::value;
        f32x16 acc[NT > 0 ? NT : 1];
#pragma unroll
        for (int t = 0; t < (NT > 0 ? NT : 1); ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        uint32_t cur = 0;  // the slab the next MFMAs read: slab0 + cur * slab_floats
        if (dim_full) {
            // steady state: one basic block of requests per slab -- all kTilePasses of them, unconditionally (passes
            // beyond the item's rows re-read row 0 from cache): a request under a branch, even a uniform one, is fenced
            // by its own s_waitcnt.  The last iteration re-requests its own slab instead of branching around the prefetch.
#pragma unroll
            for (int p = 0; p < kTilePasses; ++p) nxt[p] = tile_load4<RT>(row_ptr(p));
            write_slab(slab0);
            __syncthreads();
            for (uint32_t k0 = 0; k0 < dim_full; k0 += 32u) {
                const bool more = k0 + 32u < dim_full;
                const uint32_t kn = more ? k0 + 32u : k0;
#pragma unroll
                for (int p = 0; p < kTilePasses; ++p) nxt[p] = tile_load4<RT>(row_ptr(p) + (size_t)kn * sizeof(RT));
                __builtin_amdgcn_sched_barrier(0);  // the requests go out before the MFMAs, not behind them
                if constexpr (NT > 0) {
                    const uint32_t so = cur * slab_floats;
                    const uint32_t sa[3] = {so + trb[0] * 1056u, so + trb[1] * 1056u, so + trb[2] * 1056u};
                    const uint32_t sb[3] = {so + tcb[0] * 1056u, so + tcb[1] * 1056u, so + tcb[2] * 1056u};
                    tile_slab<NT>(lane_base, sa, sb, acc);
                }
                cur ^= 1u;
                if (more) write_slab(slab0 + cur * slab_floats);  // nobody reads this one before the barrier
                __syncthreads();
            }
        }
        if (dim_full < dim) {  // the last, partial slab (dim % 32 != 0): element-wise requests, once per item
#pragma unroll
            for (int p = 0; p < kTilePasses; ++p)
                nxt[p] = tile_fetch4<RT>(row_ptr(p) - (size_t)c4 * sizeof(RT), dim_full + c4, dim);
            write_slab(slab0 + cur * slab_floats);  // every wave is past the barrier behind the last MFMAs
            __syncthreads();
            if constexpr (NT > 0) {
                const uint32_t so = cur * slab_floats;
                const uint32_t sa[3] = {so + trb[0] * 1056u, so + trb[1] * 1056u, so + trb[2] * 1056u};
                const uint32_t sb[3] = {so + tcb[0] * 1056u, so + tcb[1] * 1056u, so + tcb[2] * 1056u};
                tile_slab<NT>(lane_base, sa, sb, acc);
            }
        }
        // C layout of v_mfma_f32_32x32x2_f32: register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
        if constexpr (NT > 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t i = (trb[t] << 5) + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * hi;
                    g[(uint64_t)i * a.mg + (tcb[t] << 5) + l31] = acc[t][r];  // i < 32 TR <= ng, column < 32 TC <= mg
                }
            }
        }
    };
    if (MAXNT >= 3 && nt == 3u) run(std::integral_constant<int, 3>{});
    else if (MAXNT >= 2 && nt == 2u) run(std::integral_constant<int, 2>{});
    else if (nt >= 1u) run(std::integral_constant<int, 1>{});
    else run(std::integral_constant<int, 0>{});
    // squared norms: the 8 threads of a row hold f64 partial sums
    float* nr = a.nrm + (uint64_t)item * a.ng;
#pragma unroll
    for (int p = 0; p < kTilePasses; ++p) {
        double v = nsq[p];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        const uint32_t r = ((uint32_t)p << 6) + lr;
        if ((tid & 7u) == 0 && r < nrows) nr[r] = (float)v;
    }
    if (tid == 0 && a.counters) {
        atomicAdd(&stat_stripe(a.counters)[2], (unsigned long long)nrows);
        atomicAdd(&stat_stripe(a.counters)[3], (unsigned long long)T * 1024ull);
    }
}

// ---- f16 rows on the f16 matrix core (round 6) ---------------------------------------------------------------------------
// gram_tiles_kernel<__half> widens f16 rows and runs v_mfma_f32_32x32x2_f32 -- the f32 matrix core, 1/16 of the f16 rate,
// and 32 LDS operand reads per tile and 32-column slab.  Here the slabs hold the rows' halfs as they are (80-byte row
// stride: the 16-byte operand reads of 16 consecutive rows cover all 64 banks) and a tile advances 16 columns per
// v_mfma_f32_32x32x16_f16: lane l supplies row l & 31, halfs 8 (l >> 5) .. + 7 of the 16-column step, for BOTH operands, so
// whatever order the hardware walks those sixteen k in, row i's k meets row j's k (scratch/probe_mfma_f16.hip: exact on
// integer data, 1 - 9 u sum|x y| off the exact product on random rows of 16 .. 1536 columns -- a third of the f32 chain's
// error).  Products of two halfs are exact in f32; the sum is not the reference's FMA chain, and does not have to be: every
// decision of the sweep goes through the error interval E = c1 (|x|^2 + |y|^2) + c2 |d'| (c1 = the chain's bound, which
// covers any summation order of exactly rounded or truncated f32 additions with room to spare) and falls back to the
// bit-exact pair kernel where E does not decide.  Same tiling, same dealing of tiles to waves, same
// output as gram_tiles_kernel.
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
constexpr uint32_t kF16SlabRowBytes = 80;  // 32 halfs + 16 bytes: conflict-free 16-byte operand reads
template <int NT>
__device__ __forceinline__ void tile_slab_f16(const uint8_t* lane_base, const uint32_t (&sa)[3], const uint32_t (&sb)[3],
                                              f32x16 (&acc)[NT]) {
    f16x8_t av[NT][2], bv[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            av[t][m] = *reinterpret_cast<const f16x8_t*>(lane_base + sa[t] + 32u * m);
            bv[t][m] = *reinterpret_cast<const f16x8_t*>(lane_base + sb[t] + 32u * m);
        }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[t][m], bv[t][m], acc[t], 0, 0, 0);
}

template <int MAXNT>
__global__ __launch_bounds__(512, MAXNT == 1 ? 6 : 4) void gram_tiles_f16_kernel(TileArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t slab_bytes = tile_slab_rows(a.ng) * kF16SlabRowBytes;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, item = a.order ? a.order[blockIdx.x] : blockIdx.x;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t wv = (blockIdx.x & 1u) ? (uint32_t)(kTileRowBlocks - 1) - wave : wave;
    const uint32_t N = a.sn[item];
    const uint32_t nrows = N < a.ng ? N : a.ng, ncols = N < a.mg ? N : a.mg;
    if (nrows == 0) return;
    const uint32_t TR = (nrows + 31u) >> 5, TC = (ncols + 31u) >> 5;
    const uint32_t* ids = a.sid + (uint64_t)item * a.pcap;
    const uint32_t dim = a.ix.dim;
    // slab fill: 8 threads x 4 halfs per row, 64 rows per pass; unconditional requests (see gram_tiles_kernel)
    const uint32_t lr = tid >> 3, c4 = (tid & 7u) << 2;
    uint32_t rowid[kTilePasses];
    double nsq[kTilePasses];
#pragma unroll
    for (int p = 0; p < kTilePasses; ++p) {
        const uint32_t r = ((uint32_t)p << 6) + lr;
        const uint32_t id = r < nrows ? ids[r] : kEmpty;
        rowid[p] = id < a.ix.nslots ? id : kEmpty;
        nsq[p] = 0.0;
    }
    const uint8_t* const rows_c4 = a.ix.rows + (size_t)c4 * 2u;
    auto row_ptr = [&](int p) -> const uint8_t* {
        return rows_c4 + (uint64_t)(rowid[p] != kEmpty ? rowid[p] : 0u) * a.ix.row_stride;
    };
    uint2 nxt[kTilePasses];
    const uint32_t dim_full = dim & ~31u;
    const uint32_t l31 = lane & 31u, hi = lane >> 5;
    uint32_t T = 0;
    for (uint32_t b = 0; b < TR; ++b) T += (b < TC ? b : TC - 1u) + 1u;
    const uint32_t nt = T > wv ? (T - wv + 7u) >> 3 : 0u;
    uint32_t trb[3] = {0, 0, 0}, tcb[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        uint32_t q = wv + 8u * (uint32_t)t, b = 0;
        if ((uint32_t)t < nt) {
            for (;;) {
                const uint32_t c = (b < TC ? b : TC - 1u) + 1u;
                if (q < c) break;
                q -= c;
                ++b;
            }
            trb[t] = b;
            tcb[t] = q;
        }
    }
    const uint8_t* const lane_base = smem + l31 * kF16SlabRowBytes + hi * 16u;
    const uint32_t fill_passes = (TR + 1u) >> 1;
    auto write_slab = [&](uint8_t* slab) {
#pragma unroll
        for (int p = 0; p < kTilePasses; ++p) {
            if ((uint32_t)p < fill_passes) {
                uint2 q = nxt[p];
                if (rowid[p] == kEmpty) q = make_uint2(0u, 0u);
                *reinterpret_cast<uint2*>(slab + (((uint32_t)p << 6) + lr) * kF16SlabRowBytes + c4 * 2u) = q;
                const float2 x = __half22float2(__builtin_bit_cast(__half2, q.x)), y = __half22float2(__builtin_bit_cast(__half2, q.y));
                nsq[p] += (double)x.x * x.x + (double)x.y * x.y + (double)y.x * y.x + (double)y.y * y.y;
            }
        }
    };
    auto fetch_tail = [&](int p) -> uint2 {  // the partial slab: elements beyond the row's end read as zero
        const __half* r = reinterpret_cast<const __half*>(row_ptr(p) - (size_t)c4 * 2u);
        const uint32_t k = dim_full + c4;
        __half h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = (k + (uint32_t)e < dim) ? r[k + (uint32_t)e] : __float2half(0.0f);
        uint2 q;
        q.x = (uint32_t)__builtin_bit_cast(uint16_t, h[0]) | ((uint32_t)__builtin_bit_cast(uint16_t, h[1]) << 16);
        q.y = (uint32_t)__builtin_bit_cast(uint16_t, h[2]) | ((uint32_t)__builtin_bit_cast(uint16_t, h[3]) << 16);
        return q;
    };
    float* const g = a.gram + (uint64_t)item * a.ng * a.mg;
    auto run = [&](auto ntc) {
        constexpr int NT = decltype(ntc)::value;
        f32x16 acc[NT > 0 ? NT : 1];
#pragma unroll
        for (int t = 0; t < (NT > 0 ? NT : 1); ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        uint32_t cur = 0;
        constexpr uint32_t kBlock = 32u * kF16SlabRowBytes;  // bytes of one 32-row block of a slab
        if (dim_full) {
#pragma unroll
            for (int p = 0; p < kTilePasses; ++p) nxt[p] = *reinterpret_cast<const uint2*>(row_ptr(p));
            write_slab(smem);
            __syncthreads();
            for (uint32_t k0 = 0; k0 < dim_full; k0 += 32u) {
                const bool more = k0 + 32u < dim_full;
                const uint32_t kn = more ? k0 + 32u : k0;
#pragma unroll
                for (int p = 0; p < kTilePasses; ++p) nxt[p] = *reinterpret_cast<const uint2*>(row_ptr(p) + (size_t)kn * 2u);
                __builtin_amdgcn_sched_barrier(0);  // the requests go out before the MFMAs, not behind them
                if constexpr (NT > 0) {
                    const uint32_t so = cur * slab_bytes;
                    const uint32_t sa[3] = {so + trb[0] * kBlock, so + trb[1] * kBlock, so + trb[2] * kBlock};
                    const uint32_t sb[3] = {so + tcb[0] * kBlock, so + tcb[1] * kBlock, so + tcb[2] * kBlock};
                    tile_slab_f16<NT>(lane_base, sa, sb, acc);
                }
                cur ^= 1u;
                if (more) write_slab(smem + cur * slab_bytes);
                __syncthreads();
            }
        }
        if (dim_full < dim) {
#pragma unroll
            for (int p = 0; p < kTilePasses; ++p) nxt[p] = fetch_tail(p);
            write_slab(smem + cur * slab_bytes);
            __syncthreads();
            if constexpr (NT > 0) {
                const uint32_t so = cur * slab_bytes;
                const uint32_t sa[3] = {so + trb[0] * kBlock, so + trb[1] * kBlock, so + trb[2] * kBlock};
                const uint32_t sb[3] = {so + tcb[0] * kBlock, so + tcb[1] * kBlock, so + tcb[2] * kBlock};
                tile_slab_f16<NT>(lane_base, sa, sb, acc);
            }
        }
        // C layout as v_mfma_f32_32x32x2_f32: register r of lane l holds row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
        if constexpr (NT > 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t i = (trb[t] << 5) + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * hi;
                    g[(uint64_t)i * a.mg + (tcb[t] << 5) + l31] = acc[t][r];
                }
            }
        }
    };
    if (MAXNT >= 3 && nt == 3u) run(std::integral_constant<int, 3>{});
    else if (MAXNT >= 2 && nt == 2u) run(std::integral_constant<int, 2>{});
    else if (nt >= 1u) run(std::integral_constant<int, 1>{});
    else run(std::integral_constant<int, 0>{});
    float* nr = a.nrm + (uint64_t)item * a.ng;
#pragma unroll
    for (int p = 0; p < kTilePasses; ++p) {
        double v = nsq[p];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        const uint32_t r = ((uint32_t)p << 6) + lr;
        if ((tid & 7u) == 0 && r < nrows) nr[r] = (float)v;
    }
    if (tid == 0 && a.counters) {
        atomicAdd(&stat_stripe(a.counters)[2], (unsigned long long)nrows);
        atomicAdd(&stat_stripe(a.counters)[3], (unsigned long long)T * 1024ull);
    }
}

// Longest lists first: a sweep is a serial walk over its list, and a launch in item order ends with a few long lists on an
// otherwise idle chip (1 M x 768, 16 384 pools per launch: 6 of 13 wavefront slots per CU occupied on average).  The
// workgroups of the Gram and sweep kernels take their items in descending order of list length instead -- a counting
// sort by length, one workgroup (the order among equal lengths is whatever the atomics give: no result depends on it).
constexpr uint32_t kOrderBins = kMaxPool + 1u;
__global__ __launch_bounds__(1024) void lpt_order_kernel(const uint32_t* sn, uint32_t m, uint32_t* order) {
    __shared__ uint32_t hist[kOrderBins];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kOrderBins; i += 1024u) hist[i] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < m; i += 1024u) atomicAdd(&hist[sn[i] < kMaxPool ? sn[i] : kMaxPool], 1u);
    __syncthreads();
    if (tid < 64u) {  // exclusive scan from the longest bin down: 64 bins per step
        uint32_t acc = 0;
        for (int base = (int)kOrderBins - 1; base >= 0; base -= 64) {
            const int b = base - (int)tid;
            const uint32_t c = b >= 0 ? hist[b] : 0u;
            uint32_t inc = c;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(inc, o);
                if ((int)tid >= o) inc += t;
            }
            if (b >= 0) hist[b] = acc + inc - c;
            acc += __shfl(inc, 63);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < m; i += 1024u) order[atomicAdd(&hist[sn[i] < kMaxPool ? sn[i] : kMaxPool], 1u)] = i;
}

}  // namespace

// f16_mfma: f16 rows through v_mfma_f32_32x32x16_f16 (gram_tiles_f16_kernel; the default) instead of widened through the
// f32 matrix core (DANN_DBG_GRAM_F16_WIDEN: the round-3 form, whose entries are the reference's FMA chain bit for bit)
int32_t launch_gram_tiles(const TileArgs& a, uint32_t grid, hipStream_t stream, bool f16_mfma) {
    if (a.ix.dtype != DT_F32 && a.ix.dtype != DT_F16) return DANN_EUNSUPPORTED;
    const bool f32 = a.ix.dtype == DT_F32;
    const bool h16 = !f32 && f16_mfma;
    const size_t lds = h16 ? 2u * (size_t)tile_slab_rows(a.ng) * kF16SlabRowBytes
                           : 2u * (size_t)tile_slab_rows(a.ng) * 33u * 4u;  // two slabs
    // the most tiles a wave of this launch can own: T tiles of a full item over eight waves
    const uint32_t tr = a.ng >> 5, tc = a.mg >> 5;
    uint32_t tmax = 0;
    for (uint32_t b2 = 0; b2 < tr; ++b2) tmax += (b2 < tc ? b2 : tc - 1u) + 1u;
    const bool narrow = tmax <= 8u;
    const auto go = [&](auto kernel) {
        return launch_kernel<decltype(kernel)::fn>("gram_tiles_kernel launch", dim3(grid), dim3(512), lds, stream, a);
    };
    if (h16) return narrow ? go(KernelOf<gram_tiles_f16_kernel<1>>{}) : go(KernelOf<gram_tiles_f16_kernel<3>>{});
    if (f32) return narrow ? go(KernelOf<gram_tiles_kernel<float, 1>>{}) : go(KernelOf<gram_tiles_kernel<float, 3>>{});
    return narrow ? go(KernelOf<gram_tiles_kernel<__half, 1>>{}) : go(KernelOf<gram_tiles_kernel<__half, 3>>{});
}

void launch_lpt_order(const uint32_t* sn, uint32_t m, uint32_t* order, hipStream_t stream) {
    hipLaunchKernelGGL(lpt_order_kernel, dim3(1), dim3(1024), 0, stream, sn, m, order);
}

}  // namespace dann

using namespace dann;

extern "C" int32_t dann_debug_gram_tiles(int32_t device, int32_t dtype, const void* rows, uint32_t n, uint32_t dim, uint32_t mg,
                                         float* out_gram, float* out_nrm) try {
    const bool widen = (dtype & 0x100) != 0;  // DANN_F16 | 0x100: f16 rows widened through the f32 matrix core
    dtype &= 0xFF;
    if (!rows || !out_gram || !out_nrm || n == 0 || n > 32u * kTileRowBlocks || dim == 0 || (dtype != DT_F32 && dtype != DT_F16))
        return DANN_EINVAL;
    mg = clamp_gram_cols(mg);
    DeviceGuard guard(device < 0 ? 0 : device);
    const size_t esz = dtype == DT_F32 ? 4 : 2;
    const size_t stride = ((size_t)dim * esz + 15) & ~(size_t)15;
    const uint32_t ng = (n + 31u) & ~31u;
    DevBuf dr, dids, dsn, dg, dn;
    DANN_HIP(dr.alloc(stride * n + 256));
    DANN_HIP(dids.alloc((size_t)ng * 4));
    DANN_HIP(dsn.alloc(4));
    DANN_HIP(dg.alloc((size_t)ng * mg * 4));
    DANN_HIP(dn.alloc((size_t)ng * 4));
    DANN_HIP(hipMemset(dr.p, 0, stride * n + 256));
    DANN_HIP(hipMemset(dg.p, 0, (size_t)ng * mg * 4));
    DANN_HIP(hipMemset(dn.p, 0, (size_t)ng * 4));
    DANN_HIP(hipMemcpy2D(dr.p, stride, rows, (size_t)dim * esz, (size_t)dim * esz, n, hipMemcpyHostToDevice));
    std::vector<uint32_t> ids(ng);
    for (uint32_t i = 0; i < ng; ++i) ids[i] = i;
    DANN_HIP(hipMemcpy(dids.p, ids.data(), (size_t)ng * 4, hipMemcpyHostToDevice));
    DANN_HIP(hipMemcpy(dsn.p, &n, 4, hipMemcpyHostToDevice));
    TileArgs ta{};
    ta.ix.rows = dr.as<uint8_t>();
    ta.ix.row_stride = stride;
    ta.ix.dim = dim;
    ta.ix.dtype = dtype;
    ta.ix.nslots = n;
    ta.sid = dids.as<uint32_t>();
    ta.sn = dsn.as<uint32_t>();
    ta.pcap = ng;
    ta.ng = ng;
    ta.mg = std::min(mg, ng);
    ta.gram = dg.as<float>();
    ta.nrm = dn.as<float>();
    ta.counters = nullptr;
    int32_t rc = launch_gram_tiles(ta, 1, 0, !widen);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipDeviceSynchronize());
    // out_gram: n x mg (row stride mg as passed, entries beyond the computed block are zero)
    std::vector<float> g((size_t)ng * ta.mg);
    DANN_HIP(hipMemcpy(g.data(), dg.p, g.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < mg; ++j) out_gram[(size_t)i * mg + j] = j < ta.mg ? g[(size_t)i * ta.mg + j] : 0.0f;
    DANN_HIP(hipMemcpy(out_nrm, dn.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return DANN_OK;
} DANN_CATCH_ALL
