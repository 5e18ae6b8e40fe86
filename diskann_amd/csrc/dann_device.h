// dann_device.h -- CDNA4 (gfx950) device primitives for the DiskANN hot path.
//
// The distance functions reproduce, bit for bit, the association order of the
// reference's x86-64-v3 kernels (diskann-vector/src/distance/simd.rs:321-483 main-loop
// strategies, :686-747 simd_op, diskann-wide/src/arch/x86_64/v3/f32x8_.rs:185-212
// sum_tree), because the returned neighbour ids must equal the CPU path's at fixed L
// and near-ties in the L-queue are decided by the last ulp.
//
// Mapping onto a 64-wide wavefront.  The CPU keeps NACC accumulators of 8 f32 lanes; element
// e of a vector is accumulated (one FMA per visit, increasing e) into "chain"
// c = e mod (8*NACC).  A chain is a strictly sequential FMA sequence, so a whole chain must
// live in one GPU lane.  We give every candidate row a group of G = 2*NACC adjacent lanes;
// lane v of the group owns chains 4v..4v+3, i.e. per "trip" of 8*NACC elements it loads the
// 4 consecutive elements [trip + 4v, trip + 4v + 4) -- one 16-byte load for f32 rows,
// one 8-byte load for f16 rows -- so a group reads 128 (64) contiguous bytes per
// instruction and a wavefront reads 64/G rows at once.  The accumulator combine
// `(s0+s1)+(s2+s3)` and the 8-lane horizontal tree are three DPP adds plus three in-lane
// adds.  The result is valid in lane v == 0 of each group.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "row_types.h"  // DT_* / M_* / OP_*, dt_is_*, resolve_metric, kEmpty

namespace dann {

__host__ __device__ constexpr int sq_bits(int dt) {
    return dt == DT_SQ8 ? 8 : dt_is_sph(dt) ? (dt & 7) : dt_is_mm(dt) ? dt - 48 : dt_is_mmq(dt) ? dt - 112 : dt - 16;  // (DT_MM*Q: the rows' bits)
}
// query layouts of spherical rows (iface::QueryLayout; dann.h DANN_QUERY_*)
enum : int { QL_SAME = 0, QL_TRANSPOSED = 1, QL_SCALAR = 2, QL_FULL = 3, QL_EIGHT_BIT = 8 };
constexpr uint32_t kSphDataMeta = 6u, kSphQueryMeta = 16u;  // bytes of DataMeta / QueryMeta
// code bytes of a scalar- or spherically quantised row: ceil(dim * bits / 8); the f32 compensation resp. the DataMeta
// follows them
__host__ __device__ constexpr uint32_t sq_code_bytes(int dt, uint32_t dim) {
    return (uint32_t)(((uint64_t)dim * (uint32_t)sq_bits(dt) + 7u) >> 3);
}
constexpr uint32_t kVisitedBit = 0x80000000u;

// DPP controls (cdna4 ISA: quad_perm = 0x00-0xFF, row_shl:n = 0x100+n)
constexpr int DPP_XOR1 = 0xB1;   // quad_perm:[1,0,3,2]
constexpr int DPP_XOR2 = 0x4E;   // quad_perm:[2,3,0,1]
constexpr int DPP_SHL4 = 0x104;  // lane i <- lane i+4 (within a row of 16)

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __builtin_bit_cast(float,
                              __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true);
}

__device__ __forceinline__ uint64_t ballot64(bool p) { return __ballot(p); }
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
// number of set bits of `m` strictly below this lane
__device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// ---- element loads: 4 consecutive elements as f32 -----------------------------------
struct F4 {
    float x, y, z, w;
};
__device__ __forceinline__ F4 load4(const float* p) {
    float4 t = *reinterpret_cast<const float4*>(p);
    return {t.x, t.y, t.z, t.w};
}
__device__ __forceinline__ F4 load4(const __half* p) {
    // exact widening (v_cvt_f32_f16), as `half` -> f32 on the CPU
    uint2 t = *reinterpret_cast<const uint2*>(p);
    __half2 a = __builtin_bit_cast(__half2, t.x), b = __builtin_bit_cast(__half2, t.y);
    float2 fa = __half22float2(a), fb = __half22float2(b);
    return {fa.x, fa.y, fb.x, fb.y};
}
__device__ __forceinline__ float load1(const float* p) { return *p; }
__device__ __forceinline__ float load1(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(__half x) { return __half2float(x); }


// Raw (unconverted) loads: converting inside a predicated block makes hipcc wait for each load
// before issuing the next (measured: 16 serialized round trips per f16 gather), so the loaders
// below only move bits; conversion happens in the compute phase.
template <typename RT>
struct Raw4;
template <>
struct Raw4<float> {
    float4 v;
    __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
    __device__ __forceinline__ F4 get() const { return {v.x, v.y, v.z, v.w}; }
};
template <>
struct Raw4<__half> {
    uint2 v;
    __device__ __forceinline__ void load(const __half* p) { v = *reinterpret_cast<const uint2*>(p); }
    __device__ __forceinline__ F4 get() const {
        float2 a = __half22float2(__builtin_bit_cast(__half2, v.x)), b = __half22float2(__builtin_bit_cast(__half2, v.y));
        return {a.x, a.y, b.x, b.y};
    }
};

// FullCosineAccumulator::sum (simd.rs:2329-2362)
__device__ __forceinline__ float cosine_finish(float normx, float normy, float prod) {
    // NB: __fsqrt_rn is NOT correctly rounded on ROCm 7.2 (15 % of inputs off by 1 ulp on gfx950);
    // __builtin_sqrtf and operator/ are (measured exhaustively in scratch probes).
    float denominator = __builtin_sqrtf(normx) * __builtin_sqrtf(normy);
    if (normx < 1.17549435e-38f || normy < 1.17549435e-38f) return 0.0f;
    float v = prod / denominator;
    float m = (v != v) ? 1.0f : (v < 1.0f ? v : 1.0f);
    return m > -1.0f ? m : -1.0f;
}

// PostOp (diskann-vector/src/distance/implementations.rs:215-401)
template <int OP, bool NORMALIZED>
__device__ __forceinline__ float post_op(float raw) {
    if (OP == OP_L2) return raw;
    if (OP == OP_IP) return NORMALIZED ? 1.0f - raw : -raw;
    return 1.0f - raw;
}

// One FMA step of a schema (simd.rs L2 :817-845, IP :1588-1616, cosine :2296-2305)
template <int OP>
struct FAcc {
    float s[4], nx[4], ny[4];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = nx[i] = ny[i] = 0.0f;
    }
    // element pairs as 2-vectors: v_pk_add_f32 / v_pk_fma_f32 (one IEEE subtract / fused multiply-add per element,
    // the same results as the scalar instructions, half as many of them)
    typedef float v2f __attribute__((ext_vector_type(2)));
    __device__ __forceinline__ void step(const F4& x, const F4& y) {
        const v2f xv[2] = {{x.x, x.y}, {x.z, x.w}}, yv[2] = {{y.x, y.y}, {y.z, y.w}};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            v2f sv = {s[2 * h], s[2 * h + 1]};
            if (OP == OP_L2) {
                const v2f c = xv[h] - yv[h];
                sv = __builtin_elementwise_fma(c, c, sv);
            } else if (OP == OP_IP) {
                sv = __builtin_elementwise_fma(xv[h], yv[h], sv);
            } else {
                v2f nxv = {nx[2 * h], nx[2 * h + 1]}, nyv = {ny[2 * h], ny[2 * h + 1]};
                nxv = __builtin_elementwise_fma(xv[h], xv[h], nxv);
                nyv = __builtin_elementwise_fma(yv[h], yv[h], nyv);
                sv = __builtin_elementwise_fma(xv[h], yv[h], sv);
                nx[2 * h] = nxv.x; nx[2 * h + 1] = nxv.y;
                ny[2 * h] = nyv.x; ny[2 * h + 1] = nyv.y;
            }
            s[2 * h] = sv.x; s[2 * h + 1] = sv.y;
        }
    }
};

// accumulator combine across the group + partial block + horizontal tree for one f32x8
// logical vector held as 4 floats in each of G lanes.  Returns the sum (valid in lane v==0).
template <int NACC, class PartialFn>
__device__ __forceinline__ float finish_vec(float (&a)[4], PartialFn&& partial) {
    // (s0+s1) [+ (s2+s3)]: lane v holds accumulator v/2, vector lanes 4*(v&1)+i
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = a[i] + dpp_f<DPP_XOR2>(a[i]);
    if (NACC == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = a[i] + dpp_f<DPP_SHL4>(a[i]);
    }
    partial(a);
    // sum_tree: ((x0+x4)+(x2+x6)) + ((x1+x5)+(x3+x7)); lane even holds x0..3, odd x4..7
    float q0 = a[0] + dpp_f<DPP_XOR1>(a[0]);
    float q1 = a[1] + dpp_f<DPP_XOR1>(a[1]);
    float q2 = a[2] + dpp_f<DPP_XOR1>(a[2]);
    float q3 = a[3] + dpp_f<DPP_XOR1>(a[3]);
    return (q0 + q2) + (q1 + q3);
}

// Distance between `q` (QT elements, any address space) and `row` (RT elements), both of
// length `dim`, computed by a group of G = 2*NACC lanes; `v` = lane index inside the group.
// DIM > 0 fixes the length at compile time (fully unrolled, all loads issued up front).
template <int NACC, int OP, int DIM, typename QT, typename RT>
__device__ __forceinline__ float group_distance_raw(const QT* __restrict__ q, const RT* __restrict__ row, int dim,
                                                    int v) {
    constexpr int G = 2 * NACC, TRIP = 4 * G;
    if (DIM > 0) dim = DIM;
    const int full_end = dim & ~7;
    FAcc<OP> acc;
    acc.init();
    if constexpr (DIM > 0) {
        constexpr int NT = (DIM / 8 * 8 + TRIP - 1) / TRIP;
        F4 ys[NT], xs[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int e = t * TRIP + 4 * v;
            if (e < full_end) ys[t] = load4(row + e);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int e = t * TRIP + 4 * v;
            if (e < full_end) xs[t] = load4(q + e);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int e = t * TRIP + 4 * v;
            if (e < full_end) acc.step(xs[t], ys[t]);
        }
    } else {
        for (int e = 4 * v; e < full_end; e += TRIP) {
            F4 y = load4(row + e);
            F4 x = load4(q + e);
            acc.step(x, y);
        }
    }
    const int rem = dim & 7;
    RT ty[4];
    if (rem) {  // all four requests issued together (index clamped into the block)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int l = 4 * (v & 1) + i;
            ty[i] = row[full_end + (l < rem ? l : 0)];
        }
    }
    // partial block: zero-padded masked load accumulated into the *combined* vector
    // (simd.rs:735-745, SIMDSchema::epilogue :545-563)
    auto partial = [&](float(&a)[4], int which) {
        if (rem == 0) return;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int l = 4 * (v & 1) + i;
            float x = 0.0f, y = 0.0f;
            if (l < rem) {
                x = load1(q + full_end + l);
                y = to_f32(ty[i]);
            }
            if (OP == OP_L2) {
                float c = x - y;
                a[i] = __builtin_fmaf(c, c, a[i]);
            } else if (which == 0) {
                a[i] = __builtin_fmaf(x, y, a[i]);
            } else if (which == 1) {
                a[i] = __builtin_fmaf(x, x, a[i]);
            } else {
                a[i] = __builtin_fmaf(y, y, a[i]);
            }
        }
    };
    float s = finish_vec<NACC>(acc.s, [&](float(&a)[4]) { partial(a, 0); });
    if (OP == OP_COS) {
        float nx = finish_vec<NACC>(acc.nx, [&](float(&a)[4]) { partial(a, 1); });
        float ny = finish_vec<NACC>(acc.ny, [&](float(&a)[4]) { partial(a, 2); });
        return cosine_finish(nx, ny, s);
    }
    return s;
}


// Stored row x stored row (RobustPrune's primitive) with every load of a T-trip window -- both rows -- issued
// before the first FMA.  group_distance_raw's run-time loop waits for each trip's loads before issuing the next
// trip's: four dependent round trips per 128-d distance, which is what the lazy prune scan then spends its time on.
// Same arithmetic, element order and partial-block rule as group_distance_raw.
template <int NACC, int OP, typename RT>
__device__ __forceinline__ float group_distance_pair(const RT* __restrict__ x, const RT* __restrict__ y, int dim, int v) {
    constexpr int G = 2 * NACC, TRIP = 4 * G;
    const int full_end = dim & ~7, rem = dim & 7;
    FAcc<OP> acc;
    acc.init();
    RT tx[4], ty[4];
    if (rem) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int l = 4 * (v & 1) + i, lc = l < rem ? l : 0;  // clamped, unconditional: no branch, no wait
            tx[i] = x[full_end + lc];
            ty[i] = y[full_end + lc];
        }
    }
    constexpr int T = 4;
    for (int e0 = 4 * v; e0 < full_end; e0 += TRIP * T) {
        Raw4<RT> xs[T], ys[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int e = e0 + t * TRIP;
            if (e < full_end) {
                xs[t].load(x + e);
                ys[t].load(y + e);
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int e = e0 + t * TRIP;
            if (e < full_end) acc.step(xs[t].get(), ys[t].get());
        }
    }
    auto partial = [&](float(&a)[4], int which) {
        if (rem == 0) return;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int l = 4 * (v & 1) + i;
            float xv = 0.0f, yv = 0.0f;
            if (l < rem) {
                xv = to_f32(tx[i]);
                yv = to_f32(ty[i]);
            }
            if (OP == OP_L2) {
                const float c = xv - yv;
                a[i] = __builtin_fmaf(c, c, a[i]);
            } else if (which == 0) {
                a[i] = __builtin_fmaf(xv, yv, a[i]);
            } else if (which == 1) {
                a[i] = __builtin_fmaf(xv, xv, a[i]);
            } else {
                a[i] = __builtin_fmaf(yv, yv, a[i]);
            }
        }
    };
    float s = finish_vec<NACC>(acc.s, [&](float(&a)[4]) { partial(a, 0); });
    if (OP == OP_COS) {
        float nx = finish_vec<NACC>(acc.nx, [&](float(&a)[4]) { partial(a, 1); });
        float ny = finish_vec<NACC>(acc.ny, [&](float(&a)[4]) { partial(a, 2); });
        return cosine_finish(nx, ny, s);
    }
    return s;
}


// Fixed-length variant with the query slice of this lane preloaded in registers
// (DIM % (8*NACC) == 0, so there is neither an epilogue block nor a partial block).
// `U` rows are processed together: all U*NT row loads are issued before the first FMA so
// one lane keeps U*NT 16-byte requests in flight.
template <int NACC, int OP, int DIM, int U, typename RT>
__device__ __forceinline__ void group_distance_pre(const F4 (&xs)[DIM / (8 * NACC)], const RT* const (&rows)[U],
                                                   const bool (&active)[U], int v, float (&out)[U]) {
    constexpr int G = 2 * NACC, TRIP = 4 * G, NT = DIM / TRIP;
    Raw4<RT> ys[U][NT];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int t = 0; t < NT; ++t) ys[u][t].load(rows[u] + t * TRIP + 4 * v);  // unconditional (see group_distance_many)
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        FAcc<OP> acc;
        acc.init();
#pragma unroll
        for (int t = 0; t < NT; ++t) acc.step(xs[t], ys[u][t].get());
        float s = finish_vec<NACC>(acc.s, [](float(&)[4]) {});
        if (OP == OP_COS) {
            float nx = finish_vec<NACC>(acc.nx, [](float(&)[4]) {});
            float ny = finish_vec<NACC>(acc.ny, [](float(&)[4]) {});
            s = cosine_finish(nx, ny, s);
        }
        out[u] = s;
    }
}


// finish_vec<4> without a partial block, for group_distance_passes: the same adds, in the same order and with the same
// left and right operands.  What differs is the instruction they become.  Left to itself the compiler packs these adds
// in pairs (v_pk_add_f32), a packed add takes no DPP operand, and every shuffled operand then costs a v_mov_b32_dpp of
// its own: 20 instructions a row.  `lone` hands a sum to the compiler as a value it knows nothing about, so the adds
// stay single, each takes its DPP operand itself (v_add_f32_dpp), and a row costs 15.  An IEEE add gives the same bits
// packed or not.
__device__ __forceinline__ float lone(float x) {
    asm("" : "+v"(x));
    return x;
}
__device__ __forceinline__ float finish_vec4_dpp(float (&a)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = lone(a[i] + dpp_f<DPP_XOR2>(a[i]));
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = lone(a[i] + dpp_f<DPP_SHL4>(a[i]));
    const float q0 = lone(a[0] + dpp_f<DPP_XOR1>(a[0]));
    const float q1 = lone(a[1] + dpp_f<DPP_XOR1>(a[1]));
    const float q2 = lone(a[2] + dpp_f<DPP_XOR1>(a[2]));
    const float q3 = lone(a[3] + dpp_f<DPP_XOR1>(a[3]));
    return lone(q0 + q2) + lone(q1 + q3);
}

// group_distance_pre for NP passes of the plain float hop's gather (search_plain_impl.h), NACC = 4, L2 or inner product:
// all NP * NT row loads are issued before the first FMA, then the NP distances are computed with finish_vec4_dpp.  The
// arithmetic, its order and the results are group_distance_pre's.
template <int OP, int DIM, int NP, typename RT>
__device__ __forceinline__ void group_distance_passes(const F4 (&xs)[DIM / 32], const RT* const (&rows)[NP], int v,
                                                      float (&out)[NP]) {
    static_assert(OP != OP_COS, "one accumulator set per row");
    constexpr int TRIP = 32, NT = DIM / TRIP;
    Raw4<RT> ys[NP][NT];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
#pragma unroll
        for (int t = 0; t < NT; ++t) ys[u][t].load(rows[u] + t * TRIP + 4 * v);  // unconditional, as group_distance_pre's
    }
    // (nothing moves across this line: with the rows' addresses formed inside the body the scheduler otherwise starts on
    // the first row's arithmetic, and so waits for its loads, before it has issued the next row's)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        FAcc<OP> acc;
        acc.init();
#pragma unroll
        for (int t = 0; t < NT; ++t) acc.step(xs[t], ys[u][t].get());
        out[u] = finish_vec4_dpp(acc.s);
    }
}


// U rows at once with run-time length: per trip the U row loads are issued together, so a lane
// keeps U (x unroll) requests in flight instead of one.  Same arithmetic as group_distance_raw.
template <int NACC, int OP, int U, typename QT, typename RT>
__device__ __forceinline__ void group_distance_multi(const QT* __restrict__ q, const RT* const (&rows)[U],
                                                     const bool (&active)[U], int dim, int v, float (&out)[U]) {
    constexpr int G = 2 * NACC, TRIP = 4 * G;
    const int full_end = dim & ~7;
    const int rem = dim & 7;
    FAcc<OP> acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u].init();
    // the partial block's elements (dim % 8 != 0) are requested first, raw, so they travel with the main
    // loads instead of costing a second dependent round trip after them (dim = 100: 2.4x)
    RT ty[U][4];
    if (rem) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int l = 4 * (v & 1) + i;
#pragma unroll
            for (int u = 0; u < U; ++u) ty[u][i] = rows[u][full_end + (l < rem ? l : 0)];  // unconditional: no branch, no wait
        }
    }
    // T trips of loads are issued before the first FMA: U*T 16-byte requests in flight per lane
    constexpr int T = 4;
    for (int e0 = 4 * v; e0 < full_end; e0 += TRIP * T) {
        Raw4<RT> ys[T][U];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int e = e0 + t * TRIP;
            const int el = e < full_end ? e : e0;  // clamped: every request is issued, none behind a branch
#pragma unroll
            for (int u = 0; u < U; ++u) ys[t][u].load(rows[u] + el);
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int e = e0 + t * TRIP;
            if (e < full_end) {
                const F4 x = load4(q + e);
#pragma unroll
                for (int u = 0; u < U; ++u) acc[u].step(x, ys[t][u].get());  // inactive rows: computed, discarded
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool act = active[u];
        auto partial = [&](float(&a)[4], int which) {
            if (rem == 0 || !act) return;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int l = 4 * (v & 1) + i;
                float x = 0.0f, y = 0.0f;
                if (l < rem) {
                    x = load1(q + full_end + l);
                    y = to_f32(ty[u][i]);
                }
                if (OP == OP_L2) {
                    float c = x - y;
                    a[i] = __builtin_fmaf(c, c, a[i]);
                } else if (which == 0) {
                    a[i] = __builtin_fmaf(x, y, a[i]);
                } else if (which == 1) {
                    a[i] = __builtin_fmaf(x, x, a[i]);
                } else {
                    a[i] = __builtin_fmaf(y, y, a[i]);
                }
            }
        };
        float s = finish_vec<NACC>(acc[u].s, [&](float(&a)[4]) { partial(a, 0); });
        if (OP == OP_COS) {
            float nx = finish_vec<NACC>(acc[u].nx, [&](float(&a)[4]) { partial(a, 1); });
            float ny = finish_vec<NACC>(acc[u].ny, [&](float(&a)[4]) { partial(a, 2); });
            s = cosine_finish(nx, ny, s);
        }
        out[u] = s;
    }
}


// ---- "wide" layout for 2-byte rows: one lane owns a whole 8-lane accumulator --------------------
// With f16 rows a 4-element slice is only 8 bytes; giving each lane 8 consecutive elements
// (one 16-byte load) and one CPU accumulator (lane w of a group of NACC lanes == accumulator w)
// halves the instructions per byte.  Chains stay in-lane, so the association order is unchanged:
// combine (s0+s1)+(s2+s3) across lanes (two DPP adds), partial block, sum_tree in-lane.
struct F8v {
    float e[8];
};
__device__ __forceinline__ F8v load8(const float* p) {
    float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    return {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ F8v load8(const __half* p) {
    uint4 t = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
    F8v r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float2 f = __half22float2(__builtin_bit_cast(__half2, w[i]));
        r.e[2 * i] = f.x;
        r.e[2 * i + 1] = f.y;
    }
    return r;
}
template <typename RT>
__device__ __forceinline__ F8v cvt8(const uint4& t);
template <>
__device__ __forceinline__ F8v cvt8<__half>(const uint4& t) {
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
    F8v r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float2 f = __half22float2(__builtin_bit_cast(__half2, w[i]));
        r.e[2 * i] = f.x;
        r.e[2 * i + 1] = f.y;
    }
    return r;
}
template <int NACC>
__device__ __forceinline__ float finish_wide(float (&a)[8], const float (&px)[8], const float (&py)[8], int rem,
                                             int op_kind /*0 L2, 1 xy, 2 xx, 3 yy*/) {
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = a[i] + dpp_f<DPP_XOR1>(a[i]);
    if (NACC == 4) {
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = a[i] + dpp_f<DPP_XOR2>(a[i]);
    }
    if (rem) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float x = px[i], y = py[i];  // zero beyond `rem`
            if (op_kind == 0) {
                const float c = x - y;
                a[i] = __builtin_fmaf(c, c, a[i]);
            } else if (op_kind == 1) {
                a[i] = __builtin_fmaf(x, y, a[i]);
            } else if (op_kind == 2) {
                a[i] = __builtin_fmaf(x, x, a[i]);
            } else {
                a[i] = __builtin_fmaf(y, y, a[i]);
            }
        }
    }
    return ((a[0] + a[4]) + (a[2] + a[6])) + ((a[1] + a[5]) + (a[3] + a[7]));
}

#ifndef DANN_WIDE_TRIPS
#define DANN_WIDE_TRIPS 4
#endif
constexpr int kWideTrips = DANN_WIDE_TRIPS;
template <int NACC, int OP, int U, typename QT, typename RT>
__device__ __forceinline__ void group_distance_wide(const QT* __restrict__ q, const RT* const (&rows)[U],
                                                    const bool (&active)[U], int dim, int w, float (&out)[U]) {
    constexpr int TRIP = 8 * NACC;
    const int full_end = dim & ~7;
    float s[U][8], nx[U][8], ny[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) s[u][i] = nx[u][i] = ny[u][i] = 0.0f;
    // the partial block (dim % 8 != 0) is requested first, unconditionally (index clamped into the block), so
    // it travels with the main loads instead of costing `rem` dependent round trips after them
    const int rem = dim & 7;
    RT ry[U][8];
    if (rem) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int i = 0; i < 8; ++i) ry[u][i] = rows[u][full_end + (i < rem ? i : 0)];
    }
    constexpr int T = kWideTrips;
    for (int e0 = 8 * w; e0 < full_end; e0 += TRIP * T) {
        // All T*U 16-byte requests of a trip are issued back to back, unconditionally: a load under a per-lane
        // condition is compiled as a branch with its own s_waitcnt vmcnt(0), which leaves ONE request in
        // flight per wave (measured: 1 M x 768 f16 at 3.65 TB/s, the same time as the f32 rows).  Out-of-range
        // trips re-read the trip's first block and inactive rows point at row 0 (the caller's contract), so
        // every address is valid; their values are never used.
        uint4 raw[T][U];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int e = e0 + t * TRIP;
            const int el = e < full_end ? e : e0;
#pragma unroll
            for (int u = 0; u < U; ++u) raw[t][u] = *reinterpret_cast<const uint4*>(rows[u] + el);
        }
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int e = e0 + t * TRIP;
            if (e >= full_end) continue;
            const F8v x = load8(q + e);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const F8v y = cvt8<RT>(raw[t][u]);  // inactive rows: computed and discarded
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (OP == OP_L2) {
                        const float c = x.e[i] - y.e[i];
                        s[u][i] = __builtin_fmaf(c, c, s[u][i]);
                    } else if (OP == OP_IP) {
                        s[u][i] = __builtin_fmaf(x.e[i], y.e[i], s[u][i]);
                    } else {
                        nx[u][i] = __builtin_fmaf(x.e[i], x.e[i], nx[u][i]);
                        ny[u][i] = __builtin_fmaf(y.e[i], y.e[i], ny[u][i]);
                        s[u][i] = __builtin_fmaf(x.e[i], y.e[i], s[u][i]);
                    }
                }
            }
        }
    }
    float px[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) px[i] = (rem && i < rem) ? load1(q + full_end + i) : 0.0f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float py[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) py[i] = (rem && i < rem) ? to_f32(ry[u][i]) : 0.0f;
        float r = finish_wide<NACC>(s[u], px, py, rem, OP == OP_L2 ? 0 : 1);
        if (OP == OP_COS) {
            float a = finish_wide<NACC>(nx[u], px, py, rem, 2);
            float b = finish_wide<NACC>(ny[u], px, py, rem, 3);
            r = cosine_finish(a, b, r);
        }
        out[u] = r;
    }
}

// ---- integer rows (u8 / i8): exact i32 accumulation, any order is bit-identical
// (simd.rs:1192-1225, 1947-1979, 2109-2143, 2790-2827, 2996-3033).  Group of 8 lanes,
// 16 bytes per lane per step, v_dot4 accumulate.  Valid in lane v == 0.
template <bool SIGNED>
__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) {
    if (SIGNED) return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
    return (int)__builtin_amdgcn_udot4(a, b, (uint32_t)c, false);
}
template <bool SIGNED>
__device__ __forceinline__ int elem(const uint8_t* p) {
    return SIGNED ? (int)(int8_t)*p : (int)*p;
}
__device__ __forceinline__ int group8_sum(int x) {
    x += dpp_i<DPP_XOR1>(x);
    x += dpp_i<DPP_XOR2>(x);
    x += dpp_i<DPP_SHL4>(x);
    return x;
}
template <int OP, bool SIGNED>
__device__ __forceinline__ float group_distance_int(const uint8_t* __restrict__ q, const uint8_t* __restrict__ row,
                                                    int dim, int v) {
    int xx = 0, yy = 0, xy = 0;
    const int vec_end = dim & ~15;
    for (int e = 16 * v; e < vec_end; e += 128) {
        uint4 x = *reinterpret_cast<const uint4*>(q + e);
        uint4 y = *reinterpret_cast<const uint4*>(row + e);
        const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xy = dot4<SIGNED>(xs[i], ys[i], xy);
            if (OP != OP_IP) {
                xx = dot4<SIGNED>(xs[i], xs[i], xx);
                yy = dot4<SIGNED>(ys[i], ys[i], yy);
            }
        }
    }
    for (int e = vec_end + v; e < dim; e += 8) {
        int a = elem<SIGNED>(q + e), b = elem<SIGNED>(row + e);
        xy += a * b;
        xx += a * a;
        yy += b * b;
    }
    xy = group8_sum(xy);
    if (OP == OP_IP) return (float)xy;
    xx = group8_sum(xx);
    yy = group8_sum(yy);
    if (OP == OP_L2) return (float)(int)((uint32_t)xx + (uint32_t)yy - 2u * (uint32_t)xy);
    return cosine_finish((float)xx, (float)yy, (float)xy);
}


template <int OP, bool SIGNED, int U>
__device__ __forceinline__ void group_distance_int_multi(const uint8_t* __restrict__ q,
                                                         const uint8_t* const (&rows)[U], const bool (&active)[U],
                                                         int dim, int v, float (&out)[U]) {
    int xx[U], yy[U], xy[U];
#pragma unroll
    for (int u = 0; u < U; ++u) xx[u] = yy[u] = xy[u] = 0;
    const int vec_end = dim & ~15;
    for (int e = 16 * v; e < vec_end; e += 128) {
        uint4 ys[U];
#pragma unroll
        for (int u = 0; u < U; ++u) ys[u] = *reinterpret_cast<const uint4*>(rows[u] + e);  // unconditional
        const uint4 x = *reinterpret_cast<const uint4*>(q + e);
        const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t yw[4] = {ys[u].x, ys[u].y, ys[u].z, ys[u].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xy[u] = dot4<SIGNED>(xs[i], yw[i], xy[u]);
                if (OP != OP_IP) {
                    xx[u] = dot4<SIGNED>(xs[i], xs[i], xx[u]);
                    yy[u] = dot4<SIGNED>(yw[i], yw[i], yy[u]);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (active[u]) {
            for (int e = vec_end + v; e < dim; e += 8) {
                int a = elem<SIGNED>(q + e), b = elem<SIGNED>(rows[u] + e);
                xy[u] += a * b;
                xx[u] += a * a;
                yy[u] += b * b;
            }
        }
        int sxy = group8_sum(xy[u]);
        if (OP == OP_IP) {
            out[u] = (float)sxy;
            continue;
        }
        int sxx = group8_sum(xx[u]), syy = group8_sum(yy[u]);
        if (OP == OP_L2) out[u] = (float)(int)((uint32_t)sxx + (uint32_t)syy - 2u * (uint32_t)sxy);
        else out[u] = cosine_finish((float)sxx, (float)syy, (float)sxy);
    }
}

// Fixed 128-byte integer rows: the lane's 16 query bytes (`x`) and the query's squared norm (`xx`, the same for
// every row, summed once per search) stay in registers; per row only xy and yy are accumulated.  Integer sums:
// any order is bit-identical.  Valid in lane v == 0; rows[] must all be readable (see group_distance_many).
template <int OP, bool SIGNED, int U>
__device__ __forceinline__ void group_distance_int_pre(const uint4& x, int xx, const uint8_t* const (&rows)[U], int v,
                                                       float (&out)[U]) {
    uint4 ys[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ys[u] = *reinterpret_cast<const uint4*>(rows[u] + 16 * v);
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t yw[4] = {ys[u].x, ys[u].y, ys[u].z, ys[u].w};
        int xy = 0, yy = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xy = dot4<SIGNED>(xs[i], yw[i], xy);
            if (OP != OP_IP) yy = dot4<SIGNED>(yw[i], yw[i], yy);
        }
        if (OP == OP_L2) {
            // |x - y|^2 = xx + sum(yy - 2 xy): one cross-lane sum of the lane's yy - 2 xy instead of two (integer sums modulo
            // 2^32: any order and grouping is bit-identical)
            const int st = group8_sum((int)((uint32_t)yy - 2u * (uint32_t)xy));
            out[u] = (float)(int)((uint32_t)xx + (uint32_t)st);
            continue;
        }
        const int sxy = group8_sum(xy);
        if (OP == OP_IP) {
            out[u] = (float)sxy;
            continue;
        }
        const int syy = group8_sum(yy);
        out[u] = cosine_finish((float)xx, (float)syy, (float)sxy);
    }
}
template <bool SIGNED>
__device__ __forceinline__ int group_norm_int_pre(const uint4& x) {
    int xx = dot4<SIGNED>(x.x, x.x, 0);
    xx = dot4<SIGNED>(x.y, x.y, xx);
    xx = dot4<SIGNED>(x.z, x.z, xx);
    xx = dot4<SIGNED>(x.w, x.w, xx);
    return group8_sum(xx);
}

// ---- packed scalar-quantised rows (SQ4: two codes per byte, SQ1: eight), CompensatedVector<NBITS> with the Dense
// permutation: element i occupies bits [i * bits, (i + 1) * bits) of the code bytes, little-endian within a byte.
// Exact integer sums as above, so any lane assignment is bit-identical to the reference's loops
// (diskann-quantization/src/bits/distances.rs:261-300 1-bit, :470-555 4-bit).
//   SQ4: v_dot8_u32_u4 on whole dwords -- xy, and for L2 xx + yy - 2 xy modulo 2^32 as the u8 path does;
//   SQ1: L2 = popcount(x ^ y), IP = popcount(x & y) (v_bcnt_u32_b32).
// Shape.  A 128-d row is 64 (SQ4) or 16 (SQ1) code bytes: the 8-lane x 16-byte step of the u8 path would leave
// half or seven eighths of the lanes idle.  A group is 4 lanes here, 16 rows per wavefront: a lane reads 16 bytes
// (SQ4) or 4 bytes (SQ1) per step, a group 64 or 16 bytes -- 128 dimensions per step for both, one request per
// lane for the common length.  Every load starts at a multiple of its own width below the code-byte count, so it
// stays inside the row's 16-byte-aligned stride; bits at or beyond dim * bits (padding of the last byte, the
// compensation, whatever follows inside the load) are masked to zero before they are used, in both operands.
template <int BITS>
struct PackedShape {
    static constexpr int NW = BITS == 4 ? 4 : BITS == 2 ? 2 : 1;  // dwords per lane per step
    static constexpr int LB = 4 * NW, G = 4, STEP = G * LB;
};
template <int NW>
struct PWords {
    uint32_t w[NW];
};
template <int NW>
__device__ __forceinline__ PWords<NW> packed_load(const uint8_t* p) {
    if constexpr (NW == 4) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        return {{t.x, t.y, t.z, t.w}};
    } else if constexpr (NW == 2) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        return {{t.x, t.y}};
    } else {
        return {{*reinterpret_cast<const uint32_t*>(p)}};
    }
}
// keep the first `valid` bits of the lane's chunk (valid <= 0: none)
template <int NW>
__device__ __forceinline__ void packed_mask(PWords<NW>& a, int valid) {
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int nb = valid - 32 * i;
        a.w[i] &= nb >= 32 ? 0xFFFFFFFFu : nb <= 0 ? 0u : ((1u << nb) - 1u);
    }
}
// acc + sum of the products of the BITS-wide fields of two dwords.  There is no dot instruction for 2-bit fields:
// the even and the odd fields are widened to nibbles (and, shift, and) and go through v_dot8_u32_u4 twice -- three
// operations per operand and two dots for 16 elements, where bit planes cost four ands, four popcounts and the
// weighting; a query kept in registers is widened once (packed_query_pre).
constexpr uint32_t kEven2 = 0x33333333u;
template <int BITS>
__device__ __forceinline__ uint32_t packed_dot(uint32_t x, uint32_t y, uint32_t acc) {
    static_assert(BITS == 4 || BITS == 2, "dot instruction widths");
    if constexpr (BITS == 4) {
        return __builtin_amdgcn_udot8(x, y, acc, false);
    } else {
        acc = __builtin_amdgcn_udot8(x & kEven2, y & kEven2, acc, false);
        return __builtin_amdgcn_udot8((x >> 2) & kEven2, (y >> 2) & kEven2, acc, false);
    }
}
__device__ __forceinline__ uint32_t group4_sum(uint32_t x) {
    x += (uint32_t)dpp_i<DPP_XOR1>((int)x);
    x += (uint32_t)dpp_i<DPP_XOR2>((int)x);
    return x;
}
// U rows against one query (or stored row) `q`; rows[u] must be readable even where the caller discards out[u]
// (the loads are unconditional, see group_distance_many).  Valid in every lane of the group.
template <int BITS, int OP, int U>
__device__ __forceinline__ void group_distance_packed(const uint8_t* __restrict__ q, const uint8_t* const (&rows)[U],
                                                      int dim, int v, float (&out)[U]) {
    static_assert(OP == OP_L2 || OP == OP_IP, "scalar-quantised rows: L2 and inner product");
    using P = PackedShape<BITS>;
    constexpr int NW = P::NW;
    const int total_bits = dim * BITS, cb = (total_bits + 7) >> 3;
    uint32_t t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = 0u;
    for (int o0 = 0; o0 < cb; o0 += P::STEP) {
        const int o = o0 + P::LB * v;
        const bool in = o < cb;
        const int ol = in ? o : 0;  // clamped: every request is issued, none behind a branch, all inside the row
        const int valid = in ? total_bits - 8 * o : 0;
        PWords<NW> y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) y[u] = packed_load<NW>(rows[u] + ol);
        PWords<NW> x = packed_load<NW>(q + ol);
        packed_mask<NW>(x, valid);
        uint32_t xx = 0u;
        if constexpr (BITS != 1 && OP == OP_L2) {
#pragma unroll
            for (int i = 0; i < NW; ++i) xx = packed_dot<BITS>(x.w[i], x.w[i], xx);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (OP == OP_L2) packed_mask<NW>(y[u], valid);  // (inner product: x's zeros suffice)
            if constexpr (BITS != 1) {
                uint32_t xy = 0u, yy = 0u;
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    xy = packed_dot<BITS>(x.w[i], y[u].w[i], xy);
                    if constexpr (OP == OP_L2) yy = packed_dot<BITS>(y[u].w[i], y[u].w[i], yy);
                }
                t[u] += OP == OP_L2 ? xx + yy - 2u * xy : xy;
            } else {
#pragma unroll
                for (int i = 0; i < NW; ++i)
                    t[u] += (uint32_t)__builtin_popcount(OP == OP_L2 ? x.w[i] ^ y[u].w[i] : x.w[i] & y[u].w[i]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) out[u] = (float)(int)group4_sum(t[u]);
}
template <int BITS, int OP>
__device__ __forceinline__ float group_distance_packed1(const uint8_t* q, const uint8_t* row, int dim, int v) {
    const uint8_t* const rows[1] = {row};
    float out[1];
    group_distance_packed<BITS, OP, 1>(q, rows, dim, v, out);
    return out[0];
}

// Fixed 128-dimension packed rows -- exactly one step of group_distance_packed: 64 code bytes (SQ4, 16 per lane) or 16
// (SQ1, 4 per lane), no tail and nothing to mask.  The lane's query dwords (`x`; SQ1 uses x.x) and, for SQ4 L2, the
// query's squared norm (`xx`, the same for every row, summed once per search) stay in registers, as in
// group_distance_int_pre; per row only xy and yy are accumulated.  rows[] must all be readable.
template <int BITS>
__device__ __forceinline__ uint4 packed_query_pre(const uint8_t* qs, int v) {
    if constexpr (BITS == 4) {
        return *reinterpret_cast<const uint4*>(qs + 16 * v);
    } else {
        return uint4{*reinterpret_cast<const uint32_t*>(qs + 4 * v), 0u, 0u, 0u};
    }
}
template <int BITS>
__device__ __forceinline__ int group_norm_packed_pre(const uint4& x) {
    if constexpr (BITS != 4) return 0;  // (1-bit rows: L2 = popcount(x ^ y) needs no norm)
    uint32_t xx = __builtin_amdgcn_udot8(x.x, x.x, 0u, false);
    xx = __builtin_amdgcn_udot8(x.y, x.y, xx, false);
    xx = __builtin_amdgcn_udot8(x.z, x.z, xx, false);
    xx = __builtin_amdgcn_udot8(x.w, x.w, xx, false);
    return (int)group4_sum(xx);
}
template <int BITS, int OP, int U>
__device__ __forceinline__ void group_distance_packed_pre(const uint4& x, int xx, const uint8_t* const (&rows)[U], int v,
                                                          float (&out)[U]) {
    static_assert(OP == OP_L2 || OP == OP_IP, "scalar-quantised rows: L2 and inner product");
    using P = PackedShape<BITS>;
    constexpr int NW = P::NW;
    PWords<NW> y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) y[u] = packed_load<NW>(rows[u] + P::LB * v);
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        uint32_t t = 0u;
        if constexpr (BITS == 4) {
            uint32_t xy = 0u, yy = 0u;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                xy = __builtin_amdgcn_udot8(xs[i], y[u].w[i], xy, false);
                if constexpr (OP == OP_L2) yy = __builtin_amdgcn_udot8(y[u].w[i], y[u].w[i], yy, false);
            }
            // |x - y|^2 = xx + sum(yy - 2 xy) modulo 2^32: one cross-lane sum
            t = OP == OP_L2 ? (uint32_t)xx + group4_sum(yy - 2u * xy) : group4_sum(xy);
        } else {
            t = group4_sum((uint32_t)__builtin_popcount(OP == OP_L2 ? xs[0] ^ y[u].w[0] : xs[0] & y[u].w[0]));
        }
        out[u] = (float)(int)t;
    }
}

// ---- spherically quantised rows (spherical::Data<NBITS>, diskann-quantization/src/spherical/vectors.rs): the code
// bytes of the packed rows above, then the 6-byte DataMeta.  Every metric needs the raw inner product of the codes
// (the epilogue is finish_distance), so these entries take no OP.  Three query forms:
//   the row image itself (SAME_AS_DATA) and Dense codes of the row's width (SCALAR_QUANTIZED): group_distance_packed's
//     inner-product form at 1, 2 or 4 bits.  The query's bits at or beyond dim are masked; a zero in one operand
//     removes the product, whatever the row holds there;
//   FOUR_BIT_TRANSPOSED against 1-bit rows (bits/distances.rs:2123-2249): per block of 64 elements four u64 words,
//     word j = bit j of the 64 four-bit values; <q, y> = sum_j 2^j popcount(y & plane_j).  A lane owns one data dword
//     (32 dimensions) per step and the four matching plane dwords: block (o / 8), half (o / 4) & 1 of the data byte
//     offset o.  The row's bits at or beyond dim are masked, the query's padding may hold anything.  The plane loads
//     stay inside the ceil(dim / 64) * 32 plane bytes because o < ceil(dim / 8).
__host__ __device__ constexpr uint32_t sph_plane_bytes(uint32_t dim) { return ((dim + 63u) >> 6) * 32u; }
// bytes of one query under `layout` (0 = the layout is not defined for the row type)
__host__ __device__ constexpr uint32_t sph_query_bytes(int dt, uint32_t dim, int layout) {
    const int bits = sq_bits(dt);
    const uint32_t cb = (uint32_t)(((uint64_t)dim * (uint32_t)bits + 7u) >> 3);
    return layout == QL_SAME                       ? cb + kSphDataMeta
           : layout == QL_TRANSPOSED && bits == 1 ? sph_plane_bytes(dim) + kSphQueryMeta
           : layout == QL_SCALAR && bits != 1     ? cb + kSphQueryMeta
                                                  : 0u;
}
__device__ __forceinline__ uint32_t transposed_dot(uint32_t y, const uint32_t (&p)[4]) {
    return (uint32_t)__builtin_popcount(y & p[0]) + ((uint32_t)__builtin_popcount(y & p[1]) << 1) +
           ((uint32_t)__builtin_popcount(y & p[2]) << 2) + ((uint32_t)__builtin_popcount(y & p[3]) << 3);
}
template <int U>
__device__ __forceinline__ void group_ip_transposed(const uint8_t* __restrict__ q, const uint8_t* const (&rows)[U],
                                                    int dim, int v, float (&out)[U]) {
    const int cb = (dim + 7) >> 3;
    uint32_t t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = 0u;
    for (int o0 = 0; o0 < cb; o0 += 16) {
        const int o = o0 + 4 * v;
        const bool in = o < cb;
        const int ol = in ? o : 0;  // clamped as in group_distance_packed: every request is issued, all in bounds
        const int valid = in ? dim - 8 * o : 0;
        PWords<1> y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) y[u] = packed_load<1>(rows[u] + ol);
        const uint8_t* pq = q + (ol >> 3) * 32 + ((ol >> 2) & 1) * 4;
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = *reinterpret_cast<const uint32_t*>(pq + 8 * j);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            packed_mask<1>(y[u], valid);
            t[u] += transposed_dot(y[u].w[0], p);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) out[u] = (float)(int)group4_sum(t[u]);
}
template <int DT, int U>
__device__ __forceinline__ void group_ip_sph(const uint8_t* q, const uint8_t* const (&rows)[U], int dim, int v,
                                             float (&out)[U]) {
    if constexpr (DT == DT_SPH1T) group_ip_transposed<U>(q, rows, dim, v, out);
    else group_distance_packed<sq_bits(DT), OP_IP, U>(q, rows, dim, v, out);
}
template <int DT>
__device__ __forceinline__ float group_ip_sph1(const uint8_t* q, const uint8_t* row, int dim, int v) {
    const uint8_t* const rows[1] = {row};
    float out[1];
    group_ip_sph<DT, 1>(q, rows, dim, v, out);
    return out[0];
}
// Fixed 128 dimensions, the lane's query words in registers: the four plane dwords (transposed), the two code dwords
// widened to four nibble dwords (2 bit), the code dwords as they are (4 bit: four, 1 bit: one).
template <int DT>
__device__ __forceinline__ uint4 sph_query_pre(const uint8_t* qs, int v) {
    if constexpr (DT == DT_SPH1T) {
        const uint8_t* pq = qs + (v >> 1) * 32 + (v & 1) * 4;
        return uint4{*reinterpret_cast<const uint32_t*>(pq), *reinterpret_cast<const uint32_t*>(pq + 8),
                     *reinterpret_cast<const uint32_t*>(pq + 16), *reinterpret_cast<const uint32_t*>(pq + 24)};
    } else if constexpr (sq_bits(DT) == 2) {
        const uint2 x = *reinterpret_cast<const uint2*>(qs + 8 * v);
        return uint4{x.x & kEven2, (x.x >> 2) & kEven2, x.y & kEven2, (x.y >> 2) & kEven2};
    } else {
        return packed_query_pre<sq_bits(DT)>(qs, v);
    }
}
template <int DT, int U>
__device__ __forceinline__ void group_ip_sph_pre(const uint4& x, const uint8_t* const (&rows)[U], int v, float (&out)[U]) {
    constexpr int BITS = sq_bits(DT);
    constexpr int NW = PackedShape<BITS>::NW;
    PWords<NW> y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) y[u] = packed_load<NW>(rows[u] + PackedShape<BITS>::LB * v);
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        uint32_t t = 0u;
        if constexpr (DT == DT_SPH1T) {
            t = transposed_dot(y[u].w[0], xs);
        } else if constexpr (BITS == 1) {
            t = (uint32_t)__builtin_popcount(xs[0] & y[u].w[0]);
        } else if constexpr (BITS == 2) {
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                t = __builtin_amdgcn_udot8(xs[2 * i], y[u].w[i] & kEven2, t, false);
                t = __builtin_amdgcn_udot8(xs[2 * i + 1], (y[u].w[i] >> 2) & kEven2, t, false);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NW; ++i) t = __builtin_amdgcn_udot8(xs[i], y[u].w[i], t, false);
        }
        out[u] = (float)(int)group4_sum(t);
    }
}

// ---- MinMax-quantised rows (minmax::Data<NBITS>, diskann-quantization/src/minmax/vectors.rs), front-canonical: the
// 20-byte MinMaxCompensation (u32 dim, f32 b, n, a, norm_squared), then the Dense code bytes of the packed rows above
// (MM8: one byte per code).  Every metric needs the raw inner product of the codes only (the epilogue is
// finish_minmax), an exact u32 sum, so any lane assignment is bit-identical.  `x` and the rows are image pointers; the
// codes start at byte 20 of an image:
//   global rows (strides are multiples of 16): 4-byte aligned.  The loads say so (mm_load copies from a pointer of
//     stated alignment, never through a uint4*), and the compiler may emit one wide load or dword loads for them;
//   a query staged in LDS sits at slot + 12 (launch_shape.h), its codes 16-byte aligned: XA = the lane's load width.
// Lane shapes: MM8 the u8 path's 8 lanes x 16 bytes (v_dot4_u32_u8), MM4 / MM2 / MM1 PackedShape's 4 lanes x 16 / 8 / 4
// bytes.  Steps that lie wholly below dim * bits use the wide loads; the one tail step reads dword by dword, each dword
// only where it starts below the code-byte count (else the row's first code dword, whose product is masked away), so no
// load ends beyond the image rounded up to 4 bytes -- inside the row's stride, the 16-byte rounded query buffers and the
// LDS slot.  x's bits at or beyond dim * bits are masked in the tail; a zero in one operand removes the product.
template <int BITS>
struct MmShape {
    static constexpr int NW = BITS >= 4 ? 4 : BITS == 2 ? 2 : 1;  // dwords per lane per step
    static constexpr int LB = 4 * NW, G = BITS == 8 ? 8 : 4, STEP = G * LB;
};
template <int NW, int ALIGN>
__device__ __forceinline__ PWords<NW> mm_load(const uint8_t* p) {
    PWords<NW> r;
    __builtin_memcpy(r.w, __builtin_assume_aligned(p, ALIGN), 4 * NW);
    return r;
}
template <int NW>
__device__ __forceinline__ PWords<NW> mm_load_tail(const uint8_t* codes, int o, int cb) {
    PWords<NW> r;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int oi = o + 4 * i;
        r.w[i] = *reinterpret_cast<const uint32_t*>(codes + (oi < cb ? oi : 0));
    }
    return r;
}
template <int BITS>
__device__ __forceinline__ uint32_t mm_dot(uint32_t x, uint32_t y, uint32_t acc) {
    if constexpr (BITS == 8) return __builtin_amdgcn_udot4(x, y, acc, false);
    else if constexpr (BITS == 1) return acc + (uint32_t)__builtin_popcount(x & y);
    else return packed_dot<BITS>(x, y, acc);
}
template <int BITS>
__device__ __forceinline__ float mm_group_sum(uint32_t t) {  // (u32 -> f32 rounds to nearest even, as `raw as f32`)
    if constexpr (BITS == 8) return (float)(uint32_t)group8_sum((int)t);  // valid in lane v == 0
    else return (float)group4_sum(t);
}
template <int BITS, int U, int XA>
__device__ __forceinline__ void group_ip_mm(const uint8_t* __restrict__ x, const uint8_t* const (&rows)[U], int dim, int v,
                                            float (&out)[U]) {
    using P = MmShape<BITS>;
    constexpr int NW = P::NW;
    const int total_bits = dim * BITS, cb = (total_bits + 7) >> 3;
    const uint8_t* xc = x + kMmHeader;
    uint32_t t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = 0u;
    int o0 = 0;
    for (; 8 * (o0 + P::STEP) <= total_bits; o0 += P::STEP) {
        const int o = o0 + P::LB * v;
        PWords<NW> y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) y[u] = mm_load<NW, 4>(rows[u] + kMmHeader + o);
        const PWords<NW> xw = mm_load<NW, XA>(xc + o);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < NW; ++i) t[u] = mm_dot<BITS>(xw.w[i], y[u].w[i], t[u]);
        }
    }
    if (8 * o0 < total_bits) {
        const int o = o0 + P::LB * v;
        const bool in = o < cb;
        const int ol = in ? o : 0;  // clamped: every request is issued, none behind a branch
        const int valid = in ? total_bits - 8 * o : 0;
        PWords<NW> y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) y[u] = mm_load_tail<NW>(rows[u] + kMmHeader, ol, cb);
        PWords<NW> xw = mm_load_tail<NW>(xc, ol, cb);
        packed_mask<NW>(xw, valid);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < NW; ++i) t[u] = mm_dot<BITS>(xw.w[i], y[u].w[i], t[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) out[u] = mm_group_sum<BITS>(t[u]);
}
template <int BITS, int XA>
__device__ __forceinline__ float group_ip_mm1(const uint8_t* x, const uint8_t* row, int dim, int v) {
    const uint8_t* const rows[1] = {row};
    float out[1];
    group_ip_mm<BITS, 1, XA>(x, rows, dim, v, out);
    return out[0];
}
// Fixed 128 dimensions -- exactly one full step (128 / 64 / 32 / 16 code bytes), nothing to mask and no load beyond the
// image.  The lane's query words stay in registers (2 bit: widened to nibbles once, as sph_query_pre); `qs` is the
// staged image.
template <int BITS>
__device__ __forceinline__ uint4 mm_query_pre(const uint8_t* qs, int v) {
    const uint8_t* c = qs + kMmHeader + MmShape<BITS>::LB * v;
    if constexpr (BITS >= 4) {
        const PWords<4> t = mm_load<4, 16>(c);
        return uint4{t.w[0], t.w[1], t.w[2], t.w[3]};
    } else if constexpr (BITS == 2) {
        const PWords<2> t = mm_load<2, 8>(c);
        return uint4{t.w[0] & kEven2, (t.w[0] >> 2) & kEven2, t.w[1] & kEven2, (t.w[1] >> 2) & kEven2};
    } else {
        return uint4{mm_load<1, 4>(c).w[0], 0u, 0u, 0u};
    }
}
template <int BITS, int U>
__device__ __forceinline__ void group_ip_mm_pre(const uint4& x, const uint8_t* const (&rows)[U], int v, float (&out)[U]) {
    constexpr int NW = MmShape<BITS>::NW;
    PWords<NW> y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) y[u] = mm_load<NW, 4>(rows[u] + kMmHeader + MmShape<BITS>::LB * v);
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        uint32_t t = 0u;
        if constexpr (BITS == 2) {
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                t = __builtin_amdgcn_udot8(xs[2 * i], y[u].w[i] & kEven2, t, false);
                t = __builtin_amdgcn_udot8(xs[2 * i + 1], (y[u].w[i] >> 2) & kEven2, t, false);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NW; ++i) t = mm_dot<BITS>(xs[i], y[u].w[i], t);
        }
        out[u] = mm_group_sum<BITS>(t);
    }
}

// ---- MinMax rows of 4, 2 or 1 bit searched with MM8 query images (MinMaxQuery::EightBit: the heterogeneous
// kernel::<8, M>, minmax/vectors.rs:206-229, whose raw product is a u32 -- exact, so any lane assignment is
// bit-identical).  The row side is group_ip_mm's: the same 4-lane group, the same loads, the same tail rule, 128
// elements per step at every width.  Only the query operand differs: one byte per element, 32 bytes per lane and step,
// staged once per query (mmq_stage_query) in the order the row's dwords are taken apart in:
//   4 bit  a row dword holds 8 elements; `& 0x0F0F0F0F` leaves the even ones in its four bytes, `>> 4 &` the odd ones.
//          Staged per 8 elements: the four even query bytes, then the four odd ones -- two v_dot4_u32_u8 per row dword;
//   2 bit  a row dword holds 16 elements; `>> 2 s & 0x03030303` leaves elements s, s + 4, s + 8, s + 12.  Staged per 16
//          elements: dword s = query bytes s, s + 4, s + 8, s + 12 (a 4 x 4 transpose) -- four dots per row dword;
//   1 bit  a row dword holds 32 elements.  Staged per 32 elements: eight plane dwords, plane j = bit j of the 32 query
//          bytes; <q, y> = sum_j 2^j popcount(plane_j & y) (v_bcnt_u32_b32), as FOUR_BIT_TRANSPOSED does with four.
// The staged codes start where the image's do (slot + 32, 16-byte aligned) and a lane's 32 bytes at a multiple of 32:
// two ds_read_b128 per full step.  Elements at or beyond dim are staged as zero, so whatever the row holds in its
// padding bits, or in the dword a clamped tail load fetched instead, meets a zero; the row needs no mask.
template <int MBITS>
__device__ __forceinline__ void mmq_stage_query(uint8_t* qs, const uint8_t* src, uint32_t dim, uint32_t tid, uint32_t nthreads) {
    static_assert(MBITS == 4 || MBITS == 2 || MBITS == 1, "rows narrower than the 8-bit query");
    for (uint32_t i = tid; i < kMmHeader; i += nthreads) qs[i] = src[i];
    const uint8_t* c = src + kMmHeader;  // exactly dim bytes are read
    uint32_t* out = reinterpret_cast<uint32_t*>(qs + kMmHeader);
    const uint32_t nd = MBITS == 1 ? ((dim + 31u) >> 5) * 8u : ((dim + 15u) >> 4) * 4u;  // staged dwords (mm_slot_bytes)
    for (uint32_t w = tid; w < nd; w += nthreads) {
        uint32_t val = 0u;
        if constexpr (MBITS == 1) {
            const uint32_t e0 = (w >> 3) * 32u, j = w & 7u;
            for (uint32_t i = 0; i < 32u; ++i)
                if (e0 + i < dim) val |= (((uint32_t)c[e0 + i] >> j) & 1u) << i;
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) {
                const uint32_t e = MBITS == 4 ? (w >> 1) * 8u + 2u * b + (w & 1u) : (w >> 2) * 16u + (w & 3u) + 4u * b;
                if (e < dim) val |= (uint32_t)c[e] << (8u * b);
            }
        }
        out[w] = val;
    }
}
// acc + the products of one row dword's fields with their staged query dwords `q` (2, 4 or 8 of them)
template <int MBITS>
__device__ __forceinline__ uint32_t mmq_dot(const uint32_t* q, uint32_t y, uint32_t acc) {
    if constexpr (MBITS == 4) {
        acc = __builtin_amdgcn_udot4(q[0], y & 0x0F0F0F0Fu, acc, false);
        return __builtin_amdgcn_udot4(q[1], (y >> 4) & 0x0F0F0F0Fu, acc, false);
    } else if constexpr (MBITS == 2) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_udot4(q[s], (y >> (2 * s)) & 0x03030303u, acc, false);
        return acc;
    } else {
        uint32_t h = (uint32_t)__builtin_popcount(q[7] & y);
#pragma unroll
        for (int j = 6; j >= 0; --j) h = (h << 1) + (uint32_t)__builtin_popcount(q[j] & y);
        return acc + h;
    }
}
// `x` is the staged query (the header, then the staged codes), the rows are images in global memory
template <int MBITS, int U>
__device__ __forceinline__ void group_ip_mmq(const uint8_t* __restrict__ x, const uint8_t* const (&rows)[U], int dim, int v,
                                             float (&out)[U]) {
    using P = MmShape<MBITS>;
    constexpr int NW = P::NW, QW = 8 / MBITS, QPB = 8 / MBITS;  // query dwords per row dword; query bytes per row byte
    static_assert(NW * QW == 8, "a lane's step is 32 query bytes");
    const int total_bits = dim * MBITS, cb = (total_bits + 7) >> 3;
    const uint8_t* xc = x + kMmHeader;
    uint32_t t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = 0u;
    int o0 = 0;
    for (; 8 * (o0 + P::STEP) <= total_bits; o0 += P::STEP) {
        const int o = o0 + P::LB * v;
        PWords<NW> y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) y[u] = mm_load<NW, 4>(rows[u] + kMmHeader + o);
        const PWords<8> xw = mm_load<8, 16>(xc + QPB * o);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < NW; ++i) t[u] = mmq_dot<MBITS>(&xw.w[QW * i], y[u].w[i], t[u]);
        }
    }
    if (8 * o0 < total_bits) {
        const int o = o0 + P::LB * v;
        PWords<NW> y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) y[u] = mm_load_tail<NW>(rows[u] + kMmHeader, o, cb);  // (beyond cb: the first code dword)
        // the query dwords of a row dword that starts below cb lie inside the staged codes; of one beyond it: zeros
        PWords<8> xw;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int oi = o + 4 * i;
            const bool in = oi < cb;
            const PWords<QW> part = mm_load<QW, (QW >= 4 ? 16 : 8)>(xc + (in ? QPB * oi : 0));
#pragma unroll
            for (int j = 0; j < QW; ++j) xw.w[QW * i + j] = in ? part.w[j] : 0u;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int i = 0; i < NW; ++i) t[u] = mmq_dot<MBITS>(&xw.w[QW * i], y[u].w[i], t[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) out[u] = mm_group_sum<MBITS>(t[u]);
}
// stages query `src` (ix.qbytes bytes) of integer rows at `qs` = slot + query_stage_off(DT): the bytes as they are, or, for
// MinMax rows searched with MM8 images, the form group_ip_mmq reads.  Every kernel that stages such a query calls this.
template <int DT>
__device__ __forceinline__ void stage_int_query(uint8_t* qs, const uint8_t* src, uint32_t qbytes, uint32_t dim, uint32_t tid,
                                                uint32_t nthreads) {
    if constexpr (dt_is_mmq(DT)) {
        mmq_stage_query<sq_bits(DT)>(qs, src, dim, tid, nthreads);
    } else {
        for (uint32_t i = tid; i < qbytes; i += nthreads) qs[i] = src[i];
    }
}

// ---- dtype dispatch ------------------------------------------------------------------
// Query-side staging type and group width for the *search* path
// (Full<T>::query_distance, diskann-inmem/src/layers/full.rs:351-504):
//   f32 rows: f32 query, L2/IP Strategy4x1 (NACC 4), cosine Strategy2x4 (NACC 2)
//   f16 rows: query widened to f32 once, L2/IP Strategy4x2 (== NACC 4), cosine NACC 2
//   u8/i8  : integer query, exact
// and for the *pair* path (DistanceProvider::distance_comparer, V3):
//   f16 x f16: L2/IP/cosine all Strategy2x4 (NACC 2)  (simd.rs:989,1752,2591)
template <int DT, int OP, bool PAIR>
struct Scheme {
    static constexpr bool kInt = (DT == DT_U8 || DT == DT_I8 || DT == DT_PQ || dt_is_sq(DT) || dt_is_sph(DT) || dt_mm_rows(DT));
    static constexpr int NACC = (OP == OP_COS) ? 2 : ((DT == DT_F16 && PAIR) ? 2 : 4);
    static constexpr int G = dt_is_packed(DT) ? 4 : kInt ? 8 : 2 * NACC;  // (packed rows: PackedShape::G)
    // search-path gather: 2-byte rows use the wide layout (one lane per accumulator)
    static constexpr bool kWide = (DT == DT_F16) && !PAIR;
    static constexpr int GS = kWide ? NACC : G;
};

template <int DT>
struct RowType {
    using type = float;
};
template <>
struct RowType<DT_F16> {
    using type = __half;
};
template <>
struct RowType<DT_U8> {
    using type = uint8_t;
};
template <>
struct RowType<DT_I8> {
    using type = uint8_t;
};
template <>
struct RowType<DT_SQ8> {
    using type = uint8_t;
};
template <>
struct RowType<DT_SQ4> {
    using type = uint8_t;
};
template <>
struct RowType<DT_SQ1> {
    using type = uint8_t;
};
template <>
struct RowType<DT_SPH1> {
    using type = uint8_t;
};
template <>
struct RowType<DT_SPH2> {
    using type = uint8_t;
};
template <>
struct RowType<DT_SPH4> {
    using type = uint8_t;
};
template <>
struct RowType<DT_SPH1T> {
    using type = uint8_t;
};
template <>
struct RowType<DT_MM1> {
    using type = uint8_t;
};
template <>
struct RowType<DT_MM2> {
    using type = uint8_t;
};
template <>
struct RowType<DT_MM4> {
    using type = uint8_t;
};
template <>
struct RowType<DT_MM8> {
    using type = uint8_t;
};
template <>
struct RowType<DT_MM1Q> {
    using type = uint8_t;
};
template <>
struct RowType<DT_MM2Q> {
    using type = uint8_t;
};
template <>
struct RowType<DT_MM4Q> {
    using type = uint8_t;
};
template <>
struct RowType<DT_PQ> {
    using type = uint8_t;
};

// `q` is the staged query: f32 for float rows, raw bytes for integer rows.
template <int DT, int OP, bool PAIR, int DIM, typename QT>
__device__ __forceinline__ float group_distance(const QT* q, const uint8_t* row, int dim, int v) {
    if constexpr (dt_is_mmq(DT)) {  // (q: the MM8 image staged by mmq_stage_query)
        const uint8_t* const rows[1] = {row};
        float out[1];
        group_ip_mmq<sq_bits(DT), 1>(reinterpret_cast<const uint8_t*>(q), rows, dim, v, out);
        return out[0];
    } else if constexpr (dt_is_mm(DT)) {  // (q: the image staged at slot + 12, codes 16-byte aligned)
        return group_ip_mm1<sq_bits(DT), MmShape<sq_bits(DT)>::LB>(reinterpret_cast<const uint8_t*>(q), row, dim, v);
    } else if constexpr (dt_is_sph(DT)) {
        return group_ip_sph1<DT>(reinterpret_cast<const uint8_t*>(q), row, dim, v);
    } else if constexpr (dt_is_packed(DT)) {
        return group_distance_packed1<sq_bits(DT), OP>(reinterpret_cast<const uint8_t*>(q), row, dim, v);
    } else if constexpr (DT == DT_U8 || DT == DT_I8 || DT == DT_SQ8) {
        return group_distance_int<OP, DT == DT_I8>(reinterpret_cast<const uint8_t*>(q), row, dim, v);
    } else {
        using RT = typename RowType<DT>::type;
        return group_distance_raw<Scheme<DT, OP, PAIR>::NACC, OP, DIM>(q, reinterpret_cast<const RT*>(row), dim, v);
    }
}


// stored row x stored row with the prune-path association (Scheme<DT, OP, true>)
template <int DT, int OP>
__device__ __forceinline__ float group_distance_rows(const uint8_t* x, const uint8_t* y, int dim, int v) {
    static_assert(!dt_is_mmq(DT), "row x row distances have no query form");
    if constexpr (dt_is_mm(DT)) {  // (both operands are rows in global memory: 4-byte aligned codes)
        return group_ip_mm1<sq_bits(DT), 4>(x, y, dim, v);
    } else if constexpr (dt_is_sph(DT)) {  // (a stored row as the query is always the symmetric form)
        static_assert(DT != DT_SPH1T, "row x row distances have no query layout");
        return group_ip_sph1<DT>(x, y, dim, v);
    } else if constexpr (dt_is_packed(DT)) {
        return group_distance_packed1<sq_bits(DT), OP>(x, y, dim, v);
    } else if constexpr (DT == DT_U8 || DT == DT_I8 || DT == DT_SQ8) {
        return group_distance_int<OP, DT == DT_I8>(x, y, dim, v);
    } else {
        using RT = typename RowType<DT>::type;
        return group_distance_pair<Scheme<DT, OP, true>::NACC, OP, RT>(reinterpret_cast<const RT*>(x),
                                                                       reinterpret_cast<const RT*>(y), dim, v);
    }
}

// U rows per lane group at once.  Contract: rows[u] is a readable row address even when !active[u] (callers pass
// row 0): the loads are issued unconditionally so that none of them sits behind a branch with its own wait.
// WIDE = false keeps the G-lane layout for 2-byte rows (kernels whose lane groups are Scheme::G wide).
template <int DT, int OP, bool PAIR, int U, bool WIDE = true, typename QT>
__device__ __forceinline__ void group_distance_many(const QT* q, const uint8_t* const (&rows)[U],
                                                    const bool (&active)[U], int dim, int v, float (&out)[U]) {
    if constexpr (dt_is_mmq(DT)) {
        group_ip_mmq<sq_bits(DT), U>(reinterpret_cast<const uint8_t*>(q), rows, dim, v, out);
    } else if constexpr (dt_is_mm(DT)) {
        group_ip_mm<sq_bits(DT), U, MmShape<sq_bits(DT)>::LB>(reinterpret_cast<const uint8_t*>(q), rows, dim, v, out);
    } else if constexpr (dt_is_sph(DT)) {
        group_ip_sph<DT, U>(reinterpret_cast<const uint8_t*>(q), rows, dim, v, out);
    } else if constexpr (dt_is_packed(DT)) {
        group_distance_packed<sq_bits(DT), OP, U>(reinterpret_cast<const uint8_t*>(q), rows, dim, v, out);
    } else if constexpr (DT == DT_U8 || DT == DT_I8 || DT == DT_SQ8) {
        group_distance_int_multi<OP, DT == DT_I8, U>(reinterpret_cast<const uint8_t*>(q), rows, active, dim, v, out);
    } else {
        using RT = typename RowType<DT>::type;
        const RT* typed[U];
#pragma unroll
        for (int u = 0; u < U; ++u) typed[u] = reinterpret_cast<const RT*>(rows[u]);
        if constexpr (Scheme<DT, OP, PAIR>::kWide && WIDE)
            group_distance_wide<Scheme<DT, OP, PAIR>::NACC, OP, U>(q, typed, active, dim, v, out);
        else
            group_distance_multi<Scheme<DT, OP, PAIR>::NACC, OP, U>(q, typed, active, dim, v, out);
    }
}

// simd_op for f32 x f32, Strategy4x1, V3 (simd.rs:321-363, 686-747); IS_L2 ? L2 : IP
template <bool IS_L2>
__device__ float simd_op_seq(const float* x, const float* y, uint32_t len) {
    float acc[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int l = 0; l < 8; ++l) acc[a][l] = 0.0f;
    const uint32_t blocks = len / 8;
    for (uint32_t g = 0; g < blocks; ++g) {
        const int a = g & 3;
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const float xv = x[8 * g + l], yv = y[8 * g + l];
#pragma unroll
            for (int aa = 0; aa < 4; ++aa) {
                if (aa == a) {
                    if (IS_L2) {
                        const float c = xv - yv;
                        acc[aa][l] = __builtin_fmaf(c, c, acc[aa][l]);
                    } else {
                        acc[aa][l] = __builtin_fmaf(xv, yv, acc[aa][l]);
                    }
                }
            }
        }
    }
    float s[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) s[l] = (acc[0][l] + acc[1][l]) + (acc[2][l] + acc[3][l]);
    const uint32_t rem = len & 7u;
    if (rem) {
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            const float xv = (uint32_t)l < rem ? x[8 * blocks + l] : 0.0f;
            const float yv = (uint32_t)l < rem ? y[8 * blocks + l] : 0.0f;
            if (IS_L2) {
                const float c = xv - yv;
                s[l] = __builtin_fmaf(c, c, s[l]);
            } else {
                s[l] = __builtin_fmaf(xv, yv, s[l]);
            }
        }
    }
    return ((s[0] + s[4]) + (s[2] + s[6])) + ((s[1] + s[5]) + (s[3] + s[7]));
}


// scalar-quantiser parameters of an SQ-8 / SQ4 / SQ1 index
struct SqParams {
    float k;              // (1/(2^bits - 1))^2 * scale^2, evaluated in f32 in the reference's order.  Spherical rows
                          // have no scale: non-zero says the query ends in a QueryMeta (SCALAR_QUANTIZED layout)
    float shift_norm_sq;  // ||shift||^2; spherical rows: CompensatedIP::squared_shift_norm
};

__device__ __forceinline__ float load_f32_unaligned(const uint8_t* p) {
    uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ uint32_t load_u16_unaligned(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ float load_f16_unaligned(const uint8_t* p) {  // f16 -> f32 is exact
    return __half2float(__ushort_as_half((unsigned short)load_u16_unaligned(p)));
}

// Spherical rows: the raw inner product of the codes -> SimilarityScore, each f32 operation in the reference's
// association (spherical/vectors.rs: kernel :494-528, query x data :612-636 and :776-801; L2 :584-594, IP :744-758,
// Cosine :867-892; no fused multiply-add).  `x` is the query -- a row image (DataMeta at the code-byte count) or
// codes / planes followed by a QueryMeta of four f32 (inner_product_correction, bit_sum, offset, metric_specific,
// vectors.rs:381-399) -- and `y` the row.  The metadata sits at any byte offset and is read bytewise.
template <int DT, int OP>
__device__ __forceinline__ float finish_spherical(float ip, const uint8_t* x, const uint8_t* y, uint32_t dim,
                                                  const SqParams& sq) {
    constexpr float off = (float)((1 << sq_bits(DT)) - 1) / 2.0f;
    const uint32_t cb = sq_code_bytes(DT, dim);
    const float D = (float)dim;
    const float cy = load_f16_unaligned(y + cb), my = load_f16_unaligned(y + cb + 2);
    const float sy = (float)load_u16_unaligned(y + cb + 4);
    float k, ms;
    if (DT == DT_SPH1T || sq.k != 0.0f) {
        const uint8_t* m = x + (DT == DT_SPH1T ? sph_plane_bytes(dim) : cb);
        const float cq = load_f32_unaligned(m), sq_sum = load_f32_unaligned(m + 4), qoff = load_f32_unaligned(m + 8),
                    mq = load_f32_unaligned(m + 12);
        k = (cy * cq) * (((ip - off * sq_sum) + qoff * sy) - (off * qoff) * D);
        if constexpr (OP == OP_L2) return (my + mq) - 2.0f * k;
        ms = (k + my) + mq;
    } else {
        const float cx = load_f16_unaligned(x + cb), mx = load_f16_unaligned(x + cb + 2);
        const float sx = (float)load_u16_unaligned(x + cb + 4);
        k = (cx * cy) * ((ip - off * (sx + sy)) + (off * off) * D);
        if constexpr (OP == OP_L2) return (mx + my) - 2.0f * k;
        ms = (mx + my) + k;
    }
    const float r = ms + sq.shift_norm_sq;
    return OP == OP_IP ? -r : 1.0f - r;
}

// MinMax rows: the raw inner product of the codes -> SimilarityScore (minmax/vectors.rs: kernel :206-229, MinMaxL2Squared /
// MinMaxIP / MinMaxCosine / MinMaxCosineNormalized :231-473), each f32 operation on its own and in the reference's
// association.  NOT symmetric in its arguments: (t0 + x.n * y.b) + y.n * x.b rounds differently when x and y swap, so
// `x` must be the reference's first argument (the query; in prunes the candidate under test) and `y` its second.  The
// headers are 4-byte aligned (image starts are 16-byte aligned in global memory, slot + 12 in LDS).
// minmax_value is the one statement of the kernel's five operations, on header values: finish_minmax reads them from two
// images, the multi-vector kernels (maxsim_mm_kernels.hip) from their own header records.
__device__ __forceinline__ float minmax_value(float raw, float xb, float xn, float xa, float yb, float yn, float ya,
                                              uint32_t dim) {
    const float t0 = (xa * ya) * raw;
    return ((t0 + xn * yb) + yn * xb) + (xb * yb) * (float)dim;
}
template <int OP, bool NORM>
__device__ __forceinline__ float finish_minmax(float raw, const uint8_t* x, const uint8_t* y, uint32_t dim) {
    const float* hx = reinterpret_cast<const float*>(x);
    const float* hy = reinterpret_cast<const float*>(y);
    const float xb = hx[1], xn = hx[2], xa = hx[3], xs = hx[4];
    const float yb = hy[1], yn = hy[2], ya = hy[3], ys = hy[4];
    const float vv = minmax_value(raw, xb, xn, xa, yb, yn, ya, dim);
    if constexpr (OP == OP_L2) return (-2.0f * vv + xs) + ys;
    else if constexpr (OP == OP_COS) return 1.0f - vv / (__builtin_sqrtf(xs) * __builtin_sqrtf(ys));  // no zero-norm guard
    else return NORM ? 1.0f - vv : -vv;
}

// raw kernel result -> SimilarityScore.  Full-precision rows: PostOp; scalar-quantised rows: the compensated
// epilogues of diskann-quantization/src/scalar/vectors.rs:216-245 (L2), :306-370 (IP),
// :403-465 (CosineNormalized); `x`, `y` are the two rows (code bytes + trailing f32 compensation, which sits at
// the code-byte count: `dim` for SQ-8, ceil(dim * bits / 8) for the packed widths).
template <int DT, int OP, bool NORM>
__device__ __forceinline__ float finish_distance(float raw, const uint8_t* x, const uint8_t* y, uint32_t dim,
                                                 const SqParams& sq) {
    if constexpr (dt_mm_rows(DT)) {
        return finish_minmax<OP, NORM>(raw, x, y, dim);
    } else if constexpr (dt_is_sph(DT)) {
        return finish_spherical<DT, OP>(raw, x, y, dim, sq);
    } else if constexpr (!dt_is_sq(DT)) {
        return post_op<OP, NORM>(raw);
    } else if constexpr (OP == OP_L2) {
        const float l2 = sq.k * raw;
        if (!NORM) return l2;
        const float sim = 1.0f - l2 / 2.0f;
        return 1.0f - sim;
    } else {
        const uint32_t cb = sq_code_bytes(DT, dim);
        const float cx = load_f32_unaligned(x + cb), cy = load_f32_unaligned(y + cb);
        const float r = __builtin_fmaf(sq.k, raw, sq.shift_norm_sq) + (cy + cx);
        return -r;
    }
}

}  // namespace dann
