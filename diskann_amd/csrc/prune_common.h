// prune_common.h -- device and host helpers shared by the translation units that run RobustPrune's row kernels
// (build_kernels.hip: insert / back-edge / pool prunes; consolidate.hip: the pool gather of graph consolidation).
#pragma once

#include "dann_device.h"
#include "dann_internal.h"

namespace dann {
namespace {

constexpr int kWave = 64;

// d(loc, pid[r]) for r < cnt into pd[r], one G-lane distance group per candidate (the search path's bit-exact groups)
template <int DT, int OP, bool NORM>
__device__ void fill_list_distances(const IndexView& ix, uint32_t loc, uint32_t* pid, float* pd, uint32_t cnt) {
    using S = Scheme<DT, OP, true>;
    using RT = typename RowType<DT>::type;
    constexpr int G = S::G, GROUPS = kWave / G;
    const uint32_t lane = threadIdx.x;
    const int g = lane / G, v = lane % G;
    const RT* x = reinterpret_cast<const RT*>(ix.rows + (uint64_t)loc * ix.row_stride);
    for (uint32_t r0 = 0; r0 < cnt; r0 += GROUPS) {
        const uint32_t r = r0 + g;
        if (r < cnt) {
            const uint8_t* y = ix.rows + (uint64_t)pid[r] * ix.row_stride;
            float d = finish_distance<DT, OP, NORM>(group_distance_rows<DT, OP>(reinterpret_cast<const uint8_t*>(x), y, (int)ix.dim, v),
                                                    reinterpret_cast<const uint8_t*>(x), y, ix.dim,
                                                    SqParams{ix.sq_k, ix.sq_shift_norm_sq});
            if (v == 0) pd[r] = d;
        }
    }
}

// Launcher<DT, OP, NORM>::run for the index's row type and metric (DANN_LAUNCHER below defines a Launcher per kernel)
template <template <int, int, bool> class Launcher, class Args>
int32_t dispatch(const IndexView& ix, const Args& a, uint32_t grid, size_t lds, hipStream_t stream) {
    int op;
    bool norm;
    if (!resolve_metric(ix.dtype, ix.metric, &op, &norm)) {
        set_error("metric %d is not defined for dtype %d", ix.metric, ix.dtype);
        return DANN_EUNSUPPORTED;
    }
#define DANN_CASE(DT)                                                                                  \
    case DT:                                                                                           \
        if (op == OP_L2) {                                                                             \
            if constexpr (dt_is_sq(DT)) {                                                              \
                if (norm) return Launcher<DT, OP_L2, true>::run(a, grid, lds, stream);                 \
            }                                                                                          \
            return Launcher<DT, OP_L2, false>::run(a, grid, lds, stream);                              \
        }                                                                                              \
        if (op == OP_IP) {                                                                             \
            if constexpr (DT == DT_F32 || DT == DT_F16 || dt_is_mm(DT)) {                              \
                if (norm) return Launcher<DT, OP_IP, true>::run(a, grid, lds, stream);                 \
            }                                                                                          \
            return Launcher<DT, OP_IP, false>::run(a, grid, lds, stream);                              \
        }                                                                                              \
        if constexpr (!dt_is_sq(DT)) return Launcher<DT, OP_COS, false>::run(a, grid, lds, stream);     \
        return DANN_EUNSUPPORTED;
    switch (ix.dtype) {
        DANN_CASE(DT_F32)
        DANN_CASE(DT_F16)
        DANN_CASE(DT_U8)
        DANN_CASE(DT_I8)
        DANN_CASE(DT_SQ8)
        DANN_CASE(DT_SQ4)
        DANN_CASE(DT_SQ1)
        DANN_CASE(DT_SPH4)
        DANN_CASE(DT_SPH2)
        DANN_CASE(DT_SPH1)
        DANN_CASE(DT_MM8)
        DANN_CASE(DT_MM4)
        DANN_CASE(DT_MM2)
        DANN_CASE(DT_MM1)
    }
#undef DANN_CASE
    set_error("bad dtype %d", ix.dtype);
    return DANN_EINVAL;
}

#define DANN_LAUNCHER(NAME, KERNEL, ARGS)                                                          \
    template <int DT, int OP, bool NORM>                                                           \
    struct NAME {                                                                                  \
        static int32_t run(const ARGS& a, uint32_t grid, size_t lds, hipStream_t stream) {         \
            auto kern = KERNEL<DT, OP, NORM>;                                                      \
            if (lds > 64 * 1024) {                                                                 \
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),            \
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
                if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute");                    \
            }                                                                                      \
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kWave), lds, stream, a);                     \
            hipError_t e = hipGetLastError();                                                      \
            if (e != hipSuccess) return hip_fail(e, #KERNEL " launch");                            \
            return DANN_OK;                                                                        \
        }                                                                                          \
    };
}  // namespace
}  // namespace dann
