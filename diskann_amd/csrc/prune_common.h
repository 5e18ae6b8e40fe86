// prune_common.h -- device and host helpers shared by the translation units that run RobustPrune's row kernels
// (prune_rows.hip, prune_gram.hip: insert / back-edge / pool prunes; consolidate.hip: the pool gather of graph consolidation).
#pragma once

#include "dann_device.h"
#include "dann_internal.h"
#include "wave_lists.h"

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

// A row kernel's instantiation as a type.  The translation units name each kernel template once, in a generic lambda
// from a RowOp to its KernelOf, e.g.
//     constexpr auto kPoolPrune = [](auto r) { using R = decltype(r); return KernelOf<pool_prune_kernel<R::dt, R::op, R::norm>>{}; };
template <auto Kern>
struct KernelOf {
    static constexpr auto fn = Kern;
};

// launch `kernel`'s instantiation for the index's row type and metric, one wavefront per block, with `a` as its argument
template <class Kernel, class Args>
int32_t launch_rows(const IndexView& ix, Kernel kernel, const char* what, const Args& a, uint32_t grid, size_t lds,
                    hipStream_t stream) {
    const int32_t rc = dispatch_row_op<kRowsStored>(ix.dtype, ix.metric, [&](auto r) {
        return launch_kernel<decltype(kernel(r))::fn>(what, dim3(grid), dim3(kWave), lds, stream, a);
    });
    if (rc != kNoRow) return rc;
    set_error("bad dtype %d", ix.dtype);
    return DANN_EINVAL;
}
}  // namespace
}  // namespace dann
