// gram_tiles.h -- the Gram tile kernel of the matrix-core prune as the other build units see it (gram_tiles.hip).
#pragma once

#include <algorithm>

#include "dann_device.h"
#include "dann_internal.h"

namespace dann {

struct TileArgs {
    IndexView ix;
    const uint32_t* sid;  // n x pcap sorted candidate ids (pool_sort_kernel)
    const uint32_t* sn;   // n
    uint32_t pcap;
    uint32_t ng, mg;      // Gram rows / columns per item: multiples of 32, ng <= 256, mg <= 96
    float* gram;          // n x ng x mg, entry (p, q) valid for q < p (and on the diagonal blocks)
    float* nrm;           // n x ng
    unsigned long long* counters;  // PruneCfg::counters: [2] += rows, [3] += tiles * 1024 (x dim x 2 = MFMA flop)
    const uint32_t* order = nullptr;  // optional: workgroup b works on item order[b] (longest lists first)
};

constexpr int kTileRowBlocks = 8;  // ng <= 256: wave w of the 8-wave workgroup owns row block w
constexpr int kTileColBlocks = 3;  // mg <= 96

// rows of one LDS slab: the fill writes whole passes of 64 rows
__host__ __device__ inline uint32_t tile_slab_rows(uint32_t ng) { return (ng + 63u) & ~63u; }
// columns of a Gram block: a multiple of 32 in [32, 96]
inline uint32_t clamp_gram_cols(uint32_t mg) {
    return std::min<uint32_t>(std::max<uint32_t>((mg + 31u) & ~31u, 32u), 32u * kTileColBlocks);
}

// f16_mfma: f16 rows through v_mfma_f32_32x32x16_f16 (the default) instead of widened through the f32 matrix core
// (DANN_DBG_GRAM_F16_WIDEN: the round-3 form, whose entries are the reference's FMA chain bit for bit)
int32_t launch_gram_tiles(const TileArgs& a, uint32_t grid, hipStream_t stream, bool f16_mfma);
// order[0..m): the items in descending order of sn[] (lpt_order_kernel)
void launch_lpt_order(const uint32_t* sn, uint32_t m, uint32_t* order, hipStream_t stream);

}  // namespace dann
