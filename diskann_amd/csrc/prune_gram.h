// prune_gram.h -- the matrix-core prune as build_batch.hip drives it (prune_gram.hip): a sort step that leaves the sorted
// candidate lists of `m` items in the scratch (g_sid / g_sd / g_sn, sized by the caller with ensure_gram_scratch), then
// Gram tiles + sweep over them.
#pragma once

#include "build_common.h"
#include "build_scratch.h"
#include "gram_tiles.h"

namespace dann {

// the rows the matrix-core prune is defined for: f32 / f16, L2 / inner product / cosine-normalized
inline bool gram_float_rows(const IndexView& ix) { return (ix.dtype == DT_F32 || ix.dtype == DT_F16) && ix.metric != M_COSINE; }
// tuning hook: DANN_DBG_GRAM_COLS (32 / 64 / 96)
inline uint32_t gram_cols(const dann_index* idx) { return clamp_gram_cols(idx->dbg_u32(DANN_DBG_GRAM_COLS, 96u)); }

// sort step of a pool prune: pool_sort_kernel over the pools of `p` (pool + intra-batch extras -> SortedNeighbors::new)
int32_t launch_pool_sort(BuildScratch& s, const PoolArgs& p, uint32_t m, hipStream_t st);
// sort step of the back-edge prunes: backedge_list_kernel over the m targets of b.work (appends where the list still
// fits; the target of item i goes to g_loc[i])
int32_t launch_backedge_list(BuildScratch& s, const BackArgs& b, uint32_t m, hipStream_t st);
// The rest of the pipeline, on the index stream, from "the sorted lists of m items are in g_sid / g_sd / g_sn": the order
// of the workgroups (longest lists first), the Gram tiles (ng x mg per item, between the tile clock's events) and the
// sweep.  `p` is what the sweep reads of a PoolArgs: ix, cfg, pcap and force_saturate, and for a pool prune locs, pos0,
// out and out_stride.  out_loc: null = pool prune; otherwise item i is the list of out_loc[i] and the result goes
// straight into that adjacency row.
int32_t gram_tiles_and_sweep(dann_index* idx, BuildScratch& s, const PoolArgs& p, uint32_t m, uint32_t ng, uint32_t mg,
                             const uint32_t* out_loc);

}  // namespace dann
