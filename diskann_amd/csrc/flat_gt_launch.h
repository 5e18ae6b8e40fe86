// flat_gt_kernels.hip: the exhaustive scan under a filter (bitmaps over slot ids, `stride` words apart, 0: one for all)
// and the range scan (d_filter null: every slot matches), cut up as flat_gt_plan.h says.  One call serves at most the
// plan's batch of queries; d_deleted: the deleted bitmap when it is to be honoured, else null.
#pragma once
#include "dann_internal.h"
#include "flat_gt_plan.h"

namespace dann {

int32_t launch_flat_filtered_search(const IndexView& ix, const FlatFilteredPlan& plan, const void* d_queries, uint32_t nq,
                                    uint32_t first, uint32_t n, const uint32_t* d_deleted, const uint32_t* d_filter,
                                    uint64_t stride, void* scratch, uint32_t* d_ids, float* d_dists,
                                    dann_search_stats* d_stats, hipStream_t stream);
int32_t launch_flat_range_search(const IndexView& ix, const FlatRangePlan& plan, const void* d_queries, uint32_t nq,
                                 uint32_t first, uint32_t n, float radius, bool has_inner, float inner_radius,
                                 const uint32_t* d_deleted, const uint32_t* d_filter, uint64_t stride, uint32_t out_cap,
                                 void* scratch, uint32_t* d_ids, float* d_dists, uint32_t* d_counts,
                                 dann_search_stats* d_stats, hipStream_t stream);

}  // namespace dann
