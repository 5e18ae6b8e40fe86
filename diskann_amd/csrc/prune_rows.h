// prune_rows.h -- the row-kernel prunes and the graph-update kernels of a batched insert as build_batch.hip launches them
// (prune_rows.hip holds the kernels; no other unit instantiates them).
#pragma once

#include "build_common.h"

namespace dann {

// robust_prune_list over explicit candidate lists (bootstrap: list = own edges ∪ other batch members; index.rs:597-645)
struct ListArgs {
    IndexView ix;
    PruneCfg cfg;
    const uint32_t* locs;
    const uint32_t* pending;  // n x pend_stride: [len, ids...] current edges of each item
    uint32_t pend_stride;
    uint32_t n;
    uint32_t pcap;
    uint32_t* out;
    uint32_t out_stride;
    uint32_t* err;
};

// every distinct target of the batch, one wave each: append the new sources if the list still fits
// (provider.rs:795-822), otherwise queue the target for a prune kernel.  No distances, 1 KiB of LDS: this is the
// launch that covers ~10^6 targets per batch, the prune kernels only see the few percent that overflow.
struct ScanArgs {
    IndexView ix;
    uint32_t cfg_max_degree;   // "max_degree_with_slack": a list longer than this is pruned
    const uint64_t* keys;
    const uint32_t* seg_start;
    const uint32_t* seg_len;
    uint32_t nseg;
    uint32_t short_cap;        // lists up to this length go to work_short, longer ones to work_long
    uint32_t* work_short;
    uint32_t* work_long;
    uint32_t* counts;          // [0] #short [1] #long [2] longest list among the long ones
    uint32_t rank = 0, world = 1;  // owner-partitioned commit: only targets with id % world == rank are queued here
};

// One wavefront per item, the LDS pool sized by the arguments' pcap, for the index's row type and metric.
int32_t launch_pool_prune(const PoolArgs& a, uint32_t items, hipStream_t st);  // pool_prune_kernel
int32_t launch_bootstrap(const ListArgs& a, hipStream_t st);                   // bootstrap_kernel, a.n items
int32_t launch_backedge(const BackArgs& a, hipStream_t st);                    // backedge_kernel, a.nseg targets
void launch_backedge_scan(const ScanArgs& a, hipStream_t st);                  // backedge_scan_kernel, four targets per wave
void launch_export_rows(const IndexView& ix, const uint64_t* keys, const uint32_t* seg_start, const uint32_t* work_short,
                        uint32_t nshort, const uint32_t* work_long, uint32_t nlong, uint32_t* out, hipStream_t st);
void launch_apply_rows(const IndexView& ix, const uint32_t* rows, uint32_t count, hipStream_t st);
// keys[item * degree + e] = (neighbour e of item) << 32 | locs[item] for e < limit, ~0 otherwise
void launch_make_keys(const uint32_t* locs, const uint32_t* pending, uint32_t pend_stride, uint32_t n, uint32_t degree,
                      uint64_t* keys, uint32_t limit, hipStream_t st);
// the segments (one per distinct target) of the sorted keys and their lengths: meta[0] #segments, [1] #valid keys, [2] longest
void launch_segments(const uint64_t* keys, uint32_t total, uint32_t* seg_start, uint32_t* seg_len, uint32_t* meta, hipStream_t st);
void launch_set_bulk(const IndexView& ix, const uint32_t* locs, const uint32_t* pending, uint32_t pend_stride, uint32_t n,
                     hipStream_t st);

}  // namespace dann
