// How dann_search_batch (host_search.hip) moves a call's host buffers: a pure function of the row type, the debug knobs,
// the batch and the caller's pinning.  No HIP here: tests/test_host_plan_host.py compiles it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/dann.h"
#include "small_calls.h"

namespace dann {
constexpr uint32_t kMaxLanes = 8, kDefaultLanes = 3;
constexpr size_t kRingBytes = (size_t)1 << 20;  // Single: the pinned ring carries calls of up to this many bytes in + out

// Small: one launch on mapped staging shared with other threads' small calls (small_calls.h; declined: Single).
// Single: one pass, copy in / search / copy out.  ZeroCopy: the kernel reads and writes page-locked, mapped caller
// buffers.  Lanes: two chunks and more, up to kMaxLanes contexts and threads take the chunks round robin.
enum class HostStrategy { Small, Single, ZeroCopy, Lanes };

struct HostPlanIn {
    int32_t dtype;
    uint32_t pipeline;    // DANN_DBG_HOST_PIPELINE: 0 never chunk, 1 default, 2 .. 8 lanes (and no temporary page-locking)
    uint32_t host_chunk;  // DANN_DBG_HOST_CHUNK: queries per chunk (at least 256)
    uint32_t nq, k;
    size_t qb;            // bytes per query
    // page-locked by the caller, asked only when host_chunked(); no statistics buffer counts as pinned
    bool q_pinned, ids_pinned, dists_pinned, stats_pinned;
};

struct HostPlan {
    HostStrategy strategy;
    bool ring;                  // Single: through the pinned ring (else hipMemcpyAsync from / to the caller's buffers)
    bool may_register;          // Lanes: temporary page-locking of buffers seen before may turn it into ZeroCopy
    bool q_direct, o_direct;    // Lanes: queries / ids and distances are the caller's page-locked memory (no ring)
    uint32_t cq, lanes;         // queries per device pass; lanes wanted
    size_t in_b, ids_b, out_b;  // device staging of one pass: queries | ids | distances | statistics (16-byte aligned)
};

inline bool host_chunked(uint32_t pipeline, uint32_t host_chunk, uint32_t nq) {
    return pipeline != 0u && nq >= 2 * std::max(host_chunk, 256u);
}
// rows whose kernels read a query once, when its wavefront stages it (PQ builds a table from it, SQ-8 a compensation)
inline bool zero_copy_rows(int32_t dtype) {
    return dtype == DANN_F32 || dtype == DANN_F16 || dtype == DANN_U8 || dtype == DANN_I8;
}

inline HostPlan plan_host_search(const HostPlanIn& in) {
    HostPlan p{};
    const bool chunked = host_chunked(in.pipeline, in.host_chunk, in.nq);
    p.cq = chunked ? std::max(in.host_chunk, 256u) : in.nq;
    p.ids_b = ((size_t)p.cq * in.k * 4 + 15) & ~(size_t)15;
    p.in_b = (size_t)p.cq * in.qb;
    p.out_b = 2 * p.ids_b + (((size_t)p.cq * sizeof(dann_search_stats) + 15) & ~(size_t)15);
    if (!chunked) {
        const bool small = in.pipeline == 1u && in.nq <= kSmallCall && small_call_bytes(in.nq, in.qb, in.k) <= kSmallStage / 4;
        p.strategy = small ? HostStrategy::Small : HostStrategy::Single;
        p.ring = p.in_b + p.out_b <= kRingBytes;
        return p;
    }
    p.lanes = std::min((in.nq + p.cq - 1) / p.cq, in.pipeline >= 2u ? std::min(in.pipeline, kMaxLanes) : kDefaultLanes);
    p.q_direct = in.q_pinned;
    p.o_direct = in.ids_pinned && in.dists_pinned;
    const bool zc = zero_copy_rows(in.dtype);
    p.strategy = zc && p.q_direct && p.o_direct && in.stats_pinned ? HostStrategy::ZeroCopy : HostStrategy::Lanes;
    p.may_register = p.strategy == HostStrategy::Lanes && zc && in.pipeline == 1u;
    return p;
}
}  // namespace dann
