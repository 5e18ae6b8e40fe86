// api_common.h -- what the translation units of the C ABI (api_index.hip, api_search.hip, api_mvset.hip,
// api_formats.hip) share: the access macros, the dtype / metric validators, the launch clock and the staging loop.
#pragma once
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <vector>

#include "dann_device.h"
#include "dann_internal.h"
#include "host_stage.h"  // HostStage, ArenaTrim

namespace dann {

inline uint32_t elem_size(int32_t dtype) { return dtype == DT_F32 ? 4u : dtype == DT_F16 ? 2u : 1u; }
inline uint32_t layer_bytes_of(int32_t dtype, uint32_t dim) {
    if (dt_is_sq(dtype)) return sq_code_bytes(dtype, dim) + 4u;  // code bytes + the f32 compensation
    if (dt_is_sph(dtype)) return sq_code_bytes(dtype, dim) + kSphDataMeta;  // code bytes + DataMeta
    if (dt_is_mm(dtype)) return kMmHeader + sq_code_bytes(dtype, dim);     // MinMaxCompensation + code bytes
    return dim * elem_size(dtype);
}
inline bool valid_dtype(int32_t d) {
    return (d >= 0 && d <= 5) || d == DT_SQ1 || d == DT_SQ4 || d == DT_SPH1 || d == DT_SPH2 || d == DT_SPH4 ||
           dt_is_mm(d);
}
inline bool valid_metric(int32_t m) { return m >= 0 && m <= 3; }
// MinMax rows written through host pointers: the image's leading u32 is the quantiser's output_dim() and must be the
// index's dim (minmax::Data::from_raw panics on a mismatch).  Device-pointer and verbatim paths do not look.
inline bool mm_headers_ok(const dann_index* idx, const void* rows, uint64_t n, uint64_t stride) {
    if (!dt_is_mm(idx->cfg.dtype)) return true;
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t d;
        memcpy(&d, static_cast<const uint8_t*>(rows) + i * stride, 4);
        if (d != idx->cfg.dim) {
            set_error("MinMax image %llu: header dim %u does not match the index's dim %u", (unsigned long long)i, d, idx->cfg.dim);
            return false;
        }
    }
    return true;
}

// time one launch on the index stream with HIP events (the stream the kernel runs on)
template <class F>
int32_t timed(dann_index* idx, int which, F&& f) {
    DANN_HIP(hipEventRecord(idx->main.ev0, idx->main.stream));
    int32_t rc = f();
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipEventRecord(idx->main.ev1, idx->main.stream));
    DANN_HIP(hipEventSynchronize(idx->main.ev1));
    float ms = 0.f;
    DANN_HIP(hipEventElapsedTime(&ms, idx->main.ev0, idx->main.ev1));
    std::lock_guard<std::mutex> lk(idx->stat_mu);
    idx->clocks[which].total_ms += ms;
    idx->clocks[which].launches += 1;
    return DANN_OK;
}

inline int32_t pq_ready(const dann_index* idx) {
    if (idx->cfg.dtype == DT_PQ && (!idx->d_pq_pivots || !idx->d_pq_offsets)) {
        set_error("DANN_PQ index has no pivot table: call dann_set_pq_table first");
        return DANN_EINVAL;
    }
    return DANN_OK;
}

}  // namespace dann

// exclusive access: mutations and every entry point that runs on idx->main
#define CHECK_IDX(idx)                                  \
    if (!(idx)) {                                       \
        ::dann::set_error("null index");                \
        return DANN_EINVAL;                             \
    }                                                   \
    ::dann::ExclusiveGuard _lock(idx);                  \
    ::dann::DeviceGuard _guard((idx)->device)

// shared access for the Knn search entry points: the index is read-only here, every call runs on its own context `ctx`
#define CHECK_IDX_SHARED(idx)                               \
    if (!(idx)) {                                           \
        ::dann::set_error("null index");                    \
        return DANN_EINVAL;                                 \
    }                                                       \
    std::shared_lock<std::shared_mutex> _rd((idx)->rw);     \
    ::dann::DeviceGuard _guard((idx)->device);              \
    ::dann::CtxLease _lease(idx);                           \
    if (_lease.status != DANN_OK) return _lease.status;     \
    ::dann::SearchCtx& ctx = *_lease.ctx
