// api_mvset.hip -- multi-vector sets (maxsim_kernels.hip): dann_mvset_*, dann_maxsim_* and dann_chamfer_* of
// include/dann.h.  A set never touches a dann_index.
// Rows are kept at a stride of whole 16-byte units with the tail zeroed -- the layout the kernels stage from -- and the
// queries of a call are brought to the same stride on their way to the device.  MinMax sets (maxsim_mm_kernels.hip): the
// rows are canonical images on the way in; the device keeps their packed codes at such a stride and a header record per row.
#include <atomic>
#include <memory>

#include "api_common.h"

using namespace dann;

extern "C" {

struct dann_mvset {
    int device = 0;
    int32_t dtype = 0;
    std::atomic<int32_t> qdtype{0};           // dann_mvset_set_query_dtype; read once at the entry of a scoring call
    uint32_t dim = 0, ndocs = 0, stride = 0;  // stride: bytes of a row on the device
    uint64_t nrows = 0;
    uint8_t* d_rows = nullptr;
    dann::MmRowHeader* d_hdr = nullptr;       // MinMax sets only
    uint64_t* d_off = nullptr;
    // HIP-event time of the scoring launches (dann_debug_mvset_kernel_time); clock_mu also keeps one call's pair of
    // events to itself
    mutable std::mutex clock_mu;
    mutable hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mutable dann::KernelClock clock;
    ~dann_mvset() {
        if (d_rows) (void)hipFree(d_rows);
        if (d_hdr) (void)hipFree(d_hdr);
        if (d_off) (void)hipFree(d_off);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

namespace {
// packed rows (host or device) -> rows at `stride` on the device, tails zero
int32_t mv_copy_rows(uint8_t* d_dst, uint32_t stride, const void* src, uint32_t row_bytes, uint64_t nrows, bool src_device) {
    if (nrows == 0) return DANN_OK;
    if (stride != row_bytes) DANN_HIP(hipMemset(d_dst, 0, (size_t)nrows * stride));
    DANN_HIP(hipMemcpy2D(d_dst, stride, src, row_bytes, row_bytes, (size_t)nrows,
                         src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return DANN_OK;
}

// bytes of a row on the device: f32 / f16 elements, or a MinMax row's packed codes, in whole 16-byte units
uint32_t mv_stride(int32_t dtype, uint32_t dim) {
    const uint32_t row_bytes = dt_is_mm(dtype) ? sq_code_bytes(dtype, dim) : dim * (dtype == DT_F32 ? 4u : 2u);
    return (row_bytes + 15u) & ~15u;
}

// packed MinMax images (host or device) -> codes at `stride` and header records on the device
int32_t mv_repack_rows(int32_t dtype, uint32_t dim, uint8_t* d_codes, uint32_t stride, MmRowHeader* d_hdr, const void* src,
                       uint64_t nrows, bool src_device) {
    if (nrows == 0) return DANN_OK;
    const uint32_t image_bytes = layer_bytes_of(dtype, dim);
    DevBuf img;
    const uint8_t* d_src = static_cast<const uint8_t*>(src);
    if (!src_device) {
        DANN_HIP(img.alloc((size_t)nrows * image_bytes));
        DANN_HIP(hipMemcpy(img.p, src, (size_t)nrows * image_bytes, hipMemcpyHostToDevice));
        d_src = img.as<uint8_t>();
    }
    if (int32_t rc = launch_mm_repack(dtype, d_src, image_bytes, nrows, dim, d_codes, stride, d_hdr, nullptr)) return rc;
    DANN_HIP(hipStreamSynchronize(nullptr));  // (`img` is freed on return)
    return DANN_OK;
}

// the arguments of one scoring call, on the device
struct MvCall {
    DevBuf q, qhdr, qoff, cand, status;
    int32_t qdtype = 0;
    std::vector<uint32_t> h_qoff;
    MaxSimArgs a{};
    uint64_t qrows_total = 0;
};

int32_t mv_prepare(const dann_mvset* s, int32_t order, const void* queries, const uint32_t* q_offsets, uint32_t nq,
                   const uint32_t* cand, uint32_t cand_stride, bool on_device, MvCall& c) {
    if (order != DANN_MAXSIM_KERNEL && order != DANN_MAXSIM_REFERENCE) {
        set_error("order %d is not a DANN_MAXSIM_* value", order);
        return DANN_EINVAL;
    }
    if (!q_offsets || !cand) return DANN_EINVAL;
    if (cand_stride == 0 || cand_stride > kMaxSimCands) {
        set_error("multi-vector scoring supports 1..%u candidates per query (got %u)", kMaxSimCands, cand_stride);
        return DANN_EUNSUPPORTED;
    }
    if (nq > kMaxSimQueries) {
        set_error("multi-vector scoring supports %u queries per call (got %u)", kMaxSimQueries, nq);
        return DANN_EUNSUPPORTED;
    }
    c.h_qoff.resize((size_t)nq + 1);
    if (on_device) DANN_HIP(hipMemcpy(c.h_qoff.data(), q_offsets, ((size_t)nq + 1) * 4, hipMemcpyDeviceToHost));
    else memcpy(c.h_qoff.data(), q_offsets, ((size_t)nq + 1) * 4);
    if (c.h_qoff[0] != 0) {
        set_error("q_offsets[0] is %u, not 0", c.h_qoff[0]);
        return DANN_ELENGTH;
    }
    for (uint32_t q = 0; q < nq; ++q) {
        if (c.h_qoff[q + 1] < c.h_qoff[q]) {
            set_error("q_offsets decrease at query %u", q);
            return DANN_ELENGTH;
        }
        if (c.h_qoff[q + 1] - c.h_qoff[q] > kMaxSimQueryRows) {
            set_error("query %u has %u rows: the supported maximum is %u", q, c.h_qoff[q + 1] - c.h_qoff[q], kMaxSimQueryRows);
            return DANN_EUNSUPPORTED;
        }
    }
    c.qrows_total = c.h_qoff[nq];
    if (c.qrows_total && !queries) return DANN_EINVAL;
    c.qdtype = s->qdtype.load();
    const uint32_t qstride = mv_stride(c.qdtype, s->dim);
    DANN_HIP(c.q.alloc((size_t)c.qrows_total * qstride + 16));
    if (dt_is_mm(s->dtype)) {
        DANN_HIP(c.qhdr.alloc(((size_t)c.qrows_total + 1) * sizeof(MmRowHeader)));
        if (int32_t rc = mv_repack_rows(c.qdtype, s->dim, c.q.as<uint8_t>(), qstride, c.qhdr.as<MmRowHeader>(), queries,
                                        c.qrows_total, on_device))
            return rc;
    } else {
        const uint32_t row_bytes = s->dim * (s->dtype == DT_F32 ? 4u : 2u);
        if (int32_t rc = mv_copy_rows(c.q.as<uint8_t>(), qstride, queries, row_bytes, c.qrows_total, on_device)) return rc;
    }
    DANN_HIP(c.status.alloc(4));
    DANN_HIP(hipMemset(c.status.p, 0, 4));
    if (!on_device) {
        DANN_HIP(c.qoff.alloc(((size_t)nq + 1) * 4));
        DANN_HIP(c.cand.alloc((size_t)nq * cand_stride * 4));
        DANN_HIP(hipMemcpy(c.qoff.p, q_offsets, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice));
        DANN_HIP(hipMemcpy(c.cand.p, cand, (size_t)nq * cand_stride * 4, hipMemcpyHostToDevice));
    }
    c.a.drows = s->d_rows;
    c.a.doff = s->d_off;
    c.a.ndocs = s->ndocs;
    c.a.dim = s->dim;
    c.a.stride = s->stride;
    c.a.qstride = qstride;
    c.a.dhdr = s->d_hdr;
    c.a.qhdr = c.qhdr.as<MmRowHeader>();
    c.a.qrows = c.q.as<uint8_t>();
    c.a.qoff = on_device ? q_offsets : c.qoff.as<uint32_t>();
    c.a.cand = on_device ? cand : c.cand.as<uint32_t>();
    c.a.cand_stride = cand_stride;
    c.a.status = c.status.as<uint32_t>();
    return DANN_OK;
}

// launch, wait, and turn the device's bounds check into the status
int32_t mv_score(const dann_mvset* s, int32_t order, MvCall& c, uint32_t nq, float* d_chamfer, float* d_scores) {
    c.a.out_chamfer = d_chamfer;
    c.a.out_scores = d_scores;
    std::lock_guard<std::mutex> lk(s->clock_mu);
    DANN_HIP(hipEventRecord(s->ev0, nullptr));
    if (int32_t rc = dt_is_mm(s->dtype) ? launch_maxsim_mm(c.qdtype, s->dtype, order, c.a, nq, nullptr)
                                        : launch_maxsim(s->dtype, order, c.a, nq, nullptr))
        return rc;
    DANN_HIP(hipEventRecord(s->ev1, nullptr));
    uint32_t st = 0;
    DANN_HIP(hipMemcpy(&st, c.status.p, 4, hipMemcpyDeviceToHost));  // (waits for the launch)
    float ms = 0.f;
    DANN_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->clock.total_ms += ms;
    s->clock.launches += 1;
    if (st) {
        set_error("a candidate id is not below the set's %u documents", s->ndocs);
        return DANN_EBOUNDS;
    }
    return DANN_OK;
}

int32_t mv_maxsim(const dann_mvset* s, int32_t order, const void* queries, const uint32_t* q_offsets, uint32_t nq,
                  const uint32_t* cand, uint32_t cand_stride, float* out_chamfer, float* out_scores, bool on_device) {
    if (!s || !out_chamfer) return DANN_EINVAL;
    DeviceGuard dev(s->device);
    if (!dev.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    MvCall c;
    if (int32_t rc = mv_prepare(s, order, queries, q_offsets, nq, cand, cand_stride, on_device, c)) return rc;
    if (nq == 0) return DANN_OK;
    if (on_device) return mv_score(s, order, c, nq, out_chamfer, out_scores);
    const size_t cb = (size_t)nq * cand_stride * 4, sb = (size_t)c.qrows_total * cand_stride * 4;
    DevBuf bc, bs;
    DANN_HIP(bc.alloc(cb));
    if (out_scores) DANN_HIP(bs.alloc(sb));
    if (int32_t rc = mv_score(s, order, c, nq, bc.as<float>(), out_scores ? bs.as<float>() : nullptr)) return rc;
    DANN_HIP(hipMemcpy(out_chamfer, bc.p, cb, hipMemcpyDeviceToHost));
    if (out_scores && sb) DANN_HIP(hipMemcpy(out_scores, bs.p, sb, hipMemcpyDeviceToHost));
    return DANN_OK;
}

int32_t mv_rerank(const dann_mvset* s, int32_t order, const void* queries, const uint32_t* q_offsets, uint32_t nq,
                  const uint32_t* cand, uint32_t cand_stride, uint32_t k, uint32_t* out_ids, float* out_dists,
                  uint32_t* out_counts, bool on_device) {
    if (!s || !out_ids || !out_dists || !out_counts || k == 0) return DANN_EINVAL;
    DeviceGuard dev(s->device);
    if (!dev.ok) return hip_fail(hipErrorInvalidDevice, "hipSetDevice");
    MvCall c;
    if (int32_t rc = mv_prepare(s, order, queries, q_offsets, nq, cand, cand_stride, on_device, c)) return rc;
    if (nq == 0) return DANN_OK;
    DevBuf bc, bi, bd, bn;
    DANN_HIP(bc.alloc((size_t)nq * cand_stride * 4));
    if (int32_t rc = mv_score(s, order, c, nq, bc.as<float>(), nullptr)) return rc;
    const size_t ob = (size_t)nq * k * 4;
    uint32_t* d_ids = out_ids;
    float* d_d = out_dists;
    uint32_t* d_n = out_counts;
    if (!on_device) {
        DANN_HIP(bi.alloc(ob));
        DANN_HIP(bd.alloc(ob));
        DANN_HIP(bn.alloc((size_t)nq * 4));
        d_ids = bi.as<uint32_t>(), d_d = bd.as<float>(), d_n = bn.as<uint32_t>();
    }
    if (int32_t rc = launch_chamfer_sort(c.a.cand, bc.as<float>(), nq, cand_stride, s->ndocs, k, d_ids, d_d, d_n, nullptr))
        return rc;
    if (!on_device) {
        DANN_HIP(hipMemcpy(out_ids, bi.p, ob, hipMemcpyDeviceToHost));
        DANN_HIP(hipMemcpy(out_dists, bd.p, ob, hipMemcpyDeviceToHost));
        DANN_HIP(hipMemcpy(out_counts, bn.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    } else {
        DANN_HIP(hipStreamSynchronize(nullptr));
    }
    return DANN_OK;
}
}  // namespace

int32_t dann_mvset_create(int32_t device, int32_t dtype, uint32_t dim, uint32_t ndocs, const uint64_t* row_offsets,
                          const void* rows, dann_mvset** out) try {
    if (!out) return DANN_EINVAL;
    *out = nullptr;
    if (!row_offsets) return DANN_EINVAL;
    if (dtype != DT_F32 && dtype != DT_F16 && !dt_is_mm(dtype)) {
        set_error("multi-vector sets hold DANN_F32, DANN_F16 or DANN_MM1 / MM2 / MM4 / MM8 rows (got dtype %d)", dtype);
        return DANN_EINVAL;
    }
    if (dim == 0) {
        set_error("dim is 0");
        return DANN_EINVAL;
    }
    if (dim > kMaxSimDim) {
        set_error("dim %u exceeds the supported maximum of %u", dim, kMaxSimDim);
        return DANN_EUNSUPPORTED;
    }
    if (row_offsets[0] != 0) {
        set_error("row_offsets[0] is %llu, not 0", (unsigned long long)row_offsets[0]);
        return DANN_ELENGTH;
    }
    for (uint32_t d = 0; d < ndocs; ++d)
        if (row_offsets[d + 1] < row_offsets[d]) {
            set_error("row_offsets decrease at document %u", d);
            return DANN_ELENGTH;
        }
    const uint64_t nrows = row_offsets[ndocs];
    if (nrows && !rows) return DANN_EINVAL;
    std::unique_ptr<dann_mvset> s(new dann_mvset());
    if (device >= 0) DANN_HIP(hipSetDevice(device));
    DANN_HIP(hipGetDevice(&s->device));
    s->dtype = dtype;
    s->qdtype = dtype;
    s->dim = dim;
    s->ndocs = ndocs;
    s->nrows = nrows;
    s->stride = mv_stride(dtype, dim);
    DANN_HIP(hipEventCreate(&s->ev0));
    DANN_HIP(hipEventCreate(&s->ev1));
    DANN_HIP(hipMalloc((void**)&s->d_rows, (size_t)nrows * s->stride + 16));
    DANN_HIP(hipMalloc((void**)&s->d_off, ((size_t)ndocs + 1) * 8));
    if (dt_is_mm(dtype)) {
        DANN_HIP(hipMalloc((void**)&s->d_hdr, ((size_t)nrows + 1) * sizeof(MmRowHeader)));
        if (int32_t rc = mv_repack_rows(dtype, dim, s->d_rows, s->stride, s->d_hdr, rows, nrows, false)) return rc;
    } else {
        const uint32_t row_bytes = dim * (dtype == DT_F32 ? 4u : 2u);
        if (int32_t rc = mv_copy_rows(s->d_rows, s->stride, rows, row_bytes, nrows, false)) return rc;
    }
    DANN_HIP(hipMemcpy(s->d_off, row_offsets, ((size_t)ndocs + 1) * 8, hipMemcpyHostToDevice));
    *out = s.release();
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_mvset_destroy(dann_mvset* set) try {
    if (!set) return DANN_OK;
    DeviceGuard dev(set->device);
    delete set;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_mvset_info(const dann_mvset* set, int32_t* dtype, uint32_t* dim, uint32_t* ndocs, uint64_t* nrows) try {
    if (!set) return DANN_EINVAL;
    if (dtype) *dtype = set->dtype;
    if (dim) *dim = set->dim;
    if (ndocs) *ndocs = set->ndocs;
    if (nrows) *nrows = set->nrows;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_mvset_set_query_dtype(dann_mvset* set, int32_t dtype) try {
    if (!set) return DANN_EINVAL;
    if (dtype != set->dtype) {
        if (!dt_is_mm(set->dtype) || !dt_is_mm(dtype)) {
            set_error("query dtype %d on a multi-vector set of dtype %d: %s", dtype, set->dtype,
                      dt_is_mm(set->dtype) ? "a MinMax set takes MinMax queries" : "queries have the set's own dtype");
            return DANN_EINVAL;
        }
        if (dtype != DT_MM8) {  // the reference's mixed pairs are (8, 4), (8, 2), (8, 1) (bits/distances.rs:1621)
            set_error("MinMax queries of dtype %d on rows of dtype %d: the supported pairs are equal widths and DANN_MM8 "
                      "queries on narrower rows", dtype, set->dtype);
            return DANN_EUNSUPPORTED;
        }
    }
    set->qdtype = dtype;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_mvset_get_query_dtype(const dann_mvset* set, int32_t* out) try {
    if (!set || !out) return DANN_EINVAL;
    *out = set->qdtype.load();
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_debug_mvset_kernel_time(const dann_mvset* set, int32_t reset, double* total_ms, uint64_t* launches) try {
    if (!set) return DANN_EINVAL;
    std::lock_guard<std::mutex> lk(set->clock_mu);
    if (total_ms) *total_ms = set->clock.total_ms;
    if (launches) *launches = set->clock.launches;
    if (reset) set->clock = KernelClock{};
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_maxsim_batch(const dann_mvset* set, int32_t order, const void* queries, const uint32_t* q_offsets,
                          uint32_t nq, const uint32_t* cand_ids, uint32_t cand_stride, float* out_chamfer,
                          float* out_scores) try {
    return mv_maxsim(set, order, queries, q_offsets, nq, cand_ids, cand_stride, out_chamfer, out_scores, false);
} DANN_CATCH_ALL

int32_t dann_maxsim_batch_device(const dann_mvset* set, int32_t order, const void* d_queries, const uint32_t* d_q_offsets,
                                 uint32_t nq, const uint32_t* d_cand_ids, uint32_t cand_stride, float* d_out_chamfer,
                                 float* d_out_scores) try {
    return mv_maxsim(set, order, d_queries, d_q_offsets, nq, d_cand_ids, cand_stride, d_out_chamfer, d_out_scores, true);
} DANN_CATCH_ALL

int32_t dann_chamfer_rerank_batch(const dann_mvset* set, int32_t order, const void* queries, const uint32_t* q_offsets,
                                  uint32_t nq, const uint32_t* cand_ids, uint32_t cand_stride, uint32_t k,
                                  uint32_t* out_ids, float* out_dists, uint32_t* out_counts) try {
    return mv_rerank(set, order, queries, q_offsets, nq, cand_ids, cand_stride, k, out_ids, out_dists, out_counts, false);
} DANN_CATCH_ALL

int32_t dann_chamfer_rerank_batch_device(const dann_mvset* set, int32_t order, const void* d_queries,
                                         const uint32_t* d_q_offsets, uint32_t nq, const uint32_t* d_cand_ids,
                                         uint32_t cand_stride, uint32_t k, uint32_t* d_out_ids, float* d_out_dists,
                                         uint32_t* d_out_counts) try {
    return mv_rerank(set, order, d_queries, d_q_offsets, nq, d_cand_ids, cand_stride, k, d_out_ids, d_out_dists,
                     d_out_counts, true);
} DANN_CATCH_ALL

}  // extern "C"
