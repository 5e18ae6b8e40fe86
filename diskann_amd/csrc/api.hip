// api.hip -- the C ABI of include/dann.h: index lifetime, HBM layout, host<->device
// staging and kernel dispatch.  No CPU fallback exists anywhere in this library: every
// distance, search and prune result comes from a HIP kernel, and a missing/failed device
// surfaces as DANN_EHIP.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "dann_device.h"
#include "dann_internal.h"
#include "flat_plan.h"
#include "wave_lists.h"  // kTagReadable

namespace dann {

static thread_local char g_err[512] = {0};

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int32_t hip_fail(hipError_t e, const char* what) {
    set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    return DANN_EHIP;
}

static uint32_t elem_size(int32_t dtype) { return dtype == DT_F32 ? 4u : dtype == DT_F16 ? 2u : 1u; }
static uint32_t layer_bytes_of(int32_t dtype, uint32_t dim) {
    if (dt_is_sq(dtype)) return sq_code_bytes(dtype, dim) + 4u;  // code bytes + the f32 compensation
    if (dt_is_sph(dtype)) return sq_code_bytes(dtype, dim) + kSphDataMeta;  // code bytes + DataMeta
    if (dt_is_mm(dtype)) return kMmHeader + sq_code_bytes(dtype, dim);     // MinMaxCompensation + code bytes
    return dim * elem_size(dtype);
}
static bool valid_dtype(int32_t d) {
    return (d >= 0 && d <= 5) || d == DT_SQ1 || d == DT_SQ4 || d == DT_SPH1 || d == DT_SPH2 || d == DT_SPH4 ||
           dt_is_mm(d);
}
// MinMax rows written through host pointers: the image's leading u32 is the quantiser's output_dim() and must be the
// index's dim (minmax::Data::from_raw panics on a mismatch).  Device-pointer and verbatim paths do not look.
static bool mm_headers_ok(const dann_index* idx, const void* rows, uint64_t n, uint64_t stride) {
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
static bool valid_metric(int32_t m) { return m >= 0 && m <= 3; }

// a block of a context's arena, carved into 256-byte aligned pieces
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return o;
    }
};
struct ArenaPtr {
    void* p;
    ArenaPtr(void* base, size_t off) : p(reinterpret_cast<uint8_t*>(base) + off) {}
    ArenaPtr() : p(nullptr) {}
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

// time one launch on the index stream with HIP events (the stream the kernel runs on)
template <class F>
static int32_t timed(dann_index* idx, int which, F&& f) {
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

int32_t SearchCtx::init() {
    DANN_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    DANN_HIP(hipEventCreate(&ev0));
    DANN_HIP(hipEventCreate(&ev1));
    DANN_HIP(hipHostMalloc((void**)&h_flag, 64, hipHostMallocMapped));
    *h_flag = 0;
    return DANN_OK;
}

void SearchCtx::destroy() {
    if (stream) (void)hipStreamSynchronize(stream);
    if (d_fail) (void)hipFree(d_fail);
    if (d_sched) (void)hipFree(d_sched);
    if (h_flag) (void)hipHostFree(h_flag);
    if (d_spill) (void)hipFree(d_spill);
    for (void* p : stage)
        if (p) (void)hipFree(p);
    if (h_stage) (void)hipHostFree(h_stage);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
    *this = SearchCtx();
}

CtxLease::CtxLease(dann_index* i, bool try_only) : idx(i) {
    std::unique_lock<std::mutex> lk(idx->ctx_mu);
    for (;;) {
        if (!idx->ctx_free.empty()) {
            ctx = idx->ctx_free.back();
            idx->ctx_free.pop_back();
            return;
        }
        if (idx->ctx_created < kMaxSearchCtx) {
            ++idx->ctx_created;
            lk.unlock();
            SearchCtx* c = new (std::nothrow) SearchCtx();
            status = c ? c->init() : DANN_ENOMEM;
            if (status != DANN_OK) {
                if (c) {
                    c->destroy();
                    delete c;
                }
                lk.lock();
                --idx->ctx_created;
                idx->ctx_cv.notify_one();
                return;
            }
            ctx = c;
            return;
        }
        if (try_only) {  // (a caller that can do without: no context is free and none may be created)
            status = DANN_EBUSY;
            return;
        }
        idx->ctx_cv.wait(lk);
    }
}

CtxLease::~CtxLease() {
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> lk(idx->ctx_mu);
        idx->ctx_free.push_back(ctx);
    }
    idx->ctx_cv.notify_one();
}

uint32_t auto_visited_entries(const dann_index* idx, uint32_t, uint32_t) {
    if (idx->visited_bits >= 64) return std::min<uint32_t>((idx->visited_bits + 63u) / 64u * 64u, 32768u);
    if (idx->visited_bits) return 1u << idx->visited_bits;
    return 0;  // sized per launch by search_with_retry (search_kernels.hip)
}

// ---- search --------------------------------------------------------------------------------
static int32_t pq_ready(const dann_index* idx) {
    if (idx->cfg.dtype == DT_PQ && (!idx->d_pq_pivots || !idx->d_pq_offsets)) {
        set_error("DANN_PQ index has no pivot table: call dann_set_pq_table first");
        return DANN_EINVAL;
    }
    return DANN_OK;
}

int32_t search_device(dann_index* idx, SearchCtx& ctx, const void* d_queries, const uint32_t* d_qslots, uint32_t nq,
                      uint32_t l_value, uint32_t beam, uint32_t k, uint32_t* d_ids, float* d_dists,
                      dann_search_stats* d_stats, uint32_t* d_rec_ids, float* d_rec_d, uint32_t rec_stride,
                      uint32_t* d_rec_n) {
    if (int32_t prc = pq_ready(idx)) return prc;
    if (idx->cfg.dtype == DT_PQ && d_qslots) {
        set_error("insert-time search (query = stored row) is not defined for DANN_PQ");
        return DANN_EUNSUPPORTED;
    }
    SearchArgs a;
    a.ix = d_qslots ? idx->view() : idx->qview();  // (a stored row as the query: always the symmetric form)
    a.queries = d_queries;
    a.qslots = d_qslots;
    a.nq = nq;
    a.l_value = l_value;
    a.beam_width = beam;
    a.k = k;
    a.ht_entries = auto_visited_entries(idx, l_value, beam);
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.stats = d_stats;
    a.rec_ids = d_rec_ids;
    a.rec_dists = d_rec_d;
    a.rec_stride = rec_stride;
    a.rec_n = d_rec_n;
    return search_with_retry(idx, ctx, a);
}

// shared access for the Knn search entry points: the index is read-only here, every call runs on its own context
#define CHECK_IDX_SHARED(idx)                               \
    if (!(idx)) {                                           \
        set_error("null index");                            \
        return DANN_EINVAL;                                 \
    }                                                       \
    std::shared_lock<std::shared_mutex> _rd((idx)->rw);     \
    DeviceGuard _guard((idx)->device);                      \
    CtxLease _lease(idx);                                   \
    if (_lease.status != DANN_OK) return _lease.status;     \
    SearchCtx& ctx = *_lease.ctx

int32_t grow_stage(SearchCtx& ctx, int i, size_t need) {
    if (ctx.stage_bytes[i] >= need) return DANN_OK;
    if (ctx.stage[i]) (void)hipFree(ctx.stage[i]);
    ctx.stage[i] = nullptr;
    ctx.stage_bytes[i] = 0;
    const size_t sz = need + need / 4;
    DANN_HIP(hipMalloc(&ctx.stage[i], sz));
    ctx.stage_bytes[i] = sz;
    return DANN_OK;
}

// The scratch arena of the range / filtered searches (stage[4]) stays resident between calls only up to this size: a
// call with per-query filter bitmaps on a large index can need gigabytes, and an index that nearly fills HBM would
// miss them in its next build or search (the pool keeps up to 16 contexts).  Beyond it the block is released when the
// call returns (a hipFree synchronises the device: the price of a call that large, not of every call).
constexpr size_t kArenaKeepBytes = (size_t)256 << 20;
struct ArenaTrim {
    SearchCtx& ctx;
    ~ArenaTrim() {
        if (ctx.stage_bytes[4] > kArenaKeepBytes) {
            (void)hipStreamSynchronize(ctx.stream);
            (void)hipFree(ctx.stage[4]);
            ctx.stage[4] = nullptr;
            ctx.stage_bytes[4] = 0;
        }
    }
};
}  // namespace dann

using namespace dann;

dann::IndexView dann_index::view() const {
    IndexView v;
    v.rows = d_rows;
    v.adj = d_adj;
    v.row_stride = cfg.row_stride;
    v.adj_stride = cfg.max_degree + 1;
    v.dim = cfg.dim;
    v.capacity = cfg.capacity;
    v.nslots = nslots;
    v.max_degree = cfg.max_degree;
    v.nstart = cfg.num_start_points;
    v.dtype = cfg.dtype;
    v.metric = cfg.metric;
    v.layer_bytes = layer_bytes;
    v.qbytes = layer_bytes;
    {   // (1/(2^bits - 1))^2 * scale^2 in f32, in the reference's order (scalar/mod.rs:129-135, vectors.rs:231-241,
        // quantizer.rs:316-320)
        const float ibs = 1.0f / (float)((1u << (dt_is_sq(cfg.dtype) ? sq_bits(cfg.dtype) : 8)) - 1u);
        const float bit_scale = ibs * ibs;
        const float scale_sq = cfg.sq_scale * cfg.sq_scale;
        v.sq_k = bit_scale * scale_sq;
        v.sq_shift_norm_sq = cfg.sq_shift_norm_sq;
    }
    v.pq_pivots = d_pq_pivots;
    v.pq_offsets = d_pq_offsets;
    v.pq_chunks = cfg.pq_chunks;
    v.pq_pack = pq_pack_valid ? d_pq_pack : nullptr;
    v.pq_pack_stride = pq_pack_stride;
    v.pq_pack_codes = pq_pack_codes;
    v.tag_off = cfg.inline_tags ? layer_bytes : 0u;
    if (dt_is_sph(cfg.dtype)) v.sq_k = 0.0f;  // (no scale; non-zero marks a QueryMeta, see qview and SqParams)
    if (dt_is_mm(cfg.dtype)) v.sq_k = v.sq_shift_norm_sq = 0.0f;  // (every row carries its own scale and offset)
    return v;
}

// The view of the entry points that take queries.  Spherical rows: the query's byte image follows the layout
// (iface::QueryLayout) -- FOUR_BIT_TRANSPOSED has an inner-product routine of its own and therefore a row type of its
// own inside the kernels (DT_SPH1T); SCALAR_QUANTIZED shares the symmetric routine and differs in the epilogue, which
// SqParams::k != 0 selects at run time.
dann::IndexView dann_index::qview(int32_t layout) const {
    IndexView v = view();
    if (!dt_is_sph(cfg.dtype)) return v;
    v.qbytes = sph_query_bytes(cfg.dtype, cfg.dim, layout);
    if (layout == QL_TRANSPOSED) v.dtype = DT_SPH1T;
    if (layout == QL_SCALAR) v.sq_k = 1.0f;
    return v;
}
dann::IndexView dann_index::qview() const { return qview(query_layout.load(std::memory_order_relaxed)); }
uint32_t dann_index::query_bytes() const {
    if (cfg.dtype == DT_PQ) return cfg.dim * 4u;  // PQ rows: f32 queries
    if (dt_is_sph(cfg.dtype)) return sph_query_bytes(cfg.dtype, cfg.dim, query_layout.load(std::memory_order_relaxed));
    return layer_bytes;
}

extern "C" {

int32_t dann_last_error(char* buf, uint64_t len) try {
    size_t n = strlen(g_err);
    if (buf && len) {
        size_t c = n < len - 1 ? n : len - 1;
        memcpy(buf, g_err, c);
        buf[c] = 0;
    }
    return (int32_t)n;
} DANN_CATCH_ALL

int32_t dann_layer_bytes(int32_t dtype, uint32_t dim) try {
    if (!valid_dtype(dtype)) {
        set_error("bad dtype %d", dtype);
        return DANN_EINVAL;
    }
    return (int32_t)layer_bytes_of(dtype, dim);
} DANN_CATCH_ALL

int32_t dann_inmem2_row_stride(int32_t dtype, uint32_t dim) try {
    int32_t b = dann_layer_bytes(dtype, dim);
    if (b < 0) return b;
    return (b + 1 + 31) / 32 * 32;
} DANN_CATCH_ALL

int32_t dann_index_create(const dann_config* cfg, const void* start_rows, uint64_t start_len, dann_index** out) try {
    if (!cfg || !out) {
        set_error("null argument");
        return DANN_EINVAL;
    }
    *out = nullptr;
    if (!valid_dtype(cfg->dtype) || !valid_metric(cfg->metric) || cfg->dim == 0 || cfg->max_degree == 0) {
        set_error("invalid config (dtype %d metric %d dim %u max_degree %u)", cfg->dtype, cfg->metric, cfg->dim,
                  cfg->max_degree);
        return DANN_EINVAL;
    }
    if (cfg->dtype == DT_PQ && (cfg->pq_chunks == 0 || cfg->pq_chunks > 128 || cfg->pq_chunks > cfg->dim)) {
        set_error("DANN_PQ needs 1 <= pq_chunks <= min(dim, 128)");
        return DANN_EINVAL;
    }
    if (dt_is_sph(cfg->dtype)) {
        // DataMeta::bit_sum is a u16 (spherical/vectors.rs:219-247); SupportedMetric has no CosineNormalized
        if ((uint64_t)cfg->dim * ((1u << sq_bits(cfg->dtype)) - 1u) > 65535u) {
            set_error("dim %u: the bit sum of a %d-bit spherical row does not fit its u16", cfg->dim, sq_bits(cfg->dtype));
            return DANN_EINVAL;
        }
        if (cfg->metric == M_COSN) {
            set_error("spherical rows: L2, inner product and cosine (CosineNormalized is not a SupportedMetric)");
            return DANN_EINVAL;
        }
    }
    if (dt_is_mm(cfg->dtype)) {  // the inner product of two rows' codes is a u32 (minmax/vectors.rs:206-229)
        const uint64_t top = (1u << sq_bits(cfg->dtype)) - 1u;
        if ((uint64_t)cfg->dim * top * top > 0xFFFFFFFFull) {
            set_error("dim %u: the inner product of two %d-bit MinMax rows does not fit a u32", cfg->dim, sq_bits(cfg->dtype));
            return DANN_EINVAL;
        }
    }
    const uint32_t lb = cfg->dtype == DT_PQ ? cfg->pq_chunks : layer_bytes_of(cfg->dtype, cfg->dim);
    {
        int op;
        bool norm;
        if (!resolve_metric(cfg->dtype, cfg->metric, &op, &norm)) {
            set_error("metric %d is not defined for dtype %d", cfg->metric, cfg->dtype);
            return DANN_EUNSUPPORTED;
        }
        if (dt_is_sq(cfg->dtype) && !(cfg->sq_scale > 0.0f)) {
            set_error("DANN_SQ8 / DANN_SQ4 / DANN_SQ1 need sq_scale > 0");
            return DANN_EINVAL;
        }
    }
    if ((uint64_t)cfg->capacity + cfg->num_start_points >= 0x7FFFFFFFull) {
        set_error("capacity + start points must be below 2^31 - 1");
        return DANN_EINVAL;
    }
    if (start_len != (uint64_t)lb * cfg->num_start_points || (cfg->num_start_points && !start_rows)) {
        set_error("start rows: expected %llu bytes, got %llu", (unsigned long long)lb * cfg->num_start_points,
                  (unsigned long long)start_len);
        return DANN_ELENGTH;
    }
    dann_index* idx = new (std::nothrow) dann_index();
    if (!idx) return DANN_ENOMEM;
    idx->cfg = *cfg;
    idx->layer_bytes = lb;
    if (!mm_headers_ok(idx, start_rows, cfg->num_start_points, lb)) {
        delete idx;
        return DANN_EINVAL;
    }
    for (auto& d : idx->dbg) d.store(__builtin_nan(""), std::memory_order_relaxed);
    if (idx->cfg.row_stride == 0) idx->cfg.row_stride = (lb + 15u) & ~15u;
    if (idx->cfg.row_stride < lb || (idx->cfg.row_stride & 15u)) {
        set_error("row_stride %u must be >= %u and a multiple of 16", idx->cfg.row_stride, lb);
        delete idx;
        return DANN_EINVAL;
    }
    if (idx->cfg.inline_tags && idx->cfg.row_stride <= lb) {
        set_error("inline_tags needs row_stride > %u payload bytes (the tag byte follows the payload, store.rs:133-158)", lb);
        delete idx;
        return DANN_EINVAL;
    }
    idx->nslots = cfg->capacity + cfg->num_start_points;
    int dev = cfg->device;
    if (dev < 0) {
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) {
            delete idx;
            return hip_fail(e, "hipGetDevice");
        }
    }
    idx->device = dev;
    idx->cfg.device = dev;
    DeviceGuard guard(dev);
    auto fail = [&](hipError_t e, const char* what) {
        int32_t rc = hip_fail(e, what);
        dann_index_destroy(idx);
        return rc;
    };
    if (!guard.ok) return fail(hipErrorInvalidDevice, "hipSetDevice");
    hipError_t e;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            idx->num_cus = (uint32_t)cus;
    }
    if (int32_t irc = idx->main.init()) {
        dann_index_destroy(idx);
        return irc;
    }
    const size_t rows_bytes = (size_t)idx->nslots * idx->cfg.row_stride + 256;
    const size_t adj_bytes = (size_t)idx->nslots * (cfg->max_degree + 1) * 4;
    if ((e = hipMalloc((void**)&idx->d_rows, rows_bytes)) != hipSuccess) return fail(e, "hipMalloc(rows)");
    if ((e = hipMalloc((void**)&idx->d_adj, adj_bytes)) != hipSuccess) return fail(e, "hipMalloc(adjacency)");
    if ((e = hipMemsetAsync(idx->d_rows, 0, rows_bytes, idx->main.stream)) != hipSuccess) return fail(e, "hipMemset");
    if ((e = hipMemsetAsync(idx->d_adj, 0, adj_bytes, idx->main.stream)) != hipSuccess) return fail(e, "hipMemset");
    if (cfg->num_start_points) {
        e = hipMemcpy2DAsync(idx->d_rows + (size_t)cfg->capacity * idx->cfg.row_stride, idx->cfg.row_stride, start_rows,
                             lb, lb, cfg->num_start_points, hipMemcpyHostToDevice, idx->main.stream);
        if (e != hipSuccess) return fail(e, "hipMemcpy2D(start rows)");
    }
    if (idx->cfg.inline_tags) {  // dynamic slots AVAILABLE (0, the memset above), start points FROZEN (store.rs:766-772)
        idx->h_tags.assign(idx->nslots, 0);
        if (cfg->num_start_points) {
            std::fill(idx->h_tags.begin() + cfg->capacity, idx->h_tags.end(), (uint8_t)255);
            e = hipMemset2DAsync(idx->d_rows + (size_t)cfg->capacity * idx->cfg.row_stride + lb, idx->cfg.row_stride, 255, 1,
                                 cfg->num_start_points, idx->main.stream);
            if (e != hipSuccess) return fail(e, "hipMemset2D(start tags)");
        }
    }
    if ((e = hipStreamSynchronize(idx->main.stream)) != hipSuccess) return fail(e, "hipStreamSynchronize");
    *out = idx;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_index_destroy(dann_index* idx) try {
    if (!idx) return DANN_OK;
    DeviceGuard guard(idx->device);
    if (idx->server) (void)dann_server_stop(idx);
    idx->main.destroy();
    for (SearchCtx* c : idx->ctx_free) {
        c->destroy();
        delete c;
    }
    idx->ctx_free.clear();
    if (idx->d_rows) (void)hipFree(idx->d_rows);
    if (idx->d_adj) (void)hipFree(idx->d_adj);
    if (idx->d_pq_pivots) (void)hipFree(idx->d_pq_pivots);
    if (idx->d_pq_offsets) (void)hipFree(idx->d_pq_offsets);
    if (idx->d_pq_pack) (void)hipFree(idx->d_pq_pack);
    if (idx->d_sched_piv) (void)hipFree(idx->d_sched_piv);
    if (idx->d_deleted) (void)hipFree(idx->d_deleted);
    if (idx->d_attr) (void)hipFree(idx->d_attr);
    if (idx->build_scratch && idx->build_scratch_free) idx->build_scratch_free(idx->build_scratch);
    delete idx;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_index_max_degree(const dann_index* idx) { return idx ? (int32_t)idx->cfg.max_degree : DANN_EINVAL; }

int32_t dann_index_get_config(const dann_index* idx, dann_config* out) try {
    if (!idx || !out) return DANN_EINVAL;
    *out = idx->cfg;
    return DANN_OK;
} DANN_CATCH_ALL

#define CHECK_IDX(idx)                                  \
    if (!(idx)) {                                       \
        set_error("null index");                        \
        return DANN_EINVAL;                             \
    }                                                   \
    ::dann::ExclusiveGuard _lock(idx); \
    DeviceGuard _guard((idx)->device)

int32_t dann_set_elements(dann_index* idx, uint32_t first_slot, uint32_t n, const void* rows, uint64_t len) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (n == 0) return DANN_OK;
    if (!rows) return DANN_EINVAL;
    if (len != (uint64_t)n * idx->layer_bytes) {
        set_error("raw byte slice of length %llu does not match expected length %llu", (unsigned long long)len,
                  (unsigned long long)n * idx->layer_bytes);
        return DANN_ELENGTH;
    }
    if ((uint64_t)first_slot + n > idx->cfg.capacity) {
        set_error("slot range [%u, %llu) exceeds capacity %u", first_slot, (unsigned long long)first_slot + n,
                  idx->cfg.capacity);
        return DANN_EBOUNDS;
    }
    if (!mm_headers_ok(idx, rows, n, idx->layer_bytes)) return DANN_EINVAL;
    DANN_HIP(hipMemcpy2DAsync(idx->d_rows + (size_t)first_slot * idx->cfg.row_stride, idx->cfg.row_stride, rows,
                              idx->layer_bytes, idx->layer_bytes, n, hipMemcpyHostToDevice, idx->main.stream));
    if (idx->cfg.inline_tags) {  // Slot::publish (store.rs:776-782)
        DANN_HIP(hipMemset2DAsync(idx->d_rows + (size_t)first_slot * idx->cfg.row_stride + idx->layer_bytes,
                                  idx->cfg.row_stride, kTagReadable, 1, n, idx->main.stream));
        std::fill(idx->h_tags.begin() + first_slot, idx->h_tags.begin() + first_slot + n, kTagReadable);
    }
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_set_elements_device(dann_index* idx, uint32_t first_slot, uint32_t n, const void* d_rows, uint64_t src_stride) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (n == 0) return DANN_OK;
    if (!d_rows) return DANN_EINVAL;
    if (src_stride < idx->layer_bytes) {
        set_error("source stride %llu is shorter than the layer's %u bytes", (unsigned long long)src_stride, idx->layer_bytes);
        return DANN_ELENGTH;
    }
    if ((uint64_t)first_slot + n > idx->cfg.capacity) {
        set_error("slot range [%u, %llu) exceeds capacity %u", first_slot, (unsigned long long)first_slot + n,
                  idx->cfg.capacity);
        return DANN_EBOUNDS;
    }
    DANN_HIP(hipMemcpy2DAsync(idx->d_rows + (size_t)first_slot * idx->cfg.row_stride, idx->cfg.row_stride, d_rows, src_stride,
                              idx->layer_bytes, n, hipMemcpyDeviceToDevice, idx->main.stream));
    if (idx->cfg.inline_tags) {  // Slot::publish (store.rs:776-782)
        DANN_HIP(hipMemset2DAsync(idx->d_rows + (size_t)first_slot * idx->cfg.row_stride + idx->layer_bytes,
                                  idx->cfg.row_stride, kTagReadable, 1, n, idx->main.stream));
        std::fill(idx->h_tags.begin() + first_slot, idx->h_tags.begin() + first_slot + n, kTagReadable);
    }
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_index_device_pointers(const dann_index* idx, const void** d_rows, const uint32_t** d_adjacency) try {
    if (!idx) return DANN_EINVAL;
    if (d_rows) *d_rows = idx->d_rows;
    if (d_adjacency) *d_adjacency = idx->d_adj;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_set_tags(dann_index* idx, uint32_t first_slot, uint32_t n, const uint8_t* tags) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (n == 0) return DANN_OK;
    if (!tags) return DANN_EINVAL;
    if (!idx->cfg.inline_tags) {
        set_error("dann_set_tags: the index was created without inline_tags");
        return DANN_EUNSUPPORTED;
    }
    if ((uint64_t)first_slot + n > idx->nslots) return DANN_EBOUNDS;
    // start points are FROZEN for the lifetime of the store (store.rs:766-772); a search that cannot read one fails
    // ("could not retrieve start point", provider.rs:408-431) -- refuse the state instead of producing it
    for (uint32_t i = 0; i < n; ++i)
        if (first_slot + i >= idx->cfg.capacity && tags[i] < kTagReadable) {
            set_error("dann_set_tags: start point slot %u must stay readable (tag >= 254), got %u", first_slot + i, tags[i]);
            return DANN_EINVAL;
        }
    DANN_HIP(hipMemcpy2DAsync(idx->d_rows + (size_t)first_slot * idx->cfg.row_stride + idx->layer_bytes,
                              idx->cfg.row_stride, tags, 1, 1, n, hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    memcpy(idx->h_tags.data() + first_slot, tags, n);
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_get_tags(const dann_index* idx, uint32_t first_slot, uint32_t n, uint8_t* tags) try {
    if (!idx || (n && !tags)) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    if ((uint64_t)first_slot + n > idx->nslots) return DANN_EBOUNDS;
    if (!idx->cfg.inline_tags) memset(tags, kTagReadable, n);  // a store without tags: every slot readable
    else memcpy(tags, idx->h_tags.data() + first_slot, n);
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_set_element(dann_index* idx, uint32_t slot, const void* bytes, uint64_t len) try {
    return dann_set_elements(idx, slot, 1, bytes, len);
} DANN_CATCH_ALL

int32_t dann_get_element(const dann_index* idx, uint32_t slot, void* bytes, uint64_t len) try {
    CHECK_IDX(idx);
    if (!bytes) return DANN_EINVAL;
    if (len != idx->layer_bytes) {
        set_error("expected slice of length %u - instead got %llu", idx->layer_bytes, (unsigned long long)len);
        return DANN_ELENGTH;
    }
    if (slot >= idx->nslots) return DANN_EBOUNDS;
    DANN_HIP(hipMemcpyAsync(bytes, idx->d_rows + (size_t)slot * idx->cfg.row_stride, len, hipMemcpyDeviceToHost,
                            idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_upload_store(dann_index* idx, const void* base, uint64_t stride, uint32_t nrows) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (!base) return DANN_EINVAL;
    if (nrows > idx->nslots) return DANN_EBOUNDS;
    if (stride < idx->layer_bytes) return DANN_ELENGTH;
    // with inline_tags the tag byte that follows each payload travels with it (needs stride > payload)
    const bool tags = idx->cfg.inline_tags != 0;
    if (tags && stride <= idx->layer_bytes) {
        set_error("dann_upload_store: inline_tags needs a source stride > %u payload bytes", idx->layer_bytes);
        return DANN_ELENGTH;
    }
    if (tags) {  // as dann_set_tags: a start point must stay readable
        const uint8_t* b = reinterpret_cast<const uint8_t*>(base) + idx->layer_bytes;
        for (uint32_t i = idx->cfg.capacity; i < nrows; ++i)
            if (b[(size_t)i * stride] < kTagReadable) {
                set_error("dann_upload_store: start point slot %u must be readable (tag >= 254), got %u", i, b[(size_t)i * stride]);
                return DANN_EINVAL;
            }
    }
    DANN_HIP(hipMemcpy2DAsync(idx->d_rows, idx->cfg.row_stride, base, stride, idx->layer_bytes + (tags ? 1u : 0u), nrows,
                              hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    if (tags) {
        const uint8_t* b = reinterpret_cast<const uint8_t*>(base) + idx->layer_bytes;
        for (uint32_t i = 0; i < nrows; ++i) idx->h_tags[i] = b[(size_t)i * stride];
    }
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_set_pq_table(dann_index* idx, const float* pivots, const uint32_t* chunk_offsets) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (!pivots || !chunk_offsets) return DANN_EINVAL;
    if (idx->cfg.dtype != DT_PQ) {
        set_error("dann_set_pq_table: the index is not DANN_PQ");
        return DANN_EINVAL;
    }
    const uint32_t nc = idx->cfg.pq_chunks, dim = idx->cfg.dim;
    if (chunk_offsets[0] != 0 || chunk_offsets[nc] != dim) {
        set_error("chunk offsets must start at 0 and end at dim");
        return DANN_EINVAL;
    }
    for (uint32_t c = 0; c < nc; ++c)
        if (chunk_offsets[c + 1] <= chunk_offsets[c]) {
            set_error("chunk offsets must be strictly increasing");
            return DANN_EINVAL;
        }
    if (!idx->d_pq_pivots) DANN_HIP(hipMalloc((void**)&idx->d_pq_pivots, (size_t)256 * dim * 4));
    if (!idx->d_pq_offsets) DANN_HIP(hipMalloc((void**)&idx->d_pq_offsets, (size_t)(nc + 1) * 4));
    DANN_HIP(hipMemcpyAsync(idx->d_pq_pivots, pivots, (size_t)256 * dim * 4, hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipMemcpyAsync(idx->d_pq_offsets, chunk_offsets, (size_t)(nc + 1) * 4, hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

// ---- query layout of spherical indexes (iface::QueryLayout) ---------------------------------------------------------
int32_t dann_set_query_layout(dann_index* idx, int32_t layout) try {
    CHECK_IDX(idx);
    if (layout == QL_EIGHT_BIT) {  // MinMaxQuery::EightBit (an MM8 image against narrower MinMax rows): not served
        set_error("query layout %d is not supported for dtype %d", layout, idx->cfg.dtype);
        return DANN_EUNSUPPORTED;
    }
    if (layout < QL_SAME || layout > QL_FULL) {
        set_error("dann_set_query_layout: unknown layout %d", layout);
        return DANN_EINVAL;
    }
    if (idx->server.load(std::memory_order_acquire)) {  // the resident kernel was sized and instantiated for a layout
        set_error("dann_set_query_layout: stop the search server first");
        return DANN_EBUSY;
    }
    const bool sph = dt_is_sph(idx->cfg.dtype);
    if (layout != QL_SAME && (!sph || sph_query_bytes(idx->cfg.dtype, idx->cfg.dim, layout) == 0u)) {
        // UnsupportedQueryLayout: FOUR_BIT_TRANSPOSED is the 1-bit rows', SCALAR_QUANTIZED the 2- and 4-bit rows',
        // FULL_PRECISION is not served
        set_error("query layout %d is not supported for dtype %d", layout, idx->cfg.dtype);
        return DANN_EUNSUPPORTED;
    }
    idx->query_layout.store(layout, std::memory_order_relaxed);
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_get_query_layout(const dann_index* idx) try {
    if (!idx) {
        set_error("null index");
        return DANN_EINVAL;
    }
    return idx->query_layout.load(std::memory_order_relaxed);
} DANN_CATCH_ALL

int32_t dann_query_bytes(const dann_index* idx) try {
    if (!idx) {
        set_error("null index");
        return DANN_EINVAL;
    }
    return (int32_t)idx->query_bytes();
} DANN_CATCH_ALL

// ---- packed search layout of PQ indexes ----------------------------------------------------------------------------
int32_t dann_pq_pack_neighbors(dann_index* idx) try {
    CHECK_IDX(idx);
    // (only pq_search_kernel reads the packed rows: an index it can never serve -- pq_lut_shape / plain_mode -- would pay
    // 1.3 KB per node for nothing)
    const uint32_t code_words = (idx->cfg.pq_chunks + 15u) / 16u;  // 16-byte words of a code row
    if (idx->cfg.dtype != DT_PQ || idx->cfg.pq_chunks > 64u || idx->cfg.inline_tags || idx->cfg.max_degree > 64u ||
        idx->cfg.num_start_points > 64u || idx->cfg.row_stride < 16u * code_words || idx->cfg.row_stride % 16u) {
        set_error("dann_pq_pack_neighbors: a DANN_PQ index of at most 64 chunks, degree <= 64, at most 64 start points, "
                  "without inline tags, rows at a 16-byte stride");
        return DANN_EUNSUPPORTED;
    }
    // the rebuild rewrites (and may free) what a concurrent dann_search_submit's relaunch reads through idx->view():
    // it is a mutation -- refused while tickets are outstanding, submits bounce while it runs, the resident kernel leaves
    DANN_MUTATION(idx);
    const uint32_t R = idx->cfg.max_degree;
    const uint32_t codes_off = ((R + 1u) * 4u + 15u) & ~15u;
    const uint32_t stride = (codes_off + 16u * code_words * R + 63u) & ~63u;
    const size_t bytes = (size_t)idx->nslots * stride;
    if (idx->pq_pack_bytes < bytes) {
        if (idx->d_pq_pack) (void)hipFree(idx->d_pq_pack);
        idx->d_pq_pack = nullptr;
        idx->pq_pack_bytes = 0;
        idx->pq_pack_valid = false;
        DANN_HIP(hipMalloc((void**)&idx->d_pq_pack, bytes));
        idx->pq_pack_bytes = bytes;
    }
    idx->pq_pack_stride = stride;
    idx->pq_pack_codes = codes_off;
    idx->pq_pack_valid = false;
    int32_t rc = launch_pq_pack(idx->view(), idx->d_pq_pack, stride, codes_off, idx->main.stream);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    idx->pq_pack_valid = true;
    return DANN_OK;
} DANN_CATCH_ALL

// ---- external ids ------------------------------------------------------------------------
int32_t dann_set_external_ids(dann_index* idx, uint32_t first_slot, uint32_t n, const uint64_t* ext_ids) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    if (n == 0) return DANN_OK;
    if (!ext_ids) return DANN_EINVAL;
    if ((uint64_t)first_slot + n > idx->cfg.capacity) return DANN_EBOUNDS;
    if (idx->ext_ids.empty()) idx->ext_ids.assign(idx->cfg.capacity, ~0ull);
    memcpy(idx->ext_ids.data() + first_slot, ext_ids, (size_t)n * 8);
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_to_external(const dann_index* idx, const uint32_t* slot_ids, uint64_t n, uint64_t* out_ext) try {
    if (!idx || (n && (!slot_ids || !out_ext))) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t s = slot_ids[i];
        if (s >= idx->cfg.capacity) out_ext[i] = ~0ull;  // start points / padding have no mapping
        else out_ext[i] = idx->ext_ids.empty() ? (uint64_t)s : idx->ext_ids[s];
    }
    return DANN_OK;
} DANN_CATCH_ALL

// ---- adjacency ---------------------------------------------------------------------------
int32_t dann_get_neighbors(const dann_index* idx, uint32_t slot, uint32_t* out, uint32_t cap, uint32_t* out_len) try {
    CHECK_IDX(idx);
    if (!out_len) return DANN_EINVAL;
    if (slot >= idx->nslots) {
        set_error("adjacency list %u is out of bounds (%u entries)", slot, idx->nslots);
        return DANN_EBOUNDS;
    }
    std::vector<uint32_t> row(idx->cfg.max_degree + 1);
    DANN_HIP(hipMemcpyAsync(row.data(), idx->d_adj + (size_t)slot * row.size(), row.size() * 4, hipMemcpyDeviceToHost,
                            idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    uint32_t len = std::min(row[0], idx->cfg.max_degree);
    *out_len = len;
    if (len > cap || (len && !out)) return DANN_ETOOLONG;
    if (len) memcpy(out, row.data() + 1, (size_t)len * 4);
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_set_neighbors(dann_index* idx, uint32_t slot, const uint32_t* ids, uint32_t n) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (slot >= idx->nslots) return DANN_EBOUNDS;
    if (n > idx->cfg.max_degree) {
        set_error("adjacency list of length %u exceeds max degree %u", n, idx->cfg.max_degree);
        return DANN_ETOOLONG;
    }
    if (n && !ids) return DANN_EINVAL;
    std::vector<uint32_t> row(n + 1);
    row[0] = n;
    if (n) memcpy(row.data() + 1, ids, (size_t)n * 4);
    DANN_HIP(hipMemcpyAsync(idx->d_adj + (size_t)slot * (idx->cfg.max_degree + 1), row.data(), row.size() * 4,
                            hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_append_neighbors(dann_index* idx, uint32_t slot, const uint32_t* ids, uint32_t n) try {
    CHECK_IDX(idx);  // recursive mutex: the get / set calls below re-enter it
    DANN_MUTATION(idx);
    if (n && !ids) return DANN_EINVAL;
    if (slot >= idx->nslots) return DANN_EBOUNDS;
    std::vector<uint32_t> cur(idx->cfg.max_degree);
    uint32_t len = 0;
    int32_t rc = dann_get_neighbors(idx, slot, cur.data(), idx->cfg.max_degree, &len);
    if (rc != DANN_OK) return rc;
    uint32_t slack = idx->cfg.max_degree - len;  // clamp, provider.rs:804-816
    uint32_t take = std::min(n, slack);
    for (uint32_t i = 0; i < take; ++i) cur[len + i] = ids[i];
    return dann_set_neighbors(idx, slot, cur.data(), len + take);
} DANN_CATCH_ALL

int32_t dann_set_neighbors_bulk(dann_index* idx, const uint32_t* slots, uint32_t n, const uint32_t* lists) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (n == 0) return DANN_OK;
    if (!slots || !lists) return DANN_EINVAL;
    const uint32_t w = idx->cfg.max_degree + 1;
    for (uint32_t i = 0; i < n; ++i) {
        if (slots[i] >= idx->nslots) return DANN_EBOUNDS;
        if (lists[(size_t)i * w] > idx->cfg.max_degree) return DANN_ETOOLONG;
    }
    for (uint32_t i = 0; i < n; ++i) {
        DANN_HIP(hipMemcpyAsync(idx->d_adj + (size_t)slots[i] * w, lists + (size_t)i * w, (size_t)w * 4,
                                hipMemcpyHostToDevice, idx->main.stream));
    }
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_upload_graph(dann_index* idx, const uint32_t* adj, uint64_t nrows) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (!adj) return DANN_EINVAL;
    if (nrows > idx->nslots) return DANN_EBOUNDS;
    DANN_HIP(hipMemcpyAsync(idx->d_adj, adj, (size_t)nrows * (idx->cfg.max_degree + 1) * 4, hipMemcpyHostToDevice,
                            idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_download_graph(const dann_index* idx, uint32_t* adj, uint64_t nrows) try {
    CHECK_IDX(idx);
    if (!adj) return DANN_EINVAL;
    if (nrows > idx->nslots) return DANN_EBOUNDS;
    DANN_HIP(hipMemcpyAsync(adj, idx->d_adj, (size_t)nrows * (idx->cfg.max_degree + 1) * 4, hipMemcpyDeviceToHost,
                            idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

// ---- distances ---------------------------------------------------------------------------
int32_t dann_distance(const dann_index* idx, const void* x, uint64_t xlen, const void* y, uint64_t ylen, float* out) try {
    CHECK_IDX(idx);
    if (!x || !y || !out) return DANN_EINVAL;
    if (xlen != idx->layer_bytes || ylen != idx->layer_bytes) {
        set_error("expected slices of length %u - instead got %llu and %llu", idx->layer_bytes,
                  (unsigned long long)xlen, (unsigned long long)ylen);
        return DANN_ELENGTH;
    }
    const size_t stride = (idx->layer_bytes + 15u) & ~15u;
    DevBuf buf;
    DANN_HIP(buf.alloc(2 * stride + 16));
    uint8_t* d = buf.as<uint8_t>();
    DANN_HIP(hipMemcpyAsync(d, x, xlen, hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipMemcpyAsync(d + stride, y, ylen, hipMemcpyHostToDevice, idx->main.stream));
    float* d_out = reinterpret_cast<float*>(d + 2 * stride);
    int32_t rc = launch_distance_raw(idx->view(), d, d + stride, stride, 1, d_out, idx->main.stream);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(out, d_out, 4, hipMemcpyDeviceToHost, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_distance_pairs(const dann_index* idx, const uint32_t* a, const uint32_t* b, uint32_t n, float* out) try {
    CHECK_IDX(idx);
    if (n == 0) return DANN_OK;
    if (!a || !b || !out) return DANN_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (a[i] >= idx->nslots || b[i] >= idx->nslots) return DANN_EBOUNDS;
    DevBuf buf;
    DANN_HIP(buf.alloc((size_t)n * 12));
    uint32_t* da = buf.as<uint32_t>();
    uint32_t* db = da + n;
    float* dout = reinterpret_cast<float*>(db + n);
    DANN_HIP(hipMemcpyAsync(da, a, (size_t)n * 4, hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipMemcpyAsync(db, b, (size_t)n * 4, hipMemcpyHostToDevice, idx->main.stream));
    int32_t rc = launch_distance_pairs(idx->view(), da, db, n, dout, idx->main.stream);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_query_create(const dann_index* idx, const void* query, uint64_t len, dann_query** out) try {
    CHECK_IDX(idx);
    if (!query || !out) return DANN_EINVAL;
    *out = nullptr;
    const int32_t layout = idx->query_layout.load(std::memory_order_relaxed);
    const uint32_t want = dt_is_sph(idx->cfg.dtype) ? sph_query_bytes(idx->cfg.dtype, idx->cfg.dim, layout) : idx->layer_bytes;
    if (len != want) {  // Full::check_dim (full.rs:86-99)
        set_error("query of %llu bytes does not match the layer's %u bytes", (unsigned long long)len, want);
        return DANN_ELENGTH;
    }
    if (!mm_headers_ok(idx, query, 1, len)) return DANN_EINVAL;
    dann_query* q = new (std::nothrow) dann_query();
    if (!q) return DANN_ENOMEM;
    q->idx = idx;
    q->layout = layout;
    hipError_t e = hipMalloc(&q->d_query, (len + 15) & ~15ull);
    if (e != hipSuccess) {
        delete q;
        return hip_fail(e, "hipMalloc(query)");
    }
    e = hipMemcpyAsync(q->d_query, query, len, hipMemcpyHostToDevice, idx->main.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(idx->main.stream);
    if (e != hipSuccess) {
        (void)hipFree(q->d_query);
        delete q;
        return hip_fail(e, "hipMemcpy(query)");
    }
    *out = q;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_query_destroy(dann_query* q) try {
    if (!q) return DANN_OK;
    DeviceGuard guard(q->idx->device);
    if (q->d_query) (void)hipFree(q->d_query);
    delete q;
    return DANN_OK;
} DANN_CATCH_ALL

// shared by dann_query_distance / dann_expand_beam: search-path kernel over a temporary row
// set or stored rows
static int32_t expand_on_device(const dann_index* idx, const IndexView& view, const void* d_query, const uint32_t* ids,
                                uint32_t n, float* out) {
    DevBuf buf;
    DANN_HIP(buf.alloc((size_t)n * 8 + 16));
    uint64_t* d_off = buf.as<uint64_t>();
    uint32_t* d_ids = reinterpret_cast<uint32_t*>(d_off + 2);
    float* d_out = reinterpret_cast<float*>(d_ids + n);
    uint64_t off[2] = {0, n};
    DANN_HIP(hipMemcpyAsync(d_off, off, 16, hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipMemcpyAsync(d_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, idx->main.stream));
    int32_t rc = launch_expand_beam(view, d_query, 1, d_ids, d_off, n, d_out, idx->main.stream);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
}

int32_t dann_query_distance(const dann_query* q, const void* row, uint64_t len, float* out) try {
    if (!q || !row || !out) return DANN_EINVAL;
    const dann_index* idx = q->idx;
    ::dann::ExclusiveGuard lock(idx);
    DeviceGuard guard(idx->device);
    if (len != idx->layer_bytes) {
        set_error("expected slice of length %u - instead got %llu", idx->layer_bytes, (unsigned long long)len);
        return DANN_ELENGTH;
    }
    DevBuf rowbuf;
    DANN_HIP(rowbuf.alloc((len + 15) & ~15ull));
    DANN_HIP(hipMemcpyAsync(rowbuf.p, row, len, hipMemcpyHostToDevice, idx->main.stream));
    IndexView v = idx->qview(q->layout);
    v.rows = rowbuf.as<uint8_t>();
    v.nslots = 1;
    uint32_t zero = 0;
    return expand_on_device(idx, v, q->d_query, &zero, 1, out);
} DANN_CATCH_ALL

int32_t dann_expand_beam(const dann_query* q, const uint32_t* ids, uint32_t n, uint32_t* out_ids, float* out_dists,
                         uint32_t* out_n) try {
    if (!q || !out_n) return DANN_EINVAL;
    const dann_index* idx = q->idx;
    ::dann::ExclusiveGuard lock(idx);
    DeviceGuard guard(idx->device);
    *out_n = 0;
    if (n == 0) return DANN_OK;
    if (!ids || !out_ids || !out_dists) return DANN_EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (ids[i] >= idx->nslots) return DANN_EBOUNDS;
    // read_in_bounds(i) -> None for a slot whose tag is not readable: skipped, not counted (provider.rs:681-686)
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (!idx->cfg.inline_tags || idx->h_tags[ids[i]] >= kTagReadable) out_ids[m++] = ids[i];
    *out_n = m;
    if (m == 0) return DANN_OK;
    return expand_on_device(idx, idx->qview(q->layout), q->d_query, out_ids, m, out_dists);
} DANN_CATCH_ALL

int32_t dann_expand_beam_batch(const dann_index* cidx, const void* queries, uint32_t nq, const uint32_t* ids,
                               const uint64_t* offsets, float* out_dists) try {
    dann_index* idx = const_cast<dann_index*>(cidx);
    CHECK_IDX(idx);
    if (nq == 0) return DANN_OK;
    if (!queries || !ids || !offsets || !out_dists) return DANN_EINVAL;
    const uint64_t total = offsets[nq];
    uint64_t max_len = 0;
    for (uint32_t i = 0; i < nq; ++i) {
        if (offsets[i + 1] < offsets[i]) return DANN_EINVAL;
        max_len = std::max(max_len, offsets[i + 1] - offsets[i]);
    }
    for (uint64_t i = 0; i < total; ++i)
        if (ids[i] >= idx->nslots) return DANN_EBOUNDS;
    if (total == 0) return DANN_OK;
    DevBuf bq, bo, bi, bd;
    DANN_HIP(bq.alloc((size_t)nq * idx->query_bytes() + 16));
    DANN_HIP(bo.alloc((size_t)(nq + 1) * 8));
    DANN_HIP(bi.alloc(total * 4));
    DANN_HIP(bd.alloc(total * 4));
    DANN_HIP(hipMemcpyAsync(bq.p, queries, (size_t)nq * idx->query_bytes(), hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipMemcpyAsync(bo.p, offsets, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipMemcpyAsync(bi.p, ids, total * 4, hipMemcpyHostToDevice, idx->main.stream));
    int32_t rc = timed(idx, 1, [&] {
        return launch_expand_beam(idx->qview(), bq.p, nq, bi.as<uint32_t>(), bo.as<uint64_t>(), max_len, bd.as<float>(),
                                  idx->main.stream);
    });
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(out_dists, bd.p, total * 4, hipMemcpyDeviceToHost, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    if (idx->cfg.inline_tags)  // the positional batch form cannot drop entries: unreadable slots report NaN
        for (uint64_t i = 0; i < total; ++i)
            if (idx->h_tags[ids[i]] < kTagReadable) out_dists[i] = __builtin_nanf("");
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_search_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, uint32_t l_value,
                                 uint32_t beam_width, uint32_t k, uint32_t* d_out_ids, float* d_out_dists,
                                 dann_search_stats* d_out_stats) try {
    CHECK_IDX_SHARED(idx);
    if (nq == 0) return DANN_OK;
    if (!d_queries || !d_out_ids || !d_out_dists) return DANN_EINVAL;
    if (!d_out_stats) {  // the overflow retry needs per-query status: context-owned stats when the caller passes none
        if (int32_t rc = grow_stage(ctx, 2, (size_t)nq * sizeof(dann_search_stats))) return rc;
        d_out_stats = reinterpret_cast<dann_search_stats*>(ctx.stage[2]);
    }
    return search_device(idx, ctx, d_queries, nullptr, nq, l_value, beam_width, k, d_out_ids, d_out_dists, d_out_stats,
                         nullptr, nullptr, 0, nullptr);
} DANN_CATCH_ALL

// RangeSearchError (range_search.rs:30-45, 93-131), for both range entry points
static int32_t check_range_params(uint32_t starting_l, uint32_t beam_width, float radius, int32_t has_inner_radius,
                                  float inner_radius, float initial_slack, float range_slack, uint32_t max_returned) {
    if (starting_l == 0 || beam_width == 0) {
        set_error("l_value and beam width cannot be zero");
        return DANN_EINVAL;
    }
    if (max_returned && max_returned < starting_l) {
        set_error("max_returned must be greater than or equal to starting_l");
        return DANN_EINVAL;
    }
    if (!(initial_slack >= 0.0f && initial_slack <= 1.0f)) {
        set_error("initial_search_slack must be between 0 and 1.0");
        return DANN_EINVAL;
    }
    if (!(range_slack >= 1.0f)) {
        set_error("range_search_slack must be greater than or equal to 1.0");
        return DANN_EINVAL;
    }
    if (has_inner_radius && inner_radius > radius) {
        set_error("inner_radius must be less than or equal to radius");
        return DANN_EINVAL;
    }
    return DANN_OK;
}

// The n per-query stats of a launch on `st`: copied back (the stream is synchronised, so the copies queued before have
// landed too), mirrored into the caller's out_stats if there is one; *first_bad = the first query whose status is
// non-zero, or n.  What an exhausted query means is the caller's to say.
static int32_t fetch_stats(hipStream_t st, const void* d_stats, uint32_t n, dann_search_stats* out_stats, uint32_t* first_bad) {
    std::vector<dann_search_stats> stats(n);
    DANN_HIP(hipMemcpyAsync(stats.data(), d_stats, (size_t)n * sizeof(dann_search_stats), hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    if (out_stats) memcpy(out_stats, stats.data(), (size_t)n * sizeof(dann_search_stats));
    uint32_t i = 0;
    while (i < n && !stats[i].status) ++i;
    *first_bad = i;
    return DANN_OK;
}

int32_t dann_range_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t starting_l,
                                uint32_t beam_width, float radius, int32_t has_inner_radius, float inner_radius,
                                float initial_slack, float range_slack, uint32_t max_returned, uint32_t out_cap,
                                uint32_t* out_ids, float* out_dists, dann_search_stats* out_stats,
                                uint32_t* out_second_round) try {
    CHECK_IDX_SHARED(idx);  // read-only: concurrent callers run side by side, each on its own context
    ArenaTrim _trim{ctx};
    if (int32_t rc = check_range_params(starting_l, beam_width, radius, has_inner_radius, inner_radius, initial_slack,
                                        range_slack, max_returned))
        return rc;
    if (nq == 0) return DANN_OK;
    if (!queries || !out_ids || !out_dists || out_cap == 0) return DANN_EINVAL;
    uint64_t cap = max_returned ? max_returned : (uint64_t)4 * out_cap + 1024;
    cap = std::min<uint64_t>(cap, idx->nslots);
    cap = std::max<uint64_t>(cap, 1);
    if (int32_t prc = pq_ready(idx)) return prc;
    const size_t qb = idx->query_bytes();
    // scratch of this call: one block of the context's grow-only arena (no hipMalloc / hipFree per call: a hipFree
    // synchronises the whole device and would serialise concurrent callers)
    Carve cv;
    const size_t o_q = cv.take((size_t)nq * qb + 16), o_i = cv.take((size_t)nq * out_cap * 4),
                 o_d = cv.take((size_t)nq * out_cap * 4), o_s = cv.take((size_t)nq * sizeof(dann_search_stats)),
                 o_ri = cv.take((size_t)nq * cap * 4), o_rd = cv.take((size_t)nq * cap * 4), o_sec = cv.take((size_t)nq * 4);
    if (int32_t grc = grow_stage(ctx, 4, cv.off)) return grc;
    const ArenaPtr bq{ctx.stage[4], o_q}, bi{ctx.stage[4], o_i}, bd{ctx.stage[4], o_d}, bs{ctx.stage[4], o_s},
        bri{ctx.stage[4], o_ri}, brd{ctx.stage[4], o_rd}, bsec{ctx.stage[4], o_sec};
    DANN_HIP(hipMemcpyAsync(bq.p, queries, (size_t)nq * qb, hipMemcpyHostToDevice, ctx.stream));
    SearchArgs a;
    a.ix = idx->qview();
    a.queries = bq.p;
    a.nq = nq;
    a.l_value = starting_l;
    a.beam_width = beam_width;
    a.k = out_cap;
    a.ht_entries = auto_visited_entries(idx, std::max<uint32_t>(starting_l, 64), beam_width);
    a.out_ids = bi.as<uint32_t>();
    a.out_dists = bd.as<float>();
    a.stats = bs.as<dann_search_stats>();
    a.range_ids = bri.as<uint32_t>();
    a.range_d = brd.as<float>();
    a.range_second = bsec.as<uint32_t>();
    a.range_cap = (uint32_t)cap;
    a.range_max = max_returned ? max_returned : 0xFFFFFFFFu;
    a.range_thresh = (uint32_t)((float)starting_l * initial_slack);
    a.has_inner = has_inner_radius ? 1u : 0u;
    a.radius = radius;
    a.inner_radius = inner_radius;
    a.range_slack = range_slack;
    int32_t rc = search_with_retry(idx, ctx, a);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(out_ids, bi.p, (size_t)nq * out_cap * 4, hipMemcpyDeviceToHost, ctx.stream));
    DANN_HIP(hipMemcpyAsync(out_dists, bd.p, (size_t)nq * out_cap * 4, hipMemcpyDeviceToHost, ctx.stream));
    if (out_second_round)
        DANN_HIP(hipMemcpyAsync(out_second_round, bsec.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx.stream));
    uint32_t bad = nq;
    if (int32_t frc = fetch_stats(ctx.stream, bs.p, nq, out_stats, &bad)) return frc;
    if (bad < nq) {
        set_error("query %u: more results than out_cap (%u), or range scratch list (%llu entries) or visited scratch "
                  "exhausted; raise out_cap", bad, out_cap, (unsigned long long)cap);
        return DANN_EOVERFLOW;
    }
    return DANN_OK;
} DANN_CATCH_ALL

// ---- filtered searches ---------------------------------------------------------------------------
// compute_adaptive_l (inline_filter_search.rs:283-301): f64, truncating casts, host libm
static uint32_t adaptive_l(uint32_t base_l, uint32_t visited, uint32_t matched, double max_multiplier) {
    if (matched == 0 || visited == 0) return (uint32_t)std::min<double>((double)base_l * max_multiplier, 4.0e9);
    const double specificity = (double)matched / (double)visited;
    double multiplier;
    if (specificity >= 0.5) multiplier = 1.0;
    else if (specificity >= 0.1) multiplier = 2.0;
    else multiplier = std::pow(2.0, -std::log10(specificity));
    multiplier = std::min(std::max(multiplier, 1.0), max_multiplier);
    return (uint32_t)std::min<double>((double)base_l * multiplier, 4.0e9);
}

namespace {
struct FilteredCall {
    const void* queries;
    uint32_t nq, l_value, beam, k;
    const dann_filter* filter;
    uint32_t* out_ids;
    float* out_dists;
    dann_search_stats* out_stats;
    // FilteredRange only
    bool range = false;
    float radius = 0.f, inner_radius = 0.f, initial_slack = 1.f, range_slack = 1.f;
    int32_t has_inner = 0;
    uint32_t max_returned = 0;
    uint32_t* out_second = nullptr;
};
}  // namespace

static int32_t filtered_search(dann_index* idx, SearchCtx& ctx, const FilteredCall& c) {
    const dann_filter* f = c.filter;
    if (!f || !f->bits || (f->mode != DANN_FILTER_INLINE && f->mode != DANN_FILTER_MULTIHOP)) {
        set_error("filter: mode must be DANN_FILTER_INLINE or DANN_FILTER_MULTIHOP and bits non-null");
        return DANN_EINVAL;
    }
    if (c.l_value == 0 || c.beam == 0) {
        set_error("l_value and beam_width must be non-zero");
        return DANN_EINVAL;
    }
    if (f->adaptive_samples && (f->mode != DANN_FILTER_INLINE || c.range)) {
        set_error("AdaptiveL applies to InlineFilterSearch only");
        return DANN_EINVAL;
    }
    if (f->adaptive_samples && !(f->adaptive_scale >= 1.0)) {
        set_error("adaptive L scale factor must be >= 1.0");  // AdaptiveLSearchError::ScaleFactorLessThanOne
        return DANN_EINVAL;
    }
    if (c.range && f->mode != DANN_FILTER_INLINE) {
        set_error("FilteredRange runs on the inline filter search (filtered_range_search.rs:148-156)");
        return DANN_EINVAL;
    }
    if (int32_t prc = pq_ready(idx)) return prc;
    const uint32_t nslots = idx->nslots;
    const uint64_t words = (nslots + 31) / 32;
    if (f->stride_words && f->stride_words < words) {
        set_error("filter stride %llu words is shorter than one bitmap (%llu words)",
                  (unsigned long long)f->stride_words, (unsigned long long)words);
        return DANN_EINVAL;
    }
    hipStream_t st = ctx.stream;
    const size_t qb = idx->query_bytes();
    const bool inl = f->mode == DANN_FILTER_INLINE;
    SearchArgs a;
    a.ix = idx->qview();
    a.l_value = c.l_value;
    a.beam_width = c.beam;
    a.k = c.k;
    a.ht_entries = auto_visited_entries(idx, c.l_value, c.beam);
    a.filter_mode = f->mode;
    a.filter_stride = f->stride_words;
    // AdaptiveL: table of new L for every (visited, matched) the decision can see
    std::vector<uint32_t> tab;  // (outlives the asynchronous upload below: the arena is sized after it)
    const uint32_t cmax = std::max<uint32_t>((c.beam * idx->cfg.max_degree + 63u) & ~63u, (idx->cfg.num_start_points + 63u) & ~63u);
    if (f->adaptive_samples) {
        const uint64_t stride = (uint64_t)f->adaptive_samples + cmax;
        if (stride * cmax > (64ull << 20)) {
            set_error("AdaptiveL sample_count %u is too large for the decision table", f->adaptive_samples);
            return DANN_EUNSUPPORTED;
        }
        tab.resize(stride * cmax);
        uint32_t lmax = 0;
        for (uint32_t dv = 0; dv < cmax; ++dv)
            for (uint64_t m = 0; m < stride; ++m) {
                const uint32_t v = f->adaptive_samples + dv;
                const uint32_t nl = m <= v ? adaptive_l(c.l_value, v, (uint32_t)m, f->adaptive_scale) : c.l_value;
                tab[dv * stride + m] = nl;
                lmax = std::max(lmax, nl);
            }
        a.ad_samples = f->adaptive_samples;
        a.ad_stride = (uint32_t)stride;
        a.qcap_max = std::max(lmax, c.l_value + idx->cfg.num_start_points);
    }
    // per-launch scratch: the matched list and its sort keys; queries go through in chunks that keep it small
    uint32_t m_cap = 0, key_cap = 0;
    if (inl) {
        m_cap = f->matched_cap ? f->matched_cap : std::min<uint32_t>(nslots, 8192);
        m_cap = std::min<uint32_t>(std::max<uint32_t>(m_cap, 64), nslots);
        key_cap = 1;
        while (key_cap < m_cap + (c.range ? c.l_value : 0)) key_cap <<= 1;
    }
    uint64_t rcap = 0;
    if (c.range) {
        // matched_within_radius: every matched id of the first round within the radius (<= m_cap) plus the
        // second round's appends, which stop at max_returned
        rcap = c.max_returned ? c.max_returned : (uint64_t)4 * c.k + 1024;
        rcap = std::max<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(rcap, m_cap), nslots), 1);
    }
    const bool tie_rust = idx->prune_tie_order == DANN_TIE_RUST;  // equal distances in the reference's own order
    const uint64_t per_query = (uint64_t)m_cap * 8 + (uint64_t)key_cap * 8 + rcap * 8 + 64 + (tie_rust ? kTieWorkBytes : 0);
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(c.nq, (1ull << 30) / per_query));
    // scratch of this call: one block of the context's grow-only arena (see dann_range_search_batch)
    const size_t fwords = f->stride_words ? (size_t)f->stride_words * c.nq : (size_t)words;
    Carve cv;
    const size_t o_q = cv.take((size_t)chunk * qb + 16), o_i = cv.take((size_t)chunk * c.k * 4),
                 o_d = cv.take((size_t)chunk * c.k * 4), o_s = cv.take((size_t)chunk * sizeof(dann_search_stats)),
                 o_f = cv.take(fwords * 4), o_tab = cv.take(tab.size() * 4),
                 o_mi = cv.take(inl ? (size_t)chunk * m_cap * 4 : 0), o_md = cv.take(inl ? (size_t)chunk * m_cap * 4 : 0),
                 o_k = cv.take(inl ? (size_t)chunk * key_cap * 8 : 0), o_tw = cv.take(tie_rust ? (size_t)chunk * kTieWorkBytes : 0),
                 o_ri = cv.take(c.range ? (size_t)chunk * rcap * 4 : 0), o_rd = cv.take(c.range ? (size_t)chunk * rcap * 4 : 0),
                 o_sec = cv.take(c.range ? (size_t)chunk * 4 : 0);
    if (int32_t grc = grow_stage(ctx, 4, cv.off)) return grc;
    void* const ar = ctx.stage[4];
    const ArenaPtr bq{ar, o_q}, bi{ar, o_i}, bd{ar, o_d}, bs{ar, o_s}, bf{ar, o_f}, btab{ar, o_tab}, bmi{ar, o_mi}, bmd{ar, o_md},
        bk{ar, o_k}, btw{ar, o_tw}, bri{ar, o_ri}, brd{ar, o_rd}, bsec{ar, o_sec};
    DANN_HIP(hipMemcpyAsync(bf.p, f->bits, fwords * 4, hipMemcpyHostToDevice, st));
    if (!tab.empty()) {
        DANN_HIP(hipMemcpyAsync(btab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
        a.ad_table = btab.as<uint32_t>();
    }
    if (tie_rust) a.tie_work = btw.as<uint8_t>();
    if (inl) {
        a.m_ids = bmi.as<uint32_t>();
        a.m_d = bmd.as<float>();
        a.m_keys = bk.as<unsigned long long>();
        a.m_cap = m_cap;
        a.key_cap = key_cap;
    }
    if (c.range) {
        a.range_ids = bri.as<uint32_t>();
        a.range_d = brd.as<float>();
        a.range_second = bsec.as<uint32_t>();
        a.range_cap = (uint32_t)rcap;
        a.range_max = c.max_returned ? c.max_returned : 0xFFFFFFFFu;
        a.range_thresh = (uint32_t)((float)c.l_value * c.initial_slack);
        a.has_inner = c.has_inner ? 1u : 0u;
        a.radius = c.radius;
        a.inner_radius = c.inner_radius;
        a.range_slack = c.range_slack;
    }
    a.out_ids = bi.as<uint32_t>();
    a.out_dists = bd.as<float>();
    a.stats = bs.as<dann_search_stats>();
    a.queries = bq.p;
    for (uint32_t off = 0; off < c.nq; off += chunk) {
        const uint32_t n = std::min(chunk, c.nq - off);
        DANN_HIP(hipMemcpyAsync(bq.p, (const uint8_t*)c.queries + (size_t)off * qb, (size_t)n * qb, hipMemcpyHostToDevice, st));
        a.nq = n;
        a.filter = bf.as<uint32_t>() + (size_t)off * f->stride_words;
        int32_t rc = search_with_retry(idx, ctx, a);
        if (rc != DANN_OK) return rc;
        DANN_HIP(hipMemcpyAsync(c.out_ids + (size_t)off * c.k, bi.p, (size_t)n * c.k * 4, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipMemcpyAsync(c.out_dists + (size_t)off * c.k, bd.p, (size_t)n * c.k * 4, hipMemcpyDeviceToHost, st));
        if (c.out_second)
            DANN_HIP(hipMemcpyAsync(c.out_second + off, bsec.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        uint32_t bad = n;
        if (int32_t frc = fetch_stats(st, bs.p, n, c.out_stats ? c.out_stats + off : nullptr, &bad)) return frc;
        if (bad < n) {
            set_error("query %u: per-query scratch exhausted (matched list %u entries, result list %llu, visited "
                      "table); raise dann_filter.matched_cap / out_cap", off + bad, m_cap, (unsigned long long)rcap);
            return DANN_EOVERFLOW;
        }
    }
    return DANN_OK;
}

int32_t dann_filtered_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t l_value,
                                   uint32_t beam_width, uint32_t k, const dann_filter* filter, uint32_t* out_ids,
                                   float* out_dists, dann_search_stats* out_stats) try {
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    if (nq == 0) return DANN_OK;
    if (!queries || !out_ids || !out_dists || k == 0) return DANN_EINVAL;
    FilteredCall c{queries, nq, l_value, beam_width, k, filter, out_ids, out_dists, out_stats};
    return filtered_search(idx, ctx, c);
} DANN_CATCH_ALL

int32_t dann_filtered_range_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t starting_l,
                                         uint32_t beam_width, float radius, int32_t has_inner_radius,
                                         float inner_radius, float initial_slack, float range_slack,
                                         uint32_t max_returned, uint32_t out_cap, const dann_filter* filter,
                                         uint32_t* out_ids, float* out_dists, dann_search_stats* out_stats,
                                         uint32_t* out_second_round) try {
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    if (int32_t rc = check_range_params(starting_l, beam_width, radius, has_inner_radius, inner_radius, initial_slack,
                                        range_slack, max_returned))
        return rc;
    if (nq == 0) return DANN_OK;
    if (!queries || !out_ids || !out_dists || out_cap == 0) return DANN_EINVAL;
    FilteredCall c{queries, nq, starting_l, beam_width, out_cap, filter, out_ids, out_dists, out_stats};
    c.range = true;
    c.radius = radius;
    c.inner_radius = inner_radius;
    c.initial_slack = initial_slack;
    c.range_slack = range_slack;
    c.has_inner = has_inner_radius;
    c.max_returned = max_returned;
    c.out_second = out_second_round;
    return filtered_search(idx, ctx, c);
} DANN_CATCH_ALL

// ---- diversity-aware search (search_diverse.hip) ---------------------------------------------------------------------
int32_t dann_set_attributes(dann_index* idx, uint32_t first_slot, uint32_t n, const uint32_t* values) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if ((uint64_t)first_slot + n > idx->nslots) {
        set_error("dann_set_attributes: slots [%u, %llu) out of bounds (%u slots)", first_slot,
                  (unsigned long long)first_slot + n, idx->nslots);
        return DANN_EBOUNDS;
    }
    if (n == 0) return DANN_OK;
    if (!values) return DANN_EINVAL;
    hipStream_t st = idx->main.stream;
    if (!idx->d_attr) {
        DANN_HIP(hipMalloc((void**)&idx->d_attr, (size_t)idx->nslots * 4));
        DANN_HIP(hipMemsetAsync(idx->d_attr, 0xFF, (size_t)idx->nslots * 4, st));  // DANN_NO_ATTRIBUTE
    }
    DANN_HIP(hipMemcpyAsync(idx->d_attr + first_slot, values, (size_t)n * 4, hipMemcpyHostToDevice, st));
    DANN_HIP(hipStreamSynchronize(st));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_get_attributes(const dann_index* idx, uint32_t first_slot, uint32_t n, uint32_t* out) try {
    if (!idx || (n && !out)) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    if ((uint64_t)first_slot + n > idx->nslots) return DANN_EBOUNDS;
    if (n == 0) return DANN_OK;
    if (!idx->d_attr) {
        for (uint32_t i = 0; i < n; ++i) out[i] = DANN_NO_ATTRIBUTE;
        return DANN_OK;
    }
    DeviceGuard guard(idx->device);
    DANN_HIP(hipMemcpyAsync(out, idx->d_attr + first_slot, (size_t)n * 4, hipMemcpyDeviceToHost, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_diverse_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t l_value,
                                  uint32_t beam_width, uint32_t k, const dann_diverse* params, uint32_t* out_ids,
                                  float* out_dists, dann_search_stats* out_stats) try {
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    if (!params) return DANN_EINVAL;
    // DiverseSearchError (diverse_search.rs:27-93) and DiverseError (:48-131)
    if (params->total_k == 0) {
        set_error("total k_value cannot be zero");
        return DANN_EINVAL;
    }
    if (params->diverse_k == 0) {
        set_error("diverse k_value cannot be zero");
        return DANN_EINVAL;
    }
    if (params->diverse_k > params->total_k) {
        set_error("diverse k_value (%u) cannot exceed total k_value (%u)", params->diverse_k, params->total_k);
        return DANN_EINVAL;
    }
    if (l_value == 0 || beam_width == 0) {
        set_error("l_value and beam_width must be non-zero (KnnSearchError, knn_search.rs:27-33)");
        return DANN_EINVAL;
    }
    if (l_value < params->total_k) {
        set_error("l_value (%u) must be greater than or equal to total_k_value (%u)", l_value, params->total_k);
        return DANN_EINVAL;
    }
    if (idx->cfg.dtype == DT_PQ) {
        set_error("dann_diverse_search_batch: not defined on DANN_PQ rows");
        return DANN_EUNSUPPORTED;
    }
    if (beam_width > 16) {
        set_error("beam_width %u exceeds the supported maximum of 16", beam_width);
        return DANN_EUNSUPPORTED;
    }
    if (l_value + idx->cfg.num_start_points > 1024) {
        set_error("search list size L + start points = %u exceeds the supported maximum of 1024",
                  l_value + idx->cfg.num_start_points);
        return DANN_EUNSUPPORTED;
    }
    if (nq == 0) return DANN_OK;
    if (!queries || !out_ids || !out_dists || k == 0) return DANN_EINVAL;
    hipStream_t st = ctx.stream;
    const size_t qb = idx->query_bytes();
    const uint32_t chunk = std::min<uint32_t>(nq, 65536u);
    Carve cv;
    const size_t o_q = cv.take((size_t)chunk * qb + 16), o_i = cv.take((size_t)chunk * k * 4),
                 o_d = cv.take((size_t)chunk * k * 4), o_s = cv.take((size_t)chunk * sizeof(dann_search_stats));
    if (int32_t grc = grow_stage(ctx, 4, cv.off)) return grc;
    void* const ar = ctx.stage[4];
    const ArenaPtr bq{ar, o_q}, bi{ar, o_i}, bd{ar, o_d}, bs{ar, o_s};
    std::vector<dann_search_stats> stats(chunk);
    for (uint32_t off = 0; off < nq; off += chunk) {
        const uint32_t n = std::min(chunk, nq - off);
        DANN_HIP(hipMemcpyAsync(bq.p, (const uint8_t*)queries + (size_t)off * qb, (size_t)n * qb, hipMemcpyHostToDevice, st));
        int32_t rc = diverse_search_device(idx, st, bq.p, n, l_value, beam_width, k, params->diverse_k, params->total_k,
                                           bi.as<uint32_t>(), bd.as<float>(), bs.as<dann_search_stats>());
        if (rc != DANN_OK) return rc;
        DANN_HIP(hipMemcpyAsync(out_ids + (size_t)off * k, bi.p, (size_t)n * k * 4, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipMemcpyAsync(out_dists + (size_t)off * k, bd.p, (size_t)n * k * 4, hipMemcpyDeviceToHost, st));
        if (out_stats)
            DANN_HIP(hipMemcpyAsync(out_stats + off, bs.p, (size_t)n * sizeof(dann_search_stats), hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
    }
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_rerank_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, const uint32_t* d_cand_ids,
                                 uint32_t cand_stride, uint32_t k, uint32_t* d_out_ids, float* d_out_dists) try {
    CHECK_IDX(idx);
    if (nq == 0) return DANN_OK;
    if (!d_queries || !d_cand_ids || !d_out_ids || !d_out_dists || k == 0) return DANN_EINVAL;
    int32_t rc = timed(idx, 1, [&] {
        return launch_rerank(idx->qview(), d_queries, nq, d_cand_ids, cand_stride, k, d_out_ids, d_out_dists,
                             idx->main.stream);
    });
    return rc;
} DANN_CATCH_ALL

int32_t dann_rerank_batch(dann_index* idx, const void* queries, uint32_t nq, const uint32_t* cand_ids,
                          uint32_t cand_stride, uint32_t k, uint32_t* out_ids, float* out_dists) try {
    CHECK_IDX(idx);
    if (nq == 0) return DANN_OK;
    if (!queries || !cand_ids || !out_ids || !out_dists || k == 0) return DANN_EINVAL;
    DevBuf bq, bc, bi, bd;
    DANN_HIP(bq.alloc((size_t)nq * idx->query_bytes() + 16));
    DANN_HIP(bc.alloc((size_t)nq * cand_stride * 4));
    DANN_HIP(bi.alloc((size_t)nq * k * 4));
    DANN_HIP(bd.alloc((size_t)nq * k * 4));
    DANN_HIP(hipMemcpyAsync(bq.p, queries, (size_t)nq * idx->query_bytes(), hipMemcpyHostToDevice, idx->main.stream));
    DANN_HIP(hipMemcpyAsync(bc.p, cand_ids, (size_t)nq * cand_stride * 4, hipMemcpyHostToDevice, idx->main.stream));
    int32_t rc = launch_rerank(idx->qview(), bq.p, nq, bc.as<uint32_t>(), cand_stride, k, bi.as<uint32_t>(),
                               bd.as<float>(), idx->main.stream);
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(out_ids, bi.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, idx->main.stream));
    DANN_HIP(hipMemcpyAsync(out_dists, bd.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, idx->main.stream));
    DANN_HIP(hipStreamSynchronize(idx->main.stream));
    return DANN_OK;
} DANN_CATCH_ALL

// ---- exhaustive scan (flat_kernels.hip): FlatIndex::knn_search ---------------------------------------------------------
}  // extern "C"
namespace {
// the checks both forms share; DANN_OK with *done set: nothing to launch and nothing to write
int32_t flat_check(const dann_index* idx, const void* queries, uint32_t nq, uint32_t first_slot, uint32_t n, uint32_t k,
                   uint32_t flags, const uint32_t* out_ids, const float* out_dists, bool* done) {
    *done = false;
    if (flags & ~(uint32_t)DANN_FLAT_SKIP_DELETED) {
        set_error("dann_flat_search_batch: unknown flag bits 0x%x", flags & ~(uint32_t)DANN_FLAT_SKIP_DELETED);
        return DANN_EINVAL;
    }
    if (k == 0) {
        set_error("dann_flat_search_batch: k cannot be zero");
        return DANN_EINVAL;
    }
    if (idx->cfg.dtype == DT_PQ) {
        set_error("dann_flat_search_batch: not defined on DANN_PQ rows (dann_pq_scan scores PQ codes)");
        return DANN_EUNSUPPORTED;
    }
    if (k > kFlatMaxK) {
        set_error("dann_flat_search_batch: k = %u exceeds the supported maximum of %u", k, kFlatMaxK);
        return DANN_EUNSUPPORTED;
    }
    if ((uint64_t)first_slot + n > idx->nslots) {
        set_error("dann_flat_search_batch: slots [%u, %llu) leave the index's %u slots", first_slot,
                  (unsigned long long)first_slot + n, idx->nslots);
        return DANN_EBOUNDS;
    }
    if (nq == 0) {
        *done = true;
        return DANN_OK;
    }
    if (!queries || !out_ids || !out_dists) {
        set_error("dann_flat_search_batch: null pointer");
        return DANN_EINVAL;
    }
    return DANN_OK;
}

// how the scan of `nq` queries is cut up (flat_plan.h)
int32_t flat_make_plan(const dann_index* idx, uint32_t nq, uint32_t n, uint32_t k, FlatPlan* plan) {
    const IndexView ix = idx->qview();
    *plan = flat_plan(n, nq, k, flat_query_slot_bytes(ix), idx->num_cus, idx->dbg_u32(DANN_DBG_FLAT_CHUNK_ROWS, 0u));
    if (plan->tile == 0) {
        set_error("dann_flat_search_batch: a query of %u bytes with k = %u does not fit the LDS", ix.qbytes, k);
        return DANN_EUNSUPPORTED;
    }
    if (idx->verbose())
        fprintf(stderr, "[dann] flat scan: n %u nq %u k %u -> tile %u, %u chunks of %u slots, %u queries per launch\n", n, nq, k,
                plan->tile, plan->nchunks, plan->chunk_rows, plan->batch);
    return DANN_OK;
}

// the scan of nq queries (at most as many as the plan was made for) on device buffers, plan.batch queries per launch;
// `scratch`: plan.scratch_bytes()
int32_t flat_run(dann_index* idx, hipStream_t st, const FlatPlan& plan, void* scratch, const void* d_queries, uint32_t nq,
                 uint32_t first_slot, uint32_t n, uint32_t flags, uint32_t* d_ids, float* d_dists, dann_search_stats* d_stats) {
    const IndexView ix = idx->qview();
    const uint32_t* deleted = (flags & DANN_FLAT_SKIP_DELETED) ? idx->d_deleted : nullptr;
    for (uint32_t off = 0; off < nq; off += plan.batch) {
        const uint32_t m = std::min(plan.batch, nq - off);
        int32_t rc = launch_flat_search(ix, plan, (const uint8_t*)d_queries + (size_t)off * ix.qbytes, m, first_slot, n, deleted,
                                        scratch, d_ids + (size_t)off * plan.k, d_dists + (size_t)off * plan.k,
                                        d_stats ? d_stats + off : nullptr, st);
        if (rc != DANN_OK) return rc;
    }
    return DANN_OK;
}
}  // namespace
extern "C" {

int32_t dann_flat_search_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                                      uint32_t k, uint32_t flags, uint32_t* d_out_ids, float* d_out_dists,
                                      dann_search_stats* d_out_stats) try {
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    bool done = false;
    if (int32_t rc = flat_check(idx, d_queries, nq, first_slot, n, k, flags, d_out_ids, d_out_dists, &done)) return rc;
    if (done) return DANN_OK;
    if (n == 0) {
        if (int32_t rc = launch_flat_empty(nq, k, d_out_ids, d_out_dists, d_out_stats, ctx.stream)) return rc;
    } else {
        FlatPlan plan;
        if (int32_t rc = flat_make_plan(idx, nq, n, k, &plan)) return rc;
        if (int32_t rc = grow_stage(ctx, 4, plan.scratch_bytes())) return rc;
        if (int32_t rc = flat_run(idx, ctx.stream, plan, ctx.stage[4], d_queries, nq, first_slot, n, flags, d_out_ids,
                                  d_out_dists, d_out_stats))
            return rc;
    }
    DANN_HIP(hipStreamSynchronize(ctx.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_flat_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                               uint32_t k, uint32_t flags, uint32_t* out_ids, float* out_dists,
                               dann_search_stats* out_stats) try {
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    bool done = false;
    if (int32_t rc = flat_check(idx, queries, nq, first_slot, n, k, flags, out_ids, out_dists, &done)) return rc;
    if (done) return DANN_OK;
    hipStream_t st = ctx.stream;
    const size_t qb = idx->query_bytes();
    // the call's queries go through the arena in pieces of at most 65536: queries | ids | distances | stats | chunk lists
    const uint32_t piece = std::min<uint32_t>(nq, 65536u);
    FlatPlan plan;
    if (n != 0)
        if (int32_t rc = flat_make_plan(idx, piece, n, k, &plan)) return rc;
    Carve cv;
    const size_t o_q = cv.take((size_t)piece * qb + 16), o_i = cv.take((size_t)piece * k * 4),
                 o_d = cv.take((size_t)piece * k * 4), o_s = cv.take((size_t)piece * sizeof(dann_search_stats)),
                 o_x = cv.take(n != 0 ? plan.scratch_bytes() : 0);
    if (int32_t grc = grow_stage(ctx, 4, cv.off)) return grc;
    void* const ar = ctx.stage[4];
    const ArenaPtr bq{ar, o_q}, bi{ar, o_i}, bd{ar, o_d}, bs{ar, o_s}, bx{ar, o_x};
    for (uint32_t off = 0; off < nq; off += piece) {
        const uint32_t m = std::min(piece, nq - off);
        DANN_HIP(hipMemcpyAsync(bq.p, (const uint8_t*)queries + (size_t)off * qb, (size_t)m * qb, hipMemcpyHostToDevice, st));
        int32_t rc = n == 0 ? launch_flat_empty(m, k, bi.as<uint32_t>(), bd.as<float>(), bs.as<dann_search_stats>(), st)
                            : flat_run(idx, st, plan, bx.p, bq.p, m, first_slot, n, flags, bi.as<uint32_t>(), bd.as<float>(),
                                       bs.as<dann_search_stats>());
        if (rc != DANN_OK) return rc;
        DANN_HIP(hipMemcpyAsync(out_ids + (size_t)off * k, bi.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipMemcpyAsync(out_dists + (size_t)off * k, bd.p, (size_t)m * k * 4, hipMemcpyDeviceToHost, st));
        if (out_stats)
            DANN_HIP(hipMemcpyAsync(out_stats + off, bs.p, (size_t)m * sizeof(dann_search_stats), hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
    }
    return DANN_OK;
} DANN_CATCH_ALL

// ---- multi-vector sets (maxsim_kernels.hip) ------------------------------------------------------------------------------
// Rows are kept at a stride of whole 16-byte units with the tail zeroed -- the layout the kernels stage from -- and the
// queries of a call are brought to the same stride on their way to the device.  MinMax sets (maxsim_mm_kernels.hip): the
// rows are canonical images on the way in; the device keeps their packed codes at such a stride and a header record per row.
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

// dann_search_record_batch / dann_search_record_queries: beam-1 searches that keep their visit records.  The queries are
// stored rows (`slots`) or rows staged from the host (`queries`); the caller passes exactly one of the two.
static int32_t search_record(dann_index* idx, const uint32_t* slots, const void* queries, uint32_t nq, uint32_t l_value,
                             uint32_t* rec_ids, float* rec_dists, uint32_t rec_stride, uint32_t* rec_n,
                             dann_search_stats* out_stats) {
    CHECK_IDX(idx);
    if (nq == 0) return DANN_OK;
    if (!(slots || queries) || !rec_ids || !rec_dists || !rec_n || rec_stride == 0) return DANN_EINVAL;
    for (uint32_t i = 0; slots && i < nq; ++i)
        if (slots[i] >= idx->nslots) return DANN_EBOUNDS;
    hipStream_t st = idx->main.stream;
    const size_t src_bytes = slots ? (size_t)nq * 4 : (size_t)nq * idx->query_bytes();
    DevBuf bsrc, bri, brd, brn, bs;
    DANN_HIP(bsrc.alloc(src_bytes + 16));  // (+ 16: the kernels read a query's tail with whole vector loads)
    DANN_HIP(bri.alloc((size_t)nq * rec_stride * 4));
    DANN_HIP(brd.alloc((size_t)nq * rec_stride * 4));
    DANN_HIP(brn.alloc((size_t)nq * 4));
    DANN_HIP(bs.alloc((size_t)nq * sizeof(dann_search_stats)));
    DANN_HIP(hipMemcpyAsync(bsrc.p, slots ? (const void*)slots : queries, src_bytes, hipMemcpyHostToDevice, st));
    int32_t rc = search_device(idx, idx->main, slots ? nullptr : bsrc.p, slots ? bsrc.as<uint32_t>() : nullptr, nq, l_value,
                               1, 0, nullptr, nullptr, bs.as<dann_search_stats>(), bri.as<uint32_t>(), brd.as<float>(),
                               rec_stride, brn.as<uint32_t>());
    if (rc != DANN_OK) return rc;
    DANN_HIP(hipMemcpyAsync(rec_ids, bri.p, (size_t)nq * rec_stride * 4, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipMemcpyAsync(rec_dists, brd.p, (size_t)nq * rec_stride * 4, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipMemcpyAsync(rec_n, brn.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    uint32_t bad = nq;
    if (int32_t frc = fetch_stats(st, bs.p, nq, out_stats, &bad)) return frc;
    if (bad < nq) {
        set_error("query %u: visited table or record buffer exhausted", bad);
        return DANN_EOVERFLOW;
    }
    return DANN_OK;
}

int32_t dann_search_record_batch(dann_index* idx, const uint32_t* slots, uint32_t nq, uint32_t l_value,
                                 uint32_t* rec_ids, float* rec_dists, uint32_t rec_stride, uint32_t* rec_n,
                                 dann_search_stats* out_stats) try {
    return search_record(idx, slots, nullptr, nq, l_value, rec_ids, rec_dists, rec_stride, rec_n, out_stats);
} DANN_CATCH_ALL

int32_t dann_search_record_queries(dann_index* idx, const void* queries, uint32_t nq, uint32_t l_value, uint32_t* rec_ids,
                                   float* rec_dists, uint32_t rec_stride, uint32_t* rec_n, dann_search_stats* out_stats) try {
    return search_record(idx, nullptr, queries, nq, l_value, rec_ids, rec_dists, rec_stride, rec_n, out_stats);
} DANN_CATCH_ALL

// ---- on-disk formats ---------------------------------------------------------------------------
struct File {
    FILE* f = nullptr;
    ~File() {
        if (f) fclose(f);
    }
};

int32_t dann_save_graph(const dann_index* idx, const char* path) try {
    CHECK_IDX(idx);
    if (!path) return DANN_EINVAL;
    const uint32_t w = idx->cfg.max_degree + 1;
    std::vector<uint32_t> adj((size_t)idx->nslots * w);
    int32_t rc = dann_download_graph(idx, adj.data(), idx->nslots);
    if (rc != DANN_OK) return rc;
    File out;
    out.f = fopen(path, "wb");
    if (!out.f) {
        set_error("cannot open %s for writing", path);
        return DANN_EINVAL;
    }
    uint64_t file_size = 24;
    for (uint32_t i = 0; i < idx->nslots; ++i) file_size += 4ull * (1 + std::min(adj[(size_t)i * w], idx->cfg.max_degree));
    const uint32_t max_degree = idx->cfg.max_degree, start = idx->cfg.capacity;
    const uint64_t nstart = idx->cfg.num_start_points;
    bool ok = fwrite(&file_size, 8, 1, out.f) == 1 && fwrite(&max_degree, 4, 1, out.f) == 1 &&
              fwrite(&start, 4, 1, out.f) == 1 && fwrite(&nstart, 8, 1, out.f) == 1;
    for (uint32_t i = 0; ok && i < idx->nslots; ++i) {
        const uint32_t len = std::min(adj[(size_t)i * w], idx->cfg.max_degree);
        ok = fwrite(&len, 4, 1, out.f) == 1 && (len == 0 || fwrite(&adj[(size_t)i * w + 1], 4, len, out.f) == len);
    }
    if (!ok) {
        set_error("short write to %s", path);
        return DANN_EINVAL;
    }
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_load_graph(dann_index* idx, const char* path, uint32_t* out_start, uint64_t* out_num_start,
                        uint64_t* out_num_points) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (!path) return DANN_EINVAL;
    File in;
    in.f = fopen(path, "rb");
    if (!in.f) {
        set_error("cannot open %s", path);
        return DANN_EINVAL;
    }
    uint64_t file_size = 0, nstart = 0;
    uint32_t max_degree = 0, start = 0;
    if (fread(&file_size, 8, 1, in.f) != 1 || fread(&max_degree, 4, 1, in.f) != 1 || fread(&start, 4, 1, in.f) != 1 ||
        fread(&nstart, 8, 1, in.f) != 1) {
        set_error("%s: truncated header", path);
        return DANN_ELENGTH;
    }
    const uint32_t w = idx->cfg.max_degree + 1;
    std::vector<uint32_t> adj((size_t)idx->nslots * w, 0u);
    std::vector<uint32_t> buf;
    uint64_t pos = 24, npts = 0;
    while (pos < file_size) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, in.f) != 1) {
            set_error("%s: truncated adjacency list %llu", path, (unsigned long long)npts);
            return DANN_ELENGTH;
        }
        // a list can be neither longer than what the header / this index allow nor than the rest of the file
        if (len > std::max(max_degree, idx->cfg.max_degree) || 4ull * len > file_size - pos) {
            set_error("%s: adjacency list %llu claims %u neighbours (header max degree %u)", path,
                      (unsigned long long)npts, len, max_degree);
            return DANN_ETOOLONG;
        }
        buf.resize(len);
        if (len && fread(buf.data(), 4, len, in.f) != len) {
            set_error("%s: truncated adjacency list %llu", path, (unsigned long long)npts);
            return DANN_ELENGTH;
        }
        if (npts < idx->nslots) {
            if (len > idx->cfg.max_degree) {
                set_error("%s: node %llu has %u neighbours, index max_degree is %u", path, (unsigned long long)npts, len,
                          idx->cfg.max_degree);
                return DANN_ETOOLONG;
            }
            adj[(size_t)npts * w] = len;
            if (len) memcpy(&adj[(size_t)npts * w + 1], buf.data(), (size_t)len * 4);
        }
        pos += 4ull * (1 + len);
        ++npts;
    }
    int32_t rc = dann_upload_graph(idx, adj.data(), idx->nslots);
    if (rc != DANN_OK) return rc;
    if (out_start) *out_start = start;
    if (out_num_start) *out_num_start = nstart;
    if (out_num_points) *out_num_points = npts;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_save_vectors_bin(const dann_index* idx, const char* path, uint32_t first_slot, uint32_t n) try {
    CHECK_IDX(idx);
    if (!path) return DANN_EINVAL;
    if ((uint64_t)first_slot + n > idx->nslots) return DANN_EBOUNDS;
    std::vector<uint8_t> rows((size_t)n * idx->layer_bytes);
    if (n) {
        DANN_HIP(hipMemcpy2DAsync(rows.data(), idx->layer_bytes, idx->d_rows + (size_t)first_slot * idx->cfg.row_stride,
                                  idx->cfg.row_stride, idx->layer_bytes, n, hipMemcpyDeviceToHost, idx->main.stream));
        DANN_HIP(hipStreamSynchronize(idx->main.stream));
    }
    File out;
    out.f = fopen(path, "wb");
    if (!out.f) {
        set_error("cannot open %s for writing", path);
        return DANN_EINVAL;
    }
    // `.bin`: dim counts elements of the stored type (scalar-quantised rows are written as their payload bytes)
    const uint32_t dim = dt_is_sq(idx->cfg.dtype) || dt_is_sph(idx->cfg.dtype) || dt_is_mm(idx->cfg.dtype) ? idx->layer_bytes : idx->cfg.dim;
    if (fwrite(&n, 4, 1, out.f) != 1 || fwrite(&dim, 4, 1, out.f) != 1 ||
        (rows.size() && fwrite(rows.data(), 1, rows.size(), out.f) != rows.size())) {
        set_error("short write to %s", path);
        return DANN_EINVAL;
    }
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_load_vectors_bin(dann_index* idx, const char* path, uint32_t first_slot, uint32_t* out_n) try {
    CHECK_IDX(idx);
    DANN_MUTATION(idx);
    if (!path) return DANN_EINVAL;
    File in;
    in.f = fopen(path, "rb");
    if (!in.f) {
        set_error("cannot open %s", path);
        return DANN_EINVAL;
    }
    uint32_t n = 0, dim = 0;
    if (fread(&n, 4, 1, in.f) != 1 || fread(&dim, 4, 1, in.f) != 1) return DANN_ELENGTH;
    const uint32_t want_dim = dt_is_sq(idx->cfg.dtype) || dt_is_sph(idx->cfg.dtype) || dt_is_mm(idx->cfg.dtype) ? idx->layer_bytes : idx->cfg.dim;
    if (dim != want_dim) {
        set_error("data of dimension %u does not match full precision layer's dimension %u", dim, want_dim);
        return DANN_ELENGTH;
    }
    if ((uint64_t)first_slot + n > idx->cfg.capacity) return DANN_EBOUNDS;
    std::vector<uint8_t> rows((size_t)n * idx->layer_bytes);
    if (rows.size() && fread(rows.data(), 1, rows.size(), in.f) != rows.size()) {
        set_error("%s: truncated payload", path);
        return DANN_ELENGTH;
    }
    int32_t rc = dann_set_elements(idx, first_slot, n, rows.data(), rows.size());
    if (rc != DANN_OK) return rc;
    if (out_n) *out_n = n;
    return DANN_OK;
} DANN_CATCH_ALL

// ---- diagnostics -----------------------------------------------------------------------------
int32_t dann_abi_version(void) { return DANN_ABI_VERSION; }
int32_t dann_kernel_time(const dann_index* idx, int32_t which, double* total_ms, uint64_t* launches) try {
    if (!idx || which < 0 || which > 5) return DANN_EINVAL;
    if (which == 5) {  // the build's MFMA Gram tiles: events on the build stream, resolved here
        ::dann::ExclusiveGuard lock(idx);
        return build_tile_clock(idx, total_ms, launches);
    }
    std::lock_guard<std::mutex> lk(idx->stat_mu);
    if (total_ms) *total_ms = idx->clocks[which].total_ms;
    if (launches) *launches = idx->clocks[which].launches;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_kernel_time_reset(dann_index* idx) try {
    if (!idx) return DANN_EINVAL;
    {
        ::dann::ExclusiveGuard lock(idx);
        build_tile_clock_reset(idx);
    }
    std::lock_guard<std::mutex> lk(idx->stat_mu);
    for (auto& c : idx->clocks) c = KernelClock();
    for (auto& c : idx->families) c = KernelClock();
    return DANN_OK;
} DANN_CATCH_ALL

// ---- development switches and the per-family launch counters (include/dann_debug.h) ----------------------------------
int32_t dann_debug_set(dann_index* idx, int32_t key, double value) try {
    if (!idx || key < 0 || key >= DANN_DBG_COUNT) return DANN_EINVAL;
    idx->dbg[key].store(value, std::memory_order_relaxed);
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_debug_get(const dann_index* idx, int32_t key, double* value) try {
    if (!idx || !value || key < 0 || key >= DANN_DBG_COUNT) return DANN_EINVAL;
    *value = idx->dbg[key].load(std::memory_order_relaxed);
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_debug_sched_pivots(dann_index* idx, float* out, uint32_t cap_floats, uint32_t* np, uint32_t* stride_halfs,
                                float* scale) try {
    if (!idx) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);  // no search is building them meanwhile
    DeviceGuard guard(idx->device);
    return sched_copy_pivots(idx, out, cap_floats, np, stride_halfs, scale);
} DANN_CATCH_ALL

int32_t dann_debug_small_call_stats(dann_index* idx, uint64_t* out2) try {
    if (!idx || !out2) return DANN_EINVAL;
    out2[0] = idx->comb.stats[0].load(std::memory_order_relaxed);
    out2[1] = idx->comb.stats[1].load(std::memory_order_relaxed);
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_debug_search_families(const dann_index* idx, uint64_t* out_launches, double* out_ms) try {
    if (!idx) return DANN_EINVAL;
    std::lock_guard<std::mutex> lk(idx->stat_mu);
    for (int f = 0; f < DANN_FAMILY_COUNT; ++f) {
        if (out_launches) out_launches[f] = idx->families[f].launches;
        if (out_ms) out_ms[f] = idx->families[f].total_ms;
    }
    return DANN_OK;
} DANN_CATCH_ALL

const char* dann_debug_family_name(int32_t family) {
    static const char* const names[DANN_FAMILY_COUNT] = {"one_wave", "team", "pair", "persistent", "server", "pq_lut", "diverse"};
    return family >= 0 && family < DANN_FAMILY_COUNT ? names[family] : nullptr;
}

int32_t dann_set_visited_bits(dann_index* idx, uint32_t bits) try {
    // 0 = automatic; 6..15 = log2(entries); >= 64 = explicit entry count (rounded up to a multiple of 64)
    if (!idx || (bits != 0 && bits < 64 && (bits < 6 || bits > 15)) || bits > 32768) return DANN_EINVAL;
    idx->visited_bits = bits;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_set_visited_format(dann_index* idx, uint32_t entry_bits) try {
    if (!idx || (entry_bits != 0 && entry_bits != 16 && entry_bits != 32)) return DANN_EINVAL;
    idx->visited_format = entry_bits;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_set_max_concurrency(dann_index* idx, uint32_t max_queries_in_flight) try {
    if (!idx) return DANN_EINVAL;
    idx->max_concurrency = max_queries_in_flight;
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_set_prune_tie_order(dann_index* idx, uint32_t order) try {
    if (!idx || (order != DANN_TIE_POSITION && order != DANN_TIE_RUST)) return DANN_EINVAL;
    dann::ExclusiveGuard g(idx);  // not while a build is running on another thread
    idx->prune_tie_order = order;
    return DANN_OK;
} DANN_CATCH_ALL

}  // extern "C"
