// api_index.hip -- the index's half of the C ABI of include/dann.h: error text, lifetime, HBM layout, the search
// contexts, the row / tag / id / attribute / adjacency setters, the knobs and the debug hooks.  No CPU fallback exists
// anywhere in this library: every distance, search and prune result comes from a HIP kernel, and a missing/failed device
// surfaces as DANN_EHIP.
#include <stdarg.h>
#include <stdio.h>

#include "api_common.h"
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
// SqParams::k != 0 selects at run time.  MinMax rows: QL_EIGHT_BIT (dann_set_query_dtype) says the queries are MM8 images.
dann::IndexView dann_index::qview(int32_t layout) const {
    IndexView v = view();
    if (layout == QL_EIGHT_BIT && dt_is_mm(cfg.dtype) && cfg.dtype != DT_MM8) {
        // MinMax rows searched with MM8 images (dann_set_query_dtype): an inner-product routine and a staged form of
        // their own, therefore internal row types; the epilogue reads the two headers as ever
        v.dtype = cfg.dtype - DT_MM1 + DT_MM1Q;
        v.qbytes = kMmHeader + cfg.dim;
        return v;
    }
    if (!dt_is_sph(cfg.dtype)) return v;
    v.qbytes = sph_query_bytes(cfg.dtype, cfg.dim, layout);
    if (layout == QL_TRANSPOSED) v.dtype = DT_SPH1T;
    if (layout == QL_SCALAR) v.sq_k = 1.0f;
    return v;
}
dann::IndexView dann_index::qview() const { return qview(query_layout.load(std::memory_order_relaxed)); }
uint32_t dann_index::query_bytes() const {
    if (cfg.dtype == DT_PQ) return cfg.dim * 4u;  // PQ rows: f32 queries
    return query_bytes(query_layout.load(std::memory_order_relaxed));
}
uint32_t dann_index::query_bytes(int32_t layout) const {
    if (cfg.dtype == DT_PQ) return cfg.dim * 4u;
    if (dt_is_sph(cfg.dtype)) return sph_query_bytes(cfg.dtype, cfg.dim, layout);
    if (layout == QL_EIGHT_BIT && dt_is_mm(cfg.dtype)) return kMmHeader + cfg.dim;  // an MM8 image
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
    // (beam_search_plain forms a row's address with 32 bits of the stride: a wider field needs a range check here)
    static_assert(sizeof(idx->cfg.row_stride) == 4, "row strides are below 4 GiB");
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
    if (layout == QL_EIGHT_BIT) {  // MinMaxQuery::EightBit is set with dann_set_query_dtype(idx, DANN_MM8), never here
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

// ---- query dtype of MinMax indexes (MinMaxQuery::EightBit) -----------------------------------------------------------
// Kept in query_layout as QL_EIGHT_BIT, which dann_set_query_layout never stores: one word says what a query image is.
int32_t dann_set_query_dtype(dann_index* idx, int32_t dtype) try {
    CHECK_IDX(idx);
    const int32_t own = idx->cfg.dtype;
    if (dtype != own) {
        if (!dt_is_mm(dtype) || !dt_is_mm(own)) {
            set_error("dann_set_query_dtype: dtype %d is no query dtype of an index of dtype %d", dtype, own);
            return DANN_EINVAL;
        }
        if (dtype != DT_MM8) {  // the reference's mixed pairs are (8, 4), (8, 2), (8, 1)
            set_error("dann_set_query_dtype: queries of dtype %d against rows of dtype %d are not supported", dtype, own);
            return DANN_EUNSUPPORTED;
        }
        // the raw product of kernel::<8, M> is a u32 (minmax/vectors.rs:216-222)
        if ((uint64_t)idx->cfg.dim * 255u * ((1u << sq_bits(own)) - 1u) > 0xFFFFFFFFull) {
            set_error("dim %u: the inner product of an 8-bit query and a %d-bit MinMax row does not fit a u32", idx->cfg.dim,
                      sq_bits(own));
            return DANN_EINVAL;
        }
    }
    if (idx->server.load(std::memory_order_acquire)) {  // the resident kernel was sized and instantiated for a query form
        set_error("dann_set_query_dtype: stop the search server first");
        return DANN_EBUSY;
    }
    if (dt_is_mm(own)) idx->query_layout.store(dtype == own ? QL_SAME : QL_EIGHT_BIT, std::memory_order_relaxed);
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_get_query_dtype(const dann_index* idx, int32_t* out) try {
    if (!idx || !out) {
        set_error("null argument");
        return DANN_EINVAL;
    }
    const bool q8 = dt_is_mm(idx->cfg.dtype) && idx->query_layout.load(std::memory_order_relaxed) == QL_EIGHT_BIT;
    *out = q8 ? DT_MM8 : idx->cfg.dtype;
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

// ---- attributes of the diversity-aware search (search_diverse.hip) ---------------------------------------------------
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
