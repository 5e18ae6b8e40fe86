// api_search.hip -- the query-taking half of the C ABI of include/dann.h: distances, dann_query_*, expand-beam, and the
// Knn, range, filtered, diverse, rerank, flat and record searches.  The host-pointer forms stage their buffers through
// HostStage (host_stage.h); dann_search_batch's own transfer strategies are in host_search.hip.
#include <cmath>

#include "api_common.h"
#include "flat_gt_launch.h"
#include "flat_plan.h"
#include "flat_pq_plan.h"
#include "wave_lists.h"  // kTagReadable

namespace dann {

uint32_t auto_visited_entries(const dann_index* idx, uint32_t, uint32_t) {
    if (idx->visited_bits >= 64) return std::min<uint32_t>((idx->visited_bits + 63u) / 64u * 64u, 32768u);
    if (idx->visited_bits) return 1u << idx->visited_bits;
    return 0;  // sized per launch by search_with_retry (search_kernels.hip)
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
}  // namespace dann

using namespace dann;

extern "C" {

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
    const uint32_t want = idx->cfg.dtype == DT_PQ ? idx->layer_bytes : idx->query_bytes(layout);
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
    // one piece; extras: the range scratch lists' ids and distances
    HostStage hs;
    if (int32_t rc = hs.layout(ctx, nq, nq, {{queries, idx->query_bytes()}},
                               {{out_ids, (size_t)out_cap * 4}, {out_dists, (size_t)out_cap * 4}, {out_second_round, 4}},
                               HostStage::kCheckStats, {(size_t)nq * cap * 4, (size_t)nq * cap * 4}))
        return rc;
    SearchArgs a;
    a.ix = idx->qview();
    a.queries = hs.in(0);
    a.nq = nq;
    a.l_value = starting_l;
    a.beam_width = beam_width;
    a.k = out_cap;
    a.ht_entries = auto_visited_entries(idx, std::max<uint32_t>(starting_l, 64), beam_width);
    a.out_ids = hs.out<uint32_t>(0);
    a.out_dists = hs.out<float>(1);
    a.stats = hs.stats();
    a.range_ids = hs.extra<uint32_t>(0);
    a.range_d = hs.extra<float>(1);
    a.range_second = hs.out<uint32_t>(2);
    a.range_cap = (uint32_t)cap;
    a.range_max = max_returned ? max_returned : 0xFFFFFFFFu;
    a.range_thresh = (uint32_t)((float)starting_l * initial_slack);
    a.has_inner = has_inner_radius ? 1u : 0u;
    a.radius = radius;
    a.inner_radius = inner_radius;
    a.range_slack = range_slack;
    uint32_t bad = nq;
    if (int32_t rc = hs.walk(out_stats, &bad, [&](uint32_t, uint32_t) { return search_with_retry(idx, ctx, a); })) return rc;
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
    // extras: the filter bitmaps and the AdaptiveL table (whole-call uploads), then the chunk's matched ids, distances and
    // sort keys, the tie-order work area, and the range scratch lists' ids and distances
    const size_t fwords = f->stride_words ? (size_t)f->stride_words * c.nq : (size_t)words;
    HostStage hs;
    if (int32_t rc = hs.layout(ctx, c.nq, chunk, {{c.queries, idx->query_bytes()}},
                               {{c.out_ids, (size_t)c.k * 4}, {c.out_dists, (size_t)c.k * 4}, {c.out_second, c.range ? 4u : 0u}},
                               HostStage::kCheckStats,
                               {fwords * 4, tab.size() * 4, inl ? (size_t)chunk * m_cap * 4 : 0, inl ? (size_t)chunk * m_cap * 4 : 0,
                                inl ? (size_t)chunk * key_cap * 8 : 0, tie_rust ? (size_t)chunk * kTieWorkBytes : 0,
                                c.range ? (size_t)chunk * rcap * 4 : 0, c.range ? (size_t)chunk * rcap * 4 : 0}))
        return rc;
    DANN_HIP(hipMemcpyAsync(hs.extra<void>(0), f->bits, fwords * 4, hipMemcpyHostToDevice, st));
    if (!tab.empty()) {
        DANN_HIP(hipMemcpyAsync(hs.extra<void>(1), tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
        a.ad_table = hs.extra<uint32_t>(1);
    }
    if (tie_rust) a.tie_work = hs.extra<uint8_t>(5);
    if (inl) {
        a.m_ids = hs.extra<uint32_t>(2);
        a.m_d = hs.extra<float>(3);
        a.m_keys = hs.extra<unsigned long long>(4);
        a.m_cap = m_cap;
        a.key_cap = key_cap;
    }
    if (c.range) {
        a.range_ids = hs.extra<uint32_t>(6);
        a.range_d = hs.extra<float>(7);
        a.range_second = hs.out<uint32_t>(2);
        a.range_cap = (uint32_t)rcap;
        a.range_max = c.max_returned ? c.max_returned : 0xFFFFFFFFu;
        a.range_thresh = (uint32_t)((float)c.l_value * c.initial_slack);
        a.has_inner = c.has_inner ? 1u : 0u;
        a.radius = c.radius;
        a.inner_radius = c.inner_radius;
        a.range_slack = c.range_slack;
    }
    a.out_ids = hs.out<uint32_t>(0);
    a.out_dists = hs.out<float>(1);
    a.stats = hs.stats();
    a.queries = hs.in(0);
    uint32_t bad = c.nq;
    if (int32_t rc = hs.walk(c.out_stats, &bad, [&](uint32_t off, uint32_t m) {
            a.nq = m;
            a.filter = hs.extra<uint32_t>(0) + (size_t)off * f->stride_words;
            return search_with_retry(idx, ctx, a);
        }))
        return rc;
    if (bad < c.nq) {
        set_error("query %u: per-query scratch exhausted (matched list %u entries, result list %llu, visited "
                  "table); raise dann_filter.matched_cap / out_cap", bad, m_cap, (unsigned long long)rcap);
        return DANN_EOVERFLOW;
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
    HostStage hs;
    if (int32_t rc = hs.layout(ctx, nq, 65536u, {{queries, idx->query_bytes()}},
                               {{out_ids, (size_t)k * 4}, {out_dists, (size_t)k * 4}}, HostStage::kCopyStats))
        return rc;
    return hs.walk(out_stats, nullptr, [&](uint32_t, uint32_t m) {
        return diverse_search_device(idx, ctx.stream, hs.in(0), m, l_value, beam_width, k, params->diverse_k, params->total_k,
                                     hs.out<uint32_t>(0), hs.out<float>(1), hs.stats());
    });
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
    ArenaTrim _trim{idx->main};
    HostStage hs;  // one piece; the candidate ids are a second per-query input
    if (int32_t rc = hs.layout(idx->main, nq, nq, {{queries, idx->query_bytes()}, {cand_ids, (size_t)cand_stride * 4}},
                               {{out_ids, (size_t)k * 4}, {out_dists, (size_t)k * 4}}, HostStage::kNoStats))
        return rc;
    return hs.walk(nullptr, nullptr, [&](uint32_t, uint32_t) {
        return launch_rerank(idx->qview(), hs.in(0), nq, hs.in<uint32_t>(1), cand_stride, k, hs.out<uint32_t>(0),
                             hs.out<float>(1), idx->main.stream);
    });
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
        set_error("dann_flat_search_batch: not defined on DANN_PQ rows (dann_pq_linear_search_batch scans PQ codes)");
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

// -- the same under a filter and within a radius (flat_gt_kernels.hip)
// the filter of a call as the kernels take it: null bits = every slot matches
struct FlatFilterArg {
    const uint32_t* bits = nullptr;
    uint64_t stride = 0;
};

int32_t flat_filter_check(const char* who, const dann_index* idx, const dann_flat_filter* filter, FlatFilterArg* f) {
    f->bits = filter ? filter->bits : nullptr;
    f->stride = f->bits ? filter->stride_words : 0;
    const uint64_t words = ((uint64_t)idx->nslots + 31) / 32;
    if (f->stride && f->stride < words) {
        set_error("%s: filter stride %llu words is shorter than one bitmap (%llu words)", who, (unsigned long long)f->stride,
                  (unsigned long long)words);
        return DANN_EINVAL;
    }
    return DANN_OK;
}

int32_t flat_filtered_make_plan(const dann_index* idx, uint32_t nq, uint32_t n, uint32_t k, FlatFilteredPlan* plan) {
    const IndexView ix = idx->qview();
    *plan = flat_filtered_plan(n, nq, k, flat_query_slot_bytes(ix), idx->num_cus, idx->dbg_u32(DANN_DBG_FLAT_CHUNK_ROWS, 0u));
    if (plan->p.tile == 0) {
        set_error("dann_flat_filtered_search_batch: a query of %u bytes with k = %u does not fit the LDS", ix.qbytes, k);
        return DANN_EUNSUPPORTED;
    }
    if (idx->verbose())
        fprintf(stderr, "[dann] filtered flat scan: n %u nq %u k %u -> tile %u, %u chunks of %u slots, %u queries per launch\n",
                n, nq, k, plan->p.tile, plan->p.nchunks, plan->p.chunk_rows, plan->p.batch);
    return DANN_OK;
}

// the filtered scan of nq queries on device buffers, plan.p.batch queries per launch; d_bits: the bitmaps of these queries
int32_t flat_filtered_run(dann_index* idx, hipStream_t st, const FlatFilteredPlan& plan, void* scratch, const void* d_queries,
                          uint32_t nq, uint32_t first_slot, uint32_t n, uint32_t flags, const uint32_t* d_bits, uint64_t stride,
                          uint32_t* d_ids, float* d_dists, dann_search_stats* d_stats) {
    const IndexView ix = idx->qview();
    const uint32_t* deleted = (flags & DANN_FLAT_SKIP_DELETED) ? idx->d_deleted : nullptr;
    const uint32_t k = plan.p.k;
    for (uint32_t off = 0; off < nq; off += plan.p.batch) {
        const uint32_t m = std::min(plan.p.batch, nq - off);
        int32_t rc = launch_flat_filtered_search(ix, plan, (const uint8_t*)d_queries + (size_t)off * ix.qbytes, m, first_slot, n,
                                                 deleted, d_bits + (size_t)off * stride, stride, scratch, d_ids + (size_t)off * k,
                                                 d_dists + (size_t)off * k, d_stats ? d_stats + off : nullptr, st);
        if (rc != DANN_OK) return rc;
    }
    return DANN_OK;
}

struct FlatRangeCall {
    uint32_t first_slot, n;
    float radius, inner_radius;
    bool has_inner;
    uint32_t flags, out_cap;
};

// the checks both forms of the range scan share; DANN_OK with *done set: nothing to launch and nothing to write
int32_t flat_range_check(const dann_index* idx, const void* queries, uint32_t nq, const FlatRangeCall& c, const uint32_t* out_ids,
                         const float* out_dists, const uint32_t* out_counts, bool* done) {
    *done = false;
    if (c.flags & ~(uint32_t)DANN_FLAT_SKIP_DELETED) {
        set_error("dann_flat_range_search_batch: unknown flag bits 0x%x", c.flags & ~(uint32_t)DANN_FLAT_SKIP_DELETED);
        return DANN_EINVAL;
    }
    if (c.radius != c.radius) {
        set_error("dann_flat_range_search_batch: the radius is NaN");
        return DANN_EINVAL;
    }
    if (c.has_inner && !(c.inner_radius <= c.radius)) {  // RangeSearchError::InnerRadiusGreaterThanRadius; a NaN too
        set_error("dann_flat_range_search_batch: inner radius %g must not exceed the radius %g", c.inner_radius, c.radius);
        return DANN_EINVAL;
    }
    if (idx->cfg.dtype == DT_PQ) {
        set_error("dann_flat_range_search_batch: not defined on DANN_PQ rows (dann_pq_linear_search_batch scans PQ codes)");
        return DANN_EUNSUPPORTED;
    }
    if ((uint64_t)c.first_slot + c.n > idx->nslots) {
        set_error("dann_flat_range_search_batch: slots [%u, %llu) leave the index's %u slots", c.first_slot,
                  (unsigned long long)c.first_slot + c.n, idx->nslots);
        return DANN_EBOUNDS;
    }
    if (nq == 0) {
        *done = true;
        return DANN_OK;
    }
    if (!queries || !out_counts || (c.out_cap && (!out_ids || !out_dists))) {
        set_error("dann_flat_range_search_batch: null pointer");
        return DANN_EINVAL;
    }
    return DANN_OK;
}

int32_t flat_range_make_plan(const dann_index* idx, uint32_t nq, uint32_t n, FlatRangePlan* plan) {
    const IndexView ix = idx->qview();
    *plan = flat_range_plan(n, nq, flat_query_slot_bytes(ix), idx->num_cus, idx->dbg_u32(DANN_DBG_FLAT_CHUNK_ROWS, 0u));
    if (plan->tile == 0) {
        set_error("dann_flat_range_search_batch: a query of %u bytes does not fit the LDS", ix.qbytes);
        return DANN_EUNSUPPORTED;
    }
    if (idx->verbose())
        fprintf(stderr, "[dann] flat range scan: n %u nq %u -> tile %u, %u chunks of %u slots, %u queries per launch\n", n, nq,
                plan->tile, plan->nchunks, plan->chunk_rows, plan->batch);
    return DANN_OK;
}

// the range scan of nq queries on device buffers, plan.batch queries per launch; the overflow flag behind the counts is
// cleared first and stays set once any query had more matches than out_cap
int32_t flat_range_run(dann_index* idx, hipStream_t st, const FlatRangePlan& plan, void* scratch, const void* d_queries,
                       uint32_t nq, const FlatRangeCall& c, const uint32_t* d_bits, uint64_t stride, uint32_t* d_ids,
                       float* d_dists, uint32_t* d_counts, dann_search_stats* d_stats) {
    const IndexView ix = idx->qview();
    const uint32_t* deleted = (c.flags & DANN_FLAT_SKIP_DELETED) ? idx->d_deleted : nullptr;
    DANN_HIP(hipMemsetAsync(flat_range_overflow_flag(plan, scratch), 0, 4, st));
    for (uint32_t off = 0; off < nq; off += plan.batch) {
        const uint32_t m = std::min(plan.batch, nq - off);
        int32_t rc = launch_flat_range_search(
            ix, plan, (const uint8_t*)d_queries + (size_t)off * ix.qbytes, m, c.first_slot, c.n, c.radius, c.has_inner,
            c.inner_radius, deleted, d_bits ? d_bits + (size_t)off * stride : nullptr, stride, c.out_cap, scratch,
            d_ids ? d_ids + (size_t)off * c.out_cap : nullptr, d_dists ? d_dists + (size_t)off * c.out_cap : nullptr,
            d_counts + off, d_stats ? d_stats + off : nullptr, st);
        if (rc != DANN_OK) return rc;
    }
    return DANN_OK;
}

int32_t flat_range_overflowed(uint32_t out_cap) {
    set_error("dann_flat_range_search_batch: a query has more matches than out_cap = %u (out_counts holds the true counts, "
              "out_stats[q].status names the queries)", out_cap);
    return DANN_EOVERFLOW;
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
    // pieces of at most 65536 queries, the plan made for one piece; extra: the plan's chunk lists
    const uint32_t piece = std::min<uint32_t>(nq, 65536u);
    FlatPlan plan;
    if (n != 0)
        if (int32_t rc = flat_make_plan(idx, piece, n, k, &plan)) return rc;
    HostStage hs;
    if (int32_t rc = hs.layout(ctx, nq, piece, {{queries, idx->query_bytes()}},
                               {{out_ids, (size_t)k * 4}, {out_dists, (size_t)k * 4}}, HostStage::kCopyStats,
                               {n != 0 ? plan.scratch_bytes() : 0}))
        return rc;
    return hs.walk(out_stats, nullptr, [&](uint32_t, uint32_t m) {
        return n == 0 ? launch_flat_empty(m, k, hs.out<uint32_t>(0), hs.out<float>(1), hs.stats(), ctx.stream)
                      : flat_run(idx, ctx.stream, plan, hs.extra<void>(0), hs.in(0), m, first_slot, n, flags,
                                 hs.out<uint32_t>(0), hs.out<float>(1), hs.stats());
    });
} DANN_CATCH_ALL

// ---- exhaustive scans under a filter and within a radius (flat_gt_kernels.hip; helpers next to flat_check above) ----

int32_t dann_flat_filtered_search_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, uint32_t first_slot,
                                               uint32_t n, uint32_t k, uint32_t flags, const dann_flat_filter* d_filter,
                                               uint32_t* d_out_ids, float* d_out_dists, dann_search_stats* d_out_stats) try {
    if (!d_filter || !d_filter->bits)  // every slot matches: the unfiltered scan
        return dann_flat_search_batch_device(idx, d_queries, nq, first_slot, n, k, flags, d_out_ids, d_out_dists, d_out_stats);
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    bool done = false;
    if (int32_t rc = flat_check(idx, d_queries, nq, first_slot, n, k, flags, d_out_ids, d_out_dists, &done)) return rc;
    FlatFilterArg f;
    if (int32_t rc = flat_filter_check("dann_flat_filtered_search_batch", idx, d_filter, &f)) return rc;
    if (done) return DANN_OK;
    if (n == 0) {
        if (int32_t rc = launch_flat_empty(nq, k, d_out_ids, d_out_dists, d_out_stats, ctx.stream)) return rc;
    } else {
        FlatFilteredPlan plan;
        if (int32_t rc = flat_filtered_make_plan(idx, nq, n, k, &plan)) return rc;
        if (int32_t rc = grow_stage(ctx, 4, plan.scratch_bytes())) return rc;
        if (int32_t rc = flat_filtered_run(idx, ctx.stream, plan, ctx.stage[4], d_queries, nq, first_slot, n, flags, f.bits,
                                           f.stride, d_out_ids, d_out_dists, d_out_stats))
            return rc;
    }
    DANN_HIP(hipStreamSynchronize(ctx.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_flat_filtered_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                                        uint32_t k, uint32_t flags, const dann_flat_filter* filter, uint32_t* out_ids,
                                        float* out_dists, dann_search_stats* out_stats) try {
    if (!filter || !filter->bits)  // every slot matches: the unfiltered scan
        return dann_flat_search_batch(idx, queries, nq, first_slot, n, k, flags, out_ids, out_dists, out_stats);
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    bool done = false;
    if (int32_t rc = flat_check(idx, queries, nq, first_slot, n, k, flags, out_ids, out_dists, &done)) return rc;
    FlatFilterArg f;
    if (int32_t rc = flat_filter_check("dann_flat_filtered_search_batch", idx, filter, &f)) return rc;
    if (done) return DANN_OK;
    // pieces by flat_host_piece, the plan made for one piece; a shared bitmap goes up once.  extras: the plan's chunk lists, the shared bitmap
    const size_t words = ((size_t)idx->nslots + 31) / 32;
    const uint32_t piece = flat_host_piece(nq, f.stride, 0);
    FlatFilteredPlan plan;
    if (n != 0)
        if (int32_t rc = flat_filtered_make_plan(idx, piece, n, k, &plan)) return rc;
    const size_t scratch = n != 0 ? plan.scratch_bytes() : 0;
    HostStage hs;
    const int32_t lrc =
        f.stride ? hs.layout(ctx, nq, piece, {{queries, idx->query_bytes()}, {f.bits, (size_t)f.stride * 4}},
                             {{out_ids, (size_t)k * 4}, {out_dists, (size_t)k * 4}}, HostStage::kCopyStats, {scratch})
                 : hs.layout(ctx, nq, piece, {{queries, idx->query_bytes()}},
                             {{out_ids, (size_t)k * 4}, {out_dists, (size_t)k * 4}}, HostStage::kCopyStats, {scratch, words * 4});
    if (lrc) return lrc;
    if (!f.stride) DANN_HIP(hipMemcpyAsync(hs.extra<void>(1), f.bits, words * 4, hipMemcpyHostToDevice, ctx.stream));
    return hs.walk(out_stats, nullptr, [&](uint32_t, uint32_t m) {
        return n == 0 ? launch_flat_empty(m, k, hs.out<uint32_t>(0), hs.out<float>(1), hs.stats(), ctx.stream)
                      : flat_filtered_run(idx, ctx.stream, plan, hs.extra<void>(0), hs.in(0), m, first_slot, n, flags,
                                          f.stride ? hs.in<uint32_t>(1) : hs.extra<uint32_t>(1), f.stride, hs.out<uint32_t>(0),
                                          hs.out<float>(1), hs.stats());
    });
} DANN_CATCH_ALL

// ---- exhaustive scan over PQ code rows (flat_pq_kernels.hip): algos::linear_search ------------------------------------
}  // extern "C"
namespace {
// the checks both forms share; DANN_OK with *done set: nothing to launch and nothing to write
int32_t pq_linear_check(const dann_index* idx, const float* queries, uint32_t nq, uint32_t first_slot, uint32_t n, uint32_t k,
                        uint32_t flags, const dann_flat_filter* filter, const uint32_t* out_ids, const float* out_dists,
                        FlatFilterArg* f, bool* done) {
    *done = false;
    if (idx->cfg.dtype != DT_PQ) {
        set_error("dann_pq_linear_search_batch: defined on DANN_PQ rows only (dann_flat_search_batch scans the other row types)");
        return DANN_EUNSUPPORTED;
    }
    if (flags & ~(uint32_t)DANN_FLAT_SKIP_DELETED) {
        set_error("dann_pq_linear_search_batch: unknown flag bits 0x%x", flags & ~(uint32_t)DANN_FLAT_SKIP_DELETED);
        return DANN_EINVAL;
    }
    if (k == 0) {
        set_error("dann_pq_linear_search_batch: k cannot be zero");
        return DANN_EINVAL;
    }
    if (k > kFlatMaxK) {
        set_error("dann_pq_linear_search_batch: k = %u exceeds the supported maximum of %u", k, kFlatMaxK);
        return DANN_EUNSUPPORTED;
    }
    if (int32_t rc = pq_ready(idx)) return rc;
    if ((uint64_t)first_slot + n > idx->nslots) {
        set_error("dann_pq_linear_search_batch: slots [%u, %llu) leave the index's %u slots", first_slot,
                  (unsigned long long)first_slot + n, idx->nslots);
        return DANN_EBOUNDS;
    }
    if (int32_t rc = flat_filter_check("dann_pq_linear_search_batch", idx, filter, f)) return rc;
    if (nq == 0) {
        *done = true;
        return DANN_OK;
    }
    if (!queries || !out_ids || !out_dists) {
        set_error("dann_pq_linear_search_batch: null pointer");
        return DANN_EINVAL;
    }
    return DANN_OK;
}

// how the scan of `nq` queries is cut up (flat_pq_plan.h)
FlatPqPlan pq_linear_make_plan(const dann_index* idx, uint32_t nq, uint32_t n, uint32_t k) {
    const FlatPqPlan plan =
        flat_pq_plan(idx->cfg.pq_chunks, n, nq, k, idx->num_cus, idx->dbg_u32(DANN_DBG_FLAT_CHUNK_ROWS, 0u));
    if (idx->verbose())
        fprintf(stderr, "[dann] PQ linear scan: %u chunks n %u nq %u k %u -> tile %u, %u chunks of %u slots, %u queries per launch\n",
                plan.chunks, n, nq, k, plan.tile, plan.nchunks, plan.chunk_rows, plan.batch);
    return plan;
}

// the scan of nq queries (at most as many as the plan was made for) on device buffers, plan.batch queries per launch;
// `scratch`: plan.scratch_bytes(); d_bits: the bitmaps of these queries (null: none)
int32_t pq_linear_run(dann_index* idx, hipStream_t st, const FlatPqPlan& plan, void* scratch, const float* d_queries, uint32_t nq,
                      uint32_t first_slot, uint32_t n, uint32_t flags, const uint32_t* d_bits, uint64_t stride, uint32_t* d_ids,
                      float* d_dists, dann_search_stats* d_stats) {
    const IndexView ix = idx->qview();
    const uint32_t* deleted = (flags & DANN_FLAT_SKIP_DELETED) ? idx->d_deleted : nullptr;
    for (uint32_t off = 0; off < nq; off += plan.batch) {
        const uint32_t m = std::min(plan.batch, nq - off);
        int32_t rc = launch_flat_pq_search(ix, plan, d_queries + (size_t)off * ix.dim, m, first_slot, n, deleted,
                                           d_bits ? d_bits + (size_t)off * stride : nullptr, stride, scratch,
                                           d_ids + (size_t)off * plan.k, d_dists + (size_t)off * plan.k,
                                           d_stats ? d_stats + off : nullptr, st);
        if (rc != DANN_OK) return rc;
    }
    return DANN_OK;
}
}  // namespace
extern "C" {

int32_t dann_pq_linear_search_batch_device(dann_index* idx, const float* d_queries, uint32_t nq, uint32_t first_slot,
                                           uint32_t n, uint32_t k, uint32_t flags, const dann_flat_filter* d_filter,
                                           uint32_t* d_out_ids, float* d_out_dists, dann_search_stats* d_out_stats) try {
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    bool done = false;
    FlatFilterArg f;
    if (int32_t rc = pq_linear_check(idx, d_queries, nq, first_slot, n, k, flags, d_filter, d_out_ids, d_out_dists, &f, &done))
        return rc;
    if (done) return DANN_OK;
    if (n == 0) {
        if (int32_t rc = launch_flat_empty(nq, k, d_out_ids, d_out_dists, d_out_stats, ctx.stream)) return rc;
    } else {
        const FlatPqPlan plan = pq_linear_make_plan(idx, nq, n, k);
        if (int32_t rc = grow_stage(ctx, 4, plan.scratch_bytes())) return rc;
        if (int32_t rc = pq_linear_run(idx, ctx.stream, plan, ctx.stage[4], d_queries, nq, first_slot, n, flags, f.bits, f.stride,
                                       d_out_ids, d_out_dists, d_out_stats))
            return rc;
    }
    DANN_HIP(hipStreamSynchronize(ctx.stream));
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_pq_linear_search_batch(dann_index* idx, const float* queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                                    uint32_t k, uint32_t flags, const dann_flat_filter* filter, uint32_t* out_ids,
                                    float* out_dists, dann_search_stats* out_stats) try {
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    bool done = false;
    FlatFilterArg f;
    if (int32_t rc = pq_linear_check(idx, queries, nq, first_slot, n, k, flags, filter, out_ids, out_dists, &f, &done)) return rc;
    if (done) return DANN_OK;
    // pieces by flat_host_piece, the plan made for one piece; a shared bitmap goes up once.  extras: the plan's scratch, the
    // shared bitmap
    const size_t words = ((size_t)idx->nslots + 31) / 32;
    const uint32_t piece = flat_host_piece(nq, f.stride, 0);
    FlatPqPlan plan;
    if (n != 0) plan = pq_linear_make_plan(idx, piece, n, k);
    const size_t scratch = n != 0 ? plan.scratch_bytes() : 0;
    const bool shared = f.bits && !f.stride;
    HostStage hs;
    const int32_t lrc =
        f.stride ? hs.layout(ctx, nq, piece, {{queries, idx->query_bytes()}, {f.bits, (size_t)f.stride * 4}},
                             {{out_ids, (size_t)k * 4}, {out_dists, (size_t)k * 4}}, HostStage::kCopyStats, {scratch})
                 : hs.layout(ctx, nq, piece, {{queries, idx->query_bytes()}},
                             {{out_ids, (size_t)k * 4}, {out_dists, (size_t)k * 4}}, HostStage::kCopyStats,
                             {scratch, shared ? words * 4 : 0});
    if (lrc) return lrc;
    if (shared) DANN_HIP(hipMemcpyAsync(hs.extra<void>(1), f.bits, words * 4, hipMemcpyHostToDevice, ctx.stream));
    return hs.walk(out_stats, nullptr, [&](uint32_t, uint32_t m) {
        const uint32_t* d_bits = f.stride ? hs.in<uint32_t>(1) : shared ? hs.extra<uint32_t>(1) : nullptr;
        return n == 0 ? launch_flat_empty(m, k, hs.out<uint32_t>(0), hs.out<float>(1), hs.stats(), ctx.stream)
                      : pq_linear_run(idx, ctx.stream, plan, hs.extra<void>(0), hs.in<float>(0), m, first_slot, n, flags, d_bits,
                                      f.stride, hs.out<uint32_t>(0), hs.out<float>(1), hs.stats());
    });
} DANN_CATCH_ALL

int32_t dann_flat_range_search_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, uint32_t first_slot,
                                            uint32_t n, float radius, int32_t has_inner_radius, float inner_radius,
                                            uint32_t flags, const dann_flat_filter* d_filter, uint32_t out_cap,
                                            uint32_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                            dann_search_stats* d_out_stats) try {
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    const FlatRangeCall c{first_slot, n, radius, inner_radius, has_inner_radius != 0, flags, out_cap};
    bool done = false;
    if (int32_t rc = flat_range_check(idx, d_queries, nq, c, d_out_ids, d_out_dists, d_out_counts, &done)) return rc;
    FlatFilterArg f;
    if (int32_t rc = flat_filter_check("dann_flat_range_search_batch", idx, d_filter, &f)) return rc;
    if (done) return DANN_OK;
    FlatRangePlan plan;
    if (int32_t rc = flat_range_make_plan(idx, nq, n, &plan)) return rc;
    if (int32_t rc = grow_stage(ctx, 4, plan.scratch_bytes())) return rc;
    if (int32_t rc = flat_range_run(idx, ctx.stream, plan, ctx.stage[4], d_queries, nq, c, f.bits, f.stride, d_out_ids,
                                    d_out_dists, d_out_counts, d_out_stats))
        return rc;
    uint32_t over = 0;
    DANN_HIP(hipMemcpyAsync(&over, flat_range_overflow_flag(plan, ctx.stage[4]), 4, hipMemcpyDeviceToHost, ctx.stream));
    DANN_HIP(hipStreamSynchronize(ctx.stream));
    return over ? flat_range_overflowed(out_cap) : DANN_OK;
} DANN_CATCH_ALL

int32_t dann_flat_range_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                                     float radius, int32_t has_inner_radius, float inner_radius, uint32_t flags,
                                     const dann_flat_filter* filter, uint32_t out_cap, uint32_t* out_ids, float* out_dists,
                                     uint32_t* out_counts, dann_search_stats* out_stats) try {
    CHECK_IDX_SHARED(idx);
    ArenaTrim _trim{ctx};
    const FlatRangeCall c{first_slot, n, radius, inner_radius, has_inner_radius != 0, flags, out_cap};
    bool done = false;
    if (int32_t rc = flat_range_check(idx, queries, nq, c, out_ids, out_dists, out_counts, &done)) return rc;
    FlatFilterArg f;
    if (int32_t rc = flat_filter_check("dann_flat_range_search_batch", idx, filter, &f)) return rc;
    if (done) return DANN_OK;
    // pieces by flat_host_piece
    const size_t words = ((size_t)idx->nslots + 31) / 32;
    const uint32_t piece = flat_host_piece(nq, f.stride, out_cap);
    FlatRangePlan plan;
    if (int32_t rc = flat_range_make_plan(idx, piece, n, &plan)) return rc;
    const size_t row = (size_t)out_cap * 4;
    uint32_t* const h_ids = out_cap ? out_ids : nullptr;
    float* const h_dists = out_cap ? out_dists : nullptr;
    HostStage hs;
    const int32_t lrc =
        f.stride ? hs.layout(ctx, nq, piece, {{queries, idx->query_bytes()}, {f.bits, (size_t)f.stride * 4}},
                             {{h_ids, row}, {h_dists, row}, {out_counts, 4}}, HostStage::kCopyStats, {plan.scratch_bytes()})
                 : hs.layout(ctx, nq, piece, {{queries, idx->query_bytes()}}, {{h_ids, row}, {h_dists, row}, {out_counts, 4}},
                             HostStage::kCopyStats, {plan.scratch_bytes(), f.bits ? words * 4 : 0});
    if (lrc) return lrc;
    if (f.bits && !f.stride) DANN_HIP(hipMemcpyAsync(hs.extra<void>(1), f.bits, words * 4, hipMemcpyHostToDevice, ctx.stream));
    if (int32_t rc = hs.walk(out_stats, nullptr, [&](uint32_t, uint32_t m) {
            const uint32_t* d_bits = !f.bits ? nullptr : f.stride ? hs.in<uint32_t>(1) : hs.extra<uint32_t>(1);
            return flat_range_run(idx, ctx.stream, plan, hs.extra<void>(0), hs.in(0), m, c, d_bits, f.stride,
                                  out_cap ? hs.out<uint32_t>(0) : nullptr, out_cap ? hs.out<float>(1) : nullptr,
                                  hs.out<uint32_t>(2), hs.stats());
        }))
        return rc;
    for (uint32_t i = 0; out_cap && i < nq; ++i)
        if (out_counts[i] > out_cap) return flat_range_overflowed(out_cap);
    return DANN_OK;
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
    ArenaTrim _trim{idx->main};
    HostStage hs;  // one piece; its input is the slots or the queries
    if (int32_t rc = hs.layout(idx->main, nq, nq, {{slots ? (const void*)slots : queries, slots ? 4u : idx->query_bytes()}},
                               {{rec_ids, (size_t)rec_stride * 4}, {rec_dists, (size_t)rec_stride * 4}, {rec_n, 4}},
                               HostStage::kCheckStats))
        return rc;
    uint32_t bad = nq;
    if (int32_t rc = hs.walk(out_stats, &bad, [&](uint32_t, uint32_t) {
            return search_device(idx, idx->main, slots ? nullptr : hs.in(0), slots ? hs.in<uint32_t>(0) : nullptr, nq, l_value,
                                 1, 0, nullptr, nullptr, hs.stats(), hs.out<uint32_t>(0), hs.out<float>(1), rec_stride,
                                 hs.out<uint32_t>(2));
        }))
        return rc;
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

}  // extern "C"
