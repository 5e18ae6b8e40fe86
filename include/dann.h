/*
 * dann.h -- C ABI of the MI355X-native DiskANN hot path (libdann_hip.so).
 *
 * This is the drop-in boundary: the batched distance-evaluation path inside Vamana beam
 * search and RobustPrune index build, behind the surface of the reference's
 * `diskann-inmem` provider.  Each entry point names the reference interface it
 * replaces (paths relative to the microsoft/DiskANN Rust workspace, v0.56).  The
 * reference-side binding a maintainer would add (Rust `extern "C"` block + adapter) is
 * shown in INTEGRATION.md.
 *
 * Conventions (those of the reference's only C surface, diskann-garnet/src/lib.rs:261-372,
 * 682-756): opaque handles, caller-owned buffers passed as pointer + length, `int32_t`
 * status (>= 0 ok, < 0 one of DANN_E*), no exceptions or aborts cross the boundary,
 * a thread-local message is available from dann_last_error().  Entry points are
 * thread-safe.  Threading model (the reference: N workers on one shared `&DiskANNIndex`, for every search kind):
 * dann_search_batch(_device), dann_range_search_batch, dann_filtered_search_batch, dann_filtered_range_search_batch,
 * dann_paged_begin / dann_paged_next take the index shared -- calls from different threads run side by side on the
 * device, each on its own stream and scratch (a pool of search contexts) -- and the server entry points
 * (dann_search_submit / wait / poll) take no lock at all; everything that mutates the index, and the fine-grained
 * seam and the record / rerank entry points, take it exclusively and wait for the searches in flight (the GPU index
 * is an immutable snapshot between mutations; the reference's EBR / tag machinery stays on the host).
 *
 * All "host" pointers are plain host memory; `_device` variants take HIP device
 * pointers that live on the index's device.
 */
#ifndef DANN_H
#define DANN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element type of the stored rows: layers::Full<T>, diskann-inmem/src/layers/full.rs:351-504 */
typedef enum {
    DANN_F32 = 0,
    DANN_F16 = 1,
    DANN_U8 = 2,
    DANN_I8 = 3,
    /* 8-bit scalar-quantised rows: `dim` code bytes followed by the f32 compensation
     * (CompensatedVector<8>, diskann-quantization/src/scalar/vectors.rs:150-175); distances are
     * CompensatedSquaredL2 / CompensatedIP / CompensatedCosineNormalized (:171-465).  Queries are
     * compressed the same way (symmetric, diskann-providers/.../inmem/scalar.rs:261-320). */
    DANN_SQ8 = 4,
    /* product-quantised rows: `pq_chunks` code bytes per row; queries are full-precision f32 vectors,
     * distances are lookup-table sums (diskann-providers/src/model/pq/fixed_chunk_pq_table.rs:82-192).
     * The pivot table is attached with dann_set_pq_table(); search entry points only -- the fine-grained
     * seam for PQ rows is dann_pq_build_lut / dann_pq_scan, dann_expand_beam returns DANN_EINVAL -- (re-rank the
     * candidates on a full-precision index with dann_rerank_batch). */
    DANN_PQ = 5,
    /* packed scalar-quantised rows, value 16 + bits (6 and 7 are not dtypes): ceil(dim * bits / 8) code bytes,
     * element i at bits [i * bits, (i + 1) * bits) little-endian within a byte (4-bit 1,2,3,4 = 0x21 0x43), then the
     * f32 compensation: CompensatedVector<1> / <4> in its canonical form, Dense permutation (scalar/vectors.rs:128-175).
     * Metrics, queries and sq_scale / sq_shift_norm_sq as for DANN_SQ8; the epilogue's constant is
     * (1/(2^bits - 1))^2 * scale^2.  Bits beyond dim never take part, whatever they hold. */
    DANN_SQ1 = 17,
    DANN_SQ4 = 20,
    /* spherically quantised rows (RaBitQ), value 32 + bits: the back-canonical byte image of spherical::Data<NBITS>
     * (diskann-quantization/src/spherical/vectors.rs) -- ceil(dim * bits / 8) code bytes in the Dense permutation,
     * packed as DANN_SQ1 / DANN_SQ4, then the 6-byte DataMeta (:219-247): f16 inner_product_correction, f16
     * metric_specific, u16 bit_sum.  `dim` is the quantiser's output dimension (SphericalQuantizer::output_dim(); a
     * padding transform makes it differ from the data's) and dim * (2^bits - 1) must fit the u16 (else DANN_EINVAL).
     * Metrics: DANN_L2, DANN_INNER_PRODUCT, DANN_COSINE (SupportedMetric; DANN_COSINE_NORMALIZED: DANN_EINVAL).
     * Distances are CompensatedSquaredL2 / CompensatedIP / CompensatedCosine (:494-528 the kernel, :584-636 L2,
     * :744-801 inner product, :867-892 cosine), bit for bit.  sq_shift_norm_sq carries CompensatedIP::squared_shift_norm
     * (inner product and cosine), sq_scale is ignored.  The index takes byte images of rows and queries; dann_spherical_compress(_device)
     * and dann_spherical_compress_queries(_device) make them from f32 vectors on the GPU (the host keeps training the
     * quantiser); the form of a query is set with dann_set_query_layout().  Elements at or beyond dim never
     * take part, whatever the padding bits hold. */
    DANN_SPH1 = 33,
    DANN_SPH2 = 34,
    DANN_SPH4 = 36,
    /* MinMax-quantised rows, value 48 + bits: the front-canonical byte image of minmax::Data<NBITS>
     * (diskann-quantization/src/minmax/vectors.rs, meta/vector.rs:124-146; what MinMax8 / MinMax4 of
     * diskann-providers/src/common/minmax_repr.rs and Garnet's MinMax8Bit store) -- the 20-byte MinMaxCompensation
     * first (vectors.rs:43-51, little-endian: u32 dim, f32 b, f32 n, f32 a, f32 norm_squared), then ceil(dim * bits / 8)
     * code bytes in the Dense permutation, packed as DANN_SQ1 / DANN_SQ4 / DANN_SPH2 rows (8 bits: one byte per code).
     * `dim` is the quantiser's output_dim(); the kernels never read the header's dim, the host-pointer row writers
     * (dann_set_element(s), dann_load_vectors_bin, the start rows of dann_index_create, dann_query_create) answer
     * DANN_EINVAL for an image whose leading u32 differs from it, the device-pointer and verbatim paths do not look.
     * dim * (2^bits - 1)^2 must fit a u32 (else DANN_EINVAL).  All four metrics: MinMaxCosine, MinMaxIP,
     * MinMaxL2Squared, MinMaxCosineNormalized (vectors.rs:206-473, distance_comparer minmax_repr.rs:330-335), bit for
     * bit, the query (in prunes: the candidate under test) as the function's first argument -- the epilogue is not
     * symmetric in its arguments.  No training: sq_scale and sq_shift_norm_sq are ignored.  Queries are row images
     * (DANN_QUERY_SAME_AS_DATA).  Elements at or beyond dim never take part, whatever the padding bits hold. */
    DANN_MM1 = 49,
    DANN_MM2 = 50,
    DANN_MM4 = 52,
    DANN_MM8 = 56
} dann_dtype;

/* iface::QueryLayout: the byte image of a query of a spherical index.  QueryMeta is four f32: inner_product_correction,
 * bit_sum, offset, metric_specific (spherical/vectors.rs:381-399). */
typedef enum {
    DANN_QUERY_SAME_AS_DATA = 0,        /* a row image, code bytes + 6 (every width; the default)                      */
    DANN_QUERY_FOUR_BIT_TRANSPOSED = 1, /* 1-bit rows: per block of 64 elements four u64 words, word j = bit j of the
                                           64 four-bit values (bits/distances.rs:2123-2249): ceil(dim / 64) * 32 plane
                                           bytes, then the QueryMeta                                                   */
    DANN_QUERY_SCALAR_QUANTIZED = 2,    /* 2- and 4-bit rows: Dense codes of the rows' width, then the QueryMeta        */
    DANN_QUERY_FULL_PRECISION = 3,      /* reserved: DANN_EUNSUPPORTED (MinMax rows: see dann_set_query_dtype for the
                                           query form that is served)                                                  */
    /* 4 .. 7: DANN_EINVAL */
    DANN_QUERY_EIGHT_BIT = 8            /* MinMaxQuery::EightBit, an MM8 image against narrower MinMax rows: not set
                                           through dann_set_query_layout (DANN_EUNSUPPORTED on every index) but with
                                           dann_set_query_dtype(idx, DANN_MM8); dann_get_query_layout reports it then   */
} dann_query_layout;

/* == `#[repr(C)] enum Metric`, diskann-vector/src/distance/metric.rs:8-20 */
typedef enum {
    DANN_COSINE = 0,
    DANN_INNER_PRODUCT = 1,
    DANN_L2 = 2,
    DANN_COSINE_NORMALIZED = 3
} dann_metric;

enum {
    DANN_OK = 0,
    DANN_EINVAL = -1,    /* null pointer / zero L / zero beam width / bad enum         */
    DANN_ELENGTH = -2,   /* byte length does not match the layer (full.rs:228-241)    */
    DANN_EBOUNDS = -3,   /* slot id out of bounds (neighbors.rs:OutOfBounds)          */
    DANN_ETOOLONG = -4,  /* adjacency list longer than max_degree (neighbors.rs:TooLong) */
    DANN_EHIP = -5,      /* a HIP runtime call failed; see dann_last_error()          */
    DANN_ENOMEM = -6,
    DANN_EOVERFLOW = -7, /* per-query scratch (visited table / record) exhausted      */
    DANN_EUNSUPPORTED = -8,
    DANN_EINTERNAL = -9, /* a consistency check inside a kernel failed (a bug, never an input)  */
    DANN_EBUSY = -10     /* a mutation while search-server tickets are outstanding, or a submit during a mutation */
} /* dann_status */;

typedef struct dann_index dann_index; /* == diskann_inmem::Provider<Full<T>, _> + DiskANNIndex */
typedef struct dann_query dann_query; /* == layers::QueryDistance / ExpandBeam object   */

/* provider::Config + Full::new (diskann-inmem/src/provider.rs:160-217, 96-131) */
typedef struct {
    int32_t dtype;             /* dann_dtype  */
    int32_t metric;            /* dann_metric */
    uint32_t dim;
    uint32_t capacity;         /* dynamic slots [0, capacity)                              */
    uint32_t max_degree;       /* adjacency capacity per slot                              */
    uint32_t num_start_points; /* frozen slots [capacity, capacity+n) (store.rs:259-262)   */
    uint32_t row_stride;       /* bytes between rows; 0 = packed (dim*sizeof(T) rounded up
                                  to 16).  dann_inmem2_row_stride() gives the reference's
                                  own stride so a Store buffer can be uploaded verbatim    */
    int32_t device;            /* HIP device ordinal, -1 = current                         */
    float sq_scale;            /* DANN_SQ8 / SQ4 / SQ1 only: ScalarQuantizer::scale()       */
    float sq_shift_norm_sq;    /* DANN_SQ8 / SQ4 / SQ1 only: ScalarQuantizer::shift_square_norm() */
    uint32_t pq_chunks;        /* DANN_PQ only: code bytes per row (number of PQ chunks)    */
    uint32_t inline_tags;      /* 1: every row carries the reference's 1-byte concurrency tag right after its
                                  payload (Store layout, store.rs:133-158; needs row_stride > payload bytes, e.g.
                                  dann_inmem2_row_stride()).  A slot whose tag is below Tag::PUBLISHED (254,
                                  tag.rs:86-133) is not readable: searches skip it after the visited insert and
                                  do not count it (provider.rs:448-473, 681-686).  dann_upload_store() then copies
                                  the tag bytes verbatim, dann_set_element(s) publishes the slots it writes,
                                  start points are FROZEN (255).  0: no tags, every slot readable.            */
} dann_config;

/* graph::config::Builder (diskann/src/graph/config/mod.rs:261-338, defaults.rs:14-41) */
typedef struct {
    uint32_t pruned_degree;
    uint32_t max_degree;             /* "max_degree_with_slack"; <= dann_config.max_degree  */
    uint32_t l_build;
    float alpha;                     /* default 1.2                                         */
    uint32_t max_occlusion_size;     /* default 750                                         */
    uint32_t max_backedges;          /* single-insert only; default pruned_degree           */
    uint32_t intra_batch_candidates; /* 0 = None, n = Max(n), 0xFFFFFFFF = All              */
    uint32_t saturate_after_prune;   /* default 0                                           */
} dann_build_config;

/* per-query search statistics: SearchStats (diskann/src/graph/index.rs:90-102) */
typedef struct {
    uint32_t cmps;
    uint32_t hops;
    uint32_t result_count; /* SearchStats::result_count as the inmem2 provider reports it: its Translate
                              post-processor counts a push only while the buffer still has room afterwards
                              (provider.rs:933-944, search_output_buffer.rs:107-124), i.e. k-1 when the output
                              buffer of length k fills, else the number written.  Range searches (unbounded
                              output Vec) report the number written.                                  */
    uint32_t status;       /* 0 ok, else DANN_E* negated (per-query overflow reporting)      */
    uint32_t written;      /* entries actually written to out_ids / out_dists (what the reference's other
                              post-processors, e.g. the test provider's, return as the count)         */
} dann_search_stats;

/* ---- layer / lifetime ---------------------------------------------------------- */
/* Layer::bytes (layers/mod.rs:37-42): dim * sizeof(T), or DANN_EINVAL */
int32_t dann_layer_bytes(int32_t dtype, uint32_t dim);
/* Store row stride of the reference: round_up(bytes + 1 tag byte, 32) (store.rs:198-211) */
int32_t dann_inmem2_row_stride(int32_t dtype, uint32_t dim);
/* Provider::new + DiskANNIndex::new (provider.rs:96-131).  start_rows: num_start_points
 * rows of dann_layer_bytes() each. */
int32_t dann_index_create(const dann_config* cfg, const void* start_rows, uint64_t start_len,
                          dann_index** out);
int32_t dann_index_destroy(dann_index* idx);
int32_t dann_index_max_degree(const dann_index* idx);   /* Provider::max_degree */
int32_t dann_index_get_config(const dann_index* idx, dann_config* out);

/* ---- vectors: Set::set / SetElement::set_element (full.rs:110-130, provider.rs:334-373) */
int32_t dann_set_element(dann_index* idx, uint32_t slot, const void* bytes, uint64_t len);
int32_t dann_set_elements(dann_index* idx, uint32_t first_slot, uint32_t n, const void* rows, uint64_t len);
int32_t dann_get_element(const dann_index* idx, uint32_t slot, void* bytes, uint64_t len);
/* the same from DEVICE memory on the index's device: n rows, `src_stride` bytes apart (>= layer bytes), copied device to
 * device -- a data set that is produced or already resident on the GPU never crosses PCIe */
int32_t dann_set_elements_device(dann_index* idx, uint32_t first_slot, uint32_t n, const void* d_rows, uint64_t src_stride);
/* read-only views of the index's device buffers for zero-copy interop (rows: (capacity + start points) x row_stride bytes;
 * adjacency: the Neighbors layout, (capacity + start points) x (max_degree + 1) u32).  Valid until the index is
 * destroyed; contents change under mutations. */
int32_t dann_index_device_pointers(const dann_index* idx, const void** d_rows, const uint32_t** d_adjacency);
/* upload a whole diskann-inmem Store buffer verbatim (rows at `stride`; with dann_config::inline_tags the tag
 * byte after each payload is uploaded too and decides readability, otherwise tag bytes are ignored) */
int32_t dann_upload_store(dann_index* idx, const void* base, uint64_t stride, uint32_t nrows);
/* inline concurrency tags of slots [first_slot, first_slot + n) (inline_tags indexes only; tag.rs:86-133:
 * 0 AVAILABLE, 1 OWNED, 2 RETIRING, 254 PUBLISHED, 255 FROZEN; readable iff >= 254).  The host keeps the
 * reference's mirror of the tags (store.rs:150) for the fine-grained dann_expand_beam seam. */
int32_t dann_set_tags(dann_index* idx, uint32_t first_slot, uint32_t n, const uint8_t* tags);
int32_t dann_get_tags(const dann_index* idx, uint32_t first_slot, uint32_t n, uint8_t* tags);

/* ---- external ids: IdMap / Translate post-processing (diskann-inmem/src/ids.rs:18-107, provider.rs:899-950).
 * Search results are slot ids; these helpers keep the slot -> external id table and translate result
 * buffers (start points and unmapped slots have no external id: to_external reports them as
 * 0xFFFFFFFFFFFFFFFF, exactly the entries Translate drops). */
int32_t dann_set_external_ids(dann_index* idx, uint32_t first_slot, uint32_t n, const uint64_t* ext_ids);
int32_t dann_to_external(const dann_index* idx, const uint32_t* slot_ids, uint64_t n, uint64_t* out_ext);

/* ---- adjacency: NeighborAccessor(Mut) (provider.rs:768-823, neighbors.rs:124-224) -- */
int32_t dann_get_neighbors(const dann_index* idx, uint32_t slot, uint32_t* out, uint32_t cap, uint32_t* out_len);
int32_t dann_set_neighbors(dann_index* idx, uint32_t slot, const uint32_t* ids, uint32_t n);
/* append with the reference's clamp-on-overflow (provider.rs:804-816) */
int32_t dann_append_neighbors(dann_index* idx, uint32_t slot, const uint32_t* ids, uint32_t n);
/* set_neighbors_bulk: lists[i] = [len, ids...] rows of (max_degree+1) u32 */
int32_t dann_set_neighbors_bulk(dann_index* idx, const uint32_t* slots, uint32_t n, const uint32_t* lists);
/* whole Neighbors buffer, (capacity+num_start_points) x (max_degree+1) u32 (neighbors.rs:60-101) */
int32_t dann_upload_graph(dann_index* idx, const uint32_t* adj, uint64_t nrows);
int32_t dann_download_graph(const dann_index* idx, uint32_t* adj, uint64_t nrows);

/* ---- distances (parity seam) ----------------------------------------------------- */
/* layers::Distance::evaluate (full.rs:224-242): two raw rows, T x T kernel */
int32_t dann_distance(const dann_index* idx, const void* x, uint64_t xlen, const void* y, uint64_t ylen,
                      float* out);
/* the same between stored rows, n pairs in one launch (RobustPrune's primitive, prune.rs:212-215) */
int32_t dann_distance_pairs(const dann_index* idx, const uint32_t* a, const uint32_t* b, uint32_t n, float* out);
/* Search::query_distance + QueryDistance::evaluate (full.rs:165-171, 317-336) */
int32_t dann_query_create(const dann_index* idx, const void* query, uint64_t len, dann_query** out);
int32_t dann_query_destroy(dann_query* q);
int32_t dann_query_distance(const dann_query* q, const void* row, uint64_t len, float* out);
/* ExpandBeam::expand_beam (provider.rs:492-497, 620-690): pre-filtered ids -> (id, dist) */
int32_t dann_expand_beam(const dann_query* q, const uint32_t* ids, uint32_t n, uint32_t* out_ids,
                         float* out_dists, uint32_t* out_n);
/* batched form: nq queries, ragged id lists (offsets has nq+1 entries); out_dists is
 * aligned with `ids` */
int32_t dann_expand_beam_batch(const dann_index* idx, const void* queries, uint32_t nq, const uint32_t* ids,
                               const uint64_t* offsets, float* out_dists);

/* ---- search: DiskANNIndex::search(Knn{l_value, beam_width}) for nq independent queries
 * (index.rs:1933-2000,2029-2065; knn_search.rs:155-193; provider.rs:408-480,899-950).
 * out_ids/out_dists: nq x k (unwritten entries 0xFFFFFFFF / +inf); ids are slot ids. ---- */
int32_t dann_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t l_value,
                          uint32_t beam_width, uint32_t k, uint32_t* out_ids, float* out_dists,
                          dann_search_stats* out_stats);
/* device-resident form: every pointer is a device pointer on the index's device; the
 * launch is enqueued on the index stream and the call returns after it completes. */
int32_t dann_search_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, uint32_t l_value,
                                 uint32_t beam_width, uint32_t k, uint32_t* d_out_ids, float* d_out_dists,
                                 dann_search_stats* d_out_stats);
/* graph::search::Range for nq queries (diskann/src/graph/search/range_search.rs:51-470): Knn-style
 * search with L = starting_l, then -- if at least starting_l * initial_slack of that list lies within
 * `radius` and fewer than max_returned -- breadth-first expansion of every point within
 * radius * range_slack.  Results (slot ids, start points dropped, `inner_radius < d <= radius`) go to
 * out_ids/out_dists (nq x out_cap, unwritten = 0xFFFFFFFF / +inf).  max_returned == 0: unlimited
 * (the GPU scratch list is then sized min(4 * out_cap + 1024, capacity + starts) per query; a longer list is
 * DANN_EOVERFLOW).  A query with more results than out_cap is DANN_EOVERFLOW too: the reference's output is unbounded,
 * and a silently shortened list cannot be told from a complete one.  After DANN_EOVERFLOW the outputs are unspecified
 * (out_stats[q].status names the queries); the same call with a larger out_cap succeeds.
 * Stats follow the reference's accounting (cmps of the first phase only, hops = initial + cumulative,
 * :308-314); out_second_round[q] = range_search_second_round.  Parameter errors == RangeSearchError. */
int32_t dann_range_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t starting_l,
                                uint32_t beam_width, float radius, int32_t has_inner_radius, float inner_radius,
                                float initial_slack, float range_slack, uint32_t max_returned, uint32_t out_cap,
                                uint32_t* out_ids, float* out_dists, dann_search_stats* out_stats,
                                uint32_t* out_second_round);
/* ---- filtered searches (diskann/src/graph/ext/labeled.rs: a SearchAccessor wrapped with a QueryLabelProvider).
 * The label provider crosses the boundary as a bitmap over slot ids: is_match(i) = bit (i & 31) of bits[i >> 5]
 * for i in [0, capacity + num_start_points) -- start points are classified too (labeled.rs:166-175). */
enum { DANN_FILTER_INLINE = 1, DANN_FILTER_MULTIHOP = 2 };
typedef struct {
    uint32_t mode;              /* DANN_FILTER_INLINE: InlineFilterSearch (search/inline_filter_search.rs:69-301);
                                   DANN_FILTER_MULTIHOP: MultihopFilterSearch (search/multihop_filter_search.rs:46-244) */
    const uint32_t* bits;       /* host memory */
    uint64_t stride_words;      /* words between the bitmaps of consecutive queries; 0 = one bitmap for all queries */
    uint32_t adaptive_samples;  /* inline only: AdaptiveL::sample_count, 0 = no AdaptiveL (:40-62) */
    double adaptive_scale;      /* AdaptiveL::scale_factor, must be >= 1.0 */
    uint32_t matched_cap;       /* inline only: capacity of the per-query matched list (every accepted id that was
                                   compared); 0 = min(capacity + starts, 8192). Exceeding it is DANN_EOVERFLOW. */
} dann_filter;
/* index.search(InlineFilterSearch | MultihopFilterSearch, Filtered<Strategy>, ..) for nq queries; outputs as
 * dann_search_batch.  Stats follow the reference: start points are not counted in cmps.  Ties: the reference sorts
 * matched results / rejected candidates with sort_unstable_by(distance); equal distances keep arrival order here. */
int32_t dann_filtered_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t l_value,
                                   uint32_t beam_width, uint32_t k, const dann_filter* filter, uint32_t* out_ids,
                                   float* out_dists, dann_search_stats* out_stats);
/* index.search(FilteredRange, ..) (search/filtered_range_search.rs:111-330); parameters and outputs as
 * dann_range_search_batch, filter->mode must be DANN_FILTER_INLINE, AdaptiveL is not used (:148-156).
 * cmps / hops accumulate over both rounds.  DANN_EOVERFLOW as dann_range_search_batch: a query with more results than
 * out_cap (the reference's output is unbounded, and a silently shortened list cannot be told from a complete one), more
 * matched ids in the first round than filter->matched_cap, or a list of matched ids within the radius longer than
 * max(max_returned ? max_returned : 4 * out_cap + 1024, matched_cap), at most capacity + starts. */
int32_t dann_filtered_range_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t starting_l,
                                         uint32_t beam_width, float radius, int32_t has_inner_radius,
                                         float inner_radius, float initial_slack, float range_slack,
                                         uint32_t max_returned, uint32_t out_cap, const dann_filter* filter,
                                         uint32_t* out_ids, float* out_dists, dann_search_stats* out_stats,
                                         uint32_t* out_second_round);

/* ---- paged search: DiskANNIndex::paged_search + PagedSearch::next_page (diskann/src/graph/index.rs:2075-2155,
 * diskann/src/graph/search/paged.rs:53-149) for nq queries at once.  The session owns the reference's per-search
 * scratch on the device: the auto-resizable candidate list (nothing is ever dropped, queue.rs:95-121), the visited
 * set and the tail of the last computed page.  list_cap bounds the list per query (0 = min(capacity + starts,
 * max(16384, 64 * l_value)), never below 64 or above capacity + starts); a query whose list would outgrow it makes
 * dann_paged_next return DANN_EOVERFLOW, from that call on (the session is over; open another with a larger list_cap --
 * the index is untouched).  next_page: k results per query (k <= l_value, errors
 * as paged.rs:57-64), out_ids/out_dists nq x k (unwritten 0xFFFFFFFF / +inf), out_counts[q] = results of the page
 * (0 = exhausted).  Pages never overlap; within a page distances are non-decreasing.  Not for DANN_PQ. */
typedef struct dann_paged dann_paged;
int32_t dann_paged_begin(dann_index* idx, const void* queries, uint32_t nq, uint32_t l_value, uint32_t list_cap,
                         dann_paged** out);
int32_t dann_paged_next(dann_paged* session, uint32_t k, uint32_t* out_ids, float* out_dists, uint32_t* out_counts);
int32_t dann_paged_end(dann_paged* session);

/* Rerank post-processor (diskann-providers/src/model/graph/provider/async_/inmem/full_precision.rs:348-397):
 * full-precision distances query x stored row for every candidate id of a quantised search, sorted
 * ascending (equal distances keep candidate order; the reference's sort is unstable), first k returned.
 * `idx` is the full-precision index; cand_ids: nq x cand_stride, entries equal to 0xFFFFFFFF are skipped. */
int32_t dann_rerank_batch(dann_index* idx, const void* queries, uint32_t nq, const uint32_t* cand_ids,
                          uint32_t cand_stride, uint32_t k, uint32_t* out_ids, float* out_dists);
/* device-pointer form (queries, cand_ids, outputs on the index's device) */
int32_t dann_rerank_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, const uint32_t* d_cand_ids,
                                 uint32_t cand_stride, uint32_t k, uint32_t* d_out_ids, float* d_out_dists);
/* Exhaustive (flat) k-NN: diskann::flat::FlatIndex::knn_search (diskann/src/flat/index.rs:57-99) for nq queries over
 * the slots [first_slot, first_slot + n), every row scored with the index's own distance (any row type but DANN_PQ, for
 * which DANN_EUNSUPPORTED; the queries are images of dann_query_bytes() bytes in the current query layout).  The
 * reference streams the elements in ascending id order through NeighborPriorityQueue::insert on a queue of capacity k
 * (diskann/src/neighbor/queue.rs:130-171): a NaN distance is dropped; a candidate is dropped only when the queue is full
 * and its last distance is smaller; otherwise it goes in at the first entry whose distance is >= its own, the last entry
 * leaving a full queue.  The result is therefore the first k non-NaN elements under the strict total order
 *     (distance ascending, with -0.0 == +0.0; scan position descending),
 * listed in that order: among equal distances the slot scanned later comes first, and wins the k-th place.
 * The caller names the populated range (start-point slots may be part of it).  On an inline_tags index a slot whose
 * tag is below Tag::PUBLISHED is skipped and not counted, as in the searches; with DANN_FLAT_SKIP_DELETED so is a slot
 * marked by dann_delete_points (without the flag the deleted state is not consulted).
 * out_ids / out_dists: nq x k, the places behind the last result hold 0xFFFFFFFF / +infinity.  out_stats (optional): cmps =
 * rows evaluated (those with a NaN distance included), hops = 0, result_count = written = min(k, rows inserted) -- the
 * Translate post-processor's k - 1 is not part of this path.
 * Errors: DANN_EINVAL for k == 0, a null pointer with nq > 0 or an unknown flag bit; DANN_EBOUNDS when the range
 * leaves [0, capacity + num_start_points); DANN_EUNSUPPORTED for k > 1024.  nq == 0 writes nothing; with n == 0 every
 * result is empty. */
enum { DANN_FLAT_SKIP_DELETED = 1 };
int32_t dann_flat_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                               uint32_t k, uint32_t flags, uint32_t* out_ids, float* out_dists,
                               dann_search_stats* out_stats);
/* device-pointer form (queries and outputs on the index's device; complete on return) */
int32_t dann_flat_search_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                                      uint32_t k, uint32_t flags, uint32_t* d_out_ids, float* d_out_dists,
                                      dann_search_stats* d_out_stats);
/* Exhaustive scans that tell whether a filtered or a range search is right: the reference's ground-truth tools
 * (diskann-tools/src/utils/ground_truth.rs) over the slots [first_slot, first_slot + n), with the distances, row types,
 * query images, flags and range rules of dann_flat_search_batch.
 * The filter is a bitmap over slot ids as dann_filter defines it -- is_match(i) = bit (i & 31) of bits[i >> 5] for i in
 * [0, capacity + num_start_points) -- one for all queries (stride_words == 0) or one per query, stride_words words apart
 * (a non-zero stride below ceil((capacity + num_start_points) / 32) is DANN_EINVAL).  A null filter or null bits: every
 * slot matches.  Bits at or beyond capacity + num_start_points in the last word are ignored.
 * A row is evaluated for query q iff it lies in the range, its tag is readable (inline_tags), it is not marked deleted
 * (DANN_FLAT_SKIP_DELETED) and q's filter holds its slot; out_stats[q].cmps counts those rows, hops is 0.  A row that no
 * query of a tile of queries accepts is not fetched at all.
 *
 * dann_flat_filtered_search_batch: compute_ground_truth_from_data with query_bitmaps (:589-693).  The queue of
 * FlatIndex::knn_search is fed the evaluated rows only, in ascending slot order; outputs, padding and stats as
 * dann_flat_search_batch, to which a call with an all-ones filter is equal in every output.
 *
 * dann_flat_range_search_batch: compute_range_ground_truth_from_data (:285-353).  The result of a query is every evaluated
 * row whose distance d passes the predicate of range_search.rs:326-335 -- d <= radius, and !(d <= inner_radius) when
 * has_inner_radius -- in ascending slot order, with the distance as computed (a NaN distance fails; -0.0 stays -0.0).
 * out_counts[q] is always the true number of matches; out_ids / out_dists (nq x out_cap) take the first out_cap of them,
 * 0xFFFFFFFF / +infinity behind.  out_stats (optional): result_count = the true count, written = min(count, out_cap).
 * If a count exceeds out_cap the call returns DANN_EOVERFLOW and out_stats[q].status is non-zero for those queries; the
 * counts and every other query's results are valid, and a second call with out_cap = max(out_counts) holds everything.
 * out_cap == 0 only counts: out_ids / out_dists may be NULL, the call returns DANN_OK.
 * Errors as dann_flat_search_batch; also DANN_EINVAL for a NaN radius or inner_radius > radius.
 * The results do not depend on how the scan is cut up, nor on the run. */
typedef struct {
    const uint32_t* bits;   /* host memory; device memory in the _device forms */
    uint64_t stride_words;  /* words between the bitmaps of consecutive queries; 0 = one bitmap for all queries */
} dann_flat_filter;
int32_t dann_flat_filtered_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                                        uint32_t k, uint32_t flags, const dann_flat_filter* filter, uint32_t* out_ids,
                                        float* out_dists, dann_search_stats* out_stats);
int32_t dann_flat_range_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                                     float radius, int32_t has_inner_radius, float inner_radius, uint32_t flags,
                                     const dann_flat_filter* filter, uint32_t out_cap, uint32_t* out_ids, float* out_dists,
                                     uint32_t* out_counts, dann_search_stats* out_stats);
/* device-pointer forms (queries, bitmaps and outputs on the index's device, the dann_flat_filter itself in host memory;
 * complete on return) */
int32_t dann_flat_filtered_search_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, uint32_t first_slot,
                                               uint32_t n, uint32_t k, uint32_t flags, const dann_flat_filter* d_filter,
                                               uint32_t* d_out_ids, float* d_out_dists, dann_search_stats* d_out_stats);
int32_t dann_flat_range_search_batch_device(dann_index* idx, const void* d_queries, uint32_t nq, uint32_t first_slot,
                                            uint32_t n, float radius, int32_t has_inner_radius, float inner_radius,
                                            uint32_t flags, const dann_flat_filter* d_filter, uint32_t out_cap,
                                            uint32_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                            dann_search_stats* d_out_stats);
/* Exhaustive k-NN over PQ code rows: the reference's product-exhaustive-search (diskann-benchmark/src/exhaustive/
 * product.rs; algos::linear_search, exhaustive/algos.rs:42-99) for nq queries over the slots [first_slot, first_slot + n)
 * of a DANN_PQ index with its table attached (dann_set_pq_table).  The queries are f32 vectors of dann_query_bytes()
 * bytes, already centred or rotated by the caller, as for the searches.
 * Distance: per query the lookup table table[c][b] = populate_chunk_distances_impl (fixed_chunk_pq_table.rs:152-192) for
 * the index's metric (L2, or the inner product, negated), and d(q, slot) = ((+0.0 + table[0][code[0]]) + table[1][code[1]])
 * + ... in f32, in chunk order (pq_dist_lookup_single, :82-100): bit for bit what the searches over a DANN_PQ index and
 * dann_pq_build_lut + dann_pq_scan produce.  The sum is never -0.0.
 * Selection: linear_search feeds every code row in ascending id order to NeighborPriorityQueue::insert on a queue of k
 * entries (diskann/src/neighbor/queue.rs:130-171), the rule of dann_flat_search_batch: the result is the first k non-NaN
 * rows under the strict total order (distance ascending, scan position descending), listed in that order.  Duplicate
 * code rows tie exactly: the slot scanned later comes first, and wins the k-th place.
 * Skipped rows: on an inline_tags index a slot whose tag is below Tag::PUBLISHED is skipped and not counted; with
 * DANN_FLAT_SKIP_DELETED so is a slot marked by dann_delete_points.  filter (optional) has the meaning it has in
 * dann_flat_filtered_search_batch -- a shared or per-query bitmap over slot ids, NULL or null bits = every slot; a
 * non-zero stride below ceil((capacity + num_start_points) / 32) is DANN_EINVAL -- and a query evaluates only the slots its
 * bitmap holds.  A call with an all-ones filter is equal to one without in every output.
 * out_ids / out_dists: nq x k, the places behind the last result hold 0xFFFFFFFF / +infinity (linear_search pads with
 * u32::MAX).  out_stats (optional): cmps = rows evaluated and accepted for the query (those with a NaN distance included),
 * hops = 0, result_count = written = min(k, rows inserted).
 * Errors: DANN_EUNSUPPORTED for an index that is not DANN_PQ or for k > 1024; DANN_EINVAL for an index without a pivot
 * table, k == 0, a null pointer with nq > 0, an unknown flag bit or a short filter stride; DANN_EBOUNDS when the range
 * leaves [0, capacity + num_start_points).  nq == 0 writes nothing; with n == 0 every result is empty.  Every chunk count
 * an index accepts is served.  The results do not depend on how the scan is cut up, nor on the run. */
int32_t dann_pq_linear_search_batch(dann_index* idx, const float* queries, uint32_t nq, uint32_t first_slot, uint32_t n,
                                    uint32_t k, uint32_t flags, const dann_flat_filter* filter, uint32_t* out_ids,
                                    float* out_dists, dann_search_stats* out_stats);
/* device-pointer form (queries, bitmaps and outputs on the index's device, the dann_flat_filter itself in host memory;
 * complete on return) */
int32_t dann_pq_linear_search_batch_device(dann_index* idx, const float* d_queries, uint32_t nq, uint32_t first_slot,
                                           uint32_t n, uint32_t k, uint32_t flags, const dann_flat_filter* d_filter,
                                           uint32_t* d_out_ids, float* d_out_dists, dann_search_stats* d_out_stats);
/* insert-time search: also returns the VisitedSearchRecord (record.rs:86-93) per query:
 * rec_ids/rec_dists: nq x rec_stride, rec_n: nq */
int32_t dann_search_record_batch(dann_index* idx, const uint32_t* slots, uint32_t nq, uint32_t l_value,
                                 uint32_t* rec_ids, float* rec_dists, uint32_t rec_stride, uint32_t* rec_n,
                                 dann_search_stats* out_stats);

/* the same for external queries (host pointer, layer bytes each): the VisitedSearchRecord of an ordinary Knn search
 * with beam width 1 -- every node the search expanded, in expansion order.  Diagnostics / replay checks. */
int32_t dann_search_record_queries(dann_index* idx, const void* queries, uint32_t nq, uint32_t l_value, uint32_t* rec_ids,
                                   float* rec_dists, uint32_t rec_stride, uint32_t* rec_n, dann_search_stats* out_stats);

/* ---- build ------------------------------------------------------------------------ */
/* occlude_list / robust_prune over caller pools (index.rs:2565-2650, prune.rs:106-259):
 * pool i = pool_ids/pool_dists[offsets[i] .. offsets[i+1]) for location locs[i];
 * out_adj: n rows of (pruned_degree+1) u32 [len, ids...] */
int32_t dann_prune_batch(dann_index* idx, const dann_build_config* cfg, const uint32_t* locs, uint32_t n,
                         const uint32_t* pool_ids, const float* pool_dists, const uint64_t* offsets,
                         int32_t force_saturate, uint32_t* out_adj);
/* DiskANNIndex::multi_insert (index.rs:815-1030) for rows already stored at `slots` */
int32_t dann_insert_batch(dann_index* idx, const dann_build_config* cfg, const uint32_t* slots, uint32_t n);
/* DiskANNIndex::insert (diskann/src/graph/index.rs:226-341) for a row already stored at `slot`: insert search (beam 1,
 * L = l_build), RobustPrune of the visited record, set_neighbors, then add_edge_and_prune towards the first
 * cfg->max_backedges of the new neighbours (:324-327; 0 = pruned_degree, the reference's default; more than
 * pruned_degree is DANN_EINVAL as in config/mod.rs:308-311).  With the default it equals dann_insert_batch of one
 * point; multi_insert itself sends back-edges to every new neighbour (index.rs:123-143). */
int32_t dann_insert(dann_index* idx, const dann_build_config* cfg, uint32_t slot);
/* multi-GPU build (replicated index, batch partitioned across ranks): multi_insert split at its
 * only exchange point.  Phase 1 = candidate generation (search + RobustPrune, index.rs:349-434) for the
 * batch positions [lo, hi), reading the graph only; phase 2 = graph update (index.rs:911-1024) from the
 * pending rows of the whole batch.  d_pending_* are DEVICE pointers, rows of (pruned_degree + 1) u32
 * [len, ids...] in batch order, i.e. directly usable as RCCL all-gather buffers.  Running phase 1 over
 * [0, n) and then phase 2 equals dann_insert_batch. */
int32_t dann_insert_batch_candidates(dann_index* idx, const dann_build_config* cfg, const uint32_t* slots, uint32_t n,
                                     uint32_t lo, uint32_t hi, uint32_t* d_pending_out);
int32_t dann_insert_batch_commit(dann_index* idx, const dann_build_config* cfg, const uint32_t* slots, uint32_t n,
                                 const uint32_t* d_pending_all);
/* phase 2 with the expensive part partitioned (multi-GPU build): every replica applies the new rows and the
 * back-edges whose target list still fits; a target whose list must be pruned (robust_prune of add_edge_and_prune,
 * index.rs:2264-2341) is handled only by the rank that owns it (id % world == rank).  The rows rewritten by this rank
 * are exported to d_rows_out (DEVICE, rows of max_degree + 2 u32: [target id, len, ids...], at most rows_cap of
 * them, *count_out on return) -- all-gather them and hand the other ranks' rows to dann_apply_neighbor_rows_device;
 * after that every replica equals the result of dann_insert_batch_commit.  world = 1 is dann_insert_batch_commit. */
int32_t dann_insert_batch_commit_part(dann_index* idx, const dann_build_config* cfg, const uint32_t* slots, uint32_t n,
                                      const uint32_t* d_pending_all, uint32_t rank, uint32_t world,
                                      uint32_t* d_rows_out, uint32_t rows_cap, uint32_t* count_out);
int32_t dann_apply_neighbor_rows_device(dann_index* idx, const uint32_t* d_rows, uint32_t count);
/* insert every slot in [first, first+n) in id order with a geometric batch schedule
 * (batch = clamp(ceil(inserted * growth), 1, max_batch)); returns the number of batches */
int32_t dann_build(dann_index* idx, const dann_build_config* cfg, uint32_t first, uint32_t n, float growth,
                   uint32_t max_batch);

/* ---- product quantisation: lookup-table build + scan -------------------------------------
 * FixedChunkPQTable::populate_chunk_distances_impl (L2 / inner product) and pq_dist_lookup_single
 * (diskann-providers/src/model/pq/fixed_chunk_pq_table.rs:152-192, 82-100), batched:
 *   pivots: 256 x dim f32 row-major (:105-128), chunk_offsets: nchunks+1 (usize -> u32),
 *   queries: nq x dim f32 (already centred/rotated by the caller), lut: nq x nchunks x 256 f32.
 * metric: DANN_L2 or DANN_INNER_PRODUCT.  Host pointers. */
int32_t dann_pq_build_lut(int32_t device, int32_t metric, const float* pivots, const uint32_t* chunk_offsets,
                          uint32_t nchunks, uint32_t dim, const float* queries, uint32_t nq, float* lut);
/* scan: out[q][i] = sum over chunks, in chunk order, of lut[q][c][codes[ids[q][i]][c]];
 * codes: npoints x nchunks u8; ids: ragged lists (offsets has nq+1 entries), out aligned with ids */
int32_t dann_pq_scan(int32_t device, const float* lut, uint32_t nq, uint32_t nchunks, const uint8_t* codes,
                     uint64_t npoints, const uint32_t* ids, const uint64_t* offsets, float* out);

/* TransposedTable::compress_into for a batch (diskann-quantization/src/product/tables/transposed/table.rs:382-403,
 * 465-530; Chunk::find_closest, pivots.rs:253-345): codes[r][c] = index of the pivot of chunk c closest (L2) to
 * row r's chunk, with the reference's arithmetic (|p|^2 - 2 x.p, fma chain in dimension order) and its lane-wise
 * tie rule.  pivots: ncenters (<= 256) x dim f32; rows: n x dim f32; codes: n x nchunks u8.  Host pointers.
 * DANN_EINVAL when a chunk is infinitely far from / NaN against every pivot (InfinityOrNaN). */
int32_t dann_pq_compress(int32_t device, const float* pivots, uint32_t ncenters, const uint32_t* chunk_offsets,
                         uint32_t nchunks, uint32_t dim, const float* rows, uint64_t n, uint8_t* codes);

/* PQ training minus the seeding: the Lloyd iterations of LightPQTrainingParameters::train
 * (diskann-quantization/src/product/train.rs:96-226 -> algorithms/kmeans/lloyds.rs:23-438) for every chunk, with the
 * reference's arithmetic (assignment scores ((n_c - ip) - ip) + |x|^2, first strictly smaller centre; f64 centroid
 * sums in row order; empty clusters become the zero vector).  `centers` (ncenters x dim f32) carries the initial
 * centres in -- k-means++ (kmeans/plusplus.rs, seeded per chunk from rand's StdRng) stays with the caller -- and the
 * trained pivots out.  data: n x dim f32.  Optional outputs: assignments nchunks x n (those of the last assignment
 * step, as lloyds_inner returns them), residuals nchunks.  Host pointers. */
int32_t dann_pq_lloyds(int32_t device, const float* data, uint64_t n, uint32_t dim, const uint32_t* chunk_offsets,
                       uint32_t nchunks, uint32_t ncenters, float* centers, uint32_t max_reps, uint32_t* assignments,
                       float* residuals);

/* the caller's random generator for the two draws of k-means++: on the Rust side closures over the
 * `rng_builder.build_boxed_rng(chunk)` generators of LightPQTrainingParameters::train (train.rs:164-165,
 * diskann-quantization/src/random.rs:33-44), so that the GPU consumes exactly the reference's stream:
 *   uniform_index(ctx, chunk, n)   == Uniform::new(0, n).unwrap().sample(rng_chunk)              (plusplus.rs:417)
 *   uniform_f64(ctx, chunk, high)  == Uniform::<f64>::new(0.0, high).unwrap().sample(rng_chunk)  (plusplus.rs:440-444)
 * Called from the calling thread only.  Draws of different chunks are interleaved (centre by centre across the
 * chunks); within one chunk they come in the reference's order -- which is all a per-chunk generator can observe. */
typedef struct {
    void* ctx;
    uint64_t (*uniform_index)(void* ctx, uint32_t chunk, uint64_t n);
    double (*uniform_f64)(void* ctx, uint32_t chunk, double high);
} dann_rng;
/* kmeans::plusplus::kmeans_plusplus_into_inner (algorithms/kmeans/plusplus.rs:366-497) for every chunk.  centers:
 * ncenters x dim out (the chunk columns of centres that could not be selected stay zero); selected: nchunks out or NULL
 * (fewer than ncenters = the reference's recoverable DatasetTooSmall / InsufficientDiversity).  DANN_EINVAL when a
 * non-finite distance total appears (SawInfinity). */
int32_t dann_pq_kmeanspp(int32_t device, const float* data, uint64_t n, uint32_t dim, const uint32_t* chunk_offsets,
                         uint32_t nchunks, uint32_t ncenters, const dann_rng* rng, float* centers, uint32_t* selected);
/* LightPQTrainingParameters::train (product/train.rs:96-226): dann_pq_kmeanspp + dann_pq_lloyds; pivots: ncenters x dim */
int32_t dann_pq_train(int32_t device, const float* data, uint64_t n, uint32_t dim, const uint32_t* chunk_offsets,
                      uint32_t nchunks, uint32_t ncenters, uint32_t lloyds_reps, const dann_rng* rng, float* pivots);

/* ---- on-disk formats of the reference (so a GPU-built index loads in the reference and vice versa)
 * graph: diskann-providers/src/storage/bin.rs:234-380 -- 24-byte header {u64 file_size, u32 max_degree,
 *        u32 start_point, u64 num_start_points} then per node {u32 len, len x u32}, nodes in slot order
 *        (dynamic slots, then the frozen start points).
 * vectors: diskann-utils/src/io.rs:24 `.bin` -- {u32 npts, u32 dim} then row-major payload. */
int32_t dann_save_graph(const dann_index* idx, const char* path);
/* loads adjacency for min(file points, index slots) nodes; out_* may be NULL */
int32_t dann_load_graph(dann_index* idx, const char* path, uint32_t* out_start, uint64_t* out_num_start,
                        uint64_t* out_num_points);
int32_t dann_save_vectors_bin(const dann_index* idx, const char* path, uint32_t first_slot, uint32_t n);
int32_t dann_load_vectors_bin(dann_index* idx, const char* path, uint32_t first_slot, uint32_t* out_n);

/* attach the PQ schema of a DANN_PQ index: pivots 256 x dim f32 row-major, chunk_offsets pq_chunks + 1
 * (FixedChunkPQTable::new, fixed_chunk_pq_table.rs:105-140) */
int32_t dann_set_pq_table(dann_index* idx, const float* pivots, const uint32_t* chunk_offsets);
/* Spherical indexes: the layout of the queries that every entry point taking `queries`, `query` or `d_queries` reads
 * (dann_query_bytes() each).  Read on every call; a dann_query keeps the layout it was created under.  Whatever uses a
 * stored row as the query -- build and insert searches, dann_search_record_batch, prunes, dann_distance_pairs,
 * consolidation, in-place deletes -- is always the symmetric row x row form.  A layout the row width does not have:
 * DANN_EUNSUPPORTED (UnsupportedQueryLayout); while the search server runs: DANN_EBUSY; any other index accepts only
 * DANN_QUERY_SAME_AS_DATA. */
int32_t dann_set_query_layout(dann_index* idx, int32_t layout);
int32_t dann_get_query_layout(const dann_index* idx);
/* bytes of one query under the current layout (every row type: f32 vectors for DANN_PQ, else the row's payload) */
int32_t dann_query_bytes(const dann_index* idx);
/* MinMax indexes: the dtype of the query images that every entry point taking `queries`, `query` or `d_queries` reads.
 * Default: the index's own.  On a DANN_MM4 / MM2 / MM1 index DANN_MM8 is also allowed (MinMaxQuery::EightBit: the query
 * is compressed to a Data<8> image and scored through the heterogeneous kernel::<8, M>, minmax/vectors.rs:206-229, x the
 * query and y the row): dann_query_bytes() is then 20 + dim and the queries are front-canonical MM8 images, the bytes
 * dann_minmax_compress writes at 8 bits.  Distances stay bit for bit the reference's: the raw product is an exact u32,
 * so dim * 255 * (2^bits - 1) must fit one (else DANN_EINVAL).  Served by the Knn, range, filtered, filtered-range,
 * paged, diverse, rerank, expand-beam, dann_query_* and flat entry points, the host-pointer forms included; the search
 * server as for every row type where the query is a multiple of 16 bytes.  Read on every call; a dann_query keeps the
 * dtype it was created under.  Whatever uses a stored row as the query (see dann_set_query_layout) stays row x row.
 * Setting the index's own dtype is accepted on every index; any other pair of MinMax dtypes is DANN_EUNSUPPORTED, any
 * other dtype DANN_EINVAL; while the search server runs: DANN_EBUSY.  The replicas of a dann_multi are set one by one. */
int32_t dann_set_query_dtype(dann_index* idx, int32_t dtype);
int32_t dann_get_query_dtype(const dann_index* idx, int32_t* out);
/* Optional GPU-private search layout of a DANN_PQ index (at most 64 chunks, no inline tags): for every slot one
 * 64-byte-aligned row holding its adjacency list AND the code rows of its neighbours, so that a hop of the beam search
 * (expand_beam over PQ rows: diskann-providers/src/model/pq/fixed_chunk_pq_table.rs:82-100 per neighbour) is one
 * contiguous read instead of one adjacency row plus one code-row gather per neighbour.  Built from the index's current
 * rows and adjacency; costs (capacity + start points) x round_up(16-rounded 4 (R + 1) + C R, 64) bytes of device
 * memory, C = the chunk count rounded up to 16.  Search results never depend on it.  Any later mutation of the index (rows, adjacency, build, load) drops
 * the layout -- searches fall back to the plain rows -- until this is called again.  DANN_EUNSUPPORTED for other
 * indexes. */
int32_t dann_pq_pack_neighbors(dann_index* idx);

/* ScalarQuantizationParameters::train (diskann-quantization/src/scalar/train.rs:33-52): shift[d] = mean_d - p,
 * scale = 2p with p = standard_deviations * sqrt(max_d variance_d) (f64 statistics in row order, utils.rs:109-199);
 * mean_norm (optional) = mean L2 norm of the rows.  data: n x dim f32, host pointers.  The reference's default is
 * standard_deviations = 2. */
int32_t dann_sq8_train(int32_t device, const float* data, uint64_t n, uint32_t dim, double standard_deviations,
                       float* shift, float* scale, float* mean_norm);

/* ---- scalar quantisation: ScalarQuantizer::compress_into for 8 bits
 * (diskann-quantization/src/scalar/quantizer.rs:189-236, 395-430): code = round(clamp((x - shift) *
 * 255/scale, 0, 255)), compensation = scale/255 * sum(code * shift).  x: n x dim f32, shift: dim f32,
 * out: n rows of dim + 4 bytes.  Host pointers. */
int32_t dann_sq8_compress(int32_t device, const float* x, uint32_t n, uint32_t dim, const float* shift, float scale,
                          void* out);
/* ScalarQuantizer::compress_into::<bits> for bits in {1, 4, 8} (anything else: DANN_EINVAL): code =
 * round(clamp((x - shift) * (2^bits - 1)/scale, 0, 2^bits - 1)) (half away from zero, NaN -> 0), compensation =
 * scale/(2^bits - 1) * sum(code * shift).  out: n rows of ceil(dim * bits / 8) + 4 bytes, codes packed as DANN_SQ1 /
 * DANN_SQ4 rows, padding bits zero; bits = 8 is dann_sq8_compress byte for byte.  dann_sq8_train serves every width
 * (the trained scale and shift do not depend on it, quantizer.rs:187-189).  Host pointers. */
int32_t dann_sq_compress(int32_t device, int32_t bits, const float* x, uint32_t n, uint32_t dim, const float* shift,
                         float scale, void* out);
/* MinMaxQuantizer::compress_into::<bits> (minmax/quantizer.rs:117-228) for vectors that have already been through the
 * quantiser's transform (the host keeps the Transform; NullTransform = the data itself).  bits in {1, 2, 4, 8}.
 * out: n row images of dann_layer_bytes(48 + bits, dim), padding bits zero; out_loss (optional, n): L2Loss::as_f32.
 * A NaN in row i: DANN_EINVAL (InputContainsNaN), outputs unspecified.  Host pointers. */
int32_t dann_minmax_compress(int32_t device, int32_t bits, const float* x, uint32_t n, uint32_t dim, float grid_scale,
                             void* out, float* out_loss);
/* ComputeMedoid (diskann-utils/src/sampling/medoid.rs:15-156), the start point of StartPointStrategy::Medoid: the row
 * nearest to the mean of the rows.  dtype: DANN_F32, DANN_F16, DANN_U8 or DANN_I8 (anything else: DANN_EUNSUPPORTED).
 * Rows lie row_stride_bytes apart (0 = packed, dim * sizeof(T); less than that, or a stride / address that is not a
 * multiple of sizeof(T): DANN_EINVAL), so an index's own store can be passed (dann_index_device_pointers).
 *   mean[c] = (f32)(sum_c / (f64)nrows), sum_c the SEQUENTIAL f64 sum of column c in row order from 0.0.  The sum is
 *   evaluated in parallel over ranges of rows wherever no addition can round -- it is then the same in any order -- and
 *   row by row from the carry elsewhere: the returned bits are those of the sequential walk.
 *   d_r = SquaredL2::evaluate(mean, row_r): f32 rows in the f32 x f32 order, f16 rows in the f32 x f16 order, u8 / i8 rows
 *   widened to f32 in the f32 x f32 order (not the integer kernels).  *out_row = the first row with d_r < min, min
 *   starting at f32::MAX: equal distances keep the earlier row, a NaN distance never wins, and -1 says that no row won
 *   (nrows == 0, or no distance below f32::MAX; the mean of no rows is the zero vector, as in the reference).
 * out_mean (dim floats, may be NULL).  out_counters (may be NULL): 4 words -- [0] ranges of a column summed in parallel,
 * [1] ranges walked row by row, [2] rows scanned, [3] distances that were NaN.  dim == 0: DANN_EINVAL; dim > 16000:
 * DANN_EUNSUPPORTED.  device < 0: the current device.  dann_medoid takes host pointers; dann_medoid_device takes rows
 * and out_mean in device memory (out_row and out_counters stay host pointers) and is host-synchronous on the null
 * stream. */
int32_t dann_medoid(int32_t device, int32_t dtype, const void* rows, uint64_t nrows, uint32_t dim,
                    uint64_t row_stride_bytes, int64_t* out_row, float* out_mean, uint64_t* out_counters);
int32_t dann_medoid_device(int32_t device, int32_t dtype, const void* rows, uint64_t nrows, uint32_t dim,
                           uint64_t row_stride_bytes, int64_t* out_row, float* out_mean, uint64_t* out_counters);

/* ---- the quantisers' transforms (diskann-quantization/src/algorithms/transforms), applied on the GPU, device to device.
 * Only CONSTRUCTING a transform draws random numbers; the host keeps doing that and hands over the parts that
 * Transform::try_from_parts and the flatbuffer carry.  Applying one is deterministic and is restated bit for bit from
 * the reference's x86-64 V3 path of hadamard_transform (algorithms/hadamard.rs:22-371):
 *   NullTransform    a copy
 *   PaddingHadamard  padding_hadamard.rs:204-273: input_dim = signs0_len, output_dim = subsample_len or padded_dim
 *   DoubleHadamard   double_hadamard.rs:238-287 (as its code runs: both transforms, also when the intermediate length is
 *                    a power of two): input_dim = signs0_len, output_dim = subsample_len or signs1_len
 *   RandomRotation   reserved: DANN_EUNSUPPORTED (a dense matrix through the reference's sgemm, whose summation order is
 *                    not part of its source)
 * Validation is that of try_from_parts (padding_hadamard.rs:137-173, double_hadamard.rs:146-206): each error variant is
 * DANN_EINVAL with the variant's name in the message; so are a padded_dim that is not a power of two, empty signs, and
 * a DoubleHadamard with a subsample whose signs1_len differs from signs0_len (the reference's constructor never builds
 * one and its transform would index out of bounds).  A working length (padded_dim, or max(input_dim, output_dim)) above
 * 16384 floats: DANN_EUNSUPPORTED. */
enum { DANN_TRANSFORM_NULL = 0,
       DANN_TRANSFORM_PADDING_HADAMARD = 1,
       DANN_TRANSFORM_DOUBLE_HADAMARD = 2,
       DANN_TRANSFORM_RANDOM_ROTATION = 3 /* reserved: DANN_EUNSUPPORTED */ } /* dann_transform_kind */;
typedef struct {
    int32_t kind;              /* DANN_TRANSFORM_* */
    uint32_t dim;              /* NULL only: input = output dim */
    const uint32_t* signs0;    /* each 0 or 0x80000000; PADDING: `signs` */
    uint32_t signs0_len;       /* = input_dim */
    const uint32_t* signs1;    /* DOUBLE only */
    uint32_t signs1_len;
    uint32_t padded_dim;       /* PADDING only */
    const uint32_t* subsample; /* NULL with subsample_len 0 = none; strictly increasing */
    uint32_t subsample_len;
} dann_transform_parts;        /* host pointers; the arrays are copied */
typedef struct dann_transform dann_transform; /* == algorithms::transforms::Transform, resident on one device */
int32_t dann_transform_create(int32_t device, const dann_transform_parts* parts, dann_transform** out);
int32_t dann_transform_destroy(dann_transform* t);
int32_t dann_transform_input_dim(const dann_transform* t);
int32_t dann_transform_output_dim(const dann_transform* t);
/* Transform::transform_into for n rows.  Host pointers, packed rows of input_dim / output_dim floats. */
int32_t dann_transform_apply(const dann_transform* t, const float* x, uint32_t n, float* out);
/* The same on the transform's device: strides in floats (>= the respective dim, else DANN_EINVAL), floats between the
 * rows of d_out are left untouched; complete on return. */
int32_t dann_transform_apply_device(const dann_transform* t, const float* d_x, uint64_t x_stride, uint32_t n, float* d_out,
                                    uint64_t out_stride);
/* MinMaxQuantizer::compress_into::<bits> INCLUDING the transform (minmax/quantizer.rs:117-228): x n rows of input_dim
 * floats, out n images of dann_layer_bytes(48 + bits, output_dim), padding bits zero; out_loss optional.  A NaN in a
 * transformed vector: DANN_EINVAL (InputContainsNaN).  bits and grid_scale as dann_minmax_compress.  Host pointers. */
int32_t dann_minmax_quantize(const dann_transform* t, int32_t bits, float grid_scale, const float* x, uint32_t n, void* out,
                             float* out_loss);
/* Device form: rows x_stride floats apart, images out_stride bytes apart (>= the layer bytes; bytes between images are
 * left untouched), ready for dann_set_elements_device or as d_queries; d_out_loss (optional) n floats on the device.
 * One 4-byte NaN flag is read back, nothing else crosses PCIe; complete on return. */
int32_t dann_minmax_quantize_device(const dann_transform* t, int32_t bits, float grid_scale, const float* d_x,
                                    uint64_t x_stride, uint32_t n, void* d_out, uint64_t out_stride, float* d_out_loss);

/* ---- SphericalQuantizer::compress_into on the GPU (diskann-quantization/src/spherical/quantizer.rs): rows
 * (spherical::Data<bits>, :805-918 with the 1-bit finish :596-647 and maximize_cosine_similarity :991-1100 over SliceHeap)
 * and queries (:1128-1212) from f32 vectors, byte for byte the reference's x86-64 V3 results: preprocess (:338-381) with
 * every f32 operation on its own and both inner products in the V3 order, the transform of the handle, then the width's
 * finish.  A dann_spherical is the compressing half of a SphericalQuantizer, resident on the transform's device.
 * Training (centroid, mean norm), RandomRotation, the FullQuery layout and 8-bit data stay with the host.
 * dann_spherical_create COPIES what it needs from `t` (signs, subsample, dims): the transform may be destroyed first.
 * Errors: DANN_EINVAL for a metric outside SupportedMetric, a shift that is not finite, pre_scale <= 0 or not finite,
 * bits outside {1, 2, 4}, a layout value that is no dann_query_layout, strides below a row / an image, a vector whose
 * shifted norm is not finite (InputContainsNaN: a NaN or an overflowing input), and a DataMeta field that does not fit
 * (EncodingError: DataMetaError::InnerProductCorrection / MetricSpecific / BitSum, vectors.rs:265-290; the variant is
 * named in dann_last_error); DANN_EUNSUPPORTED for DANN_QUERY_FULL_PRECISION and for a layout the width does not have.
 * After DANN_EINVAL from a vector the images of the other vectors are complete, the refused one's unspecified.
 * A vector at the centroid (shifted norm 0) gives an image of zero bytes, codes and meta.  n == 0 is DANN_OK. */
typedef struct {
    int32_t metric;        /* DANN_L2 | DANN_INNER_PRODUCT | DANN_COSINE (SupportedMetric) */
    const float* shift;    /* input_dim floats, host: SphericalQuantizer::shift() (the centroid as the quantiser stores it) */
    float pre_scale;       /* SphericalQuantizer::pre_scale(), > 0 and finite */
} dann_spherical_parts;
typedef struct dann_spherical dann_spherical;
int32_t dann_spherical_create(const dann_transform* t, const dann_spherical_parts* parts, dann_spherical** out);
int32_t dann_spherical_destroy(dann_spherical* q);
/* CompensatedIP::new: FastL2NormSquared(shift) -- what dann_config.sq_shift_norm_sq of the index wants */
int32_t dann_spherical_shift_norm_sq(const dann_spherical* q, float* out);
/* rows: x n rows of input_dim floats -> n images of dann_layer_bytes(32 + bits, output_dim), padding bits zero; bits in
 * {1, 2, 4}.  Host pointers. */
int32_t dann_spherical_compress(const dann_spherical* q, int32_t bits, const float* x, uint32_t n, void* out);
/* Device form: rows x_stride floats apart, images out_stride bytes apart (bytes between images are left untouched), ready
 * for dann_set_elements_device.  One 4-byte flag word is read back, nothing else crosses PCIe; complete on return. */
int32_t dann_spherical_compress_device(const dann_spherical* q, int32_t bits, const float* d_x, uint64_t x_stride,
                                       uint32_t n, void* d_out, uint64_t out_stride);
/* queries under a dann_query_layout: SAME_AS_DATA (== the rows), FOUR_BIT_TRANSPOSED (bits == 1),
 * SCALAR_QUANTIZED (bits in {2, 4}); images of the size dann_query_bytes() reports for such an index */
int32_t dann_spherical_compress_queries(const dann_spherical* q, int32_t bits, int32_t layout, const float* x,
                                        uint32_t n, void* out);
int32_t dann_spherical_compress_queries_device(const dann_spherical* q, int32_t bits, int32_t layout, const float* d_x,
                                               uint64_t x_stride, uint32_t n, void* d_out, uint64_t out_stride);

/* build-path options (never change the resulting graph).  The matrix-core path evaluates the pair similarities a
 * RobustPrune asks for (prune.rs:196-232) as the lower triangle of one Gram matrix per candidate list
 * (v_mfma_f32_32x32x2_f32; three kernels: list / sort, Gram tiles, sweep), with a bit-exact re-evaluation of every
 * comparison the rounding-error interval of the Gram value does not decide.  f32 and f16 rows, L2 / inner product /
 * cosine-normalized; other configurations ignore the flags.  Default: rows of 1 KiB and more use it. */
enum { /* back-edge prunes (add_edge_and_prune -> robust_prune_list, diskann/src/graph/index.rs:2264-2341) of any row size */
       DANN_BUILD_MFMA_BACKEDGE = 1,
       /* the pool prune of every inserted point (robust_prune_with, index.rs:2476-2532) of any row size: Gram of the
        * first <= 256 sorted candidates against the first 96; pairs outside that block use the row kernel */
       DANN_BUILD_MFMA_POOL = 2,
       /* never use the matrix-core path */
       DANN_BUILD_ROW_KERNEL_ONLY = 4 };
int32_t dann_set_build_options(dann_index* idx, uint32_t flags);
/* work counters of the build path since index creation (the algorithmic-bytes model of profiles/): out[0] back-edge
 * prunes through the MFMA path, [1] back-edge prunes of lists too long for it, [2] comparisons and [3] hops of the
 * insert-time searches, [4] pair distances d(c_i, c_j) evaluated by the row kernel in the prune sweeps, [5] list /
 * extra distances d(location, c), [6] candidate rows that went through an MFMA Gram, [7] Gram entries computed
 * (x dim x 2 = MFMA flop), [8] pair distances the lazy scans of the MFMA sweeps asked for, [9] those of [8] that needed
 * an exact re-evaluation by the row kernel (the rest were answered from a Gram), [10] tied candidate pools whose
 * DANN_TIE_RUST walk ran into the selection's last resort: after sixteen unlucky partitions core's select_nth_unstable_by
 * calls median_of_medians, which csrc/rust_order.h replaces by a sort of the range -- the index-th element is in place
 * either way, equal keys may be arranged differently, so such a pool is not guaranteed to match the reference's order
 * (never reached by the reference's goldens or by any build measured so far; 0 = the promise of
 * dann_set_prune_tie_order holds for every pool of this index's builds).  n <= 11 entries are written. */
int32_t dann_build_counters(const dann_index* idx, uint64_t* out, uint32_t n);

/* ---- deletion and graph consolidation -------------------------------------------------------
 * DataProvider::delete (diskann/src/provider.rs:165) + DiskANNIndex::consolidate_vector (diskann/src/graph/index.rs:
 * 1819-1930) + drop_adj_list (index.rs:1060).  The deleted state is one bit per slot on the device, created by the first
 * delete (an index that never deletes has none).
 *
 * dann_delete_points marks `slots` deleted; deleting a slot twice is fine.  A slot >= capacity + num_start_points is
 * DANN_EBOUNDS, a start point DANN_EINVAL (start points are FROZEN); on either error nothing is marked.  On an
 * inline_tags index the slots' tags also become RETIRING (2, diskann-inmem/src/tag.rs:81-135), so searches skip them
 * at once.  On an index without tags the mark only drives dann_consolidate: searches are unchanged and may still return a
 * deleted point until the graph has been consolidated (and its list dropped with DANN_CONSOLIDATE_DROP_DELETED).
 * Slots are never reused or freed here: a deleted slot stays deleted for dann_consolidate even if its row is written
 * again with dann_set_element(s) (which publishes its tag) -- do not rewrite a deleted slot.
 *
 * dann_get_deleted writes 0 / 1 per slot of [first_slot, first_slot + n).
 *
 * dann_consolidate runs consolidate_vector on every id of ids[0, n) -- ids == NULL: on every slot of
 * [0, capacity + num_start_points), n is then ignored -- in one batched pass whose result equals the reference's
 * sequential loop in any order:
 *   - a deleted vertex is left alone: DANN_CONSOLIDATE_DELETED;
 *   - otherwise the pool is the vertex's live neighbours plus the live neighbours of each of its deleted neighbours (not
 *     transitive), without duplicates and without the vertex itself;
 *   - no deleted neighbour and a pool (counting the vertex itself if it is listed, as the reference does) of at most
 *     cfg->pruned_degree entries: nothing is written; else a pool of fewer than pruned_degree entries becomes the list;
 *     else robust_prune_list (index.rs:2397-2454) with force_saturate = false prunes it, under the tie order of
 *     dann_set_prune_tie_order, on the kernels of the back-edge prunes (dann_set_build_options; their work is counted
 *     with theirs in dann_build_counters: [0] the prunes on the matrix cores, [4] - [9] the distances and Gram entries).
 * Pool order: the reference collects the pool in a HashSet with a random hasher, so its order -- and any tie it breaks --
 * is unspecified.  Here it is first-occurrence order: the vertex's own live neighbours in list order, then the live
 * neighbours of each deleted neighbour, the deleted neighbours taken in the order of the vertex's list.
 * out_kind (may be NULL): one DANN_CONSOLIDATE_* per id.  flags: DANN_CONSOLIDATE_DROP_DELETED empties the lists of all
 * deleted slots after the pass.  out_counters (may be NULL): 8 words -- [0] vertices scanned, [1] lists rewritten without
 * a prune, [2] pools pruned, [3] largest pool, [4] distances evaluated: d(vertex, c) of every pruned pool plus the pair
 * distances the prune sweeps asked for (dann_build_counters [4] + [8] over the call), [5] pools pruned on the matrix
 * cores, [6] pools of more than 4096 candidates (possible only with max_degree > 64): their max_occlusion_size nearest
 * are selected exactly in global memory before the prune, [7] those of [6] whose selected head holds equal distances
 * under DANN_TIE_RUST -- there the order of equal distances is by pool position, not Rust's order of the whole pool.
 * Pools of any size are consolidated.
 * Errors: DANN_EBOUNDS for an id out of range, DANN_EINVAL for a bad config or flag, DANN_EUNSUPPORTED for DANN_PQ
 * indexes and for max_occlusion_size > 4096 (as for the build).
 * All three calls are mutations: DANN_EBUSY while search-server tickets are outstanding. */
enum { DANN_CONSOLIDATE_COMPLETE = 0, DANN_CONSOLIDATE_DELETED = 1 };
enum { DANN_CONSOLIDATE_DROP_DELETED = 1 };
int32_t dann_delete_points(dann_index* idx, const uint32_t* slots, uint32_t n);
int32_t dann_get_deleted(const dann_index* idx, uint32_t first_slot, uint32_t n, uint8_t* out);
int32_t dann_consolidate(dann_index* idx, const dann_build_config* cfg, const uint32_t* ids, uint32_t n, uint32_t flags,
                         int32_t* out_kind, uint64_t* out_counters);

/* ---- finishing a build: what the reference's in-memory builder runs after its inserts
 * (diskann-disk/src/build/builder/inmem_builder.rs): final_prune, the reachability check and the degree statistics.
 *
 * dann_prune_range == DiskANNIndex::prune_range (index.rs:2656-2701) on ids[0, n), or with ids == NULL on the slots
 * [first, first + n).  A list of at most cfg->pruned_degree entries is left alone; a longer one is replaced by
 * robust_prune_list(id, list) with force_saturate = false (index.rs:2397-2454): the pool is the list in list order
 * without id itself, d(id, c) the index's pair distance, the tie order that of dann_set_prune_tie_order, the kernels
 * those of dann_set_build_options -- the pass of dann_consolidate without deleted state, its prune work counted in
 * dann_build_counters in the same way.  One vertex's prune reads only rows and its own list, so the batched pass equals
 * the sequential loop in any order; an id given twice is pruned once (the reference's second visit finds a short list).
 * On an inline-tags index a neighbour whose slot is unreadable stays out of the pool.  The reference aborts its loop
 * with an error when an id's OWN slot is unreadable; here that id is left alone and counted, and the pass goes on.
 * out_counters (may be NULL): 6 words -- [0] distinct ids scanned, [1] lists pruned, [2] longest list among them,
 * [3] distances evaluated, [4] lists pruned on the matrix cores, [5] ids left alone because their own slot is unreadable.
 * Errors: DANN_EBOUNDS for an id or a range past the last slot, and for a list to prune that holds a neighbour id past the
 * last slot (dann_set_neighbors admits one): that list is left as it is, the other lists of the call are pruned;
 * DANN_EINVAL for a bad config, DANN_EUNSUPPORTED for DANN_PQ indexes and for max_occlusion_size > 4096.  A mutation:
 * DANN_EBUSY while search-server tickets are outstanding.
 *
 * dann_count_reachable == count_reachable_nodes (index.rs:2161-2189): the number of distinct nodes a breadth-first walk
 * over the adjacency rows expands from start_ids[0, n_start) -- NULL: the index's start points.  Pure graph: no tags, no
 * deleted bitmap, no vectors; a list's length word is clamped to max_degree; duplicate start ids count once.
 * out_levels (may be NULL): the greatest depth reached, start points at depth 0.  out_bitmap (host, may be NULL):
 * (capacity + num_start_points + 31) / 32 words, bit i set = slot i was reached.  DANN_EBOUNDS for a start id or a
 * stored neighbour id past the last slot.  Takes the index shared, like a search.
 *
 * dann_degree_stats == get_degree_stats (index.rs:2191-2239) over ids[0, n) -- a repeated id counts each time -- or with
 * ids == NULL over the slots [0, capacity), the reference's non_start_points_ids.  DANN_DEGREE_SKIP_DELETED leaves out
 * slots that the deleted bitmap marks.  avg_degree = (float)total / (float)points; no points: all zeros.
 * The struct is the reference's DegreeStats with the exact totals behind avg_degree; it cannot carry the name of the call
 * that fills it (in C a typedef and a function share one namespace), hence dann_degree_summary. */
typedef struct {
    uint32_t max_degree;
    float avg_degree;
    uint32_t min_degree;
    uint32_t reserved;
    uint64_t cnt_less_than_two;
    uint64_t points; /* lists counted */
    uint64_t total;  /* sum of their lengths */
} dann_degree_summary;
enum { DANN_DEGREE_SKIP_DELETED = 1 };
int32_t dann_prune_range(dann_index* idx, const dann_build_config* cfg, const uint32_t* ids, uint32_t first, uint32_t n,
                         uint64_t* out_counters);
int32_t dann_count_reachable(const dann_index* idx, const uint32_t* start_ids, uint32_t n_start, uint64_t* out_count,
                             uint32_t* out_levels, uint32_t* out_bitmap);
int32_t dann_degree_stats(const dann_index* idx, const uint32_t* ids, uint32_t n, uint32_t flags, dann_degree_summary* out);

/* ---- diversity-aware search: graph::search::Diverse (diskann/src/graph/search/diverse_search.rs:27-233) over
 * DiverseNeighborQueue (diskann/src/neighbor/diverse_priority_queue.rs:63-238).
 *
 * Attributes: the AttributeValueProvider crosses the boundary as one u32 per slot of [0, capacity + num_start_points)
 * (the slot range of the filter bitmap), stored on the device.  The store is created by the first dann_set_attributes
 * with every slot DANN_NO_ATTRIBUTE (the provider returns None: the slot is never queued -- not the same as value 0) and
 * freed with the index.  A range past the last slot is DANN_EBOUNDS.  dann_set_attributes is a mutation.
 *
 * dann_diverse_search_batch: index.search(Diverse::new(Knn{l_value, beam_width}, DiverseSearchParams{diverse_k,
 * total_k}), ..) for nq queries; queries and outputs as dann_search_batch (host memory, nq x k, unwritten entries
 * 0xFFFFFFFF / +inf, slot ids).  DiverseSearchParams::diverse_attribute_id is never read by the queue and does not cross.
 *   - The local queues hold dl = diverse_k * l_value / total_k entries (integer division, :90-104); the global queue L.
 *   - The beam loop is search_internal (index.rs:1933-2000); the candidates of a hop are inserted one by one in
 *     adjacency order.  Afterwards every local queue is cut to diverse_k and what was cut leaves the global queue
 *     (post_process, :112-138); best.iter().take(l_value) then goes through the Knn post-processor: start points are
 *     dropped, result_count and stats as dann_search_batch.
 *   - Equal distances follow NeighborPriorityQueue exactly (neighbor/queue.rs:130-222): lower-bound insertion, and a
 *     remove that only looks at the lower-bound position and so may fail.
 *   - An index without attributes (or whose start points have none) returns 0 results, 0 hops.
 *   - Rows: f32, f16, u8, i8, SQ-8 with the metrics of dann_search_batch; DANN_PQ is DANN_EUNSUPPORTED.  Inline-tag
 *     indexes skip unreadable slots as dann_search_batch does.  l_value + num_start_points <= 1024, beam_width <= 16.
 * Errors (DiverseSearchError / DiverseError): DANN_EINVAL for total_k == 0, diverse_k == 0, diverse_k > total_k,
 * l_value < total_k, l_value == 0 or beam_width == 0. */
#define DANN_NO_ATTRIBUTE 0xFFFFFFFFu
typedef struct {
    uint32_t diverse_k;  /* DiverseSearchParams::diverse_results_k */
    uint32_t total_k;    /* DiverseSearchParams::total_k_value */
} dann_diverse;
int32_t dann_set_attributes(dann_index* idx, uint32_t first_slot, uint32_t n, const uint32_t* values);
int32_t dann_get_attributes(const dann_index* idx, uint32_t first_slot, uint32_t n, uint32_t* out);
int32_t dann_diverse_search_batch(dann_index* idx, const void* queries, uint32_t nq, uint32_t l_value,
                                  uint32_t beam_width, uint32_t k, const dann_diverse* params, uint32_t* out_ids,
                                  float* out_dists, dann_search_stats* out_stats);

/* ---- in-place deletes ------------------------------------------------------------------------
 * DiskANNIndex::multi_inplace_delete / inplace_delete (diskann/src/graph/index.rs:1338-1551, inplace_delete_inner
 * 1585-1747) + drop_deleted_neighbors (index.rs:1756-1816): the graph is repaired around the deleted points at delete
 * time, without a pass over the whole index.  Meant to be paired with an occasional dann_drop_deleted_neighbors sweep
 * and, once many points are gone, dann_consolidate.
 *
 * dann_inplace_delete is one minibatch of multi_inplace_delete (the caller splits a longer list into chunks of
 * max_minibatch_par and runs them one after another, as the reference does; n = 1 is inplace_delete):
 *   1. Deletion comes first: every id of the call is marked deleted (as dann_delete_points) before any work list is built.
 *      The reference deletes inside each parallel task; "all marks first" is one of its schedules, and the only one that
 *      makes the result deterministic.  A repeated id counts once, at its first position.
 *   2. Readable: for the whole call a slot is unreadable if it is marked deleted or, on an inline_tags index, its tag is
 *      below PUBLISHED -- so a tagless index behaves like the same index with tags.  Unreadable slots are never replace
 *      candidates or in-neighbours, and robust_prune_list leaves them out of its pool (view.get is None).
 *   3. Work lists (index.rs:1168-1336), `live` meaning readable:
 *        DANN_INPLACE_ONE_HOP: the live out-neighbours of the id, in list order, are both the replace candidates and the
 *          in-neighbour candidates;
 *        DANN_INPLACE_TWO_HOP_AND_ONE_HOP: the replace candidates as for ONE_HOP; the in-neighbour candidates are those
 *          neighbours plus every entry of their lists, deduplicated, unreadable ids removed, in first-occurrence order
 *          (the reference's HashSet order is unspecified; no output depends on it);
 *        DANN_INPLACE_VISITED_AND_TOPK: a Knn search_internal with the deleted row as the query, L = l_value, beam
 *          width 1 (NeighborPriorityQueue: capacity l_value + start points, lower-bound inserts, so a later candidate at
 *          an equal distance goes in front of an earlier one -- a start point, inserted first, included), unreadable
 *          slots put into the visited set and skipped, distances the pair distances d(id, c) of the prunes.  The CopyIds
 *          post-processor: start points kept, the first min(l_value, size) entries in queue order are the in-neighbour
 *          candidates; the first k_value of them are the replace candidates (index.rs:1168-1233);
 *        the in-neighbours are the candidates whose list contains the id.
 *   4. Replacement edges: for each in-neighbour c, d(c, r) for every replace candidate r != c (the bit-exact pair
 *      distances of the prunes), ordered as sort_unstable_by(fast_distance) under dann_set_prune_tie_order
 *      (DANN_TIE_POSITION: (distance, position); DANN_TIE_RUST: Rust's order -- insertion sort up to 20, ipnsort beyond),
 *      and the first num_to_replace give the edges c -> r.  For each live out-neighbour o of the id the same selection
 *      over the candidates r != o gives the edges r -> o.
 *   5. Aggregation: a source's targets are concatenated over the call's ids in call order, each id's in its own edge
 *      order (c's edges as in-neighbour first, then r -> o in the order of the id's list).  Every distinct source (every
 *      in-neighbour is one, even without a replacement) gets add_edge_and_prune (index.rs:2264-2341) with to_remove = the
 *      ids of this call only: edges to points deleted by earlier calls stay.  The extend skips ids already in the list.
 *      Nothing added and nothing removed: nothing is written; a list that fits cfg->max_degree (max_degree_with_slack)
 *      becomes the row; else robust_prune_list (force_saturate = false) under the index's tie order, on the back-edge
 *      prune kernels.  Each source reads only its own list and the rows, so the batch does not depend on order.
 *   6. The lists of the call's ids are dropped (drop_adj_list).
 *   out_counters (may be NULL): DANN_INPLACE_COUNTERS words -- [0] ids repaired (distinct), [1] in-neighbours found,
 *   [2] replace candidates, [3] pair distances of the edge step, [4] distinct sources, [5] lists appended, [6] lists set
 *   without a prune (an edge was removed), [7] lists pruned, [8] of those, the pools pruned on the matrix cores.
 *   Errors: DANN_EBOUNDS for an id out of range; DANN_EINVAL for a start point, an id an earlier
 *   call deleted (the reference's id translation fails for the whole chunk, diskann-inmem/src/provider.rs:274-294), a bad
 *   cfg or params (VISITED_AND_TOPK: k_value > 0, 0 < l_value <= 2048), or more than 2^20 ids; DANN_EUNSUPPORTED for
 *   DANN_PQ rows, max_degree + the replace candidates' capacity above 4096, TWO_HOP_AND_ONE_HOP with max_degree > 256,
 *   and a call whose edges would overflow its buffers (a vertex with a pool of more than 4096 candidates, 2^31 edges):
 *   split the minibatch.  Every error before the rows are rewritten removes the call's marks again; a HIP error while
 *   rows are being rewritten leaves the marks and the rows written so far.
 *   A mutation: DANN_EBUSY while search-server tickets are outstanding.
 *
 * dann_drop_deleted_neighbors runs drop_deleted_neighbors on ids[0, n) -- ids == NULL: every slot of
 * [0, capacity + num_start_points) -- in one batched pass that equals the sequential loop (a vertex's rewrite reads only
 * its own list and its deleted neighbours' list lengths, and a deleted vertex is never rewritten).  "Deleted" is
 * unreadable as above.  A deleted vertex gets DANN_CONSOLIDATE_DELETED; otherwise the pool is its live neighbours in list
 * order, then with only_orphans the deleted neighbours whose own list is non-empty, in list order.  No deleted neighbour
 * and a pool of at most cfg->pruned_degree: nothing is written; else the list becomes the pool, without a prune.
 * out_kind (may be NULL): one DANN_CONSOLIDATE_* per id.  DANN_EBOUNDS for an id out of range.  A mutation. */
enum { DANN_INPLACE_VISITED_AND_TOPK = 0, DANN_INPLACE_TWO_HOP_AND_ONE_HOP = 1, DANN_INPLACE_ONE_HOP = 2 };
enum { DANN_INPLACE_COUNTERS = 9 };
typedef struct {
    uint32_t method;         /* DANN_INPLACE_* (graph::InplaceDeleteMethod, diskann/src/graph/misc.rs:28-32) */
    uint32_t k_value;        /* VISITED_AND_TOPK only: replace candidates = the first k_value search results */
    uint32_t l_value;        /* VISITED_AND_TOPK only: the search's L and the number of results kept */
    uint32_t num_to_replace;
} dann_inplace_delete_params;
int32_t dann_inplace_delete(dann_index* idx, const dann_build_config* cfg, const uint32_t* ids, uint32_t n,
                            const dann_inplace_delete_params* p, uint64_t* out_counters);
int32_t dann_drop_deleted_neighbors(dann_index* idx, const dann_build_config* cfg, const uint32_t* ids, uint32_t n,
                                    uint32_t only_orphans, int32_t* out_kind);

/* ---- multi-vector (late-interaction) scores: diskann-quantization/src/multi_vector/ ------------------------------------
 * A query and a document are small matrices of token rows (row-major, `dim` elements each, DANN_F32 or DANN_F16, query
 * and document of one type).  MaxSim: for each query row the best inner product over the document's rows, as a
 * similarity score (negated: smaller is better); Chamfer: their sum over the query's rows.  Two orders, because their
 * bits differ -- the choice is the caller's and is never made by speed:
 *   DANN_MAXSIM_KERNEL     what build_max_sim(Auto | X86_64_V3 | X86_64_V4, query).compute_max_sim(doc, scores) returns:
 *                          ip(i, j) = one fma chain over k = 0 .. dim - 1 from +0.0 (f16 widened first, exactly),
 *                          scores[i] = -max_j ip(i, j), the maximum from f32::MIN, the negation last (a maximum of +0.0
 *                          gives -0.0).  Runs on the matrix cores (v_mfma_f32_32x32x2_f32 is that chain bit for bit).
 *   DANN_MAXSIM_REFERENCE  MaxSim::evaluate / Chamfer::evaluate / MaxSimIsa::Reference: scores[i] = min_j
 *                          InnerProduct::evaluate(q_i, d_j), the minimum from f32::MAX -- the pair function behind
 *                          dann_distance_pairs with DANN_INNER_PRODUCT.
 * Both: a document without rows scores f32::MAX for every query row and has Chamfer 0.0; Chamfer = the sequential f32 sum
 * of scores[i] in query-row order from 0.0 (0.0 for a query without rows).
 * Outside the contract: NaN or infinite inputs (the CPU's vmaxps operand rule is not reproduced), and products that
 * underflow to -0.0 (the sign of a zero maximum is then ambiguous in the reference itself).
 *
 * A dann_mvset is an immutable, device-resident set of ndocs documents in CSR form: document d is rows
 * [row_offsets[d], row_offsets[d + 1]) of `rows`; row_offsets[0] == 0, non-decreasing; documents without rows allowed.
 * Queries are CSR too: query q is rows [q_offsets[q], q_offsets[q + 1]) of `queries`, in the set's dtype.
 * cand_ids: nq x cand_stride document ids; entries equal to 0xFFFFFFFF are skipped, their out_chamfer and out_scores
 * cells written as +infinity.  out_chamfer: nq x cand_stride.  out_scores: NULL, or the per-row MaxSim scores: those of
 * (q, c) are the q_rows(q) floats at q_offsets[q] * cand_stride + c * q_rows(q).
 * Limits: 1 <= dim <= 4096; at most 1024 rows per query; any number of rows per document; cand_stride 1 .. 4096;
 * nq <= 65535 per call.  Beyond them: DANN_EUNSUPPORTED.
 * Errors: DANN_EINVAL for null pointers, an order that is not a DANN_MAXSIM_*, a dtype other than DANN_F32 / DANN_F16 /
 * DANN_MM1 / MM2 / MM4 / MM8,
 * dim == 0, k == 0; DANN_ELENGTH for offsets that decrease or do not start at 0; DANN_EBOUNDS for a candidate id >= ndocs
 * (found on the device instead of the read; the outputs of that call are then unspecified).
 * The calls are host-synchronous.  The _device forms take queries, offsets, candidates and outputs on the set's device.
 *
 * MinMax-quantised sets (diskann-quantization/src/minmax/multi/: MinMaxMeta<NBITS>, MinMaxKernel::max_sim_kernel):
 * dtype DANN_MM1 / MM2 / MM4 / MM8.  `rows` and `queries` are then packed canonical images of dann_layer_bytes(dtype, dim)
 * bytes each -- the 20-byte MinMaxCompensation, then ceil(dim * bits / 8) code bytes: what dann_minmax_compress writes.
 * With query row x the FIRST argument and document row y the second (minmax/vectors.rs:206-269; the epilogue is not
 * symmetric), raw the exact u32 inner product of the codes and every f32 operation on its own:
 *   v = (((x.a * y.a) * (f32)raw + x.n * y.b) + y.n * x.b) + (x.b * y.b) * (f32)dim
 *   scores[i] = min_j -v(i, j), the minimum from f32::MAX; Chamfer and documents or queries without rows as above.
 * `dim` is the set's; an image's u32 dim field is not read, nor are code bits at or beyond dim * bits.  raw is an integer
 * and has no summation order, so both orders return the same bits and `order` only picks the kernel: DANN_MAXSIM_KERNEL
 * the int8 matrix cores (v_mfma_i32_32x32x32_i8), DANN_MAXSIM_REFERENCE a plain loop over the packed codes.
 * Outside the contract: NaN or infinite header fields; a query row whose candidate minima include zeros of both signs.
 * dann_mvset_set_query_dtype: the dtype of the queries' images, read once at the entry of a scoring call.  Default: the
 * set's own.  On an MM4 / MM2 / MM1 set DANN_MM8 is also allowed (the reference's mixed pairs (8,4), (8,2), (8,1),
 * bits/distances.rs:1621); any other MinMax pair is DANN_EUNSUPPORTED, a non-MinMax dtype on a MinMax set and any dtype
 * but the set's own on an f32 / f16 set DANN_EINVAL. */
typedef struct dann_mvset dann_mvset;
enum { DANN_MAXSIM_KERNEL = 0, DANN_MAXSIM_REFERENCE = 1 };
int32_t dann_mvset_create(int32_t device, int32_t dtype, uint32_t dim, uint32_t ndocs, const uint64_t* row_offsets,
                          const void* rows, dann_mvset** out);
int32_t dann_mvset_destroy(dann_mvset* set);
int32_t dann_mvset_info(const dann_mvset* set, int32_t* dtype, uint32_t* dim, uint32_t* ndocs, uint64_t* nrows);
int32_t dann_mvset_set_query_dtype(dann_mvset* set, int32_t dtype);
int32_t dann_mvset_get_query_dtype(const dann_mvset* set, int32_t* out);
int32_t dann_maxsim_batch(const dann_mvset* set, int32_t order, const void* queries, const uint32_t* q_offsets,
                          uint32_t nq, const uint32_t* cand_ids, uint32_t cand_stride, float* out_chamfer,
                          float* out_scores);
int32_t dann_maxsim_batch_device(const dann_mvset* set, int32_t order, const void* d_queries, const uint32_t* d_q_offsets,
                                 uint32_t nq, const uint32_t* d_cand_ids, uint32_t cand_stride, float* d_out_chamfer,
                                 float* d_out_scores);
/* the same Chamfer scores, sorted ascending per query (equal scores keep candidate order, skipped entries dropped), the
 * first k returned: out_ids / out_dists nq x k, padded as dann_rerank_batch pads (0xFFFFFFFF / +infinity);
 * out_counts[q] = entries written for query q */
int32_t dann_chamfer_rerank_batch(const dann_mvset* set, int32_t order, const void* queries, const uint32_t* q_offsets,
                                  uint32_t nq, const uint32_t* cand_ids, uint32_t cand_stride, uint32_t k,
                                  uint32_t* out_ids, float* out_dists, uint32_t* out_counts);
int32_t dann_chamfer_rerank_batch_device(const dann_mvset* set, int32_t order, const void* d_queries,
                                         const uint32_t* d_q_offsets, uint32_t nq, const uint32_t* d_cand_ids,
                                         uint32_t cand_stride, uint32_t k, uint32_t* d_out_ids, float* d_out_dists,
                                         uint32_t* d_out_counts);

/* ABI revision of this header; bumped on any incompatible change of a signature or struct layout */
#define DANN_ABI_VERSION 5
int32_t dann_abi_version(void);

/* ---- diagnostics ------------------------------------------------------------------- */
/* thread-local message of the last failing call on this thread; returns its length */
int32_t dann_last_error(char* buf, uint64_t len);
/* HIP-event time (ms) and launch count of the named kernel since the last reset.
 * which: 0 = beam search, 1 = gather distance, 2 = prune, 3 = back-edge,
 * 4 = beam-search retry launches (their time is also part of 0; `launches` counts re-run queries),
 * 5 = gram_tiles_kernel, the matrix-core kernel of the build's prunes (with dann_build_counters()[7] x dim x 2 flop:
 *     the MFMA rate of the build) */
int32_t dann_kernel_time(const dann_index* idx, int32_t which, double* total_ms, uint64_t* launches);
int32_t dann_kernel_time_reset(dann_index* idx);
/* tuning knob: per-query LDS visited-table size. 0 = auto from L and degree; 6..15 = log2(entries);
 * 64..32768 = explicit entry count (rounded up to a multiple of 64). Never affects results. */
int32_t dann_set_visited_bits(dann_index* idx, uint32_t bits);
/* tuning knob: width of a visited-table entry.  0 (default) = automatic: 16-bit entries -- an exact set all the same:
 * slot and entry together determine the id -- where they let more queries share a compute unit, 32-bit entries
 * otherwise; 32 / 16 = always that width (16 applies to the plain searches and falls back to 32 where the index has
 * too many slots for the table).  Never affects results. */
int32_t dann_set_visited_format(dann_index* idx, uint32_t entry_bits);
/* queries in flight per search call.  0 (default) = every query of the call gets its own wavefront at once;
 * N > 0 = N persistent wavefronts take the call's queries one after the other from a shared counter -- what a
 * server does that keeps N searches in flight (the reference: N tokio workers calling DiskANNIndex::search on a
 * shared index, SURVEY 8(b) "Threading"): a finished search is replaced at once instead of waiting for the slowest
 * of its batch.  Applies to the plain searches (beam width 1, no filter, no inline tags, degree <= 64: Knn, Range,
 * the insert search); the other modes keep one wavefront per query.  Never affects results. */
int32_t dann_set_max_concurrency(dann_index* idx, uint32_t max_queries_in_flight);
/* Order of EQUAL-distance candidates in RobustPrune's candidate pool (every prune of dann_prune_batch,
 * dann_insert_batch*, dann_build*).  SortedNeighbors::new (diskann/src/graph/internal/sorted_neighbors.rs:26-44) sorts
 * with select_nth_unstable_by + sort_unstable_by, whose order of equal keys is unspecified in the API and a
 * deterministic function of the pool's arrival order in the implementation.
 *   DANN_TIE_RUST (default): the order the reference's own toolchain leaves (rust-toolchain.toml: 1.97.1; core's
 *     "ipnsort" and its selection, Rust >= 1.81), walked sequentially by one lane per pool (csrc/rust_order.h), and the
 *     bootstrap's candidate list in AdjacencyList::from_iter_untrusted's ascending id order (adjacencylist.rs:181-190).
 *     With it the GPU build reproduces the reference's tie-heavy grid_insert goldens (tests/test_gpu_tie_order.py):
 *     the graph is the reference's graph on integer lattices, byte data and duplicated rows as well.
 *     Only pools that hold equal distances are walked (the sorting network's output is inspected first): builds of
 *     float rows cost what they cost under DANN_TIE_POSITION, a 200 k x 128 u8 build 12 % more.
 *   DANN_TIE_POSITION: equal distances keep their pool order (a stable sort; one wavefront-wide sorting network per
 *     pool, no walk).  Identical to DANN_TIE_RUST wherever the distances of a pool are distinct; on tied pools one of the
 *     orders the reference's API permits, not the one its implementation produces.
 * The same setting orders equal distances in the filtered searches' post-processing (dann_filtered_search_batch): the
 * matched list of the inline-filter search (`sort_unstable_by`, inline_filter_search.rs:274) and the rejected candidates
 * a multihop hop expands (multihop_filter_search.rs:207-210) -- Rust's order under DANN_TIE_RUST (lists with ties are
 * sorted again by one lane, in global memory: a conformance mode, slow on integer data), push order under
 * DANN_TIE_POSITION; tests/test_gpu_filtered.py::test_equal_distances_follow_the_references_unstable_sort.
 * Replicas of one sharded build (dann_build_sharded; dann_multi_build: dann_multi_replica) must use the same order. */
enum { DANN_TIE_POSITION = 0, DANN_TIE_RUST = 1 };
int32_t dann_set_prune_tie_order(dann_index* idx, uint32_t order);

/* ---- multi-GPU (replicated index per device).  Search shards with no data-path collective; the build splits every
 * multi_insert batch at its only exchange point (diskann/src/graph/index.rs:815-1030, :911-1024): candidates per rank,
 * all-gather of the pending adjacency rows, the same graph update on every replica with the prunes of overflowing
 * back-edge targets done by their owner (id % world) and a second all-gather of the rewritten rows.  The collectives
 * are issued by the library on device buffers: RCCL (ncclAllGather over xGMI, librccl bound at run time), an in-process
 * form for one process driving several devices, or the caller's own callback. ---- */
typedef struct dann_comm dann_comm;
typedef struct { char internal[128]; } dann_rccl_unique_id; /* == ncclUniqueId */
typedef struct {
    void* ctx;
    uint32_t rank, world;
    /* all-gather `bytes` bytes per rank, device buffers (d_recv holds world * bytes), enqueued on `hip_stream` (a
     * hipStream_t) or complete on return; 0 = ok */
    int32_t (*all_gather)(void* ctx, const void* d_send, void* d_recv, uint64_t bytes, void* hip_stream);
} dann_comm_ops;
int32_t dann_comm_create_callbacks(const dann_comm_ops* ops, dann_comm** out);
/* one process per GPU: rank 0 draws the id, the host distributes it (MPI / torch.distributed / a socket), every rank
 * creates its communicator on its device (-1 = current).  DANN_EUNSUPPORTED when librccl cannot be loaded. */
int32_t dann_comm_rccl_unique_id(dann_rccl_unique_id* out);
int32_t dann_comm_create_rccl(const dann_rccl_unique_id* id, uint32_t rank, uint32_t world, int32_t device, dann_comm** out);
/* one process, `world` devices (ranks = host threads): out receives `world` communicators */
int32_t dann_comm_create_local(const int32_t* devices, uint32_t world, dann_comm** out);
int32_t dann_comm_destroy(dann_comm* comm);
int32_t dann_comm_rank(const dann_comm* comm);
int32_t dann_comm_world(const dann_comm* comm);
/* the communicator's all-gather on caller buffers (device pointers on `device`); the build's primitive, exported for
 * pre-flight checks of a deployment */
int32_t dann_comm_all_gather_device(dann_comm* comm, int32_t device, const void* d_send, void* d_recv, uint64_t bytes);
/* dann_build over `world` identical replicas (rows already stored on every rank): same batch schedule, same graph on
 * every replica as a single-GPU dann_build.  Collective: every rank calls it with the same arguments.  Returns the
 * number of batches; stats (optional, 4 entries): exchange rounds, bytes of pending rows gathered, rows rewritten by
 * their owners, bytes of rewritten rows gathered. */
int32_t dann_build_sharded(dann_index* idx, dann_comm* comm, const dann_build_config* cfg, uint32_t first, uint32_t n,
                           float growth, uint32_t max_batch, uint64_t* stats);
/* every rank holds the same nq queries (host) and receives all nq results: rank r searches partition r of the block
 * (diskann/src/utils/async_tools.rs:289-365), the k results per query are all-gathered.  Collective. */
int32_t dann_search_sharded(dann_index* idx, dann_comm* comm, const void* queries, uint32_t nq, uint32_t l_value,
                            uint32_t beam_width, uint32_t k, uint32_t* out_ids, float* out_dists);
/* plain copies for hosts without HIP bindings (kind 0 host->device, 1 device->host, 2 device->device; synchronous) */
int32_t dann_memcpy_device(int32_t device, void* dst, const void* src, uint64_t bytes, int32_t kind);

/* one process driving several devices ("device mask"): one replica per entry of `devices` (an ordinal may repeat).
 * set_elements replicates the rows, build runs dann_build_sharded on one host thread per replica over the in-process
 * communicator, search_batch partitions the query block over the replicas (host buffers; out_stats optional). */
typedef struct dann_multi dann_multi;
int32_t dann_multi_create(const dann_config* cfg, const void* start_rows, uint64_t start_len, const int32_t* devices,
                          uint32_t ndev, dann_multi** out);
int32_t dann_multi_destroy(dann_multi* m);
int32_t dann_multi_size(const dann_multi* m);
dann_index* dann_multi_replica(dann_multi* m, uint32_t i);
int32_t dann_multi_set_elements(dann_multi* m, uint32_t first_slot, uint32_t n, const void* rows, uint64_t len);
int32_t dann_multi_build(dann_multi* m, const dann_build_config* cfg, uint32_t first, uint32_t n, float growth,
                         uint32_t max_batch, uint64_t* stats);
int32_t dann_multi_search_batch(dann_multi* m, const void* queries, uint32_t nq, uint32_t l_value, uint32_t beam_width,
                                uint32_t k, uint32_t* out_ids, float* out_dists, dann_search_stats* out_stats);

/* ---- search server: the reference's serving model -- N workers calling DiskANNIndex::search on one shared index,
 * one query per call (diskann-benchmark-core/src/search/api.rs:399-436, tokio.rs:10-14) -- without a kernel launch
 * per call.  dann_server_start keeps `workers` wavefronts resident on the device (Knn search, beam width 1, L =
 * l_value, k results); dann_search_submit copies one query (host pointer, layer bytes) into a ring in host-mapped
 * memory and returns a ticket; dann_search_wait blocks until that query's result has arrived and copies it out
 * (ids are slot ids, unwritten entries 0xFFFFFFFF / +inf, as dann_search_batch).  Every ticket must be waited for
 * exactly once, in any order and by any thread; at most `ring` tickets can be outstanding (a further submit waits for a
 * dann_search_wait to return a result slot; collecting tickets late never holds up another caller's submission).
 * Submit / wait / poll may be called from any number of threads concurrently and take no lock on the index; results are
 * identical to dann_search_batch.  Mutations of the index (set / insert / build / load) are refused with DANN_EBUSY
 * while tickets are outstanding (submitted and not yet collected by dann_search_wait), and a submit during a mutation
 * is refused with DANN_EBUSY.  dann_server_stop may be called while other threads are inside submit / wait / poll:
 * it unpublishes the server, those calls return DANN_EINVAL ("the server is being stopped"), and nothing is freed
 * before the last of them has left; uncollected tickets die with the server.  A submit whose ring position no worker
 * takes within 30 s means the resident kernel is dead: from then on every submit / wait on this server fails at once
 * with DANN_EHIP until dann_server_stop + dann_server_start.  The resident kernel leaves after idle_timeout_us
 * without a submission (default 100 ms), and after 200 ms of residence under a steady stream of submissions, and is
 * relaunched by the next submit, wait or poll: a device-wide synchronisation elsewhere in the process (every hipFree is
 * one -- dann_index_destroy of another index, for instance) waits at most that long on this server.  Row lengths must be a multiple
 * of 16 bytes; L + start points <= 256. */
typedef struct {
    uint32_t l_value;
    uint32_t k;
    uint32_t workers;          /* searches in flight on the device (wavefronts), e.g. 1024 */
    uint32_t ring;             /* ring entries (rounded up to a power of two); 0 = 4 * workers */
    uint32_t idle_timeout_us;  /* 0 = 100000 */
} dann_server_config;
int32_t dann_server_start(dann_index* idx, const dann_server_config* cfg);
int32_t dann_server_stop(dann_index* idx);  /* also called by dann_index_destroy */
int32_t dann_search_submit(dann_index* idx, const void* query, uint64_t* ticket);
/* 1 = the result of `ticket` has arrived (dann_search_wait will not block), 0 = not yet */
int32_t dann_search_poll(dann_index* idx, uint64_t ticket);
int32_t dann_search_wait(dann_index* idx, uint64_t ticket, uint32_t* out_ids, float* out_dists,
                         dann_search_stats* out_stats);
/* tickets issued so far, relaunches of the resident kernel after an idle exit */
int32_t dann_server_stats(dann_index* idx, uint64_t* submitted, uint64_t* relaunches);

#ifdef __cplusplus
}
#endif
#endif /* DANN_H */
