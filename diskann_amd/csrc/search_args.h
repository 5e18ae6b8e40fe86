// What a beam-search launch is described by: the device views of the index and of the search server, the kernel
// arguments and the calibration state of the visited table.  Plain data shared by the kernels and the host-side launch
// planning (launch_plan.h).  No HIP here: tests/test_launch_plan_host.py compiles it with g++.
#pragma once
#include <stdint.h>

#include "../../include/dann.h"
#include "../../include/dann_debug.h"

namespace dann {

// Device view of the index, passed by value to kernels.
struct IndexView {
    const uint8_t* rows;   // (capacity + nstart) rows, row_stride bytes apart
    uint32_t* adj;         // (capacity + nstart) x (max_degree + 1) u32: [len, ids...]
    uint64_t row_stride;
    uint32_t adj_stride;   // max_degree + 1
    uint32_t dim;
    uint32_t capacity;
    uint32_t nslots;       // capacity + nstart
    uint32_t max_degree;
    uint32_t nstart;
    int32_t dtype;
    int32_t metric;
    uint32_t layer_bytes;  // bytes of one row's payload (dim * sizeof(T); SQ-8 / SQ4 / SQ1: code bytes + 4; spherical: + 6)
    uint32_t qbytes;       // integer rows: bytes of one query as the kernels read and stage it -- layer_bytes, except under
                           // a spherical query layout (dann_set_query_layout; dtype is then the layout's, see DT_SPH1T)
    float sq_k;            // SQ-8 / SQ4 / SQ1: (1/(2^bits - 1))^2 * scale^2
    float sq_shift_norm_sq;
    // PQ rows (DT_PQ): codes of pq_chunks bytes; pivots 256 x dim f32; chunk offsets pq_chunks + 1
    const float* pq_pivots;
    const uint32_t* pq_offsets;
    uint32_t pq_chunks;
    // PQ rows, packed search layout (dann_pq_pack_neighbors; null = none): node i's row at pq_pack + i * pq_pack_stride =
    // [u32 len][u32 x max_degree neighbour ids][pad to 16][16-byte code row of each neighbour], 64-byte aligned
    const uint8_t* pq_pack;
    uint32_t pq_pack_stride;
    uint32_t pq_pack_codes;  // byte offset of the code rows within a packed row
    // inline concurrency tags (dann_config::inline_tags): byte offset of a row's tag (== layer_bytes), 0 = none.
    // A slot is readable iff tag >= 254 (Tag::can_read, diskann-inmem/src/tag.rs:86-133).
    uint32_t tag_off;
};

// Persistent search server (dann_server_start): device view of the submission ring.  The ring lives in host-mapped,
// fine-grained memory: a caller copies its query into slot (ticket % ring) and publishes it by storing the slot's lap
// number; wave 0 of the kernel (the dispatcher) polls the publication words over PCIe, 64 at a time, and advances
// `avail` in device memory; the worker waves draw tickets from `head`, wait for avail > ticket, stage the query into
// device memory, run the ordinary beam search and write the result plus a completion word back to the host ring.
struct ServerView {
    const uint8_t* h_queries = nullptr;  // host ring: ring x qstride bytes
    const uint32_t* h_pub = nullptr;     // host: submission ring, entry of ticket t at t % ring: lap tag << 20 | result slot
    uint32_t* h_ack = nullptr;           // host: lap tag of the last entry a worker has taken from each ring position
    uint32_t* h_res_ids = nullptr;       // host: ring x k
    float* h_res_d = nullptr;            // host: ring x k
    dann_search_stats* h_res_stats = nullptr;  // host: ring
    uint32_t* h_done = nullptr;          // host: per result slot, low 32 bits of (ticket + 1) once the result is written
    uint32_t* h_ctl = nullptr;           // host: [0] stop request (host -> GPU), [1] the dispatcher has decided to exit
    unsigned long long* d_head = nullptr;   // device: next ticket a worker draws
    unsigned long long* d_avail = nullptr;  // device: tickets below this are published
    uint32_t* d_stop = nullptr;          // device: workers leave when they see it
    uint8_t* d_q = nullptr;              // device: workers x qstride (staged queries)
    uint32_t ring = 0;                   // entries, a power of two
    uint32_t ring_shift = 0;             // log2(ring)
    uint32_t qstride = 0;                // bytes per query slot (multiple of 16)
    uint32_t qbytes = 0;                 // bytes of one query
    uint32_t workers = 0;
    uint32_t ticks_per_us = 100;         // wall_clock64 rate (hipDeviceAttributeWallClockRate)
    uint32_t idle_timeout_us = 100000;   // the kernel leaves after this long without a new submission (a later submit
                                         // relaunches it): a device-wide synchronisation elsewhere in the process must
                                         // not wait for ever on an idle server
    uint32_t max_resident_us = 200000;   // ... nor on a busy one: the kernel also leaves (drains and is relaunched by the
                                         // next submit / wait / poll) once it has been resident this long.  hipFree is a
                                         // device-wide synchronisation: without the bound, destroying another index while
                                         // callers keep this server busy would block until they pause
};

struct SearchArgs {
    IndexView ix;
    const void* queries = nullptr;     // nq rows of layer bytes, or nullptr when `qslots` is used
    const uint32_t* qslots = nullptr;  // insert-time search: query i = stored row qslots[i]
    uint32_t nq = 0;
    uint32_t l_value = 0;
    uint32_t beam_width = 0;
    uint32_t k = 0;
    uint32_t ht_entries = 0;     // per-query LDS visited-table entries (multiple of 64)
    uint32_t ht_prime = 0;       // probing modulus, set by search_with_retry: largest prime <= ht_entries
    // 16-bit table entries (plain-mode kernels, chosen per launch by the host; search_kernel_impl.h, ht16_insert_open):
    // the table holds 2 * ht_entries slots, ht_prime is that slot count
    uint32_t ht16 = 0;
    uint32_t ht_shift = 0;       // 32 - m, m = bits of the index's slot count
    uint32_t ht_tb = 0;          // tag bits: 2^tb >= ceil(2^m / slots)
    uint32_t ht_kmax = 0;        // probes per id
    uint32_t ht_ov = 0;          // pair / PQ-table kernels: words of the overflow table behind the 16-bit table (a power
                                 // of two; 0 = none): it takes the ids whose ht_kmax probes are all taken (ov_insert)
    uint32_t ht_open = 0;        // ids the open table takes before it is frozen (set with ht_prime: 75 % of the 32-bit
                                 // table's prime, 75 % -- DANN_DBG_HT16_OPEN_EIGHTHS -- of the 16-bit table's entries)
    uint32_t* out_ids = nullptr; // nq x k (may be null in record mode)
    float* out_dists = nullptr;
    dann_search_stats* stats = nullptr;
    uint32_t* rec_ids = nullptr; // nq x rec_stride (record mode) or null
    float* rec_dists = nullptr;
    uint32_t rec_stride = 0;
    uint32_t* rec_n = nullptr;
    uint32_t* rec_max = nullptr; // optional: atomicMax of the record lengths of this launch
    // graph::search::Range (null range_ids = plain Knn): scratch list of in-range (id, dist) per query
    uint32_t* range_ids = nullptr;
    float* range_d = nullptr;
    uint32_t* range_second = nullptr;  // per query: did the second round run
    uint32_t range_cap = 0;      // entries per query in range_ids/range_d
    uint32_t range_max = 0;      // max_returned (0xFFFFFFFF = unlimited)
    uint32_t range_thresh = 0;   // (starting_l as f32 * initial_slack) as usize
    uint32_t has_inner = 0;
    float radius = 0.f, inner_radius = 0.f, range_slack = 1.f;
    uint32_t* spill = nullptr;       // pool of global-memory visited tables (all kEmpty between launches)
    uint32_t* spill_next = nullptr;  // pool allocation counter (zeroed before each launch)
    uint32_t spill_slices = 0;
    uint32_t spill_bits = 0;         // log2 entries per slice
    uint32_t* fail_flag = nullptr;   // set non-zero by any query that exhausts its scratch
    const uint32_t* qmap = nullptr;  // optional: process queries qmap[0..nq) (retry of overflowed queries)
    // filtered searches (graph/ext/labeled.rs): QueryLabelProvider == bitmap over slot ids
    uint32_t filter_mode = 0;        // 0 none, DANN_FILTER_INLINE, DANN_FILTER_MULTIHOP
    const uint32_t* filter = nullptr;
    uint64_t filter_stride = 0;      // words between the bitmaps of consecutive queries (0 = shared)
    uint32_t* m_ids = nullptr;       // inline: matched_results per query in push order (nq x m_cap)
    float* m_d = nullptr;
    uint32_t m_cap = 0;
    unsigned long long* m_keys = nullptr;  // sort scratch, nq x key_cap (key_cap a power of two)
    uint32_t key_cap = 0;
    // DANN_TIE_RUST: lists with equal distances are ordered as Rust's sort_unstable_by leaves them (rust_order.h); per
    // query kTieWorkBytes of scratch: 64 keys of a multihop hop + the sorter's work area
    uint8_t* tie_work = nullptr;
    uint32_t ad_samples = 0;         // AdaptiveL::sample_count (0 = none)
    const uint32_t* ad_table = nullptr;  // new L for (visited - ad_samples, matched): row stride ad_stride
    uint32_t ad_stride = 0;
    unsigned long long* phase_cycles = nullptr;  // -DDANN_PHASE_CYCLES builds only
    uint32_t qcap_max = 0;           // largest queue capacity an adaptive resize can ask for (0 = l_value + nstart)
    uint32_t tune = 0;               // kTune* bits, chosen per launch by search_with_retry (never affect results)
    uint32_t grid = 0;               // 0: one wave per query; else `grid` persistent waves share the nq queries through
    uint32_t* work_next = nullptr;   //    this counter (zeroed before the launch): dann_set_max_concurrency
    ServerView srv;                  // srv.ring != 0: the launch is the persistent server (grid = workers + 1 waves)
    uint32_t team = 0;               // 1: several wavefronts per query (latency regime; plain fixed-length searches only)
    uint32_t pqlut = 0;              // 1: PQ rows through pq_search_kernel (search_pq_impl.h: lookup table in registers, 16-bit
                                     //    visited table; plain Knn, <= 64 chunks, L + start points <= 256)
    uint32_t pair = 0;               // 1: two queries per wavefront (search_pair_impl.h; 128-byte integer rows, L + start
                                     //    points <= 96, degree <= 64); ht_entries = table words of ONE query then
};

// per (L, beam, mode) sizing state of the LDS visited table: cap_ids = 90th percentile of the
// comparisons per query seen in earlier launches (0 = none yet, use the prior)
struct VisitedCalib {
    uint32_t cap_ids = 0;
    uint64_t calls = 0;
    uint32_t waves = 0;  // occupancy the kernel's VGPRs allow (queries per CU); the table never costs more than that
};

}  // namespace dann
