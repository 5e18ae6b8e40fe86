// How the filtered and the range exhaustive scans (flat_gt_kernels.hip, dann_flat_filtered_search_batch,
// dann_flat_range_search_batch) are cut up.  Both tile like the k-NN scan of flat_plan.h -- a workgroup owns a tile of
// queries x a chunk of slots -- and add a work list in LDS: the chunk's bitmap words, kFlatGtSegRows slots at a time,
// become the ascending list of the slots the tile visits, and steps walk that list.  As in flat_plan.h the sizing only
// ever affects speed.  No HIP here: tests/test_flat_gt_model_host.py compiles it with g++.
#pragma once
#include "flat_plan.h"

namespace dann {

constexpr uint32_t kFlatGtSegWords = 128;                    // bitmap words one list build takes: a word a thread
constexpr uint32_t kFlatGtSegRows = kFlatGtSegWords * 32;
// a build appends at most kFlatGtSegRows slots behind the fewer than kFlatStepRows that the steps left over
constexpr uint32_t kFlatGtListCap = kFlatGtSegRows + kFlatStepRows;
// the list in LDS: a slot id and the tile's accept mask (a bit a query) per entry, behind a 64-byte header (the
// wavefronts' scan sums and what a build reads of the chunk and the filter)
constexpr size_t kFlatGtListBytes = (size_t)kFlatGtListCap * 5 + 64;
static_assert(kFlatMaxTile <= 8, "an entry's accept mask is a byte");

// ---- filtered k-NN: the plan of flat_plan.h with the list next to the candidate buffers, and a cmps count per
// (query, chunk) behind the chunk lists
struct FlatFilteredPlan {
    FlatPlan p;  // p.tile == 0: does not fit the LDS; p.scan_lds includes the list
    size_t scratch_bytes() const { return (size_t)p.batch * p.nchunks * ((size_t)p.k * 8 + 4); }
};

inline FlatFilteredPlan flat_filtered_plan(uint32_t n, uint32_t nq, uint32_t k, uint32_t qslot, uint32_t num_cus,
                                           uint32_t forced_chunk_rows) {
    FlatFilteredPlan f;
    f.p = flat_plan(n, nq, k, qslot, num_cus, forced_chunk_rows);
    FlatPlan& p = f.p;
    if (p.tile == 0) return f;
    const size_t per_query = (size_t)qslot + (size_t)p.cap * 8 + 16;
    while (p.tile > 1 && per_query * p.tile + kFlatGtListBytes > kFlatLdsBudget) p.tile >>= 1;
    if (per_query * p.tile + kFlatGtListBytes > kFlatLdsBudget) {
        p.tile = 0;
        return f;
    }
    p.scan_lds = per_query * p.tile + kFlatGtListBytes;
    // queries per launch: whole tiles, within the scratch budget and the grid's second dimension
    const size_t per_query_scratch = (size_t)p.nchunks * ((size_t)k * 8 + 4);
    uint64_t batch = kFlatScratchBudget / per_query_scratch;
    batch = batch / p.tile * p.tile;
    if (batch < p.tile) batch = p.tile;
    if (batch > (uint64_t)kFlatMaxGridY * p.tile) batch = (uint64_t)kFlatMaxGridY * p.tile;
    if (batch > nq) batch = nq;
    p.batch = (uint32_t)batch;
    return f;
}

// ---- range: a count pass leaves matches and rows evaluated per (query, chunk); an exclusive scan over a query's chunks
// turns the counts into the places where the write pass, which scores the rows again, puts each chunk's matches
struct FlatRangePlan {
    uint32_t tile = 0;  // queries per workgroup (0: a query tile does not fit the LDS)
    uint32_t chunk_rows = 0, nchunks = 0;
    uint32_t batch = 0;  // queries per launch
    size_t lds = 0;
    // per (query, chunk): matches (then: the offset of the chunk's first match) and rows evaluated; and the overflow flag
    size_t scratch_bytes() const { return (size_t)batch * nchunks * 8 + 16; }
};

// the word behind the counts that says whether any query of the call had more matches than out_cap
inline uint32_t* flat_range_overflow_flag(const FlatRangePlan& p, void* scratch) {
    return static_cast<uint32_t*>(scratch) + (size_t)p.batch * p.nchunks * 2;
}

// per query in LDS: the staged query, a step's matched distances in row order, and 8 words of counters
constexpr size_t flat_range_lds_per_query(uint32_t qslot) { return (size_t)qslot + (size_t)kFlatStepRows * 4 + 32; }

inline FlatRangePlan flat_range_plan(uint32_t n, uint32_t nq, uint32_t qslot, uint32_t num_cus, uint32_t forced_chunk_rows) {
    FlatRangePlan p;
    if (nq == 0) return p;
    const size_t per_query = flat_range_lds_per_query(qslot);
    uint32_t tile = kFlatMaxTile;
    while (tile > 1 && (tile / 2 >= nq || per_query * tile + kFlatGtListBytes > kFlatLdsBudget)) tile >>= 1;
    if (per_query * tile + kFlatGtListBytes > kFlatLdsBudget) return p;
    p.tile = tile;
    p.lds = per_query * tile + kFlatGtListBytes;
    const uint32_t tiles_all = (nq + tile - 1) / tile;
    uint32_t rows = forced_chunk_rows;
    if (rows == 0) {
        const uint64_t want_blocks = (uint64_t)(num_cus ? num_cus : 256u) * kFlatBlocksPerCu;
        const uint64_t want_chunks = (want_blocks + tiles_all - 1) / tiles_all;
        const uint64_t r = ((uint64_t)n + want_chunks - 1) / want_chunks;
        rows = r < kFlatMinChunkRows ? kFlatMinChunkRows : (uint32_t)r;
        rows = (rows + kFlatStepRows - 1) / kFlatStepRows * kFlatStepRows;
    }
    p.chunk_rows = rows;
    p.nchunks = (uint32_t)(((uint64_t)n + rows - 1) / rows);  // (n == 0: no chunk, every result is empty)
    const size_t per_query_scratch = (size_t)(p.nchunks ? p.nchunks : 1) * 8;
    uint64_t batch = kFlatScratchBudget / per_query_scratch;
    batch = batch / tile * tile;
    if (batch < tile) batch = tile;
    if (batch > (uint64_t)kFlatMaxGridY * tile) batch = (uint64_t)kFlatMaxGridY * tile;
    if (batch > nq) batch = nq;
    p.batch = (uint32_t)batch;
    return p;
}

// The offsets of a query's chunks: flat_range_offsets_kernel cuts the nchunks counts into kFlatThreads runs of
// flat_range_run_chunks(nchunks) chunks, sums every run, scans the run sums exclusively, and scans every run in place from
// its sum on.  Both scans are this function (on the device and, for the test of the header, on the host): counts[0, n)
// become the number of matches in front of each, starting at `run`; the return value is the number behind the last.
constexpr uint32_t flat_range_run_chunks(uint32_t nchunks) { return (nchunks + kFlatThreads - 1) / kFlatThreads; }
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint32_t flat_range_exclusive_scan(uint32_t* counts, uint32_t n, uint32_t run) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t x = counts[i];
        counts[i] = run;
        run += x;
    }
    return run;
}

// ---- host-pointer forms: per-query bitmaps and result places staged at a time (a set of per-query bitmaps can be
// gigabytes: never staged whole)
constexpr size_t kFlatFilterStageBytes = (size_t)64 << 20;

// queries per piece of a host-pointer call: at most 65536, kFlatFilterStageBytes of per-query bitmaps (stride_words words
// each, 0: a shared bitmap) and of result places (out_cap ids and as many distances each, 0: none), and at least one
inline uint32_t flat_host_piece(uint32_t nq, uint64_t stride_words, uint32_t out_cap) {
    uint64_t piece = nq < 65536u ? nq : 65536u;
    if (stride_words && piece > kFlatFilterStageBytes / (stride_words * 4)) piece = kFlatFilterStageBytes / (stride_words * 4);
    if (out_cap && piece > kFlatFilterStageBytes / ((uint64_t)out_cap * 4)) piece = kFlatFilterStageBytes / ((uint64_t)out_cap * 4);
    return piece ? (uint32_t)piece : 1u;
}

}  // namespace dann
