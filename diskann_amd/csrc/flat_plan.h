// How an exhaustive scan (flat_kernels.hip, dann_flat_search_batch) is cut up: queries into tiles that share each row
// fetch, slots [first, first + n) into chunks that each produce one k-list per query, and the calls' queries into
// batches whose chunk lists fit the scratch.  Sizing only ever affects speed: the result is the first k elements of a
// strict total order, whatever the cut.  No HIP here: tests/test_flat_model_host.py compiles it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dann {

constexpr uint32_t kFlatThreads = 256;      // one workgroup of the scan and of the merge
constexpr uint32_t kFlatMaxK = 1024;
constexpr uint32_t kFlatMaxTile = 8;        // queries that share one pass over a chunk's rows
// most rows a workgroup scores per step (4 lanes a row, 4 rows a lane group): the most keys a step appends to one
// query's candidate buffer
constexpr uint32_t kFlatStepRows = 256;
constexpr uint32_t kFlatMinChunkRows = 1024;  // default sizing: no chunk shorter than four steps
constexpr uint32_t kFlatBlocksPerCu = 8;      // default sizing: workgroups per compute unit the grid aims for
constexpr size_t kFlatLdsBudget = 150 * 1024;  // of the CU's 160 KiB
constexpr size_t kFlatScratchBudget = (size_t)192 << 20;  // bytes of chunk lists per batch of queries
constexpr uint32_t kFlatMaxGridY = 65535;

struct FlatPlan {
    uint32_t k = 0;
    uint32_t tile = 0;        // queries per workgroup (0: a query tile does not fit the LDS)
    uint32_t cap = 0;         // keys of one query's candidate buffer, a power of two >= k + kFlatStepRows
    uint32_t chunk_rows = 0;  // slots per chunk; the last chunk may be shorter
    uint32_t nchunks = 0;
    uint32_t batch = 0;       // queries per launch
    uint32_t merge_cap = 0;   // keys of the merge's buffer, a power of two >= 2 k
    size_t scan_lds = 0, merge_lds = 0;
    // the chunk lists [batch][nchunks][k] and the rows each chunk evaluated
    size_t scratch_bytes() const { return (size_t)batch * nchunks * sizeof(uint64_t) * k + (size_t)nchunks * 4; }
};

constexpr uint32_t flat_pow2_at_least(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// slots of chunk c: [first + c * chunk_rows, min(first + (c + 1) * chunk_rows, first + n))
constexpr uint64_t flat_chunk_lo(const FlatPlan& p, uint32_t first, uint32_t c) { return (uint64_t)first + (uint64_t)c * p.chunk_rows; }
constexpr uint64_t flat_chunk_hi(const FlatPlan& p, uint32_t first, uint32_t n, uint32_t c) {
    const uint64_t hi = flat_chunk_lo(p, first, c) + p.chunk_rows, end = (uint64_t)first + n;
    return hi < end ? hi : end;
}

// qslot: bytes of one staged query in LDS (a multiple of 16).  forced_chunk_rows: DANN_DBG_FLAT_CHUNK_ROWS, 0 = default.
inline FlatPlan flat_plan(uint32_t n, uint32_t nq, uint32_t k, uint32_t qslot, uint32_t num_cus, uint32_t forced_chunk_rows) {
    FlatPlan p;
    p.k = k;
    if (n == 0 || nq == 0 || k == 0 || k > kFlatMaxK) return p;
    p.cap = flat_pow2_at_least(k + kFlatStepRows);
    p.merge_cap = flat_pow2_at_least(2 * k < 1024 ? 1024 : 2 * k);
    // per query in LDS: the staged query, the candidate buffer, its fill count and its threshold key
    const size_t per_query = (size_t)qslot + (size_t)p.cap * 8 + 16;
    uint32_t tile = kFlatMaxTile;
    while (tile > 1 && (tile / 2 >= nq || per_query * tile > kFlatLdsBudget)) tile >>= 1;
    if (per_query * tile > kFlatLdsBudget) return p;
    p.tile = tile;
    p.scan_lds = per_query * tile + 16;
    p.merge_lds = (size_t)p.merge_cap * 8 + qslot;
    if (p.merge_lds > kFlatLdsBudget) {
        p.tile = 0;
        return p;
    }
    const uint32_t tiles_all = (nq + tile - 1) / tile;
    uint32_t rows = forced_chunk_rows;
    if (rows == 0) {
        // chunks x query tiles ~ kFlatBlocksPerCu workgroups per compute unit
        const uint64_t want_blocks = (uint64_t)(num_cus ? num_cus : 256u) * kFlatBlocksPerCu;
        const uint64_t want_chunks = (want_blocks + tiles_all - 1) / tiles_all;
        const uint64_t r = ((uint64_t)n + want_chunks - 1) / want_chunks;
        rows = r < kFlatMinChunkRows ? kFlatMinChunkRows : (uint32_t)r;
        rows = (rows + kFlatStepRows - 1) / kFlatStepRows * kFlatStepRows;
    }
    p.chunk_rows = rows;
    p.nchunks = (uint32_t)(((uint64_t)n + rows - 1) / rows);
    // queries per launch: whole tiles, within the scratch budget and the grid's second dimension
    const size_t per_query_scratch = (size_t)p.nchunks * k * 8;
    uint64_t batch = kFlatScratchBudget / per_query_scratch;
    batch = batch / tile * tile;
    if (batch < tile) batch = tile;
    if (batch > (uint64_t)kFlatMaxGridY * tile) batch = (uint64_t)kFlatMaxGridY * tile;
    if (batch > nq) batch = nq;
    p.batch = (uint32_t)batch;
    return p;
}

}  // namespace dann
