// How the exhaustive scan over PQ code rows (flat_pq_kernels.hip, dann_pq_linear_search_batch) is cut up.  It tiles like
// the k-NN scan of flat_plan.h -- a workgroup owns a tile of queries x a chunk of slots and leaves one k-list per query --
// but what a tile keeps in LDS is not its queries: it is their lookup tables, `chunks` KiB each, interleaved over the tile.
// The tables are built once per query by a kernel of their own and staged by every workgroup, so a slot chunk is long
// enough to pay for the staging.  As in flat_plan.h the sizing only ever affects speed.  No HIP here:
// tests/test_pq_linear_model_host.py compiles it with g++.
#pragma once
#include "flat_plan.h"

namespace dann {

constexpr uint32_t kFlatPqMaxChunks = 128;       // PQ chunks of a code row (dann_create's limit)
constexpr uint32_t kFlatPqTableBytes = 1024;     // one chunk of one query's table: 256 f32
// One workgroup of the scan: eight wavefronts share a tile's tables (a tile fills most of a CU's LDS, so one workgroup is
// resident and its size is the CU's occupancy), sixteen when the query tiles alone fill the device and the wider step's
// candidate buffers leave the tile as it is (measured: DESIGN.md 3.20.2).  The merge keeps kFlatThreads.
constexpr uint32_t kFlatPqThreads = 512;
constexpr uint32_t kFlatPqWideThreads = 1024;
// default sizing: staging a table costs a workgroup about as much as 256 rows; no chunk shorter than 4096
constexpr uint32_t kFlatPqMinChunkRows = 4096;
constexpr uint32_t kFlatPqBlocksPerCu = 2;  // (a tile's tables fill most of a CU's LDS: one or two workgroups are resident)

struct FlatPqPlan {
    uint32_t k = 0;
    uint32_t chunks = 0;      // PQ chunks
    uint32_t tile = 0;        // queries per workgroup: 8, 4, 2 or 1 (0: nothing to scan)
    uint32_t threads = 0;     // of a scan workgroup; lane = row: the rows of a step, the most keys it appends to a buffer
    uint32_t cap = 0;         // keys of one query's candidate buffer, a power of two >= k + threads
    uint32_t chunk_rows = 0;  // slots per chunk; the last chunk may be shorter
    uint32_t nchunks = 0;     // slot chunks
    uint32_t batch = 0;       // queries per launch
    uint32_t merge_cap = 0;   // keys of the merge's buffer, a power of two >= 2 k
    size_t scan_lds = 0, merge_lds = 0;
    // per launch: the tables [batch][chunks][256] f32, the chunk lists [batch][nchunks][k] and the rows every
    // (query, chunk) evaluated
    size_t table_bytes() const { return (size_t)batch * chunks * kFlatPqTableBytes; }
    size_t list_bytes() const { return (size_t)batch * nchunks * sizeof(uint64_t) * k; }
    size_t scratch_bytes() const { return table_bytes() + list_bytes() + (size_t)batch * nchunks * 4; }
};

// per query in LDS: its table, the candidate buffer, its threshold key, its fill count and its rows evaluated
constexpr size_t flat_pq_lds_per_query(uint32_t chunks, uint32_t cap) {
    return (size_t)chunks * kFlatPqTableBytes + (size_t)cap * 8 + 16;
}

// slots of chunk c: [first + c * chunk_rows, min(first + (c + 1) * chunk_rows, first + n))
constexpr uint64_t flat_pq_chunk_lo(const FlatPqPlan& p, uint32_t first, uint32_t c) {
    return (uint64_t)first + (uint64_t)c * p.chunk_rows;
}
constexpr uint64_t flat_pq_chunk_hi(const FlatPqPlan& p, uint32_t first, uint32_t n, uint32_t c) {
    const uint64_t hi = flat_pq_chunk_lo(p, first, c) + p.chunk_rows, end = (uint64_t)first + n;
    return hi < end ? hi : end;
}

// chunks: 1 .. kFlatPqMaxChunks.  forced_chunk_rows: DANN_DBG_FLAT_CHUNK_ROWS, 0 = default.
inline FlatPqPlan flat_pq_plan(uint32_t chunks, uint32_t n, uint32_t nq, uint32_t k, uint32_t num_cus,
                               uint32_t forced_chunk_rows) {
    FlatPqPlan p;
    p.k = k;
    p.chunks = chunks;
    if (n == 0 || nq == 0 || k == 0 || k > kFlatMaxK || chunks == 0 || chunks > kFlatPqMaxChunks) return p;
    p.merge_cap = flat_pow2_at_least(2 * k < 1024 ? 1024 : 2 * k);
    // the largest tile of 8 / 4 / 2 / 1 that fits the budget and is useful for nq, at a workgroup of `threads`
    // (tile 1 at 128 chunks and k = 1024: 128 KiB + 16 KiB + 16 bytes)
    static_assert(flat_pq_lds_per_query(kFlatPqMaxChunks, flat_pow2_at_least(kFlatMaxK + kFlatPqWideThreads)) <= kFlatLdsBudget,
                  "every accepted shape has a tile");
    const auto tile_at = [&](uint32_t threads) {
        const size_t per_query = flat_pq_lds_per_query(chunks, flat_pow2_at_least(k + threads));
        uint32_t t = kFlatMaxTile;
        while (t > 1 && (t / 2 >= nq || per_query * t > kFlatLdsBudget)) t >>= 1;
        return t;
    };
    const uint64_t want_blocks = (uint64_t)(num_cus ? num_cus : 256u) * kFlatPqBlocksPerCu;
    const uint32_t tile = tile_at(kFlatPqThreads);
    p.threads = kFlatPqThreads;
    if ((nq + tile - 1) / tile >= want_blocks && tile_at(kFlatPqWideThreads) == tile) p.threads = kFlatPqWideThreads;
    p.cap = flat_pow2_at_least(k + p.threads);
    p.tile = tile;
    p.scan_lds = flat_pq_lds_per_query(chunks, p.cap) * tile;
    p.merge_lds = (size_t)p.merge_cap * 8;
    const uint32_t tiles_all = (nq + tile - 1) / tile;
    uint32_t rows = forced_chunk_rows;
    if (rows == 0) {
        // chunks x query tiles ~ kFlatPqBlocksPerCu workgroups per compute unit
        const uint64_t want_chunks = (want_blocks + tiles_all - 1) / tiles_all;
        const uint64_t r = ((uint64_t)n + want_chunks - 1) / want_chunks;
        rows = r < kFlatPqMinChunkRows ? kFlatPqMinChunkRows : (uint32_t)r;
        const uint64_t whole = ((uint64_t)rows + p.threads - 1) / p.threads * p.threads;
        if (whole <= 0xFFFFFFFFull) rows = (uint32_t)whole;  // (whole steps, unless that leaves 32 bits)
    }
    p.chunk_rows = rows;
    p.nchunks = (uint32_t)(((uint64_t)n + rows - 1) / rows);
    // queries per launch: whole tiles, within the scratch budget and the grid's second dimension
    const size_t per_query_scratch = (size_t)p.nchunks * ((size_t)k * 8 + 4) + (size_t)chunks * kFlatPqTableBytes;
    uint64_t batch = kFlatScratchBudget / per_query_scratch;
    batch = batch / tile * tile;
    if (batch < tile) batch = tile;
    if (batch > (uint64_t)kFlatMaxGridY * tile) batch = (uint64_t)kFlatMaxGridY * tile;
    if (batch > nq) batch = nq;
    // launches of equal size: a short last launch would leave most of the device idle for a whole pass over the rows
    const uint64_t launches = ((uint64_t)nq + batch - 1) / batch;
    if (launches > 1) batch = (((uint64_t)nq + launches - 1) / launches + tile - 1) / tile * tile;
    p.batch = (uint32_t)batch;
    return p;
}

}  // namespace dann
