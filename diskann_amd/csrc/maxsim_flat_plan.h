// How the exhaustive multi-vector scan (maxsim_flat_kernels.hip, dann_mv_flat_search_batch) is cut up.  A set keeps all
// documents' rows in one CSR array, so the work is cut by ROWS: chunk c is rows [c * chunk_rows, (c + 1) * chunk_rows) of
// the scanned range, counted from the range's first row, and a document belongs to the chunk that holds its first row (a
// document without rows: the chunk of its offset; offsets at the range's very end: the last chunk).  A workgroup walks
// its chunk's documents in windows of at most kMvFlatWindowDocs, and leaves one k-list per (query, chunk).  Sizing only
// ever affects speed: the result is the first k elements of a strict total order, whatever the cut.  No HIP here:
// tests/test_mv_flat_model_host.py compiles it with g++.
#pragma once
#include "flat_plan.h"

namespace dann {

constexpr uint32_t kMvFlatThreads = 256;       // four wavefronts: one 32-row query tile each
constexpr uint32_t kMvFlatTileRows = 32;       // set rows of one MFMA tile
constexpr uint32_t kMvFlatGroupRows = 128;     // query rows of one walk over a window: four tiles
constexpr uint32_t kMvFlatWindowDocs = 256;    // documents whose offsets and running aggregates sit in LDS at a time
constexpr uint32_t kMvFlatMinChunkRows = 1024; // default sizing: no chunk shorter than 32 tiles
constexpr uint32_t kMvFlatBlocksPerCu = 8;     // default sizing: workgroups per compute unit the grid aims for

struct MvFlatPlan {
    uint32_t k = 0;
    uint32_t cap = 0;          // keys of the candidate buffer, a power of two >= k + kMvFlatWindowDocs
    uint64_t chunk_rows = 0;   // rows per chunk, a multiple of kMvFlatTileRows
    uint32_t nchunks = 0;      // >= 1 when there is a document to scan
    uint32_t batch = 0;        // queries per launch
    uint32_t merge_cap = 0;    // keys of the merge's buffer, a power of two >= 2 k
    size_t merge_lds = 0;
    size_t list_bytes() const { return (size_t)batch * nchunks * sizeof(uint64_t) * k; }
    // the chunk lists [batch][nchunks][k] and the documents every (query, chunk) evaluated
    size_t scratch_bytes() const { return list_bytes() + (size_t)batch * nchunks * 4; }
};

// the chunk of a document whose first row is `rel` rows behind the range's first row
constexpr uint32_t mv_flat_chunk_of(uint64_t rel, uint64_t chunk_rows, uint32_t nchunks) {
    const uint64_t c = rel / chunk_rows;
    return c < nchunks ? (uint32_t)c : nchunks - 1u;
}

// the first document d of [first, first + n] with row_offsets[d] - row_offsets[first] >= rel (first + n if there is none)
constexpr uint32_t mv_flat_lower_doc(const uint64_t* row_offsets, uint32_t first, uint32_t n, uint64_t rel) {
    const uint64_t want = row_offsets[first] + rel;
    uint32_t lo = first, hi = first + n;  // (the answer is in [lo, hi])
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (row_offsets[mid] < want) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// the documents [*dlo, *dhi) of chunk c: those of [first, first + n) whose mv_flat_chunk_of is c
constexpr void mv_flat_chunk_docs(const uint64_t* row_offsets, uint32_t first, uint32_t n, uint64_t chunk_rows, uint32_t nchunks,
                                  uint32_t c, uint32_t* dlo, uint32_t* dhi) {
    *dlo = c == 0 ? first : mv_flat_lower_doc(row_offsets, first, n, (uint64_t)c * chunk_rows);
    *dhi = c + 1u >= nchunks ? first + n : mv_flat_lower_doc(row_offsets, first, n, (uint64_t)(c + 1u) * chunk_rows);
}

// rows: the rows of the scanned documents.  forced_chunk_rows: 0 = default (rounded up to whole tiles otherwise).
inline MvFlatPlan mv_flat_plan(uint64_t rows, uint32_t ndocs, uint32_t nq, uint32_t k, uint32_t num_cus, uint64_t forced_chunk_rows) {
    MvFlatPlan p;
    p.k = k;
    if (ndocs == 0 || nq == 0 || k == 0 || k > kFlatMaxK) return p;
    p.cap = flat_pow2_at_least(k + kMvFlatWindowDocs);
    p.merge_cap = flat_pow2_at_least(2 * k < 1024 ? 1024 : 2 * k);
    p.merge_lds = (size_t)p.merge_cap * 8;
    uint64_t cr = forced_chunk_rows;
    if (cr == 0) {
        // chunks x queries ~ kMvFlatBlocksPerCu workgroups per compute unit
        const uint64_t want_blocks = (uint64_t)(num_cus ? num_cus : 256u) * kMvFlatBlocksPerCu;
        const uint64_t want_chunks = (want_blocks + nq - 1) / nq;
        cr = (rows + want_chunks - 1) / want_chunks;
        if (cr < kMvFlatMinChunkRows) cr = kMvFlatMinChunkRows;
    }
    cr = (cr + kMvFlatTileRows - 1) / kMvFlatTileRows * kMvFlatTileRows;
    // (documents without rows add no chunk: at most one chunk per scanned document keeps the grid's first dimension small)
    uint64_t nch = (rows + cr - 1) / cr;
    if (nch > ndocs) {
        cr = ((rows + ndocs - 1) / ndocs + kMvFlatTileRows - 1) / kMvFlatTileRows * kMvFlatTileRows;
        nch = (rows + cr - 1) / cr;
    }
    p.chunk_rows = cr;
    p.nchunks = nch ? (uint32_t)nch : 1u;
    const size_t per_query_scratch = (size_t)p.nchunks * ((size_t)k * 8 + 4);
    uint64_t batch = kFlatScratchBudget / per_query_scratch;
    if (batch < 1) batch = 1;
    if (batch > kFlatMaxGridY) batch = kFlatMaxGridY;
    if (batch > nq) batch = nq;
    p.batch = (uint32_t)batch;
    return p;
}

}  // namespace dann
