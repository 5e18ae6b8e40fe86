// maxsim_flat_kernels.hip -- exhaustive multi-vector k-NN: the reference's compute_multivec_ground_truth_from_data
// (diskann-tools/src/utils/ground_truth.rs:696-787) for a batch of queries, dann_mv_flat_search_batch.
//
// Every document of [first, first + n) is scored against the query -- MaxSim per query row, in the order the caller
// chose (maxsim_kernels.hip), then Chamfer / AvgOfMins / MinPairwise over the query's rows -- and goes, in ascending id
// order, through NeighborPriorityQueue::insert on a queue of k entries: the first k non-NaN documents under the strict
// total order of flat_kernels.hip, the key dist_key(d, ~doc).  A strict order has one answer whatever the cut.
//
// The set's rows are ONE CSR array, so a query against the whole set is one dense product Q . Rows^T followed by a
// maximum segmented by document.  Grid = (row chunks, queries), maxsim_flat_plan.h; a workgroup walks its chunk's
// documents in windows of kMvFlatWindowDocs (their offsets, filter bits and running aggregates in LDS) and each window's
// rows 32 at a time, ACROSS document boundaries:
//
//   mvflat_mfma_kernel<RT, KS>  kernel order, on the matrix cores.  Wavefront w owns the 32-row query tile w of a group of
//       four (a query of more than 128 rows walks the window once per group).  KS > 0 (dim <= 2 KS <= 128): the query
//       tile is KS registers of MFMA B operands; the set's 32-row tiles pass through two LDS slabs -- the requests of
//       tile t + 1 are in flight while tile t is multiplied, one barrier per tile.  KS == 0: 128-k slabs of both operands
//       are staged in turn while one accumulator set runs through the whole row.  v_mfma_f32_32x32x2_f32 leaves lane l
//       with 16 set rows of ONE query row; the maximum is taken per segment of the tile (a segment: the tile's rows of
//       one document), a document that goes on into the next tile keeps its running maximum in the lane, one that ends
//       writes -max to the cell [segment][query row] of the tile.  A wavefront without a tile of its own then folds a finished document's cells,
//       in query-row order, into the document's running aggregate.
//   mvflat_rows_kernel<DT>      reference order, deliberately plain: a lane group per document walks the query's rows
//       and the document's rows with the pair function (group_distance_rows), as maxsim_rows_kernel does.
//   mvflat_merge_kernel         flat_merge_rounds over a query's chunk lists, then ids, distances, padding, statistics.
//
// A key folds -0.0 into +0.0.  Chamfer and AvgOfMins are sums from +0.0 and never -0.0; a MinPairwise distance can be,
// and such a document sets its bit in a per-query bitmap that the merge reads back.
#include <float.h>

#include "flat_impl.h"
#include "maxsim_flat_plan.h"
#include "maxsim_stage.h"

namespace dann {
namespace {

constexpr uint32_t kT = kMvFlatThreads, kW = kMvFlatWindowDocs;
constexpr uint32_t kCellStride = kMvFlatGroupRows + 1u;  // (a fold lane walks one segment's cells: odd stride, no conflicts)
constexpr uint32_t kCellFloats = 32u * kCellStride;
constexpr uint32_t kMetaWords = 72;  // [0] live [1] segments [3] rows [4 .. 36] segment starts, the rows behind the last
                                     // [37 .. 68] window slot of the segment's document | ends-in-this-tile << 31
constexpr uint32_t kEndsBit = 0x80000000u;

// LDS of a scan workgroup: every piece at a constant offset from the base, the candidate keys last (their number is the
// only size a launch decides).  Bytes: offsets 8 (kW + 1) | thr 8 | aggregates 4 kW | accepted 4 kW | meta 3 x 288 |
// cnt 4, cmps 4, padding 8 | cells 2 x 16512 | slabs: 2 x 16384 (KS > 0), 5 x 16384 (KS == 0) | keys 8 cap.  The rows
// kernel has neither cells nor slabs.
struct MvfLds {
    uint64_t* keys;
    uint64_t* woff;
    float* agg;
    uint32_t* wacc;
    uint32_t* meta;
    uint64_t* thr;
    uint32_t* cnt;
    uint32_t* cmps;
    float* cells;
    float* slab;
};
constexpr size_t kMvfFixedBytes = 8 * (kW + 1) + 8 + 4 * kW + 4 * kW + 3 * 4 * kMetaWords + 16;
static_assert(kMvfFixedBytes % 16 == 0, "the cells and slabs start on a 16-byte boundary");
constexpr size_t mvf_keys_offset(uint32_t slabs) {
    return kMvfFixedBytes + (slabs ? 2 * 4 * kCellFloats + (size_t)slabs * 4 * kMsSlabFloats : 0);
}
constexpr size_t mvf_lds_bytes(uint32_t cap, uint32_t slabs) { return mvf_keys_offset(slabs) + (size_t)cap * 8; }
static_assert(mvf_lds_bytes(2048, 5) <= kFlatLdsBudget, "the largest scan workgroup fits the LDS");

template <uint32_t SLABS>
__device__ __forceinline__ MvfLds mvf_carve(uint8_t* smem) {
    MvfLds l;
    l.woff = reinterpret_cast<uint64_t*>(smem);
    l.thr = l.woff + (kW + 1);
    l.agg = reinterpret_cast<float*>(l.thr + 1);
    l.wacc = reinterpret_cast<uint32_t*>(l.agg + kW);
    l.meta = l.wacc + kW;
    l.cnt = l.meta + 3 * kMetaWords;
    l.cmps = l.cnt + 1;
    l.cells = reinterpret_cast<float*>(l.cmps + 3);  // (two words of padding: kMvfFixedBytes)
    l.slab = l.cells + 2 * kCellFloats;
    l.keys = reinterpret_cast<uint64_t*>(smem + mvf_keys_offset(SLABS));
    return l;
}
struct MvFlatArgs {
    const uint8_t* drows;     // the set's rows, `stride` bytes apart
    const uint64_t* doff;     // ndocs + 1 row offsets
    const uint8_t* qrows;     // the call's query rows, at the same stride
    const uint32_t* qoff;     // this launch's queries: nq + 1 offsets into qrows
    uint32_t dim, stride;
    uint32_t nq, first, n, k;
    int32_t aggregation;
    uint32_t nchunks;
    uint64_t chunk_rows;
    uint32_t cap, merge_cap;
    const uint32_t* fbits;    // the filter's bitmaps over document ids (null: every document), fstride words apart
    uint64_t fstride;
    uint32_t* negzero;        // DANN_MV_MIN_PAIRWISE: [nq][nz_words] bitmaps of the documents whose distance is -0.0
    uint32_t nz_words;
    uint64_t* lists;          // [nq][nchunks][k] keys, ascending, kFlatNoKey behind the last
    uint32_t* chunk_cmps;     // [nq][nchunks] documents evaluated
    uint32_t* out_ids;
    float* out_dists;
    dann_search_stats* stats;  // may be null
};

// The launch's arguments read again from the kernel-argument segment, behind a barrier the compiler cannot see through:
// what only the finish of a window and the end of the workgroup need (lists, counts, k, cap ...) is then loaded there,
// not kept in scalar registers across the tile loop.
__device__ __forceinline__ const MvFlatArgs& mvf_late_args() {
    const void* p = (const void*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *static_cast<const MvFlatArgs*>(p);
}

// ---- what both scans share: the workgroup's chunk, a window's documents, the finish of a window, the chunk's list ------
struct MvfBlock {
    uint32_t qn, dlo, dhi;
    const uint8_t* q;      // the query's first row
};  // (the chunk is blockIdx.x, the query blockIdx.y: what the ends of a window need of them is derived there)

__device__ __forceinline__ MvfBlock mvf_block(const MvFlatArgs& a, const MvfLds& l) {
    MvfBlock b;
    const uint32_t q0 = a.qoff[blockIdx.y];
    b.qn = a.qoff[blockIdx.y + 1] - q0;
    b.q = a.qrows + (uint64_t)q0 * a.stride;
    mv_flat_chunk_docs(a.doff, a.first, a.n, a.chunk_rows, a.nchunks, blockIdx.x, &b.dlo, &b.dhi);
    if (threadIdx.x == 0) {
        *l.thr = kFlatNoKey;
        *l.cnt = 0;
        *l.cmps = 0;
    }
    return b;
}

// the offsets, filter bits and fresh aggregates of documents [w0, w0 + wn); between two barriers
__device__ __forceinline__ void mvf_window_load(const MvfBlock& b, const MvfLds& l, uint32_t w0, uint32_t wn) {
    __syncthreads();
    const MvFlatArgs& a = mvf_late_args();
    const uint32_t* const fb = a.fbits ? a.fbits + (uint64_t)blockIdx.y * a.fstride : nullptr;
    for (uint32_t i = threadIdx.x; i <= wn; i += kT) l.woff[i] = a.doff[w0 + i];
    for (uint32_t i = threadIdx.x; i < wn; i += kT) {
        const uint32_t doc = w0 + i;
        l.wacc[i] = fb ? (fb[doc >> 5] >> (doc & 31u)) & 1u : 1u;
        l.agg[i] = a.aggregation == DANN_MV_MIN_PAIRWISE ? FLT_MAX : 0.0f;
    }
    __syncthreads();
}

// one more per-row score of a document: Chamfer::evaluate's and AvgOfMins' sequential sum, MinPairwise's minimum
__device__ __forceinline__ float mvf_fold(int32_t aggregation, float x, float score) {
    if (aggregation == DANN_MV_MIN_PAIRWISE) return score < x ? score : x;
    return x + score;
}

// A window's documents become keys: one lane per document, in id order within the wavefront's append.  Ends with a barrier.
__device__ __forceinline__ void mvf_window_finish(const MvfBlock& b, const MvfLds& l, uint32_t w0, uint32_t wn) {
    __syncthreads();
    const MvFlatArgs& a = mvf_late_args();
    static_assert(kW == kT, "one lane per document of a window");
    const uint32_t j = threadIdx.x, doc = w0 + j;
    const bool ok = j < wn && l.wacc[j] != 0u;
    float d = 0.0f;
    if (ok) {
        if (l.woff[j + 1] == l.woff[j]) {  // no rows: f32::MAX in every row, and Chamfer's callback never runs
            if (a.aggregation == DANN_MV_AVG_OF_MINS) {
                for (uint32_t i = 0; i < b.qn; ++i) d = d + FLT_MAX;
                d = d / (float)b.qn;
            } else if (a.aggregation == DANN_MV_MIN_PAIRWISE) {
                d = FLT_MAX;
            }
        } else {
            d = l.agg[j];
            if (a.aggregation == DANN_MV_AVG_OF_MINS) d = d / (float)b.qn;
        }
    }
    const uint64_t okm = ballot64(ok);
    const uint64_t key = dist_key(d, ~doc);
    const bool push = ok && d == d && key < *l.thr;  // (queue.rs: a NaN distance is dropped)
    const uint64_t m = ballot64(push);
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == 0 && okm) atomicAdd(l.cmps, (uint32_t)__popcll(okm));
    if (m) {
        uint32_t base = 0;
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)m) - 1u;
        if (lane == leader) base = atomicAdd(l.cnt, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, (int)leader);
        if (push) {
            l.keys[base + mbcnt(m)] = key;
            // (only a pushed key can reach the merge, so only a pushed document needs its sign kept)
            if (a.negzero && __builtin_bit_cast(uint32_t, d) == 0x80000000u)
                atomicOr(a.negzero + (uint64_t)blockIdx.y * a.nz_words + (doc >> 5), 1u << (doc & 31u));
        }
    }
    __syncthreads();
    const uint32_t fill = *l.cnt;  // (the same for the whole workgroup)
    if (fill + kW > a.cap) flat_cut_to_k<kT>(l.keys, a.cap, fill, a.k, l.cnt, l.thr);
    __syncthreads();
}

// the chunk's best k keys, ascending, kFlatNoKey behind the last; and the documents it evaluated
__device__ __forceinline__ void mvf_block_end(const MvfBlock& b, const MvfLds& l) {
    __syncthreads();
    const MvFlatArgs& a = mvf_late_args();
    const uint32_t fill = *l.cnt;
    flat_cut_to_k<kT>(l.keys, a.cap, fill, a.k, l.cnt, l.thr);
    uint64_t* out = a.lists + ((uint64_t)blockIdx.y * a.nchunks + blockIdx.x) * a.k;
    for (uint32_t i = threadIdx.x; i < a.k; i += kT) out[i] = l.keys[i];  // (cap > k: pads are in place)
    if (threadIdx.x == 0) a.chunk_cmps[(uint64_t)blockIdx.y * a.nchunks + blockIdx.x] = *l.cmps;
}

// ---- kernel order, on the matrix cores ----------------------------------------------------------------------------------
// Tile t of a window: its rows [32 t, 32 t + 32) counted from the window's first row.  The helper wavefront describes it: the
// segments (document boundaries from the window's offsets, one binary search per row), which of them end here, and
// whether any of its documents is accepted -- a tile without one is neither staged nor multiplied.
__device__ __forceinline__ void mvf_meta(uint32_t* m, const MvfLds& l, uint32_t wn, uint32_t t, uint32_t lane) {
    const uint64_t r0 = (uint64_t)t * 32u, wrows = l.woff[wn] - l.woff[0];
    if (r0 >= wrows) {
        if (lane == 0) m[0] = 0u, m[1] = 0u, m[3] = 0u;
        return;
    }
    const uint32_t nrows = wrows - r0 < 32u ? (uint32_t)(wrows - r0) : 32u;
    const bool in = lane < nrows;
    const uint64_t row = l.woff[0] + r0 + (in ? lane : 0u);
    uint32_t lo = 1, hi = wn;  // the first offset above `row` is in [1, wn]: row >= woff[0], row < woff[wn]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (l.woff[mid] > row) hi = mid;
        else lo = mid + 1u;
    }
    const uint32_t slot = lo - 1u;
    const uint32_t prev = (uint32_t)__shfl((int)slot, (int)((lane + 63u) & 63u));
    const bool head = in && (lane == 0u || slot != prev);
    const uint64_t heads = ballot64(head);
    const uint64_t live = ballot64(in && l.wacc[slot] != 0u);
    if (head) {
        const uint32_t s = mbcnt(heads);
        m[4 + s] = lane;
        m[37 + s] = slot | (l.woff[slot + 1] <= l.woff[0] + r0 + nrows ? kEndsBit : 0u);
    }
    if (lane == 0) {
        const uint32_t nseg = (uint32_t)__popcll(heads);
        m[0] = live != 0ull ? 1u : 0u;
        m[1] = nseg;
        m[3] = nrows;
        m[4 + nseg] = nrows;
    }
}

// the helper wavefront, after the barrier behind tile t's cells: a finished, accepted document takes its cells of this group's
// query rows, in order
__device__ __forceinline__ void mvf_fold_tile(const MvFlatArgs& a, const MvfLds& l, const uint32_t* m, const float* cells,
                                              uint32_t grows, uint32_t lane) {
    if (m[0] == 0u || lane >= m[1]) return;
    const uint32_t dv = m[37 + lane], slot = dv & ~kEndsBit;
    if (!(dv & kEndsBit) || l.wacc[slot] == 0u) return;
    const float* c = cells + lane * kCellStride;
    float x = l.agg[slot];
    for (uint32_t i = 0; i < grows; ++i) x = mvf_fold(a.aggregation, x, c[i]);
    l.agg[slot] = x;
}

// The maximum of every segment of a tile over this lane's 16 set rows and its partner's (l ^ 32): lane l holds register
// r = tile row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of query row l & 31.  `mx` carries a document into the next tile.
__device__ __forceinline__ void mvf_segmax(const ms_f32x16& acc, const uint32_t* m, const MvfLds& l, uint64_t tile_row0, float* cells,
                                           uint32_t col, uint32_t hi, float& mx) {
    const uint32_t nseg = (uint32_t)__builtin_amdgcn_readfirstlane((int)m[1]);
    for (uint32_t s = 0; s < nseg; ++s) {
        const uint32_t lo_row = m[4 + s], hi_row = m[5 + s], dv = m[37 + s], slot = dv & ~kEndsBit;
        float v = -FLT_MAX;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t i = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * hi;
            const float x = acc[r];
            v = (i >= lo_row && i < hi_row && x > v) ? x : v;
        }
        const float other = __shfl_xor(v, 32);
        v = other > v ? other : v;
        if (s == 0u && l.woff[slot] - l.woff[0] < tile_row0) v = mx > v ? mx : v;  // the document began in an earlier tile
        if (dv & kEndsBit) {
            if (hi == 0u) cells[s * kCellStride + col] = -v;  // the negation comes last: a maximum of +0.0 gives -0.0
        } else {
            mx = v;  // (the tile's last segment)
        }
    }
}

template <typename RT, int KS>
__global__ __launch_bounds__(kMvFlatThreads) void mvflat_mfma_kernel(MvFlatArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mvf_smem[];
    const MvfLds l = mvf_carve<(KS > 0 ? 2u : 5u)>(mvf_smem);
    const MvfBlock b = mvf_block(a, l);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, l31 = lane & 31u, hi = lane >> 5;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    // (a one-tile query would put every workgroup's MFMAs on SIMD 0: the tile owner rotates with the workgroup)
    const uint32_t wv = (wave + blockIdx.x + blockIdx.y) & 3u;
    // the wavefront that describes the tiles and folds the finished documents: the owner of a group's LAST query tile, which
    // a query of up to 96 rows leaves without MFMAs -- the descriptions and folds are then off the multiplying wavefront
    const bool helper = wv == 3u;
    const uint32_t qtiles = (b.qn + 31u) >> 5;
    const uint32_t esz = (uint32_t)sizeof(RT);
    float* const slab0 = l.slab;
    for (uint32_t w0 = b.dlo; w0 < b.dhi; w0 += kW) {
        const uint32_t wn = b.dhi - w0 < kW ? b.dhi - w0 : kW;
        mvf_window_load(b, l, w0, wn);
        const uint32_t ntiles = (uint32_t)((l.woff[wn] - l.woff[0] + 31u) >> 5);  // (2^32 tiles of 32 rows are beyond any device)
        const uint8_t* const wbase = a.drows + l.woff[0] * a.stride;
        for (uint32_t g0 = 0; g0 < qtiles && ntiles; g0 += 4u) {
            const uint32_t qt = g0 + wv;
            const bool has = qt < qtiles;
            const uint32_t grows = b.qn - (g0 << 5) < kMvFlatGroupRows ? b.qn - (g0 << 5) : kMvFlatGroupRows;
            const uint32_t qrows_here = has ? (b.qn - (qt << 5) < 32u ? b.qn - (qt << 5) : 32u) : 0u;
            const uint8_t* const qtile = b.q + (uint64_t)(has ? qt << 5 : 0u) * a.stride;
            float bq[KS > 0 ? KS : 1];
            if constexpr (KS > 0) {
                // the group's query tiles, one after the other through a slab, each into its owner's registers
                for (uint32_t w = 0; w < 4u && g0 + w < qtiles; ++w) {
                    const uint32_t t = g0 + w, n = b.qn - (t << 5) < 32u ? b.qn - (t << 5) : 32u;
                    __syncthreads();
                    ms_stage<RT, kT>(slab0, b.q + (uint64_t)(t << 5) * a.stride, a.stride, n, 0u, tid);
                    __syncthreads();
                    if (wv == w) {
#pragma unroll
                        for (int m = 0; m < KS; ++m) {
                            const uint32_t k = 2u * (uint32_t)m + hi;
                            bq[m] = slab0[k * 32u + (l31 ^ ms_swz<RT>(k))];
                        }
                    }
                }
            }
            __syncthreads();  // the slab's and the descriptions' last readers are done
            if (helper) {
                mvf_meta(l.meta, l, wn, 0, lane);
                mvf_meta(l.meta + kMetaWords, l, wn, 1, lane);
            }
            __syncthreads();
            MsFetch<RT, kT> f;
            if constexpr (KS > 0) {
                if (l.meta[0]) {
                    ms_fetch<RT, kT>(f, wbase, a.stride, l.meta[3], tid);
                    ms_place<RT, kT>(slab0, f, a.stride, tid);
                }
            }
            float mx = -FLT_MAX;
            for (uint32_t t = 0; t < ntiles; ++t) {
                const uint32_t* const m = l.meta + (t % 3u) * kMetaWords;
                const uint32_t* const mnext = l.meta + ((t + 1u) % 3u) * kMetaWords;
                float* const cells = l.cells + (t & 1u) * kCellFloats;
                __syncthreads();  // tile t is staged and described; the cells of tile t - 1 are written
                const bool live = m[0] != 0u;
                const bool live_next = t + 1u < ntiles && mnext[0] != 0u;
                if constexpr (KS > 0) {
                    if (live_next) ms_fetch<RT, kT>(f, wbase + (uint64_t)(t + 1u) * 32u * a.stride, a.stride, mnext[3], tid);
                }
                if (helper && t > 0u)
                    mvf_fold_tile(a, l, l.meta + ((t - 1u) % 3u) * kMetaWords, l.cells + ((t - 1u) & 1u) * kCellFloats,
                                  grows, lane);
                if (live) {
                    ms_f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
                    if constexpr (KS > 0) {
                        if (has) {
                            const float* const dslab = slab0 + (t & 1u) * kMsSlabFloats;
#pragma unroll
                            for (int mm = 0; mm < KS; ++mm) {
                                const uint32_t k = 2u * (uint32_t)mm + hi;
                                const float av = dslab[k * 32u + (l31 ^ ms_swz<RT>(k))];
                                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bq[mm], acc, 0, 0, 0);
                            }
                        }
                    } else {
                        float* const qslab = slab0 + kMsSlabFloats * (1u + wave);
                        const uint8_t* const dtile = wbase + (uint64_t)t * 32u * a.stride;
                        for (uint32_t k0 = 0; k0 < a.dim; k0 += kMsSlabK) {
                            if (k0) __syncthreads();
                            ms_stage<RT, kT>(slab0, dtile, a.stride, m[3], k0 * esz, tid);
                            if (has) ms_stage<RT, 64u>(qslab, qtile, a.stride, qrows_here, k0 * esz, lane);
                            __syncthreads();
                            if (has) {
                                const uint32_t left = a.dim - k0, steps = left >= kMsSlabK ? kMsSlabK / 2u : (left + 1u) >> 1;
                                for (uint32_t mm = 0; mm < steps; ++mm) {
                                    const uint32_t k = 2u * mm + hi, o = k * 32u + (l31 ^ ms_swz<RT>(k));
                                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(slab0[o], qslab[o], acc, 0, 0, 0);
                                }
                            }
                        }
                    }
                    if (has) mvf_segmax(acc, m, l, (uint64_t)t * 32u, cells, (wv << 5) + l31, hi, mx);
                }
                if constexpr (KS > 0) {
                    if (live_next) ms_place<RT, kT>(slab0 + ((t + 1u) & 1u) * kMsSlabFloats, f, a.stride, tid);
                }
                if (helper && t + 2u < ntiles) mvf_meta(l.meta + ((t + 2u) % 3u) * kMetaWords, l, wn, t + 2u, lane);
            }
            __syncthreads();
            if (helper)
                mvf_fold_tile(a, l, l.meta + ((ntiles - 1u) % 3u) * kMetaWords,
                              l.cells + ((ntiles - 1u) & 1u) * kCellFloats, grows, lane);
        }
        mvf_window_finish(b, l, w0, wn);
    }
    mvf_block_end(b, l);
}

// ---- reference order, deliberately plain --------------------------------------------------------------------------------
// A lane group of Scheme<DT, IP, pair>::G lanes per document of the window: for each query row in order the minimum, from
// f32::MAX, of the bit-exact pair function over the document's rows, folded into the document's aggregate at once.
template <int DT>
__global__ __launch_bounds__(kMvFlatThreads) void mvflat_rows_kernel(MvFlatArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mvf_smem[];
    const MvfLds l = mvf_carve<0u>(mvf_smem);
    const MvfBlock b = mvf_block(a, l);
    constexpr int G = Scheme<DT, OP_IP, true>::G;
    const uint32_t g = threadIdx.x / G, groups = kT / G;
    const int v = (int)(threadIdx.x % G);
    for (uint32_t w0 = b.dlo; w0 < b.dhi; w0 += kW) {
        const uint32_t wn = b.dhi - w0 < kW ? b.dhi - w0 : kW;
        mvf_window_load(b, l, w0, wn);
        for (uint32_t j = g; j < wn; j += groups) {  // whole groups leave together (G divides 64)
            const uint64_t d0 = l.woff[j], dn = l.woff[j + 1] - d0;
            if (l.wacc[j] == 0u || dn == 0) continue;
            float x = l.agg[j];
            for (uint32_t i = 0; i < b.qn; ++i) {
                const uint8_t* qrow = b.q + (uint64_t)i * a.stride;
                float mn = FLT_MAX;
                for (uint64_t r = 0; r < dn; ++r) {
                    const float raw = group_distance_rows<DT, OP_IP>(qrow, a.drows + (d0 + r) * a.stride, (int)a.dim, v);
                    const float d = post_op<OP_IP, false>(raw);
                    mn = d < mn ? d : mn;
                }
                x = mvf_fold(a.aggregation, x, mn);
            }
            if (v == 0) l.agg[j] = x;
        }
        mvf_window_finish(b, l, w0, wn);
    }
    mvf_block_end(b, l);
}

// ---- merge ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFlatThreads) void mvflat_merge_kernel(MvFlatArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mvf_smem[];
    uint64_t* const keys = reinterpret_cast<uint64_t*>(mvf_smem);
    const uint32_t qi = blockIdx.x, k = a.k;
    flat_merge_rounds(keys, a.lists + (uint64_t)qi * a.nchunks * k, (uint64_t)a.nchunks * k, k, a.merge_cap);
    for (uint32_t r = threadIdx.x; r < k; r += kFlatThreads) {
        const uint64_t key = keys[r];
        const bool has = key != kFlatNoKey;
        const uint32_t doc = ~(uint32_t)key;
        float d = has ? key_dist(key) : __builtin_inff();
        if (has && a.negzero && d == 0.0f && ((a.negzero[(uint64_t)qi * a.nz_words + (doc >> 5)] >> (doc & 31u)) & 1u)) d = -0.0f;
        a.out_ids[(uint64_t)qi * k + r] = has ? doc : kEmpty;
        a.out_dists[(uint64_t)qi * k + r] = d;
    }
    if (a.stats && threadIdx.x == 0) flat_merge_stats(a.stats + qi, keys, k, a.chunk_cmps + (uint64_t)qi * a.nchunks, a.nchunks);
}

template <typename RT>
int32_t launch_scan_mfma(const MvFlatArgs& a, dim3 grid, hipStream_t stream) {
    const size_t lds_reg = mvf_lds_bytes(a.cap, 2), lds_slab = mvf_lds_bytes(a.cap, 5);
    const char* what = "mvflat_mfma_kernel launch";
    if (a.dim <= 32) return launch_kernel<mvflat_mfma_kernel<RT, 16>>(what, grid, dim3(kT), lds_reg, stream, a);
    if (a.dim <= 64) return launch_kernel<mvflat_mfma_kernel<RT, 32>>(what, grid, dim3(kT), lds_reg, stream, a);
    if (a.dim <= 128) return launch_kernel<mvflat_mfma_kernel<RT, 64>>(what, grid, dim3(kT), lds_reg, stream, a);
    return launch_kernel<mvflat_mfma_kernel<RT, 0>>(what, grid, dim3(kT), lds_slab, stream, a);
}

}  // namespace

// One batch of queries (nq <= plan.batch; d_qoff: their nq + 1 offsets into d_qrows) over documents [first, first + n),
// n > 0.  `scratch`: plan.scratch_bytes().  d_filter: the bitmaps of these queries (null: every document), `fstride`
// words apart (0: one for all).  d_negzero: nq x nz_words zeroed words for DANN_MV_MIN_PAIRWISE, else null.
int32_t launch_mv_flat_search(const MvFlatSet& set, const MvFlatPlan& plan, int32_t order, int32_t aggregation, const uint8_t* d_qrows,
                              const uint32_t* d_qoff, uint32_t nq, uint32_t first, uint32_t n, const uint32_t* d_filter,
                              uint64_t fstride, uint32_t* d_negzero, uint32_t nz_words, void* scratch, uint32_t* d_ids,
                              float* d_dists, dann_search_stats* d_stats, hipStream_t stream) {
    MvFlatArgs a;
    a.drows = set.drows;
    a.doff = set.doff;
    a.qrows = d_qrows;
    a.qoff = d_qoff;
    a.dim = set.dim;
    a.stride = set.stride;
    a.nq = nq;
    a.first = first;
    a.n = n;
    a.k = plan.k;
    a.aggregation = aggregation;
    a.nchunks = plan.nchunks;
    a.chunk_rows = plan.chunk_rows;
    a.cap = plan.cap;
    a.merge_cap = plan.merge_cap;
    a.fbits = d_filter;
    a.fstride = fstride;
    a.negzero = d_negzero;
    a.nz_words = nz_words;
    a.lists = reinterpret_cast<uint64_t*>(scratch);
    a.chunk_cmps = reinterpret_cast<uint32_t*>(a.lists + (size_t)plan.batch * plan.nchunks * plan.k);
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.stats = d_stats;
    const dim3 grid(plan.nchunks, nq);
    int32_t rc;
    if (order == DANN_MAXSIM_KERNEL) {
        rc = set.dtype == DT_F32 ? launch_scan_mfma<float>(a, grid, stream) : launch_scan_mfma<__half>(a, grid, stream);
    } else {
        const char* what = "mvflat_rows_kernel launch";
        const size_t lds = mvf_lds_bytes(a.cap, 0);
        rc = set.dtype == DT_F32 ? launch_kernel<mvflat_rows_kernel<DT_F32>>(what, grid, dim3(kT), lds, stream, a)
                                 : launch_kernel<mvflat_rows_kernel<DT_F16>>(what, grid, dim3(kT), lds, stream, a);
    }
    if (rc != DANN_OK) return rc;
    return launch_kernel<mvflat_merge_kernel>("mvflat_merge_kernel launch", dim3(nq), dim3(kFlatThreads), plan.merge_lds, stream, a);
}

}  // namespace dann
