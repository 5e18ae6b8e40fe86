// flat_gt_kernels.hip -- the exhaustive scans that tell whether a filtered or a range search is right:
//   compute_ground_truth_from_data with query_bitmaps (diskann-tools/src/utils/ground_truth.rs:589-693): a point goes
//       through NeighborPriorityQueue::insert only if the query's bitmap holds its id;
//   compute_range_ground_truth_from_data (:285-353): every allowed point within the radius, in ascending id order.
// Both tile like flat_scan_kernel (a workgroup owns a tile of queries x a chunk of slots) and score with the same
// group_distance_many + finish_distance.  What is new is the work list: before it scores, a workgroup turns the chunk's
// bitmap words -- the tile's queries' words OR-ed, AND-ed with the range and the deleted state -- into the ascending list
// of the slots it visits, kFlatGtSegRows slots at a time, and the steps walk that list.  A row that no query of the tile
// accepts is never fetched; a query scores and counts only the entries whose own bit is set (an entry carries the tile's
// accept mask).  Row loads still go out unconditionally at clamped addresses and are deselected afterwards.
//
//   flat_filtered_scan_kernel  flat_scan_kernel over the list; the chunk lists go to flat_merge_kernel unchanged
//   flat_range_kernel<false>   counts matches and rows evaluated per (query, chunk)
//   flat_range_offsets_kernel  per query: exclusive scan of its chunks' counts, the true count, the stats, the padding
//   flat_range_kernel<true>    scores again and writes every chunk's matches from its offset on, a step's matches ordered
//                              by ballot prefix counts: ascending slot order, no atomics on the outputs
#include "flat_gt_launch.h"
#include "flat_impl.h"

namespace dann {
namespace {

constexpr int kWave = kFlatWave;
constexpr int kU = kFlatU;
constexpr uint32_t kWaves = kFlatThreads / kWave;
static_assert(kFlatGtSegWords <= kFlatThreads, "a thread takes at most one word of a list build");

// what a list build reads, kept in LDS and not in scalar registers: the step body between two builds already holds as
// many scalars as the register file has (flat_scan_kernel: up to 101), and every value a build needs would have to live
// across it
struct ListCtl {
    uint32_t wsum[kWaves];  // a build's entries per wavefront
    uint32_t lo, hi;        // the chunk's slots
    uint32_t tq, pad;       // queries of this tile
    const uint32_t* fbits;  // the bitmap of the tile's first query (null: every slot matches)
    uint64_t stride;        // words between the queries' bitmaps (0: one bitmap for all)
    const uint32_t* deleted;
};
static_assert(sizeof(ListCtl) <= 64, "the list's header is 64 bytes of LDS");

// the bitmaps of a filtered launch's queries, `stride` words apart (0: one for all)
struct FilterArg {
    const uint32_t* bits;
    uint64_t stride;
};

struct WorkList {
    uint32_t* ids;   // [kFlatGtListCap] slots, ascending
    uint8_t* masks;  // [kFlatGtListCap] bit t: the tile's query t accepts the slot
    ListCtl* ctl;
};

__device__ __forceinline__ WorkList work_list_at(uint8_t* lds) {
    WorkList wl;
    wl.ctl = reinterpret_cast<ListCtl*>(lds);
    wl.ids = reinterpret_cast<uint32_t*>(lds + 64);
    wl.masks = lds + 64 + (size_t)kFlatGtListCap * 4;
    return wl;
}

// (the caller's barrier after its own LDS set-up publishes the header)
__device__ __forceinline__ void work_list_init(const WorkList& wl, uint32_t lo, uint32_t hi, uint32_t tq, const uint32_t* fbits,
                                               uint64_t stride, const uint32_t* deleted) {
    if (threadIdx.x == 0) {
        wl.ctl->lo = lo;
        wl.ctl->hi = hi;
        wl.ctl->tq = tq;
        wl.ctl->fbits = fbits;
        wl.ctl->stride = stride;
        wl.ctl->deleted = deleted;
    }
}

// Appends the slots of the words [w0, w0 + kFlatGtSegWords) that lie in the chunk, are not deleted and are accepted by at
// least one of the tile's queries to the list, which holds `fill` entries, and returns the new length.  A thread takes a
// word; popcount prefixes order the list.  Per-query bitmaps take a second walk over the words, a query at a time, that
// sets the query's bit in the entries it accepts.  Ends with a barrier.
__device__ __forceinline__ uint32_t work_list_append(const WorkList& wl, uint32_t fill, uint32_t w0) {
    // (the thread index is made opaque here: otherwise every lane predicate of a build -- lane >= 1, 2, .. 32, lane == 63,
    // wave > 0, 1, 2, thread < 128 -- is hoisted out of the chunk loop as a 64-bit mask in a scalar register pair)
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = wl.ctl->lo, hi = wl.ctl->hi, tq = wl.ctl->tq;  // (LDS reads: per-lane registers from here on)
    const uint32_t* const fbits = wl.ctl->fbits;
    const uint64_t stride = wl.ctl->stride;
    const uint32_t* const deleted = wl.ctl->deleted;
    const uint32_t wi = w0 + tid;
    const uint64_t b0 = (uint64_t)wi * 32;
    const bool valid = tid < kFlatGtSegWords && b0 < hi;
    const uint32_t wc = valid ? wi : (lo >> 5);  // (word loads go out at a clamped index and are masked afterwards)
    uint32_t m = valid ? ~0u : 0u;
    if (valid && b0 < lo) m &= ~0u << (uint32_t)(lo - b0);
    if (valid && hi - b0 < 32) m &= (1u << (uint32_t)(hi - b0)) - 1u;
    if (deleted) m &= ~deleted[wc];
    const bool per_query = fbits && stride;
    uint32_t any = fbits ? 0u : m;
    if (fbits) {
        const uint32_t* p = fbits + wc;
        const uint32_t nb = per_query ? tq : 1u;
        for (uint32_t t = 0; t < nb; ++t, p += stride) any |= *p & m;
    }
    uint32_t incl = (uint32_t)__popc(any);
    const uint32_t own = incl;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
        if ((int)lane >= d) incl += y;
    }
    if (lane == kWave - 1) wl.ctl->wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t i = 0; i < kWaves; ++i) {
        const uint32_t s = wl.ctl->wsum[i];
        before += i < wave ? s : 0u;
        total += s;
    }
    const uint32_t at = fill + before + incl - own;
    const uint8_t all = per_query ? (uint8_t)0 : (uint8_t)((1u << tq) - 1u);
    uint32_t pos = at;
    for (uint32_t rest = any; rest; rest &= rest - 1u, ++pos) {
        wl.ids[pos] = (uint32_t)b0 + (uint32_t)__ffs((int)rest) - 1u;
        wl.masks[pos] = all;
    }
    if (per_query) {
        const uint32_t* p = fbits + wc;
        for (uint32_t t = 0; t < tq; ++t, p += stride) {
            // (an entry's mask byte is this thread's own: no other thread writes it)
            for (uint32_t rest = *p & m; rest; rest &= rest - 1u) {
                const uint32_t j = (uint32_t)__ffs((int)rest) - 1u;
                wl.masks[at + (uint32_t)__popc(any & ((1u << j) - 1u))] |= (uint8_t)(1u << t);
            }
        }
    }
    __syncthreads();
    return fill + (uint32_t)__builtin_amdgcn_readfirstlane((int)total);  // (the same in every lane)
}

// moves the entries [pos, fill) that the steps left over (fewer than a step's rows) to the front of the list
__device__ __forceinline__ uint32_t work_list_carry(const WorkList& wl, uint32_t pos, uint32_t fill) {
    const uint32_t rem = pos < fill ? fill - pos : 0u;
    uint32_t id = 0;
    uint8_t mask = 0;
    if (threadIdx.x < rem) {
        id = wl.ids[pos + threadIdx.x];
        mask = wl.masks[pos + threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x < rem) {
        wl.ids[threadIdx.x] = id;
        wl.masks[threadIdx.x] = mask;
    }
    __syncthreads();
    return rem;
}

// the rows of one step over the list entries [pos, fill): row u of lane group g of a wavefront is entry
// pos + (wave * kU + u) * GROUPS + g.  Loads go out unconditionally at clamped addresses (an entry past the list or an
// unpublished slot reads the chunk's first row) and are selected afterwards.
template <int GROUPS>
__device__ __forceinline__ void step_rows(const IndexView& ix, const WorkList& wl, uint32_t pos, uint32_t fill, uint32_t lo,
                                          uint32_t wave, int g, const uint8_t* (&rows)[kU], bool (&act)[kU],
                                          uint32_t (&id)[kU], uint32_t (&qm)[kU]) {
#pragma unroll
    for (int u = 0; u < kU; ++u) {
        const uint32_t li = pos + (uint32_t)((wave * kU + u) * GROUPS + g);
        const bool in = li < fill;
        const uint32_t lc = in ? li : pos;  // (pos < fill <= kFlatGtListCap)
        id[u] = in ? wl.ids[lc] : lo;
        qm[u] = in ? (uint32_t)wl.masks[lc] : 0u;
        rows[u] = ix.rows + (uint64_t)id[u] * ix.row_stride;
        bool ok = in;
        if (ix.tag_off) ok = ok && rows[u][ix.tag_off] >= kTagReadable;
        act[u] = ok;
        if (!ok) rows[u] = ix.rows + (uint64_t)lo * ix.row_stride;
    }
}

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kFlatThreads) void flat_filtered_scan_kernel(IndexView ix, FlatArgs a, FilterArg f) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using S = Scheme<DT, OP, false>;
    constexpr int G = S::G, GROUPS = kWave / G;
    constexpr uint32_t kStep = (kFlatThreads / G) * kU;  // rows a workgroup scores per step
    static_assert(kStep <= kFlatStepRows, "a step must fit the headroom of the candidate buffers and of the list");
    using QT = typename std::conditional<S::kInt, uint8_t, float>::type;
    // LDS: tile staged queries | tile candidate buffers | tile threshold keys | tile fill counts | tile cmps | the list
    uint8_t* const qbase = smem;
    uint64_t* const bufs = reinterpret_cast<uint64_t*>(smem + (size_t)a.tile * a.qslot);
    uint64_t* const thr = bufs + (size_t)a.tile * a.cap;
    uint32_t* const cnt = reinterpret_cast<uint32_t*>(thr + a.tile);
    uint32_t* const cmps = cnt + a.tile;
    const WorkList wl = work_list_at(smem + (size_t)a.tile * ((size_t)a.qslot + (size_t)a.cap * 8 + 16));

    const uint32_t chunk = blockIdx.x, q0 = blockIdx.y * a.tile;
    const uint32_t tq = a.nq - q0 < a.tile ? a.nq - q0 : a.tile;
    // (first + n <= the index's slots: a chunk's bounds fit 32 bits)
    const uint64_t lo64 = (uint64_t)a.first + (uint64_t)chunk * a.chunk_rows, end = (uint64_t)a.first + a.n;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)(lo64 + a.chunk_rows < end ? lo64 + a.chunk_rows : end);
    const SqParams sqp{ix.sq_k, ix.sq_shift_norm_sq};
    work_list_init(wl, lo, hi, tq, f.bits + (uint64_t)q0 * f.stride, f.stride, a.deleted);

    for (uint32_t t = 0; t < tq; ++t) flat_stage_query<DT, OP>(ix, a.queries, q0 + t, qbase + (size_t)t * a.qslot);
    if (threadIdx.x < a.tile) {
        thr[threadIdx.x] = kFlatNoKey;
        cnt[threadIdx.x] = 0;
        cmps[threadIdx.x] = 0;
    }
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int g = lane / G, v = lane % G;
    const uint32_t wend = (uint32_t)(((uint64_t)hi + 31) >> 5);  // (at most 2^27: w0 does not wrap)
    uint32_t fill = 0;
    for (uint32_t w0 = lo >> 5; w0 < wend; w0 += kFlatGtSegWords) {
        fill = work_list_append(wl, fill, w0);
        const bool last = w0 + kFlatGtSegWords >= wend;
        uint32_t pos = 0;
        for (; pos < fill && (fill - pos >= kStep || last); pos += kStep) {
            const uint8_t* rows[kU];
            bool act[kU];
            uint32_t id[kU], qm[kU];
            step_rows<GROUPS>(ix, wl, pos, fill, lo, wave, g, rows, act, id, qm);
            for (uint32_t t = 0; t < tq; ++t) {
                const QT* qs = reinterpret_cast<const QT*>(qbase + (size_t)t * a.qslot + query_stage_off(DT));
                float o[kU];
                group_distance_many<DT, OP, false, kU, false>(qs, rows, act, (int)ix.dim, v, o);
                const uint64_t limit = thr[t];
                uint32_t evaluated = 0;
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    if (act[u] && ((qm[u] >> t) & 1u) && v == 0) {
                        ++evaluated;
                        const float d = finish_distance<DT, OP, NORM>(o[u], reinterpret_cast<const uint8_t*>(qs), rows[u], ix.dim, sqp);
                        if (d == d) {  // (queue.rs: a NaN distance is dropped)
                            const uint64_t key = dist_key(d, ~id[u]);
                            if (key < limit) bufs[(size_t)t * a.cap + atomicAdd(&cnt[t], 1u)] = key;
                        }
                    }
                }
                if (evaluated) atomicAdd(&cmps[t], evaluated);
            }
            __syncthreads();
            for (uint32_t t = 0; t < tq; ++t) {
                const uint32_t fillq = cnt[t];  // (the same for the whole workgroup)
                if (fillq + kStep > a.cap) flat_cut_to_k(bufs + (size_t)t * a.cap, a.cap, fillq, a.k, &cnt[t], &thr[t]);
            }
            __syncthreads();
        }
        if (!last) fill = work_list_carry(wl, pos, fill);
    }
    // the chunk's best k keys of every query, ascending, kFlatNoKey behind the last; and the rows it evaluated
    for (uint32_t t = 0; t < tq; ++t) {
        const uint32_t fillq = cnt[t];
        uint64_t* keys = bufs + (size_t)t * a.cap;
        flat_cut_to_k(keys, a.cap, fillq, a.k, &cnt[t], &thr[t]);
        uint64_t* out = a.lists + ((uint64_t)(q0 + t) * a.nchunks + chunk) * a.k;
        for (uint32_t i = threadIdx.x; i < a.k; i += kFlatThreads) out[i] = keys[i];  // (cap > k: pads are in place)
    }
    if (threadIdx.x < tq) a.chunk_cmps[(uint64_t)(q0 + threadIdx.x) * a.nchunks + chunk] = cmps[threadIdx.x];
}

struct RangeArgs {
    const void* queries;
    uint32_t nq;
    uint32_t first, n;
    uint32_t chunk_rows, nchunks;
    uint32_t tile, qslot;
    const uint32_t* deleted;
    const uint32_t* filter;  // null: every slot matches
    uint64_t filter_stride;
    float radius, inner_radius;
    uint32_t has_inner;
    uint32_t out_cap;
    uint32_t* counts;  // [nq][nchunks]: matches; after flat_range_offsets_kernel the place of the chunk's first match
    uint32_t* cmps;    // [nq][nchunks]: rows evaluated
    uint32_t* overflow;  // set when a query has more matches than out_cap
    uint32_t* out_ids;   // [nq][out_cap]
    float* out_dists;
    uint32_t* out_counts;
    dann_search_stats* stats;  // may be null
};

// range_search.rs:326-335: within the radius and, given an inner radius, not within that; a NaN distance fails
__device__ __forceinline__ bool range_accepts(const RangeArgs& a, float d) {
    return d <= a.radius && !(a.has_inner && d <= a.inner_radius);
}

template <int DT, int OP, bool NORM, bool WRITE>
__global__ __launch_bounds__(kFlatThreads) void flat_range_kernel(IndexView ix, RangeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using S = Scheme<DT, OP, false>;
    constexpr int G = S::G, GROUPS = kWave / G;
    constexpr uint32_t kStep = (kFlatThreads / G) * kU;
    static_assert(kStep <= kFlatStepRows, "a step must fit the matched distances and the headroom of the list");
    using QT = typename std::conditional<S::kInt, uint8_t, float>::type;
    // LDS: tile staged queries | tile x kFlatStepRows matched distances of a step | per query 8 words: matches (count
    // pass) or the place of the next match (write pass), rows evaluated, 2 spare, the wavefronts' matches of a step
    uint8_t* const qbase = smem;
    float* const stash = reinterpret_cast<float*>(smem + (size_t)a.tile * a.qslot);
    uint32_t* const ctr = reinterpret_cast<uint32_t*>(stash + (size_t)a.tile * kFlatStepRows);
    const WorkList wl = work_list_at(smem + (size_t)a.tile * flat_range_lds_per_query(a.qslot));

    const uint32_t chunk = blockIdx.x, q0 = blockIdx.y * a.tile;
    const uint32_t tq = a.nq - q0 < a.tile ? a.nq - q0 : a.tile;
    // (first + n <= the index's slots: a chunk's bounds fit 32 bits)
    const uint64_t lo64 = (uint64_t)a.first + (uint64_t)chunk * a.chunk_rows, end = (uint64_t)a.first + a.n;
    const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)(lo64 + a.chunk_rows < end ? lo64 + a.chunk_rows : end);
    const SqParams sqp{ix.sq_k, ix.sq_shift_norm_sq};
    work_list_init(wl, lo, hi, tq, a.filter ? a.filter + (uint64_t)q0 * a.filter_stride : nullptr, a.filter_stride, a.deleted);

    for (uint32_t t = 0; t < tq; ++t) flat_stage_query<DT, OP>(ix, a.queries, q0 + t, qbase + (size_t)t * a.qslot);
    if (threadIdx.x < a.tile * 8u) ctr[threadIdx.x] = 0;
    __syncthreads();
    if (WRITE && threadIdx.x < tq) ctr[threadIdx.x * 8u] = a.counts[(uint64_t)(q0 + threadIdx.x) * a.nchunks + chunk];
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int g = lane / G, v = lane % G;
    const float kNoMatch = __builtin_nanf("");
    const uint32_t wend = (uint32_t)(((uint64_t)hi + 31) >> 5);  // (at most 2^27: w0 does not wrap)
    uint32_t fill = 0;
    for (uint32_t w0 = lo >> 5; w0 < wend; w0 += kFlatGtSegWords) {
        fill = work_list_append(wl, fill, w0);
        const bool last = w0 + kFlatGtSegWords >= wend;
        uint32_t pos = 0;
        for (; pos < fill && (fill - pos >= kStep || last); pos += kStep) {
            const uint8_t* rows[kU];
            bool act[kU];
            uint32_t id[kU], qm[kU];
            step_rows<GROUPS>(ix, wl, pos, fill, lo, wave, g, rows, act, id, qm);
            for (uint32_t t = 0; t < tq; ++t) {
                const QT* qs = reinterpret_cast<const QT*>(qbase + (size_t)t * a.qslot + query_stage_off(DT));
                float o[kU];
                group_distance_many<DT, OP, false, kU, false>(qs, rows, act, (int)ix.dim, v, o);
                uint32_t evaluated = 0, matched = 0;
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    if (v == 0) {
                        float keep = kNoMatch;
                        if (act[u] && ((qm[u] >> t) & 1u)) {
                            ++evaluated;
                            const float d = finish_distance<DT, OP, NORM>(o[u], reinterpret_cast<const uint8_t*>(qs), rows[u], ix.dim, sqp);
                            if (range_accepts(a, d)) {
                                ++matched;
                                keep = d;
                            }
                        }
                        if (WRITE) stash[(size_t)t * kFlatStepRows + (wave * kU + u) * GROUPS + g] = keep;
                    }
                }
                if (!WRITE) {
                    if (matched) atomicAdd(&ctr[t * 8u], matched);
                    if (evaluated) atomicAdd(&ctr[t * 8u + 1u], evaluated);
                }
            }
            if (WRITE) {
                // thread r owns row r of the step: its place is the query's next place + the matches of the rows before it
                // (the thread index is opaque here as in work_list_append: its lane predicates stay out of scalar pairs)
                __syncthreads();
                uint32_t r = threadIdx.x;
                asm volatile("" : "+v"(r));
                const uint32_t rlane = r & 63u, rwave = r >> 6;
                for (uint32_t t = 0; t < tq; ++t) {
                    const float x = r < kStep ? stash[(size_t)t * kFlatStepRows + r] : kNoMatch;
                    const uint64_t b = ballot64(x == x);
                    if (rlane == 0) ctr[t * 8u + 4u + rwave] = (uint32_t)__popcll(b);
                }
                __syncthreads();
                for (uint32_t t = 0; t < tq; ++t) {
                    const float x = r < kStep ? stash[(size_t)t * kFlatStepRows + r] : kNoMatch;
                    const uint64_t b = ballot64(x == x);
                    uint32_t place = ctr[t * 8u] + mbcnt(b);
#pragma unroll
                    for (uint32_t i = 0; i < kWaves; ++i) place += i < rwave ? ctr[t * 8u + 4u + i] : 0u;
                    if (x == x && place < a.out_cap) {
                        a.out_ids[(uint64_t)(q0 + t) * a.out_cap + place] = wl.ids[pos + r];
                        a.out_dists[(uint64_t)(q0 + t) * a.out_cap + place] = x;
                    }
                }
                __syncthreads();
                if (threadIdx.x < tq) {
                    uint32_t s = 0;
#pragma unroll
                    for (uint32_t i = 0; i < kWaves; ++i) s += ctr[threadIdx.x * 8u + 4u + i];
                    ctr[threadIdx.x * 8u] += s;
                }
            }
            __syncthreads();
        }
        if (!last) fill = work_list_carry(wl, pos, fill);
    }
    if (!WRITE && threadIdx.x < tq) {
        const uint64_t at = (uint64_t)(q0 + threadIdx.x) * a.nchunks + chunk;
        a.counts[at] = ctr[threadIdx.x * 8u];
        a.cmps[at] = ctr[threadIdx.x * 8u + 1u];
    }
}

// One workgroup per query: the exclusive scan of its chunks' counts in place (a thread sums a run of chunks, thread 0
// scans the runs' sums), then out_counts, the stats and the 0xFFFFFFFF / +inf behind the last result.
__global__ __launch_bounds__(kFlatThreads) void flat_range_offsets_kernel(RangeArgs a) {
    __shared__ uint32_t sums[kFlatThreads], evals[kFlatThreads];
    __shared__ uint32_t total, total_cmps;
    const uint32_t qi = blockIdx.x;
    uint32_t* counts = a.counts + (uint64_t)qi * a.nchunks;
    const uint32_t* cmps = a.cmps + (uint64_t)qi * a.nchunks;
    const uint32_t per = flat_range_run_chunks(a.nchunks);
    const uint32_t c0 = min(threadIdx.x * per, a.nchunks), c1 = min(c0 + per, a.nchunks);
    uint32_t s = 0, e = 0;
    for (uint32_t c = c0; c < c1; ++c) {
        s += counts[c];
        e += cmps[c];
    }
    sums[threadIdx.x] = s;
    evals[threadIdx.x] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        // (blockDim.x, not the constant: a known trip count has both loops unrolled into 256 registers)
        uint32_t ev = 0;
#pragma unroll 1
        for (uint32_t i = 0; i < blockDim.x; ++i) ev += evals[i];
        total = flat_range_exclusive_scan(sums, blockDim.x, 0u);
        total_cmps = ev;
    }
    __syncthreads();
    flat_range_exclusive_scan(counts + c0, c1 - c0, sums[threadIdx.x]);
    const uint32_t written = total < a.out_cap ? total : a.out_cap;
    for (uint32_t i = written + threadIdx.x; i < a.out_cap; i += kFlatThreads) {
        a.out_ids[(uint64_t)qi * a.out_cap + i] = kEmpty;
        a.out_dists[(uint64_t)qi * a.out_cap + i] = __builtin_inff();
    }
    if (threadIdx.x == 0) {
        const bool over = a.out_cap != 0 && total > a.out_cap;
        a.out_counts[qi] = total;
        if (over) atomicOr(a.overflow, 1u);
        if (a.stats) {
            dann_search_stats st;
            st.cmps = total_cmps;
            st.hops = 0;
            st.result_count = total;
            st.status = over ? (uint32_t)(-DANN_EOVERFLOW) : 0u;
            st.written = written;
            a.stats[qi] = st;
        }
    }
}

}  // namespace

// One batch of queries (nq <= plan.p.batch) under a filter over slots [first, first + n), n > 0.
// `scratch`: plan.scratch_bytes().  d_filter: the bitmaps of these queries, `stride` words apart (0: one for all).
int32_t launch_flat_filtered_search(const IndexView& ix, const FlatFilteredPlan& plan, const void* d_queries, uint32_t nq,
                                    uint32_t first, uint32_t n, const uint32_t* d_deleted, const uint32_t* d_filter,
                                    uint64_t stride, void* scratch, uint32_t* d_ids, float* d_dists,
                                    dann_search_stats* d_stats, hipStream_t stream) {
    const FlatPlan& p = plan.p;
    FlatArgs a;
    a.queries = d_queries;
    a.nq = nq;
    a.first = first;
    a.n = n;
    a.k = p.k;
    a.chunk_rows = p.chunk_rows;
    a.nchunks = p.nchunks;
    a.tile = p.tile;
    a.cap = p.cap;
    a.qslot = flat_query_slot_bytes(ix);
    a.merge_cap = p.merge_cap;
    a.deleted = d_deleted;
    a.lists = reinterpret_cast<uint64_t*>(scratch);
    a.chunk_cmps = reinterpret_cast<uint32_t*>(a.lists + (size_t)p.batch * p.nchunks * p.k);
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.stats = d_stats;
    const FilterArg f{d_filter, stride};
    const uint32_t tiles = (nq + p.tile - 1) / p.tile;
    const int32_t rc = dispatch_row_op<kRowsQuery>(ix.dtype, ix.metric, [&](auto r) {
        using R = decltype(r);
        return launch_kernel<flat_filtered_scan_kernel<R::dt, R::op, R::norm>>(
            "flat_filtered_scan_kernel launch", dim3(p.nchunks, tiles), dim3(kFlatThreads), p.scan_lds, stream, ix, a, f);
    });
    if (rc == kNoRow) {
        set_error("dann_flat_filtered_search_batch: not defined on rows of dtype %d", ix.dtype);
        return DANN_EUNSUPPORTED;
    }
    if (rc != DANN_OK) return rc;
    return launch_flat_merge(ix, a, p.nchunks, p.merge_lds, stream);
}

// One batch of queries (nq <= plan.batch) of a range scan over slots [first, first + n) (n == 0: every result is empty).
// `scratch`: plan.scratch_bytes(); its last word is the call's overflow flag, which the caller clears before the first
// batch.  d_ids / d_dists may be null when out_cap is 0.
int32_t launch_flat_range_search(const IndexView& ix, const FlatRangePlan& plan, const void* d_queries, uint32_t nq,
                                 uint32_t first, uint32_t n, float radius, bool has_inner, float inner_radius,
                                 const uint32_t* d_deleted, const uint32_t* d_filter, uint64_t stride, uint32_t out_cap,
                                 void* scratch, uint32_t* d_ids, float* d_dists, uint32_t* d_counts,
                                 dann_search_stats* d_stats, hipStream_t stream) {
    RangeArgs a;
    a.queries = d_queries;
    a.nq = nq;
    a.first = first;
    a.n = n;
    a.chunk_rows = plan.chunk_rows;
    a.nchunks = plan.nchunks;
    a.tile = plan.tile;
    a.qslot = flat_query_slot_bytes(ix);
    a.deleted = d_deleted;
    a.filter = d_filter;
    a.filter_stride = stride;
    a.radius = radius;
    a.inner_radius = inner_radius;
    a.has_inner = has_inner ? 1u : 0u;
    a.out_cap = out_cap;
    a.counts = reinterpret_cast<uint32_t*>(scratch);
    a.cmps = a.counts + (size_t)plan.batch * plan.nchunks;
    a.overflow = flat_range_overflow_flag(plan, scratch);
    a.out_ids = d_ids;
    a.out_dists = d_dists;
    a.out_counts = d_counts;
    a.stats = d_stats;
    const dim3 grid(plan.nchunks, (nq + plan.tile - 1) / plan.tile);
    if (plan.nchunks) {
        const int32_t rc = dispatch_row_op<kRowsQuery>(ix.dtype, ix.metric, [&](auto r) {
            using R = decltype(r);
            return launch_kernel<flat_range_kernel<R::dt, R::op, R::norm, false>>("flat_range_kernel (count) launch", grid,
                                                                                  dim3(kFlatThreads), plan.lds, stream, ix, a);
        });
        if (rc == kNoRow) {
            set_error("dann_flat_range_search_batch: not defined on rows of dtype %d", ix.dtype);
            return DANN_EUNSUPPORTED;
        }
        if (rc != DANN_OK) return rc;
    }
    if (int32_t rc = launch_kernel<flat_range_offsets_kernel>("flat_range_offsets_kernel launch", dim3(nq), dim3(kFlatThreads),
                                                              0, stream, a))
        return rc;
    if (plan.nchunks == 0 || out_cap == 0) return DANN_OK;
    return dispatch_row_op<kRowsQuery>(ix.dtype, ix.metric, [&](auto r) {
        using R = decltype(r);
        return launch_kernel<flat_range_kernel<R::dt, R::op, R::norm, true>>("flat_range_kernel (write) launch", grid,
                                                                             dim3(kFlatThreads), plan.lds, stream, ix, a);
    });
}

}  // namespace dann
