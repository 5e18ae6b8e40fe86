// inplace_delete.hip -- in-place deletes (the neighbourhood repair at delete time) on the GPU.
//
// Replaces, for one minibatch of ids, the reference calls
//   DiskANNIndex::multi_inplace_delete          diskann/src/graph/index.rs:1338-1496 (n = 1: inplace_delete, 1500-1551)
//     get_candidates_using_onehop / _twohop_and_onehop   index.rs:1235-1336
//     inplace_delete_inner                      index.rs:1585-1747
//     add_edge_and_prune (to_remove = the ids)  index.rs:2264-2341, robust_prune_list 2397-2454
//     drop_adj_list                             index.rs:1060
//   DiskANNIndex::drop_deleted_neighbors        index.rs:1756-1816
//
// Every id of the call is marked deleted before any work list is built (dann.h), so the result does not depend on how
// the reference's tasks would have been scheduled.  Steps:
//   idel_mark_kernel    the ids into the deleted bitmap and a per-call bitmap; RETIRING tags on inline_tags indexes;
//   idel_search_kernel  VisitedAndTopK only: one wavefront per id, search_internal (beam width 1, L = l_value) with the
//                       deleted row as the query over NeighborPriorityQueue semantics in LDS, an exact visited bitmap,
//                       CopyIds output (start points kept, queue order);
//   idel_work_kernel    one wavefront per id: the live one-hop list (ballot + mbcnt compaction, list order); for
//                       TwoHopAndOneHop the two-hop union in first-occurrence order (open-addressing hash set in global
//                       memory, as cons_gather_kernel's global pools); the replace candidates; the in-neighbour test,
//                       16 lanes per candidate row;
//   idel_edge_kernel    one wavefront per id: for every in-neighbour and live out-neighbour s, d(s, r) over the replace
//                       candidates r != s with the distance groups of the prunes, the first num_to_replace under the tie
//                       order (DANN_TIE_POSITION: (distance, position); DANN_TIE_RUST: Rust's sort_unstable_by through
//                       rust_order.h), written as (source | id position | rank) keys to a global edge list;
//   hipcub radix sort   of the edge keys: each source's targets in call order, each id's targets in its own edge order;
//   idel_agg_kernel     one wavefront per distinct source: remove the call's ids, the deduplicated extend, then
//                       nothing / write / pool for robust_prune_list (unreadable ids and the source leave the pool);
//   prune_pools_into_rows (build_batch.hip)  the back-edge prune pipeline: row kernel, or sort + Gram tiles + sweep.
// Host synchronisations per call: five (the validation read of the deleted bitmap, the edge bound, the edge count, the
// source count and longest edge run, the final counters), two more with out_counters (dann_build_counters before and
// after), one more on a rolled-back error.  Every failure before step 4 removes the call's marks again; step 4 rewrites
// rows, and a HIP error there leaves the marks and the rows written so far.
// Sources are processed in chunks (the Gram scratch of the matrix-core path stays at the build's batch scale).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "dann_device.h"
#include "dann_internal.h"
#include "prune_common.h"
#include "rust_order.h"

namespace dann {
namespace {

constexpr uint32_t kMaxIds = 1u << 20;   // id positions are 20 bits of an edge key
constexpr uint32_t kWorkChunk = 256;     // ids per work-kernel launch of TwoHopAndOneHop (bounds the hash sets)
constexpr uint32_t kMaxTwoHopDegree = 256;  // TwoHopAndOneHop: the union of up to R + R^2 candidates per id
constexpr uint32_t kMaxL = 2048;         // VisitedAndTopK: the largest l_value (the queue lives in LDS)
// device counters: [0] in-neighbours, [1] replace candidates, [2] edge bound, [3] pair distances, [4] lists appended,
// [5] lists set without a prune, [6] lists pruned
constexpr uint32_t kStatWords = 8;

__device__ __forceinline__ bool unreadable(const IndexView& ix, const uint32_t* bm, uint32_t id) {
    if (id >= ix.nslots || in_bitmap(bm, id, ix.nslots)) return true;
    return ix.tag_off && ix.rows[(uint64_t)id * ix.row_stride + ix.tag_off] < kTagReadable;
}

// rust_order::sort_keys_unstable as a real call, as the search kernels hold it (search_kernel_impl.h)
__device__ __attribute__((noinline)) void idel_rust_sort(unsigned long long* keys, uint32_t n, void* work) {
    rust_order::sort_keys_unstable(keys, n, work);
}

struct MarkArgs {
    uint32_t* bm;
    uint32_t* callbm;
    const uint32_t* ids;
    uint32_t n;
    uint8_t* rows;
    uint64_t row_stride;
    uint32_t tag_off;
    const uint8_t* old_tags;  // unmark: the tags to restore (null = mark)
};

__global__ void idel_mark_kernel(MarkArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t s = a.ids[i];
    if (a.old_tags) {
        atomicAnd(&a.bm[s >> 5], ~(1u << (s & 31u)));
        if (a.tag_off) a.rows[(uint64_t)s * a.row_stride + a.tag_off] = a.old_tags[i];
        return;
    }
    atomicOr(&a.bm[s >> 5], 1u << (s & 31u));
    atomicOr(&a.callbm[s >> 5], 1u << (s & 31u));
    if (a.tag_off) a.rows[(uint64_t)s * a.row_stride + a.tag_off] = kTagRetiring;
}

struct IdelSearchArgs {
    IndexView ix;
    const uint32_t* bm;
    const uint32_t* ids;
    uint32_t lo;           // this launch: ids[lo + blockIdx.x]
    uint32_t l_value;
    uint32_t qcap;         // l_value + nstart: the queue's capacity and search_l (scratch.rs:199-207)
    uint32_t* visited;     // one bitmap of vwords words per block, cleared before the launch
    uint32_t vwords;
    uint32_t* out;         // n x l_value: CopyIds output, queue order, start points kept
    uint32_t* out_cnt;
};

// VisitedAndTopK's candidate search (get_candidates_using_visited_and_topk, index.rs:1168-1233): search_internal with
// beam width 1 and the deleted row as the query, over NeighborPriorityQueue semantics (queue.rs:130-318: lower-bound
// insert, a full queue drops a farther candidate, the cursor).  Unreadable slots are put into the visited set and then
// skipped (provider.rs:453-454).  Distances are the prunes' pair distances d(row, candidate).  One wavefront per id;
// the queue lives in LDS and is updated by one lane (inserts are sequential in the reference), the visited set is an
// exact bitmap over the slots.
template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void idel_search_kernel(IdelSearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x, p = a.lo + blockIdx.x, R = a.ix.max_degree, Q = a.qcap;
    float* qd = reinterpret_cast<float*>(smem);
    uint32_t* qi = reinterpret_cast<uint32_t*>(qd + Q);
    uint32_t* qv = qi + Q;
    uint32_t* nb = qv + Q;                             // max(R, 64)
    float* nd = reinterpret_cast<float*>(nb + max(R, 64u));
    uint32_t* st = reinterpret_cast<uint32_t*>(nd + max(R, 64u));  // [0] size, [1] cursor, [2] popped id
    uint32_t* vis = a.visited + (uint64_t)blockIdx.x * a.vwords;
    const uint32_t v = a.ids[p], nslots = a.ix.nslots;
    if (lane == 0) {
        st[0] = 0;
        st[1] = 0;
    }
    __syncthreads();
    auto insert = [&](uint32_t id, float d) {  // NeighborPriorityQueue::insert, by lane 0
        if (d != d) return;
        uint32_t n = st[0];
        if (n == Q && qd[n - 1] < d) return;
        uint32_t pos = 0;
        while (pos < n && qd[pos] < d) ++pos;
        if (n == Q) --n;
        for (uint32_t j = n; j > pos; --j) {
            qd[j] = qd[j - 1];
            qi[j] = qi[j - 1];
            qv[j] = qv[j - 1];
        }
        qd[pos] = d;
        qi[pos] = id;
        qv[pos] = 0;
        st[0] = n + 1;
        if (pos < st[1]) st[1] = pos;
    };
    // start_point_distances: the frozen slots, in order
    const uint32_t cap_nb = max(R, 64u);
    for (uint32_t s0 = 0; s0 < a.ix.nstart; s0 += cap_nb) {
        const uint32_t cnt = min(cap_nb, a.ix.nstart - s0);
        for (uint32_t j = lane; j < cnt; j += kWave) {
            const uint32_t sp = a.ix.capacity + s0 + j;
            nb[j] = sp;
            atomicOr(&vis[sp >> 5], 1u << (sp & 31u));
        }
        __syncthreads();
        fill_list_distances<DT, OP, NORM>(a.ix, v, nb, nd, cnt);
        __syncthreads();
        if (lane == 0)
            for (uint32_t j = 0; j < cnt; ++j) insert(nb[j], nd[j]);
        __syncthreads();
    }
    for (;;) {
        if (!(st[1] < st[0])) break;  // has_notvisited: cursor < min(search_l, size)
        __syncthreads();
        if (lane == 0) {  // closest_notvisited
            uint32_t cur = st[1];
            qv[cur] = 1;
            uint32_t c = cur + 1;
            while (c < st[0] && qv[c]) ++c;
            st[1] = c;
            st[2] = qi[cur];
        }
        __syncthreads();
        const uint32_t b = st[2];
        const uint32_t* row = a.ix.adj + (uint64_t)b * a.ix.adj_stride;
        const uint32_t len = min(row[0], R);
        uint32_t cnt = 0;
        for (uint32_t e0 = 0; e0 < len; e0 += kWave) {
            const uint32_t e = e0 + lane;
            const uint32_t id = e < len ? row[1 + e] : kEmpty;
            bool take = e < len && id < nslots;
            for (int k = 0; k < 64; ++k) {  // a repeated id: its first position inserts
                const uint32_t o = (uint32_t)__shfl((int)id, k);
                take &= !((uint32_t)k < lane && o == id);
            }
            if (take) {
                const uint32_t bit = 1u << (id & 31u);
                take = (atomicOr(&vis[id >> 5], bit) & bit) == 0u && !unreadable(a.ix, a.bm, id);
            }
            const uint64_t m = ballot64(take);
            if (take) nb[cnt + mbcnt(m)] = id;
            cnt += (uint32_t)__popcll(m);
        }
        __syncthreads();
        fill_list_distances<DT, OP, NORM>(a.ix, v, nb, nd, cnt);
        __syncthreads();
        if (lane == 0)
            for (uint32_t j = 0; j < cnt; ++j) insert(nb[j], nd[j]);
        __syncthreads();
    }
    // CopyIds: the first min(l_value, size) entries in queue order
    const uint32_t nout = min(a.l_value, st[0]);
    for (uint32_t i = lane; i < nout; i += kWave) a.out[(uint64_t)p * a.l_value + i] = qi[i];
    if (lane == 0) a.out_cnt[p] = nout;
}

constexpr auto kIdelSearch = [](auto r) { using R = decltype(r); return KernelOf<idel_search_kernel<R::dt, R::op, R::norm>>{}; };

struct WorkArgs {
    IndexView ix;
    const uint32_t* bm;
    const uint32_t* ids;   // the call's distinct ids
    uint32_t lo;           // this launch: ids[lo + blockIdx.x]
    uint32_t method;       // DANN_INPLACE_*
    uint32_t icap;         // in-neighbour candidates per id (stride of in_ids)
    uint32_t ntr;
    uint32_t k_value;      // VisitedAndTopK: replace candidates = the first k_value search results
    uint32_t rcap;         // stride of rc
    uint32_t* one;         // n x max_degree: the live one-hop list
    uint32_t* one_cnt;
    uint32_t* rc;          // n x rcap: the replace candidates
    uint32_t* rc_cnt;
    uint32_t* in_ids;      // n x icap: the candidates, compacted in place to the in-neighbours
    uint32_t* in_cnt;
    uint32_t* hash;        // twohop: kWorkChunk x (hmask + 1)
    uint32_t hmask;
    unsigned long long* stats;
    uint32_t* err;
};

__global__ __launch_bounds__(kWave) void idel_work_kernel(WorkArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* one_l = reinterpret_cast<uint32_t*>(smem);  // max_degree
    const uint32_t lane = threadIdx.x, p = a.lo + blockIdx.x;
    const uint32_t v = a.ids[p], R = a.ix.max_degree;
    const uint32_t* row = a.ix.adj + (uint64_t)v * a.ix.adj_stride;
    const uint32_t len = min(row[0], R);
    uint32_t n1 = 0;
    for (uint32_t e0 = 0; e0 < len; e0 += kWave) {
        const uint32_t e = e0 + lane;
        const uint32_t id = e < len ? row[1 + e] : kEmpty;
        const bool live = e < len && !unreadable(a.ix, a.bm, id);
        const uint64_t m = ballot64(live);
        if (live) one_l[n1 + mbcnt(m)] = id;
        n1 += (uint32_t)__popcll(m);
    }
    __syncthreads();
    for (uint32_t i = lane; i < n1; i += kWave) a.one[(uint64_t)p * R + i] = one_l[i];
    // the in-neighbour candidates
    uint32_t* cand = a.in_ids + (uint64_t)p * a.icap;
    uint32_t nc = 0, nrc = 0;
    uint32_t* rc = a.rc + (uint64_t)p * a.rcap;
    if (a.method == DANN_INPLACE_VISITED_AND_TOPK) {  // the candidates are the search results (idel_search_kernel)
        nc = a.in_cnt[p];
        nrc = min(a.k_value, nc);
        for (uint32_t i = lane; i < nrc; i += kWave) rc[i] = cand[i];
    } else if (a.method == DANN_INPLACE_ONE_HOP) {
        for (uint32_t i = lane; i < n1; i += kWave) cand[i] = one_l[i];
        nc = n1;
    } else {
        uint32_t* hash = a.hash + (uint64_t)blockIdx.x * (a.hmask + 1u);
        for (uint32_t i = lane; i <= a.hmask; i += kWave) hash[i] = kEmpty;
        __syncthreads();
        for (uint32_t k = 0; k < n1; ++k) {
            const uint32_t nb = one_l[k];
            nc = append_unique(cand, hash, a.hmask, nc, a.icap, lane == 0 ? nb : kEmpty, a.err);
            const uint32_t* nrow = a.ix.adj + (uint64_t)nb * a.ix.adj_stride;
            const uint32_t nlen = min(nrow[0], R);
            for (uint32_t e0 = 0; e0 < nlen; e0 += kWave) {
                const uint32_t e = e0 + lane;
                const uint32_t id = e < nlen ? nrow[1 + e] : kEmpty;
                const bool ok = e < nlen && !unreadable(a.ix, a.bm, id);
                nc = append_unique(cand, hash, a.hmask, nc, a.icap, ok ? id : kEmpty, a.err);
            }
        }
    }
    if (a.method != DANN_INPLACE_VISITED_AND_TOPK) {
        for (uint32_t i = lane; i < n1; i += kWave) rc[i] = one_l[i];
        nrc = n1;
    }
    __syncthreads();  // the candidates, written by every lane, are read by all of them below
    // return_refs_to_deleted_vertex: 16 lanes test one candidate's row for v; hits are compacted in candidate order
    const uint32_t g = lane >> 4, sl = lane & 15u;
    uint32_t nin = 0;
    for (uint32_t k0 = 0; k0 < nc; k0 += 4u) {
        const uint32_t k = k0 + g;
        bool found = false;
        uint32_t c = kEmpty;
        if (k < nc) {
            c = cand[k];
            const uint32_t* crow = a.ix.adj + (uint64_t)c * a.ix.adj_stride;
            const uint32_t clen = min(crow[0], R);
            for (uint32_t e = sl; e < clen; e += 16u) found |= crow[1 + e] == v;
        }
        const uint64_t m = ballot64(found);
        uint32_t hits = 0;
        for (uint32_t q = 0; q < 4u; ++q) hits |= ((m >> (16u * q)) & 0xFFFFull) ? (1u << q) : 0u;
        __syncthreads();  // every lane has read cand[k0 .. k0 + 4) before they are overwritten
        if (sl == 0 && ((hits >> g) & 1u)) cand[nin + __popc(hits & ((1u << g) - 1u))] = c;
        nin += (uint32_t)__popc(hits);
        __syncthreads();
    }
    if (lane == 0) {
        a.one_cnt[p] = n1;
        a.rc_cnt[p] = nrc;
        a.in_cnt[p] = nin;
        atomicAdd(&a.stats[0], (unsigned long long)nin);
        atomicAdd(&a.stats[1], (unsigned long long)nrc);
        // every in-neighbour is a source, with at least a marker entry (edges_to_add.insert of an empty list)
        atomicAdd(&a.stats[2], (unsigned long long)nin * max(min(a.ntr, nrc), 1u) + (unsigned long long)n1 * min(a.ntr, nrc));
    }
}

struct EdgeArgs {
    IndexView ix;
    const uint32_t* one;
    const uint32_t* one_cnt;
    const uint32_t* rc;
    const uint32_t* rc_cnt;
    uint32_t rcap;
    const uint32_t* in_ids;
    const uint32_t* in_cnt;
    uint32_t icap;
    uint32_t ntr;
    uint32_t tie_rust;
    unsigned long long* keys;  // edge list: (source << 32 | id position << 12 | rank), target
    uint32_t* vals;
    uint32_t* ecount;
    uint32_t ecap;
    unsigned long long* stats;
    uint32_t* err;
};

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void idel_edge_kernel(EdgeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t R = a.ix.max_degree, lane = threadIdx.x, p = blockIdx.x;
    const uint32_t C = a.rcap;
    uint32_t P = 64;
    while (P < C) P <<= 1;
    // LDS: [keys: P u64][work: kKeyWorkBytes][cand: C][pid: C][pd: C]
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
    void* work = smem + (size_t)P * 8u;
    uint32_t* cand = reinterpret_cast<uint32_t*>(smem + (size_t)P * 8u + rust_order::kKeyWorkBytes);
    uint32_t* pid = cand + C;
    float* pd = reinterpret_cast<float*>(pid + C);
    const uint32_t n1 = a.one_cnt[p], nin = a.in_cnt[p], nrc = a.rc_cnt[p];
    for (uint32_t i = lane; i < nrc; i += kWave) cand[i] = a.rc[(uint64_t)p * C + i];
    __syncthreads();
    const uint32_t* outs = a.one + (uint64_t)p * R;
    const uint32_t* ins = a.in_ids + (uint64_t)p * a.icap;
    unsigned long long ndist = 0;
    for (uint32_t si = 0; si < nin + n1; ++si) {
        const bool in_edge = si < nin;
        const uint32_t s = in_edge ? ins[si] : outs[si - nin];
        // the pool: the replace candidates other than s, in order
        uint32_t cnt = 0;
        for (uint32_t e0 = 0; e0 < nrc; e0 += kWave) {
            const uint32_t e = e0 + lane;
            const uint32_t r = e < nrc ? cand[e] : kEmpty;
            const bool take = e < nrc && r != s;
            const uint64_t m = ballot64(take);
            if (take) pid[cnt + mbcnt(m)] = r;
            cnt += (uint32_t)__popcll(m);
        }
        __syncthreads();
        const uint32_t keep = min(a.ntr, cnt);
        // an in-neighbour without a replacement still gets add_edge_and_prune (to drop its edge to the id): a marker
        const uint32_t emit = in_edge ? max(keep, 1u) : keep;
        if (emit == 0) continue;
        if (keep) {
            fill_list_distances<DT, OP, NORM>(a.ix, s, pid, pd, cnt);
            __syncthreads();
            ndist += cnt;
        }
        if (keep && a.tie_rust) {
            if (lane == 0) {
                for (uint32_t j = 0; j < cnt; ++j) keys[j] = dist_key(pd[j], j);
                idel_rust_sort(keys, cnt, work);
            }
        } else if (keep) {
            uint32_t Q = 64;
            while (Q < cnt) Q <<= 1;
            for (uint32_t j = lane; j < Q; j += kWave) keys[j] = j < cnt ? dist_key(pd[j], j) : ~0ull;
            __syncthreads();
            block_bitonic(keys, Q, kWave);
        }
        __syncthreads();
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(a.ecount, emit);
        base = (uint32_t)__shfl((int)base, 0);
        for (uint32_t t = lane; t < emit; t += kWave) {  // rank t (num_to_replace may exceed the wavefront)
            const uint32_t r = keep ? pid[(uint32_t)keys[t]] : kEmpty;
            const uint32_t src = in_edge ? s : r, tgt = in_edge ? r : s;
            const uint32_t local = in_edge ? t : C + (si - nin);
            if (base + t < a.ecap) {
                a.keys[base + t] = ((unsigned long long)src << 32) | ((unsigned long long)p << 12) | local;
                a.vals[base + t] = tgt;
            } else {
                atomicOr(a.err, 1u);
            }
        }
        __syncthreads();
    }
    if (lane == 0) atomicAdd(&a.stats[3], ndist);
}

constexpr auto kIdelEdge = [](auto r) { using R = decltype(r); return KernelOf<idel_edge_kernel<R::dt, R::op, R::norm>>{}; };

// the first edge of every source: heads (unordered) and the largest number of edges of one source
__global__ void idel_heads_kernel(const unsigned long long* keys, uint32_t E, uint32_t* heads, uint32_t* meta) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool head = i < E && (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32));
    uint32_t t = 0;
    if (head) {
        const unsigned long long src = keys[i] >> 32;
        while (i + t < E && (keys[i + t] >> 32) == src) ++t;
    }
    wave_push(head, heads, &meta[0], i);
    if (head) atomicMax(&meta[1], t);
}

struct AggArgs {
    IndexView ix;
    const uint32_t* bm;
    const uint32_t* callbm;
    const unsigned long long* keys;
    const uint32_t* vals;
    uint32_t E;
    const uint32_t* heads;
    uint32_t lo;
    uint32_t max_degree;  // cfg->max_degree: max_degree_with_slack
    uint32_t pcap;
    uint32_t* locs;
    uint32_t* pool_ids;
    float* pool_d;
    uint32_t* counts;
    unsigned long long* stats;
};

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void idel_agg_kernel(AggArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* list = reinterpret_cast<uint32_t*>(smem);  // pcap
    const uint32_t lane = threadIdx.x, wi = blockIdx.x, R = a.ix.max_degree;
    const uint32_t h = a.heads[a.lo + wi];
    const uint32_t src = (uint32_t)(a.keys[h] >> 32);
    uint32_t* row = a.ix.adj + (uint64_t)src * a.ix.adj_stride;
    const uint32_t len = min(row[0], R);
    // retain: drop the ids of this call
    uint32_t cnt = 0;
    bool removed = false;
    for (uint32_t e0 = 0; e0 < len; e0 += kWave) {
        const uint32_t e = e0 + lane;
        const uint32_t id = e < len ? row[1 + e] : kEmpty;
        const bool rem = e < len && in_bitmap(a.callbm, id, a.ix.nslots);
        const bool keep = e < len && !rem;
        removed |= ballot64(rem) != 0ull;
        const uint64_t m = ballot64(keep);
        if (keep) list[cnt + mbcnt(m)] = id;
        cnt += (uint32_t)__popcll(m);
    }
    __syncthreads();
    // extend_from_slice: each target not yet in the list is appended, in edge order
    uint32_t added = 0;
    for (uint32_t i = h; i < a.E && (uint32_t)(a.keys[i] >> 32) == src; ++i) {
        const uint32_t t = a.vals[i];
        if (t == kEmpty) continue;  // the marker of an in-neighbour without replacements
        bool present = false;
        for (uint32_t j = lane; j < cnt; j += kWave) present |= list[j] == t;
        if (ballot64(present) == 0ull) {
            if (lane == 0) list[cnt] = t;
            ++cnt;
            ++added;
            __syncthreads();
        }
    }
    if (added == 0 && !removed) {
        if (lane == 0) a.counts[wi] = 0;
        return;
    }
    if (cnt <= a.max_degree) {  // set_neighbors / append_vector: the row becomes the list either way
        for (uint32_t i = lane; i < cnt; i += kWave) row[1 + i] = list[i];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            row[0] = cnt;
            a.counts[wi] = 0;
            atomicAdd(&a.stats[removed ? 5 : 4], 1ull);
        }
        return;
    }
    // robust_prune_list: the source and unreadable ids leave the pool (view.get is None for them)
    uint32_t pc = 0;
    for (uint32_t e0 = 0; e0 < cnt; e0 += kWave) {
        const uint32_t e = e0 + lane;
        const uint32_t id = e < cnt ? list[e] : kEmpty;
        const bool keep = e < cnt && id != src && !unreadable(a.ix, a.bm, id);
        const uint64_t m = ballot64(keep);
        __syncthreads();
        if (keep) list[pc + mbcnt(m)] = id;
        pc += (uint32_t)__popcll(m);
        __syncthreads();
    }
    if (lane == 0) atomicAdd(&a.stats[6], 1ull);
    if (pc == 0) {  // nothing to occlude: the pruned list is empty
        if (lane == 0) {
            row[0] = 0;
            a.counts[wi] = 0;
        }
        return;
    }
    uint32_t* gid = a.pool_ids + (uint64_t)wi * a.pcap;
    float* gd = a.pool_d + (uint64_t)wi * a.pcap;
    for (uint32_t i = lane; i < pc; i += kWave) gid[i] = list[i];
    fill_list_distances<DT, OP, NORM>(a.ix, src, list, gd, pc);
    if (lane == 0) {
        a.locs[wi] = src;
        a.counts[wi] = pc;
    }
}

constexpr auto kIdelAgg = [](auto r) { using R = decltype(r); return KernelOf<idel_agg_kernel<R::dt, R::op, R::norm>>{}; };

__global__ void idel_drop_lists_kernel(IndexView ix, const uint32_t* ids, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ix.adj[(uint64_t)ids[i] * ix.adj_stride] = 0;
}

struct DropArgs {
    IndexView ix;
    const uint32_t* bm;
    const uint32_t* ids;  // null = item i is slot i
    uint32_t only_orphans;
    uint32_t pruned_degree;
    uint8_t* kinds;
};

// drop_deleted_neighbors, one wavefront per vertex.  A vertex's rewrite reads its own list and the lengths of its deleted
// neighbours' lists, and a deleted vertex is never rewritten: the batch equals the sequential loop.
__global__ __launch_bounds__(kWave) void idel_drop_kernel(DropArgs a, uint32_t n) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* pool = reinterpret_cast<uint32_t*>(smem);  // max_degree
    const uint32_t lane = threadIdx.x, item = blockIdx.x, R = a.ix.max_degree;
    if (item >= n) return;
    const uint32_t v = a.ids ? a.ids[item] : item;
    if (unreadable(a.ix, a.bm, v)) {
        if (lane == 0) a.kinds[item] = (uint8_t)DANN_CONSOLIDATE_DELETED;
        return;
    }
    if (lane == 0) a.kinds[item] = (uint8_t)DANN_CONSOLIDATE_COMPLETE;
    uint32_t* row = a.ix.adj + (uint64_t)v * a.ix.adj_stride;
    const uint32_t len = min(row[0], R);
    uint32_t cnt = 0, ndel = 0;
    for (uint32_t e0 = 0; e0 < len; e0 += kWave) {
        const uint32_t e = e0 + lane;
        const uint32_t id = e < len ? row[1 + e] : kEmpty;
        const bool del = e < len && unreadable(a.ix, a.bm, id);
        const bool live = e < len && !del;
        const uint64_t m = ballot64(live);
        if (live) pool[cnt + mbcnt(m)] = id;
        cnt += (uint32_t)__popcll(m);
        ndel += (uint32_t)__popcll(ballot64(del));
    }
    if (a.only_orphans && ndel) {  // deleted neighbours whose own list is still present, after the live ones
        for (uint32_t e0 = 0; e0 < len; e0 += kWave) {
            const uint32_t e = e0 + lane;
            const uint32_t id = e < len ? row[1 + e] : kEmpty;
            const bool keep = e < len && unreadable(a.ix, a.bm, id) && id < a.ix.nslots &&
                              a.ix.adj[(uint64_t)id * a.ix.adj_stride] != 0u;
            const uint64_t m = ballot64(keep);
            if (keep) pool[cnt + mbcnt(m)] = id;
            cnt += (uint32_t)__popcll(m);
        }
    }
    __syncthreads();
    if (ndel == 0 && cnt <= a.pruned_degree) return;
    for (uint32_t i = lane; i < cnt; i += kWave) row[1 + i] = pool[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) row[0] = cnt;
}

}  // namespace
}  // namespace dann

using namespace dann;

extern "C" {

int32_t dann_inplace_delete(dann_index* idx, const dann_build_config* cfg, const uint32_t* ids, uint32_t n,
                            const dann_inplace_delete_params* prm, uint64_t* out_counters) try {
    if (!idx || !cfg || !prm) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    if (int32_t rc = check_build_cfg(idx, cfg, "dann_inplace_delete", false)) return rc;
    if (prm->method > DANN_INPLACE_ONE_HOP) {
        set_error("dann_inplace_delete: unknown method %u", prm->method);
        return DANN_EINVAL;
    }
    const bool vtk = prm->method == DANN_INPLACE_VISITED_AND_TOPK;
    const uint32_t R = idx->cfg.max_degree;
    const bool twohop = prm->method == DANN_INPLACE_TWO_HOP_AND_ONE_HOP;
    // replace candidates per id: the live one-hop list, or the first k_value search results
    const uint32_t rcap = vtk ? std::max<uint32_t>(std::min(prm->k_value, prm->l_value), 1u) : std::max<uint32_t>(R, 1u);
    if (vtk && (prm->k_value == 0 || prm->l_value == 0 || prm->l_value > kMaxL)) {
        set_error("dann_inplace_delete: VisitedAndTopK needs k_value > 0 and 0 < l_value <= %u", kMaxL);
        return DANN_EINVAL;
    }
    if (out_counters) memset(out_counters, 0, sizeof(uint64_t) * DANN_INPLACE_COUNTERS);
    if (n == 0) return DANN_OK;
    if (!ids || n > kMaxIds) {
        set_error("dann_inplace_delete: %s", ids ? "more than 2^20 ids in one call" : "ids is NULL");
        return DANN_EINVAL;
    }
    if (rcap + R > 4096u || (twohop && R > kMaxTwoHopDegree)) {
        set_error("dann_inplace_delete: max_degree %u is not supported by this method", R);
        return DANN_EUNSUPPORTED;
    }
    // validation, before anything changes: range, start points, earlier deletes; a repeat counts once
    for (uint32_t i = 0; i < n; ++i)
        if (ids[i] >= idx->nslots) {
            set_error("dann_inplace_delete: id %u out of bounds (%u slots)", ids[i], idx->nslots);
            return DANN_EBOUNDS;
        }
    for (uint32_t i = 0; i < n; ++i)
        if (ids[i] >= idx->cfg.capacity) {
            set_error("dann_inplace_delete: id %u is a start point (frozen, cannot be deleted)", ids[i]);
            return DANN_EINVAL;
        }
    DeviceGuard guard(idx->device);
    hipStream_t st = idx->main.stream;
    const uint32_t words = (idx->nslots + 31u) / 32u;
    std::vector<uint32_t> h_bm(words, 0u);
    if (idx->d_deleted) {
        DANN_HIP(hipMemcpyAsync(h_bm.data(), idx->d_deleted, (size_t)words * 4, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
    }
    std::vector<uint32_t> uid;
    uid.reserve(n);
    {
        std::vector<uint32_t> seen(words, 0u);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t s = ids[i];
            if ((h_bm[s >> 5] >> (s & 31u)) & 1u) {
                set_error("dann_inplace_delete: id %u was already deleted", s);
                return DANN_EINVAL;
            }
            if ((seen[s >> 5] >> (s & 31u)) & 1u) continue;
            seen[s >> 5] |= 1u << (s & 31u);
            uid.push_back(s);
        }
    }
    const uint32_t nu = (uint32_t)uid.size();
    if (int32_t rc = ensure_deleted_bitmap(idx)) return rc;
    const IndexView ix = idx->view();
    // in-neighbour candidates per id; the two-hop union holds at most R + R^2 distinct ids, and never more than the slots
    const uint32_t icap = vtk ? prm->l_value : twohop ? std::min<uint32_t>(R + R * R, idx->nslots) : std::max<uint32_t>(R, 1u);
    const uint32_t ntr = std::min<uint32_t>(prm->num_to_replace, rcap);
    uint64_t bc0[11] = {};
    if (out_counters) {
        if (int32_t rc = dann_build_counters(idx, bc0, 11)) return rc;
    }
    std::vector<uint8_t> old_tags(nu, 0);
    if (idx->cfg.inline_tags)
        for (uint32_t i = 0; i < nu; ++i) old_tags[i] = idx->h_tags[uid[i]];

    // everything sized by the call alone is allocated before the marks
    const uint32_t hmask = twohop ? pow2_at_least(2u * icap) - 1u : 0u;
    const uint32_t wchunk = twohop ? std::min(kWorkChunk, nu) : nu;
    const uint32_t schunk = vtk ? (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>({nu, 1024u, (256ull << 20) / ((uint64_t)words * 4)})) : 0u;
    DevBuf d_ids, d_callbm, d_one, d_one_cnt, d_rc, d_rc_cnt, d_in, d_in_cnt, d_hash, d_vis, d_meta, d_stats, d_old;
    DANN_HIP(d_ids.alloc((size_t)nu * 4));
    DANN_HIP(hipMemcpyAsync(d_ids.p, uid.data(), (size_t)nu * 4, hipMemcpyHostToDevice, st));
    DANN_HIP(d_callbm.alloc((size_t)words * 4));
    DANN_HIP(hipMemsetAsync(d_callbm.p, 0, (size_t)words * 4, st));
    DANN_HIP(d_one.alloc((size_t)nu * R * 4));
    DANN_HIP(d_one_cnt.alloc((size_t)nu * 4));
    DANN_HIP(d_rc.alloc((size_t)nu * rcap * 4));
    DANN_HIP(d_rc_cnt.alloc((size_t)nu * 4));
    DANN_HIP(d_in.alloc((size_t)nu * icap * 4));
    DANN_HIP(d_in_cnt.alloc((size_t)nu * 4));
    if (twohop) DANN_HIP(d_hash.alloc((size_t)wchunk * (hmask + 1u) * 4));
    if (vtk) DANN_HIP(d_vis.alloc((size_t)schunk * words * 4));
    DANN_HIP(d_meta.alloc(64));
    DANN_HIP(hipMemsetAsync(d_meta.p, 0, 64, st));
    DANN_HIP(d_stats.alloc(kStatWords * 8));
    DANN_HIP(hipMemsetAsync(d_stats.p, 0, kStatWords * 8, st));
    DANN_HIP(d_old.alloc(nu));
    DANN_HIP(hipMemcpyAsync(d_old.p, old_tags.data(), nu, hipMemcpyHostToDevice, st));
    uint32_t* meta = d_meta.as<uint32_t>();  // [0] edge count, [1] heads, [2] largest edge run, [3] error word
    unsigned long long* stats = d_stats.as<unsigned long long>();

    // 1. deletion comes first
    MarkArgs ma{idx->d_deleted, d_callbm.as<uint32_t>(), d_ids.as<uint32_t>(), nu, idx->d_rows,
                (uint64_t)idx->cfg.row_stride, idx->cfg.inline_tags ? idx->layer_bytes : 0u, nullptr};
    hipLaunchKernelGGL(idel_mark_kernel, dim3((nu + 255u) / 256u), dim3(256), 0, st, ma);
    DANN_HIP(hipGetLastError());
    if (ma.tag_off)
        for (uint32_t i = 0; i < nu; ++i) idx->h_tags[uid[i]] = kTagRetiring;
    auto unmark = [&]() {  // an error before any row is written: the call leaves the index as it found it
        MarkArgs ua = ma;
        ua.old_tags = d_old.as<uint8_t>();
        hipLaunchKernelGGL(idel_mark_kernel, dim3((nu + 255u) / 256u), dim3(256), 0, st, ua);
        (void)hipStreamSynchronize(st);
        if (ma.tag_off)
            for (uint32_t i = 0; i < nu; ++i) idx->h_tags[uid[i]] = old_tags[i];
    };

    // 2. - 3. work lists, replacement edges, the sort: no row is written yet, so every failure is rolled back
    DevBuf d_keys, d_keys2, d_vals, d_vals2, d_heads, d_tmp;
    uint32_t E = 0, h_meta[4] = {0, 0, 0, 0};
    auto prepare = [&]() -> int32_t {
        if (vtk) {
            IdelSearchArgs sa;
            sa.ix = ix;
            sa.bm = idx->d_deleted;
            sa.ids = d_ids.as<uint32_t>();
            sa.l_value = prm->l_value;
            sa.qcap = prm->l_value + ix.nstart;
            sa.visited = d_vis.as<uint32_t>();
            sa.vwords = words;
            sa.out = d_in.as<uint32_t>();
            sa.out_cnt = d_in_cnt.as<uint32_t>();
            const size_t lds = (size_t)sa.qcap * 12u + (size_t)std::max<uint32_t>(R, 64u) * 8u + 16u;
            for (uint32_t lo = 0; lo < nu; lo += schunk) {
                const uint32_t m = std::min(schunk, nu - lo);
                sa.lo = lo;
                DANN_HIP(hipMemsetAsync(d_vis.p, 0, (size_t)m * words * 4, st));
                if (int32_t rc = launch_rows(ix, kIdelSearch, "idel_search_kernel launch", sa, m, lds, st)) return rc;
            }
        }
        WorkArgs wa;
        wa.ix = ix;
        wa.bm = idx->d_deleted;
        wa.ids = d_ids.as<uint32_t>();
        wa.method = prm->method;
        wa.icap = icap;
        wa.ntr = ntr;
        wa.k_value = prm->k_value;
        wa.rcap = rcap;
        wa.one = d_one.as<uint32_t>();
        wa.one_cnt = d_one_cnt.as<uint32_t>();
        wa.rc = d_rc.as<uint32_t>();
        wa.rc_cnt = d_rc_cnt.as<uint32_t>();
        wa.in_ids = d_in.as<uint32_t>();
        wa.in_cnt = d_in_cnt.as<uint32_t>();
        wa.hmask = hmask;
        wa.hash = d_hash.as<uint32_t>();
        wa.stats = stats;
        wa.err = meta + 3;
        for (uint32_t lo = 0; lo < nu; lo += wchunk) {
            wa.lo = lo;
            hipLaunchKernelGGL(idel_work_kernel, dim3(std::min(wchunk, nu - lo)), dim3(kWave), (size_t)R * 4, st, wa);
            DANN_HIP(hipGetLastError());
        }
        unsigned long long h_bound = 0;
        DANN_HIP(hipMemcpyAsync(&h_bound, stats + 2, 8, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
        if (h_bound >= (1ull << 31)) {  // the radix sort counts items in an int
            set_error("dann_inplace_delete: %llu replacement edges in one call: split the minibatch", h_bound);
            return DANN_EUNSUPPORTED;
        }
        const uint32_t ecap = (uint32_t)h_bound;
        DANN_HIP(d_keys.alloc((size_t)ecap * 8));
        DANN_HIP(d_keys2.alloc((size_t)ecap * 8));
        DANN_HIP(d_vals.alloc((size_t)ecap * 4));
        DANN_HIP(d_vals2.alloc((size_t)ecap * 4));
        EdgeArgs ea;
        ea.ix = ix;
        ea.one = wa.one;
        ea.one_cnt = wa.one_cnt;
        ea.rc = wa.rc;
        ea.rc_cnt = wa.rc_cnt;
        ea.rcap = rcap;
        ea.in_ids = wa.in_ids;
        ea.in_cnt = wa.in_cnt;
        ea.icap = icap;
        ea.ntr = ntr;
        ea.tie_rust = idx->prune_tie_order == DANN_TIE_RUST ? 1u : 0u;
        ea.keys = d_keys.as<unsigned long long>();
        ea.vals = d_vals.as<uint32_t>();
        ea.ecount = meta + 0;
        ea.ecap = ecap;
        ea.stats = stats;
        ea.err = meta + 3;
        const size_t edge_lds = (size_t)pow2_at_least(rcap) * 8 + rust_order::kKeyWorkBytes + (size_t)3 * rcap * 4;
        if (int32_t rc = launch_rows(ix, kIdelEdge, "idel_edge_kernel launch", ea, nu, edge_lds, st)) return rc;
        DANN_HIP(hipMemcpyAsync(&E, meta + 0, 4, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
        E = std::min(E, ecap);
        if (E) {
            int end_bit = 32;
            while ((1ull << (end_bit - 32)) < idx->nslots) ++end_bit;
            size_t tmp = 0;
            DANN_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, ea.keys, d_keys2.as<unsigned long long>(), ea.vals,
                                                        d_vals2.as<uint32_t>(), (int)E, 0, end_bit, st));
            DANN_HIP(d_tmp.alloc(tmp));
            DANN_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tmp, ea.keys, d_keys2.as<unsigned long long>(), ea.vals,
                                                        d_vals2.as<uint32_t>(), (int)E, 0, end_bit, st));
            DANN_HIP(d_heads.alloc((size_t)E * 4));
            hipLaunchKernelGGL(idel_heads_kernel, dim3((E + 255u) / 256u), dim3(256), 0, st,
                               d_keys2.as<unsigned long long>(), E, d_heads.as<uint32_t>(), meta + 1);
            DANN_HIP(hipGetLastError());
        }
        DANN_HIP(hipMemcpyAsync(h_meta, meta, 16, hipMemcpyDeviceToHost, st));
        DANN_HIP(hipStreamSynchronize(st));
        if (h_meta[3]) {
            set_error("dann_inplace_delete: a work list outgrew its bound");
            return DANN_EINTERNAL;
        }
        if (h_meta[1] && pow2_at_least(R + h_meta[2]) > kMaxPool) {
            set_error("dann_inplace_delete: a vertex would receive %u new edges in one call (pool > %u): split the "
                      "minibatch", h_meta[2], kMaxPool);
            return DANN_EUNSUPPORTED;
        }
        return DANN_OK;
    };
    if (int32_t rc = prepare()) {
        unmark();
        return rc;
    }
    const uint32_t nsrc = h_meta[1];
    const uint32_t pcap = pow2_at_least(R + h_meta[2]);

    // 4. add_edge_and_prune per distinct source, in chunks.  From here on rows are rewritten: a failure (a HIP error)
    // leaves the marks and the rows written so far.
    if (nsrc) {
        const uint32_t chunk = std::min<uint32_t>(nsrc, prune_pools_use_gram(idx) ? 2048u : 8192u);
        DevBuf c_locs, c_ids, c_d, c_cnt;
        DANN_HIP(c_locs.alloc((size_t)chunk * 4));
        DANN_HIP(hipMemsetAsync(c_locs.p, 0, (size_t)chunk * 4, st));
        DANN_HIP(c_ids.alloc((size_t)chunk * pcap * 4));
        DANN_HIP(c_d.alloc((size_t)chunk * pcap * 4));
        DANN_HIP(c_cnt.alloc((size_t)chunk * 4));
        AggArgs ga;
        ga.ix = ix;
        ga.bm = idx->d_deleted;
        ga.callbm = d_callbm.as<uint32_t>();
        ga.keys = d_keys2.as<unsigned long long>();
        ga.vals = d_vals2.as<uint32_t>();
        ga.E = E;
        ga.heads = d_heads.as<uint32_t>();
        ga.max_degree = cfg->max_degree;
        ga.pcap = pcap;
        ga.locs = c_locs.as<uint32_t>();
        ga.pool_ids = c_ids.as<uint32_t>();
        ga.pool_d = c_d.as<float>();
        ga.counts = c_cnt.as<uint32_t>();
        ga.stats = stats;
        for (uint32_t lo = 0; lo < nsrc; lo += chunk) {
            const uint32_t m = std::min(chunk, nsrc - lo);
            ga.lo = lo;
            if (int32_t rc = launch_rows(ix, kIdelAgg, "idel_agg_kernel launch", ga, m, (size_t)pcap * 4, st)) return rc;
            bool used_gram = false;
            if (int32_t rc = prune_pools_into_rows(idx, *cfg, ga.locs, ga.pool_ids, ga.pool_d, ga.counts, pcap, m, &used_gram))
                return rc;
        }
    }
    // 5. drop the lists of the call's ids
    hipLaunchKernelGGL(idel_drop_lists_kernel, dim3((nu + 255u) / 256u), dim3(256), 0, st, ix, d_ids.as<uint32_t>(), nu);
    DANN_HIP(hipGetLastError());
    unsigned long long h_stats[kStatWords] = {};
    DANN_HIP(hipMemcpyAsync(h_stats, stats, sizeof(h_stats), hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    if (out_counters) {
        uint64_t bc1[11] = {};
        if (int32_t rc = dann_build_counters(idx, bc1, 11)) return rc;
        out_counters[0] = nu;
        out_counters[1] = h_stats[0];
        out_counters[2] = h_stats[1];
        out_counters[3] = h_stats[3];
        out_counters[4] = nsrc;
        out_counters[5] = h_stats[4];
        out_counters[6] = h_stats[5];
        out_counters[7] = h_stats[6];
        out_counters[8] = bc1[0] - bc0[0];  // the sweep of the matrix-core path counts every prune it runs
    }
    return DANN_OK;
} DANN_CATCH_ALL

int32_t dann_drop_deleted_neighbors(dann_index* idx, const dann_build_config* cfg, const uint32_t* ids, uint32_t n,
                                    uint32_t only_orphans, int32_t* out_kind) try {
    if (!idx || !cfg) return DANN_EINVAL;
    ::dann::ExclusiveGuard lock(idx);
    DANN_MUTATION(idx);
    if (cfg->pruned_degree == 0 || only_orphans > 1u) {
        set_error("dann_drop_deleted_neighbors: invalid config (pruned_degree %u, only_orphans %u)", cfg->pruned_degree,
                  only_orphans);
        return DANN_EINVAL;
    }
    // a repeated id is done once (a second pass over a vertex changes nothing and gives the same kind)
    std::vector<uint32_t> uid, pos;
    if (ids) {
        if (n == 0) return DANN_OK;
        for (uint32_t i = 0; i < n; ++i)
            if (ids[i] >= idx->nslots) {
                set_error("dann_drop_deleted_neighbors: id %u out of bounds (%u slots)", ids[i], idx->nslots);
                return DANN_EBOUNDS;
            }
        std::unordered_map<uint32_t, uint32_t> at;
        at.reserve(n * 2u);
        pos.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
            auto it = at.emplace(ids[i], (uint32_t)uid.size());
            if (it.second) uid.push_back(ids[i]);
            pos[i] = it.first->second;
        }
    } else {
        n = idx->nslots;
    }
    const uint32_t m = ids ? (uint32_t)uid.size() : n;
    DeviceGuard guard(idx->device);
    hipStream_t st = idx->main.stream;
    const IndexView ix = idx->view();
    DevBuf d_ids, d_kinds;
    if (ids) {
        DANN_HIP(d_ids.alloc((size_t)m * 4));
        DANN_HIP(hipMemcpyAsync(d_ids.p, uid.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    }
    DANN_HIP(d_kinds.alloc(m));
    DropArgs da{ix, idx->d_deleted, ids ? d_ids.as<uint32_t>() : nullptr, only_orphans, cfg->pruned_degree,
                d_kinds.as<uint8_t>()};
    const size_t lds = (size_t)ix.max_degree * 4;
    if (int32_t rc = launch_kernel<idel_drop_kernel>("hipGetLastError()", dim3(m), dim3(kWave), lds, st, da, m)) return rc;
    std::vector<uint8_t> h_kinds(out_kind ? m : 0);
    if (out_kind) DANN_HIP(hipMemcpyAsync(h_kinds.data(), d_kinds.p, m, hipMemcpyDeviceToHost, st));
    DANN_HIP(hipStreamSynchronize(st));
    if (out_kind)
        for (uint32_t i = 0; i < n; ++i) out_kind[i] = h_kinds[ids ? pos[i] : i];
    return DANN_OK;
} DANN_CATCH_ALL

}  // extern "C"
