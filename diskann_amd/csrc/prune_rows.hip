// prune_rows.hip -- RobustPrune on the row kernels, and the graph update of a batched Vamana insert.
//
// Replaces, for a batch of new points, the reference call chain
//   DiskANNIndex::multi_insert                 diskann/src/graph/index.rs:815-1030
//     search_and_prune (beam 1, L = l_build)   index.rs:349-434  (search: search_kernels.hip)
//     robust_prune_with                        index.rs:2476-2532
//       SortedNeighbors::new                   graph/internal/sorted_neighbors.rs:26-44
//       occlude_list                           index.rs:2565-2650
//       prune::robust_prune                    graph/internal/prune.rs:106-259
//       PruneKind::update_occlude_factor       graph/config/mod.rs:80-103
//     aggregate_backedges                      index.rs:123-143
//     multi_insert_bootstrap_leaf              index.rs:597-645
//     set_neighbors_bulk                       index.rs:948-962
//     add_edge_and_prune / robust_prune_list   index.rs:2264-2341, 2397-2454
// with the adjacency lists it produces identical to the CPU restatement -- and, by default, to the
// reference itself on pools with EQUAL distances as well: such a pool is put in the order the reference's
// own select_nth_unstable_by + sort_unstable_by leave it in (rust_order.h, dann_set_prune_tie_order).
// (build_batch.hip drives the batch; prune_gram.hip is the same prune with its pair distances from the matrix cores.)
//
// One wavefront owns one point.  The candidate pool is sorted in LDS (bitonic, 64-bit
// keys = order-preserving distance bits : pool position; a pool whose sorted keys show equal
// distances is then walked by one lane, rust_order_by_lane0).  The alpha sweep keeps 64/G
// candidates in flight, one per G-lane distance group (the same bit-exact groups as the
// search path): each walks the selected list in the reference's order, is rejected at the
// first entry that pushes its factor past alpha, and is selected only once it is the oldest
// candidate in flight and has seen the whole list -- so `last_checked`, and with it the
// inner-product "Occluding" rule that depends on *when* a pair is evaluated, are reproduced
// exactly, and no distance is evaluated that the sequential sweep would not evaluate
// (prune_sorted_pool; rounds 1-4 visited one candidate at a time with 64/G speculative
// distances per round and were bound by the scalar unit: profiles/r05_prune_counters.txt).
#include "prune_rows.h"

namespace dann {
namespace {

// Sort pid/pd[0..P) (already in LDS) by (distance, position), truncate to max_occlusion,
// run occlude_list for `location` and write [len, ids...] to `out`.
template <int DT, int OP, bool NORM>
__device__ void prune_sorted_pool(const IndexView& ix, const PruneCfg& cfg, uint32_t location, uint32_t P,
                                  uint32_t pcap, uint8_t* smem, const PoolLds& L, bool force_saturate, uint32_t* out) {
    using S = Scheme<DT, OP, true>;
    constexpr int G = S::G;
    const uint32_t lane = threadIdx.x;
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem + L.keys_off);
    const uint32_t* pid = reinterpret_cast<const uint32_t*>(smem + L.pid_off);
    const float* pd = reinterpret_cast<const float*>(smem + L.pd_off);
    uint32_t* sid = reinterpret_cast<uint32_t*>(smem + L.sid_off);
    float* sd = reinterpret_cast<float*>(smem + L.sd_off);
    float* occ = reinterpret_cast<float*>(smem + L.occ_off);
    uint16_t* last = reinterpret_cast<uint16_t*>(smem + L.last_off);
    uint32_t* sel = reinterpret_cast<uint32_t*>(smem + L.sel_off);

    // ---- SortedNeighbors::new -------------------------------------------------------
    bool saw_nan = false;
    for (uint32_t i = lane; i < pcap; i += kWave) {
        const float d = i < P ? pd[i] : 0.0f;
        saw_nan |= d != d;
        keys[i] = i < P ? dist_key(d, i) : ~0ull;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= pcap; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < (pcap >> 1); t += kWave) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
                const uint32_t p = i | j;
                const uint64_t a = keys[i], b = keys[p];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    keys[i] = b;
                    keys[p] = a;
                }
            }
            __syncthreads();
        }
    }
    // DANN_TIE_RUST: a pool with equal (or unordered) distances is ordered by the reference's own sort instead
    const bool rust = cfg.tie_order != 0 && pool_has_ties(keys, P, saw_nan);
    if (rust) {
        __syncthreads();
        rust_order_by_lane0(cfg, P, smem, L);
        __syncthreads();
    }
    const uint32_t N = P < cfg.max_occlusion ? P : cfg.max_occlusion;
    for (uint32_t i = lane; i < N; i += kWave) {
        const uint32_t pos = rust ? (uint32_t)last[i] : (uint32_t)keys[i];
        const uint32_t id = pid[pos];
        sid[i] = id;
        sd[i] = pd[pos];
        occ[i] = (id == location || id >= ix.nslots) ? 3.402823466e+38f : 0.0f;  // excluded / not retrievable: never visited
        last[i] = 0;
    }
    __syncthreads();

    // ---- prune::robust_prune ----------------------------------------------------------
    const uint32_t degree = cfg.pruned_degree;
    const bool occluding = (ix.metric == M_IP);  // PruneKind::from_metric (config/mod.rs:69-75)
    const float alpha = cfg.alpha;
    const float inc = alpha < 1.2f ? alpha : 1.2f;
    float cur_alpha = 1.0f;
    uint32_t found = 0, npairs = 0;
    const int g = lane / G, v = lane % G;
    // The reference visits the sorted candidates one after another, each against the entries selected so far
    // (prune.rs:196-232).  Here GROUPS of them are in flight at once, one per lane group, each walking sel[] on its
    // own, one entry per step of the wave:
    //   * candidates are handed out in list order (the pass's worklist: those whose factor does not exceed cur_alpha);
    //   * a candidate is REJECTED as soon as its running factor exceeds cur_alpha -- against a prefix of sel[], which is
    //     append-only, so it is the prefix the sequential visit would have walked;
    //   * a candidate that has seen all of sel[] is SELECTED only when it is the oldest one in flight: every earlier
    //     candidate is resolved by then, so sel[] is what the sequential visit would have found, and later candidates
    //     in flight meet the new entry at its place in the order (they are at or before the old end of sel[]).
    // Same factors (each group applies update_occlude in sel[] order), same last_checked, same sel[]; no distance is
    // evaluated speculatively, and the per-candidate scalar control flow of the one-at-a-time form (45 k scalar
    // instructions per prune, one per CU-cycle: profiles/r05_prune_counters.txt) is paid once per GROUPS candidates.
    uint16_t* work = reinterpret_cast<uint16_t*>(smem + L.keys_off);  // the sort keys are dead by now
    const uint32_t gbit = (uint32_t)(g * G);
    if (N > 0) {
        while (found < degree) {
            uint32_t M = 0;
            for (uint32_t base = 0; base < N; base += kWave) {
                const uint32_t i = base + lane;
                const bool act = i < N && !(occ[i] > cur_alpha);
                const uint64_t m = ballot64(act);
                if (act) work[M + mbcnt(m)] = (uint16_t)i;
                M += (uint32_t)__builtin_popcountll(m);
            }
            __syncthreads();
            uint32_t next = 0;
            bool busy = false;
            uint32_t c = 0, w = 0, l = 0;
            float o = 0.0f, di = 0.0f;
            const uint8_t* xi = ix.rows;
            for (;;) {
                // idle groups take the next candidates of the worklist, in group order
                const uint64_t im = ballot64(!busy && v == 0);
                if (im != 0 && next < M) {
                    const uint32_t wi = next + (uint32_t)__builtin_popcountll(im & ((1ull << gbit) - 1ull));
                    if (!busy && wi < M) {
                        w = wi;
                        c = work[wi];
                        l = last[c];
                        o = occ[c];
                        di = sd[c];
                        xi = ix.rows + (uint64_t)sid[c] * ix.row_stride;
                        busy = true;
                    }
                    const uint32_t nidle = (uint32_t)__builtin_popcountll(im);
                    next = next + nidle < M ? next + nidle : M;
                }
                if (ballot64(busy) == 0) break;  // worklist done, nothing in flight
                uint32_t wmin = busy ? w : 0xFFFFFFFFu;  // the oldest candidate in flight
#pragma unroll
                for (int off = 32; off >= G; off >>= 1) {
                    const uint32_t t = (uint32_t)__shfl_xor((int)wmin, off);
                    wmin = t < wmin ? t : wmin;
                }
                bool rej = false, evaluated = false;
                if (busy && l < found) {
                    const uint32_t rp = sel[l];
                    ++l;
                    if (rp < c) {
                        const uint8_t* y = ix.rows + (uint64_t)sid[rp] * ix.row_stride;
                        const float d = finish_distance<DT, OP, NORM>(group_distance_rows<DT, OP>(xi, y, (int)ix.dim, v), xi, y,
                                                                      ix.dim, SqParams{ix.sq_k, ix.sq_shift_norm_sq});
                        o = update_occlude<OP>(di, d, o, cur_alpha, occluding);  // (meaningful in the group's lane 0)
                        rej = o > cur_alpha;
                        evaluated = v == 0;
                    }
                }
                npairs += (uint32_t)__builtin_popcountll(ballot64(evaluated));
                const bool grej = (ballot64(rej && v == 0) >> gbit) & 1ull;
                const bool ready = busy && !grej && l == found && w == wmin;  // at most one group
                const bool commit = ballot64(ready) != 0;
                if (grej || ready) {
                    if (v == 0) {
                        last[c] = (uint16_t)l;
                        occ[c] = grej ? o : 3.402823466e+38f;
                        if (ready) sel[found] = c;
                    }
                    busy = false;
                }
                if (commit) ++found;
                __syncthreads();
                if (found >= degree) break;
            }
            if (found >= degree) break;
            if (cur_alpha == alpha) break;
            const float next_alpha = cur_alpha * inc;
            cur_alpha = next_alpha < alpha ? next_alpha : alpha;
        }
    }
    // ---- neighbours + optional saturation (index.rs:2626-2649) ---------------------------
    __syncthreads();
    uint32_t nout = found;
    if (force_saturate || (cfg.saturate_after_prune && alpha > 1.0f)) {
        // sequential in pool order; AdjacencyList::push filters duplicates
        for (uint32_t i = 0; i < N && nout < degree; ++i) {
            const uint32_t id = sid[i];
            if (id == location) continue;
            bool dup = false;
            for (uint32_t n = lane; n < nout; n += kWave) dup |= (sid[sel[n]] == id);
            if (ballot64(dup)) continue;
            if (lane == 0) sel[nout] = i;
            ++nout;
            __syncthreads();
        }
    }
    __syncthreads();
    for (uint32_t n = lane; n < nout; n += kWave) out[1 + n] = sid[sel[n]];
    if (lane == 0) {
        out[0] = nout;
        if (cfg.counters) atomicAdd(&stat_stripe(cfg.counters)[0], (unsigned long long)npairs);
    }
}

// ---- kernel A: prune caller-provided pools (phase 2 of multi_insert, dann_prune_batch) -----
template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void pool_prune_kernel(PoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using S = Scheme<DT, OP, true>;
    using RT = typename RowType<DT>::type;
    constexpr int G = S::G, GROUPS = kWave / G;
    const uint32_t lane = threadIdx.x, wi = blockIdx.x, item = a.pos0 + blockIdx.x;
    const PoolLds L = pool_lds_layout(a.pcap, a.cfg.pruned_degree);
    uint32_t* pid = reinterpret_cast<uint32_t*>(smem + L.pid_off);
    float* pd = reinterpret_cast<float*>(smem + L.pd_off);
    const uint32_t loc = a.locs[item];
    uint64_t lo;
    uint32_t cnt;
    if (a.offsets) {
        lo = a.offsets[wi];
        cnt = (uint32_t)(a.offsets[wi + 1] - lo);
    } else {
        lo = (uint64_t)wi * a.stride;
        cnt = a.counts[wi];
    }
    // extras = around(ids, position, cand) (utils/async_tools.rs:51-131)
    uint32_t nex = 0;
    if (a.cand != 0 && a.n > 1) nex = a.cand < a.n - 1 ? a.cand : a.n - 1;
    if (a.into_rows && cnt + nex == 0) return;
    uint32_t* out = a.into_rows ? a.ix.adj + (uint64_t)loc * a.ix.adj_stride : a.out + (uint64_t)wi * a.out_stride;
    if (cnt + nex > a.pcap) {
        if (lane == 0) {
            *a.err = 1;
            out[0] = 0;
        }
        return;
    }
    for (uint32_t i = lane; i < cnt; i += kWave) {
        pid[i] = a.pool_ids[lo + i];
        pd[i] = a.pool_d[lo + i];
    }
    if (nex) {
        const uint32_t half = (nex + 1) / 2;
        const uint32_t start = item >= half ? item - half : a.n - (half - item);
        const RT* x = reinterpret_cast<const RT*>(a.ix.rows + (uint64_t)loc * a.ix.row_stride);
        const int g = lane / G, v = lane % G;
        for (uint32_t r0 = 0; r0 < nex; r0 += GROUPS) {
            const uint32_t r = r0 + g;
            if (r < nex) {
                // r-th yielded position: walk from `start`, skipping `item`
                uint32_t p = start + r;
                // positions wrap; the skipped element shifts everything after it by one
                const uint32_t dist_to_item = item >= start ? item - start : item + a.n - start;
                if (r >= dist_to_item) p += 1;
                p %= a.n;
                const uint32_t id = a.locs[p];
                const uint8_t* y = a.ix.rows + (uint64_t)id * a.ix.row_stride;
                float d = finish_distance<DT, OP, NORM>(group_distance_rows<DT, OP>(reinterpret_cast<const uint8_t*>(x), y, (int)a.ix.dim, v),
                                                        reinterpret_cast<const uint8_t*>(x), y, a.ix.dim,
                                                        SqParams{a.ix.sq_k, a.ix.sq_shift_norm_sq});
                if (v == 0) {
                    pid[cnt + r] = id;
                    pd[cnt + r] = d;
                }
            }
        }
    }
    __syncthreads();
    prune_sorted_pool<DT, OP, NORM>(a.ix, a.cfg, loc, cnt + nex, a.pcap, smem, L, a.force_saturate != 0, out);
}

// ---- kernel B: robust_prune_list over explicit candidate lists ---------------------------
// (bootstrap: list = own edges ∪ other batch members; index.rs:597-645)
template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void bootstrap_kernel(ListArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x, item = blockIdx.x;
    const PoolLds L = pool_lds_layout(a.pcap, a.cfg.pruned_degree);
    uint32_t* pid = reinterpret_cast<uint32_t*>(smem + L.pid_off);
    float* pd = reinterpret_cast<float*>(smem + L.pd_off);
    const uint32_t loc = a.locs[item];
    const uint32_t* mine = a.pending + (uint64_t)item * a.pend_stride;
    const uint32_t ne = mine[0];
    uint32_t* out = a.out + (uint64_t)item * a.out_stride;
    if (ne + a.n > a.pcap) {
        if (lane == 0) {
            *a.err = 1;
            out[0] = 0;
        }
        return;
    }
    // AdjacencyList::from_iter_untrusted(edges ++ other sources): first occurrence wins.
    // Own edges are unique and never contain `loc`; a batch member already present in the
    // edges is skipped.
    for (uint32_t i = lane; i < ne; i += kWave) pid[i] = mine[1 + i];
    __syncthreads();
    uint32_t cnt = ne;
    for (uint32_t p0 = 0; p0 < a.n; p0 += kWave) {
        const uint32_t p = p0 + lane;
        uint32_t id = kEmpty;
        bool take = false;
        if (p < a.n && p != item) {
            id = a.locs[p];
            take = true;
            for (uint32_t e = 0; e < ne; ++e) take &= (pid[e] != id);
        }
        const uint64_t m = ballot64(take);
        if (take) pid[cnt + mbcnt(m)] = id;
        cnt += (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (a.cfg.tie_order != 0) {
        // from_iter_untrusted is sort_unstable + dedup (adjacencylist.rs:181-190): robust_prune_list walks the candidates
        // in ascending id order, and the reference's sort sees them arrive in that order.  The ids are distinct: an id's
        // rank is the number of smaller ones.
        uint32_t* tmp = reinterpret_cast<uint32_t*>(smem + L.keys_off);
        for (uint32_t i = lane; i < cnt; i += kWave) {
            const uint32_t id = pid[i];
            uint32_t r = 0;
            for (uint32_t j = 0; j < cnt; ++j) r += pid[j] < id ? 1u : 0u;
            tmp[r] = id;
        }
        __syncthreads();
        for (uint32_t i = lane; i < cnt; i += kWave) pid[i] = tmp[i];
        __syncthreads();
    }
    fill_list_distances<DT, OP, NORM>(a.ix, loc, pid, pd, cnt);
    __syncthreads();
    prune_sorted_pool<DT, OP, NORM>(a.ix, a.cfg, loc, cnt, a.pcap, smem, L, true, out);
}

// Partitioned commit (multi-GPU build): lists that fit are appended by every replica (cheap, deterministic); a list
// that has to be pruned -- the expensive part -- is queued only on the rank that owns the target.  The owners export
// the resulting rows, the others apply them (dann_insert_batch_commit_part / dann_apply_neighbor_rows_device).
__global__ void export_rows_kernel(IndexView ix, const uint64_t* keys, const uint32_t* seg_start, const uint32_t* work_short,
                                   uint32_t nshort, const uint32_t* work_long, uint32_t nlong, uint32_t* out) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= nshort + nlong) return;
    const uint32_t seg = i < nshort ? work_short[i] : work_long[i - nshort];
    const uint32_t tgt = (uint32_t)(keys[seg_start[seg]] >> 32);
    const uint32_t* arow = ix.adj + (uint64_t)tgt * ix.adj_stride;
    uint32_t* o = out + (uint64_t)i * (ix.max_degree + 2u);
    if (lane == 0) o[0] = tgt;
    for (uint32_t e = lane; e < ix.max_degree + 1u; e += blockDim.x) o[1 + e] = arow[e];
}

__global__ void apply_rows_kernel(IndexView ix, const uint32_t* rows, uint32_t count) {
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= count) return;
    const uint32_t* r = rows + (uint64_t)i * (ix.max_degree + 2u);
    const uint32_t tgt = r[0];
    if (tgt >= ix.nslots) return;
    uint32_t* arow = ix.adj + (uint64_t)tgt * ix.adj_stride;
    for (uint32_t e = lane; e < ix.max_degree + 1u; e += blockDim.x) arow[e] = e == 0 ? (r[1] < ix.max_degree ? r[1] : ix.max_degree) : r[1 + e];
}

// Four targets per wavefront, 16 lanes each.  A target's scan is a chain of dependent loads (segment start -> first key /
// segment length -> adjacency row) and a few compares: one wavefront per target kept 8 192 resident waves waiting on
// that chain (190 ms of the 1 M x 768 build, 900 k targets per batch); four chains per wave run side by side.  What is
// written -- the appended ids in source order, the worklists' contents -- is what the one-target form wrote.
__global__ __launch_bounds__(kWave) void backedge_scan_kernel(ScanArgs a) {
    __shared__ uint32_t newid[4][64];
    const uint32_t lane = threadIdx.x, sub = lane >> 4, sl = lane & 15u;
    const uint32_t seg_raw = blockIdx.x * 4u + sub;
    const bool have = seg_raw < a.nseg;
    const uint32_t seg = have ? seg_raw : a.nseg - 1u;  // (an idle group repeats the last segment's loads, writes nothing)
    const uint32_t start = a.seg_start[seg];
    const uint32_t src = (uint32_t)(a.keys[start] >> 32);
    uint32_t* arow = a.ix.adj + (uint64_t)src * a.ix.adj_stride;
    uint32_t len = arow[0];
    len = len < a.ix.max_degree ? len : a.ix.max_degree;
    const uint32_t nsrc = a.seg_len[start];
    const bool owned = a.world <= 1u || src % a.world == a.rank;
    const bool hub = nsrc > (uint32_t)kWave;
    if (have && hub && sl == 0 && owned) {
        // a hub hit by many back-edges: no serial scan here, the prune kernels de-duplicate 64 sources at a time
        // (len + #sources bounds the list; they also handle the case that everything still fits)
        const uint32_t bound = len + nsrc;
        if (bound <= a.short_cap) {
            a.work_short[atomicAdd(&a.counts[0], 1u)] = seg;
        } else {
            a.work_long[atomicAdd(&a.counts[1], 1u)] = seg;
            atomicMax(&a.counts[2], bound);
        }
    }
    const bool scan = have && !hub;
    // the first 64 list entries and the (at most 64) sources of the group's target: four per lane
    uint32_t mine[4], srcs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t e = sl + 16u * (uint32_t)j;
        mine[j] = (scan && e < len) ? arow[1 + e] : kEmpty;
        srcs[j] = (scan && e < nsrc) ? (uint32_t)a.keys[start + e] : kEmpty;
    }
    // AdjacencyList::extend_from_slice: a source already in the list is skipped (sources of one target are distinct)
    uint32_t kmax = 0;
    {
        uint32_t v = scan ? nsrc : 0u;  // the longest scan among the four groups
        v = max(v, (uint32_t)__shfl_xor((int)v, 16));
        v = max(v, (uint32_t)__shfl_xor((int)v, 32));
        kmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    }
    uint32_t nnew = 0;
    for (uint32_t k = 0; k < kmax; ++k) {
        const uint32_t from = (lane & 48u) | (k & 15u);
        uint32_t id = kEmpty;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((k >> 4) == (uint32_t)j) id = (uint32_t)__shfl((int)srcs[j], (int)from);
        const bool on = scan && k < nsrc;
        bool dup = (mine[0] == id) | (mine[1] == id) | (mine[2] == id) | (mine[3] == id);
        for (uint32_t e = kWave + sl; e < len; e += 16u) dup |= (arow[1 + e] == id);  // (degrees beyond 64)
        const uint32_t dm = (uint32_t)(ballot64(dup) >> (16u * sub)) & 0xFFFFu;
        if (on && dm == 0u) {
            if (sl == 0) newid[sub][nnew] = id;
            ++nnew;
        }
    }
    __syncthreads();
    if (!scan || nnew == 0) return;
    const uint32_t cnt = len + nnew;
    if (cnt <= a.cfg_max_degree) {
        const uint32_t slack = a.ix.max_degree - len;
        const uint32_t take = nnew < slack ? nnew : slack;
        for (uint32_t i = sl; i < take; i += 16u) arow[1 + len + i] = newid[sub][i];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (sl == 0) {
            arow[0] = len + take;
        }
        return;
    }
    if (sl == 0 && owned) {
        if (cnt <= a.short_cap && cnt > a.cfg_max_degree) {
            a.work_short[atomicAdd(&a.counts[0], 1u)] = seg;
        } else {
            a.work_long[atomicAdd(&a.counts[1], 1u)] = seg;
            atomicMax(&a.counts[2], cnt);
        }
    }
}

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void backedge_kernel(BackArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t lane = threadIdx.x, seg = a.work ? a.work[blockIdx.x] : blockIdx.x;
    const PoolLds L = pool_lds_layout(a.pcap, a.cfg.pruned_degree);
    uint32_t* pid = reinterpret_cast<uint32_t*>(smem + L.pid_off);
    float* pd = reinterpret_cast<float*>(smem + L.pd_off);
    const uint32_t start = a.seg_start[seg];
    const uint32_t src = (uint32_t)(a.keys[start] >> 32);
    // adjacency of `src` (Neighbors::get)
    uint32_t* arow = a.ix.adj + (uint64_t)src * a.ix.adj_stride;
    uint32_t len = arow[0];
    len = len < a.ix.max_degree ? len : a.ix.max_degree;
    for (uint32_t i = lane; i < len; i += kWave) pid[i] = arow[1 + i];
    __syncthreads();
    // extend_from_slice(sorted targets): unique append
    uint32_t cnt = len;
    bool overflow = false;
    const uint32_t end = start + a.seg_len[start];
    for (uint32_t k0 = start; k0 < end; k0 += kWave) {
        const uint32_t k = k0 + lane;
        const bool mine = k < end;
        const uint32_t id = mine ? (uint32_t)a.keys[k] : kEmpty;
        bool take = mine;
        if (mine)
            for (uint32_t e = 0; e < len; ++e) take &= (pid[e] != id);
        const uint64_t tm = ballot64(take);
        const uint32_t ntake = (uint32_t)__popcll(tm);
        if (cnt + ntake > a.pcap) {
            overflow = true;
            break;
        }
        if (take) pid[cnt + mbcnt(tm)] = id;
        cnt += ntake;
    }
    if (overflow) {
        if (lane == 0) *a.err = 1;
        return;
    }
    const uint32_t added = cnt - len;
    if (added == 0) return;
    __syncthreads();
    if (cnt <= a.cfg.max_degree) {
        // append_vector with the provider-capacity clamp (provider.rs:795-822)
        const uint32_t slack = a.ix.max_degree - len;
        const uint32_t take = added < slack ? added : slack;
        for (uint32_t i = lane; i < take; i += kWave) arow[1 + len + i] = pid[len + i];
        __syncthreads();
        if (lane == 0) {
            arow[0] = len + take;
        }
        return;
    }
    fill_list_distances<DT, OP, NORM>(a.ix, src, pid, pd, cnt);
    if (lane == 0 && a.cfg.counters) atomicAdd(&stat_stripe(a.cfg.counters)[1], (unsigned long long)cnt);
    __syncthreads();
    // the list lives in LDS, so the result can go straight into the adjacency row (nobody
    // else reads this row during the back-edge phase)
    prune_sorted_pool<DT, OP, NORM>(a.ix, a.cfg, src, cnt, a.pcap, smem, L, false, arow);
    if (lane == 0 && a.count_long && a.cfg.counters) atomicAdd(&stat_stripe(a.cfg.counters)[7], 1ull);
}

// ---- small utility kernels -------------------------------------------------------------------
// `limit`: back-edges go to the first `limit` neighbours of a new point only (DiskANNIndex::insert takes
// max_backedges of them, index.rs:324-327; multi_insert all, index.rs:123-143)
__global__ void make_keys_kernel(const uint32_t* locs, const uint32_t* pending, uint32_t pend_stride, uint32_t n,
                                 uint32_t degree, uint64_t* keys, uint32_t limit) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * degree) return;
    const uint32_t item = t / degree, e = t % degree;
    const uint32_t* row = pending + (uint64_t)item * pend_stride;
    keys[t] = (e < row[0] && e < limit) ? (((uint64_t)row[1 + e] << 32) | locs[item]) : ~0ull;
}

__global__ void segment_kernel(const uint64_t* keys, uint32_t total, uint32_t* seg_start, uint32_t* meta) {
    // meta[0] = #segments, meta[1] = #valid keys (invalid keys sort to the end)
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t k = keys[t];
    if (k == ~0ull) return;
    if (t + 1 == total || keys[t + 1] == ~0ull) meta[1] = t + 1;
    if (t == 0 || (uint32_t)(keys[t - 1] >> 32) != (uint32_t)(k >> 32)) seg_start[atomicAdd(&meta[0], 1u)] = t;
}

__global__ void seglen_kernel(const uint64_t* keys, const uint32_t* seg_start, uint32_t* seg_len, uint32_t* meta) {
    // meta[2] = max segment length
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= meta[0]) return;
    const uint32_t st = seg_start[s];
    const uint32_t tgt = (uint32_t)(keys[st] >> 32);
    uint32_t e = st + 1;
    while (e < meta[1] && (uint32_t)(keys[e] >> 32) == tgt) ++e;
    seg_len[st] = e - st;
    // (a maximum only grows: skip the atomic when a plain read already shows it -- one address, a million segments)
    if (e - st > __hip_atomic_load(&meta[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&meta[2], e - st);
}

__global__ void set_bulk_kernel(IndexView ix, const uint32_t* locs, const uint32_t* pending, uint32_t pend_stride,
                                uint32_t n) {
    const uint32_t item = blockIdx.x;
    if (item >= n) return;
    const uint32_t* row = pending + (uint64_t)item * pend_stride;
    uint32_t* arow = ix.adj + (uint64_t)locs[item] * ix.adj_stride;
    const uint32_t len = row[0];
    for (uint32_t i = threadIdx.x; i < len; i += blockDim.x) arow[1 + i] = row[1 + i];
    if (threadIdx.x == 0) arow[0] = len;
}

constexpr auto kPoolPrune = [](auto r) { using R = decltype(r); return KernelOf<pool_prune_kernel<R::dt, R::op, R::norm>>{}; };
constexpr auto kBootstrap = [](auto r) { using R = decltype(r); return KernelOf<bootstrap_kernel<R::dt, R::op, R::norm>>{}; };
constexpr auto kBackedge = [](auto r) { using R = decltype(r); return KernelOf<backedge_kernel<R::dt, R::op, R::norm>>{}; };

}  // namespace

int32_t launch_pool_prune(const PoolArgs& a, uint32_t items, hipStream_t st) {
    return launch_rows(a.ix, kPoolPrune, "pool_prune_kernel launch", a, items, pool_lds_layout(a.pcap, a.cfg.pruned_degree).total, st);
}
int32_t launch_bootstrap(const ListArgs& a, hipStream_t st) {
    return launch_rows(a.ix, kBootstrap, "bootstrap_kernel launch", a, a.n, pool_lds_layout(a.pcap, a.cfg.pruned_degree).total, st);
}
int32_t launch_backedge(const BackArgs& a, hipStream_t st) {
    return launch_rows(a.ix, kBackedge, "backedge_kernel launch", a, a.nseg, pool_lds_layout(a.pcap, a.cfg.pruned_degree).total, st);
}
void launch_backedge_scan(const ScanArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(backedge_scan_kernel, dim3((a.nseg + 3u) / 4u), dim3(kWave), 0, st, a);
}
void launch_export_rows(const IndexView& ix, const uint64_t* keys, const uint32_t* seg_start, const uint32_t* work_short,
                        uint32_t nshort, const uint32_t* work_long, uint32_t nlong, uint32_t* out, hipStream_t st) {
    hipLaunchKernelGGL(export_rows_kernel, dim3(nshort + nlong), dim3(kWave), 0, st, ix, keys, seg_start, work_short, nshort,
                       work_long, nlong, out);
}
void launch_apply_rows(const IndexView& ix, const uint32_t* rows, uint32_t count, hipStream_t st) {
    hipLaunchKernelGGL(apply_rows_kernel, dim3(count), dim3(kWave), 0, st, ix, rows, count);
}
void launch_make_keys(const uint32_t* locs, const uint32_t* pending, uint32_t pend_stride, uint32_t n, uint32_t degree,
                      uint64_t* keys, uint32_t limit, hipStream_t st) {
    hipLaunchKernelGGL(make_keys_kernel, dim3((n * degree + 255) / 256), dim3(256), 0, st, locs, pending, pend_stride, n, degree,
                       keys, limit);
}
void launch_segments(const uint64_t* keys, uint32_t total, uint32_t* seg_start, uint32_t* seg_len, uint32_t* meta, hipStream_t st) {
    hipLaunchKernelGGL(segment_kernel, dim3((total + 255) / 256), dim3(256), 0, st, keys, total, seg_start, meta);
    hipLaunchKernelGGL(seglen_kernel, dim3((total + 255) / 256), dim3(256), 0, st, keys, seg_start, seg_len, meta);
}
void launch_set_bulk(const IndexView& ix, const uint32_t* locs, const uint32_t* pending, uint32_t pend_stride, uint32_t n,
                     hipStream_t st) {
    hipLaunchKernelGGL(set_bulk_kernel, dim3(n), dim3(64), 0, st, ix, locs, pending, pend_stride, n);
}

}  // namespace dann
