// build_common.h -- what the translation units of the build path share (prune_rows.hip: the row-kernel prunes;
// prune_gram.hip: the matrix-core prune; gram_tiles.hip: its Gram tile kernel; build_batch.hip: the batch driver and the C
// entry points): the prune configuration and its counters, the LDS layout of a candidate pool, the pieces of
// RobustPrune both prunes restate, the argument blocks that cross a unit boundary and the Gram error interval.
#pragma once

#include "prune_common.h"
#include "rust_order.h"

namespace dann {

struct PruneCfg {
    uint32_t pruned_degree, max_degree, max_occlusion;
    float alpha;
    uint32_t saturate_after_prune;
    uint32_t tie_order;  // dann_set_prune_tie_order: DANN_TIE_POSITION (bitonic sort on (distance, pool position)) or
                         // DANN_TIE_RUST (rust_order.h, one lane; the bootstrap's candidates in ascending id order)
    // optional device counters (u64): [0] pair distances of the sweeps (row kernel), [1] list / extra distances
    // d(location, c), [2] rows that went through an MFMA Gram, [3] Gram entries computed (x dim x 2 = MFMA flop),
    // [4] pair distances the lazy scans of the Gram sweeps asked for, [5] those answered by an exact re-evaluation,
    // [6] back-edge prunes through the MFMA path, [7] back-edge prunes of lists too long for it.
    // kStatStripes copies of the eight, one 64-byte line each, a workgroup adds to the copy of its index (stat_stripe):
    // every workgroup of a prune launch ends with a few of these adds, and atomics on ONE address are served one after
    // another -- 354 k of them per launch were 3 ms of backedge_scan_kernel's 4.4 ms at 10 M points
    // (profiles/r05_scan_atomics.txt).  dann_build_counters sums the copies.  One more word behind the stripes
    // (counters[kStatStripes * 8]): tied pools whose DANN_TIE_RUST walk reached the selection's fallback (rust_order.h).
    unsigned long long* counters;
};
constexpr uint32_t kStatStripes = 256;

struct PoolLds {
    uint32_t keys_off, pid_off, pd_off, sid_off, sd_off, occ_off, last_off, sel_off, total;
};

// prune caller-provided pools (phase 2 of multi_insert, dann_prune_batch): pool_prune_kernel, pool_sort_kernel and
// (the fields the sweep reads) pool_sweep_kernel
struct PoolArgs {
    IndexView ix;
    PruneCfg cfg;
    const uint32_t* locs;      // n locations
    const uint32_t* pool_ids;  // pools
    const float* pool_d;
    const uint64_t* offsets;   // n+1 (ragged) or null
    uint32_t stride;           // when offsets == null: pool i at i*stride, count counts[i]
    const uint32_t* counts;
    uint32_t cand;             // intra-batch candidates per item (0 = none); batch = locs[0..n)
    uint32_t n;
    uint32_t pos0;             // batch position of work item 0 (a rank may own a slice of the batch)
    uint32_t pcap;
    int32_t force_saturate;
    uint32_t* out;             // n x out_stride
    uint32_t out_stride;
    uint32_t* err;             // set to 1 on pool overflow
    uint32_t into_rows = 0;    // 1: the result goes straight into locs[item]'s adjacency row (out unused), and an empty
                               // pool leaves the row alone (graph consolidation: prune_pools_into_rows)
};

// back-edges, one wave per distinct target (add_edge_and_prune): backedge_kernel, backedge_list_kernel
struct BackArgs {
    IndexView ix;
    PruneCfg cfg;
    const uint64_t* keys;      // sorted (target << 32 | source), `nkeys` valid entries first
    const uint32_t* seg_start; // nseg segment start indices (arbitrary order)
    const uint32_t* seg_len;   // length of the segment starting at index i (indexed by start)
    uint32_t nseg;
    uint32_t nkeys;
    uint32_t pcap;
    uint32_t* err;
    uint32_t count_long = 0;   // this launch prunes the lists too long for the MFMA path: counted in counters[7]
    const uint32_t* work;      // optional: segment indices to process (targets whose list needs a prune)
};

namespace {

__device__ __forceinline__ unsigned long long* stat_stripe(unsigned long long* counters) {
    return counters + (size_t)(blockIdx.x & (kStatStripes - 1u)) * 8u;
}

__host__ __device__ inline PoolLds pool_lds_layout(uint32_t pcap, uint32_t degree) {
    PoolLds l;
    uint32_t off = 0;
    l.keys_off = off;
    off += pcap * 8u;
    l.pid_off = off;
    off += pcap * 4u;
    l.pd_off = off;
    off += pcap * 4u;
    l.sid_off = off;
    off += pcap * 4u;
    l.sd_off = off;
    off += pcap * 4u;
    l.occ_off = off;
    off += pcap * 4u;
    l.last_off = off;
    off += ((pcap * 2u) + 15u) & ~15u;
    l.sel_off = off;
    off += ((degree + 1u) * 4u + 15u) & ~15u;
    l.total = off;
    return l;
}

// What pool_sweep_kernel's batched sweep keeps in LDS: the sorted list (ids, distances), its sweep state and the norms of the
// Gram rows -- not the unsorted pool and the sort keys of the kernels that build the list (3 KB of 7.9 KB at 256 slots: with
// them the sweep ran 12 lists per CU, without them 16).  Same field names, so sweep_gram_batched reads either layout.
__host__ __device__ inline PoolLds sweep_lds_layout(uint32_t pcap, uint32_t degree) {
    PoolLds l;
    uint32_t off = 0;
    l.keys_off = off;  // the norms of the Gram rows (at most 256 rows)
    off += (pcap < 256u ? pcap : 256u) * 4u;
    l.pid_off = l.pd_off = 0;  // (not part of this layout)
    l.sid_off = off;
    off += pcap * 4u;
    l.sd_off = off;
    off += pcap * 4u;
    l.occ_off = off;
    off += pcap * 4u;
    l.last_off = off;
    off += ((pcap * 2u) + 15u) & ~15u;
    l.sel_off = off;
    off += ((degree + 1u) * 4u + 15u) & ~15u;
    l.total = off;
    return l;
}

// PruneKind::update_occlude_factor (config/mod.rs:80-103)
template <int OP>
__device__ __forceinline__ float update_occlude(float d_ik, float d_jk, float cur, float alpha, bool occluding) {
    if (!occluding) {
        if (d_jk == 0.0f) return 3.402823466e+38f;
        float r = d_ik / d_jk;
        if (r != r) return cur;  // f32::max ignores NaN
        if (cur != cur) return r;
        return cur > r ? cur : r;
    }
    if (d_jk < alpha * d_ik) return alpha + 0.01f;
    return cur;
}

// DANN_TIE_RUST: the pool order of SortedNeighbors::new as the reference's own sort leaves it (rust_order.h).  Lane 0 walks
// the algorithm over the pool positions, kept in the `last` array (16 bits per slot, zeroed by the caller's final loop
// after it has read them); stacks and merge buffer in the region of the sort keys, whose contents (the network's output)
// are dead once the walk is decided.  Pools of fewer than 64 slots have less than kWorkBytes there -- and need none of it
// beyond the 64-byte merge buffer (quicksort starts at 33 entries).  The caller synchronises the wave afterwards.
//
// The walk is only needed where it can matter: a pool whose distances are all distinct (and ordered: no NaN) has one
// sorted order, and select_nth_unstable_by + sort_unstable_by + truncate leave exactly its head -- what the sorting
// network has already produced.  pool_has_ties looks at neighbouring keys of the network's output (wave-uniform result);
// on continuous data nearly every pool takes the network alone, on byte data and lattices the tied pools are walked.
__device__ __forceinline__ bool pool_has_ties(const uint64_t* keys, uint32_t P, bool lane_saw_nan) {
    const uint32_t lane = threadIdx.x & 63u;
    bool tie = lane_saw_nan;
    for (uint32_t i = lane; i + 1 < P; i += kWave) tie |= (uint32_t)(keys[i] >> 32) == (uint32_t)(keys[i + 1] >> 32);
    return ballot64(tie) != 0;
}
__device__ __forceinline__ void rust_order_by_lane0(const PruneCfg& cfg, uint32_t P, uint8_t* smem, const PoolLds& L) {
    uint16_t* ord = reinterpret_cast<uint16_t*>(smem + L.last_off);
    const float* pd = reinterpret_cast<const float*>(smem + L.pd_off);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t i = lane; i < P; i += kWave) ord[i] = (uint16_t)i;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // (the selection's median-of-medians fallback -- sixteen unlucky partitions in a row -- is restated as a sort of the
    // range, which may leave equal keys in another arrangement than core's: counted, so that builds and tests can assert
    // it never happened: dann_build_counters()[10])
    if (lane == 0 && rust_order::sorted_neighbors(ord, pd, P, cfg.max_occlusion, smem + L.keys_off) && cfg.counters)
        atomicAdd(cfg.counters + (size_t)kStatStripes * 8u, 1ull);
}

inline PruneCfg to_prune_cfg(const dann_index* idx, const dann_build_config& c) {
    PruneCfg p;
    p.tie_order = idx->prune_tie_order;
    p.pruned_degree = c.pruned_degree;
    p.max_degree = c.max_degree;
    p.max_occlusion = c.max_occlusion_size ? c.max_occlusion_size : 750;
    p.alpha = c.alpha;
    p.saturate_after_prune = c.saturate_after_prune;
    p.counters = nullptr;
    return p;
}

// The error interval of a pair distance derived from a Gram entry (prune_gram.hip states the derivation): one f32 FMA chain
// over the whole row per entry, K = dim rounded up to 32 terms:
//       |G_ij - <x,y>| <= gamma_K sum|x_e y_e| <= K u (|x|^2 + |y|^2) / 2, u = 2^-24;  d' = (|x|^2 + |y|^2) - 2 G_ij
//       with the norms accumulated in f64 -> c1 = (K + 4) u (+ 5 % slack) covers G, the norms' rounding and the two f32
//       operations on terms of that size.
// c2 (relative to |d'|) covers the final subtraction and the reference's own f32 rounding, which grows with the row
// length: its L2 / IP kernels run dim / (8 NACC) terms per chain plus the combine and sum_tree adds and round x - y
// before squaring -> (dim / 8 + 16) u bounds every row type and strategy (never below the 3e-6 of the 128-d analysis).
// tests/test_gram_interval.py evaluates both sides on the CPU (pairs built to cancel) and checks the bound.
constexpr float kGramC2 = 3.0e-6f;
constexpr float kUnitRoundoff = 5.9604645e-8f;  // 2^-24
inline float gram_c2_for_dim(uint32_t dim) {
    const float c = ((float)(dim / 8u) + 16.0f) * kUnitRoundoff;
    return c > kGramC2 ? c : kGramC2;
}
inline float gram_c1_chained(uint32_t dim) { return 1.05f * ((float)((dim + 31u) & ~31u) + 4.0f) * kUnitRoundoff; }

}  // namespace
}  // namespace dann
