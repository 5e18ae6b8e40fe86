// prune_gram.hip -- RobustPrune with the pair distances of a candidate list taken from its Gram matrix on the matrix
// cores: the sort kernels that leave a sorted list in global memory, the sweeps that read the Gram (gram_tiles.hip
// computes it), and the host function that runs tiles + sweep for the three callers in build_batch.hip.
#include "prune_gram.h"

namespace dann {
namespace {

// ======================================================================================================
// MFMA path (f32 / f16 rows): pair similarities of one candidate list as a Gram matrix on the matrix cores.
//
// prune::robust_prune asks for d(c_i, c_j) between a candidate and the candidates already selected
// (prune.rs:196-232, `compute_distance`) -- for a back-edge prune nearly every pair of the list, for the pool prune of
// an inserted point ~2 200 pairs among the first ~140 sorted candidates.  Instead of evaluating them one dependent row
// pair at a time, the lower triangle of the list's Gram matrix G = C C^T is computed with v_mfma_f32_32x32x2_f32
// (gram_tiles_kernel) and the sweep derives from it an *approximation* of every pair distance together with a rigorous
// bound of its deviation from the reference's own f32 value:
//     L2:  d' = |x|^2 + |y|^2 - 2<x,y>,   IP: d' = -<x,y>,   CosineNormalized: d' = 1 - <x,y>
//     |d' - d_ref| <= E = c1 * (|x|^2 + |y|^2) + c2 * |d'|
// Every decision of the sweep is a comparison of d_ref with a threshold; where the interval [d' - E, d' + E]
// does not decide it, the pair is re-evaluated with the bit-exact row kernel.  The adjacency lists are therefore
// identical to the lazy path's (and the oracle's) by construction; tests/test_gpu_build.py checks it.
// ======================================================================================================

struct GramCtx {
    const float* g;      // LDS or global: g[p * ld + q] = <row p, row q>, p < nrows, q < ncols
    const float* nrm;    // |row p|^2, p < nrows
    uint32_t ld, nrows, ncols;
    bool by_sorted;      // rows are indexed by sorted pool order (pool prune) or by pool position (back-edge lists)
    float escale;        // 1.0; tests widen the error interval (DANN_DBG_GRAM_ESCALE) to drive every decision through the exact path
    float c1, c2;        // error interval E = c1 (|x|^2 + |y|^2) + c2 |d'| of this Gram's arithmetic
    bool count_rows;     // add this list to the Gram row / flop counters (the tiles kernel counts its own)
    bool prefetch;       // g lives in global memory: touch the next candidates' rows ahead of their look-ups
};

// prune_sorted_pool with the pair distances taken from the Gram matrix (exact re-check where the error interval
// does not decide).  Single wave (lanes 0..63 of the workgroup); the other waves have exited.
// one wave: LDS accesses of a single wave retire in program order; this is the compiler + counter fence between them
__device__ __forceinline__ void wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// SortedNeighbors::new for one wave (the other waves of the workgroup may be waiting at a barrier): pid/pd[0..P) ->
// sid/sd/occ/last[0..N), keys[i] keeps the pool position of sorted entry i.  Returns N.
__device__ uint32_t sort_pool_wave(const PruneCfg& cfg, uint32_t P, uint32_t pcap, uint8_t* smem, const PoolLds& L) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem + L.keys_off);
    const uint32_t* pid = reinterpret_cast<const uint32_t*>(smem + L.pid_off);
    const float* pd = reinterpret_cast<const float*>(smem + L.pd_off);
    uint32_t* sid = reinterpret_cast<uint32_t*>(smem + L.sid_off);
    float* sd = reinterpret_cast<float*>(smem + L.sd_off);
    float* occ = reinterpret_cast<float*>(smem + L.occ_off);
    uint16_t* last = reinterpret_cast<uint16_t*>(smem + L.last_off);
    bool saw_nan = false;
    for (uint32_t i = lane; i < pcap; i += kWave) {
        const float d = i < P ? pd[i] : 0.0f;
        saw_nan |= d != d;
        keys[i] = i < P ? dist_key(d, i) : ~0ull;
    }
    wave_sync();
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
            wave_sync();
        }
    }
    const uint32_t N = P < cfg.max_occlusion ? P : cfg.max_occlusion;
    if (cfg.tie_order != 0 && pool_has_ties(keys, P, saw_nan)) {  // (see prune_sorted_pool)
        wave_sync();
        rust_order_by_lane0(cfg, P, smem, L);
        wave_sync();  // the work area of the walk is dead: keys[i] = pool position of sorted entry i, as the sort leaves it
        for (uint32_t i = lane; i < N; i += kWave) keys[i] = last[i];
    }
    for (uint32_t i = lane; i < N; i += kWave) {
        const uint32_t pos = (uint32_t)keys[i];
        sid[i] = pid[pos];
        sd[i] = pd[pos];
        occ[i] = 0.0f;
        last[i] = 0;
    }
    wave_sync();
    return N;
}

// The sweep of prune::robust_prune over a pool already sorted by sort_pool_wave, pair distances from the Gram matrix
// where it covers the pair (exact re-check where the error interval does not decide, exact evaluation where it
// does not cover it).  One wave (lanes 0..63 of the workgroup).
template <int DT, int OP, bool NORM>
__device__ void sweep_sorted_pool_gram(const IndexView& ix, const PruneCfg& cfg, uint32_t location, uint32_t N,
                                       uint8_t* smem, const PoolLds& L, bool force_saturate, uint32_t* out,
                                       const GramCtx gc) {
    using S = Scheme<DT, OP, true>;
    constexpr int G = S::G;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(smem + L.keys_off);
    const uint32_t* sid = reinterpret_cast<const uint32_t*>(smem + L.sid_off);
    const float* sd = reinterpret_cast<const float*>(smem + L.sd_off);
    float* occ = reinterpret_cast<float*>(smem + L.occ_off);
    uint16_t* last = reinterpret_cast<uint16_t*>(smem + L.last_off);
    uint32_t* sel = reinterpret_cast<uint32_t*>(smem + L.sel_off);
    const uint32_t P = N;
    const uint32_t degree = cfg.pruned_degree;
    const bool occluding = (ix.metric == M_IP);
    const float alpha = cfg.alpha;
    const float inc = alpha < 1.2f ? alpha : 1.2f;
    const float kMax = 3.402823466e+38f;
    float cur_alpha = 1.0f;
    uint32_t found = 0, nexact = 0, nasked = 0;  // nasked: pair distances the reference's lazy scan asks for
    const int v = lane % G;
    const SqParams sqp{ix.sq_k, ix.sq_shift_norm_sq};
    // first selected entry in sel[a..b) (pool order filter rp < i) whose pair distance with candidate i makes
    // update_occlude exceed `at`; returns its index in sel, or b when there is none
    auto first_exceed = [&](uint32_t i, uint32_t a, uint32_t b, float at) -> uint32_t {
        const uint32_t pi = gc.by_sorted ? i : (uint32_t)keys[i];
        const bool irow = pi < gc.nrows;
        const float gii = irow ? gc.nrm[pi] : 0.0f;
        const float di = sd[i];
        const uint8_t* xi = ix.rows + (uint64_t)sid[i] * ix.row_stride;
        const float thr = at * di;  // occluding rule: d_jk < alpha * d_ik (config/mod.rs:98)
        for (uint32_t c0 = a; c0 < b; c0 += kWave) {
            const uint32_t c = c0 + lane;
            int cls = 0;  // 0: certainly not, 1: certainly exceeds, 2: the error interval does not decide
            uint32_t rp = 0;
            if (c < b) {
                rp = sel[c];
                if (rp < i) {
                    const uint32_t pj = gc.by_sorted ? rp : (uint32_t)keys[rp];
                    cls = 2;  // pairs the Gram does not cover are evaluated exactly
                    if (irow && pj < gc.ncols) {
                    const float gij = gc.g[pi * gc.ld + pj], gjj = gc.nrm[pj];
                    const float nsum = gii + gjj;
                    float dp;
                    if (OP == OP_L2) dp = nsum - 2.0f * gij;
                    else dp = NORM ? 1.0f - gij : -gij;
                    const float e = gc.escale * (gc.c1 * nsum + gc.c2 * __builtin_fabsf(dp));
                    const float lo = dp - e, hi = dp + e;
                    if (occluding) {
                        if (hi < thr) cls = 1;
                        else if (lo >= thr) cls = 0;
                    } else if (lo > 0.0f && di >= 0.0f) {
                        const float rmin = di / hi, rmax = di / lo;
                        if (rmin > at * 1.000001f) cls = 1;
                        else if (rmax < at * 0.999999f) cls = 0;
                    }
                    }
                }
            }
            uint64_t tu = ballot64(cls != 0);
            const uint64_t valid = ballot64(c < b && rp < i);  // the pairs of this block the lazy scan would evaluate
            auto asked_upto = [&](int f) { nasked += (uint32_t)__popcll(valid & (f >= 63 ? ~0ull : ((2ull << f) - 1ull))); };
            if (!tu) asked_upto(63);
            while (tu) {
                const int f = __builtin_ctzll(tu);
                if (__builtin_amdgcn_readlane(cls, f) == 1) {
                    asked_upto(f);
                    return c0 + (uint32_t)f;
                }
                // bit-exact pair distance (every lane group evaluates the same pair)
                ++nexact;
                const uint32_t rpf = (uint32_t)__builtin_amdgcn_readlane((int)rp, f);
                const uint8_t* y = ix.rows + (uint64_t)sid[rpf] * ix.row_stride;
                const float d = finish_distance<DT, OP, NORM>(group_distance_rows<DT, OP>(xi, y, (int)ix.dim, v), xi, y,
                                                              ix.dim, sqp);
                const float dg = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d), 0));
                if (update_occlude<OP>(di, dg, 0.0f, at, occluding) > at) {
                    asked_upto(f);
                    return c0 + (uint32_t)f;
                }
                tu &= tu - 1;
                if (!tu) asked_upto(63);
            }
        }
        return b;
    };
    // Gram in global memory (three-kernel pool prune): every look-up of a candidate's row is a dependent round trip to
    // L2 / the Infinity Cache / HBM, and the sweep is a chain of them.  The rows of the next two candidates are touched
    // (one dword per 128-byte line of the row's <= 96 columns) while the current one is examined: pure prefetch into a
    // register nothing ever reads, never waited for (the loop's own loads drain the in-order queue behind it).
    uint32_t gpf = 0;
    auto touch_row = [&](uint32_t r) {
        if (!gc.prefetch || r >= gc.nrows) return;
        uint32_t col = lane < 3u ? lane * 32u : 0u;  // unconditional, clamped: no exec-mask block around the request
        col = col < gc.ncols ? col : 0u;
        const float* pr = gc.g + (size_t)r * gc.ld + col;
        asm volatile("global_load_dword %0, %1, off" : "=&v"(gpf) : "v"(pr));
    };
    if (N > 0) {
        while (found < degree) {
            touch_row(0);
            touch_row(1);
            for (uint32_t i = 0; i < N && found < degree; ++i) {
                asm volatile("" ::"v"(gpf));
                touch_row(i + 2);
                const float o = occ[i];
                uint32_t l = last[i];
                if (o == kMax) continue;                      // selected or excluded
                if (occluding && o > cur_alpha) continue;     // o is exact for the Occluding kind (alpha_then + 0.01)
                const uint32_t idi = sid[i];
                if (idi == location || idi >= ix.nslots) {
                    if (lane == 0) occ[i] = kMax;
                    continue;
                }
                // TriangleInequality kind: the stored maximum ratio is only ever compared with the current alpha;
                // it is re-derived from the entries already examined (sel[0..l))
                if (!occluding && l != 0 && first_exceed(i, 0, l, cur_alpha) != l) continue;
                bool rejected = false;
                if (l != found) {
                    const uint32_t at = first_exceed(i, l, found, cur_alpha);
                    if (at != found) {
                        l = at + 1;
                        rejected = true;
                    } else {
                        l = found;
                    }
                }
                wave_sync();
                if (lane == 0) {
                    last[i] = (uint16_t)l;
                    if (rejected) {
                        if (occluding) occ[i] = cur_alpha + 0.01f;
                    } else {
                        occ[i] = kMax;
                        sel[found] = i;
                    }
                }
                if (!rejected) ++found;
                wave_sync();
            }
            if (cur_alpha == alpha) break;
            const float next = cur_alpha * inc;
            cur_alpha = next < alpha ? next : alpha;
        }
    }
    if (gc.prefetch) {  // no prefetch load may still be in flight when its landing register is released
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" ::"v"(gpf));
    }
    wave_sync();
    uint32_t nout = found;
    if (force_saturate || (cfg.saturate_after_prune && alpha > 1.0f)) {
        for (uint32_t i = 0; i < N && nout < degree; ++i) {
            const uint32_t id = sid[i];
            if (id == location) continue;
            bool dup = false;
            for (uint32_t n = lane; n < nout; n += kWave) dup |= (sid[sel[n]] == id);
            if (ballot64(dup)) continue;
            if (lane == 0) sel[nout] = i;
            ++nout;
            wave_sync();
        }
    }
    wave_sync();
    for (uint32_t n = lane; n < nout; n += kWave) out[1 + n] = sid[sel[n]];
    if (lane == 0) {
        out[0] = nout;
        if (cfg.counters) {
            atomicAdd(&stat_stripe(cfg.counters)[0], (unsigned long long)nexact);
            if (gc.count_rows) {
                atomicAdd(&stat_stripe(cfg.counters)[2], (unsigned long long)P);
                atomicAdd(&stat_stripe(cfg.counters)[3], (unsigned long long)P * P);
            }
            atomicAdd(&stat_stripe(cfg.counters)[4], (unsigned long long)nasked);
            atomicAdd(&stat_stripe(cfg.counters)[5], (unsigned long long)nexact);
        }
    }
}

// The same sweep for lists whose Gram lives in global memory, eight candidates at a time.  In the form above every
// candidate costs a chain of dependent round trips (its queue state from LDS, then one Gram row from L2 / HBM, then the
// decision, then the state back to LDS): ~4 000 cycles each, 2.3 ms per pool prune of ~350 candidate visits.  Here a
// 64-candidate window of the sweep state is read once, the raw Gram rows of the next eight candidates that need a visit
// are requested together (two coalesced requests each: columns [0, 64) and [64, 128)), and the eight visits then run from
// registers: lane c stands for the c-th selected entry and picks G(i, sel_c) out of the row with one cross-lane read, so
// entries selected a moment ago need no new request.  The decisions, their order and the exact re-checks are those of
// sweep_sorted_pool_gram (same classes, same first-exceed rule); requires pruned_degree <= 64 (one lane per selected
// entry), a Gram indexed by sorted position and at most 128 Gram columns.
constexpr uint32_t kSweepRowsLds = 8u * 128u * 4u + 64u;  // LDS behind the pool layout: the raw Gram rows of one block of visits

template <int DT, int OP, bool NORM>
__device__ void sweep_gram_batched(const IndexView& ix, const PruneCfg& cfg, uint32_t location, uint32_t N,
                                   uint8_t* smem, const PoolLds& L, bool force_saturate, uint32_t* out, const GramCtx gc,
                                   float* rowsl) {
    constexpr int B = 8;
    using S = Scheme<DT, OP, true>;
    constexpr int G = S::G, GROUPS = kWave / G;
    const uint32_t lane = threadIdx.x & 63u;
    const int g = (int)(lane / G);
    const uint32_t* sid = reinterpret_cast<const uint32_t*>(smem + L.sid_off);
    const float* sd = reinterpret_cast<const float*>(smem + L.sd_off);
    float* occ = reinterpret_cast<float*>(smem + L.occ_off);
    uint16_t* last = reinterpret_cast<uint16_t*>(smem + L.last_off);
    uint32_t* sel = reinterpret_cast<uint32_t*>(smem + L.sel_off);
    float* nrml = reinterpret_cast<float*>(smem + L.keys_off);  // the sort keys are dead: the norms of the Gram rows
    for (uint32_t i = lane; i < gc.nrows; i += kWave) nrml[i] = gc.nrm[i];
    wave_sync();
    const uint32_t degree = cfg.pruned_degree;
    const bool occluding = (ix.metric == M_IP);
    const float alpha = cfg.alpha;
    const float inc = alpha < 1.2f ? alpha : 1.2f;
    const float kMax = 3.402823466e+38f;
    float cur_alpha = 1.0f;
    uint32_t found = 0, nexact = 0, nasked = 0;
    uint32_t my_sel = kEmpty;  // lane c < found: sorted position of the c-th selected entry
    float my_njj = 0.0f;       // its squared norm
    const int v = lane % G;
    const SqParams sqp{ix.sq_k, ix.sq_shift_norm_sq};
    const uint32_t col_lo = lane < gc.ncols ? lane : 0u, col_hi = lane + 64u < gc.ncols ? lane + 64u : 0u;
    while (N > 0 && found < degree) {
        uint32_t i0 = 0;
        while (i0 < N && found < degree) {
            // ---- a window of 64 candidates: who needs a visit in this pass
            const uint32_t wi = i0 + lane;
            float wocc = kMax;
            uint32_t wlast = 0, wsid = kEmpty;
            if (wi < N) {
                wocc = occ[wi];
                wlast = last[wi];
                wsid = sid[wi];
            }
            const bool need = wi < N && wocc != kMax && !(occluding && wocc > cur_alpha);
            uint64_t nm = ballot64(need);
            if (!nm) {
                i0 += kWave;
                continue;
            }
            uint32_t idx[B];
            uint32_t nb = 0;
#pragma unroll
            for (int j = 0; j < B; ++j) {
                if (nm) {
                    idx[j] = i0 + (uint32_t)__builtin_ctzll(nm);
                    nm &= nm - 1;
                    nb = (uint32_t)j + 1u;
                } else {
                    idx[j] = idx[j > 0 ? j - 1 : 0];
                }
            }
            // ---- their Gram rows, all requests up front (clamped, unconditional), parked in LDS: the visits below
            //      then run as an ordinary loop (one copy of the code) and pick G(i, sel_c) with one LDS read
            {
                float rlo[B], rhi[B];
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    const uint32_t r = idx[j] < gc.nrows ? idx[j] : 0u;
                    const float* row = gc.g + (size_t)r * gc.ld;
                    rlo[j] = row[col_lo];
                    rhi[j] = row[col_hi];
                }
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    rowsl[j * 128 + (int)lane] = rlo[j];
                    rowsl[j * 128 + 64 + (int)lane] = rhi[j];
                }
            }
            uint32_t* idxl = reinterpret_cast<uint32_t*>(rowsl + B * 128);  // the block's candidate indices
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < B; ++j) idxl[j] = idx[j];
            }
            wave_sync();
            // ---- the visits, in order
            for (uint32_t j = 0; j < nb && found < degree; ++j) {
                const uint32_t i = idxl[j];
                const int wl = (int)(i - i0);
                uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)wlast, wl);
                const uint32_t idi = (uint32_t)__builtin_amdgcn_readlane((int)wsid, wl);
                if (idi == location || idi >= ix.nslots) {  // excluded / not retrievable
                    if (lane == 0) occ[i] = kMax;
                    continue;
                }
                const bool irow = i < gc.nrows;
                const float gii = irow ? nrml[i] : 0.0f;
                const float di = sd[i];
                const float thr = cur_alpha * di;  // occluding rule: d_jk < alpha * d_ik (config/mod.rs:98)
                const uint8_t* xi = ix.rows + (uint64_t)idi * ix.row_stride;
                // G(i, sel_c) out of the parked row
                const float gsel = rowsl[j * 128u + (my_sel & 127u)];
                const bool have = lane < found && my_sel < i;  // the lazy scan skips selected entries that sort after i
                int cls = 0;  // 0: certainly not, 1: certainly exceeds, 2: the error interval does not decide / not covered
                if (have) {
                    cls = 2;
                    if (irow && my_sel < gc.ncols) {
                        const float gij = gsel;
                        const float nsum = gii + my_njj;
                        float dp;
                        if (OP == OP_L2) dp = nsum - 2.0f * gij;
                        else dp = NORM ? 1.0f - gij : -gij;
                        const float e = gc.escale * (gc.c1 * nsum + gc.c2 * __builtin_fabsf(dp));
                        const float lo = dp - e, hi = dp + e;
                        if (occluding) {
                            if (hi < thr) cls = 1;
                            else if (lo >= thr) cls = 0;
                        } else if (lo > 0.0f && di >= 0.0f) {
                            const float rmin = di / hi, rmax = di / lo;
                            if (rmin > cur_alpha * 1.000001f) cls = 1;
                            else if (rmax < cur_alpha * 0.999999f) cls = 0;
                        }
                    }
                }
                const uint64_t valid = ballot64(have), m1 = ballot64(cls == 1), m2 = ballot64(cls == 2);
                // first selected entry in sel[a..b) that makes update_occlude exceed the current alpha, or b
                auto first_exceed = [&](uint32_t a, uint32_t b) -> uint32_t {
                    const uint64_t below_b = b >= 64u ? ~0ull : ((1ull << b) - 1ull);
                    const uint64_t range = below_b & ~((1ull << a) - 1ull);
                    uint64_t tu = (m1 | m2) & range;
                    while (tu) {
                        const int f = __builtin_ctzll(tu);
                        const uint64_t upto = f >= 63 ? ~0ull : ((2ull << f) - 1ull);
                        if ((m1 >> f) & 1ull) {
                            nasked += (uint32_t)__popcll(valid & range & upto);
                            return (uint32_t)f;
                        }
                        // bit-exact pair distances, one lane group per pair: the undecided / uncovered entries that
                        // follow in scan order (up to the next certain one) are evaluated together -- the pairs a Gram
                        // block does not cover come in runs (the selected entries beyond its last column), and one
                        // evaluation costs a dependent fetch of two rows whether one group works or all of them.
                        // Consumed in scan order; the lazy scan stops at the first that exceeds (the rest is discarded).
                        int fs[GROUPS];
                        int ne = 0;
                        {
                            uint64_t t2 = tu;
#pragma unroll
                            for (int q = 0; q < GROUPS; ++q) {
                                fs[q] = 0;
                                if (t2 && ne == q) {
                                    const int f2 = __builtin_ctzll(t2);
                                    if (!((m1 >> f2) & 1ull)) {
                                        fs[q] = f2;
                                        ne = q + 1;
                                        t2 &= t2 - 1;
                                    }
                                }
                            }
                        }
                        uint32_t my_rp = 0;
#pragma unroll
                        for (int q = 0; q < GROUPS; ++q) {
                            const uint32_t rq = (uint32_t)__builtin_amdgcn_readlane((int)my_sel, fs[q]);
                            if (g == q) my_rp = rq;
                        }
                        const bool evalme = g < ne;
                        const uint8_t* y = ix.rows + (uint64_t)(evalme ? sid[my_rp] : idi) * ix.row_stride;
                        const float d = finish_distance<DT, OP, NORM>(group_distance_rows<DT, OP>(xi, y, (int)ix.dim, v), xi, y,
                                                                      ix.dim, sqp);
                        nexact += (uint32_t)ne;
                        for (int q = 0; q < ne; ++q) {
                            const float dg = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d), q * G));
                            const int fq = fs[q];
                            if (update_occlude<OP>(di, dg, 0.0f, cur_alpha, occluding) > cur_alpha) {
                                const uint64_t uq = fq >= 63 ? ~0ull : ((2ull << fq) - 1ull);
                                nasked += (uint32_t)__popcll(valid & range & uq);
                                return (uint32_t)fq;
                            }
                            tu &= ~(1ull << fq);
                        }
                    }
                    nasked += (uint32_t)__popcll(valid & range);
                    return b;
                };
                // TriangleInequality kind: the stored maximum ratio is only ever compared with the current alpha; it is
                // re-derived from the entries already examined (sel[0..l))
                if (!occluding && l != 0 && first_exceed(0, l) != l) continue;
                bool rejected = false;
                if (l != found) {
                    const uint32_t at = first_exceed(l, found);
                    if (at != found) {
                        l = at + 1;
                        rejected = true;
                    } else {
                        l = found;
                    }
                }
                if (lane == 0) {
                    last[i] = (uint16_t)l;
                    if (rejected) {
                        if (occluding) occ[i] = cur_alpha + 0.01f;
                    } else {
                        occ[i] = kMax;
                        sel[found] = i;
                    }
                }
                if (!rejected) {
                    if (lane == found) {
                        my_sel = i;
                        my_njj = gii;
                    }
                    ++found;
                }
            }
            wave_sync();  // lane 0's state updates before the next window is read
            i0 = idxl[nb - 1u] + 1u;
        }
        if (cur_alpha == alpha) break;
        const float next = cur_alpha * inc;
        cur_alpha = next < alpha ? next : alpha;
    }
    wave_sync();
    uint32_t nout = found;
    if (force_saturate || (cfg.saturate_after_prune && alpha > 1.0f)) {
        for (uint32_t i = 0; i < N && nout < degree; ++i) {
            const uint32_t id = sid[i];
            if (id == location) continue;
            bool dup = false;
            for (uint32_t n = lane; n < nout; n += kWave) dup |= (sid[sel[n]] == id);
            if (ballot64(dup)) continue;
            if (lane == 0) sel[nout] = i;
            ++nout;
            wave_sync();
        }
    }
    wave_sync();
    for (uint32_t n = lane; n < nout; n += kWave) out[1 + n] = sid[sel[n]];
    if (lane == 0) {
        out[0] = nout;
        if (cfg.counters) {
            atomicAdd(&stat_stripe(cfg.counters)[0], (unsigned long long)nexact);
            atomicAdd(&stat_stripe(cfg.counters)[4], (unsigned long long)nasked);
            atomicAdd(&stat_stripe(cfg.counters)[5], (unsigned long long)nexact);
        }
    }
}

// ======================================================================================================
// Pool prune (phase 1 of multi_insert: robust_prune_with, index.rs:2476-2532) on the matrix cores, three kernels:
//   pool_sort_kernel   one wave per inserted point: pool + intra-batch extras -> SortedNeighbors::new, the sorted
//                      (id, distance) list goes to global memory;
//   gram_tiles_kernel  (gram_tiles.hip) one 8-wave workgroup per point: the lower-triangular 32 x 32 tiles of
//                      G = C[0..ng) x C[0..mg)^T (the selected candidates come from the front of the sorted pool, and the
//                      sweep only ever asks for pairs (i, j) with j < i) with v_mfma_f32_32x32x2_f32, the tiles dealt out
//                      to the waves one at a time; rows streamed through two 32-column LDS slabs (the next slab's global
//                      loads in flight under the MFMAs, written to the other slab behind them, one barrier per slab);
//                      nothing else lives in this kernel: 128 registers, no scratch, two workgroups per CU (three for
//                      the short back-edge lists).  1 M x 768: 70 % of the matrix pipes' cycles in the 16 384-point
//                      launches (profiles/r04q_gram_tiles_pmc_*.csv), 91 TFLOP/s over the whole build;
//   pool_sweep_kernel  one wave per point at full occupancy: the sweep of prune::robust_prune with look-ups in G
//                      (global memory, L2 / Infinity-Cache resident) and the bit-exact row kernel where the error
//                      interval does not decide or the pair lies outside the block.
// The fused form (sort + Gram + sweep in one 4-wave workgroup, 75 KB of LDS) ran two sweeps per CU and lost to the row
// kernel (1 M x 768: 4.84 s vs 3.24 s); here the serial sweep and the Gram no longer share a workgroup.
// f16 rows run on the f16 matrix core, or widened exactly through the f32 one (the two kernels of gram_tiles.hip).
// ======================================================================================================
struct SortArgs {
    PoolArgs p;
    uint32_t* sid;   // n x pcap: ids in sorted pool order
    float* sd;       // n x pcap: their distances to the location
    uint32_t* sn;    // n: sorted pool length after the max_occlusion cut (0 = the pool overflowed)
};

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void pool_sort_kernel(SortArgs sa) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    using S = Scheme<DT, OP, true>;
    constexpr int G = S::G, GROUPS = kWave / G;
    const PoolArgs& a = sa.p;
    const uint32_t lane = threadIdx.x, wi = blockIdx.x, item = a.pos0 + blockIdx.x;
    const PoolLds L = pool_lds_layout(a.pcap, a.cfg.pruned_degree);
    uint32_t* pid = reinterpret_cast<uint32_t*>(smem + L.pid_off);
    float* pd = reinterpret_cast<float*>(smem + L.pd_off);
    const uint32_t* sid = reinterpret_cast<const uint32_t*>(smem + L.sid_off);
    const float* sd = reinterpret_cast<const float*>(smem + L.sd_off);
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
    uint32_t nex = 0;
    if (a.cand != 0 && a.n > 1) nex = a.cand < a.n - 1 ? a.cand : a.n - 1;
    if ((cnt + nex > a.pcap) || (a.into_rows && cnt + nex == 0)) {
        if (lane == 0 && cnt + nex != 0) {
            *a.err = 1;
            if (!a.into_rows) a.out[(uint64_t)wi * a.out_stride] = 0;
        }
        if (lane == 0) {
            sa.sn[wi] = 0;
        }
        return;
    }
    for (uint32_t i = lane; i < cnt; i += kWave) {
        pid[i] = a.pool_ids[lo + i];
        pd[i] = a.pool_d[lo + i];
    }
    if (nex) {  // extras = around(ids, position, cand) (utils/async_tools.rs:51-131), as pool_prune_kernel
        const uint32_t half = (nex + 1) / 2;
        const uint32_t start = item >= half ? item - half : a.n - (half - item);
        const uint8_t* x = a.ix.rows + (uint64_t)loc * a.ix.row_stride;
        const int g = lane / G, v = lane % G;
        for (uint32_t r0 = 0; r0 < nex; r0 += GROUPS) {
            const uint32_t r = r0 + g;
            if (r < nex) {
                uint32_t p = start + r;
                const uint32_t dist_to_item = item >= start ? item - start : item + a.n - start;
                if (r >= dist_to_item) p += 1;
                p %= a.n;
                const uint32_t id = a.locs[p];
                const uint8_t* y = a.ix.rows + (uint64_t)id * a.ix.row_stride;
                const float d = finish_distance<DT, OP, NORM>(group_distance_rows<DT, OP>(x, y, (int)a.ix.dim, v), x, y,
                                                              a.ix.dim, SqParams{a.ix.sq_k, a.ix.sq_shift_norm_sq});
                if (v == 0) {
                    pid[cnt + r] = id;
                    pd[cnt + r] = d;
                }
            }
        }
        if (lane == 0 && a.cfg.counters) atomicAdd(&stat_stripe(a.cfg.counters)[1], (unsigned long long)nex);
    }
    wave_sync();
    const uint32_t N = sort_pool_wave(a.cfg, cnt + nex, a.pcap, smem, L);
    uint32_t* gs = sa.sid + (uint64_t)wi * a.pcap;
    float* gd = sa.sd + (uint64_t)wi * a.pcap;
    for (uint32_t i = lane; i < N; i += kWave) {
        gs[i] = sid[i];
        gd[i] = sd[i];
    }
    if (lane == 0) sa.sn[wi] = N;
}

struct SweepArgs {
    PoolArgs p;
    const uint32_t* sid;
    const float* sd;
    const uint32_t* sn;
    const float* gram;
    const float* nrm;
    uint32_t ng, mg;
    float escale, c1, c2;
    // back-edge prunes (add_edge_and_prune): the location of item i is out_loc[i] and the result goes straight into its
    // adjacency row (nobody else reads that row during the back-edge phase); null = pool prune (p.locs, p.out)
    const uint32_t* out_loc = nullptr;
    uint32_t one_by_one = 0;         // development switch (DANN_DBG_SWEEP_ONE_BY_ONE): the candidate-at-a-time sweep
    const uint32_t* order = nullptr; // optional: workgroup b works on item order[b] (longest lists first)
    uint32_t compact_lds = 0;        // sweep_lds_layout instead of pool_lds_layout (the batched sweep only)
};

// the batched sweep (sweep_gram_batched) serves this launch: one lane per selected entry, at most 128 Gram columns
inline bool sweep_is_batched(const PruneCfg& cfg, uint32_t mg, uint32_t one_by_one) {
    return cfg.pruned_degree <= (uint32_t)kWave && mg <= 128u && !one_by_one;
}
inline size_t sweep_lds_bytes(const SweepArgs& sw) {
    const uint32_t pool = sw.compact_lds ? sweep_lds_layout(sw.p.pcap, sw.p.cfg.pruned_degree).total
                                         : pool_lds_layout(sw.p.pcap, sw.p.cfg.pruned_degree).total;
    return (((size_t)pool + 15u) & ~(size_t)15u) + kSweepRowsLds;
}

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void pool_sweep_kernel(SweepArgs sa) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const PoolArgs& a = sa.p;
    const uint32_t lane = threadIdx.x, wi = sa.order ? sa.order[blockIdx.x] : blockIdx.x, item = a.pos0 + wi;
    const uint32_t N = sa.sn[wi];
    if (N == 0) {  // pool prune: overflow (reported by pool_sort_kernel) or an empty pool; back-edges: nothing to prune
        if (lane == 0 && !sa.out_loc) a.out[(uint64_t)wi * a.out_stride] = 0;
        return;
    }
    const PoolLds L = sa.compact_lds ? sweep_lds_layout(a.pcap, a.cfg.pruned_degree) : pool_lds_layout(a.pcap, a.cfg.pruned_degree);
    uint32_t* sid = reinterpret_cast<uint32_t*>(smem + L.sid_off);
    float* sd = reinterpret_cast<float*>(smem + L.sd_off);
    float* occ = reinterpret_cast<float*>(smem + L.occ_off);
    uint16_t* last = reinterpret_cast<uint16_t*>(smem + L.last_off);
    const uint32_t* gs = sa.sid + (uint64_t)wi * a.pcap;
    const float* gd = sa.sd + (uint64_t)wi * a.pcap;
    for (uint32_t i = lane; i < N; i += kWave) {
        sid[i] = gs[i];
        sd[i] = gd[i];
        occ[i] = 0.0f;
        last[i] = 0;
    }
    wave_sync();
    const uint32_t nr = N < sa.ng ? N : sa.ng, nc = N < sa.mg ? N : sa.mg;
    const uint32_t location = sa.out_loc ? sa.out_loc[wi] : a.locs[item];
    uint32_t* out = sa.out_loc ? a.ix.adj + (uint64_t)location * a.ix.adj_stride : a.out + (uint64_t)wi * a.out_stride;
    const GramCtx gc{sa.gram + (uint64_t)wi * sa.ng * sa.mg, sa.nrm + (uint64_t)wi * sa.ng, sa.mg,
                     nr, nc, true, sa.escale, sa.c1, sa.c2, false, true};
    if (sa.compact_lds)
        sweep_gram_batched<DT, OP, NORM>(a.ix, a.cfg, location, N, smem, L, a.force_saturate != 0, out, gc,
                                         reinterpret_cast<float*>(smem + ((L.total + 15u) & ~15u)));
    else
        sweep_sorted_pool_gram<DT, OP, NORM>(a.ix, a.cfg, location, N, smem, L, a.force_saturate != 0, out, gc);
    if (lane == 0 && sa.out_loc && a.cfg.counters) atomicAdd(&stat_stripe(a.cfg.counters)[6], 1ull);
}

// back-edges on the matrix cores, first of three kernels (the other two are gram_tiles_kernel and pool_sweep_kernel):
// one wave per target of the short worklist builds the list adj(target) ++ unique new sources exactly as
// backedge_kernel does, appends when it still fits, and otherwise evaluates d(target, c) for the list, sorts it
// (SortedNeighbors::new) and leaves the sorted (id, distance) list in global memory for the Gram and the sweep.
struct BackListArgs {
    BackArgs b;
    uint32_t* sid;   // n x pcap
    float* sd;
    uint32_t* sn;    // n: sorted list length, 0 = nothing to prune for this item
    uint32_t* loc;   // n: the target
};

template <int DT, int OP, bool NORM>
__global__ __launch_bounds__(kWave) void backedge_list_kernel(BackListArgs la) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const BackArgs& a = la.b;
    const uint32_t lane = threadIdx.x, wi = blockIdx.x, seg = a.work ? a.work[wi] : wi;
    const PoolLds L = pool_lds_layout(a.pcap, a.cfg.pruned_degree);
    uint32_t* pid = reinterpret_cast<uint32_t*>(smem + L.pid_off);
    float* pd = reinterpret_cast<float*>(smem + L.pd_off);
    const uint32_t* sid = reinterpret_cast<const uint32_t*>(smem + L.sid_off);
    const float* sd = reinterpret_cast<const float*>(smem + L.sd_off);
    const uint32_t start = a.seg_start[seg];
    const uint32_t src = (uint32_t)(a.keys[start] >> 32);
    uint32_t* arow = a.ix.adj + (uint64_t)src * a.ix.adj_stride;
    if (lane == 0) {
        la.sn[wi] = 0;
        la.loc[wi] = src;
    }
    uint32_t len = arow[0];
    len = len < a.ix.max_degree ? len : a.ix.max_degree;
    for (uint32_t i = lane; i < len; i += kWave) pid[i] = arow[1 + i];
    wave_sync();
    // extend_from_slice(sorted sources): unique append
    uint32_t cnt = len;
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
            if (lane == 0) *a.err = 1;
            return;
        }
        if (take) pid[cnt + mbcnt(tm)] = id;
        cnt += ntake;
    }
    wave_sync();
    const uint32_t added = cnt - len;
    if (added == 0) return;
    if (cnt <= a.cfg.max_degree) {  // append_vector with the provider-capacity clamp (provider.rs:795-822)
        const uint32_t slack = a.ix.max_degree - len;
        const uint32_t take = added < slack ? added : slack;
        for (uint32_t i = lane; i < take; i += kWave) arow[1 + len + i] = pid[len + i];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            arow[0] = len + take;
        }
        return;
    }
    fill_list_distances<DT, OP, NORM>(a.ix, src, pid, pd, cnt);
    if (lane == 0 && a.cfg.counters) atomicAdd(&stat_stripe(a.cfg.counters)[1], (unsigned long long)cnt);
    wave_sync();
    const uint32_t N = sort_pool_wave(a.cfg, cnt, a.pcap, smem, L);
    uint32_t* gs = la.sid + (uint64_t)wi * a.pcap;
    float* gd = la.sd + (uint64_t)wi * a.pcap;
    for (uint32_t i = lane; i < N; i += kWave) {
        gs[i] = sid[i];
        gd[i] = sd[i];
    }
    if (lane == 0) la.sn[wi] = N;
}

// the three kernels of the MFMA pool prune: float rows (f32 / f16), L2 / inner product / cosine-normalized
template <class Kernel, class Args>
int32_t launch_float_rows(const IndexView& ix, Kernel kernel, const char* what, const Args& a, uint32_t grid, size_t lds,
                          hipStream_t stream) {
    const int32_t rc = visit_row_op<kRowsFloat>(ix.dtype, ix.metric, [&](auto r) -> int32_t {
        if constexpr (decltype(r)::op != OP_COS)
            return launch_kernel<decltype(kernel(r))::fn>(what, dim3(grid), dim3(kWave), lds, stream, a);
        return DANN_EUNSUPPORTED;
    });
    return rc == kNoMetric || rc == kNoRow ? DANN_EUNSUPPORTED : rc;
}
constexpr auto kPoolSort = [](auto r) { using R = decltype(r); return KernelOf<pool_sort_kernel<R::dt, R::op, R::norm>>{}; };
constexpr auto kPoolSweep = [](auto r) { using R = decltype(r); return KernelOf<pool_sweep_kernel<R::dt, R::op, R::norm>>{}; };
constexpr auto kBackedgeList = [](auto r) { using R = decltype(r); return KernelOf<backedge_list_kernel<R::dt, R::op, R::norm>>{}; };

// the order of the Gram / sweep workgroups of one slice (lpt_order_kernel)
const uint32_t* longest_first(BuildScratch& s, const uint32_t* sn, uint32_t m, hipStream_t st) {
    if (m < 4096u) return nullptr;  // (a launch that does not fill the chip twice has no tail to shorten)
    launch_lpt_order(sn, m, s.g_order.as<uint32_t>(), st);
    return s.g_order.as<uint32_t>();
}

}  // namespace

int32_t launch_pool_sort(BuildScratch& s, const PoolArgs& p, uint32_t m, hipStream_t st) {
    SortArgs so;
    so.p = p;
    so.sid = s.g_sid.as<uint32_t>();
    so.sd = s.g_sd.as<float>();
    so.sn = s.g_sn.as<uint32_t>();
    return launch_float_rows(p.ix, kPoolSort, "pool_sort_kernel launch", so, m, pool_lds_layout(p.pcap, p.cfg.pruned_degree).total, st);
}

int32_t launch_backedge_list(BuildScratch& s, const BackArgs& b, uint32_t m, hipStream_t st) {
    BackListArgs la;
    la.b = b;
    la.sid = s.g_sid.as<uint32_t>();
    la.sd = s.g_sd.as<float>();
    la.sn = s.g_sn.as<uint32_t>();
    la.loc = s.g_loc.as<uint32_t>();
    return launch_float_rows(b.ix, kBackedgeList, "backedge_list_kernel launch", la, m,
                             pool_lds_layout(b.pcap, b.cfg.pruned_degree).total, st);
}

int32_t gram_tiles_and_sweep(dann_index* idx, BuildScratch& s, const PoolArgs& p, uint32_t m, uint32_t ng, uint32_t mg,
                             const uint32_t* out_loc) {
    hipStream_t st = idx->main.stream;
    TileArgs ta;
    ta.ix = p.ix;
    ta.sid = s.g_sid.as<uint32_t>();
    ta.sn = s.g_sn.as<uint32_t>();
    ta.pcap = p.pcap;
    ta.ng = ng;
    ta.mg = mg;
    ta.gram = s.g_gram.as<float>();
    ta.nrm = s.g_nrm.as<float>();
    ta.counters = p.cfg.counters;
    ta.order = longest_first(s, ta.sn, m, st);
    if (int32_t trc = s.tile_begin(st)) return trc;
    int32_t rc = launch_gram_tiles(ta, m, st, idx->dbg_u32(DANN_DBG_GRAM_F16_WIDEN, 0u) == 0u);
    if (rc != DANN_OK) return rc;
    if (int32_t trc = s.tile_end(st)) return trc;
    SweepArgs sw;
    sw.p = p;
    sw.sid = ta.sid;
    sw.sd = s.g_sd.as<float>();
    sw.sn = ta.sn;
    sw.gram = ta.gram;
    sw.nrm = ta.nrm;
    sw.ng = ng;
    sw.mg = mg;
    sw.escale = (float)idx->dbg_value(DANN_DBG_GRAM_ESCALE, 1.0);  // test hook
    sw.c1 = gram_c1_chained(p.ix.dim);
    sw.c2 = gram_c2_for_dim(p.ix.dim);
    sw.one_by_one = idx->dbg_u32(DANN_DBG_SWEEP_ONE_BY_ONE, 0u) ? 1u : 0u;  // development switch
    sw.order = ta.order;
    sw.out_loc = out_loc;
    sw.compact_lds = sweep_is_batched(p.cfg, mg, sw.one_by_one) ? 1u : 0u;
    return launch_float_rows(p.ix, kPoolSweep, "pool_sweep_kernel launch", sw, m, sweep_lds_bytes(sw), st);
}

}  // namespace dann
