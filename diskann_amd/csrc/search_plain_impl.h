// beam_search_plain: the one-wave beam search of beam_search_one for the launches the throughput numbers come from --
// float rows of 128 elements, plain mode (beam width 1, no tags, degree <= 64, no filter), a plain Knn search, at most
// 128 queue entries -- with the hop written for the scalar unit ("The plain float hop"; 3.7 has the
// measurements the style comes from).  Same algorithm, same arithmetic, same order of queue inserts as beam_search_one:
// ids, distances and counters are those of beam_search_one bit for bit.  What differs is how the hop is written:
//   * nothing the hop does not read is live across it: the record, range and insert-time searches of this instantiation
//     stay with beam_search_one (beam_search_kernel picks by one wave-uniform test before the search), and the frozen
//     visited table with its spill table has a hop loop of its own (`hop_loop(true)`), entered from the open loop when the
//     table freezes.  Its state does not exist while the table is open;
//   * the open 32-bit table takes a hop's ids in one straight body all lanes run until the last is done
//     (ht_insert_flat, the counterpart of ht16_insert_flat);
//   * a lane that has nothing to store stores to its own sink instead of branching around the store: 8 bytes per lane
//     in the staged query, which is dead once the query slice is in registers; loads are issued on clamped addresses and
//     selected afterwards; lane predicates are combined with & and |.
// Included by search_kernel_impl.h, after beam_search_one.
#pragma once

namespace dann {
namespace {

// Insert into the open 32-bit table without a per-lane branch: same probe sequence and table contents as ht_insert_open.
// A lane with nothing (more) to insert swaps `own`, a dword of LDS that is its alone.  Double hashing over a prime
// number of slots visits every slot within `mod` probes and the open table always has an empty one, so `mod` trips bound
// the loop; *stuck is set should they ever run out (the query then reports an overflow and is re-run).
__device__ __forceinline__ bool ht_insert_flat(uint32_t* ht, uint32_t mod, uint32_t id, bool active, uint32_t* own, bool* stuck) {
    uint32_t h = __umulhi(id * 2654435761u, mod);
    const uint32_t step = 1u + __umulhi(id * 2246822519u + 0x9E3779B9u, mod - 1u);
    bool pending = active, isnew = false;
    uint32_t trips = 0;
    uint64_t left;
    do {
        uint32_t* const wp = pending ? ht + h : own;
        const uint32_t old = atomicCAS(wp, kEmpty, id);
        const bool took = old == kEmpty, same = old == id;
        isnew = isnew | (pending & took);
        pending = pending & !took & !same;
        h += step;
        h = h >= mod ? h - mod : h;
        left = ballot64(pending);
        ++trips;
    } while (left != 0 && trips < mod);
    *stuck = left != 0;
    return isnew;
}

template <int DT, int OP, bool NORM, int QS, bool HT16>
__device__ __forceinline__ void beam_search_plain(const SearchArgs& a, const uint32_t slot, uint8_t* smem) {
    static_assert(DT == DT_F32 || DT == DT_F16, "float rows");
    static_assert(QS >= 1 && QS <= 2, "at most 128 queue entries");
    constexpr int DIM = 128;
    using S = Scheme<DT, OP, false>;
    constexpr int G = S::G, GROUPS = kWave / G, U = kGatherRows, NTQ = DIM / (4 * G);
    static_assert(GROUPS * U * 2 == kWave, "a hop's candidates take at most two gather trips");
    static_assert(U == 4, "the gather has a body for each of 1 .. 4 passes");
    using RT = typename RowType<DT>::type;

    const IndexView& ix = a.ix;
    const uint32_t lane = threadIdx.x;
    const uint32_t qi = a.qmap ? a.qmap[slot] : slot;
    const SearchLds L = search_lds_layout(a.ht_entries, (uint32_t)kWave, lds_queue_entries(a), (uint32_t)DIM * 4u, false);
    float* const qs = reinterpret_cast<float*>(smem + L.q_off);
    uint32_t* const ht = reinterpret_cast<uint32_t*>(smem + L.ht_off);
    uint32_t* const cand_id = reinterpret_cast<uint32_t*>(smem + L.cand_id_off);
    float* const cand_d = reinterpret_cast<float*>(smem + L.cand_d_off);
    uint2* const stage = reinterpret_cast<uint2*>(smem + L.stage_off);
    // the lane's sink: 8 bytes of the staged query (used only after the query slice is in registers)
    uint2* const sink2 = reinterpret_cast<uint2*>(smem + L.q_off) + lane;
    uint32_t* const sink = reinterpret_cast<uint32_t*>(sink2);

    // ---- stage the query, wipe the table (as beam_search_one) ----------------------------------------------------------
    {
        const RT* src = reinterpret_cast<const RT*>(reinterpret_cast<const uint8_t*>(a.queries) + (uint64_t)qi * ix.qbytes);
        for (uint32_t i = lane; i < (uint32_t)DIM; i += kWave) qs[i] = load1(src + i);
        const u32x4 e4 = {kEmpty, kEmpty, kEmpty, kEmpty};
        for (uint32_t i = lane * 4u; i < a.ht_entries; i += kWave * 4u) *reinterpret_cast<u32x4*>(ht + i) = e4;
    }
    __syncthreads();
    const int g = lane / G, v = lane % G;
    F4 xq[NTQ];
#pragma unroll
    for (int t = 0; t < NTQ; ++t) xq[t] = load4(qs + t * 4 * G + 4 * v);

    // ---- what the hop reads, in locals ----------------------------------------------------------------------------------
    const uint8_t* const rows_base = ix.rows;
    const uint32_t* const adj_base = ix.adj;
    const uint32_t row_stride = (uint32_t)ix.row_stride;  // (below 4 GiB: dann_index_create) -- a row's address is one multiply-add
    const uint32_t adj_stride = ix.adj_stride, R = ix.max_degree, nslots = ix.nslots;
    const uint32_t qcap = a.l_value + ix.nstart;
    const uint32_t ht_mod = a.ht_prime, ht_open = a.ht_open;
    const Ht16 h16 = ht16_of(a);
    const bool row_prefetch = (a.tune & kTuneRowPrefetch) != 0;

    uint32_t qid[QS];
    float qd[QS];
#pragma unroll
    for (int s = 0; s < QS; ++s) {
        qid[s] = kEmpty;
        qd[s] = 0.0f;
    }
    uint32_t size = 0, cmps = 0, hops = 0, ht_count = 0, status = 0;
    uint32_t pf_node = kEmpty, pf_lenv = 0, pf_val = kEmpty, node0 = kEmpty;
    uint32_t pf_dummy = 0;  // landing register of the row-prefetch loads (latency mode)
    uint32_t* spill = nullptr;
#ifdef DANN_PHASE_CYCLES
    unsigned long long ph_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif

    // length (lane 0 of lenv) and neighbour `lane` of a node's adjacency row: two loads on the same cache lines
    auto adj_fetch = [&](uint32_t node, uint32_t& lenv, uint32_t& val) {
        const uint32_t* prow = adj_base + (uint64_t)node * adj_stride;
        lenv = prow[lane <= R ? lane : R];
        val = prow[1u + (lane < R ? lane : R - 1u)];
    };

    // distance of every candidate in cand_id[0..nc) -> cand_d: at most two trips of up to U passes, a pass being the
    // GROUPS rows the wave's groups take together.  A trip runs the passes that hold a candidate and no others: a hop
    // has 17.5 candidates on average for the trip's 32 slots.  One straight body per pass count, chosen by a
    // wave-uniform switch: each issues all its row loads before the first FMA (passes behind an `if` of their own
    // would wait for their loads one by one -- vmcnt is not counted across a branch).  Inside the last pass a slot
    // without a candidate reads row 0 and stores to the sink.
    auto passes = [&](uint32_t c0, uint32_t nc, auto np_tag) {
        constexpr int NP = decltype(np_tag)::value;
        const RT* rows[NP];
        bool act[NP];
        float out[NP];
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const uint32_t c = c0 + u * GROUPS + g;  // (< 64: inside the candidate block whatever nc)
            const uint32_t idv = cand_id[c];
            act[u] = c < nc;
            const uint32_t id = act[u] ? idv : 0u;
            rows[u] = reinterpret_cast<const RT*>(rows_base + (uint64_t)id * row_stride);
        }
        group_distance_passes<OP, DIM, NP>(xq, rows, v, out);
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const uint32_t c = c0 + u * GROUPS + g;
            float* const dst = (act[u] & (v == 0)) ? cand_d + c : reinterpret_cast<float*>(sink);
            *dst = post_op<OP, NORM>(out[u]);
        }
    };
    auto gather = [&](uint32_t nc) {
        for (uint32_t c0 = 0; c0 < nc; c0 += GROUPS * U) {
            const uint32_t left = nc - c0;
            const uint32_t np = left < (uint32_t)(GROUPS * U) ? (left + GROUPS - 1u) / GROUPS : (uint32_t)U;
#ifdef DANN_PHASE_CYCLES
            ph_acc[10 + np] += 1;  // trips by pass count: slots 11 .. 14
#endif
            switch (np) {
                case 1: passes(c0, nc, std::integral_constant<int, 1>{}); break;
                case 2: passes(c0, nc, std::integral_constant<int, 2>{}); break;
                case 3: passes(c0, nc, std::integral_constant<int, 3>{}); break;
                default: passes(c0, nc, std::integral_constant<int, 4>{}); break;
            }
        }
    };

    // merge the n (<= 64) candidates of cand_id / cand_d into the queue: beam_search_one's merge_regs (ranks, shifts and
    // tie rule unchanged), per-lane assignments as selects, stores through the sink
    bool stage_stale = false;
    auto merge = [&](uint32_t n) {
        bool has = lane < n;
        const float ndl = cand_d[lane];
        const uint32_t nidl = cand_id[lane];
        float nd = has ? ndl : 0.0f;
        uint32_t nid = has ? nidl : kEmpty;
        // a full queue drops what is worse than its last entry up front (queue.rs:142-146)
        const uint32_t lastp = size - 1u;
        float worst = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qd[0]), (int)(lastp & 63u)));
        if constexpr (QS == 2) {
            const float w1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qd[1]), (int)(lastp & 63u)));
            worst = (lastp >> 6) == 1u ? w1 : worst;
        }
        worst = ((size == qcap) & (qcap > 0u)) ? worst : __builtin_inff();  // (nothing is worse than +inf)
        const bool nvalid = has & !(nd != nd) & !(worst < nd);  // NaN distances are ignored (queue.rs:131-134)
        const uint64_t km = ballot64(nvalid);
        const uint32_t nv = (uint32_t)__popcll(km);
#ifdef DANN_PHASE_CYCLES
        ph_acc[8] += nv;
        ph_acc[9] += nv > kRegMerge ? 1 : 0;
        ph_acc[10] += 1;
#endif
        if (nv == 0) return;
        if (nv <= kSeqInsert) {
            for (uint64_t mm = km; mm; mm &= mm - 1) {
                const int j = __builtin_ctzll(mm);
                const float dj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nd), j));
                const uint32_t idj = (uint32_t)__builtin_amdgcn_readlane((int)nid, j);
                uint32_t pos = 0;
#pragma unroll
                for (int s = 0; s < QS; ++s)
                    pos += (uint32_t)__popcll(ballot64((((uint32_t)(s * kWave) + lane) < size) & (qd[s] < dj)));
                if (pos >= qcap) continue;  // behind a full queue's last entry (it was equal to it when tested, not any more)
#pragma unroll
                for (int s = QS - 1; s >= 0; --s) {
                    if (pos >= (uint32_t)((s + 1) * kWave) || size < (uint32_t)(s * kWave)) continue;  // slot untouched
                    const uint32_t p = (uint32_t)(s * kWave) + lane;
                    const int cd = s > 0 ? __builtin_amdgcn_readlane(__builtin_bit_cast(int, qd[s > 0 ? s - 1 : 0]), 63) : 0;
                    const int ci = s > 0 ? __builtin_amdgcn_readlane((int)qid[s > 0 ? s - 1 : 0], 63) : 0;
                    const int sd = __builtin_amdgcn_update_dpp(cd, __builtin_bit_cast(int, qd[s]), 0x138, 0xf, 0xf, false);
                    const int si = __builtin_amdgcn_update_dpp(ci, (int)qid[s], 0x138, 0xf, 0xf, false);
                    const bool up = p > pos, at = p == pos;
                    qd[s] = up ? __builtin_bit_cast(float, sd) : (at ? dj : qd[s]);
                    qid[s] = up ? (uint32_t)si : (at ? idj : qid[s]);
                }
                size = size < qcap ? size + 1u : qcap;
            }
            stage_stale = true;
            return;
        }
        uint32_t shift[QS];
        uint32_t pos_new = 0;
        if (nv <= kRegMerge) {
            uint32_t before = 0, lbound = 0;
#pragma unroll
            for (int s = 0; s < QS; ++s) shift[s] = 0;
            for (uint64_t mm = km; mm; mm &= mm - 1) {
                const int j = __builtin_ctzll(mm);
                const float dj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nd), j));
                before += (dj < nd) ? 1u : 0u;
                before += ((dj == nd) & ((uint32_t)j > lane)) ? 1u : 0u;
                uint32_t lb = 0;
#pragma unroll
                for (int s = 0; s < QS; ++s) {
                    shift[s] += (dj <= qd[s]) ? 1u : 0u;  // entries >= size: never scattered
                    lb += (uint32_t)__popcll(ballot64((((uint32_t)(s * kWave) + lane) < size) & (qd[s] < dj)));
                }
                lbound = (int)lane == j ? lb : lbound;
            }
            has = nvalid;
            pos_new = lbound + before;
        } else {
            if (stage_stale) {  // the lower-bound search below reads the queue's LDS image
#pragma unroll
                for (int s = 0; s < QS; ++s) {
                    const uint32_t p = (uint32_t)(s * kWave) + lane;
                    *(p < size ? stage + p : sink2) = make_uint2(qid[s], __builtin_bit_cast(uint32_t, qd[s]));
                }
                __syncthreads();
            }
            if (nv != n) {  // compact the survivors, emission order preserved
                const uint32_t cj = mbcnt(km);
                __syncthreads();
                *(nvalid ? cand_d + cj : reinterpret_cast<float*>(sink)) = nd;
                *(nvalid ? cand_id + cj : sink + 1) = nid;
                __syncthreads();
                has = lane < nv;
                const float cd = cand_d[lane];
                const uint32_t ci = cand_id[lane];
                nd = has ? cd : 0.0f;
                nid = has ? ci : kEmpty;
            }
            // rank among the survivors
            uint32_t before = 0;
            for (uint32_t jj = 0; jj < nv; ++jj) {
                const float dj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, nd), jj));
                before += ((dj < nd) | ((dj == nd) & (jj > lane))) ? 1u : 0u;
            }
            // (the sorted survivors go where the candidates came from: their content is in registers by now)
            float* const snew = reinterpret_cast<float*>(cand_id);
            *(has ? snew + before : reinterpret_cast<float*>(sink)) = nd;
            __syncthreads();
            // old elements: shift = #{new <= d_e}  (upper bound in snew[0..nv); reads past nv stay inside the two
            // candidate blocks and are masked out)
#pragma unroll
            for (int s = 0; s < QS; ++s) {
                uint32_t lo = 0;
#pragma unroll
                for (uint32_t step = 64; step > 0; step >>= 1) {
                    const uint32_t t = lo + step;
                    const float sv = snew[t - 1u];
                    lo = ((t <= nv) & (sv <= qd[s])) ? t : lo;
                }
                shift[s] = lo;
            }
            // new elements: #{old < d_j}  (lower bound in the queue image; a step past the queue reads entry 0)
            uint32_t lb = 0;
#pragma unroll
            for (uint32_t step = QS * kWave; step > 0; step >>= 1) {
                const uint32_t t = lb + step;
                const bool in = t <= size;
                const float sv = __builtin_bit_cast(float, stage[in ? t - 1u : 0u].y);
                lb = (in & (sv < nd)) ? t : lb;
            }
            pos_new = before + lb;
        }
        // scatter into the queue image, then reload
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const uint32_t p = (uint32_t)(s * kWave) + lane, np = p + shift[s];
            *(((p < size) & (np < qcap)) ? stage + np : sink2) = make_uint2(qid[s], __builtin_bit_cast(uint32_t, qd[s]));
        }
        *((has & (pos_new < qcap)) ? stage + pos_new : sink2) = make_uint2(nid, __builtin_bit_cast(uint32_t, nd));
        const uint32_t total = size + nv;
        size = total < qcap ? total : qcap;
        stage_stale = false;
        __syncthreads();
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const uint32_t p = (uint32_t)(s * kWave) + lane;
            const bool in = p < size;
            const uint2 e = stage[in ? p : 0u];
            qid[s] = in ? e.x : qid[s];
            qd[s] = in ? __builtin_bit_cast(float, e.y) : qd[s];
        }
    };

    // W == 1 pop (queue.rs:297-313): the first unexpanded entry goes to node0 and is marked; the second one is the node
    // the next hop expands unless a new candidate gets in front of it (the adjacency prefetch target)
    auto pop = [&](uint32_t& pf_next) -> uint32_t {
        uint32_t got = 0;
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            if (got >= 2u) continue;
            const bool cand = (((uint32_t)(s * kWave) + lane) < size) & !(qid[s] & kVisitedBit);
            uint64_t m = ballot64(cand);
            if (got == 0u && m) {
                const int l = __builtin_ctzll(m);
                node0 = (uint32_t)__builtin_amdgcn_readlane((int)qid[s], l);
                qid[s] |= (int)lane == l ? kVisitedBit : 0u;
                got = 1;
                m &= m - 1;
            }
            if (got == 1u && m) {
                pf_next = (uint32_t)__builtin_amdgcn_readlane((int)qid[s], __builtin_ctzll(m));
                got = 2;
            }
        }
        return got ? 1u : 0u;
    };

    // ---- start points: frozen slots [capacity, capacity + nstart) (index.rs:1950-1958), at most 64 in plain mode ------
    {
        const uint32_t ns = ix.nstart;
        uint32_t early = 0;
        if (lane < ns) {
            cand_id[lane] = ix.capacity + lane;
            if constexpr (HT16) {
                if (ht16_insert_open(ht, h16, ix.capacity + lane, true) == kHt16Exhausted) early = 1u;
            } else {
                ht_visit(ht, ht_mod, ix.capacity + lane, true);
            }
        }
        if (HT16 && ballot64(early != 0)) status = (uint32_t)(-DANN_EOVERFLOW);
        ht_count = ns;
        __syncthreads();
        gather(ns);
        __syncthreads();
        cmps = ns;
        merge(ns);
    }

    // ---- beam loop.  One body, compiled twice: with the visited table open (every hop of nearly every query) and with
    // it frozen (lookups in the LDS table, inserts into a spill table in global memory).  The open loop leaves for the
    // frozen one at the point beam_search_one freezes the table: before a hop's inserts when they could take the table
    // past ht_open, or (16-bit entries) in the middle of them when an id finds all its probes taken -- `resume` then
    // carries the lanes' results so far.  Returns true when the search has to go on with the table frozen.
    uint32_t nb, pf_next = kEmpty;
    bool resume = false, r_isnew = false, r_exh = false;
    uint32_t r_len = 0;
    auto hop_loop = [&](auto frozen_tag) -> bool {
        constexpr bool FROZEN = decltype(frozen_tag)::value;
        uint32_t spill_count = 0;
        const uint32_t spill_size = 1u << a.spill_bits, spill_mask = spill_size - 1u, spill_shift = 32u - a.spill_bits;
        for (;;) {
            PH_T(ph1);
            // ---- neighbours of node0 through the visited filter (provider.rs:448-454) into cand_id[0..nc)
            uint32_t len;
            bool isnew, inb;
            uint32_t id;
            bool spilled_hop = FROZEN;  // this hop's new ids count towards the spill table
            if (FROZEN && resume) {
                len = r_len;
                inb = lane < len;
                id = inb ? pf_val : kEmpty;
                isnew = r_isnew;
                if (r_exh) isnew = spill_insert(spill, spill_mask, spill_shift, id);
                resume = false;
            } else {
                const bool hit = node0 == pf_node;
#ifdef DANN_PHASE_CYCLES
                ph_acc[hit ? 5 : 6] += 1;
#endif
                if (!hit) {
                    adj_fetch(node0, pf_lenv, pf_val);
                    pf_node = node0;  // (the frozen loop, entered from below, finds the row where a hit leaves it)
                }
                len = (uint32_t)__builtin_amdgcn_readlane((int)pf_lenv, 0);
                len = len < R ? len : R;  // Neighbors::get clamps (neighbors.rs:146-148)
                if constexpr (!FROZEN) {
                    if (ht_count + len > ht_open) return true;  // freeze the table
                } else {
                    if (!spill || spill_count + len > spill_size - (spill_size >> 2)) {
                        status = (uint32_t)(-DANN_EOVERFLOW);
                        return false;
                    }
                }
                inb = lane < len;
                id = inb ? pf_val : kEmpty;
                // (HT16: the table holds ids below 2^m only; an id beyond the index is never a candidate anyway)
                const bool act = inb & (id != kEmpty) & (!HT16 | (id < nslots));
                if constexpr (!FROZEN) {
                    if constexpr (HT16) {
                        const uint32_t r = ht16_insert_flat(ht, h16, id, act, sink);
                        isnew = r == 1u;
                        const bool exh = r == 2u;
                        if (ballot64(exh)) {  // (rare) no slot among an id's probes: the table freezes in mid-hop
                            r_len = len;
                            r_isnew = isnew;
                            r_exh = exh;
                            resume = true;
                            return true;
                        }
                    } else {
                        bool stuck;
                        isnew = ht_insert_flat(ht, ht_mod, id, act, sink, &stuck);
                        if (stuck) {
                            status = (uint32_t)(-DANN_EOVERFLOW);
                            return false;
                        }
                    }
                } else {
                    isnew = false;
                    if (act) {  // frozen LDS table: lookup, then the spill table in global memory
                        if constexpr (HT16) isnew = !ht16_contains(ht, h16, id) && spill_insert(spill, spill_mask, spill_shift, id);
                        else isnew = ht_visit(ht, ht_mod, id, false) == kAbsent && spill_insert(spill, spill_mask, spill_shift, id);
                    }
                }
            }
            const bool keep = isnew & (id < nslots);
            const uint64_t nm = ballot64(isnew), km = ballot64(keep);
            *(keep ? cand_id + mbcnt(km) : sink) = id;
            const uint32_t nc = (uint32_t)__popcll(km);
            if (spilled_hop) spill_count += (uint32_t)__popcll(nm);
            else ht_count += (uint32_t)__popcll(nm);
            __syncthreads();
            PH_T(ph2);
            PH_ADD(1, ph1, ph2);
            // ---- the adjacency row of the best unexpanded entry of the current queue travels with the candidate rows: if
            // no new candidate beats it, the next hop starts without a dependent round trip.  (No such entry: node 0's
            // row is fetched and never used -- pf_node stays kEmpty.)
            pf_node = pf_next;
            adj_fetch(pf_node != kEmpty ? pf_node : 0u, pf_lenv, pf_val);
            gather(nc);
            // latency mode: touch the rows of the predicted next node's neighbours (see beam_search_one)
            asm volatile("" ::"v"(pf_dummy));
            if (row_prefetch && pf_node != kEmpty && ix.layer_bytes <= 512u) {
                const uint32_t plen = (uint32_t)__builtin_amdgcn_readlane((int)pf_lenv, 0);
                if ((lane < (plen < R ? plen : R)) & (pf_val < nslots)) {
                    const uint8_t* prow = rows_base + (uint64_t)pf_val * row_stride;
                    const uint32_t last = ix.layer_bytes >= 4u ? ix.layer_bytes - 4u : 0u;
                    const uint8_t* p1 = prow + (128u < last ? 128u : last);
                    const uint8_t* p2 = prow + (256u < last ? 256u : last);
                    const uint8_t* p3 = prow + (384u < last ? 384u : last);
                    const uint8_t* p4 = prow + last;
                    asm volatile(
                        "global_load_dword %0, %1, off\n\t"
                        "global_load_dword %0, %2, off\n\t"
                        "global_load_dword %0, %3, off\n\t"
                        "global_load_dword %0, %4, off\n\t"
                        "global_load_dword %0, %5, off"
                        : "+v"(pf_dummy)
                        : "v"(prow), "v"(p1), "v"(p2), "v"(p3), "v"(p4));
                }
            }
            __syncthreads();
            PH_T(ph3);
            PH_ADD(2, ph2, ph3);
            cmps += nc;
            merge(nc);
            PH_T(ph4);
            PH_ADD(3, ph3, ph4);
            // ---- pop the closest unexpanded entry (queue.rs:297-313)
            pf_next = kEmpty;
            nb = pop(pf_next);
            PH_T(ph5);
            PH_ADD(0, ph4, ph5);
            PH_ADD(4, ph1, ph5);
            if (nb == 0) return false;
            hops += 1u;
        }
    };
    nb = pop(pf_next);
    if (nb != 0 && !status) {
        hops += 1u;
        if (hop_loop(std::false_type{})) {
            // freeze the LDS table, claim a spill table: slices are recycled inside a launch (busy flag per slice,
            // rotating start)
            uint32_t slice = kEmpty;
            if (a.spill) {
                if (lane == 0) {
                    uint32_t* busy = a.spill_next + 16;
                    uint32_t s = atomicAdd(a.spill_next, 1u) % a.spill_slices;
                    for (uint32_t t = 0; t < 2u * a.spill_slices; ++t) {
                        if (atomicCAS(&busy[s], 0u, 1u) == 0u) {
                            slice = s;
                            break;
                        }
                        s = (s + 1 == a.spill_slices) ? 0u : s + 1;
                    }
                }
                slice = (uint32_t)__builtin_amdgcn_readfirstlane((int)slice);
            }
            if (slice < a.spill_slices) spill = a.spill + ((uint64_t)slice << a.spill_bits);
            if (resume && !spill) status = (uint32_t)(-DANN_EOVERFLOW);
            else hop_loop(std::true_type{});
        }
    }

    if (row_prefetch) {  // no prefetch load may still be in flight when its landing register is released
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("" ::"v"(pf_dummy));
    }
#ifdef DANN_PHASE_CYCLES
    if (lane == 0)
        for (int i = 0; i < 16; ++i) atomicAdd(&a.phase_cycles[i], ph_acc[i]);
#endif
    if (spill) {  // hand the spill table back clean
        const uint32_t spill_size = 1u << a.spill_bits;
        __syncthreads();
        spill_wipe(spill, spill_size, lane);
        __syncthreads();
        if (lane == 0) atomicExch(a.spill_next + 16 + (uint32_t)((spill - a.spill) >> a.spill_bits), 0u);
    }
    // ---- results: best entries in order, start points dropped (provider.rs:933-944) -----
    uint32_t written = 0;
    if (a.out_ids) {
        uint32_t* oi = a.out_ids + (uint64_t)qi * a.k;
        float* od = a.out_dists + (uint64_t)qi * a.k;
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const uint32_t p = (uint32_t)(s * kWave) + lane;
            const uint32_t id = qid[s] & ~kVisitedBit;
            const bool res = p < size && id < ix.capacity;
            const uint64_t m = ballot64(res);
            const uint32_t r = written + mbcnt(m);
            if (res && r < a.k) {
                oi[r] = id;
                od[r] = qd[s];
            }
            written += (uint32_t)__popcll(m);
        }
        written = written < a.k ? written : a.k;
        for (uint32_t r = written + lane; r < a.k; r += kWave) {
            oi[r] = kEmpty;
            od[r] = __builtin_inff();
        }
    }
    if (lane == 0) {
        if (a.stats) {
            dann_search_stats st;
            st.cmps = cmps;
            st.hops = hops;
            // Translate::post_process counts a push only while the buffer still has room afterwards
            // (provider.rs:933-944, search_output_buffer.rs:107-124): k - 1 when the buffer of length k fills
            st.result_count = (a.k && written == a.k) ? a.k - 1u : written;
            st.written = written;
            st.status = status;
            a.stats[qi] = st;
        }
        if (status && a.fail_flag) __hip_atomic_store(a.fail_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The launches of a float DIM = 128 plain instantiation that beam_search_plain serves: a Knn search of queries in
// memory.  Record, range and insert-time searches keep beam_search_kernel (launch_one decides, per launch).
inline bool plain_hop_serves(const SearchArgs& a) {
    return !a.range_ids && !a.rec_ids && !a.rec_n && !a.rec_max && !a.range_second && !a.qslots && !a.srv.ring && !a.team;
}

// beam_search_kernel's LOOP = 0 (one wave per query) and LOOP = 1 (persistent waves drawing query slots from a counter)
// around beam_search_plain.  A kernel of its own: compiled into beam_search_kernel beside beam_search_one, the two
// bodies share one register allocation and the headline instantiation spills 65 SGPRs instead of none.
template <int DT, int OP, bool NORM, int QS, int LOOP, bool HT16>
__global__ __launch_bounds__(kWave) DANN_SEARCH_KERNEL_ATTR void beam_search_plain_kernel(SearchArgs a) {
    static_assert(LOOP == 0 || LOOP == 1, "one-shot and persistent launches");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if constexpr (LOOP == 0) {
        beam_search_plain<DT, OP, NORM, QS, HT16>(a, blockIdx.x, smem);
    } else {
        uint32_t slot = blockIdx.x;
        for (;;) {
            uint32_t nxt = 0;  // the ticket for the search after this one is drawn now: its round trip hides behind the search
            if (threadIdx.x == 0) nxt = atomicAdd(a.work_next, 1u);
            beam_search_plain<DT, OP, NORM, QS, HT16>(a, slot, smem);
            __syncthreads();  // the next query reuses this wave's LDS
            slot = gridDim.x + (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt);
            if (slot >= a.nq) break;
        }
    }
}

}  // namespace
}  // namespace dann
