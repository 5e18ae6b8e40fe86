// diverse_queue.h -- DiverseNeighborQueue (diskann/src/neighbor/diverse_priority_queue.rs:63-238) for one wavefront.
//
// The reference keeps a global NeighborPriorityQueue of (id, attribute) with capacity L and one local
// NeighborPriorityQueue per attribute value with capacity dl = diverse_k * L / total_k.  NeighborPriorityQueue::remove
// (neighbor/queue.rs:197-222) only looks at the lower-bound position, so under equal distances it can fail: the local
// queues are neither a subset of the global queue nor its partition, and both are kept here as real state.
//
//   - global queue: sorted arrays (distance, id | kVisitedBit, attribute) of `L` entries plus the reference's cursor;
//   - local queues: one unsorted pool of (distance, insertion sequence, id, attribute).  A local queue's order is
//     (distance ascending, sequence descending) -- lower-bound insertion puts a new entry in front of equal distances
//     (queue.rs:142-170) -- so "is a's queue full", "a's worst entry" and "a's lower bound" are wave reductions over
//     the pool entries of attribute a.
//
// Every array may live in LDS or (the exact re-run of a query whose pool or visited table overflowed) in global
// memory: all accesses go through generic pointers and the wave synchronises after each write phase.
#pragma once
#include "dann_device.h"

namespace dann {

constexpr uint32_t kNoAttribute = 0xFFFFFFFFu;  // DANN_NO_ATTRIBUTE: AttributeValueProvider::get returned None

// (distance, sequence) -> one key whose ascending order is a local queue's order.  -0.0 is folded into +0.0: the
// reference compares distances as floats.
__device__ __forceinline__ unsigned long long dv_key(float d, uint32_t seq) {
    const uint32_t b = __builtin_bit_cast(uint32_t, d + 0.0f);
    const uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)o << 32) | (unsigned long long)(~seq);
}

__device__ __forceinline__ unsigned long long dv_wave_max(unsigned long long x) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long y = ((unsigned long long)(uint32_t)__shfl_xor((int)(x >> 32), s) << 32) |
                                     (uint32_t)__shfl_xor((int)(uint32_t)x, s);
        x = y > x ? y : x;
    }
    return x;
}
__device__ __forceinline__ unsigned long long dv_wave_min(unsigned long long x) { return ~dv_wave_max(~x); }

struct DiverseQueue {
    float* gd;        // global queue, L entries
    uint32_t* gid;    // id | kVisitedBit
    uint32_t* ga;     // attribute
    float* pd;        // local pool, pcap entries
    uint32_t* pseq;
    uint32_t* pid;
    uint32_t* pa;
    uint32_t L, dl, dk, pcap;
    uint32_t lane;
    // wave-uniform state
    uint32_t gsize = 0, cursor = 0, np = 0, seq = 0;
    float lmax = -__builtin_inff();  // an upper bound of every local distance (only grows): the exact pre-filter
    bool overflow = false;           // the pool is full: the query must be re-run with a larger one
    uint32_t failed_remove[2] = {0, 0};

    __device__ __forceinline__ void sync() const { __syncthreads(); }

    // NeighborPriorityQueue::get_lower_bound: first position with distance >= d
    __device__ uint32_t g_lower_bound(float d) const {
        uint32_t n = 0;
        for (uint32_t i0 = 0; i0 < gsize; i0 += 64) {
            const uint32_t i = i0 + lane;
            n += (uint32_t)__popcll(ballot64(i < gsize && gd[i] < d));
        }
        return n;
    }
    // NeighborPriorityQueue::insert, fixed capacity L (queue.rs:130-172)
    __device__ void g_insert(uint32_t id, float d, uint32_t at) {
        if (gsize == L && gd[L - 1] < d) return;
        const uint32_t pos = gsize ? g_lower_bound(d) : 0u;
        const uint32_t n = gsize == L ? L - 1u : gsize;
        for (uint32_t hi = n; hi > pos;) {  // shift [pos, n) up by one, highest chunk first
            const uint32_t lo = hi - pos > 64u ? hi - 64u : pos;
            const uint32_t i = lo + lane;
            float vd = 0.f;
            uint32_t vi = 0, va = 0;
            if (i < hi) {
                vd = gd[i];
                vi = gid[i];
                va = ga[i];
            }
            sync();
            if (i < hi) {
                gd[i + 1] = vd;
                gid[i + 1] = vi;
                ga[i + 1] = va;
            }
            sync();
            hi = lo;
        }
        if (lane == 0) {
            gd[pos] = d;
            gid[pos] = id;
            ga[pos] = at;
        }
        sync();
        gsize = n + 1u;
        if (pos < cursor) cursor = pos;
    }
    // NeighborPriorityQueue::remove (queue.rs:197-222): the entry at the lower bound must be (id, attribute)
    __device__ bool g_remove(uint32_t id, uint32_t at, float d) {
        if (gsize == 0) return false;
        const uint32_t pos = g_lower_bound(d);
        if (pos >= gsize || (gid[pos] & ~kVisitedBit) != id || ga[pos] != at) return false;
        for (uint32_t lo = pos + 1u; lo < gsize; lo += 64u) {
            const uint32_t i = lo + lane;
            float vd = 0.f;
            uint32_t vi = 0, va = 0;
            if (i < gsize) {
                vd = gd[i];
                vi = gid[i];
                va = ga[i];
            }
            sync();
            if (i < gsize) {
                gd[i - 1] = vd;
                gid[i - 1] = vi;
                ga[i - 1] = va;
            }
            sync();
        }
        gsize -= 1u;
        if (pos < cursor && cursor > 0) cursor -= 1u;
        return true;
    }
    __device__ bool has_notvisited() const { return cursor < (L < gsize ? L : gsize); }
    // NeighborPriorityQueue::closest_notvisited (queue.rs:297-313)
    __device__ uint32_t closest_notvisited() {
        const uint32_t cur = cursor;
        const uint32_t id = gid[cur] & ~kVisitedBit;
        sync();
        if (lane == 0) gid[cur] = id | kVisitedBit;
        sync();
        uint32_t c = gsize;
        for (uint32_t i0 = cur + 1u; i0 < gsize; i0 += 64u) {
            const uint32_t i = i0 + lane;
            const uint64_t m = ballot64(i < gsize && !(gid[i] & kVisitedBit));
            if (m) {
                c = i0 + (uint32_t)__builtin_ctzll(m);
                break;
            }
        }
        cursor = c;
        return id;
    }

    // the local queue of attribute `at`: its length and its last (worst) entry's pool position
    __device__ void l_scan(uint32_t at, uint32_t& count, uint32_t& worst_pos) const {
        uint32_t cnt = 0;
        unsigned long long best = 0ull;
        uint32_t bpos = kEmpty;
        for (uint32_t p0 = 0; p0 < np; p0 += 64u) {
            const uint32_t p = p0 + lane;
            const bool m = p < np && pa[p] == at;
            cnt += (uint32_t)__popcll(ballot64(m));
            if (m) {
                const unsigned long long k = dv_key(pd[p], pseq[p]);
                if (bpos == kEmpty || k > best) {
                    best = k;
                    bpos = p;
                }
            }
        }
        count = cnt;
        worst_pos = kEmpty;
        if (cnt) {
            const unsigned long long mx = dv_wave_max(bpos == kEmpty ? 0ull : best);
            const uint64_t who = ballot64(bpos != kEmpty && best == mx);
            worst_pos = (uint32_t)__builtin_amdgcn_readlane((int)bpos, (int)__builtin_ctzll(who));
        }
    }
    // local insert without eviction (the queue is not full)
    __device__ void l_append(uint32_t id, float d, uint32_t at) {
        if (np >= pcap) {
            overflow = true;
            return;
        }
        if (lane == 0) {
            pd[np] = d;
            pseq[np] = seq;
            pid[np] = id;
            pa[np] = at;
        }
        sync();
        ++np;
        ++seq;
        lmax = d > lmax ? d : lmax;
    }
    // local insert into a full queue: its last entry (pool position `pos`) is evicted
    __device__ void l_replace(uint32_t pos, uint32_t id, float d, uint32_t at) {
        if (lane == 0) {
            pd[pos] = d;
            pseq[pos] = seq;
            pid[pos] = id;
            pa[pos] = at;
        }
        sync();
        ++seq;
        lmax = d > lmax ? d : lmax;
    }
    // NeighborPriorityQueue::remove on the local queue of `at`: the entry at the lower bound of d must be `id`
    __device__ bool l_remove(uint32_t at, uint32_t id, float d) {
        const unsigned long long lo = dv_key(d, 0xFFFFFFFFu);  // (the smallest key of distance d)
        unsigned long long best = ~0ull;
        uint32_t bpos = kEmpty;
        for (uint32_t p0 = 0; p0 < np; p0 += 64u) {
            const uint32_t p = p0 + lane;
            if (p < np && pa[p] == at) {
                const unsigned long long k = dv_key(pd[p], pseq[p]);
                if (k >= lo && k < best) {
                    best = k;
                    bpos = p;
                }
            }
        }
        const unsigned long long mn = dv_wave_min(best);
        if (mn == ~0ull) return false;
        const uint64_t who = ballot64(bpos != kEmpty && best == mn);
        const uint32_t pos = (uint32_t)__builtin_amdgcn_readlane((int)bpos, (int)__builtin_ctzll(who));
        if (pid[pos] != id) return false;
        // unsorted pool: the last entry takes the removed one's place
        const uint32_t last = np - 1u;
        float vd = 0.f;
        uint32_t vs = 0, vi = 0, va = 0;
        if (lane == 0) {
            vd = pd[last];
            vs = pseq[last];
            vi = pid[last];
            va = pa[last];
        }
        sync();
        if (lane == 0) {
            pd[pos] = vd;
            pseq[pos] = vs;
            pid[pos] = vi;
            pa[pos] = va;
        }
        sync();
        np = last;
        return true;
    }

    // exact pre-filter: with the global queue full, no case of insert() can fire for d >= max(global worst, every
    // local distance)
    __device__ bool can_skip(float d) const {
        if (gsize < L) return false;
        const float w = gd[L - 1];
        const float t = w > lmax ? w : lmax;
        return !(d < t);
    }

    // DiverseNeighborQueue::insert (diverse_priority_queue.rs:151-220)
    __device__ void insert(uint32_t id, float d, uint32_t at) {
        if (d != d || at == kNoAttribute) return;  // NaN: every queue ignores it; None: skipped
        uint32_t cnt, wpos;
        l_scan(at, cnt, wpos);
        const bool lfull = cnt >= dl, gfull = gsize >= L;
        if (!lfull && !gfull) {  // case 1
            l_append(id, d, at);
            if (overflow) return;
            g_insert(id, d, at);
        } else if (lfull) {  // case 2
            const float wd = pd[wpos];
            if (d < wd) {
                const uint32_t wid = pid[wpos];
                sync();
                if (!g_remove(wid, at, wd)) ++failed_remove[0];
                l_replace(wpos, id, d, at);
                g_insert(id, d, at);
            }
        } else {  // case 3
            const float wd = gd[L - 1];
            if (d < wd) {
                const uint32_t wid = gid[L - 1] & ~kVisitedBit, wa = ga[L - 1];
                sync();
                l_append(id, d, at);
                if (overflow) return;
                g_insert(id, d, at);
                if (!l_remove(wa, wid, wd)) ++failed_remove[1];
            }
        }
    }

    // DiverseNeighborQueue::post_process (diverse_priority_queue.rs:112-138): entries past position dk of their local
    // queue leave the global queue (retain, order kept)
    __device__ void post_process() {
        uint32_t w = 0;
        for (uint32_t i0 = 0; i0 < gsize; i0 += 64u) {
            const uint32_t i = i0 + lane;
            bool keep = false;
            float vd = 0.f;
            uint32_t vi = 0, va = 0;
            if (i < gsize) {
                vd = gd[i];
                vi = gid[i];
                va = ga[i];
                const uint32_t id = vi & ~kVisitedBit;
                keep = true;
                for (uint32_t p = 0; p < np; ++p) {
                    if (pid[p] != id) continue;
                    const unsigned long long kp = dv_key(pd[p], pseq[p]);
                    const uint32_t ap = pa[p];
                    uint32_t rank = 0;
                    for (uint32_t q = 0; q < np; ++q) rank += (pa[q] == ap && dv_key(pd[q], pseq[q]) < kp) ? 1u : 0u;
                    keep = rank < dk;
                    break;
                }
            }
            const uint64_t m = ballot64(keep);
            sync();
            if (keep) {
                const uint32_t r = w + mbcnt(m);
                gd[r] = vd;
                gid[r] = vi;
                ga[r] = va;
            }
            sync();
            w += (uint32_t)__popcll(m);
        }
        gsize = w;
        cursor = 0;
    }
};

}  // namespace dann
