"""CPU restatement of what the reference's in-memory builder wraps around a build, over numpy arrays and the oracle's Index:
ComputeMedoid (diskann-utils/src/sampling/medoid.rs:15-156), count_reachable_nodes, get_degree_stats and prune_range
(diskann/src/graph/index.rs:2161-2239, 2656-2701) -- what dann_medoid, dann_count_reachable, dann_degree_stats and
dann_prune_range are compared with bit for bit -- and of the exactness test of diskann_amd/csrc/seq_sum.h, which says
where the medoid's sequential column sums may be taken in parallel."""
import math

import numpy as np

import oracle
from consolidate_model import robust_prune_list

RANGE_ROWS, GROUP_RANGES = 256, 64  # seq_sum.h: kMedoidRangeRows, kMedoidGroupRanges
F32_MAX = np.float32(3.4028234663852886e38)


# ---- ComputeMedoid ----------------------------------------------------------------------------------------------------
def column_sums(rows):
    """the sequential f64 sum of every column in row order from 0.0, each element widened exactly (np.cumsum adds one
    element after the other; np.sum would add pairwise)"""
    rows = np.asarray(rows)
    if rows.shape[0] == 0:
        return np.zeros(rows.shape[1], np.float64)
    with np.errstate(all="ignore"):
        return np.cumsum(rows.astype(np.float64), axis=0)[-1]


def medoid(rows):
    """(row, mean, nan_distances): mean[c] = (f32)(sum_c / (f64)nrows); the first row with d < min starting at f32::MAX
    under SquaredL2::evaluate(mean, row) -- equal distances keep the earlier row, a NaN never wins, -1 = no row won.
    Distances are the oracle's: f32 x f32 for f32 rows and for u8 / i8 rows widened to f32, f32 x f16 for f16 rows
    (the oracle's f32 x f16 kernel is its f32 x f32 kernel over the exactly widened row: one template, two element types)."""
    rows = np.asarray(rows)
    n, dim = rows.shape
    if n == 0:
        return -1, np.zeros(dim, np.float32), 0
    with np.errstate(all="ignore"):
        mean = (column_sums(rows) / np.float64(n)).astype(np.float32)
    wide = np.ascontiguousarray(rows.astype(np.float32))
    best, row, nans = F32_MAX, -1, 0
    for r in range(n):
        d = np.float32(oracle.query_distance(oracle.F32, oracle.L2, mean, wide[r]))
        if d != d:
            nans += 1
        if d < best:
            best, row = d, r
    return row, mean, nans


# ---- seq_sum.h: where a sequential sum cannot round -----------------------------------------------------------------------
SEQ_NONE, SEQ_BAD = 0x7FFFFFFF, -0x80000000


def lsb_exp(v):
    """exponent of the lowest set bit of a finite, non-zero double"""
    m, e = math.frexp(abs(v))
    mant = int(m * (1 << 53))
    return e - 53 + ((mant & -mant).bit_length() - 1)


def seq_summary(values):
    """(S, A, g) of a range: the sum in the given order, the sum of magnitudes, the lowest set bit's exponent"""
    S = A = 0.0
    g = SEQ_NONE
    for v in (float(x) for x in values):
        with np.errstate(all="ignore"):
            S, A = S + v, A + abs(v)
        if not abs(v) < math.inf:
            g = SEQ_BAD
        elif v != 0.0 and g != SEQ_BAD:
            g = min(g, lsb_exp(v))
    return S, A, g


def seq_join(a, b):
    return a[0] + b[0], a[1] + b[1], SEQ_BAD if SEQ_BAD in (a[2], b[2]) else min(a[2], b[2])


def seq_exact(acc, summary):
    """may the range be added to the running sum `acc` in any association without changing the sequential result?"""
    _, A, g = summary
    if g == SEQ_BAD or not abs(acc) < math.inf:
        return False
    if acc != 0.0:
        g = min(g, lsb_exp(acc))
    if g == SEQ_NONE:
        return True
    bound = (abs(acc) + A) * (1.0 + 2.0 ** -30)
    lim = g + 53
    if lim > 1023:
        return bound < math.inf
    if lim < -1021:
        return False
    return bound < math.ldexp(1.0, lim)


def walk_column(col):
    """the medoid's walk of one column (medoid_walk_kernel): ranges of RANGE_ROWS rows, groups of GROUP_RANGES ranges; a
    group is tested against the carry first, then each range, and a range that fails is walked row by row
    -> (sum, ranges summed in parallel, ranges walked row by row)"""
    col = np.asarray(col, np.float64)
    ranges = [col[i:i + RANGE_ROWS] for i in range(0, len(col), RANGE_ROWS)]
    sums = [seq_summary(r) for r in ranges]
    acc, par, ser = 0.0, 0, 0
    for k0 in range(0, len(ranges), GROUP_RANGES):
        group = sums[k0:k0 + GROUP_RANGES]
        joined = group[0]
        for s in group[1:]:
            joined = seq_join(joined, s)
        if seq_exact(acc, joined):
            acc, par = acc + joined[0], par + len(group)
            continue
        for j, s in enumerate(group):
            if seq_exact(acc, s):
                acc, par = acc + s[0], par + 1
                continue
            ser += 1
            for v in ranges[k0 + j]:
                acc = acc + float(v)
    return acc, par, ser


def walk_counters(rows):
    """(ranges summed in parallel, ranges walked row by row) over every column: dann_medoid's counters [0] and [1]"""
    rows = np.asarray(rows)
    par = ser = 0
    for c in range(rows.shape[1]):
        _, p, s = walk_column(rows[:, c].astype(np.float64))
        par, ser = par + p, ser + s
    return par, ser


# ---- count_reachable_nodes / get_degree_stats / prune_range --------------------------------------------------------------
def count_reachable(oix, starts=None):
    """(count, levels, reached): the nodes a breadth-first walk expands from `starts` (None: the index's start points),
    the greatest depth reached (start points: 0) and a boolean per slot.  Pure graph."""
    nslots = oix.adj.shape[0]
    if starts is None:
        starts = range(oix.capacity, nslots)
    reached = np.zeros(nslots, bool)
    frontier = []
    for s in starts:
        if not reached[s]:
            reached[s] = True
            frontier.append(int(s))
    levels = 0
    while frontier:
        nxt = []
        for v in frontier:
            for i in oix.neighbors(v):
                if not reached[i]:
                    reached[i] = True
                    nxt.append(int(i))
        if nxt:
            levels += 1
        frontier = nxt
    return int(reached.sum()), levels, reached


def degree_stats(oix, ids=None, deleted=None):
    """(max_degree, avg_degree, min_degree, cnt_less_than_two, points, total) over the ids (None: the slots [0, capacity));
    a repeated id counts each time; `deleted` (a boolean per slot) leaves its slots out"""
    if ids is None:
        ids = range(oix.capacity)
    lens = [len(oix.neighbors(int(v))) for v in ids if deleted is None or not deleted[int(v)]]
    if not lens:
        return 0, np.float32(0.0), 0, 0, 0, 0
    total = sum(lens)
    return (max(lens), np.float32(total) / np.float32(len(lens)), min(lens), sum(1 for x in lens if x < 2), len(lens), total)


def readable(oix, slot):
    return not oix.tag_offset or oix.rows[slot, oix.tag_offset] >= 254


def prune_range(oix, cfg, ids):
    """prune_range over the ids in order: a list longer than cfg.pruned_degree is replaced by robust_prune_list of it
    (unreadable neighbours of an inline-tags index stay out of the pool); an id whose own slot is unreadable is left
    alone and counted once -> (lists pruned, ids left alone)"""
    pruned, skipped = 0, set()
    for v in (int(i) for i in ids):
        nb = oix.neighbors(v)
        if len(nb) <= cfg.pruned_degree:
            continue
        if not readable(oix, v):
            skipped.add(v)
            continue
        oix.set_neighbors(v, robust_prune_list(oix, cfg, v, [i for i in nb if readable(oix, int(i))]))
        pruned += 1
    return pruned, len(skipped)
