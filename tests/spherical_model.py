"""CPU model of the spherically quantised rows (RaBitQ; spherical::Data<NBITS>, diskann-quantization/src/spherical): the
byte images of rows and queries, the three distance forms x three metrics with every f32 operation in the reference's
order, a plain compressor, and a Python restatement of the Knn search.  numpy only.

Row: ceil(dim * bits / 8) code bytes (Dense permutation, element i at bits [i * bits, (i + 1) * bits), little-endian
within a byte), then the 6-byte DataMeta (vectors.rs:219-247): f16 inner_product_correction, f16 metric_specific, u16
bit_sum.  Queries (iface::QueryLayout): 0 a row image; 1 four-bit bit-transposed planes (bits/distances.rs:2123-2249)
+ QueryMeta; 2 Dense codes of the rows' width + QueryMeta.  QueryMeta is four f32: inner_product_correction, bit_sum,
offset, metric_specific (vectors.rs:381-399).

flat_rows: rows with inner_product_correction = 1 and metric_specific = sum((code - off)^2).  Their row x row L2 is
exactly sum((x - y)^2): with off = (2^bits - 1) / 2 every intermediate of the epilogue is a multiple of 1/4 far below
2^24, so every f32 operation is exact, and the f16 fields are exact for dim % 4 == 0 (metric_specific is then an
integer) up to f16's integer range of 2048: any dim at 1 bit (dim / 4), dim <= 908 at 2 bits (dim * 2.25), dim <= 36 at
4 bits (dim * 56.25).  An oracle U8 L2 index over the unpacked codes is therefore an exact twin of such an index."""
import math

import numpy as np

f32 = np.float32
L2, IP, COSINE = 2, 1, 0  # == oracle.L2 / INNER_PRODUCT / COSINE, diskann_amd.L2 / ...
SAME_AS_DATA, FOUR_BIT_TRANSPOSED, SCALAR_QUANTIZED, FULL_PRECISION = 0, 1, 2, 3
DATA_META, QUERY_META = 6, 16


def code_bytes(bits, dim):
    return (dim * bits + 7) // 8


def layer_bytes(bits, dim):
    return code_bytes(bits, dim) + DATA_META


def store_stride(bits, dim):
    """the Store's stride (store.rs:198-211): payload + tag byte, rounded up to 32"""
    return (layer_bytes(bits, dim) + 1 + 31) // 32 * 32


def plane_bytes(dim):
    return (dim + 63) // 64 * 32


def query_bytes(bits, dim, layout):
    if layout == SAME_AS_DATA:
        return layer_bytes(bits, dim)
    if layout == FOUR_BIT_TRANSPOSED and bits == 1:
        return plane_bytes(dim) + QUERY_META
    if layout == SCALAR_QUANTIZED and bits in (2, 4):
        return code_bytes(bits, dim) + QUERY_META
    return None


def offset(bits):
    return f32(((1 << bits) - 1) / 2.0)


# ---- pack / unpack ---------------------------------------------------------------------------------------------------------
def pack(codes, bits):
    """(n, dim) codes below 2^bits -> (n, ceil(dim * bits / 8)) bytes, padding bits zero"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if codes.ndim == 1:
        return pack(codes[None, :], bits)[0]
    assert bits in (1, 2, 4) and (codes < (1 << bits)).all()
    b = ((codes[:, :, None] >> np.arange(bits, dtype=np.uint8)) & 1).reshape(codes.shape[0], -1)
    return np.packbits(b, axis=1, bitorder="little")


def unpack(packed, bits, dim):
    """code bytes (a row's trailing bytes are ignored) -> (n, dim) codes, one byte each"""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    if packed.ndim == 1:
        return unpack(packed[None, :], bits, dim)[0]
    b = np.unpackbits(packed[:, :code_bytes(bits, dim)], axis=1, bitorder="little")[:, :dim * bits]
    b = b.reshape(packed.shape[0], dim, bits).astype(np.uint8)
    return (b << np.arange(bits, dtype=np.uint8)).sum(axis=2).astype(np.uint8)


def transpose4(values):
    """(n, dim) four-bit values -> (n, plane_bytes(dim)): per block of 64 elements four u64 words, word j = bit j of the
    64 values (element e of the block at bit e of the word, little-endian)"""
    values = np.ascontiguousarray(values, dtype=np.uint8)
    if values.ndim == 1:
        return transpose4(values[None, :])[0]
    n, dim = values.shape
    nb = (dim + 63) // 64
    v = np.zeros((n, nb * 64), np.uint8)
    v[:, :dim] = values
    v = v.reshape(n, nb, 64)
    planes = np.stack([(v >> j) & 1 for j in range(4)], axis=2)  # (n, block, plane, 64)
    return np.packbits(planes.reshape(n, nb * 4 * 64), axis=1, bitorder="little")


def untranspose4(planes, dim):
    planes = np.ascontiguousarray(planes, dtype=np.uint8)
    if planes.ndim == 1:
        return untranspose4(planes[None, :], dim)[0]
    n = planes.shape[0]
    nb = (dim + 63) // 64
    b = np.unpackbits(planes[:, :nb * 32], axis=1, bitorder="little").reshape(n, nb, 4, 64)
    v = sum((b[:, :, j, :].astype(np.uint8) << j) for j in range(4))
    return v.reshape(n, nb * 64)[:, :dim].astype(np.uint8)


# ---- metadata --------------------------------------------------------------------------------------------------------------
def data_meta_bytes(ipc, ms, bit_sum):
    """(n,) f32, f32, ints -> (n, 6) bytes; the f32 -> f16 rounding is numpy's round-to-nearest-even"""
    n = np.size(ipc)
    out = np.empty((n, 6), np.uint8)
    out[:, 0:2] = np.asarray(ipc, np.float32).astype(np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    out[:, 2:4] = np.asarray(ms, np.float32).astype(np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    out[:, 4:6] = np.asarray(bit_sum).astype(np.uint16).reshape(n).view(np.uint8).reshape(n, 2)
    return out


def data_meta(row, bits, dim):
    """(inner_product_correction, metric_specific, bit_sum) of a row image as f32 (DataMeta::to_full: exact)"""
    cb = code_bytes(bits, dim)
    m = np.ascontiguousarray(row[cb:cb + 6])
    return f32(m[0:2].view(np.float16)[0]), f32(m[2:4].view(np.float16)[0]), f32(int(m[4:6].view(np.uint16)[0]))


def query_meta_bytes(ipc, bit_sum, off, ms):
    n = np.size(ipc)
    out = np.empty((n, 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = ipc, bit_sum, off, ms
    return out.view(np.uint8).reshape(n, 16)


def query_meta(q, nbytes_before):
    m = np.ascontiguousarray(q[nbytes_before:nbytes_before + 16]).view(np.float32)
    return f32(m[0]), f32(m[1]), f32(m[2]), f32(m[3])


# ---- inner products (exact integers) -----------------------------------------------------------------------------------------
def ip_dense(x, y, bits_x, bits_y, dim):
    return int((unpack(x, bits_x, dim).astype(np.int64) * unpack(y, bits_y, dim).astype(np.int64)).sum())


def ip_transposed(planes, y, dim):
    """sum_j 2^j popcount(data & plane_j), data bits at or beyond dim masked"""
    yb = np.zeros(plane_bytes(dim) // 4 * 8, np.uint8)
    yb[:dim] = unpack(y, 1, dim)
    pb = np.unpackbits(np.ascontiguousarray(planes[:plane_bytes(dim)], dtype=np.uint8), bitorder="little").reshape(-1, 4, 64)
    yb = yb.reshape(-1, 64)
    return int(sum((1 << j) * int((pb[:, j, :] & yb).sum()) for j in range(4)))


# ---- the distance forms (vectors.rs:494-528, :584-636, :744-801, :867-892) ---------------------------------------------------
def _data_meta_all(rows, bits, dim):
    cb = code_bytes(bits, dim)
    m = np.ascontiguousarray(rows[:, cb:cb + 6])
    return (m[:, 0:2].copy().view(np.float16)[:, 0].astype(np.float32), m[:, 2:4].copy().view(np.float16)[:, 0].astype(np.float32),
            m[:, 4:6].copy().view(np.uint16)[:, 0].astype(np.float32))


def distance_matrix(metric, queries, rows, dim, bits, layout=SAME_AS_DATA, ssn=0.0):
    """(nq, n) f32: every query (byte images under `layout`) against every row; numpy evaluates each f32 operation on
    its own (no fused multiply-add), in the reference's association"""
    queries = np.ascontiguousarray(queries, dtype=np.uint8).reshape(-1, np.shape(queries)[-1])
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, np.shape(rows)[-1])
    Y = unpack(rows, bits, dim).astype(np.int64)
    if layout == FOUR_BIT_TRANSPOSED:
        assert bits == 1
        X, before = untranspose4(queries, dim), plane_bytes(dim)  # (== ip_transposed, test_spherical_model_host.py)
    else:
        X, before = unpack(queries, bits, dim), code_bytes(bits, dim)
    ip = (X.astype(np.int64) @ Y.T).astype(np.float32)
    off, D, two, ssn = offset(bits), f32(dim), f32(2.0), f32(ssn)
    cy, my, sy = (a[None, :] for a in _data_meta_all(rows, bits, dim))
    with np.errstate(all="ignore"):
        if layout == SAME_AS_DATA:
            cx, mx, sx = (a[:, None] for a in _data_meta_all(queries, bits, dim))
            k = (cx * cy) * ((ip - off * (sx + sy)) + (off * off) * D)
            if metric == L2:
                return ((mx + my) - two * k).astype(np.float32)
            r = ((mx + my) + k) + ssn
        else:
            assert layout == (FOUR_BIT_TRANSPOSED if bits == 1 else SCALAR_QUANTIZED)
            qm = np.ascontiguousarray(queries[:, before:before + 16]).view(np.float32)
            cq, qsum, qoff, mq = (qm[:, i:i + 1] for i in range(4))
            c = (cy * cq) * (((ip - off * qsum) + qoff * sy) - (off * qoff) * D)
            if metric == L2:
                return ((my + mq) - two * c).astype(np.float32)
            r = ((c + my) + mq) + ssn
        assert r.dtype == np.float32
        return (-r if metric == IP else f32(1.0) - r).astype(np.float32)


def distance_rows(metric, x, y, dim, bits, ssn=0.0):
    """row x row"""
    return distance_matrix(metric, x[None, :], y[None, :], dim, bits, SAME_AS_DATA, ssn)[0, 0]


def distance_query(metric, q, y, dim, bits, layout, ssn=0.0):
    """query under `layout` x row"""
    return distance_matrix(metric, q[None, :], y[None, :], dim, bits, layout, ssn)[0, 0]


# ---- a plain compressor ---------------------------------------------------------------------------------------------------
class Quantizer:
    """centre, normalise, round onto the grid {0 .. 2^bits - 1} (1 bit: the sign).  Not the reference's compressor
    (no transform, no cosine maximisation): the contract under test is bytes -> distance bits."""

    def __init__(self, data, bits, metric):
        self.bits, self.metric = bits, metric
        self.centre = np.asarray(data, np.float32).mean(0).astype(np.float32)
        self.dim = self.centre.size
        self.ssn = float(f32((self.centre.astype(np.float64) ** 2).sum())) if metric != L2 else 0.0

    def _codes(self, x, bits):
        v = np.asarray(x, np.float64) - self.centre
        norm = np.sqrt((v * v).sum(1))
        u = v / np.where(norm > 0, norm, 1.0)[:, None]
        off = ((1 << bits) - 1) / 2.0
        scale = off / max(3.0 / math.sqrt(self.dim), 1e-9)
        codes = np.clip(np.rint(u * scale + off), 0, (1 << bits) - 1).astype(np.uint8)
        if bits == 1:
            codes = (u > 0).astype(np.uint8)
        r = codes.astype(np.float64) - off
        rn = np.sqrt((r * r).sum(1))
        self_ip = (r * u).sum(1) / np.where(rn > 0, rn, 1.0)
        ipc = norm / np.where(np.abs(self_ip) * rn > 1e-12, self_ip * rn, 1.0)
        ms = norm * norm if self.metric == L2 else (v * self.centre).sum(1)
        return codes, ipc, ms

    def rows(self, x):
        codes, ipc, ms = self._codes(x, self.bits)
        n = codes.shape[0]
        out = np.zeros((n, layer_bytes(self.bits, self.dim)), np.uint8)
        cb = code_bytes(self.bits, self.dim)
        out[:, :cb] = pack(codes, self.bits)
        out[:, cb:] = data_meta_bytes(ipc.astype(np.float32), ms.astype(np.float32), codes.sum(1))
        return out

    def queries(self, x, layout):
        if layout == SAME_AS_DATA:
            return self.rows(x)
        qbits = 4 if layout == FOUR_BIT_TRANSPOSED else self.bits
        codes, ipc, ms = self._codes(x, qbits)
        qoff = ((1 << qbits) - 1) / 2.0
        body = transpose4(codes) if layout == FOUR_BIT_TRANSPOSED else pack(codes, qbits)
        # the query stands for (code + offset) on its own grid: offset = -qoff; the grid's step is part of the correction
        meta = query_meta_bytes(ipc.astype(np.float32), codes.sum(1).astype(np.float32),
                                np.full(codes.shape[0], -qoff, np.float32), ms.astype(np.float32))
        return np.concatenate([body, meta], axis=1)


def flat_rows(codes, bits):
    """rows with inner_product_correction = 1, metric_specific = sum((code - off)^2): row x row L2 == sum((x - y)^2)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n, dim = codes.shape
    off = ((1 << bits) - 1) / 2.0
    ms = ((codes.astype(np.float64) - off) ** 2).sum(1)
    assert dim % 4 == 0 and (ms.astype(np.float32).astype(np.float16).astype(np.float64) == ms).all()
    out = np.zeros((n, layer_bytes(bits, dim)), np.uint8)
    cb = code_bytes(bits, dim)
    out[:, :cb] = pack(codes, bits)
    out[:, cb:] = data_meta_bytes(np.ones(n, np.float32), ms.astype(np.float32), codes.sum(1))
    return out


# ---- Knn search (DiskANNIndex::search_internal, index.rs:1933-2000, through the inmem SearchAccessor) ------------------------
def knn_search(dist, adj, capacity, nstart, max_degree, L, W, k, readable=None):
    """dist(id) -> f32 distance of the query to slot `id`.  Start points are the frozen slots [capacity, capacity +
    nstart); the queue holds L + nstart entries and inserts by the rule of tests/test_merge_rule.py::sequential_insert
    (NaN dropped, a full queue drops what is worse than its last entry, a new entry goes before equal old ones); a hop
    pops up to W closest unvisited entries, inserts their unseen, in-bounds, readable neighbours.  Returns (ids[k],
    dists[k], cmps, hops, written); unused output slots hold 0xFFFFFFFF / +inf."""
    cap = L + nstart
    q = []  # [distance, id, visited]
    seen = set()
    cmps = hops = 0

    def insert(d, i):
        if math.isnan(d):
            return
        if len(q) == cap and q[-1][0] < d:
            return
        pos = 0
        while pos < len(q) and q[pos][0] < d:
            pos += 1
        q.insert(pos, [d, i, False])
        del q[cap:]

    nslots = capacity + nstart
    for p in range(capacity, nslots):
        seen.add(p)
        insert(float(dist(p)), p)
        cmps += 1
    while True:
        beam = []
        for e in q:
            if len(beam) == W:
                break
            if not e[2]:
                e[2] = True
                beam.append(e[1])
        if not beam:
            break
        found = []
        for b in beam:
            n = min(int(adj[b, 0]), max_degree)
            for nb in adj[b, 1:1 + n].tolist():
                if nb in seen:
                    continue
                seen.add(nb)
                if nb < nslots and (readable is None or readable[nb]):
                    found.append((float(dist(nb)), nb))
        for d, i in found:
            insert(d, i)
        cmps += len(found)
        hops += len(beam)
    ids = np.full(k, 0xFFFFFFFF, np.uint32)
    dists = np.full(k, np.inf, np.float32)
    written = 0
    for d, i, _ in q:
        if i >= capacity:
            continue
        if written == k:
            break
        ids[written], dists[written] = i, d
        written += 1
    return ids, dists, cmps, hops, written
