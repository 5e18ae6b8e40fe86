"""numpy restatement of how the kernels score an MM8 query image against MinMax rows of 4, 2 or 1 bit (dann_device.h:
mmq_stage_query, mmq_dot, group_ip_mmq).  The query's codes, one byte per element, are staged once per query in the
order a row dword is taken apart in:
    4 bit  per 8 elements: the four even query bytes, then the four odd ones
    2 bit  per 16 elements: dword s = query bytes s, s + 4, s + 8, s + 12
    1 bit  per 32 elements: eight plane dwords, plane j = bit j of the 32 query bytes
Elements at or beyond dim are staged as zero.  numpy only."""
import numpy as np


def staged_bytes(bits, dim):
    return (dim + 31) // 32 * 32 if bits == 1 else (dim + 15) // 16 * 16


def _source_index(bits, nbytes):
    """element whose query byte is staged byte s (4 and 2 bit)"""
    s = np.arange(nbytes)
    w, b = s // 4, s % 4
    if bits == 4:
        return (w // 2) * 8 + 2 * b + (w & 1)
    return (w // 4) * 16 + (w & 3) + 4 * b


def stage(qcodes, bits):
    """(nq, dim) u8 query codes -> (nq, staged_bytes) u8"""
    qcodes = np.ascontiguousarray(qcodes, dtype=np.uint8)
    nq, dim = qcodes.shape
    nb = staged_bytes(bits, dim)
    padded = np.zeros((nq, nb), np.uint8)
    padded[:, :dim] = qcodes
    if bits != 1:
        return padded[:, _source_index(bits, nb)]
    blocks = padded.reshape(nq, nb // 32, 32).astype(np.uint32)
    planes = np.zeros((nq, nb // 32, 8), np.uint32)
    for j in range(8):
        planes[:, :, j] = (((blocks >> j) & 1) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint32)
    return np.ascontiguousarray(planes.astype("<u4")).view(np.uint8).reshape(nq, nb)


def unstage(staged, bits, dim):
    staged = np.ascontiguousarray(staged, dtype=np.uint8)
    nq, nb = staged.shape
    if bits != 1:
        out = np.zeros((nq, nb), np.uint8)
        out[:, _source_index(bits, nb)] = staged
        return out[:, :dim]
    planes = np.ascontiguousarray(staged).view("<u4").reshape(nq, nb // 32, 8).astype(np.uint32)
    out = np.zeros((nq, nb // 32, 32), np.uint32)
    for j in range(8):
        out |= ((planes[:, :, j, None] >> np.arange(32, dtype=np.uint32)) & 1) << j
    return out.reshape(nq, nb).astype(np.uint8)[:, :dim]


def _dot4(a, b):
    """sum of the products of the four bytes of two dword arrays"""
    return sum(((a >> (8 * i)) & 0xFF).astype(np.int64) * ((b >> (8 * i)) & 0xFF).astype(np.int64) for i in range(4))


def staged_product(staged, code_bytes, bits, dim):
    """(nq, n) integer products, evaluated row dword by row dword as mmq_dot does.  A row's last dword is completed with
    0xFF bytes: what follows the code bytes inside a row's stride is arbitrary and must meet staged zeros."""
    code_bytes = np.ascontiguousarray(code_bytes, dtype=np.uint8)
    n, cb = code_bytes.shape
    assert cb == (dim * bits + 7) // 8
    nd = (cb + 3) // 4
    padded = np.full((n, 4 * nd), 0xFF, np.uint8)
    padded[:, :cb] = code_bytes
    y = np.ascontiguousarray(padded).view("<u4").astype(np.uint64)           # (n, nd)
    q = np.ascontiguousarray(staged).view("<u4").astype(np.uint64)           # (nq, staged dwords)
    qw = 8 // bits                                                           # query dwords per row dword
    assert q.shape[1] >= qw * nd
    out = np.zeros((q.shape[0], n), np.int64)
    for d in range(nd):
        yd = y[None, :, d]
        qd = [q[:, qw * d + j, None] for j in range(qw)]
        if bits == 4:
            out += _dot4(qd[0], yd & 0x0F0F0F0F) + _dot4(qd[1], (yd >> 4) & 0x0F0F0F0F)
        elif bits == 2:
            for s in range(4):
                out += _dot4(qd[s], (yd >> (2 * s)) & 0x03030303)
        else:
            for j in range(8):
                v = qd[j] & yd
                out += np.array([[bin(int(t)).count("1") for t in r] for r in v], np.int64) << j
    return out
