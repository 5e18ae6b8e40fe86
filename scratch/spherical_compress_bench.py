"""The spherical compressor on the GPU (not part of bench.py): rows per second of dann_spherical_compress_device for
n x 128 f32 rows resident in HBM at 1, 2 and 4 bits (PaddingHadamard 128 -> 128, squared L2), the time of
dann_spherical_compress_queries_device for nq queries, and the search launch those queries feed (SPH1 rows made by the
compressor under a graph built on the f32 rows; FOUR_BIT_TRANSPOSED queries, L = 26 and 64).  Every timed call is
complete on return, so the host clock around it is the call's time; one warm-up call, then the median of --steps calls.
Prints one line per figure and one JSON line.
usage: python scratch/spherical_compress_bench.py [--n 1000000] [--nq 16384] [--steps 5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import diskann_amd as da  # noqa: E402
from benchdata import make_data  # noqa: E402


def timed(fn, steps):
    fn()
    t = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    dim, R, pruned, k = 128, 32, 28, 10
    base, q = make_data(torch, dev, a.n, dim, a.nq, "sift_like", 1, 2)[:2]
    base, q = base.float().contiguous(), q.float().contiguous()
    shift = base.double().mean(0).float().cpu().numpy()
    rng = np.random.default_rng(3)
    signs = (rng.integers(0, 2, dim).astype(np.uint32) << np.uint32(31)).astype(np.uint32)
    comp = da.SphericalCompressor(da.Transform.padding_hadamard(signs, dim), da.L2, shift)
    res = dict(bench="spherical_compress", n=a.n, nq=a.nq, dim=dim, steps=a.steps)
    images = {}
    for bits in (1, 2, 4):
        out = torch.empty(a.n * comp.row_bytes(bits), dtype=torch.uint8, device=dev)
        med, lo, hi = timed(lambda: comp.compress_device(base.data_ptr(), a.n, bits, out.data_ptr()), a.steps)
        images[bits] = out
        res[f"rows_{bits}bit_ms"] = dict(median=med * 1e3, min=lo * 1e3, max=hi * 1e3)
        res[f"rows_{bits}bit_per_s"] = a.n / med
        print(f"rows {bits} bit: {med * 1e3:.2f} ms median (min {lo * 1e3:.2f} max {hi * 1e3:.2f}) = {a.n / med:,.0f} rows/s",
              flush=True)
    qimg = {}
    for bits, layout in ((1, da.QUERY_FOUR_BIT_TRANSPOSED), (1, da.QUERY_SAME_AS_DATA), (4, da.QUERY_SCALAR_QUANTIZED)):
        out = torch.empty(a.nq * comp.query_bytes(bits, layout), dtype=torch.uint8, device=dev)
        med, lo, hi = timed(lambda: comp.queries_device(q.data_ptr(), a.nq, bits, layout, out.data_ptr()), a.steps)
        qimg[(bits, layout)] = out
        res[f"queries_{bits}bit_layout{layout}_ms"] = dict(median=med * 1e3, min=lo * 1e3, max=hi * 1e3)
        print(f"queries {bits} bit layout {layout}: {med * 1e3:.3f} ms median (min {lo * 1e3:.3f} max {hi * 1e3:.3f})", flush=True)
    # the search those queries feed: a graph built on the f32 rows, SPH1 rows from the compressor, all device to device
    hb = base.cpu().numpy()
    medoid = int(torch.argmin(((base - base.mean(0)[None, :]) ** 2).sum(1)).item())
    f32p = da.Provider(da.F32, da.L2, dim, a.n, R, hb[medoid:medoid + 1])
    f32p.set_elements(0, hb)
    f32p.build(da.build_config(pruned, R, 100, intra_batch_candidates=da.IBC_NONE), 0, a.n, 0.05, 16384)
    adj = f32p.download_graph()
    f32p.close()
    p = da.Provider(da.SPH1, da.L2, dim, a.n, R, comp.compress(hb[medoid:medoid + 1], 1),
                    query_layout=da.QUERY_FOUR_BIT_TRANSPOSED)
    p.set_elements_device(0, images[1].data_ptr(), a.n)
    p.upload_graph(adj)
    ids = torch.empty(a.nq * k, dtype=torch.int32, device=dev)
    dists = torch.empty(a.nq * k, dtype=torch.float32, device=dev)
    stats = torch.empty(a.nq * 20, dtype=torch.uint8, device=dev)
    qp = qimg[(1, da.QUERY_FOUR_BIT_TRANSPOSED)]
    for L in (26, 64):
        def search():
            da._ffi.check(da.lib().dann_search_batch_device(p._h, C.c_void_p(qp.data_ptr()), a.nq, L, 1, k,
                                                            C.c_void_p(ids.data_ptr()), C.c_void_p(dists.data_ptr()),
                                                            C.c_void_p(stats.data_ptr())), "dann_search_batch_device")
        med, lo, hi = timed(search, a.steps)
        res[f"search_L{L}_ms"] = dict(median=med * 1e3, min=lo * 1e3, max=hi * 1e3)
        print(f"search L={L}: {med * 1e3:.3f} ms median (min {lo * 1e3:.3f} max {hi * 1e3:.3f}) for {a.nq} queries", flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
