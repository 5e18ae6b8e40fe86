"""MinMax search at 1 M points next to the scalar quantiser and full precision (not part of bench.py): build one
1 M x 128 graph on f32 rows, then search the same graph on MM8 and MM4 copies of the data (dann_minmax_compress, grid
scale 1, no transform; queries are row images of the rows' own width; 8-bit queries against narrower rows: scratch/minmax_q8_bench.py),
on an SQ-8 copy and on the f32 rows themselves (the yardsticks: existing code), in the same run: wall-clock QPS of one
host-pointer call, the HIP-event kernel time (dann_kernel_time), the algorithmic bytes of a launch (rows + adjacency
lists read) and recall@10 against f32 brute force, at L in {26, 64}.  Prints one line per configuration and one JSON line.
usage: python scratch/minmax_bench.py [--n 1000000] [--nq 100000] [--steps 5] [--out profiles/minmax_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import diskann_amd as da  # noqa: E402
from benchdata import ground_truth, make_data, recall_at_k  # noqa: E402


def timed(prov, fn, steps):
    fn()  # warm-up (visited-table calibration, LDS limit, staging buffers)
    walls, kernels = [], []
    for _ in range(steps):
        prov.kernel_time_reset()
        t0 = time.perf_counter()
        out = fn()
        walls.append(time.perf_counter() - t0)
        kernels.append(prov.kernel_time(0)[0])
    return walls, kernels, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    dim, R, pruned = 128, 32, 28
    cfg = da.build_config(pruned, R, 100, intra_batch_candidates=da.IBC_NONE)  # as bench.py builds
    base, q = make_data(torch, dev, a.n, dim, a.nq, "sift_like", 1, 2)[:2]
    mean = base.double().mean(0).float()
    medoid = int(torch.argmin(((base - mean[None, :]) ** 2).sum(1)).item())
    hb = base.cpu().numpy().astype(np.float32)
    hq = q.cpu().numpy().astype(np.float32)
    f32p = da.Provider(da.F32, da.L2, dim, a.n, R, hb[medoid:medoid + 1])
    f32p.set_elements(0, hb)
    t0 = time.perf_counter()
    f32p.build(cfg, 0, a.n, 0.05, 16384)
    print(f"build {time.perf_counter() - t0:.2f} s", flush=True)
    adj = f32p.download_graph()
    nq_gt = min(a.nq, 2000)
    gt = np.asarray(ground_truth(torch, base, q[:nq_gt], 10))
    shift, scale, _ = da.sq8_train(hb, 2.0)
    snorm = float(np.float32((shift ** 2).sum(dtype=np.float32)))
    results = []
    configs = [("mm8", da.MM8, da.minmax_compress(hb, 8), da.minmax_compress(hq, 8)),
               ("mm4", da.MM4, da.minmax_compress(hb, 4), da.minmax_compress(hq, 4)),
               ("sq8", da.SQ8, da.sq_compress(hb, shift, scale, 8), da.sq_compress(hq, shift, scale, 8)),
               ("f32", da.F32, hb, hq)]
    for name, dtype, rows, qc in configs:
        lb = rows.shape[1] * rows.dtype.itemsize
        sq = dict(sq_scale=float(scale), sq_shift_norm_sq=snorm) if dtype == da.SQ8 else {}
        p = da.Provider(dtype, da.L2, dim, a.n, R, rows[medoid:medoid + 1], **sq)
        p.set_elements(0, rows)
        p.upload_graph(adj)
        for L in (26, 64):
            walls, kernels, (ids, _, st) = timed(p, lambda: p.search(da.Knn(L, 1), qc, 10), a.steps)
            algo = float(st["cmps"].astype(np.float64).sum() * lb + st["hops"].astype(np.float64).sum() * (R + 1) * 4)
            r = dict(rows=name, row_bytes=lb, query_bytes=p.query_bytes(), L=L, nq=a.nq,
                     qps_wall_best=a.nq / min(walls), qps_wall_median=a.nq / float(np.median(walls)),
                     kernel_ms_min=min(kernels), kernel_ms_median=float(np.median(kernels)),
                     kernel_ms_max=max(kernels), algorithmic_bytes=algo,
                     mean_cmps=float(st["cmps"].mean()), mean_hops=float(st["hops"].mean()),
                     recall_at_10=float(recall_at_k(ids[:nq_gt], gt, 10)))
            results.append(r)
            print(f"{name} L={L}: {r['qps_wall_median']:,.0f} QPS wall, kernel {r['kernel_ms_median']:.2f} ms (min "
                  f"{r['kernel_ms_min']:.2f} max {r['kernel_ms_max']:.2f}; {a.nq / (r['kernel_ms_median'] / 1e3):,.0f} QPS "
                  f"kernel), {algo / 1e6:,.0f} MB algorithmic ({algo / (r['kernel_ms_median'] / 1e3) / 1e12:.2f} TB/s), cmps "
                  f"{r['mean_cmps']:.0f} hops {r['mean_hops']:.1f}, recall@10 {r['recall_at_10']:.4f}", flush=True)
        p.close()
    line = json.dumps(dict(bench="minmax", n=a.n, dim=dim, R=R, steps=a.steps, results=results))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
