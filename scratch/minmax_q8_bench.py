"""MM4 / MM2 / MM1 rows searched with queries of their own width and with 8-bit (MM8) queries (dann_set_query_dtype), in
the same process (a sibling of scratch/minmax_bench.py, not part of bench.py): one 1 M x 128 graph built on f32 rows,
searched on MM4, MM2 and MM1 copies of the data at L in {26, 64}.  The two query forms alternate call by call on the same
index (same-width, 8-bit, same-width, ...), `--steps` timed calls each after one warm-up call each; reported per form:
recall@10 against f32 brute force, the median wall-clock QPS and the median HIP-event kernel time with its range.  No
threshold is attached.  Prints one line per configuration and one JSON line.
usage: python scratch/minmax_q8_bench.py [--n 1000000] [--nq 100000] [--steps 5] [--out profiles/minmax_q8_bench.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.steps >= 5, "median of at least 5 runs"
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
    f32p.close()
    nq_gt = min(a.nq, 2000)
    gt = np.asarray(ground_truth(torch, base, q[:nq_gt], 10))
    q8 = da.minmax_compress(hq, 8)
    results = []
    for bits, dtype in ((4, da.MM4), (2, da.MM2), (1, da.MM1)):
        rows = da.minmax_compress(hb, bits)
        forms = {"same": (dtype, da.minmax_compress(hq, bits)), "mm8": (da.MM8, q8)}
        p = da.Provider(dtype, da.L2, dim, a.n, R, rows[medoid:medoid + 1])
        p.set_elements(0, rows)
        p.upload_graph(adj)
        for L in (26, 64):
            walls = {f: [] for f in forms}
            kernels = {f: [] for f in forms}
            last = {}
            for step in range(a.steps + 1):  # step 0: the warm-up of both forms
                for f, (qdt, qc) in forms.items():
                    p.set_query_dtype(qdt)
                    p.kernel_time_reset()
                    t0 = time.perf_counter()
                    last[f] = p.search(da.Knn(L, 1), qc, 10)
                    wall = time.perf_counter() - t0
                    if step:
                        walls[f].append(wall)
                        kernels[f].append(p.kernel_time(0)[0])
            for f in forms:
                ids, _, st = last[f]
                r = dict(rows=f"mm{bits}", queries=f, query_bytes=int(forms[f][1].shape[1]), L=L, nq=a.nq,
                         qps_wall_median=a.nq / float(np.median(walls[f])), kernel_ms_median=float(np.median(kernels[f])),
                         kernel_ms_min=min(kernels[f]), kernel_ms_max=max(kernels[f]), mean_cmps=float(st["cmps"].mean()),
                         mean_hops=float(st["hops"].mean()), recall_at_10=float(recall_at_k(ids[:nq_gt], gt, 10)))
                results.append(r)
                print(f"mm{bits} rows, {f} queries, L={L}: recall@10 {r['recall_at_10']:.4f}, {r['qps_wall_median']:,.0f} QPS wall, "
                      f"kernel {r['kernel_ms_median']:.2f} ms (min {r['kernel_ms_min']:.2f} max {r['kernel_ms_max']:.2f}), cmps "
                      f"{r['mean_cmps']:.0f} hops {r['mean_hops']:.1f}", flush=True)
        p.close()
    line = json.dumps(dict(bench="minmax_q8", n=a.n, dim=dim, R=R, steps=a.steps, results=results))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
