"""Graph consolidation at 1 M points (not part of bench.py): build an index with dann_build, delete 1 % / 10 % at random,
time dann_consolidate, print its counters, the adjacency-scan rate and recall@10 of the consolidated graph against the
pre-delete graph (both on the surviving points), and the CPU restatement's time on a 10 k-vertex sample, extrapolated.
usage: python scratch/consolidate_bench.py [--n 1000000] [--specs 128:f32,768:f16] [--L 40] [--no-cpu]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import diskann_amd as da  # noqa: E402
import oracle  # noqa: E402
from benchdata import ground_truth, make_data, recall_at_k  # noqa: E402
from consolidate_model import consolidate_vector  # noqa: E402


def recall(prov, q, gt, L, dead):
    ids, _, _ = prov.search(da.Knn(L, 1), q, 10)
    ids = np.where(dead[np.minimum(ids, dead.size - 1)], 0xFFFFFFFF, ids)  # a deleted point returned is a miss
    return recall_at_k(ids, gt, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--specs", default="128:f32,768:f16")
    ap.add_argument("--L", type=int, default=40)
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    R, pruned = 32, 28
    cfg = da.build_config(pruned, R, 100, intra_batch_candidates=da.IBC_NONE)  # as bench.py builds
    for spec in a.specs.split(","):
        dim, ty = int(spec.split(":")[0]), spec.split(":")[1]
        dtype = {"f32": da.F32, "f16": da.F16}[ty]
        base, q = make_data(torch, dev, a.n, dim, a.nq, "sift_like", 1, 2)[:2]
        mean = base.double().mean(0).float()
        medoid = int(torch.argmin(((base - mean[None, :]) ** 2).sum(1)).item())
        hb = base.cpu().numpy().astype(da.NP_DTYPE[dtype])
        hq = q.cpu().numpy().astype(da.NP_DTYPE[dtype])
        start = hb[medoid:medoid + 1]
        prov = da.Provider(dtype, da.L2, dim, a.n, R, start)
        prov.set_elements(0, hb)
        t0 = time.perf_counter()
        prov.build(cfg, 0, a.n, 0.05, 16384)
        print(f"[{dim} {ty}] build {time.perf_counter() - t0:.2f} s", flush=True)
        graph = prov.download_graph()
        prov.close()
        bq = torch.from_numpy(hb.astype(np.float32)).to(dev)
        for frac in (0.01, 0.1):
            rng = np.random.default_rng(int(frac * 1000))
            dels = np.sort(rng.choice(a.n, int(frac * a.n), replace=False)).astype(np.uint32)
            dead = np.zeros(a.n + 1, bool)
            dead[dels] = True
            live = np.flatnonzero(~dead[:a.n])
            gt_live = ground_truth(torch, bq[torch.from_numpy(live).to(dev)], torch.from_numpy(hq.astype(np.float32)).to(dev), 10)
            gt = live[np.asarray(gt_live)]
            p = da.Provider(dtype, da.L2, dim, a.n, R, start)
            p.set_elements(0, hb)
            p.upload_graph(graph)
            r0 = recall(p, hq, gt, a.L, dead)
            p.delete_points(dels)
            t0 = time.perf_counter()
            kinds, c = p.consolidate(cfg, drop_deleted=True)
            ms = (time.perf_counter() - t0) * 1e3
            r1 = recall(p, hq, gt, a.L, dead)
            scan_gb = (a.n + 1) * (R + 1) * 4 / 1e9
            print(f"[{dim} {ty}] delete {frac:.0%}: dann_consolidate {ms:.1f} ms (wall, one synchronous call); counters "
                  f"scanned {c[0]} rewritten {c[1]} pruned {c[2]} largest pool {c[3]} distances {c[4]} mfma pools "
                  f"{c[5]}; adjacency scan {scan_gb / (ms / 1e3):.1f} GB/s (lower bound: one read of the graph); "
                  f"recall@10 L={a.L} on survivors: before {r0:.4f} after {r1:.4f} (diff {r1 - r0:+.4f})", flush=True)
            assert (kinds[dels] == da.CONSOLIDATE_DELETED).all()
            assert r1 >= r0 - 0.01, f"recall on the survivors fell by more than 0.01: {r0:.4f} -> {r1:.4f}"
            p.close()
            if not a.no_cpu:
                oix = oracle.Index(oracle.F16 if dtype == da.F16 else oracle.F32, oracle.L2, dim, a.n, R, start)
                oix.set_rows(0, hb)
                oix.adj[:] = graph
                sample = rng.choice(a.n, 10_000, replace=False)
                ocfg = oracle.build_config(pruned, R, 100, intra_batch_candidates=oracle.IBC_NONE)
                t0 = time.perf_counter()
                for v in sample:
                    consolidate_vector(oix, ocfg, dead, int(v))
                s = time.perf_counter() - t0
                print(f"[{dim} {ty}] delete {frac:.0%}: CPU restatement {s:.2f} s for 10 k vertices, "
                      f"{s * (a.n + 1) / 10_000:.0f} s extrapolated to the index", flush=True)
                del oix


if __name__ == "__main__":
    main()
