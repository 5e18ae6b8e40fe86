"""In-place deletes at 1 M points (not part of bench.py): build a 1 M x 128 f32 index (R 32) with dann_build, delete 1 % /
10 % at random in minibatches of 1 000 with dann_inplace_delete (VisitedAndTopK {k 10, l 64}, TwoHopAndOneHop, OneHop;
num_to_replace 3), and
print deletes per second, the summed counters, recall@10 at L = 64 on the surviving points before the deletes, after the
in-place deletes and after dann_consolidate of the same deleted set (on the pre-delete graph), and the CPU restatement's
deletes per second on a sample.
usage: python scratch/inplace_delete_bench.py [--n 1000000] [--L 64] [--minibatch 1000] [--no-cpu]"""
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
from inplace_delete_model import ONE_HOP, TWO_HOP_AND_ONE_HOP, VISITED_AND_TOPK, inplace_delete  # noqa: E402

METHODS = (("VisitedAndTopK{10,64}", VISITED_AND_TOPK, 10, 64), ("TwoHopAndOneHop", TWO_HOP_AND_ONE_HOP, 0, 0),
           ("OneHop", ONE_HOP, 0, 0))


def recall(prov, q, gt, L, dead):
    ids, _, _ = prov.search(da.Knn(L, 1), q, 10)
    ids = np.where(dead[np.minimum(ids, dead.size - 1)], 0xFFFFFFFF, ids)  # a deleted point returned is a miss
    return recall_at_k(ids, gt, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--minibatch", type=int, default=1000)
    ap.add_argument("--cpu-sample", type=int, default=50)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    R, pruned = 32, 28
    cfg = da.build_config(pruned, R, 100, intra_batch_candidates=da.IBC_NONE)  # as bench.py builds
    base, q = make_data(torch, dev, a.n, a.dim, a.nq, "sift_like", 1, 2)[:2]
    mean = base.double().mean(0).float()
    medoid = int(torch.argmin(((base - mean[None, :]) ** 2).sum(1)).item())
    hb = base.cpu().numpy().astype(np.float32)
    hq = q.cpu().numpy().astype(np.float32)
    start = hb[medoid:medoid + 1]
    prov = da.Provider(da.F32, da.L2, a.dim, a.n, R, start)
    prov.set_elements(0, hb)
    t0 = time.perf_counter()
    prov.build(cfg, 0, a.n, 0.05, 16384)
    print(f"build {time.perf_counter() - t0:.2f} s", flush=True)
    graph = prov.download_graph()
    prov.close()
    bq = torch.from_numpy(hb).to(dev)
    for frac in (0.01, 0.1):
        rng = np.random.default_rng(int(frac * 1000))
        dels = rng.choice(a.n, int(frac * a.n), replace=False).astype(np.uint32)
        dead = np.zeros(a.n + 1, bool)
        dead[dels] = True
        live = np.flatnonzero(~dead[:a.n])
        gt_live = ground_truth(torch, bq[torch.from_numpy(live).to(dev)], torch.from_numpy(hq).to(dev), 10)
        gt = live[np.asarray(gt_live)]
        p = da.Provider(da.F32, da.L2, a.dim, a.n, R, start)
        p.set_elements(0, hb)
        p.upload_graph(graph)
        r0 = recall(p, hq, gt, a.L, dead)
        p.delete_points(dels)
        t0 = time.perf_counter()
        p.consolidate(cfg, drop_deleted=True)
        ms_c = (time.perf_counter() - t0) * 1e3
        rc = recall(p, hq, gt, a.L, dead)
        p.close()
        for name, method, k, l in METHODS:
            p = da.Provider(da.F32, da.L2, a.dim, a.n, R, start)
            p.set_elements(0, hb)
            p.upload_graph(graph)
            t0 = time.perf_counter()
            c = p.inplace_delete(cfg, dels, method=method, k=k, l=l, num_to_replace=3, minibatch=a.minibatch)
            s = time.perf_counter() - t0
            r1 = recall(p, hq, gt, a.L, dead)
            p.close()
            print(f"delete {frac:.0%} ({dels.size} ids) {name}, minibatches of {a.minibatch}: {s * 1e3:.1f} ms wall, "
                  f"{dels.size / s:,.0f} deletes/s; counters ids {c[0]} in-neighbours {c[1]} candidates {c[2]} "
                  f"distances {c[3]} sources {c[4]} appended {c[5]} set {c[6]} pruned {c[7]} mfma {c[8]}; "
                  f"recall@10 L={a.L} on survivors: before {r0:.4f} in-place {r1:.4f} consolidated {rc:.4f} "
                  f"(dann_consolidate {ms_c:.1f} ms)", flush=True)
        if not a.no_cpu:
            oix = oracle.Index(oracle.F32, oracle.L2, a.dim, a.n, R, start)
            oix.set_rows(0, hb)
            oix.adj[:] = graph
            ocfg = oracle.build_config(pruned, R, 100, intra_batch_candidates=oracle.IBC_NONE)
            odead = np.zeros(a.n + 1, bool)
            for j, (name, method, k, l) in enumerate(METHODS):
                sample = dels[j * a.cpu_sample:(j + 1) * a.cpu_sample]
                t0 = time.perf_counter()
                inplace_delete(oix, ocfg, odead, sample, method, 3, k_value=k, l_value=l)
                s = time.perf_counter() - t0
                print(f"delete {frac:.0%} {name}: CPU restatement (one host thread) {sample.size / s:,.1f} deletes/s on "
                      f"{sample.size} ids", flush=True)
            del oix


if __name__ == "__main__":
    main()
