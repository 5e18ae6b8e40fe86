"""Rates of the build-finishing calls on one device.
  medoid        dann_medoid_device on device-resident rows: 1 M x 128 f32 (the benchmark's data), 1 M x 128 standard-normal
                f32 (where ranges of the column sums fall back to the row-by-row walk) and 10 M x 128 u8 -- HIP-event
                times of the two passes (dann_debug_medoid_times), their GB/s beside the stream-read probe, the counters,
                and the wall time of the call alternating three times with the torch expression of bench.py
                (f64 mean + argmin) on the same tensor.  On the benchmark's data the call must not be slower than that
                expression; on standard-normal data the row-by-row walk of one unlucky column decides, and is recorded.
  reachability  dann_count_reachable on the benchmark's 1 M graph beside benchdata.reachable_from on the same adjacency:
                count and levels must be equal, the times are recorded.
  prune_range   over the freshly built index: lists pruned, time, dann_degree_stats and recall@10 before and after
                (recorded, not gated).
usage: python scratch/build_finish_rate.py [--n 1000000] [--out profiles/build_finish_rate.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--n-u8", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--skip-graph", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import benchdata
    import diskann_amd as da
    dev = torch.device("cuda:0")
    lib = da.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    gbps = C.c_double()
    da._ffi.check(lib.dann_debug_stream_read_gbps(0, 1 << 30, 10, C.byref(gbps)), "stream_read")
    say(f"# device {torch.cuda.get_device_name(0)}; stream-read probe {gbps.value:.0f} GB/s")

    def torch_medoid(base):
        mean = base.double().mean(0).float()
        return int(torch.argmin(((base - mean[None, :]) ** 2).sum(1)).item())

    def medoid_case(name, base, dtype, against_torch, gate=False):
        n, dim = base.shape
        nbytes = base.numel() * base.element_size()
        row, cnt, ms = C.c_int64(), np.zeros(4, np.uint64), (C.c_double * 2)()
        torch.cuda.synchronize()
        passes = []
        for _ in range(3):
            da._ffi.check(lib.dann_debug_medoid_times(0, dtype, C.c_void_p(base.data_ptr()), n, dim, 0, C.byref(row),
                                                      cnt.ctypes.data_as(C.c_void_p), ms), "medoid_times")
            passes.append((ms[0], ms[1]))
        s_ms, a_ms = min(p[0] for p in passes), min(p[1] for p in passes)
        say(f"medoid {name}: {n} x {dim}, row {row.value}; sum pass {s_ms:.3f} ms = {nbytes / s_ms / 1e6:.0f} GB/s "
            f"({100 * nbytes / s_ms / 1e6 / gbps.value:.0f}% of probe), argmin pass {a_ms:.3f} ms = {nbytes / a_ms / 1e6:.0f} GB/s "
            f"({100 * nbytes / a_ms / 1e6 / gbps.value:.0f}% of probe)")
        ranges = int(cnt[0] + cnt[1])
        say(f"  counters: ranges summed in parallel {int(cnt[0])}, walked row by row {int(cnt[1])} "
            f"({100.0 * int(cnt[1]) / max(ranges, 1):.3f}% of {ranges}), NaN distances {int(cnt[3])}")
        if not against_torch:
            return
        ours, theirs = [], []
        da.medoid(base)
        t_row = torch_medoid(base)
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r, _, _ = da.medoid(base)
            t1 = time.perf_counter()
            tr = torch_medoid(base)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ours.append((t1 - t0) * 1e3)
            theirs.append((t2 - t1) * 1e3)
        say(f"  wall: dann_medoid_device {' '.join(f'{x:.2f}' for x in ours)} ms | torch f64 mean + argmin "
            f"{' '.join(f'{x:.2f}' for x in theirs)} ms (row {t_row}; ours {r})")
        assert not gate or min(ours) <= min(theirs), "dann_medoid_device is slower than the torch expression"

    base, queries = benchdata.make_data(torch, dev, args.n, args.dim, args.nq, "sift_like", 0xD15CA11, 0xD15CA12)
    medoid_case("f32 sift_like", base, da.F32, True, gate=True)
    normal = torch.randn((args.n, args.dim), device=dev, dtype=torch.float32, generator=torch.Generator(device=dev).manual_seed(5))
    medoid_case("f32 standard normal", normal, da.F32, True)
    del normal
    u8 = torch.randint(0, 256, (args.n_u8, args.dim), device=dev, dtype=torch.uint8,
                       generator=torch.Generator(device=dev).manual_seed(6))
    medoid_case("u8", u8, da.U8, False)
    del u8
    if args.skip_graph:
        return finish(args, lines)

    # ---- the benchmark's index: medoid start point, build, then the finishing steps ------------------------------------
    row, _, _ = da.medoid(base)
    prov = da.Provider(da.F32, da.L2, args.dim, args.n, 32, base[row:row + 1].cpu().numpy(), device=0)
    prov.set_elements_device(0, base.data_ptr(), args.n)
    cfg = da.build_config(28, 32, 100, intra_batch_candidates=da.IBC_NONE)
    t0 = time.perf_counter()
    prov.build(cfg, 0, args.n, 0.05, 16384)
    say(f"build: {args.n} x {args.dim}, max_degree 32 over pruned_degree 28, l_build 100: {time.perf_counter() - t0:.1f} s")
    gt = benchdata.ground_truth(torch, base, queries, 10)

    def recall():
        ids, _, _ = prov.search(da.Knn(args.L, 1), queries.cpu().numpy(), 10)
        return benchdata.recall_at_k(ids, gt, 10)

    def stats(tag):
        s = prov.degree_stats()
        say(f"degree_stats {tag}: max {s.max_degree} avg {s.avg_degree:.4f} min {s.min_degree} <2: {s.cnt_less_than_two} "
            f"(points {s.points}, total {s.total})")

    def reach(tag):
        prov.count_reachable()
        t0 = time.perf_counter()
        count, levels = prov.count_reachable()
        t1 = time.perf_counter()
        adj = prov.download_graph()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        seen, lv = benchdata.reachable_from(torch, adj, [args.n], dev)
        tcount = int(seen.sum().item())
        t3 = time.perf_counter()
        say(f"reachable {tag}: dann_count_reachable {count} nodes, {levels} levels, {(t1 - t0) * 1e3:.2f} ms | "
            f"benchdata.reachable_from {tcount} nodes, {lv - 1} levels, {(t3 - t2) * 1e3:.1f} ms ({args.n + 1 - count} unreachable)")
        assert (count, levels) == (tcount, lv - 1)

    stats("before")
    reach("before")
    say(f"recall@10 at L = {args.L} before: {recall():.4f}")
    t0 = time.perf_counter()
    cnt = prov.prune_range(cfg)
    say(f"prune_range: {(time.perf_counter() - t0) * 1e3:.1f} ms; scanned {int(cnt[0])}, lists pruned {int(cnt[1])}, longest "
        f"{int(cnt[2])}, distances {int(cnt[3])}, on the matrix cores {int(cnt[4])}")
    stats("after")
    reach("after")
    say(f"recall@10 at L = {args.L} after: {recall():.4f}")
    finish(args, lines)


def finish(args, lines):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
