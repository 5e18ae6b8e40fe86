"""The quantisers' transforms on the GPU, for the record (not part of bench.py; no threshold is attached):
 1. dann_transform_apply_device on 1 M x 128 (PaddingHadamard 128) and 1 M x 768 (DoubleHadamard 768: t = 512, windows
    [0, 512) and [256, 768)): device-event time around the call and (bytes read + bytes written) / time, next to the
    box's stream-read probe (dann_debug_stream_read_gbps, the one bench.py reports);
 2. dann_minmax_quantize_device (MM4, 1 M x 128 rows that live on the device) against the only route there was before it:
    rows to the host, a host transform (numpy butterflies here), dann_minmax_compress on host pointers -- wall times;
 3. recall@10 of DESIGN 3.15's setup (1 M x 128 sift_like, R = 32, graph built on f32) for MM4 and MM8 rows and queries
    with and without a PaddingHadamard(128) at L = 26 and 64.
usage: python scratch/transform_bench.py [--n 1000000] [--steps 7] [--out profiles/transform_bench.json]"""
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
from benchdata import ground_truth, make_data, recall_at_k  # noqa: E402


def signs(rng, n):
    return (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)).astype(np.uint32)


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def host_hadamard(x, s):
    """sign flip + plain butterflies + scaling on the host (what a caller without the GPU transform would run)"""
    v = (x.view(np.uint32) ^ s[None, :]).view(np.float32).copy()
    n, d = v.shape
    h = 1
    while h < d:
        w = v.reshape(n, d // (2 * h), 2, h)
        a, b = w[:, :, 0, :] + w[:, :, 1, :], w[:, :, 0, :] - w[:, :, 1, :]
        w[:, :, 0, :], w[:, :, 1, :] = a, b
        h *= 2
    return v * np.float32(1.0 / np.sqrt(d))


def apply_leg(name, t, n, steps):
    x = torch.randn((n, t.input_dim), dtype=torch.float32, device="cuda")
    out = torch.empty((n, t.output_dim), dtype=torch.float32, device="cuda")
    ms = []
    for i in range(steps + 2):  # two warm-ups
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t.apply_device(x.data_ptr(), n, out.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    nbytes = n * (t.input_dim + t.output_dim) * 4
    r = dict(leg=name, n=n, input_dim=t.input_dim, output_dim=t.output_dim, bytes=nbytes, event_ms=spread(ms),
             GBps_median=nbytes / (np.median(ms) / 1e3) / 1e9)
    print(f"{name}: {r['event_ms']['median']:.3f} ms (min {r['event_ms']['min']:.3f} max {r['event_ms']['max']:.3f}), "
          f"{r['GBps_median']:,.0f} GB/s read + written", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    res = dict(bench="transform", n=a.n, steps=a.steps)
    rd = C.c_double(0.0)
    if da.lib().dann_debug_stream_read_gbps(0, 4 << 30, 10, C.byref(rd)) == 0:
        res["measured_stream_read_GBps"] = rd.value
        print(f"stream-read probe: {rd.value:,.0f} GB/s", flush=True)
    # 1. the transform kernels
    s128 = signs(rng, 128)
    t128 = da.Transform.padding_hadamard(s128, 128)
    t768 = da.Transform.double_hadamard(signs(rng, 768), signs(rng, 768))
    res["apply"] = [apply_leg("padding_hadamard_128", t128, a.n, a.steps),
                    apply_leg("double_hadamard_768", t768, a.n, a.steps)]
    # 2. device rows -> MM4 images
    dim, R, pruned = 128, 32, 28
    base, q = make_data(torch, dev, a.n, dim, a.nq, "sift_like", 1, 2)[:2]
    base, q = base.float().contiguous(), q.float().contiguous()
    lb = 20 + dim // 2
    dimg = torch.empty((a.n, lb), dtype=torch.uint8, device="cuda")
    dev_wall, host_wall = [], []
    for i in range(a.steps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        da.minmax_quantize_device(t128, base.data_ptr(), a.n, 4, dimg.data_ptr())
        if i:
            dev_wall.append(time.perf_counter() - t0)
    for i in range(3):
        t0 = time.perf_counter()
        hb = base.cpu().numpy()
        t1 = time.perf_counter()
        hy = host_hadamard(hb, s128)
        t2 = time.perf_counter()
        da.minmax_compress(hy, 4)
        t3 = time.perf_counter()
        if i:
            host_wall.append(dict(to_host=t1 - t0, host_transform=t2 - t1, minmax_compress=t3 - t2, total=t3 - t0))
    res["quantize_mm4"] = dict(device_route_wall_s=spread(dev_wall), host_route_wall_s=host_wall)
    print(f"quantize MM4 1 M x 128: device route {np.median(dev_wall) * 1e3:.1f} ms; host route {host_wall}", flush=True)
    # 3. recall with and without the transform
    cfg = da.build_config(pruned, R, 100, intra_batch_candidates=da.IBC_NONE)  # as bench.py builds
    mean = base.double().mean(0).float()
    medoid = int(torch.argmin(((base - mean[None, :]) ** 2).sum(1)).item())
    hb = base.cpu().numpy()
    f32p = da.Provider(da.F32, da.L2, dim, a.n, R, hb[medoid:medoid + 1])
    f32p.set_elements(0, hb)
    f32p.build(cfg, 0, a.n, 0.05, 16384)
    adj = f32p.download_graph()
    f32p.close()
    gt = np.asarray(ground_truth(torch, base, q, 10))
    hq = q.cpu().numpy()
    res["recall"] = []
    for tname, t in (("none", da.Transform.null(dim)), ("padding_hadamard", t128)):
        for bits, dtype in ((8, da.MM8), (4, da.MM4)):
            rows = da.minmax_quantize(t, hb[medoid:medoid + 1], bits)
            lb = rows.shape[1]
            dimg = torch.empty((a.n, lb), dtype=torch.uint8, device="cuda")
            da.minmax_quantize_device(t, base.data_ptr(), a.n, bits, dimg.data_ptr())
            p = da.Provider(dtype, da.L2, dim, a.n, R, rows)
            p.set_elements_device(0, dimg.data_ptr(), a.n)
            p.upload_graph(adj)
            qc = da.minmax_quantize(t, hq, bits)
            for L in (26, 64):
                ids, _, st = p.search(da.Knn(L, 1), qc, 10)
                r = dict(transform=tname, bits=bits, L=L, recall_at_10=float(recall_at_k(ids, gt, 10)),
                         mean_cmps=float(st["cmps"].mean()), mean_hops=float(st["hops"].mean()))
                res["recall"].append(r)
                print(r, flush=True)
            p.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
