"""Rate of the exhaustive scan (dann_flat_search_batch_device) on one device: 1 M x 128 f32 / u8 and 1 M x 768 f16 at
nq in {1, 64, 4096}, k = 10, three runs each, alternating with the torch brute force of benchdata.ground_truth on the
same inputs (for scale only: its distances are not the library's).  Reports rows/s (rows x queries scored), algorithmic
GB/s (rows x row bytes x query tiles, against dann_debug_stream_read_gbps on the same device) and TF/s (2 x rows x
queries x dim).  A call of the device-pointer form is complete on return: the time is the wall time of that call, after
one warm-up call.   usage: python scratch/flat_rate.py [--n 1000000] [--out profiles/flat_rate.txt]"""
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import benchdata
    import diskann_amd as da
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    gbps = C.c_double()
    da._ffi.check(da.lib().dann_debug_stream_read_gbps(0, 1 << 30, 10, C.byref(gbps)), "stream_read")
    say(f"# device {torch.cuda.get_device_name(0)}; stream-read probe {gbps.value:.0f} GB/s; n {args.n}, k {args.k}")
    say("# rows dtype dim nq tile | flat ms (runs) | Grows/s alg GB/s (of probe) TF/s | torch brute force ms (runs)")
    shapes = [(da.F32, "f32", 128, torch.float32), (da.U8, "u8", 128, torch.uint8), (da.F16, "f16", 768, torch.float16)]
    for dt, name, dim, tdt in shapes:
        base_f, q_f = benchdata.make_data(torch, dev, args.n, dim, max(args.nq), "uniform", 1, 2)
        if dt == da.U8:
            base, queries = ((base_f + 1) * 127.5).to(tdt), ((q_f + 1) * 127.5).to(tdt)
        else:
            base, queries = base_f.to(tdt), q_f.to(tdt)
        base_t, q_t = base.float(), queries.float()  # what the torch brute force reads
        del base_f, q_f
        gix = da.Provider(dt, da.L2, dim, args.n, 4, np.zeros((1, dim), da.NP_DTYPE[dt]))
        gix.set_elements_device(0, base.data_ptr(), args.n)
        row_bytes = base.element_size() * dim
        for nq in args.nq:
            q = queries[:nq].contiguous()
            ids = torch.empty((nq, args.k), dtype=torch.int32, device=dev)
            dist = torch.empty((nq, args.k), dtype=torch.float32, device=dev)
            tile = min(8, 1 << max(nq - 1, 0).bit_length())
            torch.cuda.synchronize()

            def flat():
                t0 = time.perf_counter()
                gix.flat_search_device(q.data_ptr(), nq, args.k, ids.data_ptr(), dist.data_ptr())
                return (time.perf_counter() - t0) * 1e3

            def brute():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                benchdata.ground_truth(torch, base_t, q_t[:nq], args.k)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            flat(), brute()
            f_ms, b_ms = [], []
            for _ in range(args.runs):
                f_ms.append(flat())
                b_ms.append(brute())
            t = min(f_ms) * 1e-3
            alg = args.n * row_bytes * -(-nq // tile) / t / 1e9
            say(f"{args.n} {name} {dim} {nq} {tile} | {min(f_ms):.3f} ({' '.join(f'{x:.3f}' for x in f_ms)}) | "
                f"{args.n * nq / t / 1e9:.2f} {alg:.0f} ({100 * alg / gbps.value:.0f} %) {2 * args.n * nq * dim / t / 1e12:.2f} | "
                f"{min(b_ms):.3f} ({' '.join(f'{x:.3f}' for x in b_ms)})")
        gix.close()
        del base, queries, base_t, q_t
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
