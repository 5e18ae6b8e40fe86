#!/usr/bin/env python3
"""Rate of the exhaustive multi-vector scan: dann_mv_flat_search_batch_device, kernel order, Chamfer, on a
ColBERT-like set -- documents of 64 .. 128 rows drawn uniformly, dim 128, f32 and f16 -- 64 queries x 32 rows, k = 100,
against the same result obtained the only way the parent commit has: dann_chamfer_rerank_batch_device over every
document in slices of 4096 candidates, merged on the host.  Times are wall-clock times of the host-synchronous calls,
warm, averaged over --reps calls that rotate through --sets query sets; the scan's HIP-event time
(dann_debug_mvset_kernel_time) is printed beside it.

    python scratch/mv_flat_rate.py [--ndocs 100000] [--reps 5] > profiles/mv_flat_rate.txt

Ceilings (measured, microarchitecture guide): 155 TF/s f32 MFMA, 6.29 TB/s HBM.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_F32_TFLOPS, HBM_TBPS = 155.0, 6.29
SLICE = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndocs", type=int, default=100000)
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--qrows", type=int, default=32)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    a = ap.parse_args()
    import torch
    import diskann_amd as da
    from diskann_amd.multivector import csr
    L = da.lib()
    rng = np.random.default_rng(2025)
    base = rng.standard_normal((1 << 16, a.dim)).astype(np.float32)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda x: torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731

    print(f"# {a.nq} queries x {a.qrows} rows, dim {a.dim}, {a.ndocs} documents of 64..128 rows, k {a.k}, {a.reps} timed calls (warm)")
    print("dtype  set_MiB  path     ms/call  scan_ms   set_GB/s  of_hbm    TF/s  of_mfma")
    for dtype, npdt, name in ((da.F32, np.float32, "f32"), (da.F16, np.float16, "f16")):
        lens = rng.integers(64, 129, a.ndocs)
        off = np.zeros(a.ndocs + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        nrows = int(off[-1])
        rows = base[np.arange(nrows) % len(base)].astype(npdt)
        h = C.c_void_p()
        da._ffi.check(L.dann_mvset_create(-1, dtype, a.dim, a.ndocs, off.ctypes.data_as(C.c_void_p),
                                          rows.ctypes.data_as(C.c_void_p), C.byref(h)), "dann_mvset_create")
        nbytes, flop = rows.nbytes, 2.0 * a.nq * a.qrows * nrows * a.dim
        del rows
        qsets = []
        for _ in range(a.sets):
            qoff, qrows = csr([base[rng.integers(0, len(base), a.qrows)].astype(npdt) for _ in range(a.nq)], npdt, a.dim, np.uint32)
            qsets.append((dev(qrows), dev(qoff)))
        di = torch.zeros(a.nq * a.k, dtype=torch.int32, device="cuda")
        dd = torch.zeros(a.nq * a.k, dtype=torch.float32, device="cuda")
        dn = torch.zeros(a.nq, dtype=torch.int32, device="cuda")

        def flat(s):
            dq, do = qsets[s]
            da._ffi.check(L.dann_mv_flat_search_batch_device(h, da.MAXSIM_KERNEL, da.MV_CHAMFER, ptr(dq), ptr(do), a.nq, 0, a.ndocs,
                                                             a.k, None, ptr(di), ptr(dd), None), "dann_mv_flat_search_batch_device")
            return di.cpu().numpy().view(np.uint32).reshape(a.nq, a.k), dd.cpu().numpy().reshape(a.nq, a.k)

        def sliced(s):
            dq, do = qsets[s]
            ids, dists = [], []
            for lo in range(0, a.ndocs, SLICE):
                cand = np.tile(np.arange(lo, min(lo + SLICE, a.ndocs), dtype=np.uint32), (a.nq, 1))
                dc = dev(cand)
                da._ffi.check(L.dann_chamfer_rerank_batch_device(h, da.MAXSIM_KERNEL, ptr(dq), ptr(do), a.nq, ptr(dc), cand.shape[1],
                                                                 a.k, ptr(di), ptr(dd), ptr(dn)), "dann_chamfer_rerank_batch_device")
                ids.append(di.cpu().numpy().view(np.uint32).reshape(a.nq, a.k))
                dists.append(dd.cpu().numpy().reshape(a.nq, a.k))
            ids, dists = np.hstack(ids), np.hstack(dists)
            # (distance ascending, id descending): the queue's order; padding (+inf, 0xFFFFFFFF) sorts last
            order = np.lexsort((-ids.astype(np.int64), dists), axis=1)[:, :a.k]
            return np.take_along_axis(ids, order, 1), np.take_along_axis(dists, order, 1)

        out = {}
        for pname, fn in (("flat", flat), ("sliced", sliced)):
            fn(0)  # warm
            L.dann_debug_mvset_kernel_time(h, 1, None, None)
            t0 = time.perf_counter()
            for r in range(a.reps):
                out[pname] = fn(r % a.sets)
            t = (time.perf_counter() - t0) / a.reps
            ms = C.c_double()
            L.dann_debug_mvset_kernel_time(h, 0, C.byref(ms), None)
            scan = ms.value / a.reps * 1e-3
            print(f"{name:5s} {nbytes / 2**20:8.0f}  {pname:7s} {t * 1e3:8.2f} {scan * 1e3:8.2f} {nbytes / scan / 1e9:10.0f} "
                  f"{nbytes / scan / 1e12 / HBM_TBPS:7.3f} {flop / scan / 1e12:7.2f} {flop / scan / 1e12 / MFMA_F32_TFLOPS:8.3f}", flush=True)
        same = np.array_equal(out["flat"][1].view(np.uint32), out["sliced"][1].view(np.uint32))
        print(f"#   distances of the two paths identical: {same}", flush=True)
        L.dann_mvset_destroy(h)


if __name__ == "__main__":
    main()
