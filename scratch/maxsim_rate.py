#!/usr/bin/env python3
"""Rate of the multi-vector scoring kernels: dann_maxsim_batch_device on 64 queries x 4096 candidates over a
set too large for L2 and the Infinity Cache, both orders, f32 and f16, 32 and 64 query rows, documents of 64 rows and of
64 .. 180 rows drawn uniformly, dim 128.  Times are HIP-event times of the scoring launch alone
(dann_debug_mvset_kernel_time), warm, averaged over --reps launches.

    python scratch/maxsim_rate.py [--ndocs 24576] [--reps 5] > profiles/maxsim_rate.txt

Ceilings (measured, microarchitecture guide): 155 TF/s f32 MFMA, 6.29 TB/s HBM.  "of ceiling" is the least time the
hardware could take -- the larger of flop / 155 TF/s and document bytes / 6.29 TB/s -- over the measured time.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_F32_TFLOPS, HBM_TBPS = 155.0, 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndocs", type=int, default=24576)
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--cands", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import diskann_amd as da
    from diskann_amd.multivector import csr
    L = da.lib()
    rng = np.random.default_rng(2024)
    base = rng.standard_normal((1 << 16, a.dim)).astype(np.float32)

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def dev(x):
        return torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).cuda()

    print(f"# {a.nq} queries x {a.cands} candidates, dim {a.dim}, {a.ndocs} documents, {a.reps} timed launches each (warm)")
    print("dtype doc_rows  set_MiB  Q  order      ms/launch   Mpairs/s    TF/s    GB/s  of_ceiling  bound_by")
    for dtype, npdt, name in ((da.F32, np.float32, "f32"), (da.F16, np.float16, "f16")):
        for shape in ("64", "64..180"):
            lens = np.full(a.ndocs, 64) if shape == "64" else rng.integers(64, 181, a.ndocs)
            off = np.zeros(a.ndocs + 1, np.uint64)
            off[1:] = np.cumsum(lens)
            nrows = int(off[-1])
            rows = base[np.arange(nrows) % len(base)].astype(npdt)
            h = C.c_void_p()
            da._ffi.check(L.dann_mvset_create(-1, dtype, a.dim, a.ndocs, off.ctypes.data_as(C.c_void_p),
                                              rows.ctypes.data_as(C.c_void_p), C.byref(h)), "dann_mvset_create")
            set_mib = rows.nbytes / 2**20
            del rows
            cand = rng.integers(0, a.ndocs, (a.nq, a.cands)).astype(np.uint32)
            doc_rows = int(lens[cand].sum())
            dcand = dev(cand)
            for Q in (32, 64):
                queries = [base[rng.integers(0, len(base), Q)].astype(npdt) for _ in range(a.nq)]
                qoff, qrows = csr(queries, npdt, a.dim, np.uint32)
                dq, do = dev(qrows), dev(qoff)
                out = {}
                for order, oname in ((da.MAXSIM_KERNEL, "kernel"), (da.MAXSIM_REFERENCE, "reference")):
                    dch = torch.zeros(a.nq * a.cands, dtype=torch.float32, device="cuda")
                    reps = a.reps if order == da.MAXSIM_KERNEL else max(1, a.reps // 2)
                    for timed in (False, True):
                        L.dann_debug_mvset_kernel_time(h, 1, None, None)
                        for _ in range(reps if timed else 1):
                            da._ffi.check(L.dann_maxsim_batch_device(h, order, ptr(dq), ptr(do), a.nq, ptr(dcand), a.cands,
                                                                     ptr(dch), None), "dann_maxsim_batch_device")
                    ms, n = C.c_double(), C.c_uint64()
                    L.dann_debug_mvset_kernel_time(h, 0, C.byref(ms), C.byref(n))
                    assert n.value == reps
                    t = ms.value / reps * 1e-3
                    flop = 2.0 * Q * doc_rows * a.dim
                    nbytes = doc_rows * a.dim * np.dtype(npdt).itemsize
                    t_flop, t_mem = flop / (MFMA_F32_TFLOPS * 1e12), nbytes / (HBM_TBPS * 1e12)
                    print(f"{name:5s} {shape:8s} {set_mib:8.0f} {Q:3d}  {oname:9s} {t * 1e3:10.3f} {a.nq * a.cands / t / 1e6:10.2f} "
                          f"{flop / t / 1e12:7.2f} {nbytes / t / 1e9:7.0f} {max(t_flop, t_mem) / t:10.3f}  "
                          f"{'mfma' if t_flop >= t_mem else 'hbm'}", flush=True)
                    out[order] = dch.cpu().numpy()
                k, r = out[da.MAXSIM_KERNEL], out[da.MAXSIM_REFERENCE]
                rel = np.max(np.abs(k - r) / np.maximum(np.abs(r), 1.0))
                print(f"#   the two orders' Chamfer sums differ by at most {rel:.2e} relative (different summations)", flush=True)
            L.dann_mvset_destroy(h)
    print("# no CPU column: there is no Rust toolchain here to run the reference's own benchmark")


if __name__ == "__main__":
    main()
