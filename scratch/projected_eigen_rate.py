#!/usr/bin/env python3
"""Rate of the ProjectedEigen kernels against maxsim_mfma_kernel ON THE SAME SET AND CANDIDATES IN THE SAME
RUN: both run the same MFMAs over the same bytes, so the ratio is what the in-order epilogue costs.  64 queries x 4096
candidates over a set too large for L2 and the Infinity Cache, dim 128, 32 and 64 query rows, documents of 64 rows and of
64 .. 180 rows drawn uniformly, f32 and f16.  Times are HIP-event times of the scoring launch alone
(dann_debug_mvset_kernel_time).  Each configuration is warmed, then the configurations ALTERNATE within a round; a round's
figure is the mean of --reps launches, the table gives the median of --rounds rounds and their spread (min .. max).

    python scratch/projected_eigen_rate.py [--ndocs 24576] [--reps 3] [--rounds 7] > profiles/projected_eigen_rate.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndocs", type=int, default=24576)
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--cands", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
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

    # (column, entry point, order, launches per round): the reference-order kernel is slow and steady, one launch does
    configs = (("maxsim", L.dann_maxsim_batch_device, da.MAXSIM_KERNEL, a.reps),
               ("projeig", L.dann_projected_eigen_batch_device, da.MAXSIM_KERNEL, a.reps),
               ("projeig_ref", L.dann_projected_eigen_batch_device, da.MAXSIM_REFERENCE, 1))
    print(f"# {a.nq} queries x {a.cands} candidates, dim {a.dim}, {a.ndocs} documents; median of {a.rounds} rounds "
          f"(min .. max), {a.reps} launches per round, configurations alternating, warm")
    print("# TF/s = 2 Q D dim / time; ratio = projeig time / maxsim time (kernel order, same set, same candidates)")
    print("dtype doc_rows  set_MiB  Q   maxsim_ms (min..max)  TF/s   projeig_ms (min..max)  TF/s   ratio   projeig_ref_ms  TF/s")
    for dtype, npdt, name in ((da.F32, np.float32, "f32"), (da.F16, np.float16, "f16")):
        for shape in ("64", "64..180"):
            lens = np.full(a.ndocs, 64) if shape == "64" else rng.integers(64, 181, a.ndocs)
            off = np.zeros(a.ndocs + 1, np.uint64)
            off[1:] = np.cumsum(lens)
            rows = base[np.arange(int(off[-1])) % len(base)].astype(npdt)
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
                dout = torch.zeros(a.nq * a.cands, dtype=torch.float32, device="cuda")
                ms = {c[0]: [] for c in configs}
                for rnd in range(-1, a.rounds):  # round -1 warms every configuration and is not kept
                    for cname, fn, order, reps in configs:
                        L.dann_debug_mvset_kernel_time(h, 1, None, None)
                        for _ in range(reps):
                            da._ffi.check(fn(h, order, ptr(dq), ptr(do), a.nq, ptr(dcand), a.cands, ptr(dout), None), cname)
                        t, n = C.c_double(), C.c_uint64()
                        L.dann_debug_mvset_kernel_time(h, 0, C.byref(t), C.byref(n))
                        assert n.value == reps
                        if rnd >= 0:
                            ms[cname].append(t.value / reps)
                flop = 2.0 * Q * doc_rows * a.dim
                med = {c: float(np.median(v)) for c, v in ms.items()}
                cols = [f"{med[c]:8.3f} ({min(ms[c]):.3f}..{max(ms[c]):.3f}) {flop / med[c] / 1e9:6.2f}" for c in ("maxsim", "projeig")]
                print(f"{name:5s} {shape:8s} {set_mib:8.0f} {Q:3d}  {cols[0]}  {cols[1]}  {med['projeig'] / med['maxsim']:6.3f}  "
                      f"{med['projeig_ref']:10.3f} {flop / med['projeig_ref'] / 1e9:6.2f}", flush=True)
            L.dann_mvset_destroy(h)


if __name__ == "__main__":
    main()
