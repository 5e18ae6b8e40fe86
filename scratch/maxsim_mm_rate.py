#!/usr/bin/env python3
"""Rate of the MinMax multi-vector scoring kernels at the late-interaction shape: dim 128, 32-row queries,
128-row documents, 64 queries x 256 candidates.  Three things, alternating within each round so that they share the
machine's mood: the f32 set of the same (decompressed MM8) tokens in kernel order -- the baseline; MM8, MM4, MM1 and the
mixed pair (8, 4) in kernel order (int8 matrix cores); the same four in reference order (the plain kernel).

Times are HIP-event times of the scoring launch alone (dann_debug_mvset_kernel_time): the queries' repack is not in them.
Per configuration: --warm launches untimed, then --rounds rounds of --reps launches; the table gives the median round and
the spread (min .. max) of the per-launch time over the rounds.

    python scratch/maxsim_mm_rate.py [--ndocs 4096] > profiles/maxsim_mm_rate.txt     (the last line is one JSON object)
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndocs", type=int, default=4096)
    ap.add_argument("--doc-rows", type=int, default=128)
    ap.add_argument("--qrows", type=int, default=32)
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--cands", type=int, default=256)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import diskann_amd as da
    L = da.lib()
    rng = np.random.default_rng(2025)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda x: torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    MM = {1: da.MM1, 4: da.MM4, 8: da.MM8}

    tokens = (rng.standard_normal((1 << 15, a.dim)) * rng.uniform(0.1, 8.0, (1 << 15, 1))).astype(np.float32)

    def compress(x, bits):
        out = np.zeros((len(x), L.dann_layer_bytes(MM[bits], a.dim)), np.uint8)
        da._ffi.check(L.dann_minmax_compress(-1, bits, vp(x), len(x), a.dim, 1.0, vp(out), None), "dann_minmax_compress")
        return out

    def decompress8(img):  # a * code + b
        h = np.ascontiguousarray(img[:, 4:20]).view(np.float32)
        return (h[:, 2:3] * img[:, 20:].astype(np.float32) + h[:, 0:1]).astype(np.float32)

    nrows = a.ndocs * a.doc_rows
    doc_tok = np.arange(nrows) % len(tokens)
    q_tok = rng.integers(0, len(tokens), a.nq * a.qrows)
    off = (np.arange(a.ndocs + 1, dtype=np.uint64) * np.uint64(a.doc_rows))
    qoff = (np.arange(a.nq + 1, dtype=np.uint32) * np.uint32(a.qrows))
    cand = rng.integers(0, a.ndocs, (a.nq, a.cands)).astype(np.uint32)
    dcand, dqoff = dev(cand), dev(qoff)
    images = {b: compress(tokens, b) for b in MM}
    f32_tokens = decompress8(images[8])

    # (name, set dtype, query dtype, rows of the set, rows of the queries, order)
    configs = [("f32 kernel (baseline)", da.F32, da.F32, f32_tokens, f32_tokens, da.MAXSIM_KERNEL)]
    for order, oname in ((da.MAXSIM_KERNEL, "kernel"), (da.MAXSIM_REFERENCE, "reference")):
        for qb, db in ((8, 8), (4, 4), (1, 1), (8, 4)):
            configs.append((f"MM({qb},{db}) {oname}", MM[db], MM[qb], images[db], images[qb], order))
    sets, runs = {}, []
    for name, sdt, qdt, drows, qrows, order in configs:
        if sdt not in sets:
            h = C.c_void_p()
            rows = np.ascontiguousarray(drows[doc_tok])
            da._ffi.check(L.dann_mvset_create(-1, sdt, a.dim, a.ndocs, vp(off), vp(rows), C.byref(h)), "dann_mvset_create")
            sets[sdt] = (h, rows.nbytes / 2**20)
        h, mib = sets[sdt]
        runs.append(dict(name=name, h=h, set_mib=mib, qdt=qdt, dq=dev(np.ascontiguousarray(qrows[q_tok])), order=order,
                         out=torch.zeros(a.nq * a.cands, dtype=torch.float32, device="cuda"), ms=[]))

    def launch(r, n):
        da._ffi.check(L.dann_mvset_set_query_dtype(r["h"], r["qdt"]), "dann_mvset_set_query_dtype")
        L.dann_debug_mvset_kernel_time(r["h"], 1, None, None)
        for _ in range(n):
            da._ffi.check(L.dann_maxsim_batch_device(r["h"], r["order"], ptr(r["dq"]), ptr(dqoff), a.nq, ptr(dcand), a.cands,
                                                     ptr(r["out"]), None), "dann_maxsim_batch_device")
        ms, k = C.c_double(), C.c_uint64()
        L.dann_debug_mvset_kernel_time(r["h"], 0, C.byref(ms), C.byref(k))
        assert k.value == n
        return ms.value / n

    for r in runs:
        launch(r, a.warm)
    for _ in range(a.rounds):
        for r in runs:
            r["ms"].append(launch(r, a.reps))

    pairs = a.nq * a.cands
    print(f"# {a.nq} queries x {a.cands} candidates, {a.qrows}-row queries, {a.doc_rows}-row documents, dim {a.dim}, "
          f"{a.ndocs} documents; {a.warm} warm launches, then {a.rounds} rounds x {a.reps} launches, configurations alternating")
    print("configuration            set_MiB  ms/launch(median)   min .. max     Mpairs/s  Tmac/s  vs_f32_kernel")
    base = float(np.median(runs[0]["ms"]))
    table = []
    for r in runs:
        med, lo, hi = float(np.median(r["ms"])), min(r["ms"]), max(r["ms"])
        macs = pairs * a.qrows * a.doc_rows * a.dim
        print(f"{r['name']:24s} {r['set_mib']:7.0f} {med:12.4f}      {lo:8.4f} .. {hi:8.4f} {pairs / med / 1e3:9.2f} "
              f"{macs / med / 1e9:7.2f} {base / med:10.2f}x", flush=True)
        table.append(dict(config=r["name"], set_mib=round(r["set_mib"], 1), ms_median=round(med, 4), ms_min=round(lo, 4),
                          ms_max=round(hi, 4), speedup_vs_f32_kernel=round(base / med, 3)))
    # the two kernels of a MinMax pair return the same bits
    for i in range(1, 5):
        k, ref = runs[i]["out"].cpu().numpy(), runs[i + 4]["out"].cpu().numpy()
        assert np.array_equal(k.view(np.uint32), ref.view(np.uint32)), runs[i]["name"]
    print("# kernel order and reference order returned the same bits for every MinMax configuration")
    print(json.dumps(dict(bench="maxsim_mm_rate", nq=a.nq, cands=a.cands, qrows=a.qrows, doc_rows=a.doc_rows, dim=a.dim,
                          ndocs=a.ndocs, warm=a.warm, rounds=a.rounds, reps=a.reps, results=table)))
    for h, _ in sets.values():
        L.dann_mvset_destroy(h)


if __name__ == "__main__":
    main()
