"""Rate of the exhaustive scan over PQ code rows (dann_pq_linear_search_batch_device) on one device: 1 M rows of random
codes at 16 chunks (128-d) and 64 chunks (768-d), L2, k = 10, nq in {1, 64, 4096}; best of `--runs`, alternating with

  * the composition a caller had before this entry point for the same answer: dann_pq_build_lut + dann_pq_scan over all
    ids + a top-k on the host (numpy argpartition: no tie rule, so a lower bound of its cost).  It ships nq x n ids up and
    nq x n floats down, so above --compose-max queries it is run on the first --compose-max only and scaled linearly: such a
    figure is marked `extrapolated`;
  * optionally (--split PATH) a second build of the library whose scan keeps one table per query in LDS instead of the
    interleaved tile (flat_pq_kernels.hip compiled with -DDANN_FLAT_PQ_SPLIT_TABLES, the other objects unchanged), loaded
    as a second instance of the package on the same rows; before any timing the outputs of the two are compared.

A call of the device-pointer form is complete on return: the time is the wall time of that call, after one warm-up call.
Before the timing the scan's ids and distance bits are checked against the composition on the first queries.
usage: python scratch/pq_linear_rate.py [--n 1000000] [--split PATH/libdann_split.so] [--out profiles/pq_linear_rate.txt]
       rocprofv3 --pmc COUNTERS --kernel-trace -d DIR -o p -- python scratch/pq_linear_rate.py --scan-only --nq 4096"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_variant(path):
    """the package once more, bound to another build of the library"""
    os.environ["DANN_LIB_PATH"] = path
    pkg = os.path.join(ROOT, "diskann_amd")
    spec = importlib.util.spec_from_file_location("diskann_amd_split", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["diskann_amd_split"] = mod
    spec.loader.exec_module(mod)
    del os.environ["DANN_LIB_PATH"]
    assert mod._ffi.LIB_PATH == path
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--shapes", type=str, nargs="*", default=["16x128", "64x768"])
    ap.add_argument("--compose-max", type=int, default=64)
    ap.add_argument("--split", default=None)
    ap.add_argument("--scan-only", action="store_true", help="two calls of the scan per cell and nothing else: what a "
                    "profiler run wraps (counters in a run of their own)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import diskann_amd as da
    ds = load_variant(args.split) if args.split else None
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n, k = args.n, args.k
    say(f"# device {torch.cuda.get_device_name(0)}; n {n} random code rows, L2, k {k}; split-table build {'loaded' if ds else 'absent'}")
    say("# chunks dim nq tile | scan ms (runs) | Grows x queries/s | composition ms (runs) | composition / scan"
        + (" | split tables ms (runs) | split / interleaved" if ds else ""))
    rng = np.random.default_rng(1)
    for shape in args.shapes:
        chunks, dim = (int(x) for x in shape.split("x"))
        offsets = np.linspace(0, dim, chunks + 1).round().astype(np.uint32)
        pivots = rng.standard_normal((256, dim)).astype(np.float32)
        codes = rng.integers(0, 256, (n + 1, chunks), dtype=np.uint8)
        queries = rng.standard_normal((max(args.nq), dim)).astype(np.float32)
        make = lambda m: m.Provider(m.PQ, m.L2, dim, n, 4, codes[n:], pq_pivots=pivots, pq_offsets=offsets)  # noqa: E731
        gix = make(da)
        gix.set_elements(0, codes[:n])
        six = None
        if ds:
            six = make(ds)
            six.set_elements(0, codes[:n])
        dq = torch.from_numpy(queries).to(dev)
        every = np.arange(n, dtype=np.uint32)
        for nq in args.nq:
            ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
            dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
            cap = 1 << (k + 512 - 1).bit_length()  # (flat_pq_plan.h: a step of 512 rows above k)
            per_query = chunks * 1024 + cap * 8 + 16
            tile = next(t for t in (8, 4, 2, 1) if t == 1 or (t // 2 < nq and per_query * t <= 150 * 1024))
            m = min(nq, args.compose_max)
            ids_m, off_m = np.tile(every, m), (np.arange(m + 1, dtype=np.uint64) * n)
            torch.cuda.synchronize()

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            scan = lambda ix=gix: ix.pq_linear_search_device(dq.data_ptr(), nq, k, ids.data_ptr(), dist.data_ptr())  # noqa: E731

            def compose():
                lut = da.pq_build_lut(da.L2, pivots, offsets, queries[:m])
                d = da.pq_scan(lut, codes[:n], ids_m, off_m).reshape(m, n)
                part = np.argpartition(d, k, axis=1)[:, :k]
                pd = np.take_along_axis(d, part, 1)
                order = np.argsort(pd, axis=1, kind="stable")
                return np.take_along_axis(part, order, 1), np.take_along_axis(pd, order, 1)

            if args.scan_only:
                say(f"{chunks} {dim} {nq} {tile} | {timed(scan)[0]:.3f} {timed(scan)[0]:.3f}")
                continue
            # the same answer: distance bits always; ids wherever the k + 1 best distances of a query are distinct
            scan()
            _, (ci, cd) = timed(compose)
            gi, gd = ids[:m].cpu().numpy().view(np.uint32), dist[:m].cpu().numpy()
            assert np.array_equal(gd.view(np.uint32), cd.view(np.uint32)), "distance bits differ from the composition"
            distinct = np.array([len(set(r.tolist())) == k for r in cd])
            assert np.array_equal(gi[distinct], ci[distinct].astype(np.uint32)), "ids differ from the composition"
            if six:
                ids_s, dist_s = torch.empty_like(ids), torch.empty_like(dist)
                split = lambda: six.pq_linear_search_device(dq.data_ptr(), nq, k, ids_s.data_ptr(), dist_s.data_ptr())  # noqa: E731
                split()
                assert torch.equal(ids, ids_s) and torch.equal(dist.view(torch.int32), dist_s.view(torch.int32))
            s_ms, c_ms, p_ms = [], [], []
            for _ in range(args.runs):
                s_ms.append(timed(scan)[0])
                c_ms.append(timed(compose)[0] * (nq / m))
                if six:
                    p_ms.append(timed(split)[0])
            t = min(s_ms) * 1e-3
            runs = lambda v: f"{min(v):.3f} ({' '.join(f'{x:.3f}' for x in v)})"  # noqa: E731
            extra = " extrapolated from %d queries" % m if m < nq else ""
            line = (f"{chunks} {dim} {nq} {tile} | {runs(s_ms)} | {n * nq / t / 1e9:.2f} | {runs(c_ms)}{extra} | "
                    f"{min(c_ms) / min(s_ms):.1f}")
            if six:
                line += f" | {runs(p_ms)} | {min(p_ms) / min(s_ms):.3f}"
            say(line)
        gix.close()
        if six:
            six.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
