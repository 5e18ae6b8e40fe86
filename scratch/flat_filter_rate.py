"""Rate of the filtered and the range exhaustive scans (dann_flat_filtered_search_batch_device,
dann_flat_range_search_batch_device) on one device, next to the unfiltered scan of this build and of a parent build:
1 M x 128-d f32, L2, k = 10, nq in {64, 4096}; every line `--runs` times, the variants of a line alternating inside this
process.  The parent library (DANN_LIB_PATH_PARENT, or --parent) is loaded as a second instance of the package, so both
run on the same rows in the same process; before any timing the unfiltered outputs of the two are compared (ids and
distance bits must be equal).  A call of a device-pointer form is complete on return: the time is the wall time of that
call, after one warm-up call.
usage: python scratch/flat_filter_rate.py --parent PATH/libdann_hip.so [--n 1000000] [--out profiles/flat_filter_rate.txt]"""
import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW_EXPORTS = ("dann_flat_filtered_search_batch", "dann_flat_range_search_batch", "dann_flat_filtered_search_batch_device",
               "dann_flat_range_search_batch_device")


def load_parent(path):
    """the package once more, bound to the parent's library (which lacks the new exports)"""
    os.environ["DANN_LIB_PATH"] = path
    pkg = os.path.join(ROOT, "diskann_amd")
    spec = importlib.util.spec_from_file_location("diskann_amd_parent", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["diskann_amd_parent"] = mod
    spec.loader.exec_module(mod)
    del os.environ["DANN_LIB_PATH"]
    for name in NEW_EXPORTS:
        mod._ffi.SYMBOLS.pop(name, None)
    assert mod._ffi.LIB_PATH == path
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="*", default=[64, 4096])
    ap.add_argument("--parent", default=os.environ.get("DANN_LIB_PATH_PARENT"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import benchdata
    import diskann_amd as da
    dp = load_parent(args.parent) if args.parent else None
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n, k, dim = args.n, args.k, 128
    nslots, words = n + 1, (n + 1 + 31) // 32
    base, queries = benchdata.make_data(torch, dev, n, dim, max(args.nq), "uniform", 1, 2)
    base, queries = base.float().contiguous(), queries.float().contiguous()
    start = np.zeros((1, dim), np.float32)
    gix = da.Provider(da.F32, da.L2, dim, n, 4, start)
    gix.set_elements_device(0, base.data_ptr(), n)
    pix = None
    if dp:
        pix = dp.Provider(dp.F32, dp.L2, dim, n, 4, start)
        pix.set_elements_device(0, base.data_ptr(), n)
    say(f"# device {torch.cuda.get_device_name(0)}; n {n} x {dim} f32 L2, k {k}; parent {'loaded' if dp else 'absent'}")

    def bitmap(p, rows):
        """rows bitmaps of `words` words, every slot set with probability p"""
        out = torch.empty((rows, words), dtype=torch.int32, device=dev)
        w = (1 << torch.arange(32, device=dev, dtype=torch.int64))
        for r0 in range(0, rows, 64):
            r1 = min(rows, r0 + 64)
            m = (torch.rand((r1 - r0, words, 32), device=dev) < p) if p < 1 else torch.ones((r1 - r0, words, 32), dtype=torch.bool, device=dev)
            v = (m.to(torch.int64) * w).sum(-1)
            out[r0:r1] = torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)
        return out

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def line(name, nq, variants):
        """variants: [(label, fn)], run alternately after one warm-up each"""
        for _, fn in variants:
            fn()
        ms = {label: [] for label, _ in variants}
        for _ in range(args.runs):
            for label, fn in variants:
                ms[label].append(timed(fn))
        say(f"{name} nq {nq} | " + " | ".join(f"{label} {min(v):.3f} ({' '.join(f'{x:.3f}' for x in v)})" for label, v in ms.items()))
        return {label: min(v) for label, v in ms.items()}

    for nq in args.nq:
        q = queries[:nq].contiguous()
        ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
        dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
        new = lambda: gix.flat_search_device(q.data_ptr(), nq, k, ids.data_ptr(), dist.data_ptr())  # noqa: E731
        variants = [("new", new)]
        if pix:
            ids_p, dist_p = torch.empty_like(ids), torch.empty_like(dist)
            par = lambda: pix.flat_search_device(q.data_ptr(), nq, k, ids_p.data_ptr(), dist_p.data_ptr())  # noqa: E731
            new(), par()
            same = bool(torch.equal(ids, ids_p) and torch.equal(dist.view(torch.int32), dist_p.view(torch.int32)))
            say(f"outputs nq {nq}: new and parent unfiltered ids and distance bits {'EQUAL' if same else 'DIFFER'}")
            assert same
            variants = [("parent", par), ("new", new), ("parent again", par)]
        base_ms = line("unfiltered", nq, variants)
        ref = base_ms.get("parent", base_ms["new"])
        if pix:
            say(f"  new / parent {base_ms['new'] / base_ms['parent']:.3f}; parent again / parent {base_ms['parent again'] / base_ms['parent']:.3f}")
        for label, p, rows in (("shared 1 %", 0.01, 1), ("shared 10 %", 0.1, 1), ("all ones", 1.0, 1), ("per-query 1 %", 0.01, nq)):
            bits = bitmap(p, rows)
            stride = 0 if rows == 1 else words
            flt = lambda: gix.flat_search_device(q.data_ptr(), nq, k, ids.data_ptr(), dist.data_ptr(), d_bits=bits.data_ptr(),  # noqa: E731
                                                 stride_words=stride)
            r = line(f"filter {label}", nq, [("filtered", flt)] + ([("parent unfiltered", par)] if pix else [("unfiltered", new)]))
            say(f"  filtered / {'parent ' if pix else ''}unfiltered {r['filtered'] / (r.get('parent unfiltered') or r['unfiltered']):.4f}")
            del bits
        # a radius that gives about 100 results a query: the median 100th distance of the first queries
        m = min(nq, 64)
        i100 = torch.empty((m, 100), dtype=torch.int32, device=dev)
        d100 = torch.empty((m, 100), dtype=torch.float32, device=dev)
        gix.flat_search_device(q.data_ptr(), m, 100, i100.data_ptr(), d100.data_ptr())
        radius = float(d100[:, -1].median())
        r_cnt = torch.empty(nq, dtype=torch.int32, device=dev)
        gix.flat_range_search_device(q.data_ptr(), nq, radius, 0, 0, 0, r_cnt.data_ptr())
        cap = int(r_cnt.max())  # (the count-only call sizes the outputs: every result fits)
        r_ids = torch.empty((nq, cap), dtype=torch.int32, device=dev)
        r_d = torch.empty((nq, cap), dtype=torch.float32, device=dev)
        rng_ = lambda: gix.flat_range_search_device(q.data_ptr(), nq, radius, cap, r_ids.data_ptr(), r_d.data_ptr(), r_cnt.data_ptr())  # noqa: E731
        cnt_ = lambda: gix.flat_range_search_device(q.data_ptr(), nq, radius, 0, 0, 0, r_cnt.data_ptr())  # noqa: E731
        line(f"range r {radius:.4f}", nq, [("range", rng_), ("count only", cnt_), ("unfiltered k-NN", new)])
        say(f"  results per query: mean {float(r_cnt.float().mean()):.1f}, max {int(r_cnt.max())}; unfiltered parent {ref:.3f} ms")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
