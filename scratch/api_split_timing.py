"""Host-side cost of the staged host-pointer entry points, before and after they moved onto HostStage (host_stage.h): the
range, filtered, diverse, flat (host form), rerank and record searches at the sizes of their tests, and bench.py's
headline.  Two builds of libdann_hip.so are measured in alternation, `--runs` fresh processes each; a figure of one
process is the median wall time of `--calls` steady-state calls after three warm-up calls.  The bar: the branch's median
over its runs lies inside the parent's min-to-max range, or on the faster side of it.
   usage: python scratch/api_split_timing.py --parent-lib /path/to/parent/libdann_hip.so [--runs 3] [--bench-steps 20]
                                             [--graph-cache FILE] [--out profiles/api_split_timing.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def child(calls):
    """one process: every entry point on the library DANN_LIB_PATH names; prints {name: median ms}"""
    import numpy as np
    import diskann_amd as da
    from helpers import random_graph

    rng = np.random.default_rng(3)
    n, dim, R = 3000, 24, 16
    data = rng.standard_normal((n, dim)).astype(np.float32)
    gix = da.Provider(da.F32, da.L2, dim, n, R, data[:1].copy())
    gix.set_elements(0, data)
    gix.upload_graph(random_graph(rng, n, R))
    gix.set_attributes(0, rng.integers(0, 20, n + 1).astype(np.uint32))
    q = rng.standard_normal((40, dim)).astype(np.float32)
    match = rng.random((40, n + 1)) < 0.1
    cand = rng.integers(0, n, (40, 64)).astype(np.uint32)
    u8 = rng.integers(0, 2, (1501, 8), dtype=np.uint8)
    fix = da.Provider(da.U8, da.L2, 8, 1500, 4, u8[1500:])
    fix.set_elements(0, u8[:1500])
    fq = rng.integers(0, 2, (11, 8), dtype=np.uint8)
    fq_many = np.ascontiguousarray(np.tile(fq, (6000, 1))[:65536 + 7])
    legs = {
        "range 40q": lambda: gix.range_search(q, 16, 30.0, out_cap=3001),
        "filtered 40q": lambda: gix.filtered_search(da.Knn(20), q, 10, match),
        "filtered range 40q": lambda: gix.filtered_range_search(q, 16, 30.0, match, out_cap=3001),
        "diverse 40q": lambda: gix.diverse_search(da.Knn(20, 1), q, 10, 3, 10),
        "flat 11q": lambda: fix.flat_search(fq, 10),
        "flat 65543q": lambda: fix.flat_search(fq_many, 3, first=0, n=64),
        "rerank 40q": lambda: gix.rerank(q, cand, 10),
        "record 40q": lambda: gix.search_record_queries(q, 20),
        "record 40 slots": lambda: gix.search_record(np.arange(40, dtype=np.uint32), 20),
    }
    out = {}
    for name, f in legs.items():
        for _ in range(3):
            f()
        ms = []
        for _ in range(calls if "65543" not in name else max(3, calls // 5)):
            t0 = time.perf_counter()
            f()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = statistics.median(ms)
    print("RESULT " + json.dumps(out), flush=True)


def run(cmd, lib, limit):
    env = dict(os.environ, DANN_LIB_PATH=lib)
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)} on {lib}: exit status {r.returncode}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--parent-lib")
    ap.add_argument("--branch-lib", default=os.path.join(ROOT, "diskann_amd", "libdann_hip.so"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20, help="0: leave bench.py out")
    ap.add_argument("--graph-cache", default="", help="bench.py --graph-cache (the first run builds the graph, the others load it)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.calls)
    libs = (("parent", args.parent_lib), ("branch", args.branch_lib))
    figs = {}  # name -> {"parent": [...], "branch": [...]}
    for r in range(args.runs):
        for side, lib in libs:
            text = run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls)], lib, 300)
            res = json.loads(next(ln for ln in text.splitlines() if ln.startswith("RESULT "))[7:])
            for k, v in res.items():
                figs.setdefault(k + " (ms)", {"parent": [], "branch": []})[side].append(v)
            if args.bench_steps:
                cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "5"]
                if args.graph_cache:
                    cmd += ["--graph-cache", args.graph_cache]
                text = run(cmd, lib, 600)
                line = next(ln for ln in reversed(text.splitlines()) if ln.startswith("{") and '"value"' in ln)
                figs.setdefault("bench.py headline (QPS)", {"parent": [], "branch": []})[side].append(json.loads(line)["value"])
            print(f"run {r} {side} done", flush=True)
    lines = [f"# parent and branch alternating, {args.runs} fresh processes each; ms: median of {args.calls} steady-state calls",
             "# figure | parent min median max | branch min median max | branch median vs the parent's range"]
    for name, d in figs.items():
        p, b = sorted(d["parent"]), sorted(d["branch"])
        bm = statistics.median(b)
        higher_is_better = "QPS" in name
        if p[0] <= bm <= p[-1]:
            verdict = "inside"
        elif (bm > p[-1]) == higher_is_better:
            verdict = "faster"
        else:
            verdict = "SLOWER"
        fmt = (lambda x: f"{x:.0f}") if higher_is_better else (lambda x: f"{x:.3f}")
        lines.append(f"{name} | {fmt(p[0])} {fmt(statistics.median(p))} {fmt(p[-1])} | {fmt(b[0])} {fmt(bm)} {fmt(b[-1])} | {verdict}")
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
