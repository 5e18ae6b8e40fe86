"""Do two builds of the library plan the same launches?  Runs the configurations below once per library (a child process
each, DANN_LIB_PATH), collects the library's `[dann]` verbose lines and the kernel family of every search, and compares
the two transcripts line for line and the search outputs byte for byte.

    python scratch/launch_plan_compare.py <lib A> <lib B> <out A.txt> <out B.txt>

Every configuration is searched twice: the first search sizes the visited table from the prior (and asks for the
kernel's registers), the second from the calibrated 90th percentile of the comparisons (from 256 queries on)."""
import hashlib
import os
import subprocess
import sys

import numpy as np

N, DIM, R = 5000, 128, 32


def graph(rng, n, degree, nstart=1):
    adj = np.zeros((n + nstart, degree + 1), np.uint32)
    for i in range(n + nstart):
        ln = int(rng.integers(degree // 2, degree + 1))
        adj[i, 0] = ln
        adj[i, 1:1 + ln] = rng.choice(n, ln, replace=False)
    return adj


def child():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import diskann_amd as da

    def say(text):
        os.write(2, f"== {text}\n".encode())

    def digest(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()[:16]

    def index(dtype, rng, **debug):
        if dtype == da.PQ:
            chunks = debug.pop("chunks")
            bounds = np.linspace(0, DIM, chunks + 1).round().astype(np.uint32)
            pivots = rng.standard_normal((256, DIM)).astype(np.float32)
            ix = da.Provider(da.PQ, da.L2, DIM, N, R, rng.integers(0, 256, (1, chunks), dtype=np.uint8), pq_pivots=pivots,
                             pq_offsets=bounds)
            ix.set_elements(0, rng.integers(0, 256, (N, chunks), dtype=np.uint8))
        else:
            data = (rng.integers(0, 256, (N, DIM), dtype=np.uint8) if dtype == da.U8
                    else rng.uniform(-1, 1, (N, DIM)).astype(np.float32))
            ix = da.Provider(dtype, da.L2, DIM, N, R, data[:1])
            ix.set_elements(0, data)
        ix.upload_graph(graph(rng, N, R))
        ix.debug_set(verbose=1, **debug)
        return ix

    def queries(dtype, rng, nq):
        return rng.integers(0, 256, (nq, DIM), dtype=np.uint8) if dtype == da.U8 else rng.uniform(-1, 1, (nq, DIM)).astype(np.float32)

    def run(name, ix, fn):
        for rep in ("prior", "calibrated"):
            out, fam = ix.last_family(fn)
            say(f"{name} [{rep}]: family {sorted(fam)} outputs {digest(*out)}")

    rng = np.random.default_rng(2024)
    ix = index(da.F32, rng)
    q48, q300 = queries(da.F32, rng, 48), queries(da.F32, rng, 300)
    run("f32 L2, 48 queries (team)", ix, lambda: ix.search(da.Knn(32, 1), q48, 10))
    ix.debug_set(tune_off=4)
    run("f32 L2, 48 queries, tune_off=4 (one wave, 32-bit)", ix, lambda: ix.search(da.Knn(32, 1), q48, 10))
    run("f32 L2, 300 queries, tune_off=4", ix, lambda: ix.search(da.Knn(40, 1), q300, 10))
    ix.set_visited_format(16)
    run("f32 L2, 300 queries, visited_format=16", ix, lambda: ix.search(da.Knn(48, 1), q300, 10))
    for fmt in (16, 32):
        ix.set_visited_format(fmt)
        ix.set_visited_bits(7)
        run(f"f32 L2, 300 queries, visited_bits=7 format {fmt}", ix, lambda: ix.search(da.Knn(26, 1), q300, 10))
    ix.set_visited_format(0)
    ix.set_visited_bits(0)
    ix.set_max_concurrency(128)
    run("f32 L2, 300 queries, max_concurrency 128 (persistent)", ix, lambda: ix.search(da.Knn(56, 1), q300, 10))
    ix.set_max_concurrency(0)
    match = rng.random(N + 1) < 0.5
    run("f32 L2, 300 queries, inline filter", ix, lambda: ix.filtered_search(da.Knn(30, 1), q300, 10, match))
    radius = 75.0  # a low percentile of the squared distances between uniform [-1, 1]^128 vectors (mean 85)
    run("f32 L2, 300 queries, range search", ix, lambda: ix.range_search(q300, 20, radius, 1, None, 1.0, 1.0, 0, out_cap=500))

    rng = np.random.default_rng(2025)
    for probes in (None, 3):
        ux = index(da.U8, rng, pair_min_queries=64, **({"ht16_max_probes": probes} if probes else {}))
        for nq, L in ((64, 26), (64, 64), (300, 26)):
            qu = queries(da.U8, rng, nq)
            run(f"u8 L2, {nq} queries paired, L={L}, ht16_max_probes={probes}", ux, lambda: ux.search(da.Knn(L, 1), qu, 10))
    for chunks in (16, 48):
        px = index(da.PQ, rng, chunks=chunks)
        for nq in (48, 300):
            qp = queries(da.F32, rng, nq)
            run(f"PQ {chunks} chunks, {nq} queries", px, lambda: px.search(da.Knn(32, 1), qp, 10))


def main():
    libs, outs = sys.argv[1:3], sys.argv[3:5]
    texts = []
    for lib, out in zip(libs, outs):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env={**os.environ, "DANN_LIB_PATH": os.path.abspath(lib)},
                           capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[dann]") or ln.startswith("== ")]
        open(out, "w").write("\n".join(lines) + "\n")
        print(f"{lib}: exit {r.returncode}, {len(lines)} lines -> {out}")
        if r.returncode != 0:
            print(r.stderr[-3000:])
            return 2  # nothing more is started on the GPU after a failed child
        texts.append(lines)
    same = texts[0] == texts[1]
    print("transcripts identical" if same else "TRANSCRIPTS DIFFER")
    for a, b in zip(*texts):
        if a != b:
            print("  A:", a, "\n  B:", b)
    return 0 if same and texts[0] else 1


if __name__ == "__main__":
    sys.exit(child() if sys.argv[1:] == ["--child"] else main())
