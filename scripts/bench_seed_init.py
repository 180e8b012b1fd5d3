#!/usr/bin/env python3
"""seed_gaussians on a 2.0 M-point synthetic surface cloud (the max_points of qed-init-pc): end to end and split into
index build, grid query, brute-force fallback and fill, by device events (median of 20 runs after 5 warm-up runs, and the
spread), the number of fallback queries, and cKDTree(x).query(x, 4, workers=16) on the same array where SciPy imports.

    python scripts/bench_seed_init.py [--points 2000000] [--runs 20] [--warmup 5] [--no-scipy] [--floaters 0]

``--floaters F`` replaces F of the points by uniform ones in a 200 m cube around the scene: far from everything, they are
still open after ``max_rings`` shells and go to the brute-force kernel.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pd_ref  # noqa: E402
from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd import seed_init as S  # noqa: E402
from qed_splatter_amd.pointcloud_metrics import DEFAULT_MAX_RINGS, NNIndex  # noqa: E402


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--max-rings", type=int, default=DEFAULT_MAX_RINGS)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--floaters", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lib = L.load()
    rng = np.random.default_rng(6)
    x_np = (pd_ref._surface(rng, a.points) + pd_ref.OFFSET).astype(np.float32)
    if a.floaters:
        x_np[:a.floaters] = (pd_ref.OFFSET + rng.uniform(-100.0, 100.0, size=(a.floaters, 3))).astype(np.float32)
    x_np = x_np[rng.permutation(a.points)]
    col = rng.integers(0, 256, size=(a.points, 3), dtype=np.uint8)
    x, c = torch.from_numpy(x_np).to(dev), torch.from_numpy(col).to(dev)
    n, k = a.points, a.k
    out = {"points": n, "floaters": a.floaters, "k": k, "max_rings": a.max_rings, "runs": a.runs, "warmup": a.warmup}
    out["seed_gaussians"] = timed(lambda: S.seed_gaussians(x, c, k=k, max_rings=a.max_rings), a.runs, a.warmup)
    out["index_build"] = timed(lambda: NNIndex(x, n), a.runs, a.warmup)
    index = NNIndex(x, n)
    dist = torch.empty(n, k, dtype=torch.float32, device=dev)
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    fb = torch.zeros(1 + n, dtype=torch.int32, device=dev)
    st = L.current_stream()
    query = lambda: L.check(lib.qed_knn_query(n, L.ptr(x), n, L.ptr(index.work), index.work.numel() * 8, n, k, a.max_rings,
                                              L.KNN_SKIP_FIRST, L.ptr(dist), L.ptr(idx), L.ptr(fb), st), "qed_knn_query")
    out["grid_query"] = timed(query, a.runs, a.warmup)
    out["fallback_queries"] = int(fb[0])
    brute = lambda: L.check(lib.qed_knn_brute(n, L.ptr(x), n, L.ptr(x), L.ptr(fb), k, L.KNN_SKIP_FIRST, L.ptr(dist),
                                              L.ptr(idx), st), "qed_knn_brute")
    out["fallback_brute"] = timed(brute, a.runs, a.warmup)
    g = S.seed_gaussians(x, c, k=k)
    status = torch.zeros(L.STATUS_WORDS, dtype=torch.int32, device=dev)
    fill = lambda: L.check(lib.qed_seed_gaussians(n, L.ptr(dist), k, L.ptr(c), 16, 0, 1e-7, 0, L.ptr(g["scales"]),
                                                  L.ptr(g["quats"]), L.ptr(g["opacities"]), L.ptr(g["features_dc"]),
                                                  L.ptr(g["features_rest"]), L.ptr(status), st), "qed_seed_gaussians")
    out["fill"] = timed(fill, a.runs, a.warmup)
    if a.no_scipy:
        out["ckdtree"] = "not run (--no-scipy)"
    else:
        try:
            from scipy.spatial import cKDTree
            x64 = x_np.astype(np.float64)
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                d_ref, _ = cKDTree(x64).query(x64, k + 1, workers=16)
                times.append((time.perf_counter() - t0) * 1e3)
            out["ckdtree"] = {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "runs": 3}
            err = np.abs(dist.cpu().numpy().astype(np.float64) - d_ref[:, 1:]) / np.maximum(d_ref[:, 1:], 1e-300)
            out["max_rel_error_vs_ckdtree"] = float(err.max())
        except ImportError:
            out["ckdtree"] = "SciPy does not import here"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
