#!/usr/bin/env python3
"""PDMetrics on one MI355X at the size the project trains: two synthetic surface clouds of 2.0 M (prediction: 2 cm noise,
0.5 % floaters) and 1.5 M points (tests/pd_ref.py's generator).

    python scripts/bench_pd_metrics.py [--n-pred 2000000 --n-gt 1500000 --repeats 5] [--no-scipy] [--profile]

Prints, as JSON lines: PDMetrics.forward by device events after a warm-up (median, min, max); the split of one direction
into index build, grid query and brute-force fallback for several max_rings, with the queries in the order of their cell
and in row order; and, where SciPy is importable, the reference's two cKDTree build-and-query calls on the same arrays
(host seconds).  --profile: one warm-up and one forward only, for `rocprofv3 --kernel-trace --stats -- python ...`.
Recorded in profiles/pd_metrics.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import pd_ref as R  # noqa: E402
from qed_splatter_amd import pointcloud_metrics as PM  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def split(q, t, max_rings, natural_order):
    """ms of the index build, the grid query and the brute-force fallback of one direction (events between the calls)."""
    lib = PM.L.load()
    ms_build, index = timed(lambda: PM.NNIndex(t, len(q)))
    nq = len(q)
    dist = torch.empty(nq, dtype=torch.float32, device=q.device)
    idx = torch.empty(nq, dtype=torch.int32, device=q.device)
    fb = torch.zeros(1 + nq, dtype=torch.int32, device=q.device)
    ws = torch.empty(nq, dtype=torch.int64, device=q.device)
    st = PM.L.current_stream()
    ms_grid, _ = timed(lambda: PM.L.check(lib.qed_nn_query(
        nq, q.data_ptr(), index.n, index.work.data_ptr(), index.work.numel() * 8, index.capacity, max_rings,
        PM.L.NN_NATURAL_ORDER if natural_order else 0, dist.data_ptr(), idx.data_ptr(), fb.data_ptr(), st), "qed_nn_query"))
    ms_brute, _ = timed(lambda: PM.L.check(lib.qed_nn_brute(
        nq, q.data_ptr(), index.n, t.data_ptr(), fb.data_ptr(), dist.data_ptr(), idx.data_ptr(), ws.data_ptr(),
        ws.numel() * 8, st), "qed_nn_brute"))
    return {"build_ms": round(ms_build, 3), "grid_ms": round(ms_grid, 3), "brute_ms": round(ms_brute, 3),
            "fallback": int(fb[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-pred", type=int, default=2_000_000)
    ap.add_argument("--n-gt", type=int, default=1_500_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pd_metrics.py measures on the GPU: there is no CPU path"
    pred_np, gt_np = R.kat_clouds(args.n_pred, args.n_gt, seed=6)
    pred, gt = torch.from_numpy(pred_np).cuda(), torch.from_numpy(gt_np).cuda()
    m = PM.PDMetrics()
    acc, cmp_ = m(pred, gt)                                     # warm-up: code objects, the allocator's pools
    if args.profile:
        print(json.dumps({"what": "profile run", "accuracy": acc, "completeness": cmp_, **m.last}), flush=True)
        m(pred, gt)
        torch.cuda.synchronize()
        return
    ms = sorted(timed(lambda: m(pred, gt))[0] for _ in range(args.repeats))
    print(json.dumps({"what": "PDMetrics.forward", "n_pred": args.n_pred, "n_gt": args.n_gt, "ms_median": round(ms[len(ms) // 2], 3),
                      "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3), "repeats": args.repeats,
                      "max_rings": PM.DEFAULT_MAX_RINGS, "accuracy": acc, "completeness": cmp_, **m.last}), flush=True)
    for name, q, t in (("pred->gt", pred, gt), ("gt->pred", gt, pred)):
        for rings, natural in ((2, False), (4, False), (8, False), (8, True), (16, False)):
            split(q, t, rings, natural)
            print(json.dumps({"what": "split", "direction": name, "max_rings": rings,
                              "query_order": "rows" if natural else "cells", **split(q, t, rings, natural)}), flush=True)
    if not args.no_scipy:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            print(json.dumps({"what": "cKDTree", "skipped": "SciPy is not importable here"}))
            return
        t0 = time.perf_counter()
        d_pg = cKDTree(gt_np).query(pred_np)[0]
        t1 = time.perf_counter()
        d_gp = cKDTree(pred_np).query(gt_np)[0]
        t2 = time.perf_counter()
        print(json.dumps({"what": "cKDTree (host, one core)", "accuracy_s": round(t1 - t0, 3), "completeness_s": round(t2 - t1, 3),
                          "accuracy": float(np.percentile(d_pg, 90)),
                          "completeness": float(np.sum(d_gp < 0.05) / len(d_gp) * 100)}), flush=True)


if __name__ == "__main__":
    main()
