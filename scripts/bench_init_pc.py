#!/usr/bin/env python3
"""Timing of step 1 of qed-init-pc on the GPU (profiles/init_pc.txt).

(a) ``voxel_down_sample`` at 130 k (1080p at stride 4), 2 M and 4.1 M rows with voxel 0.03 and 0.05: the HIP kernel and
    the torch body it replaced on GPU tensors, alternating on the same tensors, event-timed after a warm-up; median and
    min..max of the repeats.
(b) step 1 end to end on a synthetic 1080p dataset held in memory (no file reading), with each implementation.

    python scripts/bench_init_pc.py [--frames 200] [--repeats 15] [--skip-e2e]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qed_splatter_amd import init_pointcloud as IP  # noqa: E402


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.array(ms)


def room_points(n, seed):
    """A 12 x 8 x 3 m room's worth of surface-like points."""
    rng = np.random.default_rng(seed)
    return rng.uniform((-6.0, -4.0, -1.5), (6.0, 4.0, 1.5), size=(n, 3)).astype(np.float32)


def bench_kernel(dev, repeats):
    print("voxel_down_sample: HIP kernel vs the torch body, ms (median, min..max)")
    for n in (129_600, 2_073_600, 4_100_000):
        pts = torch.from_numpy(room_points(n, n % 97)).to(dev)
        for v in (0.03, 0.05):
            a = timed(lambda: IP.voxel_down_sample(pts, v), repeats)
            b = timed(lambda: IP._voxel_down_sample_torch(pts, v), repeats)
            a2 = timed(lambda: IP.voxel_down_sample(pts, v), repeats)          # again, after the other: the spread between runs
            rows = int(IP.voxel_down_sample(pts, v).shape[0])
            print(f"  n={n:>9} v={v}: {rows:>8} voxels | hip {np.median(a):8.3f} ({a.min():.3f}..{a.max():.3f}) "
                  f"again {np.median(a2):8.3f} | torch {np.median(b):8.3f} ({b.min():.3f}..{b.max():.3f}) | "
                  f"torch / hip {np.median(b) / np.median(a):.2f}", flush=True)


def bench_e2e(dev, n_frames):
    h, w = 1080, 1920
    rng = np.random.default_rng(0)
    base = rng.uniform(2.5, 3.5, size=(h, w)).astype(np.float32)
    poses = []
    for i in range(n_frames):
        yaw = 2 * np.pi * i / n_frames
        c, s = np.cos(yaw), np.sin(yaw)
        c2w = np.eye(4)
        c2w[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        poses.append(torch.from_numpy(c2w))
    depth = torch.from_numpy(base).to(dev)

    def run(down_sample_fn, stride=4):
        def clouds():
            for c2w in poses:
                cloud = IP.backproject_depth(depth, 1000.0, 1000.0, w / 2, h / 2, c2w, depth_max=100.0, stride=stride)
                yield down_sample_fn(cloud, 0.05)
        merged = IP.tree_merge_pointclouds(clouds(), 0.03, 2_000_000, down_sample_fn)
        return down_sample_fn(merged, 0.05)
    print(f"step 1 end to end, {n_frames} frames of 1080p in memory, stride 4, default voxel sizes (host seconds around a synchronise)")
    for name, fn in (("hip", IP.voxel_down_sample), ("torch", IP._voxel_down_sample_torch), ("hip", IP.voxel_down_sample)):
        run(fn)                                                                  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(fn)
        torch.cuda.synchronize()
        print(f"  {name:5s}: {time.perf_counter() - t0:7.3f} s, {int(out.shape[0])} points", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_init_pc.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    bench_kernel(dev, args.repeats)
    if not args.skip_e2e:
        bench_e2e(dev, args.frames)


if __name__ == "__main__":
    main()
