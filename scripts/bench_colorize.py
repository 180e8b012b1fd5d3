#!/usr/bin/env python3
"""qed_colorize_accumulate at 2 M points and 1080p frames: HIP-event time per frame at batch_frames 1, 4, 8 and 16
(20 warm-up + 100 timed launches; median, p10, p90), the realised hit rate, the (point, frame) pairs per second, and
the NumPy restatement (tests/colorize_ref.py: the reference's arithmetic) on the host as the baseline.

    python scripts/bench_colorize.py [--points 2000000] [--out profiles/colorize_1080p.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import colorize_ref as R  # noqa: E402
from qed_splatter_amd import init_pointcloud as IP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--numpy-frames", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    H, W = 1080, 1920
    dev = torch.device("cuda:0")
    scene = R.build_scene(n_frames=a.frames, h=H, w=W, n_points=a.points, seed=9, special_frames=False)
    frames = scene["frames"]
    lines = [f"colourise: {a.points} points, {a.frames} frames of {W}x{H}, {torch.cuda.get_device_name(0)}",
             f"HIP events, {a.warmup} warm-up + {a.iters} timed launches of qed_colorize_accumulate per batch size"]

    pts = torch.from_numpy(scene["points"]).to(dev)
    depth = torch.from_numpy(np.stack([f["depth_raw"] for f in frames])).to(dev)
    color = torch.from_numpy(np.stack([f["color"] for f in frames])).to(dev)
    c2w = np.stack([f["c2w"] for f in frames])
    intr = np.array([f["intr"] for f in frames])

    pc = IP.PointColorizer(pts)
    pc.add_frames(depth, color, c2w, intr)
    torch.cuda.synchronize()
    hits = int(pc.color_count.sum())
    n_colored = pc.finalize()[1]
    pairs = a.points * a.frames
    lines.append(f"hit rate: {hits} hits of {pairs} (point, frame) pairs = {hits / pairs:.4f}; "
                 f"{n_colored} of {a.points} points coloured")
    lines.append("batch_frames   ms/launch (median)   ms/frame median [p10, p90]   G pairs/s")
    for B in (1, 4, 8, 16):
        if B > a.frames:
            continue
        pc = IP.PointColorizer(pts)
        ms = []
        for it in range(a.warmup + a.iters):
            f0 = (it * B) % (a.frames - B + 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pc.add_frames(depth[f0:f0 + B], color[f0:f0 + B], c2w[f0:f0 + B], intr[f0:f0 + B])
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        ms = np.array(ms)
        med, p10, p90 = np.median(ms), np.percentile(ms, 10), np.percentile(ms, 90)
        lines.append(f"{B:12d}   {med:18.4f}   {med / B:8.4f} [{p10 / B:.4f}, {p90 / B:.4f}]   "
                     f"{a.points * B / (med * 1e-3) / 1e9:9.2f}")
        print(lines[-1], flush=True)

    # upload of one frame's depth + colour from pageable host memory (what the tool does per frame besides decoding)
    d_h, c_h = frames[0]["depth_raw"], frames[0]["color"]
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(10):
        torch.from_numpy(d_h).to(dev)
        torch.from_numpy(c_h).to(dev)
    torch.cuda.synchronize()
    lines.append(f"upload of one frame (8.3 MB depth + 6.2 MB colour, pageable): {(time.perf_counter() - t) / 10 * 1e3:.3f} ms")

    # decoding one frame as the tool does: a 16-bit depth PNG and an RGB PNG of a rendered-like (smooth) image
    import io
    from PIL import Image
    vs, us = np.mgrid[0:H, 0:W]
    smooth = np.stack([(us // 8) % 256, (vs // 4) % 256, ((us + vs) // 16) % 256], -1).astype(np.uint8)
    bufs = []
    for img in (Image.fromarray(np.clip(np.nan_to_num(d_h), 0, 65535).astype(np.uint16)), Image.fromarray(smooth)):
        b = io.BytesIO()
        img.save(b, format="PNG")
        bufs.append(b.getvalue())
    t = time.perf_counter()
    for _ in range(5):
        np.array(Image.open(io.BytesIO(bufs[0])), dtype=np.float32)
        np.array(Image.open(io.BytesIO(bufs[1])).convert("RGB"), dtype=np.uint8)
    lines.append(f"PNG decode of one frame on one host thread (16-bit depth + RGB): {(time.perf_counter() - t) / 5 * 1e3:.1f} ms")

    nf = min(a.numpy_frames, a.frames)
    t = time.perf_counter()
    R.colorize_fp32(scene["points"], frames[:nf])
    dt = time.perf_counter() - t
    lines.append(f"NumPy restatement on the host ({os.environ.get('OMP_NUM_THREADS', '?')} threads), arrays already in "
                 f"memory: {dt / nf * 1e3:.1f} ms/frame over {nf} frames")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
