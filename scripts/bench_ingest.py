#!/usr/bin/env python3
"""The per-step ground truth at 1920x1080: the one launch of csrc/ingest.hip (QEDSplatterModel._ground_truth on a
datamanager.GpuBatch) against the eager chain the same method runs on the equivalent plain dict (.float(), / 255, the
box-filter conv2d, the composite, .contiguous(), and again for depth and mask) -- what a trainer that hands the model a
new uint8 frame every step paid before.  Every call reads ANOTHER cached frame, round robin over enough frames to exceed
the 256 MiB Infinity Cache, as a trainer's steps do; the outputs are fresh allocations, which the caching allocator hands
back from a few recycled blocks.  Device events around every call, after warm-up, the two routes alternating; the outputs
are compared before anything is timed.  Its output is the first section of profiles/ingest.txt (the kernel times below
it there come from a rocprofv3 kernel trace of this script, a run of its own).

    python scripts/bench_ingest.py [--height 1080 --width 1920 --iters 100 --frames 24] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from qed_splatter_amd.datamanager import GpuBatch  # noqa: E402
from qed_splatter_amd.model import QEDSplatterModel, QEDSplatterModelConfig  # noqa: E402
from qed_splatter_amd.scene import synthetic_scene  # noqa: E402

DEPTH_SCALE = 0.001 * 0.37


def timed(fn, iters, warmup=10):
    """fn(i) for i = 0 .. : the caller's fn picks frame i mod its number of frames"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn(warmup + i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))


def stats(ms):
    n = len(ms)
    return {"median": ms[n // 2], "p10": ms[n // 10], "p90": ms[(9 * n) // 10]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--frames", type=int, default=24, help="distinct cached frames the calls rotate through")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    torch.manual_seed(0)
    N = args.frames
    bg = torch.rand(3, device=dev)

    def make_frames(kind):
        """N distinct frames made on the device: (GpuBatch, the equivalent plain dict) pairs"""
        out = []
        for _ in range(N):
            if kind == "rgb":
                gb = GpuBatch(image=torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev),
                              depth_image=(0.5 + 11.5 * torch.rand(H, W, 1, device=dev)) * (torch.rand(H, W, 1, device=dev) >= 0.1),
                              image_idx=0, depth_scale=1.0)
            else:
                gb = GpuBatch(image=torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, device=dev),
                              depth_image=torch.randint(0, 65536, (H, W, 1), dtype=torch.int32).to(torch.uint16).to(dev),
                              mask=torch.rand(H, W, 1, device=dev) < 0.7, image_idx=0, depth_scale=DEPTH_SCALE)
            plain = {k: gb[k] for k in gb if k != "depth_scale"}          # (depth as float32 metres: gb[...] converts)
            gb.__dict__.pop("_f32", None)                                 # (the batch itself keeps no converted depth)
            out.append((gb, plain))
        return out

    sc = synthetic_scene(100, W, H, seed=1)
    model = QEDSplatterModel(QEDSplatterModelConfig(num_downscales=2, resolution_schedule=3000),
                             **{k: sc[k].to(dev) for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")})
    model.train()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# ground truth of one {W}x{H} frame per step: one launch (GpuBatch) against the eager chain (plain dict)")
    say(f"# commit {commit or '(not a git checkout)'}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}; "
        f"{args.iters} calls per round after 10 warm-up calls, three alternating rounds, device events around each call")
    say(f"# every call reads another of {N} cached frames ({N} x the input bytes of a case exceed the 256 MiB Infinity Cache); "
        "the outputs are fresh allocations from the caching allocator's recycled blocks")
    say("# bytes = inputs read once + outputs written once (what the one launch must move); GB/s = bytes over the CALL's "
        "time, host work included -- not a kernel's rate")
    say("# case                        d   MB moved   launch ms  median (p10 .. p90)   GB/s over the call    eager ms median (p10 .. p90)   eager / launch")
    cases = [("uint8 RGB + float32 depth", "rgb", d) for d in (1, 2, 4)] + [("uint8 RGBA + uint16 depth + mask", "rgba", 1)]
    results, made = [], {}
    for name, kind, d in cases:
        model.step = {4: 0, 2: 3000, 1: 6000}[d]
        assert model._get_downscale_factor() == d
        Ho, Wo = H // d, W // d
        if kind not in made:
            made.clear()                                               # (one kind's frames at a time)
            made[kind] = make_frames(kind)
        frames = made[kind]
        image, dep, msk = frames[0][0].raw("image"), frames[0][0].raw("depth_image"), frames[0][0].get("mask")
        fused = lambda i: model._ground_truth(frames[i % N][0], bg, Ho, Wo)        # noqa: E731
        eager = lambda i: model._ground_truth(frames[i % N][1], bg, Ho, Wo)        # noqa: E731
        for a, b in zip(fused(0), eager(0)):                           # the same images, before anything is timed
            if a is not None:
                err = float((a.reshape(-1) - b.reshape(-1)).abs().max() / b.abs().max().clamp_min(1e-30))
                assert err <= 1e-5, (name, d, err)
        # (a float32 depth map at d = 1 is its own ground truth on both routes: neither copies it)
        planes = [image, msk] + ([] if d == 1 and dep.dtype == torch.float32 else [dep])
        moved = sum(t.numel() * t.element_size() for t in planes if t is not None) \
            + Ho * Wo * 4 * (3 + (len(planes) - 2) + (1 if msk is not None else 0))
        t_f, t_e = [], []
        for _ in range(3):
            t_f += timed(fused, args.iters)
            t_e += timed(eager, args.iters)
        f, e = stats(sorted(t_f)), stats(sorted(t_e))
        rate = moved / (f["median"] * 1e-3)
        say(f"{name:32s} {d}   {moved / 1e6:7.2f}   {f['median']:.4f} ({f['p10']:.4f} .. {f['p90']:.4f})   "
            f"{rate / 1e9:7.1f}              {e['median']:.4f} ({e['p10']:.4f} .. {e['p90']:.4f})   "
            f"{e['median'] / f['median']:.2f} x")
        results.append({"case": name, "d": d, "bytes": moved, "launch_ms": f["median"], "eager_ms": e["median"]})
    say("# (the launch column is the whole Python call: qualification of the batch, two or three allocations, one kernel; a "
        "call shorter than ~20 us is bounded by that host work, not by the kernel)")
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
