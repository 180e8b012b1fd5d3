#!/usr/bin/env python3
"""Rendering a trained model to files at config B's synthetic scene (500 k Gaussians, 1920x1080), three questions:

1. What do the two launches of csrc/present.hip (qed_present_range + qed_present_frame, all four planes) cost on the
   device, beside the same planes made with torch ops on the same tensors (clamp / mul / floor / to(uint8), a table
   gather, a masked amin / amax) -- the only route the package offered before.  Both are captured into a hipGraph of
   ``--graph-frames`` frames and replayed, so the figure is device time without the host's launch work; the frames are
   distinct rendered views, enough of them to exceed the 256 MiB Infinity Cache (in use the planes were written by the
   render just before and are warmer than this).  The outputs of the two routes are compared before anything is timed.
2. End-to-end frames per second of render_frames + FrameWriter to a memory-backed directory with 8 and 16 encoder
   threads (and, for 16, a deeper ring of pinned buffers), beside a loop that makes the planes with torch, calls .cpu() per plane and writes with PIL serially.
3. Where the time of a frame goes: render, finish (device events), device-to-host copy (timed on its own), encode
   (summed worker seconds per frame).

    python scripts/bench_render.py [--gaussians 500000 --width 1920 --height 1080 --frames 48] [--out profiles/render.txt]
"""
import argparse
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd import render  # noqa: E402
from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig  # noqa: E402
from qed_splatter_amd.scene import synthetic_scene  # noqa: E402

NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
DEPTH_UNIT = 0.001
HBM_COPY_TBS = 5.42          # profiles/r01_hbm_copy_bench.txt: copy 1 GiB -> 1 GiB, read + write


def torch_planes(rgb, depth, alpha, inv_unit, lut_f):
    """The four planes with torch ops (rounding half up as the kernel does; products and sums rounded separately)."""
    d, a = depth[..., 0], alpha[..., 0]
    rgb8 = (rgb.clamp(0, 1) * 255 + 0.5).floor().to(torch.uint8)
    a8 = (a.clamp(0, 1) * 255 + 0.5).floor().to(torch.uint8)
    valid = (a > 0) & torch.isfinite(d) & (d > 0)
    d16 = torch.where(valid, (d * inv_unit + 0.5).floor().clamp(max=65535), 0.0).to(torch.int32).to(torch.uint16)
    lo = torch.where(valid, d, float("inf")).amin()
    hi = torch.where(valid, d, float("-inf")).amax()
    t = ((d - lo) * (1.0 / (hi - lo))).clamp(0, 1)
    k = (t * 255).to(torch.int64).clamp(max=255)
    c = a.clamp(0, 1)[..., None] * (lut_f[k] - 255) + 255
    dm = torch.where(valid[..., None], (c + 0.5).floor(), 255.0).to(torch.uint8)
    return {"rgb": rgb8, "depth16": d16, "depthmap": dm, "alpha": a8}


def replay_ms(fn, n_frames, rounds=5, replays=20):
    """Device time per frame of fn(i), i = 0 .. n_frames - 1, captured into one graph; median over ``rounds`` windows of
    ``replays`` replays each."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(n_frames):
            fn(i)                                   # warm-up: code objects, allocator
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(graph):
        for i in range(n_frames):
            keep.append(fn(i))
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / (replays * n_frames))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=48, help="frames of every end-to-end run")
    ap.add_argument("--graph-frames", type=int, default=8, help="distinct frames of the device-time graphs")
    ap.add_argument("--serial-frames", type=int, default=8, help="frames of the serial torch + PIL loop")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py measures on the GPU; none found")
    L.load()
    dev = torch.device("cuda:0")
    W, H, n = args.width, args.height, args.gaussians
    sc = synthetic_scene(n, W, H, seed=1235)
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1),
                             **{k: sc[k].to(dev) for k in NAMES})
    model.step = 10_000
    model.eval()
    K = sc["Ks"][0]
    cams = []
    for k in range(args.frames):                   # a slow pan of +-6 degrees about the scene's camera: every view is full
        a = math.radians(12.0 * k / max(args.frames - 1, 1) - 6.0)
        c2w = torch.tensor([[[math.cos(a), 0.0, math.sin(a), 0.0], [0.0, 1.0, 0.0, 0.0], [-math.sin(a), 0.0, math.cos(a), 0.0]]])
        cams.append(PinholeCameras(c2w.to(dev), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), W, H))
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# rendering to files: {n} Gaussians, {W}x{H}, synthetic scene (seed 1235), {args.frames} views panning over 12 degrees")
    say(f"# commit {commit or '(not a git checkout)'}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}; "
        f"{len(os.sched_getaffinity(0))} CPUs available to this process")

    # ---- 1. the two launches against torch ops, device time
    G = args.graph_frames
    with torch.no_grad():
        outs = []
        for k in range(G):
            o = model.get_outputs(cams[k])
            outs.append({key: o[key].clone() for key in ("rgb", "depth", "accumulation")})
    lut_f = torch.from_numpy(render.colormap("turbo")).to(dev).float()
    inv_unit = float(np.float32(1.0 / DEPTH_UNIT))
    ours = lambda i: render.present_frame(outs[i], depth_unit=DEPTH_UNIT)                                    # noqa: E731
    eager = lambda i: torch_planes(outs[i]["rgb"], outs[i]["depth"], outs[i]["accumulation"], inv_unit, lut_f)  # noqa: E731
    a, b = ours(0), eager(0)
    for p in render.PLANES:
        diff = (a[p].to(torch.int32) - b[p].to(torch.int32)).abs()
        frac = float((diff != 0).float().mean())
        say(f"# {p}: kernel against torch ops, largest difference {int(diff.max())} step(s), {100 * frac:.4f} % of values differ "
            "(one rounding in the kernel's fmaf, two in torch's mul + add)")
        assert int(diff.max()) <= 1 and frac < 0.01, p
    px = H * W
    moved = px * (20 + 9) + px * 8                 # present_frame: 20 B in, 9 out per pixel; present_range: depth + alpha again
    t_k = replay_ms(ours, G)
    t_t = replay_ms(eager, G)
    mk, mt = t_k[len(t_k) // 2], t_t[len(t_t) // 2]
    say("# 1. device time per frame, all four planes (hipGraph replay of %d distinct frames, median of 5 windows of %d frames; min .. max)" % (G, 20 * G))
    say(f"present.hip, two launches    {mk * 1e3:8.1f} us ({t_k[0] * 1e3:.1f} .. {t_k[-1] * 1e3:.1f})   {moved / 1e6:.1f} MB moved, "
        f"{moved / (mk * 1e-3) / 1e12:.2f} TB/s = {100 * moved / (mk * 1e-3) / 1e12 / HBM_COPY_TBS:.0f} % of the {HBM_COPY_TBS} TB/s copy rate")
    say(f"torch ops                    {mt * 1e3:8.1f} us ({t_t[0] * 1e3:.1f} .. {t_t[-1] * 1e3:.1f})   {mt / mk:.1f} x the two launches")

    # ---- 3a. the frame itself and the copy, on their own
    with torch.no_grad():
        for k in range(4):
            model.get_outputs(cams[k])
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.frames + 1)]
        ev[0].record()
        for k in range(args.frames):
            model.get_outputs(cams[k])
            ev[k + 1].record()
        torch.cuda.synchronize()
    t_render = sorted(ev[k].elapsed_time(ev[k + 1]) for k in range(args.frames))
    planes = ours(0)
    pinned = {p: torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for p, t in planes.items()}
    t_copy = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for p, t in planes.items():
            pinned[p].copy_(t, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        t_copy.append(e0.elapsed_time(e1))
    t_copy = sorted(t_copy)[5:]
    out_bytes = sum(t.numel() * t.element_size() for t in planes.values())

    # ---- 2. end to end
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="qed_render_bench_", dir=base)
    results = {}
    try:
        say(f"# 2. end to end, {args.frames} frames, four PNG planes each (compress level 1), into {'a tmpfs' if base else 'a temporary'} directory")
        for workers, slots in ((8, 3), (16, 3), (16, 8)) * 2:      # alternating; the first round also warms the allocator
            out_dir = os.path.join(tmp, f"w{workers}_{slots}")
            shutil.rmtree(out_dir, ignore_errors=True)
            timings = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with render.FrameWriter(out_dir, n_workers=workers, n_slots=slots) as writer:
                t_sub0 = time.perf_counter()
                render.render_frames(model, cams, writer, depth_unit=DEPTH_UNIT, timings=timings)
                t_submitted = time.perf_counter() - t_sub0
            elapsed = time.perf_counter() - t0
            fin = sorted(a_.elapsed_time(b_) for a_, b_ in timings["finish"])
            results[(workers, slots)] = dict(fps=args.frames / elapsed, bytes=writer.bytes_written, encode_s=writer.encode_seconds,
                                             submitted_s=t_submitted, finish_ms=fin[len(fin) // 2])
            say(f"render_frames, {workers:2d} workers, {slots} slots   {args.frames / elapsed:7.1f} frames/s   ({elapsed:.2f} s; the render "
                f"loop had submitted everything after {t_submitted:.2f} s; {writer.bytes_written / 1e6:.0f} MB written; "
                f"{writer.encode_seconds / args.frames * 1e3:.0f} ms of encoder thread time per frame)")
        # the serial loop: torch planes, .cpu() per plane, PIL
        from PIL import Image
        ser_dir = os.path.join(tmp, "serial")
        for sub in render.PLANE_DIRS.values():
            os.makedirs(os.path.join(ser_dir, sub))
        ns = args.serial_frames
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for k in range(ns):
                o = model.get_outputs(cams[k])
                pl = torch_planes(o["rgb"], o["depth"], o["accumulation"], inv_unit, lut_f)
                for p, t in pl.items():
                    Image.fromarray(t.cpu().numpy()).save(os.path.join(ser_dir, render.PLANE_DIRS[p], f"{k:05d}.png"),
                                                          compress_level=1)
        ser = time.perf_counter() - t0
        say(f"torch planes, .cpu(), PIL     {ns / ser:7.1f} frames/s   ({ser:.2f} s for {ns} frames, serial)")
        best = max(r["fps"] for r in results.values())
        say(f"# render_frames is {best / (ns / ser):.1f} x the serial loop")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    # ---- 3. where the time goes
    r16, r8 = results[(16, 8)], results[(8, 3)]
    say("# 3. one frame: where the time goes")
    say(f"render (get_outputs, eval)   {t_render[len(t_render) // 2]:8.3f} ms device events, median of {args.frames} (the call's host work included)")
    say(f"finish (two launches)        {mk:8.3f} ms device (section 1); {r16['finish_ms']:.3f} ms between events in the loop, host work included")
    say(f"copy to pinned memory        {t_copy[len(t_copy) // 2]:8.3f} ms for {out_bytes / 1e6:.1f} MB = {out_bytes / (t_copy[len(t_copy) // 2] * 1e-3) / 1e9:.1f} GB/s, on a side stream beside the next render")
    say(f"encode + write (PNG)         {r16['encode_s'] / args.frames * 1e3:8.1f} ms of one thread per frame; over 16 threads that allows at most "
        f"{16 / (r16['encode_s'] / args.frames):.0f} frames/s, over 8 at most {8 / (r8['encode_s'] / args.frames):.0f}")
    say("# (a slot is held until the slowest of its frame's four files is written, so a ring of 3 slots keeps at most 12 encoder "
        "jobs in flight and 3 / (the longest file's time) frames/s; more slots let 16 threads work)")
    print(json.dumps({"present_us": mk * 1e3, "torch_us": mt * 1e3, "fps_8w_3s": results[(8, 3)]["fps"], "fps_16w_3s": results[(16, 3)]["fps"], "fps_16w_8s": results[(16, 8)]["fps"],
                      "serial_fps": ns / ser}))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
