#!/usr/bin/env python
"""What the camera pose optimiser costs a training step at config B (500 k Gaussians, one camera @ 1920x1080).

Three variants of train.Trainer.train_step's sequence (fused_loss -> backward_fused -> FlatAdam.step(fused_sh=True); no
densifier), each on its own copy of bench.py's scene, measured in ONE process, alternating, after a warm-up:

  a  no camera optimiser
  b  the fused camera optimiser: fused_loss(camera_optimizer=...) + CameraOptimizer.step_fused
  c  what could be done without it: a camera-to-world matrix that requires grad, made by the torch statements of
     tests/camera_opt_ref.py in float32 from a [1,6] parameter, through the same fused_loss (the pose then takes the eager
     get_viewmat chain and autograd's backward of it), stepped by torch.optim.Adam

    python scripts/bench_camera_opt.py [--rounds 5] [--steps 20] [--warmup 10]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_camera_opt.py --variant b --steps 20 --warmup 5

The first form prints ms per step per variant and round, the medians and one JSON line.  ``--variant X`` runs one variant
alone, for a kernel trace: the difference of two variants' kernel dispatch counts over the same number of steps is the
number of extra launches per step (the set-up is the same), and the trace's per-kernel averages split (b) - (a) into
qed_project_bwd's share (the view-matrix gradient: 12 wave-level atomics per wave) and the two pose launches.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(variant: str, args, dev):
    """(step function, model) of one variant on its own copy of the scene."""
    from bench import make_scene
    from qed_splatter_amd.camera_optimizer import CameraOptimizer, CameraOptimizerConfig
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from tests import camera_opt_ref as R
    sc = make_scene(args.gaussians, args.width, args.height, 0, dev)
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1)
    model = QEDSplatterModel(cfg, **{k: sc[k] for k in ("means", "scales", "quats", "opacities", "features_dc",
                                                         "features_rest")})
    model.step = 30000
    model.train()
    K = sc["Ks"][0].cpu()
    c2w0 = sc["camera_to_worlds"].contiguous()
    cam = PinholeCameras(c2w0, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), args.width, args.height,
                         metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"].contiguous(), "depth_image": sc["gt_depth"].contiguous()}
    opt = FlatAdam(model, means_schedule=FlatAdam.MEANS_SCHEDULE)
    count = [0]

    if variant == "a":
        def step():
            for p in model.parameters():
                p.grad = None
            losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0)
            model.backward_fused(losses)
            opt.step(fused_sh=True)
            count[0] += 1
    elif variant == "b":
        pose_opt = CameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), args.cameras, dev)

        def step():
            for p in model.parameters():
                p.grad = None
            losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0, camera_optimizer=pose_opt, cam_idx=0)
            model.backward_fused(losses)
            pose_opt.step_fused(2000 + count[0])
            opt.step(fused_sh=True)
            count[0] += 1
    elif variant == "c":
        pose = torch.zeros(args.cameras, 6, device=dev, requires_grad=True)
        adam = torch.optim.Adam([pose], lr=1e-4, eps=1e-15)

        def step():
            for p in model.parameters():
                p.grad = None
            adam.zero_grad(set_to_none=True)
            cam.camera_to_worlds = R.apply(c2w0, pose[0:1])
            losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0)
            (losses["loss"] + R.regularizer(pose)).backward()
            opt.step(fused_sh=True)
            adam.step()
            count[0] += 1
    else:
        raise SystemExit(f"unknown variant {variant!r}")
    return step, model


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--cameras", type=int, default=200, help="rows of pose_adjustment (training cameras)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--variant", choices=("a", "b", "c"), default=None, help="run this variant alone (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from qed_splatter_amd import _lib as L
    L.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    names = [args.variant] if args.variant else ["a", "b", "c"]
    steps = {v: build(v, args, dev)[0] for v in names}
    for v in names:
        for _ in range(args.warmup):
            steps[v]()
    torch.cuda.synchronize()
    if args.variant:
        for _ in range(args.steps):
            steps[args.variant]()
        torch.cuda.synchronize()
        print(json.dumps({"variant": args.variant, "steps": args.warmup + args.steps}))
        return
    ms = {v: [] for v in names}
    for r in range(args.rounds):
        for v in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                steps[v]()
            torch.cuda.synchronize()
            ms[v].append((time.perf_counter() - t0) / args.steps * 1e3)
        print(f"round {r}: " + ", ".join(f"({v}) {ms[v][-1]:.3f} ms/step" for v in names), flush=True)
    med = {v: statistics.median(ms[v]) for v in names}
    print(f"median ms/step: (a) {med['a']:.3f}  (b) {med['b']:.3f}  (c) {med['c']:.3f};  (b) - (a) = {med['b'] - med['a']:+.3f}, "
          f"(c) - (a) = {med['c'] - med['a']:+.3f}")
    print(json.dumps({"workload": f"{args.gaussians} Gaussians, 1 cam @ {args.width}x{args.height}, {args.cameras} pose rows",
                      "steps_per_round": args.steps, "ms_per_step": ms, "median_ms_per_step": med,
                      "b_minus_a_ms": med["b"] - med["a"], "c_minus_a_ms": med["c"] - med["a"]}))


if __name__ == "__main__":
    main()
