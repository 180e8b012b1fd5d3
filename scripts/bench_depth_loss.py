#!/usr/bin/env python
"""What the robust depth terms and the depth smoothness term cost a training step at config B (500 k Gaussians, one camera @
1920x1080).

Variants, each on its own copy of bench.py's scene, measured in ONE process, alternating, after a warm-up.  On the trainer's
route (fused_loss -> backward_fused -> FlatAdam.step(fused_sh=True); no densifier):

  a    the feature off (depth_loss_type "L1", depth_tv_lambda 0): the built-in depth term, the parent's launches
  m l h e    depth_loss_type "MSE" / "LogL1" / "HuberL1" / "EdgeAwareLogL1": K8 with depth_lambda = 0 and qed_depth_loss' two
       launches behind it
  lt et    "LogL1" / "EdgeAwareLogL1" with depth_tv_lambda 0.05 (edge-aware weights)

On the reference-shaped route (get_outputs -> get_loss_dict -> sum -> backward -> FlatAdam.step()):

  ga   the feature off
  gn   "EdgeAwareLogL1" with the smoothness term: the node (losses._DepthLoss)
  gt   the same two terms written as torch statements on outputs["depth"], the built-in term handed depth_lambda = 0 --
       the only way to get them before this feature

    python scripts/bench_depth_loss.py [--rounds 5] [--steps 20] [--warmup 8]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_depth_loss.py --variant et --steps 20 --warmup 5

The first form prints ms per step per variant and round, the medians and one JSON line.  ``--variant X`` runs one variant
alone, for a kernel trace in a run of its own.
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

TV_LAMBDA, DELTA = 0.05, 0.1
FUSED = {"a": {}, "m": dict(depth_loss_type="MSE"), "l": dict(depth_loss_type="LogL1"),
         "h": dict(depth_loss_type="HuberL1", depth_huber_delta=DELTA), "e": dict(depth_loss_type="EdgeAwareLogL1"),
         "lt": dict(depth_loss_type="LogL1", depth_tv_lambda=TV_LAMBDA),
         "et": dict(depth_loss_type="EdgeAwareLogL1", depth_tv_lambda=TV_LAMBDA)}
API = {"ga": {}, "gn": dict(depth_loss_type="EdgeAwareLogL1", depth_tv_lambda=TV_LAMBDA), "gt": dict(depth_lambda=0.0)}
NAMES = list(FUSED) + list(API)


def torch_terms(depth, alpha, gt_depth, image, depth_lambda):
    """depth_lambda * EdgeAwareLogL1 and TV_LAMBDA * the edge-aware smoothness term of include/qed_splat.h in torch statements
    on the [H,W,1] depth get_outputs returned (float32, no mask)."""
    H, W = depth.shape[:2]
    d, a, g = depth.reshape(H, W), alpha.reshape(H, W), gt_depth.reshape(H, W)
    gx, gy = torch.zeros_like(d), torch.zeros_like(d)
    gx[:, :-1] = (image[:, 1:] - image[:, :-1]).abs().mean(-1)
    gy[:-1, :] = (image[1:, :] - image[:-1, :]).abs().mean(-1)
    V = torch.isfinite(d) & torch.isfinite(g) & (g > 0)
    zero = torch.zeros_like(d)
    r = (torch.where(V, d, zero) - torch.where(V, g, zero)).abs()
    w = (torch.exp(-gx) + torch.exp(-gy)) * 0.5
    data = depth_lambda * torch.where(V, w * torch.log1p(r), zero).sum() / V.sum().clamp(min=1)
    ok = (a > 0) & torch.isfinite(d)
    ds = torch.where(ok, d, zero)
    px, py = ok[:, :-1] & ok[:, 1:], ok[:-1, :] & ok[1:, :]
    ex = torch.where(px, torch.exp(-gx[:, :-1]) * (ds[:, 1:] - ds[:, :-1]).abs(), zero[:, :-1]).sum() / px.sum().clamp(min=1)
    ey = torch.where(py, torch.exp(-gy[:-1, :]) * (ds[1:, :] - ds[:-1, :]).abs(), zero[:-1, :]).sum() / py.sum().clamp(min=1)
    return data, TV_LAMBDA * (ex + ey)


def build(variant: str, args, dev):
    """The step function of one variant on its own copy of the scene."""
    from bench import make_scene
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    sc = make_scene(args.gaussians, args.width, args.height, 0, dev)
    kw = FUSED[variant] if variant in FUSED else API[variant]
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1, graph_segments=False, **kw)
    model = QEDSplatterModel(cfg, **{k: sc[k] for k in ("means", "scales", "quats", "opacities", "features_dc",
                                                         "features_rest")})
    model.step = 30000
    model.train()
    K = sc["Ks"][0].cpu()
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    cam = PinholeCameras(sc["camera_to_worlds"].contiguous(), *intr, args.width, args.height, metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"].contiguous(), "depth_image": sc["gt_depth"].contiguous()}
    opt = FlatAdam(model, means_schedule=FlatAdam.MEANS_SCHEDULE)
    depth_lambda = QEDSplatterModelConfig.depth_lambda

    if variant in FUSED:
        def step():
            for p in model.parameters():
                p.grad = None
            losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0)
            model.backward_fused(losses)
            opt.step(fused_sh=True)
            return losses
        return step

    def step():
        for p in model.parameters():
            p.grad = None
        out = model.get_outputs(cam)
        losses = model.get_loss_dict(out, batch)
        if variant == "gt":
            losses["depth_loss"], losses["depth_tv_loss"] = torch_terms(out["depth"], out["accumulation"], batch["depth_image"],
                                                                        batch["image"], depth_lambda)
        sum(losses.values()).backward()
        opt.step()
        return losses
    return step


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--variant", choices=NAMES, default=None, help="run this variant alone (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from qed_splatter_amd import _lib as L
    L.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    names = [args.variant] if args.variant else NAMES
    steps = {v: build(v, args, dev) for v in names}
    last = {}
    for v in names:
        for _ in range(args.warmup):
            last[v] = steps[v]()
    torch.cuda.synchronize()
    if "gn" in last and "gt" in last:                         # (the first steps differ by the terms' rounding only)
        print("warm-up values: " + ", ".join(f"({v}) depth {float(last[v]['depth_loss']):.6f} tv "
                                             f"{float(last[v]['depth_tv_loss']):.6f}" for v in ("et", "gn", "gt")), flush=True)
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
        print(f"round {r}: " + ", ".join(f"({v}) {ms[v][-1]:.3f}" for v in names) + " ms/step", flush=True)
    med = {v: statistics.median(ms[v]) for v in names}
    print("median ms/step: " + "  ".join(f"({v}) {med[v]:.3f}" for v in names))
    print("ranges ms/step: " + "  ".join(f"({v}) {min(ms[v]):.3f}..{max(ms[v]):.3f}" for v in names))
    print(json.dumps({"workload": f"{args.gaussians} Gaussians, 1 cam @ {args.width}x{args.height}",
                      "steps_per_round": args.steps, "ms_per_step": ms, "median_ms_per_step": med,
                      "fused_minus_off_ms": {v: med[v] - med["a"] for v in FUSED if v != "a"},
                      "api_node_minus_off_ms": med["gn"] - med["ga"], "api_torch_minus_off_ms": med["gt"] - med["ga"]}))


if __name__ == "__main__":
    main()
