#!/usr/bin/env python
"""What the normal consistency and smoothness terms cost a training step at config B (500 k Gaussians, one camera @ 1920x1080).

Three variants of train.Trainer.train_step's sequence (fused_loss -> backward_fused -> FlatAdam.step(fused_sh=True); no
densifier), each on its own copy of bench.py's scene, measured in ONE process, alternating, after a warm-up:

  a  both terms off
  b  config.use_normal_consistency and config.use_normal_tv on (normals.py: qed_gaussian_normals, one 4-channel compositing
     forward and backward on the colour pass's lists, qed_normal_consistency's reduce and gradient passes,
     qed_normal_rows_merge_depth, qed_gaussian_normals_bwd)
  c  the same loss made the only way available before: the accumulated normal by accumulated_normals (3 channels), the
     stencil, both terms and their means in torch statements (float64, as the definition asks) with autograd over
     ``render`` / ``alpha``, whose gradient the colour pass's compositing backward then adds to its own

    python scripts/bench_normal_consistency.py [--rounds 5] [--steps 20] [--warmup 10]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_normal_consistency.py --variant b --steps 20 --warmup 5

The first form prints ms per step per variant and round, the medians and one JSON line.  ``--variant X`` runs one variant
alone, for a kernel trace: the difference of two variants' kernel dispatch counts over the same number of steps is the number
of extra launches per step, and the trace's per-kernel averages give the new kernels' times.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAM_C, LAM_TV, MIN_ALPHA = 0.05, 0.1, 0.5


def torch_terms(A, alpha, D, intr, mask=None):
    """lambda_c * consistency + lambda_tv * smoothness of include/qed_splat.h in torch statements: A [H,W,3], alpha [H,W],
    D [H,W] float32 with graphs; the stencil in float64."""
    fx, fy, cx, cy = intr
    H, W = alpha.shape
    ln = A.norm(dim=-1)
    ok_n = (alpha >= MIN_ALPHA) & (ln > 1e-8)
    if mask is not None:
        ok_n = ok_n & (mask.reshape(H, W) != 0)
    n = (A / ln.clamp(min=1e-8)[..., None]).double()
    ok_z = alpha >= MIN_ALPHA
    z = D.double() / torch.where(ok_z, alpha, torch.ones_like(alpha)).double()
    ok_z = ok_z & torch.isfinite(z) & (z > 0)
    z = torch.where(ok_z, z, torch.ones_like(z))
    xs = torch.arange(W, dtype=torch.float64, device=A.device)[None, :]
    ys = torch.arange(H, dtype=torch.float64, device=A.device)[:, None]
    P = torch.stack([(xs + 0.5 - cx) / fx * z, (ys + 0.5 - cy) / fy * z, z], dim=-1)
    dx = P[1:-1, 2:] - P[1:-1, :-2]
    dy = P[2:, 1:-1] - P[:-2, 1:-1]
    cr = torch.linalg.cross(dy, dx, dim=-1)
    cl = cr.norm(dim=-1)
    Vc = ok_z[1:-1, 1:-1] & ok_z[1:-1, 2:] & ok_z[1:-1, :-2] & ok_z[2:, 1:-1] & ok_z[:-2, 1:-1] & (cl > 1e-20) \
        & ok_n[1:-1, 1:-1]
    N = cr / torch.where(Vc, cl, torch.ones_like(cl))[..., None]
    loss_c = ((1.0 - (n[1:-1, 1:-1] * N).sum(-1)) * Vc).sum() / Vc.sum().clamp(min=1)
    Ex, Ey = ok_n[:, :-1] & ok_n[:, 1:], ok_n[:-1, :] & ok_n[1:, :]
    tv_x = ((n[:, 1:] - n[:, :-1]).abs().sum(-1) * Ex).sum() / (3 * Ex.sum().clamp(min=1))
    tv_y = ((n[1:, :] - n[:-1, :]).abs().sum(-1) * Ey).sum() / (3 * Ey.sum().clamp(min=1))
    return (LAM_C * loss_c).float(), (LAM_TV * (tv_x + tv_y)).float()


def build(variant: str, args, dev):
    """(step function, model) of one variant on its own copy of the scene."""
    from bench import make_scene
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.normals import accumulated_normals
    sc = make_scene(args.gaussians, args.width, args.height, 0, dev)
    on = variant in ("b", "c")
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1, use_normal_consistency=on, use_normal_tv=on,
                                           normal_consistency_lambda=LAM_C, normal_tv_lambda=LAM_TV)
    model = QEDSplatterModel(cfg, **{k: sc[k] for k in ("means", "scales", "quats", "opacities", "features_dc",
                                                         "features_rest")})
    model.step = 30000
    model.train()
    K = sc["Ks"][0].cpu()
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    cam = PinholeCameras(sc["camera_to_worlds"].contiguous(), *intr, args.width, args.height, metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"].contiguous(), "depth_image": sc["gt_depth"].contiguous()}
    opt = FlatAdam(model, means_schedule=FlatAdam.MEANS_SCHEDULE)

    if variant == "c":
        def torch_route(self, out, normal, info, render, alpha, mask):
            """fused_loss's hook for the two terms, with the loss in torch statements over ``render`` / ``alpha``."""
            _target, sink, viewmat, (intr_, _c, _tv) = normal
            A = accumulated_normals(self.means, self.quats, self.scales, viewmat, info, render, log_scales=True,
                                    quat_sink=sink)
            info.pop("_splats", None)
            info.pop("_isect_offsets_full", None)
            lc, ltv = torch_terms(A[0], alpha[0, ..., 0], render[0, ..., 3], intr_, mask)
            out["loss"] = out["loss"] + lc + ltv
            out["normal_consistency_loss"], out["normal_tv_loss"] = lc.detach(), ltv.detach()
        model._add_fused_normal_terms = types.MethodType(torch_route, model)
    elif variant not in ("a", "b"):
        raise SystemExit(f"unknown variant {variant!r}")

    def step():
        for p in model.parameters():
            p.grad = None
        losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0)
        model.backward_fused(losses)
        opt.step(fused_sh=True)
        return losses
    return step, model


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
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
    last = {}
    for v in names:
        for _ in range(args.warmup):
            last[v] = steps[v]()
    torch.cuda.synchronize()
    if "b" in last and "c" in last:                           # (the first steps differ by the optimiser's path only)
        print("warm-up values: " + ", ".join(f"({v}) consistency {float(last[v]['normal_consistency_loss']):.6f} tv "
                                             f"{float(last[v]['normal_tv_loss']):.6f}" for v in ("b", "c")), flush=True)
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
    print(json.dumps({"workload": f"{args.gaussians} Gaussians, 1 cam @ {args.width}x{args.height}",
                      "steps_per_round": args.steps, "ms_per_step": ms, "median_ms_per_step": med,
                      "b_minus_a_ms": med["b"] - med["a"], "c_minus_a_ms": med["c"] - med["a"]}))


if __name__ == "__main__":
    main()
