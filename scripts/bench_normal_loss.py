#!/usr/bin/env python
"""What the normal loss costs a training step at config B (500 k Gaussians, one camera @ 1920x1080).

Three variants of train.Trainer.train_step's sequence (fused_loss -> backward_fused -> FlatAdam.step(fused_sh=True); no
densifier), each on its own copy of bench.py's scene, measured in ONE process, alternating, after a warm-up:

  a  config.use_normal_loss off
  b  config.use_normal_loss on (normals.py: qed_gaussian_normals, one more compositing forward and backward on the colour
     pass's lists, qed_normal_loss, qed_normal_rows_merge, qed_gaussian_normals_bwd)
  c  the same loss made the only way available before: the per-Gaussian normals in torch statements, a SECOND
     rasterization() call with them as colours (its own projection, binning, compositing and their backward passes), the
     loss in torch statements on A / |A|; the target's normals by qed_depth_normals in all variants

    python scripts/bench_normal_loss.py [--rounds 5] [--steps 20] [--warmup 10]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_normal_loss.py --variant b --steps 20 --warmup 5

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

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def torch_normals(means, quats, scales, viewmat):
    """[N,3]: the camera-frame normals of qed_gaussian_normals in torch statements (differentiable in ``quats``)."""
    q = quats / quats.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                      2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                      2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    k = scales.detach().argmin(dim=-1)
    n_w = Rm[torch.arange(Rm.shape[0], device=Rm.device), :, k]
    Rv, t = viewmat[0, :3, :3], viewmat[0, :3, 3]
    o = -(Rv.T @ t)
    flip = ((n_w.detach() * (means.detach() - o)).sum(-1) > 0)
    n_w = torch.where(flip[:, None], -n_w, n_w)
    return n_w @ Rv.T


def build(variant: str, args, dev):
    """(step function, model) of one variant on its own copy of the scene."""
    from bench import make_scene
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.normals import depth_normal_target
    from qed_splatter_amd.rasterization import rasterization
    sc = make_scene(args.gaussians, args.width, args.height, 0, dev)
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1, use_normal_loss=(variant == "b"),
                                           normal_lambda=0.1, use_normal_cosine_loss=True)
    model = QEDSplatterModel(cfg, **{k: sc[k] for k in ("means", "scales", "quats", "opacities", "features_dc",
                                                         "features_rest")})
    model.step = 30000
    model.train()
    K = sc["Ks"][0].cpu()
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    cam = PinholeCameras(sc["camera_to_worlds"].contiguous(), *intr, args.width, args.height, metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"].contiguous(), "depth_image": sc["gt_depth"].contiguous()}
    opt = FlatAdam(model, means_schedule=FlatAdam.MEANS_SCHEDULE)
    H, W = args.height, args.width

    if variant in ("a", "b"):
        def step():
            for p in model.parameters():
                p.grad = None
            losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0)
            model.backward_fused(losses)
            opt.step(fused_sh=True)
    elif variant == "c":
        from qed_splatter_amd.model import get_viewmat

        def step():
            for p in model.parameters():
                p.grad = None
            losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0)
            viewmat = get_viewmat(cam.camera_to_worlds).to(dev, torch.float32)
            normals = torch_normals(model.means, model.quats, model.scales, viewmat)
            A, alpha, _ = rasterization(model.means, model.quats, model.scales, model.opacities, normals, viewmat,
                                        sc["Ks"], W, H, render_mode="RGB", sh_degree=None,
                                        _flags=L.F_LOG_SCALES | L.F_LOGIT_OPAC | L.F_TIGHT_TILES)
            target, valid = depth_normal_target(batch["depth_image"], *intr)
            ln = A[0].norm(dim=-1)
            V = (alpha[0, ..., 0] >= 0.5) & (ln > 1e-8) & ((valid & L.NV_DEPTH_NORMAL) != 0)
            n = A[0] / ln.clamp(min=1e-8)[..., None]
            cnt = V.sum().clamp(min=1)
            l1 = ((n - target).abs().sum(-1) * V).sum() / (3 * cnt)
            cs = ((1 - (n * target).sum(-1)) * V).sum() / cnt
            (losses["loss"] + 0.1 * (l1 + cs)).backward()
            opt.step(fused_sh=True)
    else:
        raise SystemExit(f"unknown variant {variant!r}")
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
    print(json.dumps({"workload": f"{args.gaussians} Gaussians, 1 cam @ {args.width}x{args.height}",
                      "steps_per_round": args.steps, "ms_per_step": ms, "median_ms_per_step": med,
                      "b_minus_a_ms": med["b"] - med["a"], "c_minus_a_ms": med["c"] - med["a"]}))


if __name__ == "__main__":
    main()
