#!/usr/bin/env python
"""What the relative-depth terms cost, at 1920 x 1080.

Part 1, the entry against torch statements (no model): on one seeded depth / alpha / prior triple (12 % of the pixels with
alpha == 0, 1 % of the prior 0) the value AND the gradient of each type,

  k    qed_relative_depth_loss with QED_RD_REDUCE | QED_RD_GRAD into a dense plane (the launches of one step)
  k4   the same on channel 3 of an [H,W,4] image, read and written with stride 4, QED_RD_ACCUMULATE (the fused route's form)
  t    the same value and gradient formed with float32 torch statements and autograd on the same tensors -- the only way to
       get them before this feature (for PatchPearson: box sums by index_add_ over a precomputed box index)

each timed as a batch of ``--iters`` back-to-back calls between two synchronisations, ``--rounds`` times, alternating; the
first round's values are printed against each other.

Part 2, the trainer's step at config B (500 k Gaussians, one camera; fused_loss -> backward_fused -> FlatAdam.step(fused_sh=
True); no densifier), on its own copy of bench.py's scene per variant, alternating in ONE process after a warm-up:

  off   the feature off: the parent's launches
  p  pi  s  b  b8    Pearson, Pearson in inverse space, ScaleShiftL1, PatchPearson with P = 64 (jitter on), with P = 8
  st    ScaleShiftL1 beside depth_tv_lambda 0.05

    python scripts/bench_relative_depth.py [--rounds 5] [--iters 50] [--steps 20] [--warmup 8] [--skip-step]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_relative_depth.py --variant b --steps 20 --warmup 5

``--variant X`` runs one step variant alone, for a kernel trace in a run of its own.  Prints the figures and one JSON line.
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

LAM = 0.1
STEP = {"off": {}, "p": dict(relative_depth_loss_type="Pearson"),
        "pi": dict(relative_depth_loss_type="Pearson", relative_depth_space="inverse"),
        "s": dict(relative_depth_loss_type="ScaleShiftL1"), "b": dict(relative_depth_loss_type="PatchPearson"),
        "b8": dict(relative_depth_loss_type="PatchPearson", relative_depth_patch=8),
        "st": dict(relative_depth_loss_type="ScaleShiftL1", depth_tv_lambda=0.05)}
ENTRY = {"Pearson": 64, "ScaleShiftL1": 64, "PatchPearson": 64, "PatchPearson8": 8}


def torch_term(kind, d, alpha, prior, box, n_boxes, K):
    """The term in float32 torch statements; ``d`` [H,W] requires grad."""
    V = (alpha > 0) & torch.isfinite(d) & torch.isfinite(prior) & (prior > 0)
    zero = torch.zeros_like(d)
    x, g = torch.where(V, d, zero), torch.where(V, prior, zero)
    if kind.startswith("Patch"):
        idx = box.reshape(-1)
        w = V.reshape(-1).to(d.dtype)

        def sums(v):
            return torch.zeros(n_boxes, dtype=d.dtype, device=d.device).index_add_(0, idx, v.reshape(-1))
        n = sums(w)
        nn = n.clamp(min=1)
        mx, mg = sums(x) / nn, sums(g) / nn
        dx, dg = (x.reshape(-1) - mx[idx]) * w, (g.reshape(-1) - mg[idx]) * w
        vx, vg, cov = sums(dx * dx) / nn, sums(dg * dg) / nn, sums(dx * dg) / nn
        on = (n >= K) & (vx > 1e-12 * sums(x * x) / nn) & (vg > 1e-12 * sums(g * g) / nn)
        rho = cov / torch.sqrt(torch.where(on, vx * vg, torch.ones_like(vx)))
        return LAM * torch.where(on, 1 - rho, torch.zeros_like(rho)).sum() / on.sum().clamp(min=1)
    n = V.sum()
    mx, mg = x.sum() / n, g.sum() / n
    dx, dg = torch.where(V, d - mx, zero), torch.where(V, prior - mg, zero)
    vx, vg, cov = (dx * dx).sum() / n, (dg * dg).sum() / n, (dx * dg).sum() / n
    if kind == "Pearson":
        return LAM * (1 - cov / torch.sqrt(vx * vg))
    s = (cov / vg).detach()
    t = (mx - s * mg).detach()
    return LAM * torch.where(V, d - (s * prior + t), zero).abs().sum() / n


def bench_entry(args, dev):
    from qed_splatter_amd import _lib as L
    lib = L.load()
    H, W = args.height, args.width
    g = torch.Generator().manual_seed(3)
    depth = (1.0 + 4.0 * torch.rand(H, W, generator=g))
    alpha = 0.1 + 0.9 * torch.rand(H, W, generator=g)
    alpha[torch.rand(H, W, generator=g) < 0.12] = 0.0
    prior = (0.37 * depth + 0.8 + 0.3 * torch.randn(H, W, generator=g)).clamp(min=0.05)
    prior[torch.rand(H, W, generator=g) < 0.01] = 0.0
    depth, alpha, prior = depth.to(dev), alpha.to(dev), prior.to(dev)
    render = torch.zeros(H, W, 4, device=dev)
    render[..., 3] = depth
    v, v4 = torch.empty(H, W, device=dev), torch.zeros(H, W, 4, device=dev)
    out = torch.empty(8, dtype=torch.float64, device=dev)
    out_f = torch.empty(2, device=dev)
    st = L.current_stream()
    runs, first = {}, {}
    for name, P in ENTRY.items():
        kind = name.rstrip("8")
        type_id = L.RELATIVE_DEPTH_TYPES[kind]
        ws = torch.empty(L.relative_depth_ws_doubles(H, W, P if kind == "PatchPearson" else 0), dtype=torch.float64, device=dev)
        box = ((torch.arange(H, device=dev)[:, None] // P) * ((W - 1) // P + 1) + torch.arange(W, device=dev)[None, :] // P)
        n_boxes, K = int(box.max()) + 1, max(2, -(-P * P // 4))
        d_leaf = depth.clone().requires_grad_(True)

        def dense(type_id=type_id, P=P, ws=ws):
            L.check(lib.qed_relative_depth_loss(H, W, L.ptr(depth), 1, L.ptr(alpha), L.ptr(prior), None, type_id, LAM, P, 0, 0,
                                                0.25, L.RD_REDUCE | L.RD_GRAD, None, None, L.ptr(ws), L.ptr(v), 1, L.ptr(out),
                                                L.ptr(out_f), st), "qed_relative_depth_loss")

        def strided(type_id=type_id, P=P, ws=ws):
            L.check(lib.qed_relative_depth_loss(H, W, render.data_ptr() + 12, 4, L.ptr(alpha), L.ptr(prior), None, type_id, LAM,
                                                P, 0, 0, 0.25, L.RD_REDUCE | L.RD_GRAD | L.RD_ACCUMULATE, None, None, L.ptr(ws),
                                                v4.data_ptr() + 12, 4, L.ptr(out), L.ptr(out_f), st), "qed_relative_depth_loss")

        def statements(kind=kind, box=box, n_boxes=n_boxes, K=K, d_leaf=d_leaf):
            d_leaf.grad = None
            loss = torch_term(kind, d_leaf, alpha, prior, box, n_boxes, K)
            loss.backward()
            return loss
        runs[name] = {"k": dense, "k4": strided, "t": statements}
        dense()
        loss_t = statements()
        torch.cuda.synchronize()
        first[name] = (float(out[0]), float(loss_t), float((v - d_leaf.grad).abs().max()), float(d_leaf.grad.abs().max()))
        print(f"{name}: value kernel {first[name][0]:.7f} torch {first[name][1]:.7f}; gradient max |difference| "
              f"{first[name][2]:.3e} of max {first[name][3]:.3e}", flush=True)
    for fns in runs.values():                                 # warm-up
        for fn in fns.values():
            for _ in range(5):
                fn()
    torch.cuda.synchronize()
    us = {n: {k: [] for k in fns} for n, fns in runs.items()}
    for r in range(args.rounds):
        for n, fns in runs.items():
            for k, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    fn()
                torch.cuda.synchronize()
                us[n][k].append((time.perf_counter() - t0) / args.iters * 1e6)
        print(f"round {r}: " + "  ".join(f"{n} " + " ".join(f"({k}) {us[n][k][-1]:.1f}" for k in us[n]) for n in us) + " us/call",
              flush=True)
    med = {n: {k: statistics.median(x) for k, x in us[n].items()} for n in us}
    for n in us:
        print(f"{n}: median us/call " + "  ".join(f"({k}) {med[n][k]:.1f} [{min(us[n][k]):.1f}..{max(us[n][k]):.1f}]"
                                                   for k in us[n]))
    return {"entry_us_per_call": us, "entry_median_us": med, "entry_first_values": first}


def build_step(variant: str, args, dev):
    """The trainer's step of one variant on its own copy of the scene."""
    from bench import make_scene
    from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    sc = make_scene(args.gaussians, args.width, args.height, 0, dev)
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1, graph_segments=False, **STEP[variant])
    model = QEDSplatterModel(cfg, **{k: sc[k] for k in ("means", "scales", "quats", "opacities", "features_dc",
                                                         "features_rest")})
    model.step = 30000
    model.train()
    K = sc["Ks"][0].cpu()
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    cam = PinholeCameras(sc["camera_to_worlds"].contiguous(), *intr, args.width, args.height, metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"].contiguous(), "depth_image": sc["gt_depth"].contiguous()}
    opt = FlatAdam(model, means_schedule=FlatAdam.MEANS_SCHEDULE)

    def step():
        for p in model.parameters():
            p.grad = None
        model.step += 1                                       # (PatchPearson's boxes move with it)
        losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0)
        model.backward_fused(losses)
        opt.step(fused_sh=True)
        return losses
    return step


def bench_step(args, dev):
    names = [args.variant] if args.variant else list(STEP)
    steps = {v: build_step(v, args, dev) for v in names}
    last = {}
    for v in names:
        for _ in range(args.warmup):
            last[v] = steps[v]()
    torch.cuda.synchronize()
    print("warm-up values: " + ", ".join(f"({v}) loss {float(last[v]['loss']):.6f}"
                                         + (f" relative {float(last[v]['relative_depth_loss']):.6f}" if v != "off" else "")
                                         for v in names), flush=True)
    if args.variant:
        for _ in range(args.steps):
            steps[args.variant]()
        torch.cuda.synchronize()
        return {"variant": args.variant, "steps": args.warmup + args.steps}
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
    return {"workload": f"{args.gaussians} Gaussians, 1 cam @ {args.width}x{args.height}", "steps_per_round": args.steps,
            "step_ms": ms, "step_median_ms": med, "step_minus_off_ms": {v: med[v] - med["off"] for v in names if v != "off"}}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="calls per timed batch of part 1")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per variant and round of part 2")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true", help="part 1 only")
    ap.add_argument("--variant", choices=list(STEP), default=None, help="run this step variant alone (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from qed_splatter_amd import _lib as L
    L.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    result = {}
    if not args.variant:
        result.update(bench_entry(args, dev))
    if not args.skip_step:
        result.update(bench_step(args, dev))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
