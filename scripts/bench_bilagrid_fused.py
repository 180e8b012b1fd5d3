#!/usr/bin/env python
"""What the bilateral grids cost a training step at config B (500 k Gaussians, one camera @ 1920x1080), and what the fused
grid step (qed_bilagrid_step) costs against the launches it replaces.

Step variants, each on its own copy of bench.py's scene, measured in ONE process, alternating, after a warm-up:

  a  the fused route without grids: fused_loss -> backward_fused -> FlatAdam.step(fused_sh=True)  (train.Trainer's sequence
     without the densifier)
  b  the fused route with ``--grids`` grids: fused_loss(grid_optimizer=...) -> backward_fused -> FlatAdam.step(fused_sh=True)
     -> BilateralGridOptimizer.step_fused
  c  the reference-shaped route, the only way to train grids before: get_outputs -> get_metrics_dict -> get_loss_dict
     (+ tv_loss) -> sum -> backward -> six QedAdam groups + torch.optim.Adam on "bilateral_grid" (scripts/bilagrid_bench.py's
     sequence, graph_segments="always")

    python scripts/bench_bilagrid_fused.py [--grids 200] [--rounds 5] [--steps 20] [--warmup 10]
    python scripts/bench_bilagrid_fused.py --micro [--grids 1000]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_bilagrid_fused.py --variant b --steps 20 --warmup 5

The first form prints ms per step per variant and round, the medians and one JSON line.  ``--micro`` times, with device
events and alternating, on grids alone: (s) one qed_bilagrid_step launch, (t) the passes the torch route makes over all
grids for the same work -- qed_bilagrid_tv_bwd, a zeros_like for the slice gradient, autograd's add of the two, and
torch.optim.Adam.step -- and (k) a device-to-device copy of the bytes (s) has to move (3 arrays read, 3 written), the box's
copy rate.  ``--variant X`` runs one variant alone, for a kernel trace: the difference of two variants' dispatch counts over
the same number of steps is the number of launches per step between them.
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def build(variant: str, args, dev):
    """The step function of one variant on its own copy of the scene."""
    from bench import make_scene
    from qed_splatter_amd.bilagrid import BilateralGridOptimizer
    from qed_splatter_amd.model import (FlatAdam, PinholeCameras, QedAdam, QEDSplatterModel, QEDSplatterModelConfig,
                                        exponential_decay_lr)
    sc = make_scene(args.gaussians, args.width, args.height, 0, dev)
    grid = variant != "a"
    extra = dict(graph_segments="always") if variant == "c" else {}
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1, use_bilateral_grid=grid, **extra)
    model = QEDSplatterModel(cfg, num_train_data=args.grids if grid else None, **{k: sc[k] for k in NAMES})
    model.step = 2000
    model.train()
    K = sc["Ks"][0].cpu()
    cam = PinholeCameras(sc["camera_to_worlds"].contiguous(), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
                         args.width, args.height, metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"].contiguous(), "depth_image": sc["gt_depth"].contiguous()}
    count = [0]

    if variant in ("a", "b"):
        opt = FlatAdam(model, means_schedule=FlatAdam.MEANS_SCHEDULE)
        grid_opt = BilateralGridOptimizer(model.bil_grids) if grid else None

        def step():
            for p in model.parameters():
                p.grad = None
            i = count[0] % args.grids
            losses = model.fused_loss(cam, batch, compact_sh_grad=True, frame_key=0, grid_optimizer=grid_opt, cam_idx=i)
            model.backward_fused(losses)
            opt.step(fused_sh=True)
            if grid_opt is not None:
                grid_opt.step_fused(2000 + count[0])
            count[0] += 1
    elif variant == "c":
        opts = {k: QedAdam([model.gauss_params[k]], lr=FlatAdam.DEFAULT_LRS[k], eps=1e-15) for k in NAMES}
        opts["bilateral_grid"] = torch.optim.Adam(model.get_param_groups()["bilateral_grid"], lr=2e-3, eps=1e-15)

        def step():
            for o in opts.values():
                o.zero_grad(set_to_none=True)
            cam.metadata["cam_idx"] = count[0] % args.grids
            out = model.get_outputs(cam)
            ld = model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch))
            functools.reduce(torch.add, ld.values()).backward()
            opts["bilateral_grid"].param_groups[0]["lr"] = exponential_decay_lr(2000 + count[0], 2e-3, 1e-4, 30000, 1000)
            for o in opts.values():
                o.step()
            count[0] += 1
    else:
        raise SystemExit(f"unknown variant {variant!r}")
    return step


def micro(args, dev) -> None:
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.bilagrid import BilateralGrid, total_variation_loss
    lib = L.load()
    n, (GX, GY, GL) = args.grids, args.grid_shape
    gen = torch.Generator(device=dev).manual_seed(0)

    def grids():
        g = BilateralGrid(n, GX, GY, GL, device=dev).grids.detach()
        return (g + 0.05 * torch.randn(g.shape, generator=gen, device=dev)).contiguous()

    numel = n * 12 * GL * GY * GX
    # (s) the fused step
    p, m, v = grids(), torch.zeros(numel, device=dev), torch.zeros(numel, device=dev)
    ws = torch.zeros(GY, GX, GL, 12, device=dev)
    t = [0]

    def fused():
        t[0] += 1
        L.check(lib.qed_bilagrid_step(n, L.ptr(p), L.ptr(m), L.ptr(v), GX, GY, GL, 10.0, t[0] % n, L.ptr(ws), 2e-3, 0.9, 0.999,
                                      1e-15, t[0], None, None, L.current_stream()), "qed_bilagrid_step")

    # (t) the torch route's passes over all grids: TV backward, the slice gradient's zeros_like, the add, Adam
    q = grids().requires_grad_(True)
    adam = torch.optim.Adam([q], lr=2e-3, eps=1e-15)
    ten = torch.full((), 10.0, device=dev)

    def torch_route():
        v_tv = torch.empty_like(q)
        L.check(lib.qed_bilagrid_tv_bwd(n, L.ptr(q), GX, GY, GL, L.ptr(ten), L.ptr(v_tv), L.current_stream()), "qed_bilagrid_tv_bwd")
        v_slice = torch.zeros_like(q)
        q.grad = v_tv + v_slice
        adam.step()

    # (k) a copy of the bytes (s) moves: three arrays
    src, dst = torch.empty(3 * numel, device=dev), torch.empty(3 * numel, device=dev)

    def copy():
        dst.copy_(src)

    # (f) the TV value fused_loss computes for the logged loss
    def tv_value():
        with torch.no_grad():
            total_variation_loss(p)

    cases = {"s": fused, "t": torch_route, "k": copy, "f": tv_value}
    for fn in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in cases}
    for r in range(args.rounds):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) / args.steps * 1e3)
        print(f"round {r}: " + ", ".join(f"({k}) {us[k][-1]:.1f} us" for k in cases), flush=True)
    med = {k: statistics.median(vs) for k, vs in us.items()}
    moved = 6 * numel * 4
    print(f"{n} grids of {GX}x{GY}x{GL}: {numel * 4 / 1e6:.1f} MB of parameters; the step reads and writes p, m, v once: "
          f"{moved / 1e6:.1f} MB")
    print(f"median us: (s) qed_bilagrid_step {med['s']:.1f} = {moved / med['s'] / 1e6:.2f} TB/s;  (k) copy of the same bytes "
          f"{med['k']:.1f} = {moved / med['k'] / 1e6:.2f} TB/s;  (t) torch route {med['t']:.1f};  (f) TV value {med['f']:.1f}")
    print(json.dumps({"grids": n, "grid_shape": [GX, GY, GL], "bytes_moved": moved, "us": us, "median_us": med,
                      "step_TBps": moved / med["s"] / 1e6, "copy_TBps": moved / med["k"] / 1e6,
                      "torch_over_fused": med["t"] / med["s"]}))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grids", type=int, default=200, help="training images: one grid each")
    ap.add_argument("--grid-shape", type=int, nargs=3, default=[16, 16, 8], metavar=("X", "Y", "L"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="timed steps per variant and round")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--variant", choices=("a", "b", "c"), default=None, help="run this variant alone (for a kernel trace)")
    ap.add_argument("--micro", action="store_true", help="time the grid step against the launches it replaces, grids alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from qed_splatter_amd import _lib as L
    L.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    if args.micro:
        micro(args, dev)
        return
    names = [args.variant] if args.variant else ["a", "b", "c"]
    steps = {v: build(v, args, dev) for v in names}
    for v in names:
        for _ in range(args.warmup):
            steps[v]()
    torch.cuda.synchronize()
    if args.variant:
        for _ in range(args.steps):
            steps[args.variant]()
        torch.cuda.synchronize()
        print(json.dumps({"variant": args.variant, "grids": args.grids, "steps": args.warmup + args.steps}))
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
    print(f"{args.grids} grids, median ms/step: (a) {med['a']:.3f}  (b) {med['b']:.3f}  (c) {med['c']:.3f};  (b) - (a) = "
          f"{med['b'] - med['a']:+.3f}, (c) - (a) = {med['c'] - med['a']:+.3f}")
    print(json.dumps({"workload": f"{args.gaussians} Gaussians, 1 cam @ {args.width}x{args.height}, {args.grids} grids",
                      "steps_per_round": args.steps, "ms_per_step": ms, "median_ms_per_step": med,
                      "b_minus_a_ms": med["b"] - med["a"], "c_minus_a_ms": med["c"] - med["a"]}))


if __name__ == "__main__":
    main()
