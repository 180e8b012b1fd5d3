#!/usr/bin/env python3
"""Step time of the reference-shaped route with the bilateral grid off and on, at config B (500 k Gaussians @ 1920x1080):

    zero_grad -> get_outputs(camera with cam_idx) -> get_metrics_dict -> get_loss_dict (+ tv_loss) -> sum -> backward ->
    six QedAdam groups + torch.optim.Adam on "bilateral_grid" (config.py: lr 2e-3, eps 1e-15, exponential decay to 1e-4
    over 30 000 steps after a 1 000-step warm-up)

for num_train_data 1 and 300 (the TV term runs over all grids).  Prints one line per case and a JSON line.

    python scripts/bilagrid_bench.py [--steps K] [--warmup W]
"""
import argparse
import functools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from qed_splatter_amd.model import (FlatAdam, PinholeCameras, QedAdam, QEDSplatterModel,  # noqa: E402
                                    QEDSplatterModelConfig, exponential_decay_lr)

NAMES = ("means", "features_dc", "features_rest", "opacities", "scales", "quats")


def step_ms(sc, dev, w, h, num_train_data, steps, warmup):
    grid = num_train_data is not None
    cfg = QEDSplatterModelConfig.synthetic(sh_degree=3, sh_degree_interval=1, graph_segments="always",
                                           use_bilateral_grid=grid)
    model = QEDSplatterModel(cfg, num_train_data=num_train_data, **{k: sc[k].clone() for k in NAMES})
    model.step = 2000
    model.train()
    K = sc["Ks"][0].cpu()
    cam = PinholeCameras(sc["camera_to_worlds"], float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), w, h,
                         metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"].contiguous(), "depth_image": sc["gt_depth"].contiguous()}
    opts = {k: QedAdam([model.gauss_params[k]], lr=FlatAdam.DEFAULT_LRS[k], eps=1e-15) for k in NAMES}
    if grid:
        opts["bilateral_grid"] = torch.optim.Adam(model.get_param_groups()["bilateral_grid"], lr=2e-3, eps=1e-15)

    def step():
        for o in opts.values():
            o.zero_grad(set_to_none=True)
        out = model.get_outputs(cam)
        ld = model.get_loss_dict(out, batch, model.get_metrics_dict(out, batch))
        functools.reduce(torch.add, ld.values()).backward()
        if grid:
            opts["bilateral_grid"].param_groups[0]["lr"] = exponential_decay_lr(model.step, 2e-3, 1e-4, 30000, 1000)
        for o in opts.values():
            o.step()
        model.step += 1

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bilagrid_bench.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))
    sc = bench.make_scene(a.gaussians, a.width, a.height, 0, dev)
    res = {}
    # off / on alternated twice: the spread between the two rounds says how far apart two cases must be to differ
    for rnd in range(2):
        for name, ntd in (("off", None), ("on_1", 1), ("on_300", 300)):
            ms = step_ms(sc, dev, a.width, a.height, ntd, a.steps, a.warmup)
            res.setdefault(name, []).append(ms)
            print(f"[bilagrid_bench] round {rnd} grid {name:7s}: {ms:.3f} ms/step", flush=True)
            torch.cuda.empty_cache()
    print(json.dumps({"workload": f"{a.gaussians} Gaussians @ {a.width}x{a.height}, reference-shaped route",
                      "steps": a.steps, "ms_per_step": {k: [round(v, 4) for v in vs] for k, vs in res.items()}}))


if __name__ == "__main__":
    main()
