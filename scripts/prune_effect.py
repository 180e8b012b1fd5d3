#!/usr/bin/env python3
"""What pruning by blending contribution does to a trained model (prune.py): the share of Gaussians removed, the PSNR over
the training views before and after, and the step time before and after -- pruned once after training and once during
training with training continued.  The scene of examples/train_synthetic.py seen from several cameras: the ground truth
is a render of the unperturbed scene, training starts from perturbed parameters.

    python scripts/prune_effect.py [--gaussians 20000 --width 640 --height 360 --cameras 4 --steps 400]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd.model import FlatAdam, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig  # noqa: E402
from qed_splatter_amd.prune import PruneConfig, prune, score_views  # noqa: E402
from qed_splatter_amd.scene import synthetic_scene  # noqa: E402

NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=20000)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--cameras", type=int, default=4)
    ap.add_argument("--steps", type=int, default=400)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L.load()
    sc = synthetic_scene(a.gaussians, a.width, a.height, seed=0, n_cameras=a.cameras)
    K = sc["Ks"][0]
    cams = [PinholeCameras(sc["camera_to_worlds"][k:k + 1].to(dev), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                           float(K[1, 2]), a.width, a.height) for k in range(a.cameras)]
    cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1)
    gt_model = QEDSplatterModel(cfg, **{k: sc[k].to(dev) for k in NAMES})
    gt_model.step = 10_000
    gt_model.eval()
    with torch.no_grad():
        gts = [gt_model.get_outputs(c) for c in cams]
    batches = [{"image": g["rgb"].contiguous(), "depth_image": g["depth"].contiguous()} for g in gts]

    def fresh():
        g = torch.Generator().manual_seed(1)
        init = {k: sc[k].clone() for k in NAMES}
        init["means"] += 0.01 * torch.randn(init["means"].shape, generator=g)
        init["features_dc"] += 0.3 * torch.randn(init["features_dc"].shape, generator=g)
        init["opacities"] -= 1.0
        m = QEDSplatterModel(cfg, **{k: v.to(dev) for k, v in init.items()})
        m.step = 10_000
        return m, FlatAdam(m, means_schedule=FlatAdam.MEANS_SCHEDULE)

    def train(model, opt, first, steps):
        model.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(first, first + steps):
            for p in model.parameters():
                p.grad = None
            out = model.fused_loss(cams[s % len(cams)], batches[s % len(cams)])
            out["loss"].backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / max(steps, 1) * 1e3

    @torch.no_grad()
    def psnr(model):
        model.eval()
        vals = []
        for c, b in zip(cams, batches):
            mse = ((model.get_outputs(c)["rgb"] - b["image"]) ** 2).mean()
            vals.append(float(10.0 * torch.log10(1.0 / mse)))
        return sum(vals) / len(vals)

    def clone(model, opt):
        m = QEDSplatterModel(cfg, **{k: model.gauss_params[k].detach().clone() for k in NAMES})
        m.step = model.step
        o = FlatAdam(m, means_schedule=FlatAdam.MEANS_SCHEDULE)
        o.load_state_dict(opt.state_dict())
        return m, o

    result = {"gaussians": a.gaussians, "size": [a.width, a.height], "cameras": a.cameras, "steps": a.steps}
    model, opt = fresh()
    ms = train(model, opt, 0, a.steps)
    base = {"n": model.num_points, "psnr": psnr(model), "step_ms": ms}
    result["trained"] = base
    for name, pc in (("after_training_min_score_0.01", PruneConfig(score="max", min_score=0.01)),
                     ("after_training_keep_fraction_0.5", PruneConfig(score="sum", keep_fraction=0.5))):
        m, o = clone(model, opt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = prune(m, o, score_views(m, cams), pc)
        torch.cuda.synchronize()
        result[name] = {"n_after": info["n_after"], "removed_share": info["n_pruned"] / info["n_before"], "psnr": psnr(m),
                        "score_and_prune_ms": (time.perf_counter() - t0) * 1e3, "step_ms_after": train(m, o, a.steps, 40)}
    for name, pc in (("during_training_min_score_0.01", PruneConfig(score="max", min_score=0.01)),
                     ("during_training_keep_fraction_0.5", PruneConfig(score="sum", keep_fraction=0.5))):
        m, o = fresh()
        ms0 = train(m, o, 0, a.steps // 2)
        info = prune(m, o, score_views(m, cams), pc)
        ms1 = train(m, o, a.steps // 2, a.steps - a.steps // 2)
        result[name] = {"n_after": info["n_after"], "removed_share": info["n_pruned"] / info["n_before"], "psnr": psnr(m),
                        "step_ms_before": ms0, "step_ms_after": ms1}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
