"""Train on a dataset directory -- what ``ns-train qed-splatter --data PATH`` does in the reference, on one GPU:

    python -m qed_splatter_amd.train --data DIR --steps 30000 [--save ckpt.pt] [--resume ckpt.pt]
                                     [--export-ply splat.ply [--export-frame dataset]] [--render-eval DIR]

The dataset is read by ``dataparser.parse_dataset``, cached by ``datamanager.FullImageDatamanager`` (uint8 images on
the GPU), and every step takes the next training camera and its frame through the eager fused route: ``fused_loss``
(which makes the step's ground truth in one launch, csrc/ingest.hip) -> ``backward_fused`` -> ``FlatAdam.step`` ->
``Densifier``.  ``--undistort`` accepts datasets whose cameras carry OPENCV or OPENCV_FISHEYE distortion: their frames are
resampled to a pinhole on the GPU while the cache is filled (dataparser.py, csrc/undistort.hip).  The captured hipGraph step (graph.py) is not used: it replays ONE camera and ONE ground truth.

The Gaussians are seeded from the dataset's ``ply_file_path`` (``--init-from-ply`` overrides it) in the frame of the
cameras, or from random points when there is none.  Every ``--eval-every`` steps and at the end the evaluation split
is rendered and its metrics averaged; the last line of output is one JSON object.
"""
from __future__ import annotations

import argparse
import json
import time
from typing import Dict, Optional

import torch

from . import _lib as L
from .datamanager import FullImageDatamanager
from .dataparser import DataparserConfig
from .densify import DensifyConfig, Densifier
from .model import GROUP_ORDER, FlatAdam, QEDSplatterModel, QEDSplatterModelConfig


class Trainer:
    """One model, its optimiser and densifier, driven by a datamanager."""

    def __init__(self, model: QEDSplatterModel, datamanager: FullImageDatamanager, seed: int = 0,
                 densify_config: Optional[DensifyConfig] = None):
        self.model, self.datamanager, self.seed = model, datamanager, int(seed)
        self.densify_config = densify_config
        self.step = 0
        self._bind_optimizer()

    def _bind_optimizer(self) -> None:
        self.optimizer = FlatAdam(self.model, means_schedule=FlatAdam.MEANS_SCHEDULE)
        self.densifier = Densifier(self.model, self.optimizer, self.densify_config or DensifyConfig(),
                                   num_train_data=self.datamanager.num_train, seed=self.seed)

    def train_step(self) -> Dict[str, torch.Tensor]:
        """One training iteration on the next camera; returns fused_loss's dict (device tensors, nothing is read back)."""
        model, step = self.model, self.step
        model.train()
        model.step = step
        camera, batch = self.datamanager.next_train(step)
        for p in model.parameters():
            p.grad = None
        idx = batch["image_idx"]
        # frame_key: the camera's index -- its compositing forward reuses the launch order of this camera's last frame
        losses = model.fused_loss(camera, batch, compact_sh_grad=True, frame_key=idx)
        model.backward_fused(losses)
        self.optimizer.step(fused_sh=True)
        self.densifier.after_train(step)
        if step % self.densifier.config.refine_every == 0:
            self.densifier.refinement_after(step)
        self.step = step + 1
        return losses

    @torch.no_grad()
    def evaluate(self) -> Dict[str, float]:
        """The evaluation split through eval() / get_outputs / get_metrics_dict, averaged.  The per-frame values stay
        on the device until all frames are done."""
        model = self.model
        was_training = model.training
        model.eval()
        per_frame = []
        try:
            for camera, batch in self.datamanager.eval_items():
                per_frame.append(model.get_metrics_dict(model.get_outputs(camera), batch))
        finally:
            model.train(was_training)
        out: Dict[str, float] = {}
        if per_frame:
            for key in per_frame[0]:
                vals = [m[key] for m in per_frame]
                if torch.is_tensor(vals[0]):
                    out[key] = float(torch.stack([v.detach().reshape(()).float() for v in vals]).mean())
                else:
                    out[key] = float(sum(vals)) / len(vals)
        out["gaussian_count"] = model.num_points
        return out

    def save(self, path) -> None:
        """The six tensors, the step, the optimiser state -- and the dataparser's transform and scale and the SH degree,
        so that ``python -m qed_splatter_amd.gaussian_ply export --frame dataset`` works from the file alone."""
        out = self.datamanager.outputs
        torch.save({"params": {n: self.model.gauss_params[n].detach().clone() for n in GROUP_ORDER}, "step": self.step,
                    "optimizer": self.optimizer.state_dict(),
                    "dataparser_transform": out.dataparser_transform.detach().cpu().clone(),
                    "dataparser_scale": float(out.dataparser_scale), "sh_degree": int(self.model.config.sh_degree)}, path)

    def export_ply(self, path, frame: str = "model", color_mode: str = "sh_coeffs") -> Dict[str, int]:
        """The Gaussians as a 3DGS PLY file (gaussian_ply.py), in the model's frame or the dataset's."""
        from .gaussian_ply import export_gaussian_ply
        out = self.datamanager.outputs
        return export_gaussian_ply(self.model, path, frame=frame, dataparser_transform=out.dataparser_transform,
                                   dataparser_scale=out.dataparser_scale, color_mode=color_mode)

    def resume(self, path) -> None:
        """The six tensors, the step and the optimiser state of ``save`` (its other keys are for the exporter and are not
        read): the model is rebuilt around the loaded Gaussians (their number may differ from the seeded model's) with
        this trainer's configuration."""
        ckpt = torch.load(path, map_location=self.model.device, weights_only=False)
        self.model = QEDSplatterModel(self.model.config, **{n: ckpt["params"][n] for n in GROUP_ORDER})
        self._bind_optimizer()
        self.optimizer.load_state_dict(ckpt["optimizer"])
        self.step = int(ckpt["step"])


def build_model(config: QEDSplatterModelConfig, datamanager: FullImageDatamanager, init_from_ply=None, seed: int = 0,
                device=None) -> QEDSplatterModel:
    """Seeded from ``init_from_ply`` or the dataset's ``ply_file_path`` (through the dataparser's transform and scale,
    so that points and cameras share a frame); random points when there is neither."""
    out = datamanager.outputs
    device = device if device is not None else datamanager.compute_device
    ply = init_from_ply if init_from_ply is not None else out.ply_file_path
    if ply is not None:
        # the cloud is in the frame of the json's poses (see DataparserOutputs.ply_file_path): it moves as the cameras do
        return QEDSplatterModel.from_ply(config, ply, out.dataparser_transform, out.dataparser_scale, seed=seed,
                                         device=device)
    return QEDSplatterModel.from_seed_points(config, None, None, random_init=True, seed=seed, device=device)


def main(argv=None) -> Dict:
    ap = argparse.ArgumentParser(prog="python -m qed_splatter_amd.train", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", required=True, help="dataset directory (transforms.json, images, depth maps)")
    ap.add_argument("--steps", type=int, default=30000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--eval-every", type=int, default=0, help="evaluate every this many steps (0: only at the end)")
    ap.add_argument("--init-from-ply", metavar="PATH", default=None)
    ap.add_argument("--save", metavar="PATH", default=None)
    ap.add_argument("--resume", metavar="PATH", default=None)
    ap.add_argument("--orientation-method", choices=("up", "none"), default="up")
    ap.add_argument("--center-method", choices=("poses", "none"), default="poses")
    ap.add_argument("--auto-scale-poses", choices=("True", "False"), default="True")
    ap.add_argument("--depth-unit-scale-factor", type=float, default=0.001)
    ap.add_argument("--train-split-fraction", type=float, default=0.9)
    ap.add_argument("--scale-factor", type=float, default=1.0, help="the dataparser's scale_factor")
    ap.add_argument("--num-downscales", type=int, default=2, help="halvings of the resolution at the start of training")
    ap.add_argument("--resolution-schedule", type=int, default=3000, help="steps per halving")
    ap.add_argument("--background-color", choices=("random", "black", "white"), default="random")
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--undistort", action="store_true",
                    help="accept OPENCV / OPENCV_FISHEYE distortion: undistort the frames on the GPU while caching them")
    ap.add_argument("--export-ply", metavar="PATH", default=None,
                    help="after the last evaluation, write the Gaussians as a 3DGS PLY file (gaussian_ply.py)")
    ap.add_argument("--export-frame", choices=("model", "dataset"), default="model",
                    help="'dataset': undo the dataparser's orientation, centring and scale in the exported file")
    ap.add_argument("--cache-device", default=None, help="'cpu' keeps the image cache in pinned host memory")
    ap.add_argument("--render-eval", metavar="DIR", default=None,
                    help="after the last evaluation, write the evaluation views as PNG files (render.py: colour, 16-bit depth "
                         "in the dataset's unit, colour-mapped depth, accumulation)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("qed_splatter_amd.train needs a GPU")
    L.load()
    torch.manual_seed(a.seed)
    dp_cfg = DataparserConfig(orientation_method=a.orientation_method, center_method=a.center_method,
                              auto_scale_poses=a.auto_scale_poses == "True",
                              depth_unit_scale_factor=a.depth_unit_scale_factor,
                              train_split_fraction=a.train_split_fraction, scale_factor=a.scale_factor,
                              undistort=a.undistort)
    dm = FullImageDatamanager(a.data, dp_cfg, device=a.cache_device, seed=a.seed)
    config = QEDSplatterModelConfig(num_downscales=a.num_downscales, resolution_schedule=a.resolution_schedule,
                                    background_color=a.background_color, sh_degree=a.sh_degree)
    model = build_model(config, dm, a.init_from_ply, a.seed)
    print(f"seeded {model.num_points} Gaussians")
    trainer = Trainer(model, dm, seed=a.seed)
    if a.resume:
        trainer.resume(a.resume)
        print(f"resumed {a.resume} at step {trainer.step} with {trainer.model.num_points} Gaussians")
    metrics: Dict[str, float] = {}
    first = trainer.step
    torch.cuda.synchronize()
    t0 = time.time()
    while trainer.step < a.steps:
        trainer.train_step()
        if a.eval_every and trainer.step % a.eval_every == 0 and trainer.step < a.steps:
            metrics = trainer.evaluate()
            print(f"step {trainer.step}: " + ", ".join(f"{k} {v:.5g}" for k, v in metrics.items()), flush=True)
    torch.cuda.synchronize()
    elapsed = time.time() - t0
    metrics = trainer.evaluate()
    print(f"step {trainer.step}: " + ", ".join(f"{k} {v:.5g}" for k, v in metrics.items()), flush=True)
    if a.save:
        trainer.save(a.save)
    if a.export_ply:
        res = trainer.export_ply(a.export_ply, a.export_frame)
        print(f"exported {res['written']} Gaussians to {a.export_ply} ({a.export_frame} frame; dropped "
              f"{res['dropped_nonfinite']} non-finite, {res['dropped_low_opacity']} below opacity 1/255)")
    done = trainer.step - first
    result = {"steps": trainer.step, "steps_per_s": done / elapsed if elapsed > 0 and done else 0.0,
              "eval": metrics, "gaussian_count": trainer.model.num_points}
    if a.render_eval:
        from .render import dataset_path, render_to_directory
        unit = float(dm.outputs.dataparser_scale) * float(dm.outputs.depth_unit_scale_factor)
        result["render_eval"] = render_to_directory(trainer.model, dataset_path(dm, "eval"), a.render_eval, depth_unit=unit)
        print(f"rendered {result['render_eval']['frames']} evaluation views to {a.render_eval}")
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
