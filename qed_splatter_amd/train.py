"""Train on a dataset directory -- what ``ns-train qed-splatter --data PATH`` does in the reference, on one GPU:

    python -m qed_splatter_amd.train --data DIR --steps 30000 [--save ckpt.pt] [--resume ckpt.pt]
                                     [--export-ply splat.ply [--export-frame dataset]] [--render-eval DIR]
                                     [--camera-optimizer SO3xR3 [--camera-opt-lr 1e-4] [--save-poses poses.json]]
                                     [--use-bilateral-grid [--grid-shape 16 16 8]] [--color-corrected-metrics]
                                     [--prune-at STEP [STEP ...] [--prune-min-score X | --prune-keep-fraction F]
                                      [--prune-score max|sum] [--prune-view-stride S]]
                                     [--grow-from-depth-every K [--grow-start STEP] [--grow-until STEP] [--grow-stride S]
                                      [--grow-hole-alpha A] [--grow-depth-tol T] [--grow-depth-tol-rel R]
                                      [--grow-init-opacity O] [--grow-max-new M] [--grow-max-gaussians G]]

The dataset is read by ``dataparser.parse_dataset``, cached by ``datamanager.FullImageDatamanager`` (uint8 images on
the GPU), and every step takes the next training camera and its frame through the eager fused route: ``fused_loss``
(which makes the step's ground truth in one launch, csrc/ingest.hip) -> ``backward_fused`` -> ``FlatAdam.step`` ->
``Densifier``.  ``--undistort`` accepts datasets whose cameras carry OPENCV or OPENCV_FISHEYE distortion: their frames are
resampled to a pinhole on the GPU while the cache is filled (dataparser.py, csrc/undistort.hip).  The captured hipGraph step (graph.py) is not used: it replays ONE camera and ONE ground truth.

``--camera-optimizer SO3xR3`` refines the training cameras' poses along with the Gaussians (camera_optimizer.py: Nerfstudio's
CameraOptimizer, two extra launches per step); ``--save-poses`` writes the refined poses in the dataset's own frame.

``--use-bilateral-grid`` gives every training image a grid of affine colour transforms (bilagrid.py: splatfacto's
use_bilateral_grid) that absorbs its exposure and white balance; the grids train on the same route (one slice launch each way
and one launch, qed_bilagrid_step, for their TV gradient and Adam step).  Evaluation renders stay uncorrected, as upstream;
``--color-corrected-metrics`` (splatfacto's color_corrected_metrics) adds, under ``"eval_images"``, the evaluation split's
psnr / ssim / lpips and the same three of every render colour-corrected towards its ground truth (``Trainer.evaluate_images``,
color_correct.py) -- the figures that do not measure the cameras' exposure differences.

``--prune-at`` scores every Gaussian by its blending contribution over the training cameras after the named steps'
refinement and drops the low scorers from the model and the optimiser (prune.py, csrc/importance.hip); the last JSON line
then carries ``"prune": [{"step", "n_before", "n_after", "seconds"}]``.

``--grow-from-depth-every K`` seeds new Gaussians from the step's own depth image every K-th step between ``--grow-start``
and ``--grow-until``, where that camera's render has a hole or lies behind the measurement (depth_grow.py,
csrc/depth_grow.hip); the last JSON line then carries ``"grown": {"calls", "n_added", "n_holes", "n_behind"}``.

The Gaussians are seeded from the dataset's ``ply_file_path`` (``--init-from-ply`` overrides it) in the frame of the
cameras, or from random points when there is none.  Every ``--eval-every`` steps and at the end the evaluation split
is rendered and its metrics averaged; the last line of output is one JSON object.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from .bilagrid import BilateralGridOptimizer, BilateralGridOptimizerConfig, check_step_shape
from .camera_optimizer import CameraOptimizer, CameraOptimizerConfig
from .datamanager import FullImageDatamanager
from .dataparser import DataparserConfig
from .densify import DensifyConfig, Densifier
from .model import GROUP_ORDER, FlatAdam, QEDSplatterModel, QEDSplatterModelConfig


class Trainer:
    """One model, its optimiser and densifier -- and, with ``camera_opt_config`` in a mode other than "off", a camera pose
    optimiser over the training cameras; for a model that holds bilateral grids, their optimiser --, driven by a
    datamanager."""

    def __init__(self, model: QEDSplatterModel, datamanager: FullImageDatamanager, seed: int = 0,
                 densify_config: Optional[DensifyConfig] = None, camera_opt_config: Optional[CameraOptimizerConfig] = None,
                 grid_opt_config: Optional[BilateralGridOptimizerConfig] = None, grow_config=None, grow_every: int = 0,
                 grow_start: Optional[int] = None, grow_until: Optional[int] = None):
        """``grow_config`` (a depth_grow.GrowConfig) with ``grow_every`` = K > 0: every K-th step from ``grow_start`` (default:
        the densifier's warmup_length) up to, not including, ``grow_until`` (default: its stop_split_at) grows Gaussians from
        that step's depth image."""
        self.model, self.datamanager, self.seed = model, datamanager, int(seed)
        self.grow_config, self.grow_every = grow_config, int(grow_every)
        self.grow_start, self.grow_until = grow_start, grow_until
        self.grown = {"calls": 0, "n_added": 0, "n_holes": 0, "n_behind": 0}
        self.densify_config = densify_config
        self.grid_opt_config = grid_opt_config
        self.step = 0
        self.camera_optimizer: Optional[CameraOptimizer] = None
        if camera_opt_config is not None and camera_opt_config.mode != "off":
            self.camera_optimizer = CameraOptimizer(camera_opt_config, datamanager.num_train, model.device)
        if self.grow_every > 0:
            from .depth_grow import GrowConfig, _refuse
            self.grow_config = (self.grow_config or GrowConfig()).validate()
            _refuse(model, "Trainer(grow_every=...)", self.camera_optimizer)       # (before any step is taken)
        self._bind_optimizer()

    def _bind_optimizer(self) -> None:
        self.optimizer = FlatAdam(self.model, means_schedule=FlatAdam.MEANS_SCHEDULE)
        self.grid_optimizer: Optional[BilateralGridOptimizer] = None
        if self.model.bil_grids is not None:
            self.grid_optimizer = BilateralGridOptimizer(self.model.bil_grids, self.grid_opt_config)
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
        pose_opt = self.camera_optimizer
        grid_opt = self.grid_optimizer
        losses = model.fused_loss(camera, batch, compact_sh_grad=True, frame_key=idx, camera_optimizer=pose_opt, cam_idx=idx,
                                  grid_optimizer=grid_opt)
        model.backward_fused(losses)
        if pose_opt is not None:
            pose_opt.step_fused(step)           # the camera's row gradient, the regulariser's, Adam over all rows: one launch
        self.optimizer.step(fused_sh=True)
        if grid_opt is not None:
            grid_opt.step_fused(step)           # every grid's TV gradient, this camera's slab gradient, Adam: one launch
        # growth from this step's depth image: after the optimiser step and before the densifier's statistics, which then
        # go to the rows this step rendered while the appended rows start from their initial values
        n_rendered = None
        if self._grow_due(step):
            n_rendered = model.num_points
            self.grow(camera, batch)
        self.densifier.after_train(step, n_rendered)
        if step % self.densifier.config.refine_every == 0:
            self.densifier.refinement_after(step)
        self.step = step + 1
        return losses

    def _grow_due(self, step: int) -> bool:
        if self.grow_every <= 0 or step % self.grow_every != 0:
            return False
        cfg = self.densifier.config
        start = cfg.warmup_length if self.grow_start is None else int(self.grow_start)
        until = cfg.stop_split_at if self.grow_until is None else int(self.grow_until)
        return start <= step < until

    def grow(self, camera, batch) -> Dict:
        """Seed Gaussians from ``batch``'s depth image where ``camera``'s render misses the surface (depth_grow.py): the
        model, the optimiser's moments and the densifier's running statistics grow together.  Returns depth_grow.grow's dict
        and adds it to ``self.grown``."""
        from .depth_grow import GrowConfig, grow_from_view
        info = grow_from_view(self.model, self.optimizer, camera, batch, self.grow_config or GrowConfig(),
                              densifier=self.densifier, camera_optimizer=self.camera_optimizer)
        self.grown["calls"] += 1
        for key in ("n_added", "n_holes", "n_behind"):
            self.grown[key] += int(info[key])
        return info

    def prune(self, config, view_stride: int = 1) -> Dict:
        """Score the training cameras (every ``view_stride``-th, in evaluation mode, the dataset's masks as pixel masks) and
        drop the low scorers from the model and the optimiser (prune.py); the densifier's running statistics are cleared.
        Returns prune.prune's dict with ``seconds``."""
        from .prune import prune, score_views
        items = list(self.datamanager.train_items())
        masks = [b["mask"] if "mask" in b else None for _, b in items]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = score_views(self.model, [cam for cam, _ in items], masks if any(m is not None for m in masks) else None,
                             view_stride)
        info = prune(self.model, self.optimizer, scores, config, densifier=self.densifier)
        torch.cuda.synchronize()
        info["seconds"] = time.perf_counter() - t0
        return info

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

    @torch.no_grad()
    def depth_pearson(self):
        """The mean of get_metrics_dict's ``depth_pearson`` over the TRAINING cameras, in eval() (None when the relative-depth
        term is off): what the run reports where the evaluation split is empty."""
        model = self.model
        was_training = model.training
        model.eval()
        vals = []
        try:
            for camera, batch in self.datamanager.train_items():
                md = model.get_metrics_dict(model.get_outputs(camera), batch)
                if "depth_pearson" in md:
                    vals.append(md["depth_pearson"].detach().reshape(()).float())
        finally:
            model.train(was_training)
        return float(torch.stack(vals).mean()) if vals else None

    def evaluate_images(self, get_std: bool = True) -> Dict[str, float]:
        """The evaluation split through ``evaluate_image_items``: Nerfstudio's get_average_eval_image_metrics."""
        return evaluate_image_items(self.model, self.datamanager.eval_items(), get_std)

    def save(self, path) -> None:
        """The six tensors, the step, the optimiser state -- and the dataparser's transform and scale and the SH degree,
        so that ``python -m qed_splatter_amd.gaussian_ply export --frame dataset`` works from the file alone."""
        out = self.datamanager.outputs
        ckpt = {"params": {n: self.model.gauss_params[n].detach().clone() for n in GROUP_ORDER}, "step": self.step,
                "optimizer": self.optimizer.state_dict(),
                "dataparser_transform": out.dataparser_transform.detach().cpu().clone(),
                "dataparser_scale": float(out.dataparser_scale), "sh_degree": int(self.model.config.sh_degree)}
        if self.camera_optimizer is not None:           # pose_adjustment, its Adam moments and step count
            ckpt["camera_opt"] = {k: (v.detach().clone() if torch.is_tensor(v) else v)
                                  for k, v in self.camera_optimizer.state_dict().items()}
        if self.grid_optimizer is not None:             # the grids, their Adam moments and step count
            ckpt["bilateral_grid"] = {"grids": self.model.bil_grids.grids.detach().clone(),
                                      "optimizer": {k: (v.detach().clone() if torch.is_tensor(v) else v)
                                                    for k, v in self.grid_optimizer.state_dict().items()}}
        torch.save(ckpt, path)

    def camera_opt_metrics(self) -> Dict[str, float]:
        """camera_optimizer.get_metrics_dict as floats ({} without a camera optimiser)."""
        out: Dict = {}
        if self.camera_optimizer is not None:
            self.camera_optimizer.get_metrics_dict(out)
        return {k: float(v) for k, v in out.items()}

    def save_poses(self, path, data_dir=None) -> int:
        """The training cameras' (refined) poses as a ``transforms.json``-shaped file: ``frames`` = [{"file_path",
        "transform_matrix" 4x4}], in the dataset's own frame -- ``dataparser_scale`` and ``dataparser_transform`` undone in
        float64 on the host.  ``file_path`` is relative to ``data_dir`` when that is given.  Returns the number of frames."""
        out = self.datamanager.outputs
        adj = self.camera_optimizer.pose_adjustment.detach().cpu().numpy() if self.camera_optimizer is not None else None
        poses = poses_in_dataset_frame(out, self.datamanager.i_train, adj)
        frames = []
        for k, m in zip(self.datamanager.i_train, poses):
            name = out.image_filenames[k]
            name = os.path.relpath(name, data_dir) if data_dir is not None else str(name)
            frames.append({"file_path": name.replace(os.sep, "/"), "transform_matrix": m.tolist()})
        mode = self.camera_optimizer.config.mode if self.camera_optimizer is not None else "off"
        with open(path, "w") as f:
            json.dump({"camera_optimizer": mode, "frames": frames}, f, indent=1)
        return len(frames)

    def export_ply(self, path, frame: str = "model", color_mode: str = "sh_coeffs") -> Dict[str, int]:
        """The Gaussians as a 3DGS PLY file (gaussian_ply.py), in the model's frame or the dataset's."""
        from .gaussian_ply import export_gaussian_ply
        out = self.datamanager.outputs
        return export_gaussian_ply(self.model, path, frame=frame, dataparser_transform=out.dataparser_transform,
                                   dataparser_scale=out.dataparser_scale, color_mode=color_mode)

    def export_pointcloud(self, path, frame: str = "model", split: str = "all", **options):
        """An oriented surface point cloud of the model over the dataset's views (surface_cloud.export_pointcloud; its
        keyword ``options``, ``voxel_size`` 0.01 model units unless given), in the model's frame or the dataset's."""
        from .render import dataset_path
        from .surface_cloud import export_pointcloud
        out = self.datamanager.outputs
        options.setdefault("voxel_size", 0.01)
        return export_pointcloud(self.model, dataset_path(self.datamanager, split), path, frame=frame,
                                 dataparser_transform=out.dataparser_transform, dataparser_scale=out.dataparser_scale,
                                 **options)

    def resume(self, path) -> None:
        """The six tensors, the step and the optimiser state of ``save`` (its other keys are for the exporter and are not
        read): the model is rebuilt around the loaded Gaussians (their number may differ from the seeded model's) with
        this trainer's configuration."""
        ckpt = torch.load(path, map_location=self.model.device, weights_only=False)
        n_grids = self.model.bil_grids.grids.shape[0] if self.model.bil_grids is not None else None
        self.model = QEDSplatterModel(self.model.config, num_train_data=n_grids, **{n: ckpt["params"][n] for n in GROUP_ORDER})
        # (a checkpoint written without grids: they start from the identity)
        if self.model.bil_grids is not None and "bilateral_grid" in ckpt:
            with torch.no_grad():
                self.model.bil_grids.grids.copy_(ckpt["bilateral_grid"]["grids"])
        self._bind_optimizer()
        if self.grid_optimizer is not None and "bilateral_grid" in ckpt:
            self.grid_optimizer.load_state_dict(ckpt["bilateral_grid"]["optimizer"])
        self.optimizer.load_state_dict(ckpt["optimizer"])
        self.step = int(ckpt["step"])
        # (a checkpoint written without a camera optimiser: the poses start from zero adjustments)
        if self.camera_optimizer is not None and "camera_opt" in ckpt:
            self.camera_optimizer.load_state_dict(ckpt["camera_opt"])


@torch.no_grad()
def evaluate_image_items(model: QEDSplatterModel, items, get_std: bool = True) -> Dict[str, float]:
    """``items`` ((camera, batch) pairs) through eval() / get_outputs / get_image_metrics_and_images (Nerfstudio's
    get_average_eval_image_metrics, what ``ns-eval`` reports): for every key the mean over the frames and, with
    ``get_std``, ``KEY_std``, the unbiased standard deviation (``torch.std_mean``: NaN for a single frame); ``fps`` and
    ``num_rays_per_sec`` from the render time alone (events around get_outputs).  The per-frame values stay on the device
    until all frames are done: one synchronisation, one read-back."""
    was_training = model.training
    model.eval()
    per_frame, render_events, rays = [], [], []
    timed = model.device.type == "cuda"
    try:
        for camera, batch in items:
            if timed:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
            outputs = model.get_outputs(camera)
            if timed:
                t1.record()
                render_events.append((t0, t1))
            rays.append(int(outputs["rgb"].shape[-3]) * int(outputs["rgb"].shape[-2]))
            per_frame.append(model.get_image_metrics_and_images(outputs, batch)[0])
    finally:
        model.train(was_training)
    out = aggregate_image_metrics(per_frame, get_std)
    if render_events:
        torch.cuda.synchronize(model.device)
        seconds = [max(a.elapsed_time(b), 1e-6) * 1e-3 for a, b in render_events]
        out.update(aggregate_image_metrics([{"num_rays_per_sec": n / s, "fps": 1.0 / s} for n, s in zip(rays, seconds)],
                                           get_std))
    return out


def aggregate_image_metrics(per_frame, get_std: bool = True) -> Dict[str, float]:
    """[{key: 0-dim tensor or number}] per frame -> {key: mean, key_std: unbiased standard deviation} as floats, the keys in
    the first frame's order (Nerfstudio's get_average_eval_image_metrics: ``torch.std_mean`` of the per-frame values, so a
    single frame has the standard deviation NaN).  All keys are stacked on their device and read back once."""
    if not per_frame:
        return {}
    keys = list(per_frame[0])
    as_f64 = lambda v: v.detach().reshape(()).to(torch.float64) if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
    table = torch.stack([torch.stack([as_f64(m[k]) for m in per_frame]) for k in keys])       # [keys, frames]
    if table.shape[1] > 1:
        std, mean = torch.std_mean(table, dim=1)                           # (unbiased)
    else:
        std, mean = torch.full_like(table[:, 0], float("nan")), table[:, 0]
    mean, std = torch.stack([mean, std]).tolist()
    out: Dict[str, float] = {}
    for i, k in enumerate(keys):
        out[k] = float(mean[i])
        if get_std:
            out[f"{k}_std"] = float(std[i])
    return out


def exp_map_SO3xR3_f64(pose_adjustment: np.ndarray) -> np.ndarray:
    """[n,6] -> [n,4,4] float64 on the host: the adjustment matrices [[R, d], [0, 0, 0, 1]] of camera_optimizer.py."""
    t = np.asarray(pose_adjustment, dtype=np.float64)
    out = np.tile(np.eye(4), (t.shape[0], 1, 1))
    for i, (d, w) in enumerate(zip(t[:, :3], t[:, 3:])):
        a = np.sqrt(max(float(w @ w), 1e-4))
        K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        out[i, :3, :3] = np.eye(3) + (np.sin(a) / a) * K + ((1.0 - np.cos(a)) / (a * a)) * (K @ K)
        out[i, :3, 3] = d
    return out


def poses_in_dataset_frame(outputs, indices, pose_adjustment=None) -> np.ndarray:
    """[len(indices),4,4] float64: the cameras ``indices`` of the dataparser's outputs, adjusted by the rows of
    ``pose_adjustment`` (row j belongs to indices[j]; None: as parsed), mapped back to the frame of the dataset's own
    ``transform_matrix`` entries: translation / dataparser_scale, then the inverse of dataparser_transform."""
    idx = np.asarray(list(indices), dtype=np.int64)
    c2w = outputs.camera_to_worlds_f64
    c2w = np.asarray(c2w if c2w is not None else outputs.camera_to_worlds.double().numpy(), dtype=np.float64)[idx]
    T = outputs.dataparser_transform_f64
    T = np.asarray(T if T is not None else outputs.dataparser_transform.double().numpy(), dtype=np.float64)
    full = np.tile(np.eye(4), (len(idx), 1, 1))
    full[:, :3] = c2w[:, :3]
    if pose_adjustment is not None:
        full = full @ exp_map_SO3xR3_f64(pose_adjustment)
    full[:, :3, 3] /= float(outputs.dataparser_scale)
    inv = np.eye(4)
    inv[:3, :3] = T[:, :3].T
    inv[:3, 3] = -T[:, :3].T @ T[:, 3]
    return inv @ full


def build_model(config: QEDSplatterModelConfig, datamanager: FullImageDatamanager, init_from_ply=None, seed: int = 0,
                device=None) -> QEDSplatterModel:
    """Seeded from ``init_from_ply`` or the dataset's ``ply_file_path`` (through the dataparser's transform and scale,
    so that points and cameras share a frame); random points when there is neither.  With ``config.use_bilateral_grid`` the
    model holds one bilateral grid per training image."""
    out = datamanager.outputs
    device = device if device is not None else datamanager.compute_device
    ply = init_from_ply if init_from_ply is not None else out.ply_file_path
    if ply is not None:
        # the cloud is in the frame of the json's poses (see DataparserOutputs.ply_file_path): it moves as the cameras do
        return QEDSplatterModel.from_ply(config, ply, out.dataparser_transform, out.dataparser_scale, seed=seed,
                                         device=device, num_train_data=datamanager.num_train)
    return QEDSplatterModel.from_seed_points(config, None, None, random_init=True, seed=seed, device=device,
                                             num_train_data=datamanager.num_train)


def build_parser() -> argparse.ArgumentParser:
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
    ap.add_argument("--export-pointcloud", metavar="PATH", default=argparse.SUPPRESS,
                    help="after the last evaluation, write an oriented, coloured surface point cloud of the model over the "
                         "dataset's views as a PLY file (surface_cloud.py), in the frame of --export-frame")
    ap.add_argument("--cache-device", default=None, help="'cpu' keeps the image cache in pinned host memory")
    ap.add_argument("--render-eval", metavar="DIR", default=None,
                    help="after the last evaluation, write the evaluation views as PNG files (render.py: colour, 16-bit depth "
                         "in the dataset's unit, colour-mapped depth, accumulation)")
    ap.add_argument("--camera-optimizer", choices=("off", "SO3xR3"), default="off",
                    help="refine the training cameras' poses (Nerfstudio's CameraOptimizer; camera_optimizer.py)")
    ap.add_argument("--camera-opt-lr", type=float, default=1e-4,
                    help="the pose optimiser's learning rate (decays to 5e-7 over 30000 steps after a 1000-step warm-up)")
    ap.add_argument("--save-poses", metavar="PATH", default=None,
                    help="after training, write the training cameras' (refined) poses in the dataset's own frame, as a "
                         "transforms.json-shaped file")
    ap.add_argument("--use-bilateral-grid", action="store_true",
                    help="one grid of affine colour transforms per training image (splatfacto's use_bilateral_grid; bilagrid.py)")
    ap.add_argument("--grid-shape", type=int, nargs=3, metavar=("X", "Y", "L"), default=[16, 16, 8],
                    help="the extents of each bilateral grid (every one >= 2, X * Y * L <= 16384)")
    # (argparse.SUPPRESS: the parsed namespace of a command line without the option is what it was before the option)
    ap.add_argument("--color-corrected-metrics", action="store_true", default=argparse.SUPPRESS,
                    help="after the last evaluation, run the evaluation split through get_image_metrics_and_images with "
                         "splatfacto's color_corrected_metrics (color_correct.py) and add the result as \"eval_images\"")
    ap.add_argument("--output-normals", action="store_true", default=argparse.SUPPRESS,
                    help="after training: render normal maps (normals.py) in the final \"eval_images\" evaluation, which then "
                         "reports their angular errors, and write a normal/ plane with --render-eval; training is unaffected")
    ap.add_argument("--normal-loss", action="store_true", default=argparse.SUPPRESS,
                    help="supervise the rendered normals with the normals of the sensor depth (config.use_normal_loss; "
                         "normals.py); not with --camera-optimizer")
    ap.add_argument("--normal-lambda", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="the normal loss's weight (default 0.1)")
    ap.add_argument("--normal-cosine-loss", action="store_true", default=argparse.SUPPRESS,
                    help="add the mean of 1 - n . g to the normal loss's L1 term")
    ap.add_argument("--normal-consistency", action="store_true", default=argparse.SUPPRESS,
                    help="tie the rendered normals to the normals of the rendered depth (config.use_normal_consistency; "
                         "normals.py); needs no sensor normals; not with --camera-optimizer")
    ap.add_argument("--normal-consistency-lambda", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="the consistency term's weight (default 0.05)")
    ap.add_argument("--normal-consistency-from", type=int, default=argparse.SUPPRESS, metavar="STEP",
                    help="the first step that carries the consistency term (default 0)")
    ap.add_argument("--normal-tv", action="store_true", default=argparse.SUPPRESS,
                    help="total variation of the rendered normals (config.use_normal_tv); not with --camera-optimizer")
    ap.add_argument("--normal-tv-lambda", type=float, default=argparse.SUPPRESS, metavar="Y",
                    help="the smoothness term's weight (default 0.1)")
    ap.add_argument("--depth-loss-type", choices=tuple(L.DEPTH_LOSS_TYPES), default=argparse.SUPPRESS,
                    help="the depth data term (config.depth_loss_type, default L1: the reference's); residuals are in the "
                         "model's units, after the dataparser's scale")
    ap.add_argument("--depth-huber-delta", type=float, default=argparse.SUPPRESS, metavar="D",
                    help="HuberL1's fixed threshold, in the model's units (default 0.1)")
    ap.add_argument("--depth-tv-lambda", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="weight of the total variation of the rendered depth (config.depth_tv_lambda; default 0 = off)")
    ap.add_argument("--no-depth-tv-edge-aware", action="store_true", default=argparse.SUPPRESS,
                    help="do not weight the depth smoothness term down at colour edges of the ground-truth image")
    ap.add_argument("--relative-depth-loss", choices=("off", *L.RELATIVE_DEPTH_TYPES), default=argparse.SUPPRESS, metavar="TYPE",
                    help="treat the depth files as a PRIOR known up to scale and shift (a monocular network's) and supervise "
                         "with Pearson, PatchPearson or ScaleShiftL1 (config.relative_depth_loss_type, default off); the "
                         "metric depth term is then not computed")
    ap.add_argument("--relative-depth-lambda", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="the relative-depth term's weight (default 0.1)")
    ap.add_argument("--relative-depth-space", choices=("depth", "inverse"), default=argparse.SUPPRESS,
                    help="compare the prior with the rendered depth or with its reciprocal (default depth)")
    ap.add_argument("--relative-depth-patch", type=int, default=argparse.SUPPRESS, metavar="P",
                    help="PatchPearson's box size: 8, 16, 32, 64 or 128 pixels (default 64)")
    ap.add_argument("--relative-depth-min-valid", type=float, default=argparse.SUPPRESS, metavar="F",
                    help="a box contributes from this share of valid pixels on, in (0, 1] (default 0.25)")
    ap.add_argument("--no-relative-depth-jitter", action="store_true", default=argparse.SUPPRESS,
                    help="keep PatchPearson's boxes where they are instead of moving them with the step")
    ap.add_argument("--depth-distortion-lambda", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="weight of the depth distortion term: the spread of each pixel's blending weights in depth "
                         "(config.depth_distortion_lambda, depth_distortion.py; default 0 = off), in the model's units")
    ap.add_argument("--depth-distortion-from-step", type=int, default=argparse.SUPPRESS, metavar="K",
                    help="the first step that carries the depth distortion term (default 0)")
    ap.add_argument("--output-depth-spread", action="store_true", default=argparse.SUPPRESS,
                    help="after training: render the depth standard deviation along each ray in the final \"eval_images\" "
                         "evaluation, which then reports depth_std_mean; training is unaffected")
    ap.add_argument("--prune-at", type=int, nargs="+", default=argparse.SUPPRESS, metavar="STEP",
                    help="after these steps' refinement: score the training cameras and prune by blending contribution "
                         "(prune.py)")
    ap.add_argument("--prune-min-score", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="rows whose score is below X go (default 0.01 with --prune-score max)")
    ap.add_argument("--prune-keep-fraction", type=float, default=argparse.SUPPRESS, metavar="F",
                    help="keep the best ceil(F N) rows instead")
    ap.add_argument("--prune-score", choices=("max", "sum"), default=argparse.SUPPRESS)
    ap.add_argument("--prune-view-stride", type=int, default=argparse.SUPPRESS, metavar="S", help="score every S-th camera")
    ap.add_argument("--grow-from-depth-every", type=int, default=argparse.SUPPRESS, metavar="K",
                    help="every K-th step: seed new Gaussians from the step's depth image where its camera's render has a "
                         "hole or lies behind the measurement (depth_grow.py); not with --camera-optimizer or "
                         "--relative-depth-loss")
    ap.add_argument("--grow-start", type=int, default=argparse.SUPPRESS, metavar="STEP",
                    help="the first step that may grow (default: the densifier's warmup_length, 500)")
    ap.add_argument("--grow-until", type=int, default=argparse.SUPPRESS, metavar="STEP",
                    help="growth stops at this step (default: the densifier's stop_split_at, 15000)")
    ap.add_argument("--grow-stride", type=int, default=argparse.SUPPRESS, metavar="S", help="look at every S-th pixel (default 2)")
    ap.add_argument("--grow-hole-alpha", type=float, default=argparse.SUPPRESS, metavar="A",
                    help="a pixel whose accumulated alpha is below A is a hole (default 0.5)")
    ap.add_argument("--grow-depth-tol", type=float, default=argparse.SUPPRESS, metavar="T",
                    help="the render is behind the measurement d beyond max(T, R d), T in model units (default 0)")
    ap.add_argument("--grow-depth-tol-rel", type=float, default=argparse.SUPPRESS, metavar="R", help="(default 0.05)")
    ap.add_argument("--grow-init-opacity", type=float, default=argparse.SUPPRESS, metavar="O",
                    help="the new Gaussians' opacity (default 0.5)")
    ap.add_argument("--grow-max-new", type=int, default=argparse.SUPPRESS, metavar="M",
                    help="at most M new Gaussians per growth, spread evenly over the candidates (default 50000)")
    ap.add_argument("--grow-max-gaussians", type=int, default=argparse.SUPPRESS, metavar="G",
                    help="growth never takes the model past G Gaussians (default: no limit)")
    return ap


def depth_config_of(a) -> Dict:
    """The model-config fields of the --depth-* options (the config's defaults where an option is absent)."""
    cfg = QEDSplatterModelConfig
    return {"depth_loss_type": str(getattr(a, "depth_loss_type", cfg.depth_loss_type)),
            "depth_huber_delta": float(getattr(a, "depth_huber_delta", cfg.depth_huber_delta)),
            "depth_tv_lambda": float(getattr(a, "depth_tv_lambda", cfg.depth_tv_lambda)),
            "depth_tv_edge_aware": not bool(getattr(a, "no_depth_tv_edge_aware", False))}


def depth_distortion_config_of(a) -> Dict:
    """The model-config fields of the --depth-distortion-* options (the config's defaults where an option is absent)."""
    cfg = QEDSplatterModelConfig
    return {"depth_distortion_lambda": float(getattr(a, "depth_distortion_lambda", cfg.depth_distortion_lambda)),
            "depth_distortion_from_step": int(getattr(a, "depth_distortion_from_step", cfg.depth_distortion_from_step))}


def relative_depth_config_of(a) -> Dict:
    """The model-config fields of the --relative-depth-* options (the config's defaults where an option is absent)."""
    cfg = QEDSplatterModelConfig
    return {"relative_depth_loss_type": str(getattr(a, "relative_depth_loss", cfg.relative_depth_loss_type)),
            "relative_depth_lambda": float(getattr(a, "relative_depth_lambda", cfg.relative_depth_lambda)),
            "relative_depth_space": str(getattr(a, "relative_depth_space", cfg.relative_depth_space)),
            "relative_depth_patch": int(getattr(a, "relative_depth_patch", cfg.relative_depth_patch)),
            "relative_depth_patch_min_valid": float(getattr(a, "relative_depth_min_valid",
                                                            cfg.relative_depth_patch_min_valid)),
            "relative_depth_patch_jitter": not bool(getattr(a, "no_relative_depth_jitter", False))}


def prune_config_of(a):
    """The PruneConfig of the --prune-* options (None without --prune-at)."""
    if not getattr(a, "prune_at", None):
        return None
    from .prune import PruneConfig
    score = getattr(a, "prune_score", "max")
    min_score, keep = getattr(a, "prune_min_score", None), getattr(a, "prune_keep_fraction", None)
    if min_score is not None and keep is not None:
        raise SystemExit("--prune-min-score and --prune-keep-fraction: give one")
    if min_score is None and keep is None and score != "max":
        raise SystemExit("--prune-score sum needs --prune-min-score or --prune-keep-fraction")
    return PruneConfig(score=score, min_score=0.01 if min_score is None else float(min_score), keep_fraction=keep)


def grow_config_of(a):
    """``(GrowConfig, every)`` of the --grow-* options, ``(None, 0)`` without --grow-from-depth-every.  The combinations
    depth_grow.grow refuses end the run here, when the arguments are parsed."""
    every = int(getattr(a, "grow_from_depth_every", 0) or 0)
    if every <= 0:
        if getattr(a, "grow_from_depth_every", None) is not None:
            raise SystemExit("--grow-from-depth-every: a positive number of steps")
        return None, 0
    if a.camera_optimizer != "off":
        raise SystemExit("--grow-from-depth-every with --camera-optimizer: the pose growth would back-project with is not "
                         "the one training renders with")
    if getattr(a, "relative_depth_loss", "off") != "off":
        raise SystemExit("--grow-from-depth-every with --relative-depth-loss: the depth files are then a prior of unknown "
                         "scale and cannot place a point")
    from .depth_grow import GrowConfig
    names = {"grow_stride": "stride", "grow_hole_alpha": "hole_alpha", "grow_depth_tol": "depth_tol",
             "grow_depth_tol_rel": "depth_tol_rel", "grow_init_opacity": "init_opacity", "grow_max_new": "max_new_per_view",
             "grow_max_gaussians": "max_gaussians"}
    try:
        return GrowConfig(**{field: getattr(a, opt) for opt, field in names.items() if hasattr(a, opt)}).validate(), every
    except ValueError as e:
        raise SystemExit(f"--grow-*: {e}")


def main(argv=None) -> Dict:
    a = build_parser().parse_args(argv)
    grow_config, grow_every = grow_config_of(a)
    color_corrected = bool(getattr(a, "color_corrected_metrics", False))
    output_normals = bool(getattr(a, "output_normals", False))
    if a.use_bilateral_grid:
        check_step_shape(*a.grid_shape)
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
                                    background_color=a.background_color, sh_degree=a.sh_degree,
                                    use_bilateral_grid=a.use_bilateral_grid, grid_shape=tuple(a.grid_shape),
                                    color_corrected_metrics=color_corrected,
                                    use_normal_loss=bool(getattr(a, "normal_loss", False)),
                                    normal_lambda=float(getattr(a, "normal_lambda", QEDSplatterModelConfig.normal_lambda)),
                                    use_normal_cosine_loss=bool(getattr(a, "normal_cosine_loss", False)),
                                    use_normal_consistency=bool(getattr(a, "normal_consistency", False)),
                                    normal_consistency_lambda=float(getattr(
                                        a, "normal_consistency_lambda", QEDSplatterModelConfig.normal_consistency_lambda)),
                                    normal_consistency_from_step=int(getattr(a, "normal_consistency_from", 0)),
                                    use_normal_tv=bool(getattr(a, "normal_tv", False)),
                                    normal_tv_lambda=float(getattr(a, "normal_tv_lambda",
                                                                   QEDSplatterModelConfig.normal_tv_lambda)),
                                    **depth_config_of(a), **relative_depth_config_of(a), **depth_distortion_config_of(a))
    from .losses import depth_terms, relative_depth_terms
    dterms = depth_terms(config)                 # (a refused combination ends the run before the model is built)
    rterms = relative_depth_terms(config)
    model = build_model(config, dm, a.init_from_ply, a.seed)
    print(f"seeded {model.num_points} Gaussians")
    trainer = Trainer(model, dm, seed=a.seed,
                      camera_opt_config=CameraOptimizerConfig(mode=a.camera_optimizer, lr=a.camera_opt_lr),
                      grow_config=grow_config, grow_every=grow_every, grow_start=getattr(a, "grow_start", None),
                      grow_until=getattr(a, "grow_until", None))
    if a.resume:
        trainer.resume(a.resume)
        print(f"resumed {a.resume} at step {trainer.step} with {trainer.model.num_points} Gaussians")
    metrics: Dict[str, float] = {}
    prune_config, prune_log = prune_config_of(a), []
    first = trainer.step
    torch.cuda.synchronize()
    t0 = time.time()
    losses = None
    while trainer.step < a.steps:
        losses = trainer.train_step()
        if prune_config is not None and trainer.step - 1 in a.prune_at:
            info = trainer.prune(prune_config, int(getattr(a, "prune_view_stride", 1)))
            prune_log.append({"step": trainer.step - 1, "n_before": info["n_before"], "n_after": info["n_after"],
                              "seconds": info["seconds"]})
            print(f"step {trainer.step - 1}: pruned {info['n_pruned']} of {info['n_before']} Gaussians", flush=True)
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
    if getattr(a, "export_pointcloud", None):
        cloud = trainer.export_pointcloud(a.export_pointcloud, a.export_frame)
        print(f"exported a surface cloud of {len(cloud)} points to {a.export_pointcloud} ({a.export_frame} frame)")
    done = trainer.step - first
    result = {"steps": trainer.step, "steps_per_s": done / elapsed if elapsed > 0 and done else 0.0,
              "eval": metrics, "gaussian_count": trainer.model.num_points}
    if prune_config is not None:
        result["prune"] = prune_log
    if grow_every:
        result["grown"] = dict(trainer.grown)
    if trainer.camera_optimizer is not None:
        result["camera_opt"] = trainer.camera_opt_metrics()
    if trainer.grid_optimizer is not None:
        result["tv_loss"] = float(losses["tv_loss"]) if losses is not None else None
    if config.use_normal_loss:
        result["normal_loss"] = float(losses["normal_loss"]) if losses is not None else None
    for flag, key in ((config.use_normal_consistency, "normal_consistency_loss"), (config.use_normal_tv, "normal_tv_loss")):
        if flag:                                 # (None: no step carried the term, e.g. all before --normal-consistency-from)
            result[key] = float(losses[key]) if (losses is not None and key in losses) else None
    if dterms is not None:
        result["depth_loss"] = float(losses["depth_loss"]) if losses is not None else None
        if dterms.tv_lambda > 0.0:
            result["depth_tv_loss"] = float(losses["depth_tv_loss"]) if losses is not None else None
    if rterms is not None:
        # (depth_pearson, in the configured space: the evaluation split's mean; the training cameras' where that split is empty)
        result["relative_depth_loss"] = float(losses["relative_depth_loss"]) if losses is not None else None
        result["depth_pearson"] = metrics["depth_pearson"] if "depth_pearson" in metrics else trainer.depth_pearson()
    if config.depth_distortion_lambda > 0.0:     # (None: no step carried the term, e.g. all before --depth-distortion-from-step)
        key = "depth_distortion_loss"
        result[key] = float(losses[key]) if (losses is not None and key in losses) else None
    if output_normals:
        trainer.model.config.output_normals = True      # (from here on: the final evaluation and --render-eval only)
    output_spread = bool(getattr(a, "output_depth_spread", False))
    if output_spread:
        trainer.model.config.output_depth_spread = True
    if color_corrected or output_normals or output_spread:
        result["eval_images"] = trainer.evaluate_images()
    if a.save_poses:
        result["save_poses"] = trainer.save_poses(a.save_poses, a.data)
        print(f"wrote {result['save_poses']} training poses to {a.save_poses}")
    if a.render_eval:
        from .render import EXTRA_PLANES, PLANES, SPREAD_PLANES, dataset_path, render_to_directory
        unit = float(dm.outputs.dataparser_scale) * float(dm.outputs.depth_unit_scale_factor)
        result["render_eval"] = render_to_directory(trainer.model, dataset_path(dm, "eval"), a.render_eval, depth_unit=unit,
                                                    planes=PLANES + (EXTRA_PLANES if output_normals else ())
                                                    + (SPREAD_PLANES if output_spread else ()))
        print(f"rendered {result['render_eval']['frames']} evaluation views to {a.render_eval}")
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
