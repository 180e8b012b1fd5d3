"""A trained model to an oriented, coloured surface point cloud: rendered depth and rendered normals of every camera
back-projected, filtered and merged on a voxel grid -- the product a Poisson tool meshes and ``pointcloud_metrics`` scores.

    python -m qed_splatter_amd.surface_cloud --load CKPT --data DIR --output PLY [--voxel-size V --stride S ...]

Per view ONE call of ``qed_surface_samples`` (csrc/surface.hip) turns the planes ``get_outputs`` returns in evaluation mode
with ``config.output_normals`` into a compact list of world points, normals and colours.  include/qed_splat.h states the
definition; in short, for every ``stride``-th pixel, in this order: alpha >= min_alpha (and the mask); z = depth / alpha
finite inside [depth_min, depth_max]; the chosen normal (rendered, or the depth map's) valid; where both normals are valid,
the angle between them at most ``max_normal_angle_deg``; P = ((x + .5 - cx) z / fx, (y + .5 - cy) z / fy, z) -- the
renderer's pixel centres, as normals.py, NOT the integer pixels of ``init_pointcloud.backproject_depth``; the normal within
``min_view_cos`` of facing the camera; world point R^T (P - t), world normal R^T n.

The views are merged with ``qed_voxel_down_sample_attr`` (csrc/voxel.hip): per occupied voxel the WEIGHTED mean of the
positions, normals and colours of its members and the sum of their weights (a fresh sample weighs 1).  The mean of a
voxel's members lies in that voxel, so with one voxel size merging clouds that were down-sampled already equals
down-sampling everything at once, up to rounding: ``export_pointcloud`` merges in ``init_pointcloud``'s pairwise tree and
down-samples whenever a concatenation grows past ``max_rows_in_flight``.  Normals ride as a linear attribute and are
normalised once, at the end (a voxel whose normals cancel is dropped).

The filters and the weighted merge are THIS PROJECT'S definitions, in the spirit of DN-Splatter's / AGS-Mesh's
back-projection of rendered depth and normals; they are not checked against those projects and are not in the reference.
Meshing (Poisson, TSDF) is out of scope: hand the PLY (x y z, nx ny nz, red green blue) to any tool that does it.
"""
from __future__ import annotations

import argparse
import json
import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L

NORMAL_SOURCES = {"rendered": L.SURFACE_NORMAL_RENDERED, "depth": L.SURFACE_NORMAL_DEPTH}
N_ATTRS = 6                     # what a cloud carries through the merge beside its positions: normal, colour


@dataclass
class SurfaceCloud:
    """``points`` [n,3], ``normals`` [n,3], ``colors`` [n,3] (the render's float values) and ``weights`` [n] (the number
    of samples a point stands for), float32 tensors on one device."""
    points: Tensor
    normals: Tensor
    colors: Tensor
    weights: Tensor

    def __len__(self) -> int:
        return int(self.points.shape[0])

    def to_dataset_frame(self, fc) -> "SurfaceCloud":
        """The cloud moved through ``gaussian_ply.frame_change(..., inverse=True)``'s similarity p' = s (R p + t):
        points get scale, rotation and translation, normals the rotation only; float64 arithmetic, rounded once."""
        dev = self.points.device
        R = torch.from_numpy(np.asarray(fc.R, np.float64)).to(dev)
        t = torch.from_numpy(np.asarray(fc.t, np.float64)).to(dev)
        points = (float(fc.s) * (self.points.double() @ R.T + t)).to(torch.float32)
        normals = (self.normals.double() @ R.T).to(torch.float32)
        return SurfaceCloud(points, normals, self.colors, self.weights)

    def colors_u8(self) -> np.ndarray:
        """uint8 [n,3] on the host: round(255 c) (half to even) clamped to 0 .. 255."""
        c = self.colors.detach().double().cpu().numpy()
        return np.clip(np.rint(255.0 * c), 0.0, 255.0).astype(np.uint8)

    def write_ply(self, path) -> None:
        """Binary PLY: x y z, nx ny nz (float), red green blue (uchar)."""
        from .init_pointcloud import write_ply
        write_ply(path, self.points.detach().cpu().numpy(), self.colors_u8(), normals=self.normals.detach().cpu().numpy())


def _empty_cloud(device) -> SurfaceCloud:
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
    return SurfaceCloud(z(0, 3), z(0, 3), z(0, 3), z(0))


def _plane(t: Tensor, name: str, numel: int, dtype=torch.float32) -> Tensor:
    if not torch.is_tensor(t) or t.dtype != dtype or t.numel() != numel:
        raise ValueError(f"{name}: a {dtype} tensor of {numel} values")
    if not t.is_cuda:
        raise L.QedSplatError(f"{name} must live on the GPU: the surface kernels have no CPU path")
    return t.detach().contiguous()


def cos_max_normal_angle(max_normal_angle_deg: Optional[float]) -> float:
    """The agreement filter's threshold as the kernel takes it: cos of the angle as a float32 value, -2 (off) for None."""
    if max_normal_angle_deg is None:
        return -2.0
    return float(np.float32(math.cos(math.radians(float(max_normal_angle_deg)))))


@torch.no_grad()
def surface_samples(rgb: Tensor, depth: Tensor, alpha: Tensor, normal: Tensor, depth_normal: Tensor, valid: Tensor,
                    viewmat: Tensor, intrinsics: Sequence[float], *, mask: Optional[Tensor] = None, stride: int = 1,
                    min_alpha: float = 0.5, depth_min: float = 0.0, depth_max: float = math.inf,
                    normals: str = "rendered", max_normal_angle_deg: Optional[float] = None, min_view_cos: float = 0.0,
                    capacity: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """qed_surface_samples on one view's planes -> (points, normals, colors), each [n,3], in row-major pixel order.
    ``depth``: the ACCUMULATED depth, [H,W(,1)] or any evenly strided view (``render[..., 3]``); ``viewmat`` [4,4]: the
    OpenCV world-to-camera matrix on the device; ``intrinsics``: (fx, fy, cx, cy) host floats.  ``capacity``: rows to
    allocate (default: every strided pixel); more samples than that raise.  One host read (the count and the status)."""
    from .normals import _strided_plane
    if normals not in NORMAL_SOURCES:
        raise ValueError(f"normals {normals!r}: 'rendered' or 'depth'")
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    n_pix = H * W
    rgb = _plane(rgb, "rgb", 3 * n_pix)
    alpha = _plane(alpha, "alpha", n_pix)
    normal = _plane(normal, "normal", 3 * n_pix)
    depth_normal = _plane(depth_normal, "depth_normal", 3 * n_pix)
    valid = _plane(valid, "valid", n_pix, torch.uint8)
    viewmat = _plane(viewmat, "viewmat", 16)
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.to(torch.uint8)
        mask = _plane(mask.to(rgb.device), "mask", n_pix, torch.uint8)
    depth, depth_stride = _strided_plane(depth, H, W)
    dev = rgb.device
    lib = L.load()
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be at least 1")
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    cap = ((W + stride - 1) // stride) * ((H + stride - 1) // stride) if capacity is None else int(capacity)
    out = torch.empty(3, max(cap, 1), 3, dtype=torch.float32, device=dev)
    meta = torch.zeros(1 + L.STATUS_WORDS, dtype=torch.int32, device=dev)            # n_out, status[4]
    if n_pix == 0:
        return out[0, :0], out[1, :0], out[2, :0]
    ws_ints = int(lib.qed_surface_workspace_ints(H, W, stride))
    if ws_ints < 0:
        raise L.QedSplatError(f"surface_samples: a {H}x{W} image is more than one call takes")
    work = torch.empty(ws_ints, dtype=torch.int32, device=dev)
    L.check(lib.qed_surface_samples(H, W, L.ptr(rgb), L.ptr(depth), depth_stride, L.ptr(alpha), L.ptr(normal),
                                    L.ptr(depth_normal), L.ptr(valid), L.ptr(mask), fx, fy, cx, cy, L.ptr(viewmat), stride,
                                    float(min_alpha), float(depth_min), float(depth_max), NORMAL_SOURCES[normals],
                                    cos_max_normal_angle(max_normal_angle_deg), float(min_view_cos), cap, L.ptr(out[0]),
                                    L.ptr(out[1]), L.ptr(out[2]), L.ptr(meta), L.ptr(work), ws_ints, L.ptr(meta[1:]),
                                    L.current_stream()), "qed_surface_samples")
    n, needed = (int(v) for v in meta[:2].tolist())
    if needed:
        raise L.QedSplatError(f"surface_samples: {needed} samples do not fit the capacity of {cap} rows")
    return out[0, :n], out[1, :n], out[2, :n]


def camera_viewmat(camera, device) -> Tensor:
    """The OpenCV world-to-camera matrix [4,4] (float32, on ``device``) of a one-camera object, formed on the device."""
    from .model import get_viewmat
    c2w = camera.camera_to_worlds
    if c2w.shape[0] != 1:
        raise ValueError("one camera at a time")
    return get_viewmat(c2w.detach().to(device, torch.float32))[0].contiguous()


def _camera_intrinsics(outputs: Dict, camera) -> Tuple[float, float, float, float]:
    intr = getattr(outputs.get("normal"), "_qed_intrinsics", None)          # (get_outputs read them back already)
    if intr is not None:
        return tuple(float(v) for v in intr)
    return tuple(float(getattr(camera, k).reshape(-1)[0]) for k in ("fx", "fy", "cx", "cy"))


@torch.no_grad()
def frame_surface_samples(outputs: Dict, camera, *, stride: int = 1, min_alpha: float = 0.5, depth_min: float = 0.0,
                          depth_max: float = math.inf, normals: str = "rendered",
                          max_normal_angle_deg: Optional[float] = None, min_view_cos: float = 0.0,
                          mask: Optional[Tensor] = None, max_depth_std: Optional[float] = None) -> SurfaceCloud:
    """The oriented samples of ONE view, a single launch sequence on the planes as they are: ``outputs`` is what
    ``get_outputs(camera)`` returned in evaluation mode with ``config.output_normals`` (rgb, depth, accumulation, normal,
    depth_normal, normal_valid).  Every sample weighs 1.  ``max_depth_std`` (model units; None: no filter, the call is
    what it was): pixels whose ``outputs["depth_std"]`` (config.output_depth_spread: the standard deviation of the depth along
    the ray, depth_distortion.py) exceeds it -- or is not a number -- are dropped AHEAD of qed_surface_samples, through its
    mask plane, so the compact list is written without them."""
    missing = [k for k in ("rgb", "depth", "accumulation", "normal", "depth_normal", "normal_valid") if outputs.get(k) is None]
    if missing:
        raise ValueError(f"frame_surface_samples: outputs lack {missing}: render in evaluation mode with config.output_normals")
    rgb = outputs["rgb"]
    if not rgb.is_cuda:
        raise L.QedSplatError("frame_surface_samples needs GPU tensors: there is no CPU path in the product")
    if max_depth_std is not None:
        std = outputs.get("depth_std")
        if std is None:
            raise ValueError("frame_surface_samples(max_depth_std=...): outputs lack 'depth_std': render with "
                             "config.output_depth_spread")
        if not float(max_depth_std) >= 0.0:
            raise ValueError(f"max_depth_std must be a number >= 0, got {max_depth_std}")
        keep = std.reshape(rgb.shape[0], rgb.shape[1]) <= float(max_depth_std)
        if mask is not None:
            keep = keep & (mask.to(rgb.device).reshape(keep.shape) != 0)
        mask = keep.to(torch.uint8)
    points, nrm, colors = surface_samples(
        rgb, outputs["depth"], outputs["accumulation"], outputs["normal"], outputs["depth_normal"], outputs["normal_valid"],
        camera_viewmat(camera, rgb.device), _camera_intrinsics(outputs, camera), mask=mask, stride=stride,
        min_alpha=min_alpha, depth_min=depth_min, depth_max=depth_max, normals=normals,
        max_normal_angle_deg=max_normal_angle_deg, min_view_cos=min_view_cos)
    return SurfaceCloud(points, nrm, colors, torch.ones(points.shape[0], dtype=torch.float32, device=points.device))


@torch.no_grad()
def voxel_down_sample_attr(points: Tensor, attrs: Tensor, weights: Optional[Tensor], voxel_size: float,
                           return_dropped: bool = False):
    """qed_voxel_down_sample_attr -> (points [m,3], attrs [m,K], weights [m]): per occupied voxel the weighted means and
    the weight sum, in ascending (ix, iy, iz) order.  ``attrs`` [n,K] with 1 <= K <= 8; ``weights`` [n] or None (all 1).
    Rows with a non-finite value or a weight <= 0 are dropped; ``return_dropped`` adds their number as a fourth result.
    One host read (the count and the status words)."""
    if not (torch.is_tensor(points) and points.is_cuda):
        raise L.QedSplatError("voxel_down_sample_attr needs GPU tensors: there is no CPU path")
    if points.dim() != 2 or points.shape[1] != 3 or attrs.dim() != 2 or attrs.shape[0] != points.shape[0]:
        raise ValueError("points [n,3], attrs [n,K]")
    K = int(attrs.shape[1])
    if not 1 <= K <= L.VOXEL_MAX_ATTRS:
        raise ValueError(f"attrs: 1 to {L.VOXEL_MAX_ATTRS} columns, got {K}")
    lib = L.load()
    dev = points.device
    pts = points.detach().to(torch.float32).contiguous()
    att = attrs.detach().to(device=dev, dtype=torch.float32).contiguous()
    wts = None
    if weights is not None:
        wts = weights.detach().to(device=dev, dtype=torch.float32).contiguous()
        if wts.shape != (pts.shape[0],):
            raise ValueError("weights [n]")
    n = int(pts.shape[0])
    out_p = torch.empty(n, 3, dtype=torch.float32, device=dev)
    out_a = torch.empty(n, K, dtype=torch.float32, device=dev)
    out_w = torch.empty(n, dtype=torch.float32, device=dev)
    meta = torch.zeros(1 + L.STATUS_WORDS, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.qed_voxel_attr_workspace_bytes(n, K))
    if ws_bytes < 0:
        raise L.QedSplatError(f"voxel_down_sample_attr: {n} points are more than one call takes (2^30)")
    work = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=dev)
    L.check(lib.qed_voxel_down_sample_attr(n, L.ptr(pts), K, L.ptr(att), L.ptr(wts), float(voxel_size), L.ptr(out_p),
                                           L.ptr(out_a), L.ptr(out_w), L.ptr(meta), L.ptr(work), work.numel() * 8,
                                           L.ptr(meta[1:]), L.current_stream()), "qed_voxel_down_sample_attr")
    n_out, refused, n_dropped, span, _ = (int(v) for v in meta.tolist())
    if refused:
        raise L.QedSplatError(f"voxel_down_sample_attr: the cloud spans {span} voxels of {float(voxel_size):g} on one "
                              f"axis; at most 2^21 = {1 << 21} are supported")
    keep = (lambda t: t[:n_out].clone()) if 2 * n_out < n else (lambda t: t[:n_out])
    res = (keep(out_p), keep(out_a), keep(out_w))
    return res + (n_dropped,) if return_dropped else res


# ---- the merge: a cloud travels as ONE [n, 10] tensor (x y z | nx ny nz | r g b | weight) through init_pointcloud's tree ----
def _pack(cloud: SurfaceCloud) -> Tensor:
    return torch.cat([cloud.points, cloud.normals, cloud.colors, cloud.weights[:, None]], dim=1)


def _unpack(packed: Tensor) -> SurfaceCloud:
    return SurfaceCloud(packed[:, 0:3].contiguous(), packed[:, 3:6].contiguous(), packed[:, 6:9].contiguous(),
                        packed[:, 9].contiguous())


def _down_sample_packed(packed: Tensor, voxel_size: float) -> Tensor:
    p, a, w = voxel_down_sample_attr(packed[:, 0:3], packed[:, 3:3 + N_ATTRS], packed[:, 3 + N_ATTRS], voxel_size)
    return torch.cat([p, a, w[:, None]], dim=1)


def merge_clouds(clouds, voxel_size: float, max_rows_in_flight: int = 4_000_000) -> SurfaceCloud:
    """``clouds`` (an iterable of SurfaceCloud) through ``init_pointcloud.tree_merge_pointclouds`` -- a concatenation of
    more than ``max_rows_in_flight`` rows is down-sampled on the spot -- and one final down-sample: one row per occupied
    voxel, normals NOT yet normalised.  No clouds: an empty cloud on the current device."""
    from .init_pointcloud import NoCloudsError, tree_merge_pointclouds
    try:
        merged = tree_merge_pointclouds((_pack(c) for c in clouds), voxel_size=voxel_size, max_points=int(max_rows_in_flight),
                                        down_sample_fn=_down_sample_packed)
    except NoCloudsError:
        return _empty_cloud(torch.device("cuda", torch.cuda.current_device()))
    return _unpack(_down_sample_packed(merged, voxel_size))


def finish_cloud(cloud: SurfaceCloud, min_samples: float = 1) -> SurfaceCloud:
    """Voxels lighter than ``min_samples`` dropped; then the normals normalised (in float64, rounded once), a voxel whose
    normals sum to zero dropped."""
    keep = cloud.weights >= float(min_samples)
    n64 = cloud.normals.double()
    length = n64.norm(dim=1)
    keep = keep & (length > 0) & torch.isfinite(length)
    unit = (n64 / length.clamp_min(1e-300)[:, None]).to(torch.float32)
    return SurfaceCloud(cloud.points[keep], unit[keep], cloud.colors[keep], cloud.weights[keep])


def export_pointcloud(model, cameras, path=None, *, voxel_size: float, stride: int = 1, min_alpha: Optional[float] = None,
                      depth_min: float = 0.0, depth_max: float = math.inf, normals: str = "rendered",
                      max_normal_angle_deg: Optional[float] = None, min_view_cos: float = 0.0, min_samples: float = 1,
                      max_rows_in_flight: int = 4_000_000, frame: str = "model", dataparser_transform=None,
                      dataparser_scale: float = 1.0, max_depth_std: Optional[float] = None) -> SurfaceCloud:
    """``max_depth_std`` (None: off): ``config.output_depth_spread`` is forced on for the run as well and every view drops the
    pixels whose depth standard deviation along the ray exceeds it (``frame_surface_samples``).  The whole export: every camera through ``model.get_outputs`` (evaluation mode, no gradients, ``output_normals``
    forced on for the run and restored afterwards; ``model.crop_box`` applies) and ``frame_surface_samples``; the views
    merged on the voxel grid (``merge_clouds``); voxels of fewer than ``min_samples`` samples dropped; normals
    normalised; ``frame="dataset"``: moved back through ``dataparser_transform`` / ``dataparser_scale`` (refused without
    the transform); written to ``path`` as a PLY when one is given.  ``min_alpha`` None: ``config.normals_min_alpha``."""
    from .render import _on_device
    if frame not in ("model", "dataset"):
        raise ValueError(f"frame must be 'model' or 'dataset', got {frame!r}")
    if normals not in NORMAL_SOURCES:
        raise ValueError(f"normals {normals!r}: 'rendered' or 'depth'")
    if not (float(voxel_size) > 0.0 and math.isfinite(float(voxel_size))):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    fc = None
    if frame == "dataset":
        from .gaussian_ply import frame_change
        if dataparser_transform is None:
            raise ValueError("frame='dataset' needs the dataparser_transform (and dataparser_scale) the model was trained under")
        fc = frame_change(dataparser_transform, dataparser_scale, inverse=True)
    device = torch.device(model.device)
    if device.type != "cuda":
        raise L.QedSplatError("export_pointcloud needs a model on the GPU: there is no CPU path in the product")
    L.load()
    if min_alpha is None:
        min_alpha = float(model.config.normals_min_alpha)
    was_training = model.training
    had_normals = bool(getattr(model.config, "output_normals", False))
    had_spread = bool(getattr(model.config, "output_depth_spread", False))
    model.eval()
    model.config.output_normals = True
    if max_depth_std is not None:
        model.config.output_depth_spread = True

    def frame_clouds():
        for cam in cameras:
            cam = _on_device(cam, device)
            outputs = model.get_outputs(cam)
            if outputs.get("normal") is None:             # (a crop box that leaves no Gaussian: an empty frame)
                continue
            cloud = frame_surface_samples(outputs, cam, stride=stride, min_alpha=min_alpha, depth_min=depth_min,
                                          depth_max=depth_max, normals=normals, max_normal_angle_deg=max_normal_angle_deg,
                                          min_view_cos=min_view_cos, max_depth_std=max_depth_std)
            if len(cloud):
                yield cloud

    try:
        with torch.no_grad(), torch.cuda.device(device):
            cloud = finish_cloud(merge_clouds(frame_clouds(), float(voxel_size), max_rows_in_flight), min_samples)
            if fc is not None:
                cloud = cloud.to_dataset_frame(fc)
    finally:
        model.train(was_training)
        model.config.output_normals = had_normals
        model.config.output_depth_spread = had_spread
    if path is not None:
        cloud.write_ply(path)
    return cloud


# ---- the command line -----------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    from .render import add_dataparser_arguments
    ap = argparse.ArgumentParser(prog="python -m qed_splatter_amd.surface_cloud",
                                 description="Export an oriented, coloured surface point cloud of a trained model (PLY).")
    ap.add_argument("--load", required=True, metavar="CKPT", help="a checkpoint written by train.py --save")
    ap.add_argument("--data", required=True, metavar="DIR", help="dataset directory (its cameras are the views)")
    ap.add_argument("--output", required=True, metavar="PLY")
    ap.add_argument("--split", choices=("train", "eval", "all"), default="all")
    ap.add_argument("--voxel-size", type=float, default=0.01, help="voxel size of the merge, in the model's units")
    ap.add_argument("--stride", type=int, default=1, help="use every stride-th pixel in x and y")
    ap.add_argument("--min-alpha", type=float, default=None, help="default: the model's normals_min_alpha (0.5)")
    ap.add_argument("--depth-max", type=float, default=math.inf, help="largest surface depth that is used (model units)")
    ap.add_argument("--normals", choices=tuple(NORMAL_SOURCES), default="rendered",
                    help="the normal a sample carries: the rendered normal map, or the rendered depth map's normals")
    ap.add_argument("--max-normal-angle", type=float, default=None, metavar="DEG",
                    help="drop pixels whose rendered normal and depth normal differ by more than this")
    ap.add_argument("--min-view-cos", type=float, default=0.0, metavar="C",
                    help="drop pixels seen at a grazing angle: -dot(normal, view direction) below this")
    ap.add_argument("--max-depth-std", type=float, default=None, metavar="V",
                    help="drop pixels whose blending weights are spread along the ray by more than this standard deviation of "
                         "the depth, in the model's units (depth_distortion.py; default: no filter)")
    ap.add_argument("--min-samples", type=float, default=1, metavar="K", help="drop voxels that hold fewer samples")
    ap.add_argument("--frame", choices=("model", "dataset"), default="model",
                    help="'dataset': undo the dataparser's orientation, centring and scale")
    ap.add_argument("--downscale", type=float, default=1.0, help="render at 1 / D of the cameras' size")
    ap.add_argument("--crop", type=float, nargs=9, default=None, metavar="V",
                    help="cx cy cz  roll pitch yaw  sx sy sz: an oriented box in the model's frame; Gaussians outside are left out")
    ap.add_argument("--gt", metavar="PLY", default=None, help="also print PDMetrics of the export against this cloud")
    add_dataparser_arguments(ap)
    return ap


def main(argv=None) -> dict:
    a = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("qed_splatter_amd.surface_cloud needs a GPU")
    from .datamanager import FullImageDatamanager
    from .dataparser import DataparserConfig
    from .render import OrientedBox, dataset_path, load_model
    L.load()
    device = torch.device("cuda:0")
    model, ckpt = load_model(a.load, device)
    if a.frame == "dataset" and "dataparser_transform" not in ckpt:
        raise SystemExit(f"{a.load} stores no dataparser_transform (saved by an older trainer): only --frame model")
    if a.crop is not None:
        model.crop_box = OrientedBox(a.crop[0:3], a.crop[3:6], a.crop[6:9])
    dp_cfg = DataparserConfig(orientation_method=a.orientation_method, center_method=a.center_method,
                              auto_scale_poses=a.auto_scale_poses == "True",
                              depth_unit_scale_factor=a.depth_unit_scale_factor,
                              train_split_fraction=a.train_split_fraction, scale_factor=a.scale_factor,
                              undistort=a.undistort)
    dm = FullImageDatamanager(a.data, dp_cfg, device=a.cache_device)
    scale = float(dm.outputs.dataparser_scale)
    if "dataparser_scale" in ckpt and abs(float(ckpt["dataparser_scale"]) - scale) > 1e-6 * abs(scale):
        raise SystemExit(f"the checkpoint was trained with dataparser_scale {ckpt['dataparser_scale']}, these dataparser "
                         f"options give {scale}: pass the options of the training run")
    cameras = dataset_path(dm, a.split)
    if a.downscale != 1.0:
        for cam in cameras:
            cam.rescale_output_resolution(1.0 / a.downscale)
    cloud = export_pointcloud(model, cameras, a.output, voxel_size=a.voxel_size, stride=a.stride, min_alpha=a.min_alpha,
                              depth_max=a.depth_max, normals=a.normals, max_normal_angle_deg=a.max_normal_angle,
                              min_view_cos=a.min_view_cos, min_samples=a.min_samples, frame=a.frame,
                              dataparser_transform=ckpt.get("dataparser_transform"),
                              dataparser_scale=float(ckpt.get("dataparser_scale", 1.0)), max_depth_std=a.max_depth_std)
    result = {"output": str(a.output), "points": len(cloud), "views": len(cameras), "frame": a.frame,
              "voxel_size": a.voxel_size}
    if a.gt is not None:
        from .init_pointcloud import read_ply_positions
        from .pointcloud_metrics import pd_metrics
        result["pd_metrics"] = pd_metrics(read_ply_positions(a.output), read_ply_positions(a.gt))
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
