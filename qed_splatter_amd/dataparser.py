"""A dataset directory as the reference's trainer sees it: the Nerfstudio dataparser the reference configures
(``dataparser.py``, ``config.py:36``), for ``transforms.json`` datasets with one depth map per image.

Nerfstudio is not a dependency of this package and is not installed where this was written: the definitions below
(the frame order, the train / eval split, ``auto_orient_and_center_poses`` for the methods offered, the auto-scale) are
RESTATED FROM MEMORY of nerfstudio 1.1.x, not checked against it.  Each is written out in the docstring of the function
that implements it, and tests/test_dataparser_cpu.py pins the stated properties.

Distorted cameras.  By default a file or frame with non-zero ``k1 k2 k3 k4 p1 p2``, or with ``camera_model:
OPENCV_FISHEYE``, is refused.  With ``DataparserConfig.undistort`` such cameras are accepted: ``fx fy cx cy`` then hold
the NEW pinhole ``K'`` (``undistort.optimal_new_intrinsics`` of the file's values; the distortion model, ``K'`` and the
resampling are defined in undistort.py), ``src_intrinsics`` / ``distortion_params`` / ``camera_models`` keep the file's,
and the datamanager resamples every such frame on the GPU before it enters the cache (csrc/undistort.hip).  The output
has the size of the input.  Two deviations from nerfstudio, which only crops the depth map (leaving it distorted) and
blends masks before testing non-zero: here depth and mask are resampled with the nearest tap through the same map as
the colour, so that a depth value supervises the pixel it belongs to.

Not offered: the other camera models, ``k4`` with OPENCV, tangential coefficients with the fisheye, resizing of depth
images, the other orientation / centre methods, the other split modes.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch
from torch import Tensor

from .init_pointcloud import frame_intrinsics, load_transforms
from .undistort import (DISTORTION_KEYS, check_coefficients, distort_points, is_distorted,  # noqa: F401 (public here too)
                        optimal_new_intrinsics, undistort_points)

CAMERA_MODELS = (None, "OPENCV", "PINHOLE")


@dataclass
class DataparserConfig:
    """The fields of the reference's dataparser configuration that are offered, with its defaults.  (The reference's
    README tells its users to set ``orientation_method``, ``center_method`` to "none" and ``auto_scale_poses`` to False.)"""
    orientation_method: str = "up"           # "up" | "none"
    center_method: str = "poses"             # "poses" | "none"
    auto_scale_poses: bool = True
    scale_factor: float = 1.0
    train_split_fraction: float = 0.9
    depth_unit_scale_factor: float = 0.001   # integer depth files are in millimetres
    undistort: bool = False                  # accept distorted OPENCV / OPENCV_FISHEYE cameras (see the module docstring)


@dataclass
class DataparserOutputs:
    """All frames of the dataset that have a depth map, sorted by ``file_path``; ``i_train`` / ``i_eval`` index them."""
    image_filenames: List[Path]
    depth_filenames: List[Path]
    mask_filenames: List[Optional[Path]]
    camera_to_worlds: Tensor                 # [n,3,4] float32, OpenGL, AFTER the dataparser transform and scale
    fx: np.ndarray
    fy: np.ndarray
    cx: np.ndarray
    cy: np.ndarray
    widths: np.ndarray
    heights: np.ndarray
    i_train: np.ndarray
    i_eval: np.ndarray
    dataparser_transform: Tensor             # [3,4] float32: world -> the frame the cameras are in (before the scale)
    dataparser_scale: float
    depth_unit_scale_factor: float
    n_skipped: int = 0                       # frames without depth_file_path
    # The seed cloud, in the frame of the json's poses: ``qed-init-pc`` back-projects with the frames' transform_matrix, and
    # ns-process-data writes sparse_pc.ply with applied_transform already applied, as it does the poses.  So the points
    # move exactly as the cameras do: from_ply(cfg, ply_file_path, dataparser_transform, dataparser_scale).  (The json's
    # applied_transform only matters for mapping results back to the ORIGINAL coordinates; nothing here does that.)
    ply_file_path: Optional[Path] = None
    config: DataparserConfig = field(default_factory=DataparserConfig)
    # With ``undistort``: the file's (fx, fy, cx, cy) [n,4] and (k1, k2, k3, k4, p1, p2) [n,6] and camera_model of every
    # frame, while fx fy cx cy above are the new pinhole's.  None without ``undistort``.
    src_intrinsics: Optional[np.ndarray] = None
    distortion_params: Optional[np.ndarray] = None
    camera_models: Optional[List[Optional[str]]] = None
    # camera_to_worlds [n,3,4] and dataparser_transform [3,4] before their rounding to float32: what maps poses back to the
    # dataset's own frame (train.py --save-poses) without the float32 rounding of the translations
    camera_to_worlds_f64: Optional[np.ndarray] = None
    dataparser_transform_f64: Optional[np.ndarray] = None
    # Per frame the class map of semantic.py (``label_path``: an 8-bit single-channel PNG of the frame's size, value = class,
    # 255 = unlabelled) or None; None for the whole dataset when no frame has one.
    label_filenames: Optional[List[Optional[Path]]] = None

    def __len__(self) -> int:
        return len(self.image_filenames)


def split_indices(n: int, train_split_fraction: float = 0.9):
    """Nerfstudio's "fraction" split: ``n_train = ceil(n * fraction)`` frames at ``linspace(0, n - 1, n_train)``
    truncated to int train, the rest evaluate.  -> (i_train, i_eval), both ascending."""
    n_train = int(math.ceil(n * train_split_fraction))
    i_all = np.arange(n)
    i_train = np.linspace(0, n - 1, n_train, dtype=int)
    return i_train, np.setdiff1d(i_all, i_train)


def rotation_between(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The rotation that takes direction ``a`` onto direction ``b`` about their common normal (Rodrigues).  Parallel:
    the identity.  Antiparallel: a half turn about x."""
    a = a / np.linalg.norm(a)
    b = b / np.linalg.norm(b)
    v = np.cross(a, b)
    c = float(np.dot(a, b))
    if c > 1.0 - 1e-12:
        return np.eye(3)
    if c < -1.0 + 1e-12:
        return np.diag([1.0, -1.0, -1.0])
    vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + vx + vx @ vx / (1.0 + c)


def orient_and_center(c2w: np.ndarray, orientation_method: str = "up", center_method: str = "poses"):
    """``auto_orient_and_center_poses`` for the methods offered.  c2w [n,4,4] or [n,3,4] float64 -> (new c2w [n,3,4],
    transform [3,4]) with ``new = transform @ c2w``:
      * centre ``t`` = the mean camera origin ("poses") or 0 ("none");
      * "up": ``R`` = rotation_between(normalised mean of the cameras' y axes c2w[:, :3, 1], (0, 0, 1)); "none": identity;
      * ``transform = [R | R (-t)]``."""
    if orientation_method not in ("up", "none"):
        raise NotImplementedError(f"orientation_method {orientation_method!r}: only 'up' and 'none' are offered")
    if center_method not in ("poses", "none"):
        raise NotImplementedError(f"center_method {center_method!r}: only 'poses' and 'none' are offered")
    n = c2w.shape[0]
    full = np.zeros((n, 4, 4))
    full[:, :3] = c2w[:, :3]
    full[:, 3, 3] = 1.0
    t = full[:, :3, 3].mean(axis=0) if center_method == "poses" else np.zeros(3)
    R = np.eye(3)
    if orientation_method == "up":
        R = rotation_between(full[:, :3, 1].mean(axis=0), np.array([0.0, 0.0, 1.0]))
    transform = np.concatenate([R, (R @ -t)[:, None]], axis=1)
    return transform @ full, transform


def _check_undistorted(meta: dict, where: str) -> None:
    model = meta.get("camera_model")
    if model not in CAMERA_MODELS:
        raise NotImplementedError(f"{where}: camera_model {model!r}: undistortion is not supported (only undistorted "
                                  "OPENCV / PINHOLE cameras)")
    bad = [k for k in DISTORTION_KEYS if float(meta.get(k, 0.0)) != 0.0]
    if bad:
        raise NotImplementedError(f"{where}: non-zero distortion {', '.join(bad)}: undistortion is not supported "
                                  "(undistort the images first)")


def _frame_distortion(contents: dict, frame: dict, where: str):
    """(coefficients in DISTORTION_KEYS order, camera_model): the frame's values win over the file's, as for the
    intrinsics.  Refuses what undistort.py does not define."""
    model = frame.get("camera_model", contents.get("camera_model"))
    dist = tuple(float(frame.get(k, contents.get(k, 0.0))) for k in DISTORTION_KEYS)
    check_coefficients(dist, model, where)
    return dist, model


def _frame_size(contents: dict, frame: dict, image_path: Path):
    """(w, h): the frame's values win over the file's; a dataset that stores neither has its image header read."""
    w = frame.get("w", contents.get("w"))
    h = frame.get("h", contents.get("h"))
    if w is None or h is None:
        from PIL import Image
        with Image.open(image_path) as im:
            w, h = im.size
    return int(w), int(h)


def parse_dataset(data_dir, config: Optional[DataparserConfig] = None, verbose: bool = True) -> DataparserOutputs:
    """Reads ``data_dir/transforms.json``.  Frames are sorted by ``file_path``; frames without ``depth_file_path`` are
    skipped (their number is reported); ``mask_path`` and ``label_path`` (a class map, semantic.py) are optional.
    Intrinsics and sizes are the frame's, else the file's.  Poses go through ``orient_and_center`` and are then scaled by ``scale_factor / max |origin coordinate|``
    (``auto_scale_poses``) or by ``scale_factor``.  With ``config.undistort`` the intrinsics of a distorted frame are
    replaced by ``optimal_new_intrinsics`` of the frame's own (see the module docstring)."""
    cfg = config or DataparserConfig()
    data_dir = Path(data_dir)
    contents = load_transforms(data_dir)
    if not cfg.undistort:
        _check_undistorted(contents, "transforms.json")
    frames = sorted(contents["frames"], key=lambda f: f["file_path"])
    with_depth = [f for f in frames if "depth_file_path" in f]
    n_skipped = len(frames) - len(with_depth)
    if verbose and n_skipped:
        print(f"dataparser: skipped {n_skipped} of {len(frames)} frames without depth_file_path")
    if not with_depth:
        raise ValueError(f"{data_dir}: no frame of transforms.json has a depth_file_path")
    images, depths, masks, poses, intr, sizes, labels = [], [], [], [], [], [], []
    src_intr, dists, models, new_K = [], [], [], {}
    for f in with_depth:
        if not cfg.undistort:
            _check_undistorted(f, f"frame {f['file_path']}")
        images.append(data_dir / f["file_path"])
        depths.append(data_dir / f["depth_file_path"])
        masks.append(data_dir / f["mask_path"] if "mask_path" in f else None)
        labels.append(data_dir / f["label_path"] if "label_path" in f else None)
        poses.append(np.asarray(f["transform_matrix"], dtype=np.float64))
        intr.append(frame_intrinsics(contents, f))
        sizes.append(_frame_size(contents, f, images[-1]))
        if cfg.undistort:
            dist, model = _frame_distortion(contents, f, f"frame {f['file_path']}")
            src_intr.append(intr[-1])
            dists.append(dist)
            models.append(model)
            if is_distorted(dist, model):
                key = (intr[-1], dist, model, sizes[-1])                 # K' is computed once per distinct camera
                if key not in new_K:
                    new_K[key] = optimal_new_intrinsics(intr[-1], dist, model, *sizes[-1])
                intr[-1] = new_K[key]
    c2w = np.stack([p[:3] for p in poses])                                     # [n,3,4]
    c2w, transform = orient_and_center(c2w, cfg.orientation_method, cfg.center_method)
    scale = float(cfg.scale_factor)
    if cfg.auto_scale_poses:
        scale /= float(np.max(np.abs(c2w[:, :3, 3])))
    c2w[:, :3, 3] *= scale
    i_train, i_eval = split_indices(len(images), cfg.train_split_fraction)
    intr = np.asarray(intr, dtype=np.float64)
    sizes = np.asarray(sizes, dtype=np.int64)
    transform_t = torch.from_numpy(transform).to(torch.float32)
    ply = data_dir / contents["ply_file_path"] if "ply_file_path" in contents else None
    return DataparserOutputs(
        image_filenames=images, depth_filenames=depths, mask_filenames=masks,
        camera_to_worlds=torch.from_numpy(c2w).to(torch.float32), fx=intr[:, 0], fy=intr[:, 1], cx=intr[:, 2],
        cy=intr[:, 3], widths=sizes[:, 0], heights=sizes[:, 1], i_train=i_train, i_eval=i_eval,
        dataparser_transform=transform_t, dataparser_scale=scale, depth_unit_scale_factor=float(cfg.depth_unit_scale_factor),
        n_skipped=n_skipped, ply_file_path=ply, config=cfg,
        src_intrinsics=np.asarray(src_intr, dtype=np.float64) if cfg.undistort else None,
        distortion_params=np.asarray(dists, dtype=np.float64) if cfg.undistort else None,
        camera_models=models if cfg.undistort else None,
        camera_to_worlds_f64=np.array(c2w, dtype=np.float64), dataparser_transform_f64=np.array(transform, dtype=np.float64),
        label_filenames=labels if any(p is not None for p in labels) else None)
