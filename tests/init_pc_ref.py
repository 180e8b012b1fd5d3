"""Test helpers of step 1 of qed-init-pc (building the point cloud): synthetic datasets, the NumPy oracle's functions
in the shape ``create_pointcloud_from_transforms`` takes them, and a level-by-level restatement of the merge tree.
Not part of the product; nothing under qed_splatter_amd/ imports it."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import backproject_oracle as B


# ---- the oracle's functions, in the driver's calling convention ------------------------------------------------------
def backproject_o3d(depth, K32, w2c32, depth_max, stride):
    """What the reference asks of Open3D (create_from_depth_image with a float32 intrinsic matrix and a float32 OpenCV
    world-to-camera extrinsic), answered by the oracle in float64."""
    c2w = np.linalg.inv(np.asarray(w2c32, dtype=np.float64))
    c2w[:3, 1:3] *= -1                                       # back to the OpenGL camera-to-world the oracle takes
    return B.backproject_frame(depth, np.asarray(K32, dtype=np.float64), c2w, depth_max=depth_max, stride=stride)


def oracle_backproject_fn(depth, fx, fy, cx, cy, c2w_opengl, depth_max, stride):
    """The same arithmetic the reference's backproject_frame reaches backproject_o3d with (:173-186)."""
    K32 = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float32)
    w2c32 = B.opengl_c2w_to_opencv_w2c(np.asarray(c2w_opengl, dtype=np.float64)).astype(np.float32)
    return backproject_o3d(depth, K32, w2c32, depth_max, stride)


class RecordingDownSample:
    """``down_sample_fn`` that answers with ``fn`` and notes (rows in, voxel size, rows out) and, with ``keep_voxels``,
    the occupied voxels of every call; ``last_out``: what the last call returned."""

    def __init__(self, fn=B.voxel_down_sample, keep_voxels=False):
        self.fn, self.keep_voxels, self.calls, self.voxels, self.last_out = fn, keep_voxels, [], [], None

    def __call__(self, points, voxel_size):
        out = self.last_out = self.fn(points, voxel_size)
        self.calls.append((int(len(points)), float(voxel_size), int(len(out))))
        if self.keep_voxels:
            self.voxels.append(np.unique(np.floor(np.asarray(points, dtype=np.float64) / voxel_size).astype(np.int64), axis=0))
        return out


def merge_counts(calls, frame_voxel, merge_voxel, final_voxel):
    """The recorded calls by role: per-frame calls in frame order, merge calls as a sorted list (the reference merges
    level by level, the product as soon as two clouds of a level exist: same tree, another order), the final call."""
    frames = [c for c in calls[:-1] if c[1] == frame_voxel]
    merges = sorted(c for c in calls[:-1] if c[1] == merge_voxel)
    assert len(frames) + len(merges) == len(calls) - 1 and calls[-1][1] == final_voxel
    return frames, merges, calls[-1]


def sort_by_voxel(points, voxel_size):
    p = np.asarray(points, dtype=np.float64)
    k = np.floor(p / voxel_size).astype(np.int64)
    return p[np.lexsort(k.T[::-1])]


# ---- the merge tree, level by level (create_init_pointcloud.py:101-145 without the files) --------------------------------
def tree_merge_levels(clouds, voxel_size, max_points, down_sample_fn):
    current = list(clouds)
    while len(current) > 1:
        nxt = []
        for i in range(0, len(current), 2):
            if i + 1 < len(current):
                merged = np.concatenate([current[i], current[i + 1]], axis=0)
                nxt.append(down_sample_fn(merged, voxel_size) if len(merged) > max_points else merged)
            else:
                nxt.append(current[i])
        current = nxt
    return current[0]


# ---- synthetic datasets --------------------------------------------------------------------------------------------------
def _pose(rng, yaw_max, offset_max):
    yaw = rng.uniform(-yaw_max, yaw_max)
    c, s = np.cos(yaw), np.sin(yaw)
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    c2w[:3, 3] = rng.uniform(-offset_max, offset_max, size=3)
    return c2w


def build_scene(seed, n_usable=7, h=24, w=32, focal=40.0, special=True, density=None):
    """Frames looking at a rough wall 3 +- 0.5 m away from slightly different poses; raw depth in millimetres.
    ``special``: adds a frame without depth_file_path, an all-zero / NaN frame, a frame wholly beyond depth_max, and
    gives one usable frame its own intrinsics.  ``density[i]``: share of valid pixels of usable frame i."""
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n_usable):
        depth = rng.uniform(2500.0, 3500.0, size=(h, w)).astype(np.float32)
        if density is not None and density[i] < 1.0:
            depth[rng.uniform(size=(h, w)) >= density[i]] = 0.0
        frames.append(dict(depth_raw=depth, c2w=_pose(rng, 0.1, 0.2), kind="usable"))
    if special:
        frames[2]["intr"] = (focal * 1.05, focal * 0.95, w / 2 + 0.5, h / 2 - 0.25)
        frames.insert(1, dict(depth_raw=None, c2w=_pose(rng, 0.1, 0.2), kind="no_depth_file"))
        bad = np.zeros((h, w), dtype=np.float32)
        bad[::2] = np.nan
        bad[1, 1] = -5.0
        frames.insert(4, dict(depth_raw=bad, c2w=_pose(rng, 0.1, 0.2), kind="no_valid_depth"))
        frames.append(dict(depth_raw=np.full((h, w), 250_000.0, dtype=np.float32), c2w=_pose(rng, 0.1, 0.2),
                           kind="beyond_depth_max"))
    return dict(h=h, w=w, fl_x=focal, fl_y=focal, cx=w / 2.0, cy=h / 2.0, frames=frames)


def write_dataset(root, scene, colors=False):
    """transforms.json + depth/frame_XXX.npy (raw millimetres) (+ uniform grey RGB images) under ``root``."""
    os.makedirs(os.path.join(root, "depth"), exist_ok=True)
    out = dict(fl_x=scene["fl_x"], fl_y=scene["fl_y"], cx=scene["cx"], cy=scene["cy"], w=scene["w"], h=scene["h"], frames=[])
    for i, fr in enumerate(scene["frames"]):
        entry = dict(file_path=f"images/frame_{i:03d}.png", transform_matrix=np.asarray(fr["c2w"]).tolist())
        if fr["depth_raw"] is not None:
            entry["depth_file_path"] = f"depth/frame_{i:03d}.npy"
            np.save(os.path.join(root, entry["depth_file_path"]), fr["depth_raw"])
        if "intr" in fr:
            entry.update(dict(zip(("fl_x", "fl_y", "cx", "cy"), (float(v) for v in fr["intr"]))))
        if colors:
            from PIL import Image
            os.makedirs(os.path.join(root, "images"), exist_ok=True)
            Image.fromarray(np.full((scene["h"], scene["w"], 3), 40 + 20 * (i % 8), dtype=np.uint8)).save(
                os.path.join(root, entry["file_path"]))
        out["frames"].append(entry)
    with open(os.path.join(root, "transforms.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, indent=4)


# the fixture's dataset and settings (tests/golden/make_init_pc_kats.py, tests/test_init_pc_driver.py)
KAT_SEED = 20261016
KAT_DENSITY = (1.0, 1.0, 0.3, 0.3, 1.0, 1.0, 1.0, 1.0, 0.5)      # nine usable frames: a cloud is carried forward at three levels
KAT_SETTINGS = dict(depth_unit_scale_factor=0.001, voxel_size=0.25, merge_voxel_size=0.15, frame_voxel_size=0.1,
                    max_points=1000, depth_max=100.0, stride=1)


def kat_scene():
    return build_scene(KAT_SEED, n_usable=len(KAT_DENSITY), h=24, w=32, focal=40.0, special=True, density=KAT_DENSITY)


def scene_from_fixture(k):
    """The dataset stored in tests/golden/init_pc_kats.npz."""
    frames = []
    for i, kind in enumerate(str(k["kinds"]).split(",")):
        fr = dict(depth_raw=k[f"depth_raw_{i}"] if f"depth_raw_{i}" in k.files else None, c2w=k["c2w"][i], kind=kind)
        if np.isfinite(k["frame_intr"][i]).all():
            fr["intr"] = tuple(k["frame_intr"][i])
        frames.append(fr)
    g = k["file_intr"]
    return dict(h=int(k["hw"][0]), w=int(k["hw"][1]), fl_x=float(g[0]), fl_y=float(g[1]), cx=float(g[2]), cy=float(g[3]),
                frames=frames)


# the dataset of the GPU driver test and of its CPU self-check: nested power-of-two voxel sizes
DRIVER_SETTINGS = dict(depth_unit_scale_factor=0.001, voxel_size=0.25, merge_voxel_size=0.125, frame_voxel_size=0.0625,
                       max_points=30_000, depth_max=100.0, stride=2)
DRIVER_SEED = 0


def driver_scene(seed=DRIVER_SEED):
    return build_scene(seed, n_usable=7, h=270, w=480, focal=400.0, special=False)
