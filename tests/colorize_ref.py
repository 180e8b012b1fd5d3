"""NumPy restatement of the colourise step of ``qed-init-pc`` (create_init_pointcloud.py:264-390) and the synthetic
RGB-D dataset its tests run on.  Shared by tests/golden/make_colorize_kats.py (which pins the restatement AND the
kernels to the reference's own function) and by the large GPU cases of tests/test_colorize.py.

``colorize_fp32`` follows the reference operation by operation in float32.  ``colorize_fp64`` is the same chain in
float64 (un-rounded world-to-camera matrix) and also returns the FRAGILE mask: points for which an fp32 evaluation may
legitimately decide differently, because a pixel-rounding boundary, the depth tolerance or depth_max lies within a
margin of the exact value.  The margins come from ``measure_fp32_error``: 8 x the largest fp32 error of u, v and z seen
on the input at hand (one factor 2 for another BLAS / FMA contraction, the rest head-room for the GPU's own order).
"""
from __future__ import annotations

import json
import os

import numpy as np

DEFAULTS = dict(depth_unit_scale_factor=0.001, depth_max=100.0, depth_tolerance=0.05, depth_tolerance_rel=0.02)
MARGIN_FACTOR = 8.0
FRAGILE_CAP = 0.05


def w2c_opencv_f64(c2w_opengl) -> np.ndarray:
    c2w = np.array(c2w_opengl, dtype=np.float64).copy()
    c2w[:3, 1:3] *= -1
    return np.linalg.inv(c2w)


def project(positions, w2c, intr, dtype):
    """u, v, z as the reference's _project_points, in ``dtype``; NaN u, v where the point is not in front."""
    fx, fy, cx, cy = (dtype(t) for t in intr)
    pts_h = np.concatenate([positions.astype(dtype), np.ones((positions.shape[0], 1), dtype=dtype)], axis=1)
    pts_cam = pts_h @ w2c.astype(dtype).T
    z = pts_cam[:, 2]
    valid_z = np.isfinite(z) & (z > 1e-6)
    z_safe = np.where(valid_z, z, dtype(1.0))
    with np.errstate(all="ignore"):
        u = fx * (pts_cam[:, 0] / z_safe) + cx
        v = fy * (pts_cam[:, 1] / z_safe) + cy
    u = np.where(valid_z & np.isfinite(u), u, np.nan)
    v = np.where(valid_z & np.isfinite(v), v, np.nan)
    return u, v, z


def clean_depth(raw, scale) -> np.ndarray:
    """:310-312 in float32: scale, then non-finite and <= 0 -> 0."""
    with np.errstate(all="ignore"):
        depth = raw.astype(np.float32) * np.float32(scale)
        depth[~np.isfinite(depth)] = 0.0
        depth[depth <= 0.0] = 0.0
    return depth


def finalize(color_sum, color_count):
    colored = color_count > 0
    colors = np.zeros((color_count.shape[0], 3), dtype=np.uint8)
    colors[colored] = (color_sum[colored] / color_count[colored, None] * 255.0).clip(0.0, 255.0).astype(np.uint8)
    return colors


def _hits(u, v, z, depth, dtype, depth_max, tol_abs, tol_rel):
    """Indices of the points the frame hits, and their pixels (the chain of :327-358)."""
    h, w = depth.shape
    with np.errstate(all="ignore"):
        cand = (np.isfinite(u) & np.isfinite(v) & np.isfinite(z) & (z > 0.0) & (z <= dtype(depth_max)) & (u >= -0.5)
                & (u < (w - 0.5)) & (v >= -0.5) & (v < (h - 0.5)))
    idx = np.flatnonzero(cand)
    ui = np.rint(u[idx]).astype(np.int32)
    vi = np.rint(v[idx]).astype(np.int32)
    inb = (ui >= 0) & (ui < w) & (vi >= 0) & (vi < h)
    idx, ui, vi = idx[inb], ui[inb], vi[inb]
    zv = z[idx]
    measured = depth[vi, ui].astype(dtype)
    tol = np.maximum(dtype(tol_abs), dtype(tol_rel) * zv)
    ok = (measured > 0.0) & (np.abs(measured - zv) <= tol)
    return idx[ok], ui[ok], vi[ok]


def usable(frames):
    return [f for f in frames if not f.get("rgb_missing") and f["color"].shape[:2] == f["depth_raw"].shape[:2]]


def colorize_fp32(points, frames, depth_unit_scale_factor=0.001, depth_max=100.0, depth_tolerance=0.05,
                  depth_tolerance_rel=0.02):
    """-> colors uint8 [N,3], color_sum float64 [N,3], color_count int32 [N]; frames: dicts with depth_raw, color
    (uint8), c2w (float64 4x4), intr (fx, fy, cx, cy)."""
    positions = np.asarray(points, dtype=np.float32)
    n = positions.shape[0]
    color_sum = np.zeros((n, 3), dtype=np.float64)
    color_count = np.zeros((n,), dtype=np.int32)
    for fr in usable(frames):
        depth = clean_depth(fr["depth_raw"], depth_unit_scale_factor)
        color = fr["color"].astype(np.float32) / 255.0
        w2c = w2c_opencv_f64(fr["c2w"]).astype(np.float32)
        u, v, z = project(positions, w2c, np.asarray(fr["intr"], dtype=np.float32), np.float32)
        idx, ui, vi = _hits(u, v, z, depth, np.float32, depth_max, depth_tolerance, depth_tolerance_rel)
        color_sum[idx] += color[vi, ui]
        color_count[idx] += 1
    return finalize(color_sum, color_count), color_sum, color_count


def _in_view(u, v, z, h, w):
    with np.errstate(all="ignore"):
        return np.isfinite(u) & np.isfinite(v) & (z > 1e-6) & (u >= -1.5) & (u < w + 0.5) & (v >= -1.5) & (v < h + 0.5)


def measure_fp32_error(points, frames, project32=None):
    """max |u32 - u64|, |v32 - v64|, |z32 - z64| over the points in front of a camera and within one pixel of its image.
    ``project32(positions, w2c_f32, K_f32) -> u, v, z``: the fp32 projection to measure (default: this file's)."""
    positions = np.asarray(points, dtype=np.float32)
    du = dv = dz = 0.0
    for fr in usable(frames):
        h, w = fr["depth_raw"].shape
        w2c = w2c_opencv_f64(fr["c2w"])
        intr = np.asarray(fr["intr"], dtype=np.float32)
        u6, v6, z6 = project(positions, w2c, intr.astype(np.float64), np.float64)
        if project32 is None:
            u3, v3, z3 = project(positions, w2c.astype(np.float32), intr, np.float32)
        else:
            K = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]], dtype=np.float32)
            u3, v3, z3 = project32(positions, w2c.astype(np.float32), K)
        m = _in_view(u6, v6, z6, h, w) & np.isfinite(u3) & np.isfinite(v3)
        if m.any():
            du = max(du, float(np.abs(u3[m] - u6[m]).max()))
            dv = max(dv, float(np.abs(v3[m] - v6[m]).max()))
            dz = max(dz, float(np.abs(z3[m] - z6[m]).max()))
    return du, dv, dz


def margins(du, dv, dz):
    return MARGIN_FACTOR * max(du, dv), MARGIN_FACTOR * dz


def colorize_fp64(points, frames, eps_px, eps_m, depth_unit_scale_factor=0.001, depth_max=100.0, depth_tolerance=0.05,
                  depth_tolerance_rel=0.02):
    """-> colors uint8 [N,3], fragile bool [N].  The float64 restatement (positions and the cleaned depth are the fp32
    values both sides see) and the points whose hit set may legitimately differ in fp32."""
    positions = np.asarray(points, dtype=np.float32)
    n = positions.shape[0]
    color_sum = np.zeros((n, 3), dtype=np.float64)
    color_count = np.zeros((n,), dtype=np.int32)
    fragile = np.zeros((n,), dtype=bool)
    for fr in usable(frames):
        depth = clean_depth(fr["depth_raw"], depth_unit_scale_factor)
        h, w = depth.shape
        color = fr["color"].astype(np.float32) / 255.0
        intr = np.asarray(fr["intr"], dtype=np.float32).astype(np.float64)
        u, v, z = project(positions, w2c_opencv_f64(fr["c2w"]), intr, np.float64)
        near = _in_view(u, v, z, h, w)
        with np.errstate(all="ignore"):
            fu, fv = u + 0.5, v + 0.5
            fragile |= near & ((np.abs(fu - np.rint(fu)) < eps_px) | (np.abs(fv - np.rint(fv)) < eps_px))
            fragile |= near & (np.abs(z - depth_max) < eps_m)
            cand = near & (z <= depth_max) & (u >= -0.5) & (u < w - 0.5) & (v >= -0.5) & (v < h - 0.5)
        ci = np.flatnonzero(cand)
        ui = np.clip(np.rint(u[ci]).astype(np.int64), 0, w - 1)
        vi = np.clip(np.rint(v[ci]).astype(np.int64), 0, h - 1)
        measured = depth[vi, ui].astype(np.float64)
        tol = np.maximum(depth_tolerance, depth_tolerance_rel * z[ci])
        fragile[ci] |= (measured > 0.0) & (np.abs(np.abs(measured - z[ci]) - tol) < eps_m)
        idx, hu, hv = _hits(u, v, z, depth, np.float64, depth_max, depth_tolerance, depth_tolerance_rel)
        color_sum[idx] += color[hv, hu]
        color_count[idx] += 1
    return finalize(color_sum, color_count), fragile


def check_against(colors, want, fragile):
    """The comparison rule: at most FRAGILE_CAP fragile points, exact equality elsewhere, and over ALL points no larger a
    share of differing colours than the fragile share.  Returns (fragile share, differing share)."""
    share = float(fragile.mean()) if fragile.size else 0.0
    differ = float((np.asarray(colors) != np.asarray(want)).any(axis=1).mean()) if fragile.size else 0.0
    print(f"fragile share {share:.4%}, differing share over all points {differ:.4%}")
    assert share <= FRAGILE_CAP, share
    np.testing.assert_array_equal(np.asarray(colors)[~fragile], np.asarray(want)[~fragile])
    assert differ <= share, (differ, share)
    return share, differ


# ---- the synthetic scene: a wall plane and an occluding sphere, ray-cast analytically to z-depth ----------------------
WALL_Z = -4.0
SPHERE_C = np.array([0.2, 0.1, -2.5])
SPHERE_R = 0.6


def _pose(yaw, pitch, offset):
    cy_, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    c2w = np.eye(4)
    c2w[:3, :3] = Ry @ Rx
    c2w[:3, 3] = offset
    return c2w


def raycast_depth(h, w, intr, c2w):
    """z-depth (metres, float64) of the scene seen by an OpenGL camera; 0 where nothing is hit."""
    fx, fy, cx, cy = intr
    vs, us = np.mgrid[0:h, 0:w].astype(np.float64)
    d_cam = np.stack([(us - cx) / fx, -(vs - cy) / fy, -np.ones_like(us)], -1)      # z-forward component 1: t IS z-depth
    d = d_cam @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(all="ignore"):
        t_wall = (WALL_Z - o[2]) / d[..., 2]
        t_wall = np.where(t_wall > 0, t_wall, np.inf)
        oc = o - SPHERE_C
        a = (d * d).sum(-1)
        b = 2.0 * (d * oc).sum(-1)
        c = float(oc @ oc) - SPHERE_R ** 2
        disc = b * b - 4 * a * c
        t_s = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf)
        t_s = np.where(t_s > 0, t_s, np.inf)
    t = np.minimum(t_wall, t_s)
    return np.where(np.isfinite(t), t, 0.0)


def build_scene(n_frames=8, h=48, w=64, n_points=4000, seed=0, special_frames=True):
    """-> dict(points float32 [N,3], frames [dict(depth_raw float32 mm, color uint8, c2w float64, intr, frame_level,
    rgb_missing)]).  With ``special_frames`` (>= 8 frames): frame 2 carries frame-level intrinsics, frame 5 has no RGB
    file, frame 6 has another size (with matching RGB), so the file rules are on the path."""
    rng = np.random.default_rng(seed)
    frames = []
    for f in range(n_frames):
        fh, fw = (h, w)
        if special_frames and f == 6:
            fh, fw = (h * 5) // 6, (w * 7) // 8
        intr = (0.9 * fw, 0.92 * fw, fw / 2 - 0.3, fh / 2 + 0.2)
        frame_level = bool(special_frames and f == 2)
        if frame_level:
            intr = (1.05 * fw, 1.0 * fw, fw / 2 + 1.1, fh / 2 - 0.7)
        c2w = _pose(rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(-0.6, 0.6, size=3) * [1, 0.6, 0.8])
        depth = raycast_depth(fh, fw, intr, c2w)
        raw = (depth * 1000.0).astype(np.float32)
        raw[rng.uniform(size=raw.shape) < 0.05] = 0.0
        if f == 0:
            raw[fh // 3, fw // 3] = np.nan
        color = rng.integers(0, 256, size=(fh, fw, 3), dtype=np.uint8)
        frames.append(dict(depth_raw=raw, color=color, c2w=c2w, intr=tuple(float(t) for t in intr),
                           frame_level=frame_level, rgb_missing=bool(special_frames and f == 5)))
    n_wall, n_sph = n_points // 2, n_points // 3
    n_box = n_points - n_wall - n_sph
    wall = np.stack([rng.uniform(-3.5, 3.5, n_wall), rng.uniform(-2.6, 2.6, n_wall), np.full(n_wall, WALL_Z)], -1)
    dirs = rng.normal(size=(n_sph, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    sph = SPHERE_C + SPHERE_R * dirs
    box = rng.uniform([-3.5, -2.6, -5.0], [3.5, 2.6, 1.5], size=(n_box, 3))          # z > ~0.5: behind the cameras
    pts = np.concatenate([wall, sph, box]) + rng.normal(scale=0.04, size=(n_points, 3))
    pts = pts[rng.permutation(n_points)]
    pts[n_points // 7, 1] = np.nan                                                    # one NaN coordinate
    pts[n_points // 5] = [0.1, -0.2, -150.0]                                          # one beyond depth_max
    return dict(points=pts.astype(np.float32), frames=frames)


def write_dataset(root, scene, base_intr=None):
    """The scene as a dataset directory: transforms.json, depth as float32 millimetres in .npy, RGB as PNG (not written
    for ``rgb_missing`` frames).  File-level intrinsics are those of frame 0; a frame that differs carries its own."""
    from PIL import Image
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "depths"), exist_ok=True)
    base = tuple(base_intr or scene["frames"][0]["intr"])
    contents = dict(fl_x=base[0], fl_y=base[1], cx=base[2], cy=base[3], frames=[])
    for f, fr in enumerate(scene["frames"]):
        entry = dict(file_path=f"images/frame_{f:05d}.png", depth_file_path=f"depths/frame_{f:05d}.npy",
                     transform_matrix=np.asarray(fr["c2w"], dtype=np.float64).tolist())
        if tuple(fr["intr"]) != base:
            entry.update(fl_x=fr["intr"][0], fl_y=fr["intr"][1], cx=fr["intr"][2], cy=fr["intr"][3])
        np.save(os.path.join(root, entry["depth_file_path"]), fr["depth_raw"])
        if not fr.get("rgb_missing"):
            Image.fromarray(fr["color"]).save(os.path.join(root, entry["file_path"]))
        contents["frames"].append(entry)
    contents["frames"].append(dict(file_path="images/no_depth.png", transform_matrix=np.eye(4).tolist()))   # no depth: unused
    with open(os.path.join(root, "transforms.json"), "w", encoding="utf-8") as fh:
        json.dump(contents, fh)
    return contents


def scene_from_fixture(k):
    """The scene dict back from tests/golden/colorize_kats.npz."""
    frames = []
    for f in range(int(k["n_frames"])):
        frames.append(dict(depth_raw=k[f"depth_raw_{f}"], color=k[f"color_{f}"], c2w=k["c2w"][f],
                           intr=tuple(float(t) for t in k["intr"][f]), frame_level=bool(k["frame_level"][f]),
                           rgb_missing=bool(k["rgb_missing"][f])))
    return dict(points=k["points"], frames=frames)
