"""The initial point cloud: the reference's ``qed-init-pc`` tool on the GPU, both steps, no Open3D.

Step 1, geometry (create_init_pointcloud.py:83-261 and the branch of ``main`` without ``--colorize``):
``create_pointcloud_from_transforms`` walks the frames of a transforms.json, back-projects each depth map
(``backproject_depth``, csrc/backproject.hip, for Open3D's ``create_from_depth_image``), thins it with
``voxel_down_sample`` (csrc/voxel.hip: sort by voxel + segmented float64 means, a pure function of its input, output
in ascending voxel order) and merges the frames' clouds in the reference's pairwise tree (``tree_merge_pointclouds``,
in memory: the reference's per-frame PLY cache and on-disk merge levels are not offered).
``python -m qed_splatter_amd.init_pointcloud --data DIR`` writes the geometry-only ``sparse_pc.ply``.

Step 2, colour (``--colorize``, :264-390): ``PointColorizer`` (csrc/colorize.hip), ``colorize_pointcloud`` (the
reference's frame loop and file rules), a NumPy PLY reader / writer in place of the two ``o3d.t.io`` calls, and
``python -m qed_splatter_amd.init_pointcloud --data DIR --colorize``.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
from pathlib import Path

import numpy as np
import torch
from torch import Tensor

from . import _lib as L


def frame_intrinsics(contents: dict, frame: dict):
    """(fx, fy, cx, cy) of one frame of a transforms.json: frame-level values win over the file's, and a missing ``fl_y``
    falls back to the FRAME's ``fl_x`` before the file's (create_init_pointcloud.py:49-56; pinned by
    tests/golden/reference_kats.npz ``ip_intrinsics_*``)."""
    fl_x = float(frame.get("fl_x", contents["fl_x"]))
    fl_y = float(frame.get("fl_y", contents.get("fl_y", fl_x)))
    return fl_x, fl_y, float(frame.get("cx", contents["cx"])), float(frame.get("cy", contents["cy"]))


@torch.no_grad()
def backproject_depth(depth: Tensor, fx: float, fy: float, cx: float, cy: float, c2w_opengl: Tensor,
                      depth_max: float = 100.0, stride: int = 1) -> Tensor:
    """depth [H,W] (metres; non-finite / non-positive = invalid) on the GPU, OpenGL camera-to-world [3,4] or
    [4,4] -> world points [n,3] in row-major pixel order.  One host read (the point count)."""
    lib = L.load()
    assert depth.is_cuda and depth.dim() == 2
    depth = depth.to(torch.float32).contiguous()
    H, W = depth.shape
    gw, gh = (W + stride - 1) // stride, (H + stride - 1) // stride
    cap = gw * gh
    pts = torch.empty(cap, 3, dtype=torch.float32, device=depth.device)
    n_pts = torch.zeros(1, dtype=torch.int32, device=depth.device)
    work = torch.empty(int(lib.qed_backproject_workspace_ints(H, W, stride)), dtype=torch.int32, device=depth.device)
    status = torch.zeros(4, dtype=torch.int32, device=depth.device)
    pose = [float(v) for v in torch.as_tensor(c2w_opengl, dtype=torch.float32).cpu()[:3, :4].reshape(-1)]
    h_pose = (C.c_float * 12)(*pose)
    L.check(lib.qed_backproject_depth(H, W, L.ptr(depth), float(fx), float(fy), float(cx), float(cy),
                                      C.cast(h_pose, C.c_void_p), float(depth_max), int(stride), cap, L.ptr(pts),
                                      L.ptr(n_pts), L.ptr(work), L.ptr(status), torch.cuda.current_stream().cuda_stream),
            "qed_backproject_depth")
    return pts[: int(n_pts)]


def _voxel_down_sample_torch(points: Tensor, voxel_size: float) -> Tensor:
    """unique over voxel keys + index_add: the body CPU tensors take (on a GPU its sums depend on atomic order)."""
    if points.shape[0] == 0:
        return points
    keys = torch.floor(points / voxel_size).to(torch.int64)
    keys = keys - keys.min(dim=0).values
    span = keys.max(dim=0).values + 1
    flat = (keys[:, 0] * span[1] + keys[:, 1]) * span[2] + keys[:, 2]
    _, inv, counts = torch.unique(flat, return_inverse=True, return_counts=True)
    out = torch.zeros(counts.shape[0], 3, dtype=points.dtype, device=points.device)
    out.index_add_(0, inv, points)
    return out / counts[:, None].to(points.dtype)


@torch.no_grad()
def voxel_down_sample(points: Tensor, voxel_size: float) -> Tensor:
    """One point per occupied voxel: the mean of its members (Open3D semantics), in ascending (ix, iy, iz) order of
    the voxels floor(p / voxel_size).  A tensor on the GPU goes to qed_voxel_down_sample (float64 sums, bit-identical
    from run to run, points with a non-finite coordinate dropped; one host read: the count and the status words);
    a CPU tensor to the torch body."""
    if not points.is_cuda:
        return _voxel_down_sample_torch(points, voxel_size)
    lib = L.load()
    assert points.dim() == 2 and points.shape[1] == 3
    pts = points.to(torch.float32).contiguous()
    n = int(pts.shape[0])
    out = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
    meta = torch.zeros(1 + L.STATUS_WORDS, dtype=torch.int32, device=pts.device)        # n_out, status[4]
    ws_bytes = int(lib.qed_voxel_workspace_bytes(n))
    if ws_bytes < 0:
        raise L.QedSplatError(f"voxel_down_sample: {n} points are more than one call takes (2^30)")
    work = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=pts.device)
    L.check(lib.qed_voxel_down_sample(n, L.ptr(pts), float(voxel_size), L.ptr(out), L.ptr(meta), L.ptr(work),
                                      work.numel() * 8, L.ptr(meta[1:]), torch.cuda.current_stream().cuda_stream),
            "qed_voxel_down_sample")
    n_out, refused, _n_dropped, span, _ = (int(v) for v in meta.tolist())
    if refused:
        raise L.QedSplatError(f"voxel_down_sample: the cloud spans {span} voxels of {float(voxel_size):g} m on one axis; "
                              f"at most 2^21 = {1 << 21} are supported (62 km at 3 cm)")
    res = out[:n_out]
    return res.clone() if 2 * n_out < n else res          # (do not keep a frame-sized buffer alive behind a small cloud)


# ---- step 1: the frame loop and the merge tree (create_init_pointcloud.py:83-261) --------------------------------------
def _rows(cloud) -> int:
    return int(cloud.shape[0])


def _concat(left, right):
    if torch.is_tensor(left):
        return torch.cat([left, right], dim=0)
    return np.concatenate([left, right], axis=0)


class NoCloudsError(ValueError):
    """tree_merge_pointclouds was given no cloud at all."""


def tree_merge_pointclouds(clouds, voxel_size: float = 0.03, max_points: int = 2_000_000, down_sample_fn=None):
    """The reference's pairwise merge tree (tree_merge_pointclouds_on_disk, :101-145), in memory: level by level cloud
    2k (first in the concatenation) with cloud 2k + 1; the concatenation is down-sampled with ``voxel_size`` only if
    it has more than ``max_points`` rows; an unpaired last cloud moves up unchanged; one cloud in, that cloud out.
    ``clouds`` may be an iterator: a binary-counter stack (two clouds of one level merge as soon as both exist; at the
    end the smallest is carried upwards) builds exactly that tree while holding O(log F) clouds."""
    if down_sample_fn is None:
        down_sample_fn = voxel_down_sample

    def merge(left, right):
        merged = _concat(left, right)
        return down_sample_fn(merged, voxel_size) if _rows(merged) > max_points else merged

    stack = []                                   # (level, cloud), levels strictly decreasing towards the top
    for cloud in clouds:
        level = 0
        while stack and stack[-1][0] == level:
            cloud = merge(stack.pop()[1], cloud)
            level += 1
        stack.append((level, cloud))
    if not stack:
        raise NoCloudsError("tree_merge_pointclouds: no clouds")
    level, cloud = stack.pop()                   # the unpaired last cloud of its level: carried up to the next partner
    while stack:
        level, left = stack.pop()
        cloud = merge(left, cloud)
    return cloud


def _backproject_on_gpu(device):
    def fn(depth, fx, fy, cx, cy, c2w_opengl, depth_max, stride):
        return backproject_depth(torch.from_numpy(depth).to(device), fx, fy, cx, cy,
                                 torch.as_tensor(np.asarray(c2w_opengl, dtype=np.float64)), depth_max=depth_max,
                                 stride=stride)
    return fn


def create_pointcloud_from_transforms(dataset_path, depth_unit_scale_factor: float = 0.001, voxel_size: float = 0.05,
                                      merge_voxel_size: float = 0.03, frame_voxel_size=0.05,
                                      max_points: int = 2_000_000, depth_max: float = 100.0, stride: int = 1,
                                      device=None, backproject_fn=None, down_sample_fn=None,
                                      verbose: bool = True) -> np.ndarray:
    """The reference's create_pointcloud_from_transforms (:199-261) without its disk cache -> positions [n,3] float32.
    Frames without ``depth_file_path`` are not used; depth = file * depth_unit_scale_factor in fp32 with non-finite
    and <= 0 values zeroed; a frame with no positive depth or an empty cloud is skipped; each frame's cloud is thinned
    with ``frame_voxel_size`` (None or <= 0: not), the clouds go through ``tree_merge_pointclouds`` with
    ``merge_voxel_size`` / ``max_points``, and the result is ALWAYS down-sampled once more with ``voxel_size``.
    ``backproject_fn(depth, fx, fy, cx, cy, c2w_opengl, depth_max, stride)`` and ``down_sample_fn(points, voxel_size)``
    default to the GPU functions (tests substitute a NumPy oracle's)."""
    dataset_path = Path(dataset_path)
    contents = load_transforms(dataset_path)
    say = print if verbose else (lambda *a, **k: None)
    if backproject_fn is None:
        backproject_fn = _backproject_on_gpu(torch.device(device if device is not None else "cuda"))
    if down_sample_fn is None:
        down_sample_fn = voxel_down_sample
    n_used = [0]

    def frame_clouds():
        for frame in contents["frames"]:
            if "depth_file_path" not in frame:
                continue
            depth_path = dataset_path / frame["depth_file_path"]
            say(f"Backprojecting {depth_path}")
            depth = load_depth(depth_path) * depth_unit_scale_factor
            depth[~np.isfinite(depth)] = 0.0
            depth[depth <= 0.0] = 0.0
            depth = np.ascontiguousarray(depth, dtype=np.float32)
            if not np.any(depth > 0.0):
                say(f"  Skipping frame with no valid depth: {depth_path}")
                continue
            fx, fy, cx, cy = frame_intrinsics(contents, frame)
            cloud = backproject_fn(depth, fx, fy, cx, cy, np.array(frame["transform_matrix"], dtype=np.float64),
                                   depth_max, stride)
            if _rows(cloud) == 0:
                say(f"  Skipping empty point cloud for {depth_path}")
                continue
            if frame_voxel_size is not None and frame_voxel_size > 0:
                cloud = down_sample_fn(cloud, frame_voxel_size)
            say(f"  {_rows(cloud)} points")
            n_used[0] += 1
            yield cloud

    try:
        merged = tree_merge_pointclouds(frame_clouds(), voxel_size=merge_voxel_size, max_points=max_points,
                                        down_sample_fn=down_sample_fn)
    except NoCloudsError:
        raise RuntimeError("No valid point clouds could be generated from the dataset.") from None
    say(f"Merged {n_used[0]} frame point clouds: {_rows(merged)} points")
    final = down_sample_fn(merged, voxel_size)
    final = final.cpu().numpy() if torch.is_tensor(final) else np.asarray(final)
    return np.ascontiguousarray(final, dtype=np.float32)


# ---- step 2: colour (create_init_pointcloud.py:264-390) ----------------------------------------------------------------
class PointColorizer:
    """Per-point colour accumulators of ``qed-init-pc --colorize`` on the GPU: float64 colour sums and int32 hit counts
    of ``points`` [N,3], fed frame batches by ``add_frames`` and turned into uint8 colours by ``finalize``.  Any split of
    one frame sequence into batches gives bit-identical results (include/qed_splat.h: qed_colorize_accumulate)."""

    def __init__(self, points: Tensor, depth_unit_scale_factor: float = 0.001, depth_max: float = 100.0,
                 depth_tolerance: float = 0.05, depth_tolerance_rel: float = 0.02):
        assert points.is_cuda and points.dim() == 2 and points.shape[1] == 3
        self.lib = L.load()
        self.points = points.to(torch.float32).contiguous()
        self.n = int(self.points.shape[0])
        self.depth_unit_scale_factor = float(depth_unit_scale_factor)
        self.depth_max = float(depth_max)
        self.depth_tolerance = float(depth_tolerance)
        self.depth_tolerance_rel = float(depth_tolerance_rel)
        self.color_sum = torch.zeros(self.n, 3, dtype=torch.float64, device=points.device)
        self.color_count = torch.zeros(self.n, dtype=torch.int32, device=points.device)

    @torch.no_grad()
    def add_frames(self, depth, color, c2w_opengl, intrinsics) -> None:
        """One qed_colorize_accumulate call.  depth [F,H,W] | [H,W]: the RAW file values (scaled and cleaned in the
        kernel); color uint8 [F,H,W,3] | [H,W,3]; c2w_opengl [F,4,4] | [4,4] (float64 is kept); intrinsics
        (fx, fy, cx, cy) once or per frame.  Host arrays are uploaded; tensors already on the device are used as is."""
        dev = self.points.device
        depth = torch.as_tensor(depth)
        color = torch.as_tensor(color)
        if depth.dim() == 2:
            depth, color = depth[None], color[None]
        assert depth.dim() == 3 and color.dim() == 4 and color.shape[-1] == 3 and color.dtype == torch.uint8
        F, H, W = (int(v) for v in depth.shape)
        assert tuple(color.shape[:3]) == (F, H, W), "colour and depth sizes differ"
        depth = depth.to(device=dev, dtype=torch.float32).contiguous()
        color = color.to(device=dev).contiguous()
        poses = np.ascontiguousarray(np.asarray(torch.as_tensor(c2w_opengl).cpu(), dtype=np.float64).reshape(-1, 4, 4))
        intr = np.asarray(intrinsics, dtype=np.float64).reshape(-1, 4)
        if intr.shape[0] == 1 and F > 1:
            intr = np.repeat(intr, F, axis=0)
        intr = np.ascontiguousarray(intr, dtype=np.float32)
        assert poses.shape[0] == F and intr.shape[0] == F, "one pose and one intrinsics row per frame"
        L.check(self.lib.qed_colorize_accumulate(
            self.n, L.ptr(self.points), F, H, W, L.ptr(depth), self.depth_unit_scale_factor, L.ptr(color),
            poses.ctypes.data, intr.ctypes.data, self.depth_max, self.depth_tolerance, self.depth_tolerance_rel,
            L.ptr(self.color_sum), L.ptr(self.color_count), torch.cuda.current_stream().cuda_stream),
            "qed_colorize_accumulate")

    @torch.no_grad()
    def finalize(self):
        """-> (colors uint8 [N,3] on the device, number of coloured points).  One host read."""
        colors = torch.zeros(self.n, 3, dtype=torch.uint8, device=self.points.device)
        n_colored = torch.zeros(1, dtype=torch.int32, device=self.points.device)
        L.check(self.lib.qed_colorize_finalize(self.n, L.ptr(self.color_sum), L.ptr(self.color_count), L.ptr(colors),
                                               L.ptr(n_colored), torch.cuda.current_stream().cuda_stream),
                "qed_colorize_finalize")
        return colors, int(n_colored)


def load_depth(path) -> np.ndarray:
    """A depth map from ``.npy`` / ``.npz`` or an image file, as float32; the first channel of a 3-D array (:30-40)."""
    from PIL import Image
    path = Path(path)
    if path.suffix.lower() in {".npy", ".npz"}:
        depth = np.load(path).astype(np.float32)
    else:
        depth = np.array(Image.open(path), dtype=np.float32)
    if depth.ndim == 3:
        depth = depth[..., 0]
    return depth


def load_color_u8(path):
    """An RGB image as uint8 [H,W,3], or None if the file is missing (:43-47, without the division: the kernel takes
    uint8 and divides by 255 itself)."""
    from PIL import Image
    path = Path(path)
    if not path.exists():
        return None
    return np.array(Image.open(path).convert("RGB"), dtype=np.uint8)


def load_transforms(dataset_path) -> dict:
    transforms_path = Path(dataset_path) / "transforms.json"
    if not transforms_path.exists():
        raise FileNotFoundError(f"No transforms.json found at {transforms_path}")
    with open(transforms_path, encoding="utf-8") as f:
        return json.load(f)


def colorize_pointcloud(dataset_path, points, depth_unit_scale_factor: float = 0.001, depth_max: float = 100.0,
                        depth_tolerance: float = 0.05, depth_tolerance_rel: float = 0.02, batch_frames: int = 8,
                        device=None, colorizer_cls=None, verbose: bool = True) -> np.ndarray:
    """The reference's colorize_pointcloud (:284-390): points [N,3] (array or tensor) -> colours uint8 [N,3] (NumPy).
    Frames that lack ``depth_file_path`` or ``file_path`` are not used, a missing RGB file and an RGB / depth size
    mismatch are skipped; consecutive usable frames of equal size go to the GPU in batches of at most ``batch_frames``.
    ``colorizer_cls``: the accumulator class (PointColorizer; tests substitute a recorder)."""
    dataset_path = Path(dataset_path)
    contents = load_transforms(dataset_path)
    say = print if verbose else (lambda *a, **k: None)
    if colorizer_cls is None:
        colorizer_cls = PointColorizer
        points = torch.as_tensor(np.asarray(points, dtype=np.float32) if not torch.is_tensor(points) else points)
        points = points.to(device=device if device is not None else "cuda", dtype=torch.float32)
    colorizer = colorizer_cls(points, depth_unit_scale_factor=depth_unit_scale_factor, depth_max=depth_max,
                              depth_tolerance=depth_tolerance, depth_tolerance_rel=depth_tolerance_rel)
    frames = [f for f in contents["frames"] if "depth_file_path" in f and "file_path" in f]
    say(f"Colorizing {len(points)} points using {len(frames)} RGB-D frames...")
    batch = []                                  # (depth, color, c2w, intrinsics) of consecutive frames of one size

    def flush():
        if batch:
            colorizer.add_frames(np.stack([b[0] for b in batch]), np.stack([b[1] for b in batch]),
                                 np.stack([b[2] for b in batch]), np.array([b[3] for b in batch], dtype=np.float64))
            batch.clear()

    for frame in frames:
        image_path = dataset_path / frame["file_path"]
        color = load_color_u8(image_path)
        if color is None:
            say(f"  Skipping missing RGB: {image_path}")
            continue
        depth = load_depth(dataset_path / frame["depth_file_path"])
        h, w = depth.shape[:2]
        if color.shape[0] != h or color.shape[1] != w:
            say(f"  Skipping size mismatch RGB {color.shape[:2]} vs depth {(h, w)}: {image_path}")
            continue
        if batch and (batch[0][0].shape != depth.shape or len(batch) >= max(int(batch_frames), 1)):
            flush()
        batch.append((depth, color, np.array(frame["transform_matrix"], dtype=np.float64),
                      frame_intrinsics(contents, frame)))
    flush()
    colors, n_colored = colorizer.finalize()
    if n_colored == 0:
        raise RuntimeError("No points received color from any RGB frame.")
    say(f"Colored {n_colored}/{len(points)} points ({100.0 * n_colored / max(len(points), 1):.1f}%)")
    return colors.cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)


# ---- a minimal PLY reader / writer (in place of o3d.t.io in the colourise branch, :467 and :505) ----------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _read_ply_header(f, path, what: str = "point cloud"):
    """``(format, n, [(name, numpy type)], vertex element seen)`` of the PLY open at ``f``, which is left at the first
    byte of the body.  The vertex element must come first and have scalar properties only."""
    if f.readline().strip() != b"ply":
        raise RuntimeError(f"Failed to read {what}: {path}")
    fmt, n, props, in_vertex, seen_vertex = None, 0, [], False, False
    while True:
        line = f.readline()
        if not line:
            raise RuntimeError(f"Failed to read {what} (no end_header): {path}")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            in_vertex = tok[1] == "vertex" and not seen_vertex
            if in_vertex:
                n, seen_vertex = int(tok[2]), True
            elif not seen_vertex:
                raise RuntimeError(f"unsupported PLY (an element before 'vertex'): {path}")
        elif tok[0] == "property" and in_vertex:
            if tok[1] == "list":
                raise RuntimeError(f"unsupported PLY (list property on vertices): {path}")
            props.append((tok[2], _PLY_TYPES[tok[1]]))
        elif tok[0] == "end_header":
            break
    return fmt, n, props, seen_vertex


def _read_ply_vertex(path, optional=()):
    """``(n, {name: column})`` of a PLY's vertex element: ``x y z`` and, when the file has all of them, the properties
    named in ``optional``, each in its stored type.  ASCII and binary little-endian; the vertex element must come first
    and have scalar properties only."""
    with open(path, "rb") as f:
        fmt, n, props, seen_vertex = _read_ply_header(f, path)
        names = [p[0] for p in props]
        if not seen_vertex or not all(k in names for k in "xyz"):
            raise RuntimeError(f"Failed to read point cloud (no x y z): {path}")
        wanted = list("xyz") + (list(optional) if all(k in names for k in optional) else [])
        if fmt == "binary_little_endian":
            dt = np.dtype([(k, "<" + t) for k, t in props])
            rec = np.frombuffer(f.read(n * dt.itemsize), dtype=dt, count=n)
            cols = {k: rec[k] for k in wanted}
        elif fmt == "ascii":
            rows = np.loadtxt(f, dtype=np.float64, max_rows=n, ndmin=2) if n else np.zeros((0, len(props)))
            cols = {k: rows[:, names.index(k)].astype(dict(props)[k]) for k in wanted}
        else:
            raise RuntimeError(f"unsupported PLY format {fmt!r}: {path}")
    return n, cols


def _stack_positions(n, cols) -> np.ndarray:
    out_t = np.float64 if any(cols[k].dtype == np.float64 for k in "xyz") else np.float32
    return np.stack([cols[k].astype(out_t) for k in "xyz"], axis=1) if n else np.zeros((0, 3), dtype=out_t)


def read_ply_positions(path) -> np.ndarray:
    """The ``x y z`` of a PLY's vertex element as [N,3] (float32, or float64 if the file stores doubles).  ASCII and
    binary little-endian; the vertex element must come first and have scalar properties only."""
    return _stack_positions(*_read_ply_vertex(path))


def read_ply(path, with_normals: bool = False):
    """``(positions, colors | None)`` of a PLY's vertex element: positions as ``read_ply_positions`` returns them,
    colours [N,3] from the properties ``red green blue`` -- uint8 as stored (uchar), or float32 / float64 as Open3D's
    tensor API writes them (the caller decides how to quantise) -- or None when the file has none.  Same supported
    formats and the same refusals as ``read_ply_positions``.  ``with_normals``: a third result, the properties
    ``nx ny nz`` as [N,3] float32 (float64 if stored so), or None when the file has none."""
    rgb = ("red", "green", "blue")
    n, cols = _read_ply_vertex(path, rgb)
    positions = _stack_positions(n, cols)
    normals = None
    if with_normals:
        nxyz = ("nx", "ny", "nz")
        _, ncols = _read_ply_vertex(path, nxyz)
        if nxyz[0] in ncols:
            if any(ncols[k].dtype.kind != "f" for k in nxyz):
                raise RuntimeError(f"unsupported PLY (nx ny nz must be float): {path}")
            nrm_t = np.float64 if any(ncols[k].dtype == np.float64 for k in nxyz) else np.float32
            normals = np.stack([ncols[k].astype(nrm_t) for k in nxyz], axis=1) if n else np.zeros((0, 3), dtype=nrm_t)
    if rgb[0] not in cols:
        return (positions, None, normals) if with_normals else (positions, None)
    kinds = {cols[k].dtype.kind for k in rgb}
    if kinds == {"f"}:
        col_t = np.float64 if any(cols[k].dtype == np.float64 for k in rgb) else np.float32
    elif all(cols[k].dtype == np.uint8 for k in rgb):
        col_t = np.uint8
    else:
        raise RuntimeError(f"unsupported PLY (red green blue must be uchar or float): {path}")
    colors = np.stack([cols[k].astype(col_t) for k in rgb], axis=1) if n else np.zeros((0, 3), dtype=col_t)
    return (positions, colors, normals) if with_normals else (positions, colors)


def write_ply(path, positions: np.ndarray, colors: np.ndarray = None, normals: np.ndarray = None) -> None:
    """Binary little-endian PLY: ``x y z`` float and, with ``colors`` (uint8 [N,3]), ``red green blue`` uchar -- the
    layout the reference stores on purpose (:388) and its dataparser reads back.  ``normals`` ([N,3], stored as float):
    ``nx ny nz`` right after ``x y z``, where Poisson tools look for them; without them the file is what it always was."""
    positions = np.asarray(positions)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {positions.shape[0]}",
              "property float x", "property float y", "property float z"]
    if normals is not None:
        normals = np.asarray(normals)
        assert normals.shape == (positions.shape[0], 3)
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        colors = np.asarray(colors)
        assert colors.dtype == np.uint8 and colors.shape == (positions.shape[0], 3)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.empty(positions.shape[0], dtype=np.dtype(fields))
    for j, k in enumerate("xyz"):
        rec[k] = positions[:, j]
    if normals is not None:
        for j, k in enumerate(("nx", "ny", "nz")):
            rec[k] = normals[:, j]
    if colors is not None:
        for j, k in enumerate(("red", "green", "blue")):
            rec[k] = colors[:, j]
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\nend_header\n").encode("ascii"))
        f.write(rec.tobytes())


# ---- the command line (create_init_pointcloud.py:393-511) ---------------------------------------------------------------
def update_transforms_ply_path(dataset_path, output_name: str) -> None:
    transforms_path = Path(dataset_path) / "transforms.json"
    with open(transforms_path, encoding="utf-8") as f:
        contents = json.load(f)
    contents["ply_file_path"] = output_name
    with open(transforms_path, "w", encoding="utf-8") as f:
        json.dump(contents, f, indent=4)
    print(f"Updated {transforms_path} with ply_file_path={output_name}")


def resolve_dataset_path(data) -> Path:
    """A dataset directory, or the path of its transforms.json."""
    path = Path(data).expanduser().resolve()
    if path.is_file() and path.name == "transforms.json":
        return path.parent
    if path.is_dir():
        return path
    raise ValueError(f"Expected a dataset directory or transforms.json, got: {data}")


def _optional_voxel(text: str):
    """``--frame-voxel-size``: a size in metres; ``none`` or 0 turns the per-frame down-sampling off."""
    if text.strip().lower() == "none":
        return None
    value = float(text)
    return value if value > 0 else None


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m qed_splatter_amd.init_pointcloud",
                                description="Build an initialisation point cloud from a dataset's depth frames (step "
                                            "1), or with --colorize colour an existing one from its RGB-D frames "
                                            "(step 2): qed-init-pc on the GPU.")
    p.add_argument("--data", type=Path, required=True, help="dataset directory, or path to transforms.json")
    p.add_argument("--colorize", action="store_true", help="colourise an existing point cloud instead of building one")
    p.add_argument("--input-name", default="sparse_pc.ply", help="--colorize: input PLY inside the dataset directory")
    p.add_argument("--output-name", default="sparse_pc.ply", help="output PLY written into the dataset directory")
    p.add_argument("--depth-unit-scale-factor", type=float, default=0.001, help="raw depth -> metres (0.001: millimetres)")
    p.add_argument("--depth-max", type=float, default=100.0, help="largest depth (metres) that is used")
    p.add_argument("--voxel-size", type=float, default=0.05, help="step 1: voxel size of the final down-sampling, metres")
    p.add_argument("--merge-voxel-size", type=float, default=0.03,
                   help="step 1: voxel size for merges that exceed --max-points")
    p.add_argument("--frame-voxel-size", type=_optional_voxel, default=0.05,
                   help="step 1: voxel size of the per-frame down-sampling ('none' or 0: off)")
    p.add_argument("--max-points", type=int, default=2_000_000, help="step 1: a merge above this many points is down-sampled")
    p.add_argument("--stride", type=int, default=4, help="step 1: use every stride-th pixel of a depth map")
    p.add_argument("--depth-tolerance", type=float, default=0.05, help="--colorize: absolute depth consistency tolerance, metres")
    p.add_argument("--depth-tolerance-rel", type=float, default=0.02, help="--colorize: relative tolerance (fraction of z)")
    p.add_argument("--batch-frames", type=int, default=8, help="--colorize: frames per kernel launch")
    p.add_argument("--update-transforms", dest="update_transforms", action="store_true", default=True,
                   help="set transforms.json ply_file_path to the output PLY (default)")
    p.add_argument("--no-update-transforms", dest="update_transforms", action="store_false")
    return p


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    dataset_path = resolve_dataset_path(args.data)
    output_path = dataset_path / args.output_name
    if not args.colorize:
        positions = create_pointcloud_from_transforms(
            dataset_path, depth_unit_scale_factor=args.depth_unit_scale_factor, voxel_size=args.voxel_size,
            merge_voxel_size=args.merge_voxel_size, frame_voxel_size=args.frame_voxel_size, max_points=args.max_points,
            depth_max=args.depth_max, stride=args.stride)
        print(f"Writing {positions.shape[0]} points to {output_path}")
        write_ply(output_path, positions)
        if args.update_transforms:
            update_transforms_ply_path(dataset_path, args.output_name)
        return
    input_path = dataset_path / args.input_name
    if not input_path.exists():
        raise FileNotFoundError(f"Input point cloud not found: {input_path}. Back-project depth first.")
    print(f"Loading {input_path} for colorization...")
    positions = read_ply_positions(input_path)
    colors = colorize_pointcloud(dataset_path, positions.astype(np.float32),
                                 depth_unit_scale_factor=args.depth_unit_scale_factor, depth_max=args.depth_max,
                                 depth_tolerance=args.depth_tolerance, depth_tolerance_rel=args.depth_tolerance_rel,
                                 batch_frames=args.batch_frames)
    print(f"Writing {positions.shape[0]} points with colors to {output_path}")
    write_ply(output_path, positions, colors)
    if args.update_transforms:
        update_transforms_ply_path(dataset_path, args.output_name)


if __name__ == "__main__":
    main()
