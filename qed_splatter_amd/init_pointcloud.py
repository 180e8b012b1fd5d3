"""The initial point cloud: the reference's ``qed-init-pc`` tool on the GPU.

Step 1, geometry (create_init_pointcloud.py:148-196).  File handling (PLY caches, the pairwise on-disk merge of
:100-145) stays with the reference tool; this module replaces the per-frame Open3D calls: ``backproject_depth`` for
``create_from_depth_image`` and ``voxel_down_sample`` for the method of the same name.

Step 2, colour (``--colorize``, :264-390), completely: ``PointColorizer`` (csrc/colorize.hip), ``colorize_pointcloud``
(the reference's frame loop and file rules), a NumPy PLY reader / writer in place of the two ``o3d.t.io`` calls, and
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


@torch.no_grad()
def voxel_down_sample(points: Tensor, voxel_size: float) -> Tensor:
    """One point per occupied voxel: the mean of its members (Open3D semantics).  Device-side torch ops
    (unique over voxel keys + index_add); offline tool, not a training hot path."""
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


def read_ply_positions(path) -> np.ndarray:
    """The ``x y z`` of a PLY's vertex element as [N,3] (float32, or float64 if the file stores doubles).  ASCII and
    binary little-endian; the vertex element must come first and have scalar properties only."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise RuntimeError(f"Failed to read point cloud: {path}")
        fmt, n, props, in_vertex, seen_vertex = None, 0, [], False, False
        while True:
            line = f.readline()
            if not line:
                raise RuntimeError(f"Failed to read point cloud (no end_header): {path}")
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
        names = [p[0] for p in props]
        if not seen_vertex or not all(k in names for k in "xyz"):
            raise RuntimeError(f"Failed to read point cloud (no x y z): {path}")
        if fmt == "binary_little_endian":
            dt = np.dtype([(k, "<" + t) for k, t in props])
            rec = np.frombuffer(f.read(n * dt.itemsize), dtype=dt, count=n)
            cols = [rec[k] for k in "xyz"]
        elif fmt == "ascii":
            rows = np.loadtxt(f, dtype=np.float64, max_rows=n, ndmin=2) if n else np.zeros((0, len(props)))
            cols = [rows[:, names.index(k)].astype(dict(props)[k]) for k in "xyz"]
        else:
            raise RuntimeError(f"unsupported PLY format {fmt!r}: {path}")
    out_t = np.float64 if any(c.dtype == np.float64 for c in cols) else np.float32
    return np.stack([c.astype(out_t) for c in cols], axis=1) if n else np.zeros((0, 3), dtype=out_t)


def write_ply(path, positions: np.ndarray, colors: np.ndarray = None) -> None:
    """Binary little-endian PLY: ``x y z`` float and, with ``colors`` (uint8 [N,3]), ``red green blue`` uchar -- the
    layout the reference stores on purpose (:388) and its dataparser reads back."""
    positions = np.asarray(positions)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {positions.shape[0]}",
              "property float x", "property float y", "property float z"]
    if colors is not None:
        colors = np.asarray(colors)
        assert colors.dtype == np.uint8 and colors.shape == (positions.shape[0], 3)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.empty(positions.shape[0], dtype=np.dtype(fields))
    for j, k in enumerate("xyz"):
        rec[k] = positions[:, j]
    if colors is not None:
        for j, k in enumerate(("red", "green", "blue")):
            rec[k] = colors[:, j]
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\nend_header\n").encode("ascii"))
        f.write(rec.tobytes())


# ---- the command line of the colourise branch (create_init_pointcloud.py:393-511) -------------------------------------
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


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m qed_splatter_amd.init_pointcloud",
                                description="Colourise an initialisation point cloud from a dataset's RGB-D frames "
                                            "(the --colorize step of qed-init-pc) on the GPU.")
    p.add_argument("--data", type=Path, required=True, help="dataset directory, or path to transforms.json")
    p.add_argument("--colorize", action="store_true", help="colourise an existing point cloud (the only step this tool has)")
    p.add_argument("--input-name", default="sparse_pc.ply", help="input PLY inside the dataset directory")
    p.add_argument("--output-name", default="sparse_pc.ply", help="output PLY written into the dataset directory")
    p.add_argument("--depth-unit-scale-factor", type=float, default=0.001, help="raw depth -> metres (0.001: millimetres)")
    p.add_argument("--depth-max", type=float, default=100.0, help="largest depth (metres) a colour check accepts")
    p.add_argument("--depth-tolerance", type=float, default=0.05, help="absolute depth consistency tolerance, metres")
    p.add_argument("--depth-tolerance-rel", type=float, default=0.02, help="relative tolerance (fraction of z)")
    p.add_argument("--batch-frames", type=int, default=8, help="frames per kernel launch")
    p.add_argument("--update-transforms", dest="update_transforms", action="store_true", default=True,
                   help="set transforms.json ply_file_path to the output PLY (default)")
    p.add_argument("--no-update-transforms", dest="update_transforms", action="store_false")
    return p


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    if not args.colorize:
        raise SystemExit("only --colorize is implemented here: back-project with backproject_depth / the reference "
                         "tool first, then colourise")
    dataset_path = resolve_dataset_path(args.data)
    input_path = dataset_path / args.input_name
    if not input_path.exists():
        raise FileNotFoundError(f"Input point cloud not found: {input_path}. Back-project depth first.")
    print(f"Loading {input_path} for colorization...")
    positions = read_ply_positions(input_path)
    colors = colorize_pointcloud(dataset_path, positions.astype(np.float32),
                                 depth_unit_scale_factor=args.depth_unit_scale_factor, depth_max=args.depth_max,
                                 depth_tolerance=args.depth_tolerance, depth_tolerance_rel=args.depth_tolerance_rel,
                                 batch_frames=args.batch_frames)
    output_path = dataset_path / args.output_name
    print(f"Writing {positions.shape[0]} points with colors to {output_path}")
    write_ply(output_path, positions, colors)
    if args.update_transforms:
        update_transforms_ply_path(dataset_path, args.output_name)


if __name__ == "__main__":
    main()
