"""A trained model to image files -- what ``ns-render dataset | interpolate | camera-path`` and
``ns-eval --render-output-path`` give a user of the reference:

    python -m qed_splatter_amd.render dataset     --load CKPT --output DIR --data DIR [--split eval|train|all]
    python -m qed_splatter_amd.render interpolate --load CKPT --output DIR --data DIR [--split ...] [--steps-per-pair N]
    python -m qed_splatter_amd.render camera-path --load CKPT --output DIR --camera-path-file camera_path.json

``dataset`` and ``interpolate`` need the dataparser options of the training run (the poses go through the same
transform); ``camera-path`` poses are in the dataparser's frame already.  The last line of output is one JSON object.

Per frame: ``model.get_outputs(camera)`` in eval mode, ``present_frame`` (csrc/present.hip: the float planes become uint8
colour, uint16 depth, a colour-mapped depth and uint8 accumulation in one launch, the depth range of the colour map in
one more, nothing is read back), and ``FrameWriter.submit``: device-to-host copies into a ring of pinned buffers on a side
stream while the next frame renders, PNG encoding in a thread pool.

Files: ``rgb/00042.png``, ``depth/00042.png`` (16-bit, in the dataset's own unit: ``depth_unit_scale_factor`` metres of
the ORIGINAL scene per step, i.e. value = rendered depth / (dataparser_scale * depth_unit_scale_factor); 0 = no surface,
as the datasets store "no measurement"), ``depth_vis/00042.png`` (colour map over white), ``accumulation/00042.png``;
with ``--planes ... normal`` also ``normal/00042.png``, the rendered normal map (normals.py) in the usual colouring;
with ``--planes ... semantic --field FIELD.pt`` also ``semantic/00042.png`` (the palette colour of every pixel's class) and
``semantic_label/00042.png`` (the class byte, 255 where the accumulation is below 0.5), semantic.py.
The depth files are read back by datamanager._load_depth, init_pointcloud and PDMetrics like any dataset's.

Camera paths are float64 host arithmetic.  ``load_camera_path`` reads the viewer's ``camera_path.json``; its layout is
RESTATED FROM MEMORY of nerfstudio 1.1.x (as dataparser.py is), not checked against it: ``render_height``,
``render_width`` and ``camera_path``, a list whose entries hold ``camera_to_world`` (16 floats, row-major, OpenGL, in
the dataparser's frame), ``fov`` (vertical, degrees) and ``aspect`` (ignored in favour of the render size).

The "turbo" table below is data: matplotlib 3.10's ``colormaps["turbo"](arange(256), bytes=True)``.  Turbo is Google's
colour map (Anton Mikhailov, 2019; Apache-2.0), which matplotlib redistributes.  Nothing imports matplotlib at run time.
"""
from __future__ import annotations

import argparse
import copy
import io
import json
import math
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .model import GROUP_ORDER, PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig

PLANES = ("rgb", "depth16", "depthmap", "alpha")
# planes that are not part of the default: "normal" (the rendered normal map as 8-bit RGB, normals.py) turns
# config.output_normals on for the run, "depth_std" (the depth standard deviation along the ray through the depth colour map,
# depth_distortion.py) config.output_depth_spread
EXTRA_PLANES = ("normal",)
SPREAD_PLANES = ("depth_std",)
# "semantic" (with a field, semantic.py: --field FIELD.pt) writes two directories: semantic/ (the class colours) and
# semantic_label/ (the class byte); SEMANTIC_FILES are the names of the two in a frame's dict
SEMANTIC_PLANES = ("semantic",)
SEMANTIC_FILES = ("semantic", "semantic_label")
ALL_PLANES = PLANES + EXTRA_PLANES + SPREAD_PLANES + SEMANTIC_PLANES
PLANE_DIRS = {"rgb": "rgb", "depth16": "depth", "depthmap": "depth_vis", "alpha": "accumulation", "normal": "normal",
              "depth_std": "depth_std", "semantic": "semantic", "semantic_label": "semantic_label"}
MAX_WORKERS = 16

_TURBO_HEX = (
    "30123b31154232184a341b51351e5836215f37236538266c3929723a2c793b2f7f3c32853c358b3d37913e3a963f3d9c"
    "4040a14043a64145ab4148b0424bb5434eba4350be4353c24456c74458cb455bce455ed24560d64563d94666dd4668e0"
    "466be3466de64670e84673eb4675ed4678f0467af2467df4467ff64682f84584f94587fb4589fc448cfd438efd4291fe"
    "4193fe4096fe3f98fe3e9bfe3c9dfd3ba0fc39a2fc38a5fb36a8f934aaf833acf631aff52fb1f32db4f12bb6ef2ab9ed"
    "28bbeb26bde925c0e623c2e421c4e120c6df1ec9dc1dcbda1ccdd71bcfd41ad1d219d3cf18d5cc18d7ca17d9c717dac4"
    "17dcc217debf18e0bd18e1ba19e3b81ae4b61be5b41de7b11ee8af20e9ac22eba924eca627eda329eea02cef9d2ff09a"
    "32f19735f39438f4913bf48d3ff58a42f68746f7834af8804df97c51f97955fa7659fb725dfb6f61fc6c65fc6869fd65"
    "6dfd6271fd5f74fe5c78fe597cfe5680fe5384fe5087fe4d8bfe4b8efe4892fe4695fe4498fe429bfd409efd3ea1fc3d"
    "a4fc3ba6fb3aa9fb39acfa37aef937b1f836b3f835b6f735b9f534bbf434bef334c0f233c3f133c5ef33c8ee33caed33"
    "cdeb34cfea34d1e834d4e735d6e535d8e335dae236dde036dfde36e1dc37e3da37e5d838e7d738e8d538ead339ecd139"
    "edcf39efcd39f0cb3af2c83af3c63af4c43af6c23af7c039f8be39f9bc39f9ba38fab737fbb537fbb336fcb035fcae34"
    "fdab33fda932fda631fda330fea12ffe9e2efe9b2dfe982cfd952bfd9229fd8f28fd8c27fc8926fc8624fb8323fb8022"
    "fa7d20fa7a1ff9771ef8741cf7711bf76e1af66b18f56817f46516f36315f26014f15d13ef5a11ee5810ed550fec520e"
    "ea500de94d0de84b0ce6490be5460ae3440ae24209e04008de3e08dd3c07db3a07d93806d73606d63405d43205d23005"
    "d02f04ce2d04cb2b03c92903c72803c52602c32402c02302be2102bb1f01b91e01b61c01b41b01b11901ae1801ac1601"
    "a91501a61401a31201a011019d10019a0e01970d01940c01910b018e0a018b09018708018407018106027d05027a0402")


def colormap(name: str = "turbo") -> np.ndarray:
    """The [256,3] uint8 table of ``"turbo"`` (the constant above) or ``"gray"`` (k, k, k)."""
    if name == "turbo":
        return np.frombuffer(bytes.fromhex(_TURBO_HEX), dtype=np.uint8).reshape(256, 3).copy()
    if name == "gray":
        k = np.arange(256, dtype=np.uint8)
        return np.stack([k, k, k], axis=1)
    raise ValueError(f"colormap {name!r}: 'turbo' or 'gray' (or pass a [256,3] uint8 table)")


_LUTS: Dict[tuple, Tensor] = {}


def _device_lut(lut, device) -> Tensor:
    """``lut``: None ("turbo"), a name, or a [256,3] table -> contiguous uint8 tensor on ``device`` (names are cached)."""
    if lut is None:
        lut = "turbo"
    if isinstance(lut, str):
        key = (lut, str(device))
        if key not in _LUTS:
            _LUTS[key] = torch.from_numpy(colormap(lut)).to(device)
        return _LUTS[key]
    t = torch.as_tensor(lut)
    if tuple(t.shape) != (256, 3) or t.dtype != torch.uint8:
        raise ValueError("lut: a [256,3] uint8 table")
    return t.to(device).contiguous()


def _plane(t: Tensor, name: str, h: int, w: int, c: int) -> Tensor:
    if not (t.is_cuda and t.dtype == torch.float32 and t.numel() == h * w * c):
        raise ValueError(f"outputs[{name!r}]: a float32 GPU tensor of {h}x{w}x{c} values")
    return t if t.is_contiguous() else t.contiguous()


def present_frame(outputs, *, depth_unit: float, near: Optional[float] = None, far: Optional[float] = None, lut=None,
                  planes: Sequence[str] = PLANES) -> Dict[str, Tensor]:
    """The integer planes of one rendered frame, as device tensors, from ``get_outputs``' dict as it is (``rgb``
    [H,W,3], ``depth`` [H,W,1] or None, ``accumulation`` [H,W,1]): a thin wrapper over qed_present_range and
    qed_present_frame (include/qed_splat.h states every definition).

      "rgb"      uint8 [H,W,3]      "alpha"    uint8 [H,W]        (the accumulation)
      "depth16"  uint16 [H,W]: depth / ``depth_unit`` rounded half up, saturating at 65535, 0 where nothing was hit.
                 ``depth_unit`` = dataparser_scale * depth_unit_scale_factor: model units per stored step
      "depthmap" uint8 [H,W,3]: ``lut`` ("turbo", "gray" or a [256,3] uint8 table) over ``near`` .. ``far``, composited
                 over white by the accumulation.  Both None: the frame's own range of valid depths, found on the device
                 and never read back

      "normal"   uint8 [H,W,3] (not in the default): ``outputs["normal_vis"]``, the colouring of the rendered normal map that
                 get_outputs made with config.output_normals -- round(255 (.5 + .5 (n_x, -n_y, -n_z))) of the camera-frame
                 normal, a facing surface blue-violet, black where there is none

      "depth_std" uint8 [H,W,3] (not in the default): ``outputs["depth_std"]`` (config.output_depth_spread) through the same
                 ``lut`` and kernel as "depthmap", over the frame's own range of its positive values, over white by the
                 accumulation; a pixel with one contributor (0) or none is white

    An ``outputs["depth"]`` of None leaves both depth planes out of the result.  Launched on the current stream."""
    unknown = [p for p in planes if p not in ALL_PLANES]
    if unknown:
        raise ValueError(f"planes {unknown}: choose from {ALL_PLANES}")
    if (near is None) != (far is None):
        raise ValueError("near and far: give both or neither")
    rgb, depth, alpha = outputs["rgb"], outputs.get("depth"), outputs["accumulation"]
    h, w = int(rgb.shape[0]), int(rgb.shape[1])
    rgb = _plane(rgb, "rgb", h, w, 3)
    alpha = _plane(alpha, "accumulation", h, w, 1)
    dev = rgb.device
    want = [p for p in planes if p in PLANES and (depth is not None or p not in ("depth16", "depthmap"))]
    if depth is not None:
        depth = _plane(depth, "depth", h, w, 1)
    out: Dict[str, Tensor] = {}
    if "normal" in planes:
        vis = outputs.get("normal_vis")
        if vis is None:
            raise ValueError("planes: 'normal' needs outputs of a model with config.output_normals (outputs['normal_vis'])")
        out["normal"] = vis
    if "depth_std" in planes:
        std = outputs.get("depth_std")
        if std is None:
            raise ValueError("planes: 'depth_std' needs outputs of a model with config.output_depth_spread "
                             "(outputs['depth_std'])")
        std = _plane(std, "depth_std", h, w, 1)
        out["depth_std"] = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        lib, st = L.load(), L.current_stream()
        std_rng = torch.empty(2, dtype=torch.float32, device=dev)
        L.check(lib.qed_present_range(h, w, L.ptr(std), L.ptr(alpha), L.ptr(std_rng), st), "qed_present_range")
        L.check(lib.qed_present_frame(h, w, None, L.ptr(std), L.ptr(alpha), 1.0, L.ptr(std_rng), 0.0, 0.0,
                                      L.ptr(_device_lut(lut, dev)), None, None, L.ptr(out["depth_std"]), None, st),
                "qed_present_frame")
    if not want:
        return out
    shapes = {"rgb": ((h, w, 3), torch.uint8), "depth16": ((h, w), torch.uint16), "depthmap": ((h, w, 3), torch.uint8),
              "alpha": ((h, w), torch.uint8)}
    for p in want:
        out[p] = torch.empty(shapes[p][0], dtype=shapes[p][1], device=dev)
    lib, st = L.load(), L.current_stream()
    rng, table = None, None
    if "depthmap" in want:
        table = _device_lut(lut, dev)
        if near is None:
            rng = torch.empty(2, dtype=torch.float32, device=dev)
            L.check(lib.qed_present_range(h, w, L.ptr(depth), L.ptr(alpha), L.ptr(rng), st), "qed_present_range")
    inv_unit = float(np.float32(1.0 / float(depth_unit)))
    L.check(lib.qed_present_frame(h, w, L.ptr(rgb), L.ptr(depth), L.ptr(alpha), inv_unit, L.ptr(rng),
                                  float(near) if near is not None else 0.0, float(far) if far is not None else 0.0,
                                  L.ptr(table), L.ptr(out.get("rgb")), L.ptr(out.get("depth16")),
                                  L.ptr(out.get("depthmap")), L.ptr(out.get("alpha")), st), "qed_present_frame")
    return out


# ---- writing ----------------------------------------------------------------------------------------------------------
def encode_png(array: np.ndarray, compress_level: int = 1) -> bytes:
    """One plane as a PNG file's bytes: uint8 [H,W,3] (RGB), uint8 [H,W] (L) or uint16 [H,W] (PIL mode ``I;16``)."""
    from PIL import Image
    a = np.asarray(array)
    if (a.dtype == np.uint16 and a.ndim == 2) or (a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3))):
        im = Image.fromarray(np.ascontiguousarray(a))
    else:
        raise ValueError(f"encode_png: uint8 [H,W,3], uint8 [H,W] or uint16 [H,W], not {a.dtype} {a.shape}")
    buf = io.BytesIO()
    im.save(buf, format="PNG", compress_level=int(compress_level))
    return buf.getvalue()


class _Slot:
    def __init__(self):
        self.host: Dict[str, Tensor] = {}       # plane -> pinned tensor
        self.event = None
        self.jobs: list = []                    # futures of the writes that read this slot


class FrameWriter:
    """Frames to ``out_dir/<plane directory>/<index:05d>.png`` without stalling the renderer.

    ``submit(index, frame)`` takes ``present_frame``'s dict: its device-to-host copies go to slot ``k % n_slots`` of a ring
    of pinned buffers on a side stream (one event per slot), and one job per plane in a pool of ``n_workers`` threads (at
    most 16, whatever the machine has) waits for that event, encodes and writes.  A slot is reused only after both its
    copy event and its writes have completed: ``submit`` waits for the writes of the frame ``n_slots`` back, and those
    waited for the event.  ``write_arrays(index, arrays)`` is the encoding half on its own, from NumPy arrays (which must
    stay unchanged until ``close``).  ``close()`` drains everything and re-raises the first exception a worker met;
    ``frames`` and ``bytes_written`` count what reached the disk."""

    def __init__(self, out_dir, planes: Sequence[str] = PLANES, n_slots: int = 3, n_workers: int = 8,
                 png_compress_level: int = 1):
        unknown = [p for p in planes if p not in ALL_PLANES]
        if unknown:
            raise ValueError(f"planes {unknown}: choose from {ALL_PLANES}")
        if n_slots < 1 or n_workers < 1:
            raise ValueError("n_slots and n_workers must be at least 1")
        self.out_dir = Path(out_dir)
        self.planes = tuple(planes)
        if "semantic" in self.planes:           # (one plane, two files per frame)
            self.planes += ("semantic_label",)
        self.compress_level = int(png_compress_level)
        for p in self.planes:
            (self.out_dir / PLANE_DIRS[p]).mkdir(parents=True, exist_ok=True)
        self._pool = ThreadPoolExecutor(max_workers=min(int(n_workers), MAX_WORKERS), thread_name_prefix="qed-png")
        self._slots = [_Slot() for _ in range(int(n_slots))]
        self._submitted = 0
        self._loose: list = []                  # futures of write_arrays
        self._error: Optional[BaseException] = None
        self._lock = threading.Lock()
        self._stream = None
        self.frames = 0
        self.bytes_written = 0
        self.encode_seconds = 0.0               # summed over the workers

    def path(self, plane: str, index: int) -> Path:
        return self.out_dir / PLANE_DIRS[plane] / f"{int(index):05d}.png"

    # -- the encoding half (no GPU)
    def _write(self, plane: str, index: int, array, event=None) -> None:
        if event is not None:
            event.synchronize()
        t0 = time.perf_counter()
        data = encode_png(array() if callable(array) else array, self.compress_level)
        with open(self.path(plane, index), "wb") as f:
            f.write(data)
        with self._lock:
            self.bytes_written += len(data)
            self.encode_seconds += time.perf_counter() - t0

    def _collect(self, futures) -> None:
        for f in futures:
            try:
                f.result()
            except BaseException as e:          # noqa: BLE001 (kept, and raised by close())
                if self._error is None:
                    self._error = e

    def write_arrays(self, index: int, arrays: Dict[str, np.ndarray]) -> None:
        """Encode and write the planes of one frame from host arrays, in the pool."""
        for p in self.planes:
            if p in arrays:
                self._loose.append(self._pool.submit(self._write, p, index, arrays[p]))
        self.frames += 1

    # -- the device half
    def submit(self, index: int, frame: Dict[str, Tensor]) -> None:
        slot = self._slots[self._submitted % len(self._slots)]
        self._submitted += 1
        self._collect(slot.jobs)                # the writes that read this slot (they waited for its copy event)
        slot.jobs = []
        todo = [p for p in self.planes if p in frame]
        if not todo:
            return
        dev = frame[todo[0]].device
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=dev)
        if slot.event is None:
            slot.event = torch.cuda.Event()
        side = self._stream
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for p in todo:
                t = frame[p]
                h = slot.host.get(p)
                if h is None or h.shape != t.shape or h.dtype != t.dtype:
                    h = slot.host[p] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                h.copy_(t, non_blocking=True)
                t.record_stream(side)           # (allocated on the render stream, read on this one)
            slot.event.record(side)
        for p in todo:
            slot.jobs.append(self._pool.submit(self._write, p, index, slot.host[p].numpy, slot.event))
        self.frames += 1

    def drain(self) -> None:
        for slot in self._slots:
            self._collect(slot.jobs)
            slot.jobs = []
        self._collect(self._loose)
        self._loose = []

    def close(self) -> None:
        self.drain()
        self._pool.shutdown(wait=True)
        if self._error is not None:
            err, self._error = self._error, None
            raise err

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                   # (the body's exception wins)
            self.drain()
            self._pool.shutdown(wait=True)
        return False


# ---- camera paths (float64, on the host) ----------------------------------------------------------------------------------
def _camera(c2w: np.ndarray, fx, fy, cx, cy, width, height, metadata=None) -> PinholeCameras:
    cam = PinholeCameras(torch.from_numpy(np.ascontiguousarray(c2w[None, :3, :4], dtype=np.float64)), float(fx), float(fy),
                         float(cx), float(cy), int(width), int(height), metadata=metadata)
    return cam


def _camera_values(cam: PinholeCameras):
    """(c2w [3,4] float64, fx, fy, cx, cy, width, height) of a one-camera object."""
    if cam.camera_to_worlds.shape[0] != 1:
        raise ValueError("camera paths are made of one-camera objects")
    c2w = cam.camera_to_worlds[0, :3, :4].detach().double().cpu().numpy()
    return (c2w, float(cam.fx.reshape(-1)[0]), float(cam.fy.reshape(-1)[0]), float(cam.cx.reshape(-1)[0]),
            float(cam.cy.reshape(-1)[0]), int(cam.width.reshape(-1)[0]), int(cam.height.reshape(-1)[0]))


def dataset_path(datamanager, split: str = "eval") -> List[PinholeCameras]:
    """The datamanager's cameras of ``split`` ("eval", "train", or "all": both, in the dataset's frame order), one
    one-camera object each, copies as the datamanager hands them out."""
    dm = datamanager
    if split == "eval":
        cams = list(dm._eval_cameras)
    elif split == "train":
        cams = list(dm._train_cameras)
    elif split == "all":
        both = list(zip(dm.i_train, dm._train_cameras)) + list(zip(dm.i_eval, dm._eval_cameras))
        cams = [c for _, c in sorted(both, key=lambda kc: kc[0])]
    else:
        raise ValueError(f"split {split!r}: 'eval', 'train' or 'all'")
    return [dm._hand_out(c) for c in cams]


def rotation_to_quaternion(R: np.ndarray) -> np.ndarray:
    """wxyz of a rotation matrix (Shepperd's method: the largest of the four candidates is the pivot)."""
    R = np.asarray(R, np.float64)
    t = np.trace(R)
    cand = np.array([t, R[0, 0], R[1, 1], R[2, 2]])
    i = int(np.argmax(cand))
    if i == 0:
        q = np.array([1.0 + t, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif i == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + 2 * R[0, 0] - t, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif i == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + 2 * R[1, 1] - t, R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + 2 * R[2, 2] - t])
    return q / np.linalg.norm(q)


def quaternion_to_rotation(q: np.ndarray) -> np.ndarray:
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def slerp(q0: np.ndarray, q1: np.ndarray, t: float) -> np.ndarray:
    """Spherical interpolation of unit quaternions the short way (q and -q are one rotation: q1 is negated when the two
    are more than a quarter turn of S^3 apart); normalised.  Nearly parallel: the normalised linear blend."""
    q0, q1 = np.asarray(q0, np.float64), np.asarray(q1, np.float64)
    d = float(np.dot(q0, q1))
    if d < 0.0:
        q1, d = -q1, -d
    if d > 1.0 - 1e-10:
        q = (1.0 - t) * q0 + t * q1
    else:
        th = math.acos(min(d, 1.0))
        q = (math.sin((1.0 - t) * th) * q0 + math.sin(t * th) * q1) / math.sin(th)
    return q / np.linalg.norm(q)


def order_nearest(c2ws: Sequence[np.ndarray]) -> List[int]:
    """Greedy order: start at the first pose, always go on to the nearest camera position not visited yet."""
    left = list(range(1, len(c2ws)))
    order = [0] if len(c2ws) else []
    while left:
        here = c2ws[order[-1]][:, 3]
        j = min(left, key=lambda k: float(np.linalg.norm(c2ws[k][:, 3] - here)))
        left.remove(j)
        order.append(j)
    return order


def interpolate_path(cameras: Sequence[PinholeCameras], steps_per_pair: int, order_poses: bool = False) -> List[PinholeCameras]:
    """``steps_per_pair`` frames per consecutive pair of key cameras, at t = j / steps_per_pair for j = 0 ..
    steps_per_pair - 1, and the last key camera once at the end: (n - 1) * steps_per_pair + 1 frames, every key camera
    reproduced exactly and once.  Rotations are slerped as quaternions the short way; translations, fx, fy, cx, cy are
    interpolated linearly; a pair's frames take the size of its first camera.  ``order_poses``: visit the key cameras
    in ``order_nearest`` order.  Poses come back as float64 CPU tensors (``render_frames`` moves them)."""
    if steps_per_pair < 1:
        raise ValueError("steps_per_pair must be at least 1")
    keys = [_camera_values(c) for c in cameras]
    if order_poses:
        keys = [keys[i] for i in order_nearest([k[0] for k in keys])]
    if not keys:
        return []
    out: List[PinholeCameras] = []
    for a, b in zip(keys[:-1], keys[1:]):
        qa, qb = rotation_to_quaternion(a[0][:, :3]), rotation_to_quaternion(b[0][:, :3])
        for j in range(steps_per_pair):
            if j == 0:
                out.append(_camera(*a))
                continue
            t = j / steps_per_pair
            c2w = np.empty((3, 4))
            c2w[:, :3] = quaternion_to_rotation(slerp(qa, qb, t))
            c2w[:, 3] = (1.0 - t) * a[0][:, 3] + t * b[0][:, 3]
            out.append(_camera(c2w, *((1.0 - t) * a[i] + t * b[i] for i in range(1, 5)), a[5], a[6]))
    out.append(_camera(*keys[-1]))
    return out


def load_camera_path(json_path) -> List[PinholeCameras]:
    """The viewer's ``camera_path.json`` (layout restated from memory of nerfstudio 1.1.x, see the module docstring): one
    camera of ``render_width`` x ``render_height`` per entry of ``camera_path``; ``camera_to_world`` is 16 row-major floats
    already in the dataparser's frame; ``fov`` is vertical and in degrees, fx = fy = H / (2 tan(fov / 2)), the principal
    point is the centre; ``aspect`` is ignored in favour of the render size."""
    meta = json.loads(Path(json_path).read_text())
    w, h = int(meta["render_width"]), int(meta["render_height"])
    out = []
    for i, entry in enumerate(meta["camera_path"]):
        m = np.asarray(entry["camera_to_world"], dtype=np.float64).reshape(-1)
        if m.size != 16:
            raise ValueError(f"{json_path}: camera_path[{i}].camera_to_world must hold 16 values")
        fov = float(entry.get("fov", meta.get("default_fov", 50.0)))
        if not 0.0 < fov < 180.0:
            raise ValueError(f"{json_path}: camera_path[{i}].fov = {fov}")
        f = h / (2.0 * math.tan(math.radians(fov) / 2.0))
        out.append(_camera(m.reshape(4, 4), f, f, w / 2.0, h / 2.0, w, h))
    return out


class OrientedBox:
    """A crop box for ``model.crop_box``: ``center`` [3], ``rpy`` [3] (radians; R = Rz(yaw) Ry(pitch) Rx(roll)), ``scale``
    [3] (the box's full extent along its own axes), in the model's frame.  ``within(points)``: bool [N,1], True where
    R^T (p - center) lies strictly inside (-scale / 2, scale / 2) on every axis; evaluated in float64 on the points'
    device."""

    def __init__(self, center, rpy, scale):
        self.center = np.asarray(center, np.float64).reshape(3)
        self.rpy = np.asarray(rpy, np.float64).reshape(3)
        self.scale = np.asarray(scale, np.float64).reshape(3)
        r, p, y = self.rpy
        rx = np.array([[1, 0, 0], [0, math.cos(r), -math.sin(r)], [0, math.sin(r), math.cos(r)]])
        ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
        rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
        self.R = rz @ ry @ rx

    def within(self, points: Tensor) -> Tensor:
        p = points.detach().double()
        R = torch.from_numpy(self.R).to(p.device)
        local = (p - torch.from_numpy(self.center).to(p.device)) @ R          # rows: R^T (p - c)
        half = torch.from_numpy(self.scale / 2.0).to(p.device)
        return ((local > -half) & (local < half)).all(dim=-1, keepdim=True)


# ---- rendering --------------------------------------------------------------------------------------------------------
def _on_device(cam: PinholeCameras, device) -> PinholeCameras:
    """The camera as the model wants it: a float32 pose and intrinsics on ``device`` (a copy unless it is there already)."""
    c2w = cam.camera_to_worlds
    if c2w.device == device and c2w.dtype == torch.float32 and cam.fx.device == device:
        return cam
    out = copy.copy(cam)
    out.camera_to_worlds = c2w.to(device, torch.float32).contiguous()
    for k in ("fx", "fy", "cx", "cy"):
        setattr(out, k, getattr(cam, k).to(device, torch.float32))
    out._intr = None
    return out


def render_frames(model: QEDSplatterModel, cameras: Sequence[PinholeCameras], writer: FrameWriter, *, depth_unit: float,
                  near: Optional[float] = None, far: Optional[float] = None, lut=None, start_index: int = 0,
                  timings: Optional[dict] = None, field=None) -> int:
    """Every camera through ``get_outputs`` (eval mode, no gradients), ``present_frame`` and ``writer.submit``, numbered
    from ``start_index``; the model's training mode is restored afterwards.  Returns the number of frames.  The writer is
    left open (``close()`` it to wait for the files).  ``timings``: a dict that receives lists of (start, end) event pairs
    under "render" and "finish" for measurements.  ``field`` (a semantic.SemanticField of the model's Gaussians): what the
    "semantic" plane is rendered from; the plane without it is refused, and so is the plane under a crop box."""
    semantic = "semantic" in writer.planes
    if semantic:
        if field is None:
            raise ValueError("planes: 'semantic' needs a field (render.py --field FIELD.pt; semantic.py fits one)")
        if model.crop_box is not None:
            raise NotImplementedError("planes: 'semantic' under a crop box: the field's rows are the whole model's")
        field.check_model(model)
        from .semantic import composite_features, present_labels
    frame_planes = tuple(p for p in writer.planes if p not in SEMANTIC_FILES)
    was_training = model.training
    model.eval()
    had_normals = bool(getattr(model.config, "output_normals", False))
    had_spread = bool(getattr(model.config, "output_depth_spread", False))
    if "normal" in writer.planes:
        model.config.output_normals = True      # (asking for the plane turns the normal pass on for this run)
    if "depth_std" in writer.planes:
        model.config.output_depth_spread = True
    if semantic:
        model.__dict__["_score_records"] = True  # (the records and lists of every render stay for the field's pass)
    n = 0
    try:
        with torch.no_grad():
            for cam in cameras:
                cam = _on_device(cam, model.device)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timings is not None else None
                if ev:
                    ev[0].record()
                outputs = model.get_outputs(cam)
                if ev:
                    ev[1].record()
                frame = present_frame(outputs, depth_unit=depth_unit, near=near, far=far, lut=lut, planes=frame_planes)
                if semantic:
                    info = model.info
                    logits = composite_features(info, 1, model.num_points, field.logits)[0]
                    info.pop("_splats", None)
                    info.pop("_isect_offsets_full", None)
                    frame["semantic_label"], frame["semantic"] = present_labels(logits, outputs["accumulation"], field.palette)
                if ev:
                    ev[2].record()
                    timings.setdefault("render", []).append((ev[0], ev[1]))
                    timings.setdefault("finish", []).append((ev[1], ev[2]))
                writer.submit(start_index + n, frame)
                n += 1
    finally:
        model.__dict__.pop("_score_records", None)
        model.train(was_training)
        model.config.output_normals = had_normals
        model.config.output_depth_spread = had_spread
    return n


def load_model(ckpt_path, device, background_color: str = "random"):
    """(model, checkpoint dict) of a ``Trainer.save`` file: the six tensors and ``sh_degree``, as ``Trainer.resume``
    rebuilds them; ``model.step`` is the checkpoint's, so the SH bands the training had reached are used."""
    ckpt = torch.load(ckpt_path, map_location=device, weights_only=False)
    cfg = QEDSplatterModelConfig(sh_degree=int(ckpt.get("sh_degree", 3)), background_color=background_color)
    model = QEDSplatterModel(cfg, **{n: ckpt["params"][n] for n in GROUP_ORDER})
    model.step = int(ckpt.get("step", 0))
    return model, ckpt


def render_to_directory(model, cameras, out_dir, *, depth_unit, planes=PLANES, colormap_name="turbo", near=None, far=None,
                        n_workers: int = 8, n_slots: Optional[int] = None, png_compress_level: int = 1, field=None) -> dict:
    """``render_frames`` into a fresh ``FrameWriter`` on ``out_dir``, closed; -> {"frames", "frames_per_s",
    "bytes_written", "output"}.  ``n_slots`` None: half as many slots as workers, at least 3 -- a slot is held until the
    slowest of its frame's files is written, and three slots keep no more than eight threads busy (profiles/render.txt)."""
    if n_slots is None:
        n_slots = max(3, min(int(n_workers), MAX_WORKERS) // 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with FrameWriter(out_dir, planes, n_slots=n_slots, n_workers=n_workers, png_compress_level=png_compress_level) as writer:
        n = render_frames(model, cameras, writer, depth_unit=depth_unit, near=near, far=far, lut=colormap_name, field=field)
    elapsed = time.perf_counter() - t0
    return {"frames": n, "frames_per_s": n / elapsed if elapsed > 0 and n else 0.0,
            "bytes_written": writer.bytes_written, "output": str(out_dir)}


def add_dataparser_arguments(ap) -> None:
    """The dataparser options of train.py, with its defaults: they must match the training run's."""
    ap.add_argument("--orientation-method", choices=("up", "none"), default="up")
    ap.add_argument("--center-method", choices=("poses", "none"), default="poses")
    ap.add_argument("--auto-scale-poses", choices=("True", "False"), default="True")
    ap.add_argument("--depth-unit-scale-factor", type=float, default=0.001,
                    help="metres (of the original scene) per step of the 16-bit depth files, read and written")
    ap.add_argument("--train-split-fraction", type=float, default=0.9)
    ap.add_argument("--scale-factor", type=float, default=1.0, help="the dataparser's scale_factor")
    ap.add_argument("--undistort", action="store_true")
    ap.add_argument("--cache-device", default=None, help="'cpu' keeps the image cache in pinned host memory")


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(prog="python -m qed_splatter_amd.render", description=__doc__.split("\n\n")[0])
    ap.add_argument("command", choices=("dataset", "interpolate", "camera-path"))
    ap.add_argument("--load", required=True, metavar="CKPT", help="a checkpoint written by train.py --save")
    ap.add_argument("--output", required=True, metavar="DIR")
    ap.add_argument("--data", metavar="DIR", default=None, help="dataset directory (dataset, interpolate)")
    ap.add_argument("--split", choices=("eval", "train", "all"), default="eval")
    ap.add_argument("--steps-per-pair", type=int, default=10)
    ap.add_argument("--order-poses", action="store_true", help="interpolate: visit the cameras nearest-first")
    ap.add_argument("--camera-path-file", metavar="JSON", default=None)
    ap.add_argument("--planes", nargs="+", choices=ALL_PLANES, default=list(PLANES),
                    help="'normal' (not in the default) adds normal/: the rendered normal map as 8-bit RGB; 'semantic' (with "
                         "--field) adds semantic/ and semantic_label/")
    ap.add_argument("--field", metavar="FIELD.pt", default=None, help="a semantic field (semantic.py fit) for the 'semantic' plane")
    ap.add_argument("--colormap", choices=("turbo", "gray"), default="turbo")
    ap.add_argument("--near", type=float, default=None)
    ap.add_argument("--far", type=float, default=None, help="depth map range in model units (default: every frame's own)")
    ap.add_argument("--crop", type=float, nargs=9, default=None, metavar="V",
                    help="cx cy cz  roll pitch yaw  sx sy sz: an oriented box in the model's frame; Gaussians outside are left out")
    ap.add_argument("--downscale", type=float, default=1.0, help="render at 1 / D of the cameras' size")
    ap.add_argument("--background-color", choices=("random", "black", "white"), default="random",
                    help="'random' renders over the reference's fixed evaluation colour")
    ap.add_argument("--workers", type=int, default=8, help=f"PNG encoding threads (at most {MAX_WORKERS})")
    ap.add_argument("--slots", type=int, default=None, help="pinned frames in flight (default: workers / 2, at least 3)")
    add_dataparser_arguments(ap)
    a = ap.parse_args(argv)
    if (a.near is None) != (a.far is None):
        ap.error("--near and --far: give both or neither")
    if a.command in ("dataset", "interpolate") and not a.data:
        ap.error(f"{a.command} needs --data (and the dataparser options of the training run)")
    if a.command == "camera-path" and not a.camera_path_file:
        ap.error("camera-path needs --camera-path-file")
    if "semantic" in a.planes and not a.field:
        ap.error("--planes semantic needs --field FIELD.pt")
    if not torch.cuda.is_available():
        raise SystemExit("qed_splatter_amd.render needs a GPU")
    L.load()
    device = torch.device("cuda:0")
    model, ckpt = load_model(a.load, device, a.background_color)
    if a.crop is not None:
        model.crop_box = OrientedBox(a.crop[0:3], a.crop[3:6], a.crop[6:9])
    if a.command == "camera-path":
        cameras = load_camera_path(a.camera_path_file)
    else:
        from .datamanager import FullImageDatamanager
        from .dataparser import DataparserConfig
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
        if a.command == "interpolate":
            cameras = interpolate_path(cameras, a.steps_per_pair, a.order_poses)
    if a.downscale != 1.0:
        for cam in cameras:
            cam.rescale_output_resolution(1.0 / a.downscale)
    depth_unit = float(ckpt.get("dataparser_scale", 1.0)) * a.depth_unit_scale_factor
    field = None
    if a.field:
        from .semantic import SemanticField
        field = SemanticField.load(a.field, device)
    result = render_to_directory(model, cameras, a.output, depth_unit=depth_unit, planes=tuple(a.planes),
                                 colormap_name=a.colormap, near=a.near, far=a.far, n_workers=a.workers, n_slots=a.slots,
                                 field=field)
    result["command"] = a.command
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
